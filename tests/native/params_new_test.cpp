// Native test of trh::Params::create (Params::new: hash_to_curve on the device, include/trh.hpp; compiled host, no Python in the process): writes the
// Params file of (curve, k) for each k given, so that tests/test_gpu_hashtocurve.py can compare it byte for byte with the file Python's Params.new
// writes and with tests/hash_to_curve_model.py.  Prints one JSON line.
//   usage: params_new_test <pallas|vesta> <out prefix> <k> [<k> ...]      writes <out prefix><k>.params
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/trh.hpp"

using namespace trh;

int main(int argc, char** argv) {
    if (argc < 4 || (std::strcmp(argv[1], "pallas") && std::strcmp(argv[1], "vesta"))) {
        std::fprintf(stderr, "usage: %s <pallas|vesta> <out prefix> <k> [<k> ...]\n", argv[0]);
        return 2;
    }
    const Curve c = std::strcmp(argv[1], "pallas") ? Curve::Vesta : Curve::Pallas;
    int failed = 0, files = 0;
    try {
        check(trh_init(0), "trh_init");
        for (int i = 3; i < argc; ++i) {
            const uint32_t k = (uint32_t)std::strtoul(argv[i], nullptr, 10);
            const Params p = Params::create(c, k);
            const std::vector<uint8_t> file = p.write();
            if (file.size() != 4 + 32 * (2 * p.n + 2)) { ++failed; continue; }
            const std::string path = std::string(argv[2]) + argv[i] + ".params";
            std::FILE* f = std::fopen(path.c_str(), "wb");
            if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size()) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); ++failed; }
            if (f) std::fclose(f);
            ++files;
        }
        trh_shutdown();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        ++failed;
    }
    std::printf("{\"test\": \"params_new\", \"files\": %d, \"checks_failed\": %d}\n", files, failed);
    return failed ? 1 : 0;
}
