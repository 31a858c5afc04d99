// Native test of trh::Rng over include/trh.hpp (compiled host, no Python in the process): 1000 elements per field filled on the device from a
// fixed seed and stream id, one host draw behind them, and a fill_rows into a zeroed batch of columns.  Prints one JSON line with an FNV-1a
// digest of each result, which tests/test_gpu_rng.py compares with the same digest of tests/chacha_model.py's elements.
#include <cstdio>
#include <vector>

#include "../../include/trh.hpp"

using namespace trh;

static uint64_t fnv(const std::vector<Limbs>& v) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (const Limbs& e : v) for (uint64_t w : e) { h ^= w; h *= 0x100000001b3ull; }
    return h;
}

int main() {
    int failed = 0;
    std::printf("{\"test\": \"rng_fill\"");
    try {
        check(trh_init(0), "trh_init");
        std::array<uint8_t, 32> seed;
        for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(0xa5 ^ (7 * i));
        const size_t n = 1000, rows = 3, row_len = 40, first = 34, count = 6;
        for (Field f : {Field::Fp, Field::Fq}) {
            const char* name = f == Field::Fp ? "fp" : "fq";
            Rng rng(seed, 0x0123456789abcdefull);
            rng.seek(77);
            DeviceBuffer d(n * 32);
            rng.fill(f, d.data(), n);
            std::vector<Limbs> got(n);
            check(trh_stream_synchronize(nullptr), "sync");
            d.download(got.data(), n * 32);
            const Limbs next = rng.next_scalar(f);                  // element 77 + 1000
            std::vector<Limbs> cols(rows * row_len, Limbs{0, 0, 0, 0});
            DeviceBuffer c(cols.size() * 32);
            c.upload(cols.data(), cols.size() * 32);
            rng.fill_rows(f, c.data(), rows, row_len, first, count);  // elements 77 + 1001 ..
            check(trh_stream_synchronize(nullptr), "sync");
            c.download(cols.data(), cols.size() * 32);
            if (rng.position() != 77 + n + 1 + rows * count) ++failed;
            std::printf(", \"%s_fill\": \"%016llx\", \"%s_next\": \"%016llx\", \"%s_rows\": \"%016llx\"", name, (unsigned long long)fnv(got), name,
                        (unsigned long long)fnv({next}), name, (unsigned long long)fnv(cols));
        }
        trh_shutdown();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        ++failed;
    }
    std::printf(", \"checks_failed\": %d}\n", failed);
    return failed ? 1 : 0;
}
