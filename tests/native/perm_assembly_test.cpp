// Native test of trh::PermutationAssembly over include/trh.hpp (compiled host, no Python in the process): reads a shape and a list of copies
// from the file tests/test_gpu_permkeygen.py wrote, records them -- half one by one, half as a batch, through a moved object -- and prints one
// JSON line with FNV-1a digests of the mapping and of the sigma columns (whole and a window), and what check_columns says of the sigma columns
// taken as witness values (every cell that does not map to itself differs from its image), and digests of build_vk's commitments and build_pk's
// polynomials and cosets.  The Python side compares them with its own.
//   file: <fp|fq> <k> <n_columns> <copies>  then <copies> lines  <left_column> <left_row> <right_column> <right_row>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/trh.hpp"

using namespace trh;

template <class T>
static uint64_t fnv(const std::vector<T>& v) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (const T& w : v) { h ^= (uint64_t)w; h *= 0x100000001b3ull; }
    return h;
}

int main(int argc, char** argv) {
    int failed = 0;
    std::printf("{\"test\": \"perm_assembly\"");
    try {
        require(argc == 2, "usage: perm_assembly_test <file>");
        FILE* in = std::fopen(argv[1], "r");
        require(in != nullptr, "the input file opens");
        char fname[8] = "";
        unsigned k = 0, n_columns = 0, copies = 0;
        require(std::fscanf(in, "%7s %u %u %u", fname, &k, &n_columns, &copies) == 4, "header");
        const Field f = std::strcmp(fname, "fp") == 0 ? Field::Fp : Field::Fq;
        std::vector<std::array<uint32_t, 4>> quads(copies);
        for (auto& q : quads) require(std::fscanf(in, "%u %u %u %u", &q[0], &q[1], &q[2], &q[3]) == 4, "a copy");
        std::fclose(in);

        PermutationAssembly first(f, k, n_columns);
        const size_t half = quads.size() / 2;
        for (size_t i = 0; i < half; ++i) first.copy(quads[i][0], quads[i][1], quads[i][2], quads[i][3]);
        PermutationAssembly a(std::move(first));
        if (first.handle() != nullptr) ++failed;
        a.copy_many(std::vector<std::array<uint32_t, 4>>(quads.begin() + half, quads.end()));
        const std::vector<uint32_t> mapping = a.mapping();
        std::printf(", \"mapping\": \"%016llx\"", (unsigned long long)fnv(mapping));
        bool refused = false;  // a cell outside the columns throws and changes nothing
        try { a.copy(n_columns, 0, 0, 0); } catch (const Error&) { refused = true; }
        if (!refused || a.mapping() != mapping) ++failed;

        check(trh_init(0), "trh_init");
        const size_t n = a.n;
        const DeviceBuffer sigma = a.sigma_columns();
        std::vector<uint64_t> words(n_columns * n * 4);
        check(trh_stream_synchronize(nullptr), "sync");
        sigma.download(words.data(), words.size() * 8);
        std::printf(", \"sigma\": \"%016llx\"", (unsigned long long)fnv(words));
        if (n_columns >= 2) {
            const DeviceBuffer window = a.sigma_columns(n_columns - 1, 1);
            std::vector<uint64_t> w(n * 4);
            check(trh_stream_synchronize(nullptr), "sync");
            window.download(w.data(), w.size() * 8);
            if (std::memcmp(w.data(), words.data() + (size_t)(n_columns - 1) * n * 4, w.size() * 8) != 0) ++failed;
        }
        // build_vk over synthetic resident generators (the Python side makes the same set), build_pk over a j = 4 domain
        const Curve cv = f == Field::Fq ? Curve::Pallas : Curve::Vesta;
        const Params params(cv, k, 11, 3);
        const std::vector<Point> vk = a.build_vk(params);
        std::vector<uint64_t> vk_words(vk.size() * 12);
        std::memcpy(vk_words.data(), vk.data(), vk_words.size() * 8);
        std::printf(", \"vk\": \"%016llx\"", (unsigned long long)fnv(vk_words));
        const EvaluationDomain dom(f, 4, k);
        const PermutationAssembly::ProvingKey pk = a.build_pk(dom);
        check(trh_stream_synchronize(nullptr), "sync");
        std::vector<uint64_t> perm_words(words.size()), poly_words(words.size()), coset_words(n_columns * dom.extended_len() * 4);
        pk.permutations.download(perm_words.data(), perm_words.size() * 8);
        pk.polys.download(poly_words.data(), poly_words.size() * 8);
        pk.cosets.download(coset_words.data(), coset_words.size() * 8);
        if (perm_words != words) ++failed;
        std::printf(", \"polys\": \"%016llx\", \"cosets\": \"%016llx\"", (unsigned long long)fnv(poly_words), (unsigned long long)fnv(coset_words));
        std::vector<const void*> columns;
        for (unsigned j = 0; j < n_columns; ++j) columns.push_back(sigma.at((size_t)j * n * 32));
        const PermutationAssembly::Check c = a.check_columns(columns);
        std::printf(", \"n_bad\": %llu, \"first_bad_cell\": %llu", (unsigned long long)c.n_bad, (unsigned long long)c.first_bad_cell);
        trh_shutdown();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        ++failed;
    }
    std::printf(", \"checks_failed\": %d}\n", failed);
    return failed ? 1 : 0;
}
