// csrc/permkeygen.h on the host, alone: reads assemblies and their copies from a file, applies them with PermAssembly::copy and writes the
// return codes and the mapping back.  Built with address + undefined sanitizers; every property is asserted by tests/test_permkeygen_host.py.
//   in:  <cases>  then per case  <n_columns> <k> <copies>  and <copies> lines  <left_column> <left_row> <right_column> <right_row>
//   out: per case one line  <return code of init> <return code of every copy ...>  and one line with the mapping (empty when init refused)
#include <cinttypes>
#include <cstdio>

#include "../../tiny-ram-halo2_amd/csrc/permkeygen.h"

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: permkeygen_test <in> <out>\n"); return 2; }
    FILE* in = std::fopen(argv[1], "r");
    FILE* out = std::fopen(argv[2], "w");
    if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    unsigned long cases = 0;
    if (std::fscanf(in, "%lu", &cases) != 1) return 2;
    for (unsigned long t = 0; t < cases; ++t) {
        uint64_t n_columns = 0, k = 0, copies = 0;
        if (std::fscanf(in, "%" SCNu64 " %" SCNu64 " %" SCNu64, &n_columns, &k, &copies) != 3) return 2;
        trh::PermAssembly a;
        const int rc = (n_columns >> 32 || k >> 32) ? TRH_EINVAL : a.init((uint32_t)n_columns, (uint32_t)k);
        std::fprintf(out, "%d", rc);
        for (uint64_t i = 0; i < copies; ++i) {
            uint64_t q[4];
            if (std::fscanf(in, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &q[0], &q[1], &q[2], &q[3]) != 4) return 2;
            if (rc != TRH_OK) continue;
            const bool fits = !(q[0] >> 32 || q[1] >> 32 || q[2] >> 32 || q[3] >> 32);
            std::fprintf(out, " %d", fits ? a.copy((uint32_t)q[0], (uint32_t)q[1], (uint32_t)q[2], (uint32_t)q[3]) : TRH_EINVAL);
        }
        std::fprintf(out, "\n");
        if (rc == TRH_OK) {
            for (size_t i = 0; i < a.cells; ++i) std::fprintf(out, i ? " %" PRIu32 : "%" PRIu32, a.mapping[i]);
            // the bookkeeping the mapping was built with must still describe it: every cell's representative is in its own cycle
            for (size_t i = 0; i < a.cells; ++i) if (a.aux[a.mapping[i]] != a.aux[i] || a.aux[a.aux[i]] != a.aux[i]) { std::fprintf(stderr, "aux broken at cell %zu\n", i); return 1; }
        }
        std::fprintf(out, "\n");
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    std::printf("permkeygen: ok (%lu cases)\n", cases);
    return 0;
}
