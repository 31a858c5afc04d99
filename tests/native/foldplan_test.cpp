// csrc/foldplan.h without a device: the bucket lists the generator collapse (ipafold.hip) walks, for scalars and table shapes read from a
// file.  The plans go back to a file as they are; tests/test_foldplan.py reconstructs every scalar from them with big integers.  Built
// with address + undefined sanitizers.
//   in : cases, then per case "c W w0 w1 n" and n scalars as four hexadecimal 64-bit words, least significant first
//   out: per case "rc nbk words" and the plan's words in decimal on one line (none when rc != 0)
// Plain C++: foldplan_test <in> <out>
#include <cinttypes>
#include <cstdio>

#include "../../tiny-ram-halo2_amd/csrc/foldplan.h"

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: foldplan_test <in> <out>\n"); return 2; }
    FILE* in = std::fopen(argv[1], "r");
    FILE* out = std::fopen(argv[2], "w");
    if (!in || !out) { std::fprintf(stderr, "foldplan: cannot open the files\n"); return 2; }
    unsigned cases = 0;
    if (std::fscanf(in, "%u", &cases) != 1) { std::fprintf(stderr, "foldplan: no case count\n"); return 2; }
    for (unsigned q = 0; q < cases; ++q) {
        int c = 0, W = 0;
        unsigned w0 = 0, w1 = 0;
        size_t n = 0;
        if (std::fscanf(in, "%d %d %u %u %zu", &c, &W, &w0, &w1, &n) != 5) { std::fprintf(stderr, "foldplan: case %u: bad header\n", q); return 2; }
        std::vector<trh::hostcombine::H> sc(n);
        for (size_t t = 0; t < n; ++t)
            if (std::fscanf(in, "%" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64, &sc[t].l[0], &sc[t].l[1], &sc[t].l[2], &sc[t].l[3]) != 4) {
                std::fprintf(stderr, "foldplan: case %u: bad scalar %zu\n", q, t);
                return 2;
            }
        std::vector<uint32_t> plan;
        uint32_t nbk = 0;
        const int rc = trh::foldplan::fold_plan(sc, c, W, w0, w1, plan, nbk);
        if (rc != trh::foldplan::FOLD_PLAN_OK) plan.clear();
        std::fprintf(out, "%d %u %zu\n", rc, nbk, plan.size());
        for (size_t e = 0; e < plan.size(); ++e) std::fprintf(out, e ? " %u" : "%u", plan[e]);
        std::fprintf(out, "\n");
    }
    std::fclose(in);
    if (std::fclose(out) != 0) { std::fprintf(stderr, "foldplan: write failed\n"); return 2; }
    std::printf("foldplan: ok (%u cases)\n", cases);
    return 0;
}
