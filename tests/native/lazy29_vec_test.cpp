// Host driver of the lazy-domain case runner (lazy29_cases.h): the records of a case file through the plain C++ branch of
// csrc/field.h / csrc/curve.h.  Built by g++ with -fsanitize=undefined -fno-sanitize-recover (tests/test_lazy29_vectors.py): a record
// at the edge of a stated bound that overflows a 32-bit limb or a 64-bit column ends the run there.  No GPU, no HIP.
//   usage: lazy29_vec_test <case file> <result file>
#include "lazy29_cases.h"

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s <case file> <result file>\n", argv[0]); return 1; }
    std::vector<lz::Rec> recs;
    if (!lz::read_cases(argv[1], recs)) return 1;
    std::vector<lz::Out> out(recs.size());
    for (size_t i = 0; i < recs.size(); ++i) lz::host_case(recs[i], out[i]);
    if (!lz::write_results(argv[2], out)) return 1;
    std::printf("lazy29_vec: %zu records ok\n", recs.size());
    return 0;
}
