// Host driver of csrc/fieldsqrt.h: fe_sqrt through the plain C++ branch of the header, record by record.  Built by g++ with
// -fsanitize=undefined -fno-sanitize-recover (tests/test_encoding_host.py).  No GPU, no HIP.
//   usage: fieldsqrt_vec_test <fp|fq> <case file> <result file>
//   case file: records of 4 x u64 (Montgomery words); result file: per record 4 x u64 (the root, Montgomery) and one byte (is_square)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../tiny-ram-halo2_amd/csrc/fieldsqrt.h"

template <class F> static int run(const char* src, const char* dst) {
    std::FILE* in = std::fopen(src, "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", src); return 1; }
    std::vector<unsigned char> buf;
    unsigned char chunk[4096];
    for (size_t got; (got = std::fread(chunk, 1, sizeof(chunk), in)) > 0;) buf.insert(buf.end(), chunk, chunk + got);
    std::fclose(in);
    if (buf.size() % 32) { std::fprintf(stderr, "%s: not a whole number of records\n", src); return 1; }
    std::FILE* out = std::fopen(dst, "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", dst); return 1; }
    const size_t n = buf.size() / 32;
    for (size_t i = 0; i < n; ++i) {
        trh::u32 w[8];
        std::memcpy(w, &buf[32 * i], 32);
        bool sq = false;
        const trh::Fe<F> r = trh::fe_sqrt(trh::fe_load<F>(w), &sq);
        trh::fe_store(r, w);
        const unsigned char flag = sq ? 1 : 0;
        if (std::fwrite(w, 1, 32, out) != 32 || std::fwrite(&flag, 1, 1, out) != 1) { std::fprintf(stderr, "short write\n"); return 1; }
    }
    std::fclose(out);
    std::printf("fieldsqrt_vec: %zu records ok\n", n);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: %s <fp|fq> <case file> <result file>\n", argv[0]); return 1; }
    if (!std::strcmp(argv[1], "fp")) return run<trh::FpParams>(argv[2], argv[3]);
    if (!std::strcmp(argv[1], "fq")) return run<trh::FqParams>(argv[2], argv[3]);
    std::fprintf(stderr, "unknown field %s\n", argv[1]);
    return 1;
}
