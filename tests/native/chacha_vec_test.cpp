// Host driver of csrc/chacha.h: chacha20_block and fe_from_u512 through the plain C++ branch of the header, record by record.  Built by g++ with
// -fsanitize=undefined -fno-sanitize-recover (tests/test_rng_host.py).  No GPU, no HIP.
//   usage: chacha_vec_test <block|fp|fq> <case file> <result file>
//   block:   records of 32 key bytes, counter (u64), stream id (u64), little endian; result: the block's 64 bytes per record
//   fp / fq: records of 64 bytes (a 512-bit little-endian value); result: 4 x u64 per record (from_u512, Montgomery words)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../tiny-ram-halo2_amd/csrc/chacha.h"

static bool read_all(const char* src, size_t record, std::vector<unsigned char>& buf) {
    std::FILE* in = std::fopen(src, "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", src); return false; }
    unsigned char chunk[4096];
    for (size_t got; (got = std::fread(chunk, 1, sizeof(chunk), in)) > 0;) buf.insert(buf.end(), chunk, chunk + got);
    std::fclose(in);
    if (buf.size() % record) { std::fprintf(stderr, "%s: not a whole number of records\n", src); return false; }
    return true;
}

static int run_blocks(const char* src, const char* dst) {
    std::vector<unsigned char> buf;
    if (!read_all(src, 48, buf)) return 1;
    std::FILE* out = std::fopen(dst, "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", dst); return 1; }
    const size_t n = buf.size() / 48;
    for (size_t i = 0; i < n; ++i) {
        trh::u32 key[8], blk[16];
        trh::u64 counter, stream_id;
        std::memcpy(key, &buf[48 * i], 32);
        std::memcpy(&counter, &buf[48 * i + 32], 8);
        std::memcpy(&stream_id, &buf[48 * i + 40], 8);
        trh::chacha20_block(key, counter, stream_id, blk);
        if (std::fwrite(blk, 1, 64, out) != 64) { std::fprintf(stderr, "short write\n"); return 1; }
    }
    std::fclose(out);
    std::printf("chacha_vec: %zu records ok\n", n);
    return 0;
}

template <class F> static int run_reduce(const char* src, const char* dst) {
    std::vector<unsigned char> buf;
    if (!read_all(src, 64, buf)) return 1;
    std::FILE* out = std::fopen(dst, "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", dst); return 1; }
    const size_t n = buf.size() / 64;
    for (size_t i = 0; i < n; ++i) {
        trh::u32 w[16], r[8];
        std::memcpy(w, &buf[64 * i], 64);
        trh::fe_store(trh::fe_from_u512<F>(w), r);
        if (std::fwrite(r, 1, 32, out) != 32) { std::fprintf(stderr, "short write\n"); return 1; }
    }
    std::fclose(out);
    std::printf("chacha_vec: %zu records ok\n", n);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: %s <block|fp|fq> <case file> <result file>\n", argv[0]); return 1; }
    if (!std::strcmp(argv[1], "block")) return run_blocks(argv[2], argv[3]);
    if (!std::strcmp(argv[1], "fp")) return run_reduce<trh::FpParams>(argv[2], argv[3]);
    if (!std::strcmp(argv[1], "fq")) return run_reduce<trh::FqParams>(argv[2], argv[3]);
    std::fprintf(stderr, "unknown mode %s\n", argv[1]);
    return 1;
}
