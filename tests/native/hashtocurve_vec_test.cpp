// Host driver of csrc/blake2b.h and csrc/hashtocurve.h through the plain C++ branch of the headers, record by record.  Built by the Makefile
// with -fsanitize=address,undefined -fno-sanitize-recover=all; run by tests/test_hashtocurve_host.py, which checks the results against hashlib
// and tests/hash_to_curve_model.py.  No GPU, no HIP.
//   usage: hashtocurve_vec_test <mode> <pallas|vesta> <case file> <result file>
// A case file is a run of byte strings, each a little-endian u32 length and that many bytes; a record is the strings its mode names:
//   blake2b   input                      -> the 64-byte digest (the curve argument is ignored)
//   field     prefix, message            -> u0, u1 (2 x 4 u64 Montgomery) through the byte-wise path of trh_hash_to_curve
//   indexed   prefix, tag (1), index (4) -> u0, u1 through H2cPlan and h2c_hash_to_field_indexed, the path of the device kernel
//   map       1 or 2 elements (32 or 64) -> the 64-byte affine POD of iso_map(sum swu(u))
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../tiny-ram-halo2_amd/csrc/hashtocurve.h"

typedef std::vector<unsigned char> Bytes;

static bool read_strings(const char* src, std::vector<Bytes>& out) {
    std::FILE* in = std::fopen(src, "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", src); return false; }
    Bytes buf;
    unsigned char chunk[4096];
    for (size_t got; (got = std::fread(chunk, 1, sizeof(chunk), in)) > 0;) buf.insert(buf.end(), chunk, chunk + got);
    std::fclose(in);
    for (size_t at = 0; at < buf.size();) {
        if (buf.size() - at < 4) { std::fprintf(stderr, "%s: truncated length\n", src); return false; }
        trh::u32 len;
        std::memcpy(&len, &buf[at], 4);
        at += 4;
        if (buf.size() - at < len) { std::fprintf(stderr, "%s: truncated string\n", src); return false; }
        out.emplace_back(buf.begin() + at, buf.begin() + at + len);
        at += len;
    }
    return true;
}

template <class F> static void put_fe(Bytes& out, const trh::Fe<F>& v) {
    trh::u32 w[8];
    trh::fe_store(v, w);
    const unsigned char* p = (const unsigned char*)w;
    out.insert(out.end(), p, p + 32);
}

template <class F> static int run(const std::string& mode, bool pallas, const std::vector<Bytes>& s, Bytes& out, size_t& records) {
    using namespace trh;
    const size_t per = mode == "blake2b" || mode == "map" ? 1 : mode == "field" ? 2 : 3;
    if (s.size() % per) { std::fprintf(stderr, "not a whole number of records\n"); return 1; }
    for (size_t i = 0; i < s.size(); i += per) {
        if (mode == "blake2b") {
            unsigned char d[BLAKE2B_OUT];
            blake2b_512(s[i].data(), s[i].size(), d);
            out.insert(out.end(), d, d + BLAKE2B_OUT);
        } else if (mode == "map") {
            if (s[i].size() != 32 && s[i].size() != 64) { std::fprintf(stderr, "map: 32 or 64 bytes per record\n"); return 1; }
            XYZZ<F> acc = xyzz_identity<F>();
            for (size_t j = 0; j < s[i].size() / 32; ++j) {
                u32 w[8];
                std::memcpy(w, &s[i][32 * j], 32);
                h2c_accumulate(acc, fe_load<F>(w), sqrt_table_host<F>());
            }
            const Affine<F> p = xyzz_to_affine(acc);
            put_fe(out, p.x); put_fe(out, p.y);
        } else {
            if (s[i].size() > H2C_MAX_PREFIX) { std::fprintf(stderr, "prefix too long\n"); return 1; }
            uint8_t dstp[H2C_MAX_DSTP];
            const size_t dstp_len = h2c_dst_prime(pallas, (const char*)s[i].data(), s[i].size(), dstp);
            Fe<F> u0, u1;
            if (mode == "field") {
                h2c_hash_to_field_bytes<F>(dstp, dstp_len, s[i + 1].data(), s[i + 1].size(), u0, u1);
            } else {
                if (s[i + 1].size() != 1 || s[i + 2].size() != 4) { std::fprintf(stderr, "indexed: tag is 1 byte, index 4\n"); return 1; }
                u32 index;
                std::memcpy(&index, s[i + 2].data(), 4);
                H2cPlan plan;
                h2c_plan_build(plan, dstp, dstp_len, s[i + 1][0]);
                h2c_hash_to_field_indexed<F>(plan, index, u0, u1);
            }
            put_fe(out, u0); put_fe(out, u1);
        }
        ++records;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 5) { std::fprintf(stderr, "usage: %s <blake2b|field|indexed|map> <pallas|vesta> <case file> <result file>\n", argv[0]); return 1; }
    const std::string mode = argv[1], curve = argv[2];
    if (mode != "blake2b" && mode != "field" && mode != "indexed" && mode != "map") { std::fprintf(stderr, "unknown mode %s\n", argv[1]); return 1; }
    if (curve != "pallas" && curve != "vesta") { std::fprintf(stderr, "unknown curve %s\n", argv[2]); return 1; }
    std::vector<Bytes> strings;
    if (!read_strings(argv[3], strings)) return 1;
    Bytes out;
    size_t records = 0;
    const int rc = curve == "pallas" ? run<trh::FpParams>(mode, true, strings, out, records) : run<trh::FqParams>(mode, false, strings, out, records);
    if (rc) return rc;
    std::FILE* f = std::fopen(argv[4], "wb");
    if (!f) { std::fprintf(stderr, "cannot write %s\n", argv[4]); return 1; }
    if (!out.empty() && std::fwrite(out.data(), 1, out.size(), f) != out.size()) { std::fprintf(stderr, "short write\n"); return 1; }
    std::fclose(f);
    std::printf("hashtocurve_vec: %zu records ok\n", records);
    return 0;
}
