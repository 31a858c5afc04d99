// Host driver of csrc/blake2b.h (with a personalisation), csrc/transcript.h and trh::Blake2bWrite / Blake2bRead of include/trh.hpp.  Built by
// the Makefile with -fsanitize=address,undefined -fno-sanitize-recover=all; run by tests/test_transcript_host.py, which checks the results
// against hashlib and tests/transcript_model.py.  No GPU, no HIP, no libtrh: the trh_tr_* entries trh.hpp calls come from
// tests/native/transcript_abi.cpp, which defines them from csrc/transcript.h (a file of its own: csrc/curve.h and trh.hpp both name a trh::Affine).
//   usage: transcript_test hash <case file> <result file>
//          transcript_test script <pallas|vesta> <case file> <result file>
// hash: the case file is a run of byte strings, each a little-endian u32 length and that many bytes; the result is the 64-byte digest of each
//       under the personalisation "Halo2-Transcript", absorbed in two pieces (split in the middle) through the incremental form.
// script: the case file is a run of operations, one byte each and their operand:
//       'p' common_point (96 bytes, normalised Jacobian)   'P' write_point (96)   's' common_scalar (32, Montgomery)   'S' write_scalar (32)
//       'C' squeeze_challenge_scalar
//   A Blake2bWrite runs them; a Blake2bRead over its bytes then runs them again with reads in place of the writes and has to see the same
//   points, scalars and challenges, to be finished() exactly after the last item, and to refuse -- for good -- one read more.  The result
//   file holds the challenges (32 bytes each, Montgomery) and then the proof.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/trh.hpp"
#include "../../tiny-ram-halo2_amd/csrc/blake2b.h"

static const uint8_t PERSON[16] = {'H', 'a', 'l', 'o', '2', '-', 'T', 'r', 'a', 'n', 's', 'c', 'r', 'i', 'p', 't'};

typedef std::vector<unsigned char> Bytes;

static bool read_file(const char* src, Bytes& buf) {
    std::FILE* in = std::fopen(src, "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", src); return false; }
    unsigned char chunk[4096];
    for (size_t got; (got = std::fread(chunk, 1, sizeof(chunk), in)) > 0;) buf.insert(buf.end(), chunk, chunk + got);
    std::fclose(in);
    return true;
}
static bool write_file(const char* dst, const Bytes& out) {
    std::FILE* f = std::fopen(dst, "wb");
    if (!f) { std::fprintf(stderr, "cannot write %s\n", dst); return false; }
    const bool ok = out.empty() || std::fwrite(out.data(), 1, out.size(), f) == out.size();
    std::fclose(f);
    if (!ok) std::fprintf(stderr, "short write\n");
    return ok;
}

static int run_hash(const Bytes& in, Bytes& out) {
    size_t records = 0;
    for (size_t at = 0; at < in.size(); ++records) {
        if (in.size() - at < 4) { std::fprintf(stderr, "truncated length\n"); return 1; }
        trh::u32 len;
        std::memcpy(&len, &in[at], 4);
        at += 4;
        if (in.size() - at < len) { std::fprintf(stderr, "truncated string\n"); return 1; }
        trh::Blake2b s(PERSON);
        s.update(in.data() + at, len / 2);
        s.update(in.data() + at + len / 2, len - len / 2);
        const trh::Blake2b before = s;
        trh::Blake2b copy = s;  // as the sponge squeezes: the digest comes from a copy
        unsigned char d[trh::BLAKE2B_OUT];
        copy.finish(d);
        if (std::memcmp(&before, &s, sizeof(s)) != 0) { std::fprintf(stderr, "finish on a copy changed the state\n"); return 1; }
        out.insert(out.end(), d, d + trh::BLAKE2B_OUT);
        at += len;
    }
    std::printf("transcript_test: %zu digests ok\n", records);
    return 0;
}

struct Op { char kind; trh::Point point; trh::Limbs scalar; };

template <class Fn> static bool throws(Fn&& fn) {
    try { fn(); } catch (const trh::Error&) { return true; }
    return false;
}

static int run_script(trh::Curve curve, const Bytes& in, Bytes& out) {
    std::vector<Op> ops;
    for (size_t at = 0; at < in.size();) {
        Op op{};
        op.kind = (char)in[at++];
        const size_t need = op.kind == 'p' || op.kind == 'P' ? 96 : op.kind == 's' || op.kind == 'S' ? 32 : op.kind == 'C' ? 0 : (size_t)-1;
        if (need == (size_t)-1 || in.size() - at < need) { std::fprintf(stderr, "bad operation at byte %zu\n", at - 1); return 1; }
        if (need == 96) std::memcpy(&op.point, &in[at], 96);
        if (need == 32) std::memcpy(op.scalar.data(), &in[at], 32);
        at += need;
        ops.push_back(op);
    }
    trh::Blake2bWrite w(curve);
    std::vector<trh::Limbs> challenges;
    for (const Op& op : ops) {
        switch (op.kind) {
            case 'p': w.common_point(op.point); break;
            case 'P': w.write_point(op.point); break;
            case 's': w.common_scalar(op.scalar); break;
            case 'S': w.write_scalar(op.scalar); break;
            default: challenges.push_back(w.squeeze_challenge_scalar());
        }
    }
    w.throw_if_failed();
    const Bytes proof = w.bytes();

    // the callbacks of the library over a second writer: the same bytes and challenges as the methods
    trh::Blake2bWrite w2(curve);
    const trh_transcript_t cb = w2.callbacks();
    size_t next = 0;
    for (const Op& op : ops) {
        switch (op.kind) {
            case 'p': w2.common_point(op.point); break;
            case 'P': cb.write_point(cb.ctx, (const uint64_t*)&op.point); break;
            case 's': w2.common_scalar(op.scalar); break;
            case 'S': cb.write_scalar(cb.ctx, op.scalar.data()); break;
            default: {
                trh::Limbs c;
                cb.squeeze_challenge_scalar(cb.ctx, c.data());
                if (c != challenges[next++]) { std::fprintf(stderr, "the callback squeezed another challenge\n"); return 1; }
            }
        }
    }
    w2.throw_if_failed();
    if (w2.bytes() != proof) { std::fprintf(stderr, "the callbacks wrote other bytes\n"); return 1; }

    // the round trip
    trh::Blake2bRead r(curve, proof);
    next = 0;
    size_t items_left = 0;
    for (const Op& op : ops) items_left += op.kind == 'P' || op.kind == 'S';
    for (const Op& op : ops) {
        if (r.finished() != (items_left == 0)) { std::fprintf(stderr, "finished() with %zu items left\n", items_left); return 1; }
        switch (op.kind) {
            case 'p': r.common_point(op.point); break;
            case 's': r.common_scalar(op.scalar); break;
            case 'P': {
                const trh::Affine a = r.read_point();
                if (std::memcmp(&a, &op.point, 64) != 0) { std::fprintf(stderr, "read_point gave another point\n"); return 1; }
                --items_left;
                break;
            }
            case 'S':
                if (r.read_scalar() != op.scalar) { std::fprintf(stderr, "read_scalar gave another scalar\n"); return 1; }
                --items_left;
                break;
            default:
                if (r.squeeze_challenge_scalar() != challenges[next++]) { std::fprintf(stderr, "the reader squeezed another challenge\n"); return 1; }
        }
    }
    if (!r.finished() || r.remaining() != 0) { std::fprintf(stderr, "the reader is not finished at the end\n"); return 1; }
    // one read too many: trh::Error, and the error stays
    if (!throws([&] { r.read_scalar(); }) || !throws([&] { r.squeeze_challenge_scalar(); }) || !throws([&] { r.throw_if_failed(); })) {
        std::fprintf(stderr, "a read past the end was not refused for good\n");
        return 1;
    }
    // the identity is no transcript point, and a reader does not write
    trh::Blake2bWrite w3(curve);
    trh::Point identity{};
    if (!throws([&] { w3.write_point(identity); }) || !w3.bytes().empty() || !throws([&] { w3.write_scalar(trh::Limbs{0, 0, 0, 0}); })) {
        std::fprintf(stderr, "the identity was written\n");
        return 1;
    }
    trh::Blake2bRead r2(curve, proof);
    trh_transcript_t none;
    if (trh_tr_callbacks(r2.handle(), &none) != TRH_EINVAL || trh_tr_write_scalar(r2.handle(), ops[0].scalar.data()) != TRH_EINVAL) {
        std::fprintf(stderr, "a reader wrote\n");
        return 1;
    }
    if (!throws([] { trh::Blake2bWrite bad((trh::Curve)2); }) || !std::strstr(trh_last_error(), "unknown curve id")) {
        std::fprintf(stderr, "curve id 2 was taken\n");
        return 1;
    }
    for (const trh::Limbs& c : challenges) out.insert(out.end(), (const unsigned char*)c.data(), (const unsigned char*)c.data() + 32);
    out.insert(out.end(), proof.begin(), proof.end());
    std::printf("transcript_test: %zu operations, %zu challenges, %zu proof bytes ok\n", ops.size(), challenges.size(), proof.size());
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    Bytes in, out;
    int rc = 1;
    try {
        if (mode == "hash" && argc == 4) {
            if (!read_file(argv[2], in)) return 1;
            rc = run_hash(in, out);
        } else if (mode == "script" && argc == 5 && (!std::strcmp(argv[2], "pallas") || !std::strcmp(argv[2], "vesta"))) {
            if (!read_file(argv[3], in)) return 1;
            rc = run_script(argv[2][0] == 'p' ? trh::Curve::Pallas : trh::Curve::Vesta, in, out);
        } else {
            std::fprintf(stderr, "usage: %s hash <case file> <result file> | script <pallas|vesta> <case file> <result file>\n", argv[0]);
            return 1;
        }
    } catch (const trh::Error& e) {
        std::fprintf(stderr, "trh::Error: %s\n", e.what());
        return 1;
    }
    if (rc) return rc;
    return write_file(argv[argc - 1], out) ? 0 : 1;
}
