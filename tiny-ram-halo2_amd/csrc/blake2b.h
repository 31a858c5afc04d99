// BLAKE2b (RFC 7693) with a 64-byte digest, no key and no salt.  With an all-zero personalisation it is the hash under hash_to_curve's
// expand_message (csrc/hashtocurve.h), one message per lane; with the 16 bytes "Halo2-Transcript" it is the sponge of the proof transcript
// (csrc/transcript.h, host only).
//
// The compression function works on 64-bit words with add / xor / rotate right by 32, 24, 16 and 63.  gfx950's vector ALU is 32 bits wide: an
// add is an add plus an add-with-carry, a xor two xors, and the rotations cost what their amount allows -- 32 swaps the two halves (no
// instruction at all once the rounds are unrolled), 24 and 16 move whole bytes (one v_perm_b32 per half), 63 is one v_alignbit_b32 per half.
// The rotation is written as plain shifts below and left to the compiler, as chacha.h leaves its 32-bit ones.
// The twelve rounds are unrolled through the template parameter R, so that SIGMA[R][i] is a constant and m[SIGMA[R][i]] names a register;
// with a runtime round counter the sixteen message words would be indexed at run time and live in scratch memory.
//
// Plain C++ for host and device, no inline assembly: the host branch serves trh_hash_to_curve and the stand-alone test program
// (tests/native/hashtocurve_vec_test.cpp, against hashlib).
#pragma once
#include <stddef.h>

#include "field.h"

namespace trh {

constexpr size_t BLAKE2B_BLOCK = 128, BLAKE2B_OUT = 64;

template <int K> struct Blake2bIv;
#define TRH_B2_IV(k, val) template <> struct Blake2bIv<k> { static constexpr u64 v = val; }
TRH_B2_IV(0, 0x6a09e667f3bcc908ull); TRH_B2_IV(1, 0xbb67ae8584caa73bull); TRH_B2_IV(2, 0x3c6ef372fe94f82bull); TRH_B2_IV(3, 0xa54ff53a5f1d36f1ull);
TRH_B2_IV(4, 0x510e527fade682d1ull); TRH_B2_IV(5, 0x9b05688c2b3e6c1full); TRH_B2_IV(6, 0x1f83d9abfb41bd6bull); TRH_B2_IV(7, 0x5be0cd19137e2179ull);
#undef TRH_B2_IV

// SIGMA of RFC 7693 section 2.7, row R mod 10, as a compile-time function (a table in memory would be read with a runtime address on the device)
constexpr int blake2b_sigma(int r, int i) {
    constexpr unsigned char S[10][16] = {
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
        {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
        {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
        {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
        {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
    return S[r % 10][i];
}

template <int R, int I> struct Blake2bSigma { static constexpr int v = blake2b_sigma(R, I); };

TRH_HD u64 blake2b_rotr(u64 v, int c) { return (v >> c) | (v << (64 - c)); }  // c in {32, 24, 16, 63}

#define TRH_B2_G(a, b, c, d, x, y)                       \
    do {                                                 \
        a = a + b + (x); d = blake2b_rotr(d ^ a, 32);    \
        c = c + d;       b = blake2b_rotr(b ^ c, 24);    \
        a = a + b + (y); d = blake2b_rotr(d ^ a, 16);    \
        c = c + d;       b = blake2b_rotr(b ^ c, 63);    \
    } while (0)

template <int R> TRH_HD void blake2b_rounds(u64 (&v)[16], const u64 (&m)[16]) {
    if constexpr (R < 12) {
        TRH_B2_G(v[0], v[4], v[8], v[12], (m[Blake2bSigma<R, 0>::v]), (m[Blake2bSigma<R, 1>::v]));
        TRH_B2_G(v[1], v[5], v[9], v[13], (m[Blake2bSigma<R, 2>::v]), (m[Blake2bSigma<R, 3>::v]));
        TRH_B2_G(v[2], v[6], v[10], v[14], (m[Blake2bSigma<R, 4>::v]), (m[Blake2bSigma<R, 5>::v]));
        TRH_B2_G(v[3], v[7], v[11], v[15], (m[Blake2bSigma<R, 6>::v]), (m[Blake2bSigma<R, 7>::v]));
        TRH_B2_G(v[0], v[5], v[10], v[15], (m[Blake2bSigma<R, 8>::v]), (m[Blake2bSigma<R, 9>::v]));
        TRH_B2_G(v[1], v[6], v[11], v[12], (m[Blake2bSigma<R, 10>::v]), (m[Blake2bSigma<R, 11>::v]));
        TRH_B2_G(v[2], v[7], v[8], v[13], (m[Blake2bSigma<R, 12>::v]), (m[Blake2bSigma<R, 13>::v]));
        TRH_B2_G(v[3], v[4], v[9], v[14], (m[Blake2bSigma<R, 14>::v]), (m[Blake2bSigma<R, 15>::v]));
        blake2b_rounds<R + 1>(v, m);
    }
}
#undef TRH_B2_G

// h after section 3.2's initialisation for a 64-byte digest without key: IV with the parameter word 0x01010040 folded into h[0]
TRH_HD void blake2b_init(u64 (&h)[8]) {
    h[0] = Blake2bIv<0>::v ^ 0x01010040ull; h[1] = Blake2bIv<1>::v; h[2] = Blake2bIv<2>::v; h[3] = Blake2bIv<3>::v;
    h[4] = Blake2bIv<4>::v; h[5] = Blake2bIv<5>::v; h[6] = Blake2bIv<6>::v; h[7] = Blake2bIv<7>::v;
}

// the same with a 16-byte personalisation: bytes 48 .. 63 of the parameter block (section 2.5) are its words 6 and 7, little endian
inline void blake2b_init_personal(u64 (&h)[8], const uint8_t person[16]) {
    blake2b_init(h);
    u64 p0 = 0, p1 = 0;
    for (int i = 0; i < 8; ++i) { p0 |= (u64)person[i] << (8 * i); p1 |= (u64)person[8 + i] << (8 * i); }
    h[6] ^= p0;
    h[7] ^= p1;
}

// F of section 3.2: m the block's sixteen little-endian words, t the number of bytes hashed up to and including this block (below 2^64:
// the high counter word stays zero), last for the final block
TRH_HD void blake2b_compress(u64 (&h)[8], const u64 (&m)[16], u64 t, bool last) {
    u64 v[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = h[i];
    v[8] = Blake2bIv<0>::v; v[9] = Blake2bIv<1>::v; v[10] = Blake2bIv<2>::v; v[11] = Blake2bIv<3>::v;
    v[12] = Blake2bIv<4>::v ^ t; v[13] = Blake2bIv<5>::v;
    v[14] = last ? ~Blake2bIv<6>::v : Blake2bIv<6>::v; v[15] = Blake2bIv<7>::v;
    blake2b_rounds<0>(v, m);
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[i + 8];
}

// the words of a block from bytes (fewer than 128: zero padded)
inline void blake2b_block_words(const uint8_t* in, size_t len, u64 (&m)[16]) {
    for (int i = 0; i < 16; ++i) m[i] = 0;
    for (size_t i = 0; i < len && i < BLAKE2B_BLOCK; ++i) m[i >> 3] |= (u64)in[i] << (8 * (i & 7));
}

// Incremental form for byte strings (host side).  A full buffer is compressed only when more input follows: the last block -- a full one
// when the length is a positive multiple of 128 -- must carry the final flag.  finish() ends the state it is called on: a sponge that goes
// on absorbing after a digest calls it on a COPY, so the struct stays trivially copyable.
struct Blake2b {
    u64 h[8];
    u64 t = 0;
    uint8_t buf[BLAKE2B_BLOCK];
    size_t fill = 0;
    Blake2b() { blake2b_init(h); }
    explicit Blake2b(const uint8_t person[16]) { blake2b_init_personal(h, person); }
    void update(const uint8_t* in, size_t len) {
        while (len) {
            if (fill == BLAKE2B_BLOCK) {
                u64 m[16];
                blake2b_block_words(buf, BLAKE2B_BLOCK, m);
                t += BLAKE2B_BLOCK;
                blake2b_compress(h, m, t, false);
                fill = 0;
            }
            size_t take = BLAKE2B_BLOCK - fill;
            if (take > len) take = len;
            for (size_t i = 0; i < take; ++i) buf[fill + i] = in[i];
            fill += take; in += take; len -= take;
        }
    }
    void finish(uint8_t out[BLAKE2B_OUT]) {
        u64 m[16];
        blake2b_block_words(buf, fill, m);
        t += fill;
        blake2b_compress(h, m, t, true);
        for (size_t i = 0; i < BLAKE2B_OUT; ++i) out[i] = (uint8_t)(h[i >> 3] >> (8 * (i & 7)));
    }
};
inline void blake2b_512(const uint8_t* in, size_t len, uint8_t out[BLAKE2B_OUT]) {
    Blake2b s;
    s.update(in, len);
    s.finish(out);
}

}  // namespace trh
