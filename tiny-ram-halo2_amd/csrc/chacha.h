// The prover's random scalars as a deterministic stream: ChaCha20 blocks turned into Pasta field elements, for one element per lane.
//
// What it replaces: a host loop of `C::Scalar::random(&mut rng)` over a `rand_chacha::ChaCha20Rng::from_seed(seed)` -- eight next_u64 and one
// `from_u512` per scalar -- followed by an upload of 32 bytes per scalar.  Here the host hands over the 32-byte key once and element i of the
// stream is made where it is used:
//   1. ChaCha20 block number i: the block function of RFC 8439 section 2.3 (20 rounds) over the ORIGINAL 64 + 64 state layout -- words 0 - 3
//      the constants, 4 - 11 the key, 12 - 13 the 64-bit block counter (low word first), 14 - 15 the 64-bit stream id (low word first).  The RFC's
//      32 + 96 layout is the same function: its counter is word 12 and its nonce words 13 - 15.
//   2. the 64 output bytes as eight little-endian u64 limbs[0 .. 8) (sixteen u32 words here, the same bytes);
//   3. pasta_curves' `from_u512`: (limbs[0 .. 4) + 2^256 limbs[4 .. 8)) mod m, in Montgomery form, fully reduced.
// One element is exactly one block and a position in the stream is a block number, so any range of elements can be produced by any
// number of threads without state.  That rand_chacha / pasta_curves produce these very words is recalled, not pinned by anything in the
// reference; the block function is pinned by the RFC's vectors, the reduction by integers (tests/chacha_model.py).
//
// Plain C++ for host and device, no inline assembly: the host branch serves trh_rng_next_scalar and the stand-alone test program.
#pragma once
#include "field.h"

namespace trh {

// the key as a kernel argument (32 bytes of the launch's argument block: nothing to upload, nothing left behind in device memory)
struct ChaChaKey {
    u32 w[8];
};

TRH_HD u32 chacha_rotl(u32 v, int c) { return (v << c) | (v >> (32 - c)); }  // c in {16, 12, 8, 7}; the compiler makes it one v_alignbit_b32

#define TRH_CHACHA_QR(a, b, c, d)                    \
    do {                                             \
        a += b; d ^= a; d = chacha_rotl(d, 16);      \
        c += d; b ^= c; b = chacha_rotl(b, 12);      \
        a += b; d ^= a; d = chacha_rotl(d, 8);       \
        c += d; b ^= c; b = chacha_rotl(b, 7);       \
    } while (0)

// out: the block's sixteen words; its 64 bytes are these words in little-endian order
TRH_HD void chacha20_block(const u32 key[8], u64 counter, u64 stream_id, u32 out[16]) {
    const u32 s0 = 0x61707865u, s1 = 0x3320646eu, s2 = 0x79622d32u, s3 = 0x6b206574u;  // "expand 32-byte k"
    const u32 s12 = (u32)counter, s13 = (u32)(counter >> 32), s14 = (u32)stream_id, s15 = (u32)(stream_id >> 32);
    u32 x0 = s0, x1 = s1, x2 = s2, x3 = s3, x4 = key[0], x5 = key[1], x6 = key[2], x7 = key[3];
    u32 x8 = key[4], x9 = key[5], x10 = key[6], x11 = key[7], x12 = s12, x13 = s13, x14 = s14, x15 = s15;
#pragma unroll
    for (int r = 0; r < 10; ++r) {  // ten double rounds: columns, then diagonals
        TRH_CHACHA_QR(x0, x4, x8, x12);
        TRH_CHACHA_QR(x1, x5, x9, x13);
        TRH_CHACHA_QR(x2, x6, x10, x14);
        TRH_CHACHA_QR(x3, x7, x11, x15);
        TRH_CHACHA_QR(x0, x5, x10, x15);
        TRH_CHACHA_QR(x1, x6, x11, x12);
        TRH_CHACHA_QR(x2, x7, x8, x13);
        TRH_CHACHA_QR(x3, x4, x9, x14);
    }
    out[0] = x0 + s0; out[1] = x1 + s1; out[2] = x2 + s2; out[3] = x3 + s3;
    out[4] = x4 + key[0]; out[5] = x5 + key[1]; out[6] = x6 + key[2]; out[7] = x7 + key[3];
    out[8] = x8 + key[4]; out[9] = x9 + key[5]; out[10] = x10 + key[6]; out[11] = x11 + key[7];
    out[12] = x12 + s12; out[13] = x13 + s13; out[14] = x14 + s14; out[15] = x15 + s15;
}
#undef TRH_CHACHA_QR

// a: ANY 256-bit word (eight u32, up to 2^256 - 1) -> a mod m in register form.  2^256 - 1 < 4 m for both moduli (m > 2^254), so three
// rounds of "subtract m if that does not borrow" end below m: after round j the value is below max(m, 4 m - j m).  fe_load takes any eight
// words (limbs < 2^30, the top one < 2^16) and fe_cond_sub's subtraction is exact for any such limbs, not only below 2 m.
template <class F> TRH_HD Fe<F> fe_reduce_u256(const u32* w) {
    Fe<F> a = fe_load<F>(w);
    fe_cond_sub(a);
    fe_cond_sub(a);
    fe_cond_sub(a);
    return a;
}

// w: sixteen little-endian u32 = lo (w[0 .. 8)) + 2^256 hi (w[8 .. 16)) -> that 512-bit value mod m, Montgomery form, fully reduced
// (pasta_curves `Fp::from_u512` / `Fq::from_u512`).
//
// THE OPERAND BOUND.  The halves are arbitrary 256-bit words, about 4 m, NOT field elements, while Fe<F> promises value < m (field.h, "register
// form") and every fe_* relies on it.  What fe_mul(a, b) itself needs is
//     (i)  limbs below 2^30, so that a column of the schoolbook product -- nine products and the reduction's terms -- stays below 2^64, and
//     (ii) a b < m 2^256, so that (a b + Q m) / 2^256 with Q < 2^256 is below 2 m and fe_mont_reduce's single conditional subtraction finishes.
// (ii) would hold for a < 2^256 against b = R^2 < m, but it would not for the SUM of two such products, and an Fe above m is one line away
// from a fe_add or fe_sub whose "a + b < 2 m" does not hold.  So nothing above m leaves fe_reduce_u256: both halves are reduced below m first,
// and from there on every operand of fe_mul and fe_add is a field element in the ordinary sense:
//     lo' = lo mod m, hi' = hi mod m                      (fe_reduce_u256: < m)
//     L  = fe_mul(lo', R^2)           = lo R              (both operands < m; result < m)
//     H  = fe_mul(fe_mul(hi', R^2), R^2) = hi R^2 = (2^256 hi) R     (each product of two values < m; results < m)
//     fe_add(L, H)                                        (< 2 m before its conditional subtraction, < m after)
// No new constant: 2^256 = R, so the high half's weight is one more multiplication by R^2.
template <class F> TRH_HD Fe<F> fe_from_u512(const u32 w[16]) {
    const Fe<F> r2 = fe_r2<F>();
    const Fe<F> lo = fe_mul(fe_reduce_u256<F>(w), r2);
    const Fe<F> hi = fe_mul(fe_mul(fe_reduce_u256<F>(w + 8), r2), r2);
    return fe_add(lo, hi);
}

// element `index` of the stream (key, stream_id): one block, one reduction
template <class F> TRH_HD Fe<F> chacha_field_element(const u32 key[8], u64 stream_id, u64 index) {
    u32 blk[16];
    chacha20_block(key, index, stream_id, blk);
    return fe_from_u512<F>(blk);
}

}  // namespace trh
