// hash_to_curve for Pallas and Vesta, one point per lane: what `Params::new(k)` of halo2_proofs 0.2.0 calls 2^k + 2 times
// (`C::hash_to_curve("Halo2-Parameters")` of pasta_curves 0.4) before its first commitment.
//
// THE FUNCTION (DESIGN.md section 3 "Params::new" restates it too; tests/hash_to_curve_model.py is the same in Python integers).
//   hash_to_field(curve_id, prefix, msg)   RFC 9380 section 5.3.1, expand_message_xmd over BLAKE2b-512 (blake2b.h; block 128 bytes, digest 64):
//       DST  = prefix || "-" || curve_id || "_XMD:BLAKE2b_SSWU_RO_",  curve_id "pallas" / "vesta";   DST' = DST || byte(len(DST))
//       b0 = H(0^128 || msg || 00 80 00 || DST'),  b1 = H(b0 || 01 || DST'),  b2 = H((b0 xor b1) || 02 || DST')
//       u_j = b_(j+1) read as a BIG-endian 512-bit integer mod the curve's base field: the 64 bytes reversed, then chacha.h's fe_from_u512
//   map_to_curve(u)   RFC 9380 section 6.6.2, simplified SWU onto the iso-curve E': y^2 = x^3 + A x + 1265 with Z = -13 (A in hashtocurve_consts.h);
//       sgn0 is the parity of the canonical value
//   iso_map           the 3-isogeny E' -> y^2 = x^3 + 5 in Velu's form, kernel abscissa x0, d = x - x0:
//                         X = (x d^2 + t d + u) / (9 d^2),   Y = y (d^3 - t d - 2 u) / (27 d^3)
//                     x0, t, u are DERIVED from A and 1265 (tests/golden/make_hashtocurve_consts.py), none is typed in
//   hash_to_curve     iso_map(swu(u0) + swu(u1)); cofactor 1; the identity is the all-zero POD
//   Params::new(k)    g[i] = hash("Halo2-Parameters")(00 || le32(i)),  w = hash(01),  u = hash(02)
// That the Rust crates use this DST layout, these message bytes and this isogeny is RECALLED: the reference holds none of this code and
// pins nothing.  RFC 7693 / RFC 9380 and the integer checks of tests/test_hashtocurve_host.py (group orders, Velu's codomain, additivity)
// pin the rest.
//
// THE MAP WITHOUT AN INVERSION.  Appendix F.2's straight-line form leaves gx1 as a fraction num / den, den = tv4^3, and asks for
// sqrt_ratio(num, den).  Here ONE chain of fieldsqrt.h runs on a = num den, and everything else is read off it:
//   * is gx1 a square?     a^T = g^e (fe_sqrt_chain): a, and so num / den = a / den^2, is a square exactly when e is even
//   * r = x g^(-(e >> 1))  squares to a for even e and to a g for odd e (g = ROOT_OF_UNITY, a non-square)
//   * the square branch    y1 = sqrt(num / den) = r / den
//   * the other branch     gx2 = Z^3 u^6 gx1, so y2 = Z u^3 sqrt(Z num / den) = Z sqrt(Z / g) u^3 r / den = THETA u^3 r / den: the same r,
//                          one constant per field and no second chain
//   * 1 / a                a w^2 = a^T = g^e, so 1 / a = w^2 g^-e: eight table products, not an exponentiation.  1 / den = num / a and
//                          1 / tv4 = tv4^2 / den follow, and the map returns an AFFINE point of E' -- which sgn0(y) needs anyway
// a = 0 would need num = 0 (den = (A tv4')^3 is never zero), a root of x^3 + A x + 1265, a point of order two; the groups have odd prime
// order, so there is none.  Every lane runs the same instructions: is_square, tv2 = 0 (u = 0 and u^2 = -1 / Z, where x1 = B / (Z A))
// and the sign are selects.
//
// THE ADDITION.  E' has A != 0 and curve.h's formulas are for a = 0, so both points go through the isogeny FIRST and are added on the target
// curve: the isogeny is a homomorphism, the results are equal.  Velu's form fits curve.h's XYZZ coordinates as it stands -- x = Xn / ZZ,
// y = Yn / ZZZ with ZZ = (3 d)^2, ZZZ = (3 d)^3 -- so iso_map costs no inversion either, xyzz_add brings its complete case analysis (u1 = -u0
// gives the identity, u1 = u0 the doubling), and the single inversion of a point is xyzz_to_affine at the end.
//
// Plain C++ for host and device, no inline assembly: the host branch serves trh_hash_to_curve and tests/native/hashtocurve_vec_test.cpp.
#pragma once
#include <string.h>

#include "blake2b.h"
#include "chacha.h"
#include "curve.h"
#include "fieldsqrt.h"
#include "hashtocurve_consts.h"

namespace trh {

constexpr size_t H2C_MAX_PREFIX = 128;
constexpr size_t H2C_MAX_DSTP = H2C_MAX_PREFIX + 1 + 6 + 21 + 1;  // prefix - curve _XMD:BLAKE2b_SSWU_RO_ len
// the words that follow a lane's own words in the three hashes, zero padded: two blocks each hold any DST' up to H2C_MAX_DSTP
constexpr int H2C_TAIL0 = 31, H2C_TAIL12 = 24;
static_assert(8 + H2C_MAX_DSTP <= 8 * (1 + H2C_TAIL0) && 64 + 1 + H2C_MAX_DSTP <= 8 * (8 + H2C_TAIL12), "the tails hold DST'");

// DST' = prefix || "-" || curve_id || "_XMD:BLAKE2b_SSWU_RO_" || len; returns its length (prefix_len <= H2C_MAX_PREFIX)
inline size_t h2c_dst_prime(bool pallas, const char* prefix, size_t prefix_len, uint8_t out[H2C_MAX_DSTP]) {
    static const char suffix[] = "_XMD:BLAKE2b_SSWU_RO_";
    size_t n = 0;
    if (prefix_len) memcpy(out, prefix, prefix_len);
    n += prefix_len;
    out[n++] = '-';
    memcpy(out + n, pallas ? "pallas" : "vesta", pallas ? 6 : 5); n += pallas ? 6 : 5;
    memcpy(out + n, suffix, sizeof(suffix) - 1); n += sizeof(suffix) - 1;
    out[n] = (uint8_t)n;
    return n + 1;
}

// What is the same for every message tag || le32(index) of one (curve, prefix, tag): a kernel argument, nothing to upload.
struct H2cPlan {
    u64 h0[8];               // the chaining value after b0's first block, 128 zero bytes
    u64 tail0[H2C_TAIL0];    // DST'                (follows the lane's word tag || le32(index) || 00 80 00)
    u64 tail1[H2C_TAIL12];   // 01 || DST'          (follows b0)
    u64 tail2[H2C_TAIL12];   // 02 || DST'          (follows b0 xor b1)
    u32 dstp_len;
    u32 tag;
};
inline void h2c_plan_build(H2cPlan& p, const uint8_t* dstp, size_t dstp_len, uint8_t tag) {
    memset(&p, 0, sizeof(p));
    blake2b_init(p.h0);
    u64 zero[16] = {0};
    blake2b_compress(p.h0, zero, BLAKE2B_BLOCK, false);
    for (size_t i = 0; i < dstp_len; ++i) {
        p.tail0[i >> 3] |= (u64)dstp[i] << (8 * (i & 7));
        p.tail1[(i + 1) >> 3] |= (u64)dstp[i] << (8 * ((i + 1) & 7));
        p.tail2[(i + 1) >> 3] |= (u64)dstp[i] << (8 * ((i + 1) & 7));
    }
    p.tail1[0] |= 1;
    p.tail2[0] |= 2;
    p.dstp_len = (u32)dstp_len;
    p.tag = tag;
}

// The end of a message: HW words of the lane's own, then tail_len bytes that every lane shares (as zero-padded words), after t0 bytes
// already compressed into h.  Any number of blocks: the block count comes from the length, the last one carries the final flag.
template <int HW, int TW> TRH_HD void h2c_absorb_final(u64 (&h)[8], const u64 (&head)[HW], const u64 (&tail)[TW], u32 tail_len, u64 t0) {
    const u32 len = 8 * HW + tail_len;
    const u32 nblk = (len + (u32)BLAKE2B_BLOCK - 1) / (u32)BLAKE2B_BLOCK;  // HW > 0: at least one
#pragma unroll 1
    for (u32 blk = 0; blk < nblk; ++blk) {
        u64 m[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const u32 pos = 16 * blk + k;  // word of the stream
            const u64 shared = pos >= HW && pos - HW < TW ? tail[pos >= HW ? pos - HW : 0] : 0;
            m[k] = k < HW && blk == 0 ? head[k < HW ? k : 0] : shared;
        }
        const bool last = blk + 1 == nblk;
        blake2b_compress(h, m, t0 + (last ? len : (u32)BLAKE2B_BLOCK * (blk + 1)), last);
    }
}

// a digest as a big-endian 512-bit integer mod m: word j of the little-endian form is the byte-swapped word 15 - j of the digest
template <class F> TRH_HD Fe<F> h2c_digest_to_field(const u64 (&d)[8]) {
    u32 w[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const u64 q = d[(15 - j) >> 1];
        w[j] = __builtin_bswap32(((15 - j) & 1) ? (u32)(q >> 32) : (u32)q);
    }
    return fe_from_u512<F>(w);
}

// hash_to_field of the message tag || le32(index)
template <class F> TRH_HD void h2c_hash_to_field_indexed(const H2cPlan& p, u32 index, Fe<F>& u0, Fe<F>& u1) {
    u64 b0[8], b[8], x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) b0[i] = p.h0[i];
    const u64 own[1] = {(u64)p.tag | (u64)index << 8 | (u64)0x80 << 48};  // msg (5 bytes) || I2OSP(128, 2) || I2OSP(0, 1)
    h2c_absorb_final<1, H2C_TAIL0>(b0, own, p.tail0, p.dstp_len, BLAKE2B_BLOCK);
    blake2b_init(b);
    h2c_absorb_final<8, H2C_TAIL12>(b, b0, p.tail1, p.dstp_len + 1, 0);
    u0 = h2c_digest_to_field<F>(b);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = b0[i] ^ b[i];
    blake2b_init(b);
    h2c_absorb_final<8, H2C_TAIL12>(b, x, p.tail2, p.dstp_len + 1, 0);
    u1 = h2c_digest_to_field<F>(b);
}

// hash_to_field of any message (host side), byte by byte as the RFC writes it
template <class F> inline void h2c_hash_to_field_bytes(const uint8_t* dstp, size_t dstp_len, const uint8_t* msg, size_t msg_len, Fe<F>& u0, Fe<F>& u1) {
    const uint8_t zeros[BLAKE2B_BLOCK] = {0}, lib[3] = {0, 128, 0}, one = 1, two = 2;
    uint8_t b0[BLAKE2B_OUT], b1[BLAKE2B_OUT], b2[BLAKE2B_OUT];
    Blake2b s0, s1, s2;
    s0.update(zeros, sizeof(zeros)); s0.update(msg, msg_len); s0.update(lib, 3); s0.update(dstp, dstp_len); s0.finish(b0);
    s1.update(b0, BLAKE2B_OUT); s1.update(&one, 1); s1.update(dstp, dstp_len); s1.finish(b1);
    for (size_t i = 0; i < BLAKE2B_OUT; ++i) b2[i] = b0[i] ^ b1[i];
    s2.update(b2, BLAKE2B_OUT); s2.update(&two, 1); s2.update(dstp, dstp_len); s2.finish(b2);
    u64 d[8];
    memcpy(d, b1, 64); u0 = h2c_digest_to_field<F>(d);
    memcpy(d, b2, 64); u1 = h2c_digest_to_field<F>(d);
}

#define TRH_H2C_CONST(F, NAME)                                                                                                      \
    fe_load<F>(H2cConsts<F>::NAME[0], H2cConsts<F>::NAME[1], H2cConsts<F>::NAME[2], H2cConsts<F>::NAME[3], H2cConsts<F>::NAME[4], \
               H2cConsts<F>::NAME[5], H2cConsts<F>::NAME[6], H2cConsts<F>::NAME[7])

template <class F> TRH_HD Fe<F> fe_select(bool c, const Fe<F>& a, const Fe<F>& b) {  // c ? a : b, limb by limb
    Fe<F> r;
#pragma unroll
    for (int i = 0; i < NLIMBS; ++i) r.l[i] = c ? a.l[i] : b.l[i];
    return r;
}
template <class F> TRH_HD u32 fe_sgn0(const Fe<F>& a) { return fe_from_mont(a).l[0] & 1u; }

// map_to_curve_simple_swu: an affine point of E' (never the identity); see "THE MAP WITHOUT AN INVERSION" above
template <class F> TRH_HD Affine<F> h2c_swu(const Fe<F>& u, const SqrtTable<F>* tab) {
    const Fe<F> A = TRH_H2C_CONST(F, A), B = TRH_H2C_CONST(F, B), Z = TRH_H2C_CONST(F, Z);
    const Fe<F> u2 = fe_sqr(u);
    const Fe<F> tv1 = fe_mul(Z, u2);
    const Fe<F> tv2 = fe_add(fe_sqr(tv1), tv1);
    const Fe<F> tv3 = fe_mul(B, fe_add(tv2, fe_one<F>()));                        // x1 = tv3 / tv4
    const Fe<F> tv4 = fe_mul(A, fe_select(fe_is_zero(tv2), Z, fe_neg(tv2)));
    const Fe<F> tv4s = fe_sqr(tv4);
    const Fe<F> den = fe_mul(tv4s, tv4);
    const Fe<F> num = fe_add(fe_mul(fe_add(fe_sqr(tv3), fe_mul(A, tv4s)), tv3), fe_mul(B, den));  // gx1 = num / den
    const SqrtChain<F> ch = fe_sqrt_chain(fe_mul(num, den), tab);
    const bool square = !(ch.e & 1u);
    const Fe<F> r = fe_mul_root_pow_neg(ch.x, ch.e >> 1, tab);
    const Fe<F> inv_den = fe_mul(num, fe_mul_root_pow_neg(fe_sqr(ch.w), ch.e, tab));
    const Fe<F> inv_tv4 = fe_mul(tv4s, inv_den);
    const Fe<F> xn = fe_select(square, tv3, fe_mul(tv1, tv3));                   // x2 = Z u^2 x1
    const Fe<F> yn = fe_select(square, r, fe_mul(fe_mul(TRH_H2C_CONST(F, THETA), fe_mul(u2, u)), r));
    Affine<F> p;
    p.x = fe_mul(xn, inv_tv4);
    p.y = fe_mul(yn, inv_den);
    p.y = fe_select(fe_sgn0(u) == fe_sgn0(p.y), p.y, fe_neg(p.y));
    return p;
}

// the 3-isogeny E' -> y^2 = x^3 + 5 into XYZZ coordinates, ZZ = (3 d)^2, ZZZ = (3 d)^3; a point of the kernel (d = 0) gives the identity
template <class F> TRH_HD XYZZ<F> h2c_iso_map(const Affine<F>& p) {
    const Fe<F> T = TRH_H2C_CONST(F, ISO_T), U = TRH_H2C_CONST(F, ISO_U);
    const Fe<F> d = fe_sub(p.x, TRH_H2C_CONST(F, ISO_X0));
    const Fe<F> d2 = fe_sqr(d), d3 = fe_mul(d2, d), td = fe_mul(T, d);
    XYZZ<F> r;
    r.x = fe_add(fe_add(fe_mul(p.x, d2), td), U);
    r.y = fe_mul(p.y, fe_sub(fe_sub(d3, td), fe_dbl(U)));
    const Fe<F> n2 = fe_add(fe_dbl(fe_dbl(fe_dbl(d2))), d2), n3 = fe_add(fe_dbl(fe_dbl(fe_dbl(d3))), d3);  // 9 d^2, 9 d^3
    r.zz = n2;
    r.zzz = fe_add(fe_dbl(n3), n3);
    return r;
}

// acc += iso_map(swu(u)).  From the identity, one step is map_to_curve and two are hash_to_curve's second half; xyzz_to_affine ends both.
template <class F> TRH_HD void h2c_accumulate(XYZZ<F>& acc, const Fe<F>& u, const SqrtTable<F>* tab) { acc = xyzz_add(acc, h2c_iso_map(h2c_swu(u, tab))); }

}  // namespace trh
