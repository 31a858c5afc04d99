// Witness intake, one element per lane: machine integers and flag bits into Pasta field elements, and the even-bits decomposition.
//
// What it replaces: a host that knows its trace as machine words wraps every cell in `F::from(u64)` and hands over 32 bytes per cell.  Every
// instance and advice column of the reference's circuit is a flag, a WORD_BITS-bit word or an even-bits half of a word (replay.column_classes),
// so the words and bits cross the link instead and the columns are made where they are used:
//   fe_from_u64 / fe_from_i64    the value as a field element in Montgomery form: ONE multiplication by R^2 (fe_to_mont).  The operand is
//                                (lo, hi, 0, .., 0): six of its nine limbs are zero at compile time, so the unrolled schoolbook product keeps
//                                27 of its 81 multiplications; 0 and 1 take no multiplication at all (flags stored as bytes)
//   even_part / odd_part         the two halves of the reference's even-bits decomposition (src/circuits/tables/even_bits.rs `decompose`,
//                                restated): both have bits at even positions only and  even + 2 odd = w
//   spread_bits                  row i of the even-bits table: bit j of i moves to position 2 j
// Plain C++ for host and device, no inline assembly beyond what fe_mul brings: the host branch serves the stand-alone sanitizer program
// (tests/native/witness_vec_test.cpp).
#pragma once
#include "field.h"

namespace trh {

typedef int64_t i64;

constexpr u64 EVEN_BITS_MASK = 0x5555555555555555ull;

template <class F> TRH_HD Fe<F> fe_from_u64(u64 v) {
    if (v == 0) return fe_zero<F>();
    if (v == 1) return fe_one<F>();
    return fe_to_mont(fe_load<F>((u32)v, (u32)(v >> 32), 0u, 0u, 0u, 0u, 0u, 0u));
}

// v < 0: m - |v|.  The magnitude is formed in the unsigned type, where 0 - 2^63 = 2^63 (negating INT64_MIN as an i64 is undefined)
template <class F> TRH_HD Fe<F> fe_from_i64(i64 v) {
    const bool negative = v < 0;
    const u64 magnitude = negative ? (u64)0 - (u64)v : (u64)v;
    const Fe<F> r = fe_from_u64<F>(magnitude);
    return negative ? fe_neg(r) : r;
}

TRH_HD u64 even_part(u64 w) { return w & EVEN_BITS_MASK; }
TRH_HD u64 odd_part(u64 w) { return (w & ~EVEN_BITS_MASK) >> 1; }

// sum_j bit_j(i) 4^j: the sixteen-bit halves are spread by the usual doubling steps
TRH_HD u64 spread_bits(u32 i) {
    u64 x = i;
    x = (x | (x << 16)) & 0x0000ffff0000ffffull;
    x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
    x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & EVEN_BITS_MASK;
    return x;
}

}  // namespace trh
