// The a_flag column of trh_exe_chips_dev: the one field inversion of the Exe chips, over a column that the row kernel has filled with the
// denominators c + flag' (zero off the flag2 rows and behind the trace).  A kernel of its own, because a per-lane fe_inv is 255 squarings and
// ~250 multiplications next to a row kernel whose whole arithmetic is some forty.
//
// Lane t of a workgroup takes rows base + t + EXE_THREADS j, j < B (base = blockIdx.x EXE_THREADS B): every load and store of a wave is 64
// consecutive elements, 2 KiB in one piece.  It multiplies the non-zero denominators of its strip together, inverts the product once and
// unwinds the inverses (Montgomery's trick): 3 (B - 1) multiplications and one fe_inv for up to B inverses; zeros are skipped in the product
// and stay zero.  Which rows carry flag2 comes from the instruction word and the chips table (a chain of selects, as in the row kernel), so
// rows without it are neither loaded nor stored, and the rows that carry it are counted into a verdict sum word.
// B is a template parameter so that tools/exechips_inv_probe.hip can time B = 1, 4 and 8 from this one definition; the library instantiates
// EXE_CHIPS_STRIP alone (profiles/exechips_probe.txt has the three).  No LDS, no scratch: the strip's B denominators and B - 1 prefix
// products live in registers (every loop below is unrolled, every index a constant).
#pragma once
#include "devmem.h"
#include "exetable.h"

namespace trh {
namespace exetable {

// rows per lane of the inversion kernel.  Measured (profiles/exechips_probe.txt): at k = 18 strips of 4 and 8 both take one fe_inv's latency
// (0.199 and 0.191 ms: the grid is one wave per SIMD or less), a plain fe_inv per row three times that (0.617 ms); at k = 20 and 22 a strip
// of 8 is 1.8 times faster than one of 4
constexpr u32 EXE_CHIPS_STRIP = 8;

template <class F, u32 B>
__global__ void __launch_bounds__(EXE_THREADS) exe_chips_inverse_kernel(const u32* __restrict__ inst, size_t m, Selection chips, uint4* __restrict__ column,
                                                                        unsigned long long* __restrict__ flag2_rows) {
    const size_t base = (size_t)blockIdx.x * (EXE_THREADS * B) + threadIdx.x;
    Fe<F> x[B], before[B];  // before[j]: the product of the non-zero x[0 .. j - 1]
    bool live[B];           // a flag2 row with a non-zero denominator
    bool any = false;
    u32 counted = 0;
    Fe<F> product = fe_one<F>();
#pragma clang loop unroll(full)
    for (u32 j = 0; j < B; ++j) {
        const size_t row = base + (size_t)EXE_THREADS * j;
        const bool flag2 = row < m && (entry_of(chips, inst_opcode(inst[row < m ? row : 0])) & (u32)TRH_CHIP_FLAG2) != 0;
        counted += (u32)__popcll(__ballot(flag2));
        x[j] = fe_zero<F>();
        if (flag2) x[j] = load_fe<F>(column + 2 * row);
        live[j] = flag2 && !fe_is_zero(x[j]);
        any = any || live[j];
        before[j] = product;
        if (B > 1 && live[j]) product = fe_mul(product, x[j]);
    }
    if ((threadIdx.x & 63) == 0 && counted) atomicAdd(flag2_rows, (unsigned long long)counted);
    if (!any) return;  // nothing to invert in this strip: a wave without a live lane skips the inversion altogether
    if (B == 1) {
        if (live[0]) store_fe(column + 2 * base, fe_inv(x[0]));
        return;
    }
    Fe<F> inverse = fe_inv(product);  // of the product of the strip's live denominators; 1 for a strip without one
#pragma clang loop unroll(full)
    for (u32 k = 0; k < B; ++k) {
        const u32 j = B - 1 - k;
        if (live[j]) {
            store_fe(column + 2 * (base + (size_t)EXE_THREADS * j), fe_mul(inverse, before[j]));
            inverse = fe_mul(inverse, x[j]);
        }
    }
}

inline unsigned exe_chips_inverse_blocks(size_t m, u32 strip) { return (unsigned)((m + (size_t)EXE_THREADS * strip - 1) / ((size_t)EXE_THREADS * strip)); }

}  // namespace exetable
}  // namespace trh
