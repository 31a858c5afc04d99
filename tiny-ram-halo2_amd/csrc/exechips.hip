// trh_exe_chips_dev (include/trh.h): the steps of a trace into the 52 + reg_count columns the Exe table's sub-chips read -- the Out
// selectors, the changed flags, and the advice of the logic, ssum, sprod, shift and flag2 - flag4 chips -- over csrc/exetable.h.  Every cell
// is a function of the row's a, b, c, d (exetable::exe_row, derived here again: no column of trh_exe_table_dev is read), of the successor's
// flag and of the opcode's chips entry (exetable::chip_row).
//   validate  exetable.hip's exe_validate_kernel and the host's read of its verdict (steps_verdict): the entry's one synchronisation,
//             BEFORE anything is written to the destination
//   rows      one lane owns one row, so the 64 lanes of a wave write 64 consecutive 32-byte elements of one column -- 2 KiB in one piece
//             per store pair -- and walk the columns together.  Out and changed cells are zero or the constant R mod p; every other cell is
//             converted once from chip_row's sign and magnitude (csrc/witness.h: one Montgomery multiplication, none for 0 and 1).  The
//             a_flag column receives the DENOMINATOR c + flag' on flag2 rows.  Rows m .. n - 1 are zeroed by the same kernel.  No LDS and
//             no scratch: both tables ride in the kernel's arguments and are read with chains of selects, never indexed by a lane's opcode
//   inverse   csrc/exechips_inv.h over the a_flag column: one fe_inv per strip of EXE_CHIPS_STRIP rows per lane; it counts the flag2 rows
//             it visits into the verdict's sum word, which is copied on the stream to the context (trh_stat "exechips_flag2_rows")
#include "ctx.h"
#include "devmem.h"
#include "exechips_inv.h"
#include "exetable.h"
#include "verdict.h"

namespace trh {
namespace {

using namespace exetable;

template <class F>
__global__ void __launch_bounds__(EXE_THREADS) exe_chips_rows_kernel(StepPtrs g, Selection t, Selection chips, uint4* __restrict__ dst, size_t n) {
    const u32 R = g.reg_count, ncols = chip_columns(R);
    for (size_t r = (size_t)blockIdx.x * EXE_THREADS + threadIdx.x; r < n; r += (size_t)gridDim.x * EXE_THREADS) {
        const auto cell = [=](u32 c) { return dst + 2 * ((size_t)c * n + r); };
        if (r >= g.m) {
            for (u32 c = 0; c < ncols; ++c) store_zero(cell(c));
            continue;
        }
        const Step st = load_step(g, r);
        const u32 opcode = inst_opcode(st.inst), ri = inst_ri(st.inst);
        const Row row = exe_row(g.word_bits, R, entry_of(t, opcode), st);
        const size_t next = r + 1;  // the successor's flag: 0 behind the last step (its bitmap word may not exist)
        const bool flag_next = next < g.m && ((g.flag_bits[next >> 5] >> (next & 31)) & 1u);
        const u32 mask = entry_of(chips, opcode);
        const Fe<F> one = fe_one<F>();
        const auto bit = [&](u32 c, bool set) {
            if (set) store_fe(cell(c), one);
            else store_zero(cell(c));
        };
#pragma unroll
        for (u32 o = 0; o < (u32)OUTS; ++o) bit(col_out(o), (mask >> o) & 1u);
        const bool ch_reg = (mask & (u32)TRH_CHIP_CH_REG) != 0;
        for (u32 k = 0; k < R; ++k) bit(col_ch_reg(k), ch_reg && k == ri);
        bit(col_ch_pc(R), (mask & (u32)TRH_CHIP_CH_PC) != 0);
        bit(col_ch_flag(R), (mask & (u32)TRH_CHIP_CH_FLAG) != 0);
        // every cell is stored as chip_cells yields it: one conversion each, none for 0 and 1
        const auto put = [&](u32 k, const Value& v) {
            if (v.magnitude == 0) store_zero(cell(col_cell(R, k)));
            else store_fe(cell(col_cell(R, k)), fe_from_value<F>(v));
        };
        chip_cells(g.word_bits, mask, row.tv[0], row.tv[1], row.tv[2], row.tv[3], flag_next, put);
    }
}

}  // namespace
}  // namespace trh

using namespace trh;
using namespace trh::exetable;

extern "C" {

int trh_exe_chips_dev(int field_id, trh_exe_chips_args_t* a) {
    if (!a) { set_error("exe_chips_dev: null arguments"); return TRH_EINVAL; }
    TRH_TRY(check_step_args("exe_chips_dev", field_id, StepArgs{a->word_bits, a->reg_count, a->pc, a->inst, a->a, a->value, a->regs, a->flag_bits, a->m, a->selection, a->dst, a->n}));
    if (!chips_word_bits_ok(a->word_bits)) { set_error("exe_chips_dev: word_bits %u is odd (the signed check puts the sign at an odd bit)", a->word_bits); return TRH_EINVAL; }
    const u32 bad = chips_first_bad(a->selection, a->chips);
    if (bad != OPCODES * CHIPS_FAULTS) {
        const char* const why[CHIPS_FAULTS] = {"sets a bit above 16", "sets flag3 and shift, which share r_word, r_even and r_odd", "sets b_flag (bit 13) without flag4",
                                               "and selection's entry are not both known or both unknown"};
        set_error("exe_chips_dev: chips[%u] = 0x%x %s", bad / CHIPS_FAULTS, a->chips[bad / CHIPS_FAULTS], why[bad % CHIPS_FAULTS]);
        return TRH_EINVAL;
    }
    TRH_ENTER(a->stream);
    Range range("trh_exe_chips_dev");
    Ctx& c = ctx();
    const hipStream_t s = (hipStream_t)a->stream;
    const StepPtrs g{a->pc, a->inst, a->a, a->value, a->regs, a->flag_bits, a->m, a->word_bits, a->reg_count};
    Selection t, chips;
    for (u32 o = 0; o < OPCODES; ++o) { t.e[o] = a->selection[o]; chips.e[o] = a->chips[o]; }
    TRH_TRY(c.exechips_flag2.ensure(8));  // before the verdict: nothing is allocated between the kernels

    unsigned long long* d_flag2_rows;  // the verdict's sum word: the flag2 rows the inversion kernel visits
    TRH_TRY(steps_verdict("exe_chips_dev", c, g, t, s, 1, &d_flag2_rows));
    const unsigned blocks = blocks_of(a->n, EXE_THREADS);
    uint4* const a_flag = (uint4*)a->dst + 2 * (size_t)col_cell(a->reg_count, CELL_A_FLAG) * a->n;
    with_field(field_id, [&](auto f) {
        using F = decltype(f);
        hipLaunchKernelGGL((exe_chips_rows_kernel<F>), dim3(blocks < 4096u ? blocks : 4096u), dim3(EXE_THREADS), 0, s, g, t, chips, (uint4*)a->dst, a->n);
        hipLaunchKernelGGL((exe_chips_inverse_kernel<F, EXE_CHIPS_STRIP>), dim3(exe_chips_inverse_blocks(a->m, EXE_CHIPS_STRIP)), dim3(EXE_THREADS), 0, s, a->inst, a->m, chips,
                           a_flag, d_flag2_rows);
    });
    TRH_HIP_TRY(hipGetLastError());
    TRH_HIP_TRY(hipMemcpyAsync(c.exechips_flag2.p, d_flag2_rows, 8, hipMemcpyDeviceToDevice, s));
    c.exechips_rows = a->m;
    return TRH_OK;
}

}  // extern "C"
