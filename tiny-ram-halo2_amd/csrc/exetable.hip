// trh_exe_table_dev (include/trh.h): the steps of a trace into the 28 + 9 reg_count columns of the Exe table -- the plain trace cells, the
// four temporary variables with their non-deterministic advice, and their one-hot selectors -- over csrc/exetable.h.  Every row is a
// function of its step and the step behind it, so there is nothing to sort or scan: two kernels, one lane per step.
//   validate  exetable::step_ok and step_regs_ok on every step, atomicMin of the first index that breaks them into a verdict of one min
//             word (verdict.h).  The host reads it (the entry's one synchronisation) BEFORE anything is written to the destination
//   rows      one lane owns one row, so the 64 lanes of a wave write 64 consecutive 32-byte elements of one column -- 2 KiB in one piece
//             per store pair -- and walk the columns together.  exe_row gives the row's integers; each distinct word of the row is
//             converted once (csrc/witness.h: one Montgomery multiplication, none for 0 and 1): a temporary variable that equals pc, a
//             register, the immediate or the value of its own row is stored from that cell's conversion.  A selector cell is zero or the
//             constant R mod p, chosen by comparing the column's index with the four one-hot indices of the row.  Rows m .. n - 1 are
//             zeroed by the same kernel.  No LDS and no scratch: the selection table rides in the kernel's arguments and is read with a
//             chain of selects, never indexed by a lane's opcode.
#include "ctx.h"
#include "devmem.h"
#include "exetable.h"
#include "verdict.h"

namespace trh {
namespace {

using namespace exetable;

__global__ void __launch_bounds__(EXE_THREADS) exe_validate_kernel(StepPtrs g, Selection t, unsigned long long* __restrict__ first_bad) {
    const size_t i = (size_t)blockIdx.x * EXE_THREADS + threadIdx.x;
    if (i >= g.m) return;
    const u32 inst = g.inst[i];
    const bool ok = step_ok(g.word_bits, g.reg_count, entry_of(t, inst_opcode(inst)), g.pc[i], inst, g.a[i], g.value[i], i + 1 == g.m) &&
                    step_regs_ok(g.word_bits, g.reg_count, g.regs + i * g.reg_count);
    if (!ok) atomicMin(first_bad, (unsigned long long)i);
}

// the validation has passed: ri, rj and a register operand are below reg_count, so every register read stays inside the step's own block
template <class F>
__global__ void __launch_bounds__(EXE_THREADS) exe_rows_kernel(StepPtrs g, Selection t, uint4* __restrict__ dst, size_t n) {
    const u32 R = g.reg_count, ncols = columns(R);
    for (size_t r = (size_t)blockIdx.x * EXE_THREADS + threadIdx.x; r < n; r += (size_t)gridDim.x * EXE_THREADS) {
        const auto cell = [=](u32 c) { return dst + 2 * ((size_t)c * n + r); };
        if (r >= g.m) {
            for (u32 c = 0; c < ncols; ++c) store_zero(cell(c));
            continue;
        }
        const Step st = load_step(g, r);
        const u32 inst = st.inst;
        const u32* __restrict__ regs = g.regs + r * R;
        const Row row = exe_row(g.word_bits, R, entry_of(t, inst_opcode(inst)), st);
        const Fe<F> one = fe_one<F>();

        // a plain cell, and every temporary variable that is the same word
        const auto plain = [&](u32 c, u32 word, u32 alias) {
            const Fe<F> fe = fe_from_u64<F>((u64)word);
            store_fe(cell(c), fe);
#pragma unroll
            for (u32 v = 0; v < VARS; ++v)
                if (row.alias[v] == alias) store_fe(cell(col_tv(R, v)), fe);
        };
        store_fe(cell(COL_S_TRACE), one);
        plain(COL_PC, st.pc, ALIAS_PC);
        if ((g.flag_bits[r >> 5] >> (r & 31)) & 1u) store_fe(cell(COL_FLAG), one);
        else store_zero(cell(COL_FLAG));
        for (u32 k = 0; k < R; ++k) plain(COL_REG0 + k, regs[k], ALIAS_REG0 + k);
        store_fe(cell(col_opcode(R)), fe_from_u64<F>((u64)row.opcode));
        plain(col_immediate(R), row.immediate, ALIAS_IMMEDIATE);
        plain(col_value(R), st.value, ALIAS_VALUE);
#pragma unroll
        for (u32 v = 0; v < VARS; ++v)
            if (row.alias[v] == ALIAS_NONE) store_fe(cell(col_tv(R, v)), fe_from_value<F>(row.tv[v]));
        for (u32 c = col_family(R, 0); c < ncols; ++c) {
            if (c == row.hot[0] || c == row.hot[1] || c == row.hot[2] || c == row.hot[3]) store_fe(cell(c), one);
            else store_zero(cell(c));
        }
    }
}

}  // namespace
}  // namespace trh

using namespace trh;

namespace trh {
namespace exetable {

int check_step_args(const char* who, int field, const StepArgs& a) {
    TRH_TRY(check_field(field));
    if (!word_bits_ok(a.word_bits)) { set_error("%s: word_bits %u outside 2 .. 32", who, a.word_bits); return TRH_EINVAL; }
    if (!reg_count_ok(a.reg_count)) { set_error("%s: reg_count %u outside 1 .. %u", who, a.reg_count, MAX_REGS); return TRH_EINVAL; }
    const u32 bad = table_first_bad(a.selection);
    if (bad != OPCODES * VARS) {
        set_error("%s: selection[%u] gives variable %c the source %u, for which it has no selector column", who, bad / VARS, "abcd"[bad % VARS],
                  entry_source(a.selection[bad / VARS], bad % VARS));
        return TRH_EINVAL;
    }
    if (a.m == 0 || a.m >= a.n) { set_error("%s: %zu steps do not fit columns of %zu rows (1 <= m < n: the row behind the trace closes it)", who, a.m, a.n); return TRH_EINVAL; }
    if (a.n >= ((u64)1 << 32)) { set_error("%s: n out of range", who); return TRH_EINVAL; }
    if (!a.dst || ((uintptr_t)a.dst & 15) != 0) { set_error("%s: dst must be a 16-byte aligned device pointer", who); return TRH_EINVAL; }
    if (!a.pc || !a.inst || !a.a || !a.value || !a.regs || !a.flag_bits) { set_error("%s: null step array", who); return TRH_EINVAL; }
    if ((((uintptr_t)a.pc | (uintptr_t)a.inst | (uintptr_t)a.a | (uintptr_t)a.value | (uintptr_t)a.regs | (uintptr_t)a.flag_bits) & 3) != 0) {
        set_error("%s: the word arrays must be 4-byte aligned", who);
        return TRH_EINVAL;
    }
    return TRH_OK;
}

int steps_verdict(const char* who, Ctx& c, const StepPtrs& g, const Selection& t, hipStream_t s, size_t n_sums, unsigned long long** sums_dev) {
    unsigned long long* d_first_bad;  // the verdict: the smallest step index that breaks a rule
    TRH_TRY(verdict_begin(c, n_sums, 1, s, sums_dev, &d_first_bad));
    hipLaunchKernelGGL(exe_validate_kernel, dim3(blocks_of(g.m, EXE_THREADS)), dim3(EXE_THREADS), 0, s, g, t, d_first_bad);
    TRH_HIP_TRY(hipGetLastError());
    // the one synchronisation: the verdict on the steps, before the destination is touched
    const u64* min;
    TRH_TRY(verdict_read(c, s, nullptr, &min));
    if (lowered(min[0])) {
        set_error("%s: step %llu breaks the table's rules (an opcode the selection knows, ri, rj and a register operand below %u, pc, a, registers and value "
                  "below 2^%u, Answer on the last step)", who, (unsigned long long)min[0], g.reg_count, g.word_bits);
        return TRH_EINVAL;
    }
    return TRH_OK;
}

}  // namespace exetable
}  // namespace trh

using namespace trh::exetable;

extern "C" {

int trh_exe_table_dev(int field_id, trh_exe_table_args_t* a) {
    if (!a) { set_error("exe_table_dev: null arguments"); return TRH_EINVAL; }
    TRH_TRY(check_step_args("exe_table_dev", field_id, StepArgs{a->word_bits, a->reg_count, a->pc, a->inst, a->a, a->value, a->regs, a->flag_bits, a->m, a->selection, a->dst, a->n}));
    TRH_ENTER(a->stream);
    Range range("trh_exe_table_dev");
    Ctx& c = ctx();
    const hipStream_t s = (hipStream_t)a->stream;
    const StepPtrs g{a->pc, a->inst, a->a, a->value, a->regs, a->flag_bits, a->m, a->word_bits, a->reg_count};
    Selection t;
    for (u32 o = 0; o < OPCODES; ++o) t.e[o] = a->selection[o];
    TRH_TRY(steps_verdict("exe_table_dev", c, g, t, s, 0, nullptr));
    const unsigned blocks = blocks_of(a->n, EXE_THREADS);
    with_field(field_id, [&](auto f) {
        hipLaunchKernelGGL((exe_rows_kernel<decltype(f)>), dim3(blocks < 4096u ? blocks : 4096u), dim3(EXE_THREADS), 0, s, g, t, (uint4*)a->dst, a->n);
    });
    TRH_HIP_TRY(hipGetLastError());
    c.exetable_rows = a->m;
    return TRH_OK;
}

}  // extern "C"
