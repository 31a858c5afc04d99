// The Exe table of the reference's circuit (ExeChip::assign_trace over the trace's steps), as far as it can be said without a device: the
// decode of a packed instruction, the rule a selection table and a step must keep, the layout of the columns, and exe_row(), which yields one
// row's values and the one-hot selector of each temporary variable.  exetable.hip writes the table with them;
// tests/native/exetable_vec_test.cpp drives the same functions on the host under the address and undefined-behaviour sanitizers, against
// tests/exetable_model.py.  Further down: the chips (Out, the changed flags, the sub-chips' advice) for exechips.hip, and what the two
// entries share on the device.
//
// A step is (pc, inst, a, regs[reg_count] BEFORE the step, flag BEFORE the step, value); its successor is the next step, the zero row
// behind the last one.  inst packs the opcode in bits 0 - 4, ri in bits 8 - 11, rj in bits 12 - 15 and "operand A is a register" in bit 16;
// `a` is the immediate or the register's number.
//
// Columns, R = reg_count (columns(R) = 28 + 9 R):
//   s_trace pc flag reg[R] opcode immediate value tv_a tv_b tv_c tv_d                                          10 + R plain cells
//   sa_: pc_next reg[R] reg_next[R] a v_addr                                                                    the four selector families,
//   sb_: pc pc_next pc_plus_one reg[R] reg_next[R] a max_word                                                   each a subsequence of
//   sc_: reg[R] reg_next[R] a zero                                                                              pc pc_next pc_plus_one reg[R]
//   sd_: pc reg[R] reg_next[R] a zero one                                                                       reg_next[R] a v_addr max_word zero one
//   sa_non_det sb_non_det sc_non_det sd_non_det
// Which source a temporary variable takes is DATA: selection[opcode] holds one source per variable (include/trh.h TRH_EXE_*), byte v for
// variable v (a, b, c, d), 0xFFFFFFFF for an opcode the table does not know.  A source is legal for a variable when the variable's family
// has its selector column; UNSET (no selector, value 0) and NONDET(rule) (the family's non_det column) are legal everywhere.  Operand A
// as a source sets s?_reg[A] and takes the register's CONTENT when A is a register, s?_a and the immediate when it is not.
//
// Non-deterministic rules, as integers over RI = reg[ri], RJ = reg[rj], A = the operand's value and W = word_bits (nondet_value): all but
// SHR_LO are non-negative and below 2^33; SHR_LO = 2^s RJ - 2^W (RJ >> s) can be negative as a field element, so every value carries a
// sign next to its 64-bit magnitude.  pc + 1 and 2^W are integers: they do not wrap at 32 bits.
#pragma once
#include "../../include/trh.h"
#include "witness.h"

namespace trh {
namespace exetable {

constexpr u32 OPCODES = 32, ANSWER_OPCODE = 0x1Fu, MAX_REGS = 16;
constexpr u32 UNKNOWN_ENTRY = 0xFFFFFFFFu;
constexpr u32 NO_COLUMN = 0xFFFFFFFFu;
constexpr u32 EXE_THREADS = 256;  // rows per workgroup of the row kernel: four waves of 64 lanes, one lane per row
constexpr u32 VARS = 4;           // a, b, c, d

// ---- the instruction word --------------------------------------------------------------------------------------------------------------
TRH_HD u32 inst_opcode(u32 inst) { return inst & 31u; }
TRH_HD u32 inst_ri(u32 inst) { return (inst >> 8) & 15u; }
TRH_HD u32 inst_rj(u32 inst) { return (inst >> 12) & 15u; }
TRH_HD bool inst_a_is_reg(u32 inst) { return (inst >> 16) & 1u; }

// ---- the layout ----------------------------------------------------------------------------------------------------------------------
// the slots a selector family can have, in the order they stand in every family; REG and REG_NEXT are reg_count columns wide
enum { SLOT_PC = 0, SLOT_PC_NEXT, SLOT_PC_PLUS_ONE, SLOT_REG, SLOT_REG_NEXT, SLOT_A, SLOT_VALUE, SLOT_MAX_WORD, SLOT_ZERO, SLOT_ONE, SLOTS };
TRH_HD u32 family_slots(u32 v) {
    const u32 regs = 1u << SLOT_REG | 1u << SLOT_REG_NEXT | 1u << SLOT_A;
    return v == 0 ? regs | 1u << SLOT_PC_NEXT | 1u << SLOT_VALUE
         : v == 1 ? regs | 1u << SLOT_PC | 1u << SLOT_PC_NEXT | 1u << SLOT_PC_PLUS_ONE | 1u << SLOT_MAX_WORD
         : v == 2 ? regs | 1u << SLOT_ZERO
                  : regs | 1u << SLOT_PC | 1u << SLOT_ZERO | 1u << SLOT_ONE;
}
// the columns of family v in front of `slot` (slot = SLOTS: the family's width)
TRH_HD u32 slot_offset(u32 v, u32 slot, u32 R) {
    const u32 has = family_slots(v);
    u32 off = 0;
#pragma unroll
    for (u32 s = 0; s < SLOTS; ++s)
        if (s < slot && ((has >> s) & 1u)) off += s == SLOT_REG || s == SLOT_REG_NEXT ? R : 1u;
    return off;
}
TRH_HD u32 columns(u32 R) { return 28u + 9u * R; }
enum { COL_S_TRACE = 0, COL_PC = 1, COL_FLAG = 2, COL_REG0 = 3 };
TRH_HD u32 col_opcode(u32 R) { return 3u + R; }
TRH_HD u32 col_immediate(u32 R) { return 4u + R; }
TRH_HD u32 col_value(u32 R) { return 5u + R; }
TRH_HD u32 col_tv(u32 R, u32 v) { return 6u + R + v; }
TRH_HD u32 col_family(u32 R, u32 v) {
    u32 at = 10u + R;
#pragma unroll
    for (u32 w = 0; w < VARS; ++w)
        if (w < v) at += slot_offset(w, SLOTS, R);
    return at;
}
TRH_HD u32 col_non_det(u32 R, u32 v) { return 24u + 9u * R + v; }

// ---- the selection table ---------------------------------------------------------------------------------------------------------------
TRH_HD u32 entry_source(u32 entry, u32 v) { return (entry >> (8u * v)) & 0xFFu; }
TRH_HD bool source_is_nondet(u32 src) { return src >= (u32)TRH_EXE_NONDET; }
// the slot whose selector a deterministic source sets (SLOTS for UNSET); operand A as a register goes through SLOT_REG
TRH_HD u32 source_slot(u32 src, bool a_is_reg) {
    switch (src) {
    case TRH_EXE_PC: return SLOT_PC;
    case TRH_EXE_PC_NEXT: return SLOT_PC_NEXT;
    case TRH_EXE_PC_PLUS_ONE: return SLOT_PC_PLUS_ONE;
    case TRH_EXE_REG_RI: case TRH_EXE_REG_RJ: return SLOT_REG;
    case TRH_EXE_REG_NEXT_RI: return SLOT_REG_NEXT;
    case TRH_EXE_A: return a_is_reg ? (u32)SLOT_REG : (u32)SLOT_A;
    case TRH_EXE_VALUE: return SLOT_VALUE;
    case TRH_EXE_ZERO: return SLOT_ZERO;
    case TRH_EXE_ONE: return SLOT_ONE;
    case TRH_EXE_MAX_WORD: return SLOT_MAX_WORD;
    default: return SLOTS;
    }
}
TRH_HD bool source_ok(u32 v, u32 src) {
    if (src == (u32)TRH_EXE_UNSET) return true;
    if (source_is_nondet(src)) return src - (u32)TRH_EXE_NONDET < (u32)TRH_EXE_RULES;
    if (src > (u32)TRH_EXE_MAX_WORD) return false;
    const u32 has = family_slots(v);
    return ((has >> source_slot(src, false)) & 1u) && ((has >> source_slot(src, true)) & 1u);
}
// the first (opcode, variable) whose source is illegal, as opcode * 4 + variable; OPCODES * 4 for a good table
TRH_HD u32 table_first_bad(const u32* selection) {
    for (u32 op = 0; op < OPCODES; ++op) {
        if (selection[op] == UNKNOWN_ENTRY) continue;
        for (u32 v = 0; v < VARS; ++v)
            if (!source_ok(v, entry_source(selection[op], v))) return op * VARS + v;
    }
    return OPCODES * VARS;
}

TRH_HD bool word_bits_ok(u32 word_bits) { return word_bits >= 2 && word_bits <= 32; }
TRH_HD bool reg_count_ok(u32 R) { return R >= 1 && R <= MAX_REGS; }
TRH_HD u64 word_limit(u32 W) { return (u64)1 << W; }

// The rule of one step, as far as it shows in the step's own scalars (the registers' words are checked next to it, step_regs_ok): a known
// opcode, ri, rj and a register operand below reg_count, pc, a and value below 2^word_bits, Answer on the last step.
TRH_HD bool step_ok(u32 W, u32 R, u32 entry, u32 pc, u32 inst, u32 a, u32 value, bool last) {
    const u64 limit = word_limit(W);
    if (entry == UNKNOWN_ENTRY) return false;
    if (inst_ri(inst) >= R || inst_rj(inst) >= R || (inst_a_is_reg(inst) && a >= R)) return false;
    if ((u64)pc >= limit || (u64)a >= limit || (u64)value >= limit) return false;
    return !last || inst_opcode(inst) == ANSWER_OPCODE;
}
TRH_HD bool step_regs_ok(u32 W, u32 R, const u32* regs) {
    const u64 limit = word_limit(W);
    bool ok = true;
    for (u32 k = 0; k < R; ++k) ok = ok && (u64)regs[k] < limit;
    return ok;
}

// ---- one row ---------------------------------------------------------------------------------------------------------------------------
struct Value { u64 magnitude; bool negative; };
TRH_HD Value positive(u64 v) { Value r; r.magnitude = v; r.negative = false; return r; }

TRH_HD i64 signed_word(u32 W, u64 w) {  // the reference's Word::into_signed
    const u64 m = (u64)1 << (W - 1);
    return (i64)(w & (m - 1)) - (i64)(w & m);
}

TRH_HD Value nondet_value(u32 rule, u32 W, u64 RI, u64 RJ, u64 A, u64 pc) {
    const u64 two_w = word_limit(W), mask = two_w - 1;
    const u32 s = A < W ? (u32)A : W;  // the shifts' amount: min(A, W)
    switch (rule) {
    case TRH_EXE_RULE_REM: return positive(A == 0 ? 0u : (u32)RJ % (u32)A);  // words: a 32-bit division
    case TRH_EXE_RULE_QUOT: return positive(A == 0 ? 0u : (u32)RJ / (u32)A);
    case TRH_EXE_RULE_CMP_GT: return positive(RI > A ? two_w - (RI - A) : A - RI);
    case TRH_EXE_RULE_CMP_GE: return positive(RI >= A ? two_w - 1 - (RI - A) : A - RI - 1);
    case TRH_EXE_RULE_MUL_HI: return positive((RJ * A) >> W);
    case TRH_EXE_RULE_MUL_LO: return positive((RJ * A) & mask);
    case TRH_EXE_RULE_SMUL_LO: return positive((u64)(signed_word(W, A) * signed_word(W, RJ)) & mask);  // |product| <= 2^62
    case TRH_EXE_RULE_XOR: return positive(RI ^ A);
    case TRH_EXE_RULE_SHL_HI: return positive((RJ << s) >> W);
    case TRH_EXE_RULE_SHR_LO: {
        const u64 up = RJ << s, down = (RJ >> s) << W;  // both below 2^64: RJ < 2^W, s <= W <= 32
        Value r;
        r.negative = up < down;
        r.magnitude = r.negative ? down - up : up - down;
        return r;
    }
    default: return positive(pc + 1);  // TRH_EXE_RULE_PC_PLUS_ONE
    }
}

// what a row is made from: the step's scalars, the registers it names, and the two words of its successor a source can ask for
struct Step {
    u32 pc, inst, a, value;
    u32 reg_ri, reg_rj, reg_a;  // regs[ri], regs[rj]; regs[a] when A is a register (else unused)
    u32 pc_next, reg_next_ri;   // of the successor: 0 behind the last step
};
// a temporary variable that equals a plain cell of its own row shares that cell's conversion
enum { ALIAS_NONE = 0, ALIAS_PC, ALIAS_IMMEDIATE, ALIAS_VALUE, ALIAS_REG0 };  // ALIAS_REG0 + k: reg[k]
struct Row {
    u32 opcode, immediate;
    Value tv[VARS];
    u32 alias[VARS];  // ALIAS_*: tv[v] is that cell's word (its value is in tv[v] as well)
    u32 hot[VARS];    // the one selector column of variable v that is set, NO_COLUMN for UNSET
};

TRH_HD Row exe_row(u32 W, u32 R, u32 entry, const Step& st) {
    Row r;
    const bool a_is_reg = inst_a_is_reg(st.inst);
    const u32 ri = inst_ri(st.inst), rj = inst_rj(st.inst);
    const u64 A = a_is_reg ? st.reg_a : st.a;
    r.opcode = inst_opcode(st.inst);
    r.immediate = a_is_reg ? 0u : st.a;
#pragma unroll
    for (u32 v = 0; v < VARS; ++v) {
        const u32 src = entry_source(entry, v);
        Value val = positive(0);
        u32 alias = ALIAS_NONE, k = 0;
        switch (src) {
        case TRH_EXE_PC: val = positive(st.pc); alias = ALIAS_PC; break;
        case TRH_EXE_PC_NEXT: val = positive(st.pc_next); break;
        case TRH_EXE_PC_PLUS_ONE: val = positive((u64)st.pc + 1); break;
        case TRH_EXE_REG_RI: val = positive(st.reg_ri); k = ri; alias = ALIAS_REG0 + ri; break;
        case TRH_EXE_REG_RJ: val = positive(st.reg_rj); k = rj; alias = ALIAS_REG0 + rj; break;
        case TRH_EXE_REG_NEXT_RI: val = positive(st.reg_next_ri); k = ri; break;
        case TRH_EXE_A: val = positive(A); k = a_is_reg ? st.a : 0u; alias = a_is_reg ? ALIAS_REG0 + st.a : (u32)ALIAS_IMMEDIATE; break;
        case TRH_EXE_VALUE: val = positive(st.value); alias = ALIAS_VALUE; break;
        case TRH_EXE_ONE: val = positive(1); break;
        case TRH_EXE_MAX_WORD: val = positive(word_limit(W) - 1); break;
        default: break;  // UNSET, ZERO
        }
        u32 hot = NO_COLUMN;
        if (source_is_nondet(src)) {
            val = nondet_value(src - (u32)TRH_EXE_NONDET, W, st.reg_ri, st.reg_rj, A, st.pc);
            hot = col_non_det(R, v);
        } else {
            const u32 slot = source_slot(src, a_is_reg);
            if (slot != SLOTS) hot = col_family(R, v) + slot_offset(v, slot, R) + k;
        }
        r.tv[v] = val; r.alias[v] = alias; r.hot[v] = hot;
    }
    return r;
}


// ---- the chips: Out, the changed flags and the sub-chips' advice (trh_exe_chips_dev, csrc/exechips.hip) ----------------------------------------
// A second per-opcode table, chips[opcode] (include/trh.h TRH_CHIP_*): bits 0 - 12 the reference's Out in Out::new order, bit 13 b_flag,
// bits 14 - 16 ch_pc, ch_flag, ch_reg[ri]; 0xFFFFFFFF for an opcode the table does not know.  Columns, R = reg_count
// (chip_columns(R) = 52 + R):
//   out_* (13) | ch_reg[R] ch_pc ch_flag | the CHIP_CELLS = 37 cells below, which chip_row() yields in this order
//   a_even a_odd b_even b_odd c_even c_odd d_even d_odd | es_word es_even es_odd os_word os_even os_odd
//   sg_a_{msb sigma check check_even check_odd} sg_b_{..} sg_c_{..} | r_word r_even r_odd | a_shift a_power | a_flag | lsb_b b_flag
// A cell is computed on a row whose mask has one of the cell's enabling bits and is zero elsewhere; halves, msb, sigma and check come from
// an input that is a word (0 <= v < 2^W), else the whole group is zero.  The a_flag cell of chip_row() is the DENOMINATOR c + flag' (on
// flag2 rows): the inversion is the field's, csrc/exechips.hip does it.
// Magnitudes stay below 2^64: every value of exe_row but SHR_LO is at most 2^32, |SHR_LO| <= (2^32 - 1)^2, and two SHR_LO of one row are
// equal, so |c - a - 1| < 2^64.
enum { OUT_AND = 0, OUT_XOR, OUT_OR, OUT_SUM, OUT_PROD, OUT_SSUM, OUT_SPROD, OUT_MOD, OUT_SHIFT, OUT_FLAG1, OUT_FLAG2, OUT_FLAG3, OUT_FLAG4, OUTS };
constexpr u32 CHIP_BITS = 17;  // the bits a chips entry may set
enum { CELL_A_EVEN = 0, CELL_B_EVEN = 2, CELL_C_EVEN = 4, CELL_D_EVEN = 6, CELL_ES_WORD = 8, CELL_OS_WORD = 11, CELL_SG_A = 14, CELL_SG_B = 19, CELL_SG_C = 24,
       CELL_R_WORD = 29, CELL_A_SHIFT = 32, CELL_A_POWER = 33, CELL_A_FLAG = 34, CELL_LSB_B = 35, CELL_B_FLAG = 36, CHIP_CELLS = 37 };
TRH_HD u32 chip_columns(u32 R) { return 52u + R; }
TRH_HD u32 col_out(u32 o) { return o; }
TRH_HD u32 col_ch_reg(u32 k) { return (u32)OUTS + k; }
TRH_HD u32 col_ch_pc(u32 R) { return (u32)OUTS + R; }
TRH_HD u32 col_ch_flag(u32 R) { return (u32)OUTS + R + 1u; }
TRH_HD u32 col_cell(u32 R, u32 cell) { return (u32)OUTS + R + 2u + cell; }
TRH_HD bool chips_word_bits_ok(u32 W) { return word_bits_ok(W) && (W & 1u) == 0; }  // the signed check puts the sign at an odd bit

enum { CHIPS_BAD_BIT = 0, CHIPS_BAD_R, CHIPS_BAD_B_FLAG, CHIPS_BAD_KNOWN, CHIPS_FAULTS };
// the first opcode whose chips entry is refused, as opcode * CHIPS_FAULTS + fault; OPCODES * CHIPS_FAULTS for a good table
TRH_HD u32 chips_first_bad(const u32* selection, const u32* chips) {
    for (u32 op = 0; op < OPCODES; ++op) {
        const u32 e = chips[op];
        if ((e == UNKNOWN_ENTRY) != (selection[op] == UNKNOWN_ENTRY)) return op * CHIPS_FAULTS + CHIPS_BAD_KNOWN;
        if (e == UNKNOWN_ENTRY) continue;
        if (e >> CHIP_BITS) return op * CHIPS_FAULTS + CHIPS_BAD_BIT;
        if ((e & (u32)TRH_CHIP_FLAG3) && (e & (u32)TRH_CHIP_SHIFT)) return op * CHIPS_FAULTS + CHIPS_BAD_R;  // they share r_word, r_even, r_odd
        if ((e & (u32)TRH_CHIP_B_FLAG) && !(e & (u32)TRH_CHIP_FLAG4)) return op * CHIPS_FAULTS + CHIPS_BAD_B_FLAG;
    }
    return OPCODES * CHIPS_FAULTS;
}

TRH_HD bool is_word(u32 W, const Value& v) { return !v.negative && v.magnitude < word_limit(W); }
TRH_HD Value negated(const Value& v) { Value r; r.magnitude = v.magnitude; r.negative = !v.negative && v.magnitude != 0; return r; }
// x + y in sign and magnitude (zero is never negative); the caller keeps the magnitudes' sum below 2^64
TRH_HD Value sum_of(const Value& x, const Value& y) {
    Value r;
    if (x.negative == y.negative) { r.magnitude = x.magnitude + y.magnitude; r.negative = x.negative; return r; }
    const bool x_wins = x.magnitude >= y.magnitude;
    r.magnitude = x_wins ? x.magnitude - y.magnitude : y.magnitude - x.magnitude;
    r.negative = r.magnitude != 0 && (x_wins ? x.negative : y.negative);
    return r;
}

// the even / odd split of `v` when `on` and v is a word, else two zeros: cells at, at + 1
template <class Put>
TRH_HD void put_halves(Put& put, u32 at, bool on, u32 W, const Value& v) {
    const bool live = on && is_word(W, v);
    put(at, positive(live ? even_part(v.magnitude) : 0u));
    put(at + 1, positive(live ? odd_part(v.magnitude) : 0u));
}
// the signed word's msb, sigma = |signed(v)|, check = odd + (1 - 2 msb) 2^(W - 2) (never negative: a set msb is odd's bit W - 2) and check's
// halves: cells at .. at + 4
template <class Put>
TRH_HD void put_signed(Put& put, u32 at, bool on, u32 W, const Value& v) {
    const bool live = on && is_word(W, v);
    const u64 w = live ? v.magnitude : 0u, msb = (w >> (W - 1)) & 1u, quarter = (u64)1 << (W - 2);
    const u64 check = !live ? 0u : msb ? odd_part(w) - quarter : odd_part(w) + quarter;
    put(at, positive(msb));
    put(at + 1, positive(msb ? word_limit(W) - w : w));
    put(at + 2, positive(check));
    put(at + 3, positive(even_part(check)));
    put(at + 4, positive(odd_part(check)));
}

// One row's CHIP_CELLS cells, handed to put(cell, value) in the order of the columns, each once: the row kernel stores them as they come
// (no array of cells, which would live in scratch), chip_row() below collects them.  tv: the row's a, b, c, d as exe_row gives them;
// flag_next: the successor's flag, false behind the last step.  The CELL_A_FLAG value is the DENOMINATOR c + flag' on a flag2 row.
template <class Put>
TRH_HD void chip_cells(u32 W, u32 mask, const Value& a, const Value& b, const Value& c, const Value& d, bool flag_next, Put& put) {
    const auto has = [mask](u32 bits) { return (mask & bits) != 0; };
    const u32 logic = TRH_CHIP_AND | TRH_CHIP_XOR | TRH_CHIP_OR, signed_ops = TRH_CHIP_SSUM | TRH_CHIP_SPROD;
    put_halves(put, CELL_A_EVEN, has(TRH_CHIP_MOD | logic | signed_ops), W, a);
    put_halves(put, CELL_B_EVEN, has(TRH_CHIP_MOD | TRH_CHIP_SUM | signed_ops | TRH_CHIP_FLAG4 | logic), W, b);
    put_halves(put, CELL_C_EVEN, has(TRH_CHIP_XOR | TRH_CHIP_PROD | TRH_CHIP_SHIFT | signed_ops), W, c);
    put_halves(put, CELL_D_EVEN, has(TRH_CHIP_PROD | TRH_CHIP_SPROD), W, d);
    {  // the sums of two even-bits halves stay below 2^W
        const bool live = has(logic) && is_word(W, a) && is_word(W, b);
        const Value es = positive(live ? even_part(a.magnitude) + even_part(b.magnitude) : 0u), os = positive(live ? odd_part(a.magnitude) + odd_part(b.magnitude) : 0u);
        put(CELL_ES_WORD, es); put_halves(put, CELL_ES_WORD + 1, true, W, es);
        put(CELL_OS_WORD, os); put_halves(put, CELL_OS_WORD + 1, true, W, os);
    }
    put_signed(put, CELL_SG_A, has(signed_ops), W, a);
    put_signed(put, CELL_SG_B, has(TRH_CHIP_SPROD | TRH_CHIP_FLAG4), W, b);
    put_signed(put, CELL_SG_C, has(signed_ops), W, c);
    {  // flag3 and shift are never both set: chips_first_bad
        Value rem = positive(0);
        if (has(TRH_CHIP_FLAG3)) { if (c.magnitude != 0) rem = sum_of(sum_of(c, negated(a)), negated(positive(1))); }
        else if (has(TRH_CHIP_SHIFT) && (a.negative || a.magnitude <= W)) rem = sum_of(positive(W), negated(a));
        put(CELL_R_WORD, rem);
        put_halves(put, CELL_R_WORD + 1, true, W, rem);
    }
    // a_power = 2^min(a, W): saturated where the reference's 2u64.pow overflows; 0 for a negative a
    const bool shift = has(TRH_CHIP_SHIFT), flag4 = has(TRH_CHIP_FLAG4);
    put(CELL_A_SHIFT, positive(shift && !a.negative && a.magnitude > W ? 1u : 0u));
    put(CELL_A_POWER, positive(!shift || a.negative ? 0u : (u64)1 << (a.magnitude < W ? (u32)a.magnitude : W)));
    put(CELL_A_FLAG, has(TRH_CHIP_FLAG2) ? sum_of(c, positive(flag_next ? 1u : 0u)) : positive(0));
    put(CELL_LSB_B, positive(flag4 ? b.magnitude & 1u : 0u));
    put(CELL_B_FLAG, positive(flag4 && (mask & (u32)TRH_CHIP_B_FLAG) ? 1u : 0u));
}

struct ChipRow { Value cell[CHIP_CELLS]; };
struct ChipRowPut {
    ChipRow* row;
    u32 next;  // the cells come in the order of the columns
    TRH_HD void operator()(u32 cell, const Value& v) { if (cell == next) row->cell[next++] = v; }
};
// the same as an array (the host's form: tests/native/exechips_vec_test.cpp); `complete` is false if a cell came out of order or twice
TRH_HD ChipRow chip_row(u32 W, u32 mask, const Value* tv, bool flag_next, bool* complete) {
    ChipRow r;
    for (u32 k = 0; k < CHIP_CELLS; ++k) r.cell[k] = positive(0);
    ChipRowPut put{&r, 0u};
    chip_cells(W, mask, tv[0], tv[1], tv[2], tv[3], flag_next, put);
    *complete = put.next == CHIP_CELLS;
    return r;
}

template <class F>
TRH_HD Fe<F> fe_from_value(const Value& v) {
    const Fe<F> r = fe_from_u64<F>(v.magnitude);
    return v.negative ? fe_neg(r) : r;
}

}  // namespace exetable
}  // namespace trh

// ---- what the two entries over the steps share on the device (exetable.hip, exechips.hip) ---------------------------------------------------
#ifdef __HIPCC__
#include "ctx.h"
namespace trh {
namespace exetable {

struct StepPtrs {
    const u32 *pc, *inst, *a, *value, *regs, *flag_bits;
    size_t m;
    u32 word_bits, reg_count;
};
struct Selection { u32 e[OPCODES]; };  // a per-opcode table in a kernel's arguments: the selection, or the chips

// t.e[opcode] without an indexed read of the argument block (which would move the table to scratch): opcode < 32 always
__device__ __forceinline__ u32 entry_of(const Selection& t, u32 opcode) {
    u32 e = UNKNOWN_ENTRY;
#pragma unroll
    for (u32 o = 0; o < OPCODES; ++o) e = o == opcode ? t.e[o] : e;
    return e;
}

// the step's own scalars and what it reads of its successor (index m of no array is read); the validation has passed, so ri, rj and a
// register operand are below reg_count and every register read stays inside the step's own block
__device__ __forceinline__ Step load_step(const StepPtrs& g, size_t r) {
    const u32 R = g.reg_count, inst = g.inst[r], ri = inst_ri(inst);
    const u32* __restrict__ regs = g.regs + r * R;
    const bool has_next = r + 1 < g.m;
    Step st;
    st.pc = g.pc[r]; st.inst = inst; st.a = g.a[r]; st.value = g.value[r];
    st.reg_ri = regs[ri]; st.reg_rj = regs[inst_rj(inst)]; st.reg_a = inst_a_is_reg(inst) ? regs[st.a] : 0u;
    st.pc_next = has_next ? g.pc[r + 1] : 0u;
    st.reg_next_ri = has_next ? regs[R + ri] : 0u;
    return st;
}

// what both entries take: the step arrays, the selection and the destination (`who` names the entry in the refusals' text)
struct StepArgs {
    u32 word_bits, reg_count;
    const u32 *pc, *inst, *a, *value, *regs, *flag_bits;
    size_t m;
    const u32* selection;
    void* dst;
    size_t n;
};
int check_step_args(const char* who, int field, const StepArgs& a);
// exe_validate_kernel over the steps into a verdict of n_sums sum words and one min word, and the host's read of it -- the one
// synchronisation, before anything is written: TRH_EINVAL naming the first step that breaks a rule.  sums_dev (may be null): the sum words,
// which later kernels on s may add to
int steps_verdict(const char* who, Ctx& c, const StepPtrs& g, const Selection& t, hipStream_t s, size_t n_sums, unsigned long long** sums_dev);

}  // namespace exetable
}  // namespace trh
#endif
