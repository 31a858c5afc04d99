// The Exe table of the reference's circuit (ExeChip::assign_trace over the trace's steps), as far as it can be said without a device: the
// decode of a packed instruction, the rule a selection table and a step must keep, the layout of the columns, and exe_row(), which yields one
// row's values and the one-hot selector of each temporary variable.  exetable.hip writes the table with them;
// tests/native/exetable_vec_test.cpp drives the same functions on the host under the address and undefined-behaviour sanitizers, against
// tests/exetable_model.py.
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

}  // namespace exetable
}  // namespace trh
