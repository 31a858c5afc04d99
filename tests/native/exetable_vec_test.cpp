// csrc/exetable.h on the host, compiled with -fsanitize=address,undefined (Makefile): reads cases from stdin, one per line, and prints what
// the header's functions return; tests/test_exetable_host.py compares the lines with tests/exetable_model.py.  Never loads libtrh.
//   l <R>                                                 columns, the four families' first columns, the first non_det column, EXE_THREADS
//   d <inst>                                              opcode ri rj a_is_reg
//   t <32 entries>                                        table_first_bad: opcode * 4 + variable, 128 for a good table
//   s <W> <R> <entry> <pc> <inst> <a> <value> <last>      step_ok: 0 or 1
//   g <W> <R> <R words>                                   step_regs_ok: 0 or 1
//   r <W> <R> <entry> <pc> <inst> <a> <value> <reg_ri> <reg_rj> <reg_a> <pc_next> <reg_next_ri>
//                                                         exe_row: opcode immediate, then per variable  sign magnitude alias hot  (hot -1: none);
//                                                         an alias that does not hold the variable's word ends the program with status 3
// Integers are decimal.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../tiny-ram-halo2_amd/csrc/exetable.h"

using namespace trh;
using namespace trh::exetable;

static bool alias_holds(const Row& r, const Step& st, u32 v) {
    const u32 alias = r.alias[v];
    const u64 word = r.tv[v].magnitude;
    if (alias == ALIAS_NONE) return true;
    if (r.tv[v].negative) return false;
    if (alias == ALIAS_PC) return word == st.pc;
    if (alias == ALIAS_IMMEDIATE) return word == r.immediate;
    if (alias == ALIAS_VALUE) return word == st.value;
    const u32 k = alias - ALIAS_REG0;
    return (k == inst_ri(st.inst) && word == st.reg_ri) || (k == inst_rj(st.inst) && word == st.reg_rj) || (inst_a_is_reg(st.inst) && k == st.a && word == st.reg_a);
}

int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        char op = 0;
        int used = 0;
        if (sscanf(line, " %c%n", &op, &used) != 1) continue;
        unsigned long long a[40];
        int count = 0;
        for (char* p = line + used; count < 40;) {
            char* end = nullptr;
            const unsigned long long x = strtoull(p, &end, 10);
            if (end == p) break;
            a[count++] = x;
            p = end;
        }
        if (op == 'l' && count == 1) {
            const u32 R = (u32)a[0];
            printf("%u %u %u %u %u %u %u\n", columns(R), col_family(R, 0), col_family(R, 1), col_family(R, 2), col_family(R, 3), col_non_det(R, 0), EXE_THREADS);
        } else if (op == 'd' && count == 1) {
            const u32 inst = (u32)a[0];
            printf("%u %u %u %d\n", inst_opcode(inst), inst_ri(inst), inst_rj(inst), inst_a_is_reg(inst) ? 1 : 0);
        } else if (op == 't' && count == 32) {
            u32 table[OPCODES];
            for (u32 o = 0; o < OPCODES; ++o) table[o] = (u32)a[o];
            printf("%u\n", table_first_bad(table));
        } else if (op == 's' && count == 8) {
            printf("%d\n", step_ok((u32)a[0], (u32)a[1], (u32)a[2], (u32)a[3], (u32)a[4], (u32)a[5], (u32)a[6], a[7] != 0) ? 1 : 0);
        } else if (op == 'g' && count >= 2 && count == 2 + (int)a[1]) {
            u32* regs = (u32*)malloc(sizeof(u32) * (size_t)a[1]);  // exactly R words: a read behind them is the sanitizer's to report
            for (u32 k = 0; k < (u32)a[1]; ++k) regs[k] = (u32)a[2 + k];
            printf("%d\n", step_regs_ok((u32)a[0], (u32)a[1], regs) ? 1 : 0);
            free(regs);
        } else if (op == 'r' && count == 12) {
            Step st;
            st.pc = (u32)a[3]; st.inst = (u32)a[4]; st.a = (u32)a[5]; st.value = (u32)a[6];
            st.reg_ri = (u32)a[7]; st.reg_rj = (u32)a[8]; st.reg_a = (u32)a[9]; st.pc_next = (u32)a[10]; st.reg_next_ri = (u32)a[11];
            const Row r = exe_row((u32)a[0], (u32)a[1], (u32)a[2], st);
            printf("%u %u", r.opcode, r.immediate);
            for (u32 v = 0; v < VARS; ++v) {
                if (!alias_holds(r, st, v)) { fprintf(stderr, "exetable_vec_test: alias %u of variable %u does not hold its word: %s", r.alias[v], v, line); return 3; }
                printf(" %d %" PRIu64 " %u %lld", r.tv[v].negative ? 1 : 0, r.tv[v].magnitude, r.alias[v], r.hot[v] == NO_COLUMN ? -1ll : (long long)r.hot[v]);
            }
            printf("\n");
        } else {
            fprintf(stderr, "exetable_vec_test: bad line: %s", line);
            return 2;
        }
    }
    return 0;
}
