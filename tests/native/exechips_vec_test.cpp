// The chips part of csrc/exetable.h on the host, compiled with -fsanitize=address,undefined (Makefile): reads cases from stdin, one per
// line, and prints what the header's functions return; tests/test_exechips_host.py compares the lines with tests/exechips_model.py.  Never
// loads libtrh.
//   l <R>                                                  chip_columns, the columns of ch_reg0, ch_pc, ch_flag, a_even and a_flag, CHIP_CELLS,
//                                                          whether W = 2, 3, 32, 34 are word sizes the chips take
//   t <32 selection entries> <32 chips entries>            chips_first_bad: opcode * 4 + fault, 128 for a good pair
//   c <W> <mask> <a> <b> <c> <d> <flag_next>               chip_row: the CHIP_CELLS cells as  sign magnitude; a .. d are  sign magnitude  pairs;
//                                                          cells out of order, or a negative zero, end the program with status 3
// Integers are decimal.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../tiny-ram-halo2_amd/csrc/exetable.h"

using namespace trh;
using namespace trh::exetable;

int main() {
    static char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        char op = 0;
        int used = 0;
        if (sscanf(line, " %c%n", &op, &used) != 1) continue;
        unsigned long long a[64];
        int count = 0;
        for (char* p = line + used; count < 64;) {
            char* end = nullptr;
            const unsigned long long x = strtoull(p, &end, 10);
            if (end == p) break;
            a[count++] = x;
            p = end;
        }
        if (op == 'l' && count == 1) {
            const u32 R = (u32)a[0];
            printf("%u %u %u %u %u %u %u %d %d %d %d\n", chip_columns(R), col_ch_reg(0), col_ch_pc(R), col_ch_flag(R), col_cell(R, CELL_A_EVEN), col_cell(R, CELL_A_FLAG),
                   (u32)CHIP_CELLS, chips_word_bits_ok(2) ? 1 : 0, chips_word_bits_ok(3) ? 1 : 0, chips_word_bits_ok(32) ? 1 : 0, chips_word_bits_ok(34) ? 1 : 0);
        } else if (op == 't' && count == 64) {
            u32* tables = (u32*)malloc(sizeof(u32) * 64);  // exactly 2 x 32 words: a read behind them is the sanitizer's to report
            for (u32 o = 0; o < 64; ++o) tables[o] = (u32)a[o];
            printf("%u\n", chips_first_bad(tables, tables + OPCODES));
            free(tables);
        } else if (op == 'c' && count == 11) {
            Value tv[VARS];
            for (u32 v = 0; v < VARS; ++v) { tv[v].negative = a[2 + 2 * v] != 0; tv[v].magnitude = a[3 + 2 * v]; }
            bool complete = false;
            const ChipRow r = chip_row((u32)a[0], (u32)a[1], tv, a[10] != 0, &complete);
            if (!complete) { fprintf(stderr, "exechips_vec_test: the cells did not come in the order of the columns, each once: %s", line); return 3; }
            for (u32 k = 0; k < CHIP_CELLS; ++k) {
                if (r.cell[k].negative && r.cell[k].magnitude == 0) { fprintf(stderr, "exechips_vec_test: cell %u is a negative zero: %s", k, line); return 3; }
                printf("%s%d %" PRIu64, k ? " " : "", r.cell[k].negative ? 1 : 0, r.cell[k].magnitude);
            }
            printf("\n");
        } else {
            fprintf(stderr, "exechips_vec_test: bad line: %s", line);
            return 2;
        }
    }
    return 0;
}
