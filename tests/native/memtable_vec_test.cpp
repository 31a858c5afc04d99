// csrc/memtable.h on the host, compiled with -fsanitize=address,undefined (Makefile): reads cases from stdin, one per line, and prints what
// the header's functions return; tests/test_memtable_host.py compares the lines with tests/memtable_model.py.  Never loads libtrh.
//   c                                                     SORT_TILE SCAN_TILE MEM_COLUMNS
//   p <m> <t> <n> <word_bits>                             make_plan: passes records row_cap sort_tiles hist_scan_tiles record_scan_tiles row_scan_tiles bytes,
//                                                         then "ok" when the scratch arrays lie in order, 256-byte aligned, without overlap
//   k <word_bits> <address> <time> <value> <prev_time>    record_ok: 0 or 1
//   w <word_bits> <t>                                     word_bits_ok and tape_ok: two of 0 or 1
//   r <address> <time> <init> <store> <prev_time> <prev_run_address> <carried>    derive_row: the 13 integers
// Integers are decimal.
#include <inttypes.h>
#include <stdio.h>

#include "../../tiny-ram-halo2_amd/csrc/memtable.h"

using namespace trh;
using namespace trh::memtable;

static bool layout_ok(const Plan& p) {
    const u64 off[] = {p.off_keys[0], p.off_index[0], p.off_keys[1], p.off_index[1], p.off_hist, p.off_hist_sums, p.off_place, p.off_place_sums, p.off_row_address,
                       p.off_row_time, p.off_row_value, p.off_row_source, p.off_last, p.off_last_sums, p.bytes};
    const u64 size[] = {4 * p.records, 4 * p.records, 4 * p.records, 4 * p.records, 4 * (u64)RADIX * p.sort_tiles, 4 * p.hist_scan_tiles, 4 * p.records,
                        4 * p.record_scan_tiles, 4 * p.row_cap, 4 * p.row_cap, 4 * p.row_cap, 4 * p.row_cap, 8 * p.row_cap, 8 * p.row_scan_tiles};
    if (off[0] != 0) return false;
    for (int i = 0; i < 14; ++i)
        if (off[i] % 256 != 0 || off[i] + size[i] > off[i + 1]) return false;
    return true;
}

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        char op = 0;
        unsigned long long a[7] = {0, 0, 0, 0, 0, 0, 0};
        if (sscanf(line, " p %llu %llu %llu %llu", &a[0], &a[1], &a[2], &a[3]) == 4) {
            const Plan p = make_plan(a[0], a[1], a[2], (u32)a[3]);
            printf("%u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %s\n", p.passes, p.records, p.row_cap, p.sort_tiles, p.hist_scan_tiles,
                   p.record_scan_tiles, p.row_scan_tiles, p.bytes, layout_ok(p) ? "ok" : "BAD");
        } else if (sscanf(line, " k %llu %llu %llu %llu %llu", &a[0], &a[1], &a[2], &a[3], &a[4]) == 5) {
            printf("%d\n", record_ok((u32)a[0], (u32)a[1], (u32)a[2], (u32)a[3], (u32)a[4]) ? 1 : 0);
        } else if (sscanf(line, " w %llu %llu", &a[0], &a[1]) == 2) {
            printf("%d %d\n", word_bits_ok((u32)a[0]) ? 1 : 0, word_bits_ok((u32)a[0]) && tape_ok((u32)a[0], a[1]) ? 1 : 0);
        } else if (sscanf(line, " r %llu %llu %llu %llu %llu %llu %llu", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6]) == 7) {
            const Row r = derive_row((u32)a[0], (u32)a[1], a[2] != 0, a[3] != 0, (u32)a[4], (u32)a[5], (u32)a[6]);
            for (u32 c = 0; c < MEM_COLUMNS; ++c) printf("%s%u", c ? " " : "", r.c[c]);
            printf("\n");
        } else if (sscanf(line, " %c", &op) == 1 && op == 'c') {
            printf("%u %u %u\n", SORT_TILE, SCAN_TILE, MEM_COLUMNS);
        } else if (op) {
            fprintf(stderr, "memtable_vec_test: bad line: %s", line);
            return 2;
        }
    }
    return 0;
}
