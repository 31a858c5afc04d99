// The memory-consistency table of the reference's circuit (its Mem chip over the trace's access log), as far as it can be said without a
// device: the plan of trh_mem_table_dev's launches and scratch, the rule a log record must keep, and the thirteen small integers of one
// row.  memtable.hip builds the table with them; tests/native/memtable_vec_test.cpp drives the same functions on the host under the
// address and undefined-behaviour sanitizers, against tests/memtable_model.py.
//
// The table: the accesses (address, time, value, store?) grouped by address, runs in ascending address order, every run opened by an Init
// row (time 0; the tape word that lives at the address, or 0) and followed by its accesses in time order.  Tape word i lives at address
// i * word_bits / 8, and every tape address has a run whether it is accessed or not.  rows = #runs + m.
//
// Columns, in this order (MEM_COLUMNS):
//   s_trace  address  time  init  store  load  value  addr_inc  time_inc  addr_inc_even  addr_inc_odd  time_inc_even  time_inc_odd
//   value      the value of the latest Init or Store row at or above the row, inside its run (a load's own claimed value is only compared)
//   addr_inc   max(address - address of the previous run - 1, 0), the same on every row of a run; the first run measures from 0
//   time_inc   time - time of the previous row of the run; 0 on the Init row
// All arithmetic is on unsigned 32-bit words: address 0xFFFFFFFF next to address 0 and times up to 2^32 - 1 are ordinary inputs.
#pragma once
#include "witness.h"

namespace trh {
namespace memtable {

constexpr u32 MEM_COLUMNS = 13;
enum { COL_S_TRACE = 0, COL_ADDRESS, COL_TIME, COL_INIT, COL_STORE, COL_LOAD, COL_VALUE, COL_ADDR_INC, COL_TIME_INC, COL_ADDR_INC_EVEN, COL_ADDR_INC_ODD,
       COL_TIME_INC_EVEN, COL_TIME_INC_ODD };

constexpr u32 RADIX_BITS = 8;
constexpr u32 RADIX = 1u << RADIX_BITS;
constexpr u32 MEM_THREADS = 256;                       // four waves of 64 lanes
constexpr u32 SORT_ITEMS = 8, SCAN_ITEMS = 4;          // records per lane of a sort tile, elements per lane of a scan tile
constexpr u32 SORT_TILE = MEM_THREADS * SORT_ITEMS;    // 2048 records: one workgroup's histogram and its stable ranks
constexpr u32 SCAN_TILE = MEM_THREADS * SCAN_ITEMS;    // 1024 elements: one workgroup's scan; the tile sums are scanned by one more workgroup
constexpr u32 NO_SOURCE = 0xFFFFFFFFu;                 // src_index of an Init row
// the entry counts records and rows in 32-bit words; rows <= t + 2 m
constexpr u64 MAX_RECORDS = (u64)1 << 31;

TRH_HD bool word_bits_ok(u32 word_bits) { return word_bits >= 2 && word_bits <= 32 && (word_bits & 1) == 0; }
// a tape of t words needs byte-sized words and addresses below 2^word_bits
TRH_HD bool tape_ok(u32 word_bits, u64 t) {
    if (t == 0) return true;
    if (word_bits % 8 != 0) return false;
    return (t - 1) * (word_bits / 8) < ((u64)1 << word_bits);
}
TRH_HD u32 tape_address(u32 word_bits, u64 i) { return (u32)(i * (word_bits / 8)); }

// The rule of one log record: address, time and value below 2^word_bits, and time above the time of the record before it (prev_time = 0 for
// the first record, so its time is at least 1).  The entry refuses the log at the smallest index that breaks it.
TRH_HD bool record_ok(u32 word_bits, u32 address, u32 time, u32 value, u32 prev_time) {
    const u64 limit = (u64)1 << word_bits;
    return (u64)address < limit && (u64)time < limit && (u64)value < limit && time > prev_time;
}

struct Row { u32 c[MEM_COLUMNS]; };
// One row from its own fields and what the scans carry to it: prev_time is the time of the row above (read only when the row is no Init),
// prev_run_address the address of the run before this one (0 for the first run), carried the value of the latest Init or Store row at or
// above this row.
TRH_HD Row derive_row(u32 address, u32 time, bool init, bool store, u32 prev_time, u32 prev_run_address, u32 carried) {
    Row r;
    const u32 addr_inc = address > prev_run_address ? address - prev_run_address - 1u : 0u;
    const u32 time_inc = init ? 0u : time - prev_time;
    r.c[COL_S_TRACE] = 1u;
    r.c[COL_ADDRESS] = address;
    r.c[COL_TIME] = init ? 0u : time;
    r.c[COL_INIT] = init ? 1u : 0u;
    r.c[COL_STORE] = !init && store ? 1u : 0u;
    r.c[COL_LOAD] = !init && !store ? 1u : 0u;
    r.c[COL_VALUE] = carried;
    r.c[COL_ADDR_INC] = addr_inc;
    r.c[COL_TIME_INC] = time_inc;
    r.c[COL_ADDR_INC_EVEN] = (u32)even_part(addr_inc);
    r.c[COL_ADDR_INC_ODD] = (u32)odd_part(addr_inc);
    r.c[COL_TIME_INC_EVEN] = (u32)even_part(time_inc);
    r.c[COL_TIME_INC_ODD] = (u32)odd_part(time_inc);
    return r;
}

TRH_HD u64 tiles_of(u64 count, u32 tile) { return (count + tile - 1) / tile; }

// What one call launches and where its scratch lies: one block of the device pool, every array 256-byte aligned, offsets in bytes.
//   records   t + m: the tape words ahead of the log
//   row_cap   the rows the call may write: min(t + 2 m, n) -- a log whose table is longer than max_rows <= n is refused before the row arrays
//             are touched
struct Plan {
    u32 passes;            // ceil(word_bits / 8) passes of the stable LSD radix sort
    u64 records, row_cap;
    u64 sort_tiles;        // tiles of SORT_TILE records; the histogram is RADIX x sort_tiles counters, digit-major
    u64 hist_scan_tiles;   // tiles of SCAN_TILE counters of the histogram's scan
    u64 record_scan_tiles; // tiles of SCAN_TILE records of the scan that places the synthesized Init rows
    u64 row_scan_tiles;    // tiles of SCAN_TILE rows of the max-scan
    u64 off_keys[2], off_index[2];        // records x u32 each: the sort's ping-pong pairs
    u64 off_hist, off_hist_sums;          // RADIX x sort_tiles, hist_scan_tiles x u32
    u64 off_place, off_place_sums;        // records, record_scan_tiles x u32
    u64 off_row_address, off_row_time, off_row_value, off_row_source;  // row_cap x u32 each
    u64 off_last, off_last_sums;          // row_cap, row_scan_tiles x (u32, u32)
    u64 bytes;
};

TRH_HD Plan make_plan(u64 m, u64 t, u64 n, u32 word_bits) {
    Plan p;
    p.passes = (word_bits + RADIX_BITS - 1) / RADIX_BITS;
    p.records = m + t;
    p.row_cap = p.records + m < n ? p.records + m : n;
    p.sort_tiles = tiles_of(p.records, SORT_TILE);
    p.hist_scan_tiles = tiles_of((u64)RADIX * p.sort_tiles, SCAN_TILE);
    p.record_scan_tiles = tiles_of(p.records, SCAN_TILE);
    p.row_scan_tiles = tiles_of(p.row_cap, SCAN_TILE);
    u64 at = 0;
    auto take = [&at](u64 bytes) { const u64 here = at; at += (bytes + 255) / 256 * 256; return here; };
    for (int b = 0; b < 2; ++b) { p.off_keys[b] = take(4 * p.records); p.off_index[b] = take(4 * p.records); }
    p.off_hist = take(4 * RADIX * p.sort_tiles);
    p.off_hist_sums = take(4 * p.hist_scan_tiles);
    p.off_place = take(4 * p.records);
    p.off_place_sums = take(4 * p.record_scan_tiles);
    p.off_row_address = take(4 * p.row_cap);
    p.off_row_time = take(4 * p.row_cap);
    p.off_row_value = take(4 * p.row_cap);
    p.off_row_source = take(4 * p.row_cap);
    p.off_last = take(8 * p.row_cap);
    p.off_last_sums = take(8 * p.row_scan_tiles);
    p.bytes = at;
    return p;
}

}  // namespace memtable
}  // namespace trh
