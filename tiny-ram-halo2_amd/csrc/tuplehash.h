// The set behind trh_lookup_check_dev (mockcheck.hip): exact membership of width-column tuples of field elements, as MockProver::verify asks
// of a lookup -- does the input tuple of this row occur among the table's rows.  Plain C++ for host and device: the kernels and
// tests/native/tuplehash_test.cpp run the very same hash, slot sequence, insert and probe.
//
// An open-addressing set of table ROW INDICES: `capacity` u32 slots (a power of two, at least twice the rows: load <= 1/2), EMPTY = 0xFFFFFFFF,
// linear probing from hash & (capacity - 1).  A slot is claimed once (EMPTY -> row) and never changes again.  An insert that meets an occupied
// slot compares its tuple with the occupant's: equal -> the duplicate is dropped (a padded table repeats one row thousands of times and must
// not build a chain), different -> next slot.  Elements are canonical stored words (8 x u32, 16-byte aligned) compared as they are.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TRH_TUPLE_HD __host__ __device__
#else
#define TRH_TUPLE_HD
#endif

namespace trh {
namespace tuplehash {

constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr uint32_t MAX_WIDTH = 16;

struct alignas(16) Words8 {
    uint32_t w[8];
};

TRH_TUPLE_HD inline Words8 load_elem(const void* column, size_t row) { return ((const Words8*)column)[row]; }

// the power of two at or above 2 * rows (rows >= 1)
TRH_TUPLE_HD inline uint64_t capacity_for(size_t rows) {
    uint64_t cap = 2;
    while (cap < 2 * (uint64_t)rows) cap <<= 1;
    return cap;
}

// one step of the chain: multiply-xorshift.  The multiplication carries every bit of w upwards, the shift brings the top half back down, so
// the next word meets a state that depends on all bits seen so far
TRH_TUPLE_HD inline uint64_t mix(uint64_t h, uint64_t w) {
    h = (h ^ w) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}
// the 8 * width words of row `row`, column 0 first; the two closing rounds spread the last word (tuples that differ in the top word of the
// last column only) over the low bits the slot index is taken from
TRH_TUPLE_HD inline uint64_t hash_tuple(const void* const* columns, uint32_t width, size_t row) {
    uint64_t h = 0x243F6A8885A308D3ull ^ width;
    for (uint32_t j = 0; j < width; ++j) {
        const Words8 e = load_elem(columns[j], row);
        for (int i = 0; i < 8; ++i) h = mix(h, e.w[i]);
    }
    h = (h ^ (h >> 32)) * 0xD6E8FEB86659FD93ull;
    h = (h ^ (h >> 32)) * 0xD6E8FEB86659FD93ull;
    return h ^ (h >> 32);
}
TRH_TUPLE_HD inline uint64_t slot_at(uint64_t hash, uint64_t step, uint64_t capacity) { return (hash + step) & (capacity - 1); }

TRH_TUPLE_HD inline bool tuples_equal(const void* const* a_columns, size_t a_row, const void* const* b_columns, size_t b_row, uint32_t width) {
    uint32_t diff = 0;
    for (uint32_t j = 0; j < width; ++j) {
        const Words8 a = load_elem(a_columns[j], a_row), b = load_elem(b_columns[j], b_row);
        for (int i = 0; i < 8; ++i) diff |= a.w[i] ^ b.w[i];
    }
    return diff == 0;
}

// Inserts table row `row`; returns the number of slots visited.  claim(slot, row) returns what the slot held before: EMPTY when this call
// claimed it (the device passes an atomic compare-and-swap, the sequential host a plain one).  Reading the occupant's tuple is safe while
// other inserts run: the columns are immutable inputs, complete before the first insert starts -- only the slots change.
template <class Claim>
TRH_TUPLE_HD inline uint32_t insert_row(uint32_t* slots, uint64_t capacity, const void* const* tables, uint32_t width, uint32_t row, Claim claim) {
    const uint64_t h = hash_tuple(tables, width, row);
    uint32_t visited = 0;
    for (uint64_t step = 0; step < capacity; ++step) {  // bounded by the capacity; at load <= 1/2 an EMPTY slot always comes first
        const uint32_t occupant = claim(slots + slot_at(h, step, capacity), row);
        ++visited;
        if (occupant == EMPTY) break;
        if (tuples_equal(tables, row, tables, occupant, width)) break;  // a duplicate of a row already in the set: dropped
    }
    return visited;
}

// Whether the tuple of input row `row` is in the set; *visited receives the number of slots looked at.  Runs after every insert is complete.
TRH_TUPLE_HD inline bool probe_row(const uint32_t* slots, uint64_t capacity, const void* const* inputs, const void* const* tables, uint32_t width, size_t row,
                             uint32_t* visited) {
    const uint64_t h = hash_tuple(inputs, width, row);
    uint32_t seen = 0;
    bool found = false;
    for (uint64_t step = 0; step < capacity; ++step) {
        const uint32_t occupant = slots[slot_at(h, step, capacity)];
        ++seen;
        if (occupant == EMPTY) break;
        if (tuples_equal(inputs, row, tables, occupant, width)) { found = true; break; }
    }
    *visited = seen;
    return found;
}

}  // namespace tuplehash
}  // namespace trh
