// trh_mem_table_dev (include/trh.h): the access log of a trace into the thirteen columns of the memory-consistency table, over
// csrc/memtable.h.  It is the one table of the reference's circuit whose rows are no per-row function of the trace: the accesses have to be
// grouped by address, every group opened by an Init row, and the stored value carried down each group.  The pipeline, all on the device:
//   keys      one lane per record: the tape words' addresses ahead of the log's, the rule of memtable::record_ok on every log record
//             (atomicMin of the first index that breaks it)
//   sort      ceil(word_bits / 8) passes of a stable LSD radix sort of (address, record index): per pass a histogram per tile of SORT_TILE
//             records, an exclusive scan of the digit-major counters, and a scatter whose in-tile ranks come from wave ballots -- the order
//             of equal digits is the order of the records, which is what keeps time order inside a run (time is never sorted on)
//   place     head flags of the sorted addresses; a run whose first record is no tape word needs a synthesized Init row, and the exclusive
//             sum scan of those flags says how far every record moves down.  Its total gives rows = records + synthesized, BEFORE anything
//             is written to the destination (first host synchronisation)
//   rows      the records and the synthesized Init rows scattered into row order (address, time, own value, log index)
//   last      ONE inclusive max-scan over row indices of a pair: the latest Init row, the latest Init or Store row.  Every run opens on an
//             Init row, so a plain scan needs no segment flags; the pair yields the carried value and the previous run's address
//   columns   one lane per row: memtable::derive_row, thirteen conversions (csrc/witness.h) and 26 sixteen-byte stores, a wave writing
//             2 KiB of each column in one piece; inconsistent loads counted (atomicAdd) and the first one named (atomicMin); rows behind
//             the table zeroed.  The verdict is read back with the scratch's return to the pool (second host synchronisation)
// What the host reads is ONE verdict (verdict.h) in the context: sums {rows that place adds, inconsistent loads}, mins {first bad record, first inconsistent load}.
// Scans are multi-tile in the manner of lookup.hip's scan_tiles_kernel / scan_sums_kernel: a scan per tile, one workgroup over the tile
// sums, and the consumer adds its tile's offset.  Tiles are sized for wave64: 256 lanes, 4 KiB (sort) and 1 - 2 KiB (scan) of the LDS.
#include "ctx.h"
#include "devmem.h"
#include "memtable.h"
#include "verdict.h"

namespace trh {
namespace {

using namespace memtable;

struct OpAdd {
    typedef u32 T;
    static __device__ __forceinline__ T id() { return 0u; }
    static __device__ __forceinline__ T op(T a, T b) { return a + b; }
};
struct OpMaxPair {
    typedef uint2 T;
    static __device__ __forceinline__ T id() { return make_uint2(0u, 0u); }
    static __device__ __forceinline__ T op(T a, T b) { return make_uint2(a.x > b.x ? a.x : b.x, a.y > b.y ? a.y : b.y); }
};

// inclusive Hillis-Steele scan of one value per lane of the workgroup, in sh[MEM_THREADS]; returns the exclusive prefix of this lane
template <class OP>
__device__ __forceinline__ typename OP::T block_scan(typename OP::T* sh, typename OP::T mine, typename OP::T& total) {
    typedef typename OP::T T;
    const u32 t = threadIdx.x;
    sh[t] = mine;
    __syncthreads();
    for (u32 off = 1; off < MEM_THREADS; off <<= 1) {
        const T v = t >= off ? sh[t - off] : OP::id();
        __syncthreads();
        sh[t] = OP::op(v, sh[t]);
        __syncthreads();
    }
    total = sh[MEM_THREADS - 1];
    const T before = t ? sh[t - 1] : OP::id();
    __syncthreads();
    return before;
}

// One tile of a scan.  LOAD(i) gives element i < count; out[i] takes the tile-local prefix (exclusive, or inclusive), sums[tile] the tile's total.
template <class OP, bool INCLUSIVE, class LOAD>
__device__ __forceinline__ void scan_tile(LOAD load, size_t count, typename OP::T* __restrict__ out, typename OP::T* __restrict__ sums) {
    typedef typename OP::T T;
    __shared__ T sh[MEM_THREADS];
    const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    T v[SCAN_ITEMS], sum = OP::id();
#pragma unroll
    for (u32 q = 0; q < SCAN_ITEMS; ++q) { v[q] = base + q < count ? load(base + q) : OP::id(); sum = OP::op(sum, v[q]); }
    T total;
    T run = block_scan<OP>(sh, sum, total);
#pragma unroll
    for (u32 q = 0; q < SCAN_ITEMS; ++q) {
        const T next = OP::op(run, v[q]);
        if (base + q < count) out[base + q] = INCLUSIVE ? next : run;
        run = next;
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: the tile sums become their exclusive scan, in place; *total_out (may be null) takes the grand total
template <class OP>
__global__ void __launch_bounds__(MEM_THREADS) mem_scan_sums_kernel(typename OP::T* __restrict__ sums, u32 ntiles, typename OP::T* __restrict__ total_out) {
    typedef typename OP::T T;
    __shared__ T sh[MEM_THREADS];
    T carry = OP::id();  // the same in every lane
    for (u32 b0 = 0; b0 < ntiles; b0 += MEM_THREADS) {
        const bool live = b0 + threadIdx.x < ntiles;
        const T v = live ? sums[b0 + threadIdx.x] : OP::id();
        T total;
        const T before = block_scan<OP>(sh, v, total);
        if (live) sums[b0 + threadIdx.x] = OP::op(carry, before);
        carry = OP::op(carry, total);
    }
    if (threadIdx.x == 0 && total_out) *total_out = carry;
}

struct LogPtrs {
    const u32 *address, *time, *value, *store_bits, *tape;
    size_t m, t;
    u32 word_bits;
};
__device__ __forceinline__ bool is_store(const u32* __restrict__ store_bits, u32 i) { return (store_bits[i >> 5] >> (i & 31)) & 1u; }

// record j < t is tape word j, record t + i log record i
__global__ void __launch_bounds__(MEM_THREADS) mem_keys_kernel(LogPtrs g, u32* __restrict__ keys, u32* __restrict__ index, unsigned long long* __restrict__ result) {
    const size_t j = (size_t)blockIdx.x * MEM_THREADS + threadIdx.x;
    if (j >= g.m + g.t) return;
    u32 key;
    if (j < g.t) key = tape_address(g.word_bits, j);
    else {
        const size_t i = j - g.t;
        key = g.address[i];
        if (!record_ok(g.word_bits, key, g.time[i], g.value[i], i ? g.time[i - 1] : 0u)) atomicMin(result, (unsigned long long)i);
    }
    keys[j] = key;
    index[j] = (u32)j;
}

// hist[digit * ntiles + tile]: the records of the tile with that digit
__global__ void __launch_bounds__(MEM_THREADS) mem_hist_kernel(const u32* __restrict__ keys, size_t count, u32 shift, u32* __restrict__ hist) {
    __shared__ u32 h[RADIX];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * SORT_TILE;
#pragma unroll
    for (u32 q = 0; q < SORT_ITEMS; ++q) {
        const size_t j = base + (size_t)q * MEM_THREADS + threadIdx.x;
        if (j < count) atomicAdd(&h[(keys[j] >> shift) & (RADIX - 1)], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}
static_assert(RADIX == MEM_THREADS, "one lane per digit");

__global__ void __launch_bounds__(MEM_THREADS) mem_scan_u32_kernel(u32* __restrict__ a, size_t count, u32* __restrict__ sums) {
    scan_tile<OpAdd, false>([a](size_t i) { return a[i]; }, count, a, sums);
}

// Wave w of the workgroup takes the records base + w * 64 * SORT_ITEMS ..., 64 consecutive ones per round, so (wave, round, lane) is the order
// of the records.  A round's lanes with equal digits find each other with eight ballots; the lowest of them advances the wave's counter of
// the digit, and a lane's rank is the counter before the round plus the equal lanes below it.
__global__ void __launch_bounds__(MEM_THREADS) mem_scatter_kernel(const u32* __restrict__ keys_in, const u32* __restrict__ index_in, u32* __restrict__ keys_out,
                                                                  u32* __restrict__ index_out, size_t count, u32 shift, const u32* __restrict__ hist,
                                                                  const u32* __restrict__ hist_sums) {
    constexpr u32 WAVES = MEM_THREADS / 64;
    __shared__ u32 cnt[WAVES][RADIX];
    __shared__ u32 digit_base[RADIX];
    const u32 w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (u32 i = threadIdx.x; i < WAVES * RADIX; i += MEM_THREADS) (&cnt[0][0])[i] = 0u;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * SORT_TILE + (size_t)w * (64 * SORT_ITEMS) + lane;
    u32 key[SORT_ITEMS], idx[SORT_ITEMS], rank[SORT_ITEMS];
#pragma unroll
    for (u32 q = 0; q < SORT_ITEMS; ++q) {
        const size_t j = base + (size_t)q * 64;
        const bool valid = j < count;
        key[q] = valid ? keys_in[j] : 0u;
        idx[q] = valid ? index_in[j] : 0u;
        const u32 d = (key[q] >> shift) & (RADIX - 1);
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (u32 b = 0; b < RADIX_BITS; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long set = __ballot(bit);
            same &= bit ? set : ~set;
        }
        const u32 leader = valid ? (u32)(__ffsll((long long)same) - 1) : lane;
        u32 before = 0u;
        if (valid && lane == leader) {
            before = cnt[w][d];
            cnt[w][d] = before + (u32)__popcll(same);
        }
        before = __shfl(before, (int)leader);
        rank[q] = before + (u32)__popcll(same & ((1ull << lane) - 1ull));
        __syncthreads();  // the next round's leader of a digit may be another lane
    }
    {   // the waves' counters become their exclusive prefix over the waves; the digit's place among all tiles comes from the scanned histogram
        const u32 d = threadIdx.x;
        u32 run = 0u;
#pragma unroll
        for (u32 v = 0; v < WAVES; ++v) { const u32 c = cnt[v][d]; cnt[v][d] = run; run += c; }
        const size_t at = (size_t)d * gridDim.x + blockIdx.x;
        digit_base[d] = hist[at] + hist_sums[at / SCAN_TILE];
    }
    __syncthreads();
#pragma unroll
    for (u32 q = 0; q < SORT_ITEMS; ++q) {
        const size_t j = base + (size_t)q * 64;
        if (j >= count) continue;
        const u32 d = (key[q] >> shift) & (RADIX - 1);
        const u32 pos = digit_base[d] + cnt[w][d] + rank[q];  // < count: the histogram counted these very digits
        keys_out[pos] = key[q];
        index_out[pos] = idx[q];
    }
}

// a sorted record opens a run that no tape word opens: it needs a synthesized Init row above it
__device__ __forceinline__ u32 needs_init(const u32* __restrict__ keys, const u32* __restrict__ index, size_t t, size_t j) {
    return (j == 0 || keys[j] != keys[j - 1]) && index[j] >= t ? 1u : 0u;
}
__global__ void __launch_bounds__(MEM_THREADS) mem_place_scan_kernel(const u32* __restrict__ keys, const u32* __restrict__ index, size_t t, size_t count,
                                                                     u32* __restrict__ place, u32* __restrict__ sums) {
    scan_tile<OpAdd, false>([=](size_t j) { return needs_init(keys, index, t, j); }, count, place, sums);
}

// sorted record j goes to row j + (synthesized rows above it) + (its own synthesized row)
__global__ void __launch_bounds__(MEM_THREADS) mem_rows_scatter_kernel(LogPtrs g, const u32* __restrict__ keys, const u32* __restrict__ index, const u32* __restrict__ place,
                                                                       const u32* __restrict__ place_sums, u32* __restrict__ row_address, u32* __restrict__ row_time,
                                                                       u32* __restrict__ row_value, u32* __restrict__ row_source, size_t rows) {
    const size_t j = (size_t)blockIdx.x * MEM_THREADS + threadIdx.x;
    if (j >= g.m + g.t) return;
    const u32 address = keys[j], rec = index[j];
    size_t r = j + place[j] + place_sums[j / SCAN_TILE];
    if (needs_init(keys, index, g.t, j)) {
        if (r < rows) { row_address[r] = address; row_time[r] = 0u; row_value[r] = 0u; row_source[r] = NO_SOURCE; }
        ++r;
    }
    if (r >= rows) return;  // cannot happen: rows is this scan's own total
    row_address[r] = address;
    if (rec < g.t) { row_time[r] = 0u; row_value[r] = g.tape[rec]; row_source[r] = NO_SOURCE; }
    else {
        const u32 i = rec - (u32)g.t;
        row_time[r] = g.time[i]; row_value[r] = g.value[i]; row_source[r] = i;
    }
}

// last[r] = (1 + the latest Init row <= r, 1 + the latest Init or Store row <= r) inside the tile, 0 where the tile has none yet
__global__ void __launch_bounds__(MEM_THREADS) mem_last_scan_kernel(const u32* __restrict__ row_source, const u32* __restrict__ store_bits, size_t rows,
                                                                    uint2* __restrict__ last, uint2* __restrict__ sums) {
    scan_tile<OpMaxPair, true>([=](size_t r) {
        const u32 src = row_source[r];
        const bool init = src == NO_SOURCE;
        return make_uint2(init ? (u32)r + 1u : 0u, init || is_store(store_bits, src) ? (u32)r + 1u : 0u);
    }, rows, last, sums);
}

// *n_inconsistent += inconsistent loads, *first_inconsistent = min(., log index of one); source_fill (may be null): NO_SOURCE behind the table
template <class F>
__global__ void __launch_bounds__(MEM_THREADS) mem_columns_kernel(const u32* __restrict__ row_address, const u32* __restrict__ row_time, const u32* __restrict__ row_value,
                                                                  const u32* __restrict__ row_source, const uint2* __restrict__ last, const uint2* __restrict__ last_sums,
                                                                  const u32* __restrict__ store_bits, size_t rows, uint4* __restrict__ dst, size_t n,
                                                                  u32* __restrict__ source_fill, unsigned long long* __restrict__ n_inconsistent, unsigned long long* __restrict__ first_inconsistent) {
    for (size_t r = (size_t)blockIdx.x * MEM_THREADS + threadIdx.x; r < n; r += (size_t)gridDim.x * MEM_THREADS) {
        if (r >= rows) {
#pragma unroll
            for (u32 c = 0; c < MEM_COLUMNS; ++c) store_zero(dst + 2 * ((size_t)c * n + r));
            if (source_fill) source_fill[r] = NO_SOURCE;
            continue;
        }
        const u32 src = row_source[r];
        const bool init = src == NO_SOURCE, store = !init && is_store(store_bits, src);
        const uint2 local = last[r], carry = last_sums[r / SCAN_TILE];
        // row 0 is an Init row, so both are at least 1 (the fallback keeps the indices inside the arrays whatever the scan holds)
        const u32 head1 = local.x > carry.x ? local.x : carry.x, holder1 = local.y > carry.y ? local.y : carry.y;
        const u32 run_head = head1 ? head1 - 1u : 0u, holder = holder1 ? holder1 - 1u : (u32)r;
        const u32 prev_run_address = run_head ? row_address[run_head - 1u] : 0u;
        const u32 prev_time = init ? 0u : row_time[r - 1];
        const u32 carried = row_value[holder];
        const Row row = derive_row(row_address[r], row_time[r], init, store, prev_time, prev_run_address, carried);
        if (!init && !store && row_value[r] != carried) {
            atomicAdd(n_inconsistent, 1ull);
            atomicMin(first_inconsistent, (unsigned long long)src);
        }
#pragma unroll
        for (u32 c = 0; c < MEM_COLUMNS; ++c) store_fe(dst + 2 * ((size_t)c * n + r), fe_from_u64<F>((u64)row.c[c]));
    }
}

int check_args(int field, const trh_mem_table_args_t* a) {
    if (!a) { set_error("mem_table_dev: null arguments"); return TRH_EINVAL; }
    TRH_TRY(check_field(field));
    if (!word_bits_ok(a->word_bits)) { set_error("mem_table_dev: word_bits %u is not an even number in 2 .. 32", a->word_bits); return TRH_EINVAL; }
    if (!tape_ok(a->word_bits, a->t)) { set_error("mem_table_dev: a tape of %zu words does not fit %u-bit words (byte-sized words, addresses below 2^word_bits)", a->t, a->word_bits); return TRH_EINVAL; }
    if ((u64)a->m >= MAX_RECORDS || (u64)a->t >= MAX_RECORDS || (u64)a->t + 2 * (u64)a->m >= MAX_RECORDS) { set_error("mem_table_dev: t + 2 m must stay below 2^31"); return TRH_EINVAL; }
    if (a->max_rows > a->n) { set_error("mem_table_dev: max_rows %zu above the columns' %zu rows", a->max_rows, a->n); return TRH_EINVAL; }
    if (a->n >= MAX_RECORDS * 2) { set_error("mem_table_dev: n out of range"); return TRH_EINVAL; }
    if ((!a->dst && a->n) || ((uintptr_t)a->dst & 15) != 0) { set_error("mem_table_dev: dst must be a 16-byte aligned device pointer"); return TRH_EINVAL; }
    if (a->m && (!a->address || !a->time || !a->value || !a->store_bits)) { set_error("mem_table_dev: null log array"); return TRH_EINVAL; }
    if (a->t && !a->tape) { set_error("mem_table_dev: null tape"); return TRH_EINVAL; }
    if ((((uintptr_t)a->address | (uintptr_t)a->time | (uintptr_t)a->value | (uintptr_t)a->store_bits | (uintptr_t)a->tape | (uintptr_t)a->src_index) & 3) != 0) {
        set_error("mem_table_dev: the word arrays must be 4-byte aligned");
        return TRH_EINVAL;
    }
    return TRH_OK;
}

// everything queued between the scratch's allocation and its return; the first failure ends it.  *sums / *mins: where the verdict lands (its second pair: once s has drained)
int run(int field, trh_mem_table_args_t* a, const Plan& p, char* block, Ctx& c, const u64** sums, const u64** mins) {
    const hipStream_t s = (hipStream_t)a->stream;
    u32* keys[2] = {(u32*)(block + p.off_keys[0]), (u32*)(block + p.off_keys[1])};
    u32* index[2] = {(u32*)(block + p.off_index[0]), (u32*)(block + p.off_index[1])};
    u32 *hist = (u32*)(block + p.off_hist), *hist_sums = (u32*)(block + p.off_hist_sums);
    u32 *place = (u32*)(block + p.off_place), *place_sums = (u32*)(block + p.off_place_sums);
    u32 *row_address = (u32*)(block + p.off_row_address), *row_time = (u32*)(block + p.off_row_time), *row_value = (u32*)(block + p.off_row_value);
    u32* row_source = a->src_index ? a->src_index : (u32*)(block + p.off_row_source);
    uint2 *last = (uint2*)(block + p.off_last), *last_sums = (uint2*)(block + p.off_last_sums);
    const LogPtrs g{a->address, a->time, a->value, a->store_bits, a->tape, a->m, a->t, a->word_bits};
    const size_t count = (size_t)p.records;

    unsigned long long *d_sums, *d_mins;
    TRH_TRY(verdict_begin(c, 2, 2, s, &d_sums, &d_mins));
    u32 sorted = 0;
    if (count) {
        hipLaunchKernelGGL(mem_keys_kernel, dim3(blocks_of(count, MEM_THREADS)), dim3(MEM_THREADS), 0, s, g, keys[0], index[0], d_mins);
        for (u32 pass = 0; pass < p.passes; ++pass, sorted ^= 1u) {
            const u32 shift = pass * RADIX_BITS;
            hipLaunchKernelGGL(mem_hist_kernel, dim3((unsigned)p.sort_tiles), dim3(MEM_THREADS), 0, s, (const u32*)keys[sorted], count, shift, hist);
            hipLaunchKernelGGL(mem_scan_u32_kernel, dim3((unsigned)p.hist_scan_tiles), dim3(MEM_THREADS), 0, s, hist, (size_t)(RADIX * p.sort_tiles), hist_sums);
            hipLaunchKernelGGL(mem_scan_sums_kernel<OpAdd>, dim3(1), dim3(MEM_THREADS), 0, s, hist_sums, (u32)p.hist_scan_tiles, (u32*)nullptr);
            hipLaunchKernelGGL(mem_scatter_kernel, dim3((unsigned)p.sort_tiles), dim3(MEM_THREADS), 0, s, (const u32*)keys[sorted], (const u32*)index[sorted], keys[sorted ^ 1u],
                               index[sorted ^ 1u], count, shift, (const u32*)hist, (const u32*)hist_sums);
        }
        hipLaunchKernelGGL(mem_place_scan_kernel, dim3((unsigned)p.record_scan_tiles), dim3(MEM_THREADS), 0, s, (const u32*)keys[sorted], (const u32*)index[sorted], (size_t)a->t, count,
                           place, place_sums);
        // the total lands in the low word of sum 0 (little-endian; the high word was seeded zero with it)
        hipLaunchKernelGGL(mem_scan_sums_kernel<OpAdd>, dim3(1), dim3(MEM_THREADS), 0, s, place_sums, (u32)p.record_scan_tiles, (u32*)d_sums);
        TRH_HIP_TRY(hipGetLastError());
    }
    // first synchronisation: the verdict on the log and the number of rows, before the destination is touched
    TRH_TRY(verdict_read(c, s, sums, mins));
    if (lowered((*mins)[0])) {
        set_error("mem_table_dev: log record %llu breaks the table's rules (address, time and value below 2^%u, times strictly increasing from 1)", (unsigned long long)(*mins)[0], a->word_bits);
        return TRH_EINVAL;
    }
    const u64 rows = p.records + (*sums)[0];
    a->rows = rows;
    if (rows > a->max_rows) { set_error("mem_table_dev: the table has %llu rows, max_rows is %zu", (unsigned long long)rows, a->max_rows); return TRH_EINVAL; }
    const u64 row_tiles = tiles_of(rows, SCAN_TILE);  // <= p.row_scan_tiles: rows <= row_cap
    if (rows) {
        hipLaunchKernelGGL(mem_rows_scatter_kernel, dim3(blocks_of(count, MEM_THREADS)), dim3(MEM_THREADS), 0, s, g, (const u32*)keys[sorted], (const u32*)index[sorted], (const u32*)place,
                           (const u32*)place_sums, row_address, row_time, row_value, row_source, (size_t)rows);
        hipLaunchKernelGGL(mem_last_scan_kernel, dim3((unsigned)row_tiles), dim3(MEM_THREADS), 0, s, (const u32*)row_source, a->store_bits, (size_t)rows, last, last_sums);
        hipLaunchKernelGGL(mem_scan_sums_kernel<OpMaxPair>, dim3(1), dim3(MEM_THREADS), 0, s, last_sums, (u32)row_tiles, (uint2*)nullptr);
    }
    if (a->n) {
        const unsigned blocks = blocks_of(a->n, MEM_THREADS);
        with_field(field, [&](auto f) {
            hipLaunchKernelGGL((mem_columns_kernel<decltype(f)>), dim3(blocks < 4096u ? blocks : 4096u), dim3(MEM_THREADS), 0, s, (const u32*)row_address, (const u32*)row_time,
                               (const u32*)row_value, (const u32*)row_source, (const uint2*)last, (const uint2*)last_sums, a->store_bits, (size_t)rows, (uint4*)a->dst, a->n,
                               a->src_index, d_sums + 1, d_mins + 1);
        });
    }
    TRH_HIP_TRY(hipGetLastError());
    TRH_TRY(verdict_fetch(c, s));
    c.memtable_rows = rows;
    c.memtable_sort_passes = count ? p.passes : 0;
    const u64 tiles[3] = {p.sort_tiles, p.record_scan_tiles, row_tiles};
    c.memtable_tiles = tiles[0] < tiles[1] ? tiles[0] : tiles[1];
    if (tiles[2] < c.memtable_tiles) c.memtable_tiles = tiles[2];
    return TRH_OK;
}

}  // namespace
}  // namespace trh

using namespace trh;

extern "C" {

int trh_mem_table_dev(int field_id, trh_mem_table_args_t* a) {
    TRH_TRY(check_args(field_id, a));
    TRH_ENTER(a->stream);
    Range range("trh_mem_table_dev");
    Ctx& c = ctx();
    a->rows = 0; a->n_inconsistent = 0; a->first_inconsistent = 0;
    const Plan p = make_plan(a->m, a->t, a->n, a->word_bits);
    void* block = nullptr;
    TRH_TRY(trh_malloc(&block, (size_t)p.bytes));
    const u64 *sums = nullptr, *mins = nullptr;
    const int rc = run(field_id, a, p, (char*)block, c, &sums, &mins);
    // second synchronisation: trh_free returns once the device has drained (as hipFree does), which is when the verdict has landed
    const int rc_free = trh_free(block);
    TRH_TRY(rc);
    TRH_TRY(rc_free);
    a->n_inconsistent = sums[1];
    a->first_inconsistent = min_or(mins[1], a->m);
    return TRH_OK;
}

}  // extern "C"
