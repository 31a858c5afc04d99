// The lookup part of MockProver::verify on resident columns: trh_lookup_check_dev (include/trh.h).
// halo2_proofs 0.2.0 dev.rs collects the table's rows of evaluated expressions and reports every usable row whose input tuple is not among
// them.  Here the table's rows go into a lock-free open-addressing set of row indices (csrc/tuplehash.h: the hash, the slot sequence, insert
// and probe, shared with the host test) and every input row probes it: exact tuple membership, not the theta compression of the prover.
// The verdict leaves as in expr.hip's gate check (verdict.h): one ballot per wave of 64 consecutive rows, written by lane 0 as a bitmap
// word, and one atomicAdd / atomicMin per wave that saw a bad row.  Sums: bad rows, slots visited; min: the smallest bad row.
#include "ctx.h"
#include "tuplehash.h"
#include "verdict.h"

namespace trh {
namespace {

constexpr unsigned MC_BLOCK = 256;

// lane 0 of every wave adds the wave's total to *counter
__device__ __forceinline__ void wave_add(unsigned long long* counter, u32 v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(counter, (unsigned long long)v);
}

// cols: the `width` table columns.  One thread per table row below `rows`.
__global__ void __launch_bounds__(MC_BLOCK) tuple_insert_kernel(u32* __restrict__ slots, u64 capacity, const void* const* __restrict__ tables, u32 width, size_t rows,
                                                                unsigned long long* __restrict__ probes) {
    const size_t gid = (size_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    u32 visited = 0;
    if (gid < rows) {
        // a slot only ever goes from EMPTY to a row: a plain read that finds it occupied is final (and spares the atomic -- a padded table
        // sends thousands of threads to one slot), one that finds it EMPTY may be stale and is settled by the compare-and-swap
        auto claim = [](u32* slot, u32 row) -> u32 {
            const u32 seen = *(volatile u32*)slot;
            return seen != tuplehash::EMPTY ? seen : atomicCAS(slot, tuplehash::EMPTY, row);
        };
        visited = tuplehash::insert_row(slots, capacity, tables, width, (u32)gid, claim);
    }
    wave_add(probes, visited);
}

// cols: the `width` input columns, then the `width` table columns.  One thread per input row; rows at or beyond usable_rows are never read.
// *n_bad += bad rows, *first_bad = min(*first_bad, smallest bad row); bitmap (may be null): ceil(usable_rows / 64) words, every one written.
__global__ void __launch_bounds__(MC_BLOCK) tuple_probe_kernel(const u32* __restrict__ slots, u64 capacity, const void* const* __restrict__ cols, u32 width,
                                                               size_t usable_rows, unsigned long long* __restrict__ n_bad, unsigned long long* __restrict__ first_bad,
                                                               unsigned long long* __restrict__ bitmap, unsigned long long* __restrict__ probes) {
    const size_t gid = (size_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    u32 visited = 0;
    bool bad = false;
    if (gid < usable_rows) bad = !tuplehash::probe_row(slots, capacity, cols, cols + width, width, gid, &visited);
    const unsigned long long ballot = wave_verdict(bad, gid, n_bad, first_bad);
    if ((threadIdx.x & 63) == 0 && bitmap && (gid >> 6) < (usable_rows + 63) / 64) bitmap[gid >> 6] = ballot;
    wave_add(probes, visited);
}

}  // namespace
}  // namespace trh

using namespace trh;

extern "C" {

int trh_lookup_check_dev(int field_id, const void* const* inputs_dev, const void* const* tables_dev, uint32_t width, size_t usable_rows, uint64_t* n_bad,
                         uint64_t* first_bad_row, void* bad_bitmap_dev_or_null) {
    TRH_TRY(require_init());
    TRH_TRY(check_field(field_id));  // both fields store an element in the same eight words: the id only has to be a known one
    if (!inputs_dev || !tables_dev || !n_bad || !first_bad_row) { set_error("lookup_check: null pointer"); return TRH_EINVAL; }
    if (width == 0 || width > tuplehash::MAX_WIDTH) { set_error("lookup_check: width %u outside 1 .. %u", width, tuplehash::MAX_WIDTH); return TRH_EINVAL; }
    if (usable_rows == 0 || usable_rows > ((size_t)1 << 30)) { set_error("lookup_check: usable_rows %zu outside 1 .. 2^30", usable_rows); return TRH_EINVAL; }
    if (((uintptr_t)bad_bitmap_dev_or_null & 7) != 0) { set_error("lookup_check: the bitmap must be 8-byte aligned"); return TRH_EINVAL; }
    const void* h_cols[2 * tuplehash::MAX_WIDTH];
    for (uint32_t j = 0; j < 2 * width; ++j) {
        const void* p = j < width ? inputs_dev[j] : tables_dev[j - width];
        if (!p) { set_error("lookup_check: %s column %u is a null pointer", j < width ? "input" : "table", j < width ? j : j - width); return TRH_EINVAL; }
        if (((uintptr_t)p & 15) != 0) { set_error("lookup_check: %s column %u: elements must be 16-byte aligned", j < width ? "input" : "table", j < width ? j : j - width); return TRH_EINVAL; }
        h_cols[j] = p;
    }
    TRH_ENTER(0);  // the verdict goes to host memory: no stream parameter, the work follows the context's previous call (trh.h)
    Range range("trh_lookup_check_dev");
    Ctx& c = ctx();
    const hipStream_t s = nullptr;
    // one block of the device pool: the slots, then the column pointers
    const u64 capacity = tuplehash::capacity_for(usable_rows);
    const size_t slot_bytes = (size_t)capacity * sizeof(u32), ptr_bytes = 2 * (size_t)width * sizeof(void*);
    void* block = nullptr;
    unsigned long long *d_sums, *d_min;
    TRH_TRY(verdict_begin(c, 2, 1, s, &d_sums, &d_min));
    TRH_TRY(trh_malloc(&block, slot_bytes + ptr_bytes));
    u32* d_slots = (u32*)block;
    const void** d_cols = (const void**)((char*)block + slot_bytes);
    const unsigned blocks = blocks_of(usable_rows, MC_BLOCK);
    const u64 *sums = nullptr, *min = nullptr;
    hipError_t err = hipMemsetAsync(d_slots, 0xFF, slot_bytes, s);
    if (err == hipSuccess) err = hipMemcpyAsync(d_cols, h_cols, ptr_bytes, hipMemcpyHostToDevice, s);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(tuple_insert_kernel, dim3(blocks), dim3(MC_BLOCK), 0, s, d_slots, capacity, (const void* const*)(d_cols + width), width, usable_rows, d_sums + 1);
        hipLaunchKernelGGL(tuple_probe_kernel, dim3(blocks), dim3(MC_BLOCK), 0, s, (const u32*)d_slots, capacity, (const void* const*)d_cols, width, usable_rows, d_sums, d_min,
                           (unsigned long long*)bad_bitmap_dev_or_null, d_sums + 1);
        err = hipGetLastError();
    }
    if (err == hipSuccess && verdict_read(c, s, &sums, &min) != TRH_OK && (err = hipGetLastError()) == hipSuccess) err = hipErrorUnknown;  // reported in this entry's own text
    const int rc_free = trh_free(block);
    if (err != hipSuccess) { set_error("lookup_check: %s", hipGetErrorString(err)); return TRH_EHIP; }
    TRH_TRY(rc_free);
    c.lookup_check_probes = sums[1];
    *n_bad = sums[0];
    *first_bad_row = min_or(min[0], usable_rows);
    return TRH_OK;
}

}  // extern "C"
