// The resident base set (trh_bases_t) and what its two users inside the library share: bases.hip (create / download / destroy, the lazily
// built copies) and msmapi.hip (every MSM entry over a handle).  ipa*.hip read the handle's fields.
#pragma once
#include <memory>

#include "ctx.h"

struct trh_bases {
    int curve;
    void* d_xy;
    size_t n;
    bool owned;
    void* d_z = nullptr;  // owned (immutable) sets: the bases converted once to the lazy Montgomery domain
    void* d_table = nullptr;  // trh_bases_precompute: W x n shifted copies (see MsmFixedBase)
    trh::MsmFixedBase fb{nullptr, 0, 0};
    trh::Ctx* owner = nullptr;  // the context (device) the memory lives on
    // handles are shared by every context of their device: the lazily built copies (d_z, d_table) are created / replaced under this lock
    // (two threads on two contexts running their first MSM over the same set would otherwise both convert, and one copy would leak)
    std::mutex mu;
    // range-sharded set (trh_init_multi): shard g holds bases [shard_off[g], shard_off[g + 1]) on its own context's device;
    // d_xy is null and the per-shard handles carry the device memory
    std::vector<trh_bases*> shards;
    std::vector<size_t> shard_off;
};

namespace trh {

// a handle that is destroyed (shards, device memory and all) unless it is released to the caller
struct BasesDeleter { void operator()(trh_bases* b) const { trh_bases_destroy(b); } };
typedef std::unique_ptr<trh_bases, BasesDeleter> BasesOwner;

// capi.hip: the device group of trh_init_multi (front: the process default) and the context the calling thread's entries resolve to
const std::vector<Ctx*>& device_group();
Ctx* thread_ctx();
bool on_group_default();   // a device group exists and the caller is on the default context: what it does goes to every shard's context
bool use_group(size_t n);  // ... and a set of n bases is large enough (trh_set_shard_min) to be range-sharded over the group

// what of [offset, offset + n) shard g of a range-sharded set holds: from `local` inside the shard, `count` pairs (0: none), whose first
// is element `at` of the caller's array
struct ShardRange { size_t local, count, at; };
inline ShardRange shard_range(const trh_bases* b, size_t g, size_t offset, size_t n) {
    const size_t lo = b->shard_off[g] > offset ? b->shard_off[g] : offset;
    const size_t hi = b->shard_off[g + 1] < offset + n ? b->shard_off[g + 1] : offset + n;
    return hi > lo ? ShardRange{lo - b->shard_off[g], hi - lo, lo - offset} : ShardRange{0, 0, 0};
}

// bases.hip
int sharded_create(int curve, const uint64_t* xy_host, uint64_t s0, uint64_t d, uint64_t first, size_t n, trh_bases_t* out, const uint8_t* comp = nullptr);
// THE launch of an MSM over a resident set on the entered context: `batch` rows of n scalars (row b at scalars_dev + b * stride elements)
// over the bases [offset, offset + n), with the set's lazy-domain copy (made at first use) and, when the range is the whole of a tabled
// set, its fixed-base table -- so a range tile of a larger call never finds one.  msm_finish collects the result.
int msm_launch(trh_bases* b, size_t offset, const void* scalars_dev, size_t n, size_t batch, size_t stride, int mont, hipStream_t s, const void* tails_dev = nullptr,
               MsmFlags flags = {});

// msmapi.hip
// TRH_EINVAL unless the handle is ONE set on the entered context's device, then msm_idle (ctx.h): handle and context can take an MSM
int msm_ready(trh_bases* b, const char* what);
void bases_cache_clear();  // trh_shutdown: the cached sets go while their contexts still exist

}  // namespace trh
