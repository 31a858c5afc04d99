// Resident base sets (trh_bases_t): created from host points, 32-byte encodings or the generator, wrapped around device memory, range-sharded
// over the device group; their lazily built copies (lazy-domain records, fixed-base table) and the one MSM launch that reads them.
#include "bases.h"

using namespace trh;

namespace trh {
namespace {

struct DevTemp {  // a device buffer that lives for one call
    void* p = nullptr;
    ~DevTemp() { if (p) (void)hipFree(p); }
};

// one resident set on the entered context's device: uploaded from the host, decoded from 32-byte encodings (comp != null; index_base: the
// position of comp[0] in the caller's array, for the message that names an invalid one), or generated (xy == null)
int bases_create_local(int curve, const uint64_t* xy, uint64_t s0, uint64_t d, uint64_t first, size_t n, trh_bases_t* out, const uint8_t* comp = nullptr,
                       size_t index_base = 0) {
    BasesOwner b(new trh_bases{curve, nullptr, n, true});
    b->owner = &ctx();
    hipError_t e = hipMalloc(&b->d_xy, n * 64 + 64);
    if (e == hipSuccess && n && xy) e = hipMemcpy(b->d_xy, xy, n * 64, hipMemcpyHostToDevice);
    if (e != hipSuccess) { set_error("bases_create: %s", hipGetErrorString(e)); return e == hipErrorOutOfMemory ? TRH_ENOMEM : TRH_EHIP; }
    if (comp && n) {
        DevTemp enc;
        u64 bad = n;
        e = hipMalloc(&enc.p, n * 32);
        if (e == hipSuccess) e = hipMemcpy(enc.p, comp, n * 32, hipMemcpyHostToDevice);
        if (e != hipSuccess) { set_error("bases_create_compressed: %s", hipGetErrorString(e)); return e == hipErrorOutOfMemory ? TRH_ENOMEM : TRH_EHIP; }
        TRH_TRY(points_decompress_device(curve, enc.p, b->d_xy, nullptr, n, 0, &bad));
        if (bad < n) { set_error("bases_create_compressed: encoding %zu is not a point of the curve", index_base + (size_t)bad); return TRH_EINVAL; }
    } else if (!comp && !xy && n) {
        TRH_TRY(bases_generate_device(curve, s0, d, first, n, b->d_xy, 0));
        if (hipStreamSynchronize(0) != hipSuccess) { set_error("bases_generate: kernel failed"); return TRH_EHIP; }
    }
    *out = b.release();
    return TRH_OK;
}

// owned base sets are immutable: convert them to the lazy Montgomery domain once and keep the copy
const void* lazy_bases(trh_bases_t b, size_t offset, hipStream_t s) {
    if (!b->owned || b->n == 0) return nullptr;
    std::lock_guard<std::mutex> lk(b->mu);
    if (!b->d_z) {
        void* z = nullptr;
        if (hipMalloc(&z, b->n * ZREC + ZREC) != hipSuccess) return nullptr;  // fall back to per-call conversion
        if (msm_convert_bases(b->curve, b->d_xy, z, b->n, s) != TRH_OK || hipStreamSynchronize(s) != hipSuccess) { (void)hipFree(z); return nullptr; }
        b->d_z = z;
    }
    return (const char*)b->d_z + offset * ZREC;
}

// the fixed-base table covers the whole set: used for full-range MSMs unless a window width is forced
const MsmFixedBase* fixed_base(trh_bases_t b, size_t offset, size_t n) {
    return (b->d_table && offset == 0 && n == b->n && ctx().window_override == 0) ? &b->fb : nullptr;
}

}  // namespace

int msm_launch(trh_bases* b, size_t offset, const void* scalars_dev, size_t n, size_t batch, size_t stride, int mont, hipStream_t s, const void* tails_dev, MsmFlags flags) {
    return msm_enqueue(b->curve, (const char*)b->d_xy + offset * 64, lazy_bases(b, offset, s), scalars_dev, n, batch, stride, mont, s, fixed_base(b, offset, n), tails_dev, flags);
}

// ---- range-sharded base sets over the device group (trh_init_multi) ---------------------------------------------------
// Shard g of G owns the pairs [g * per, (g + 1) * per) (per = ceil(n / G)) on the group's g-th context -- the partition
// best_multiexp itself makes per rayon thread.  An MSM enqueues one local Pippenger per shard on that context's own stream from
// the calling host thread, then collects the G partial points with plain device-to-host copies into pinned memory and adds them
// on the host (point_sum_host).  No RCCL here: EC addition is not a reduce op, the payload is 96 B per GPU, the result is
// consumed by the host (transcript), and everything happens inside ONE process -- a collective would only add a rendezvous.
// (bench.py's process-per-GPU harness does use RCCL's all_gather for the same 96-byte partials: there the ranks are processes.)
int sharded_create(int curve, const uint64_t* xy_host, uint64_t s0, uint64_t d, uint64_t first, size_t n, trh_bases_t* out, const uint8_t* comp) {
    const std::vector<Ctx*>& group = device_group();
    const size_t G = group.size();
    BasesOwner B(new trh_bases{curve, nullptr, n, true});
    B->owner = group[0];
    const size_t per = (n + G - 1) / G;
    B->shard_off.push_back(0);
    for (size_t g = 0; g < G; ++g) {
        const size_t lo = g * per < n ? g * per : n, hi = lo + per < n ? lo + per : n;
        trh_bases* sh = nullptr;
        Enter en;
        TRH_TRY(en.begin(nullptr, group[g]));
        TRH_TRY(bases_create_local(curve, xy_host ? xy_host + 8 * lo : nullptr, s0, d, first + lo, hi - lo, &sh, comp ? comp + 32 * lo : nullptr, lo));
        B->shards.push_back(sh);
        B->shard_off.push_back(hi);
    }
    *out = B.release();
    return TRH_OK;
}

}  // namespace trh

extern "C" {

static int bases_create(int curve, const uint64_t* xy, size_t n, trh_bases_t* out) {
    TRH_TRY(require_init());
    if (!out || (n && !xy)) { set_error("bases_create: null pointer"); return TRH_EINVAL; }
    if (use_group(n)) return sharded_create(curve, xy, 0, 0, 0, n, out);
    TRH_ENTER(0);
    return bases_create_local(curve, xy, 0, 0, 0, n, out);
}
int trh_bases_create_pallas(const uint64_t* xy, size_t n, trh_bases_t* out) { return bases_create(TRH_PALLAS, xy, n, out); }
int trh_bases_create_vesta(const uint64_t* xy, size_t n, trh_bases_t* out) { return bases_create(TRH_VESTA, xy, n, out); }

int trh_bases_create_compressed(int curve, const uint8_t* bytes_host, size_t n, trh_bases_t* out) {
    TRH_TRY(require_init());
    TRH_TRY(check_curve(curve));
    if (!out || (n && !bytes_host)) { set_error("bases_create_compressed: null pointer"); return TRH_EINVAL; }
    if (use_group(n)) return sharded_create(curve, nullptr, 0, 0, 0, n, out, bytes_host);
    TRH_ENTER(0);
    static const uint8_t none[1] = {0};
    return bases_create_local(curve, nullptr, 0, 0, 0, n, out, n ? bytes_host : none);
}

int trh_bases_download_compressed(trh_bases_t b, size_t offset, size_t n, uint8_t* bytes_host) {
    if (!b || (n && !bytes_host) || offset + n > b->n) { set_error("bases_download_compressed: bad range"); return TRH_EINVAL; }
    if (!b->shards.empty()) {
        for (size_t g = 0; g < b->shards.size(); ++g) {
            const ShardRange r = shard_range(b, g, offset, n);
            if (r.count) TRH_TRY(trh_bases_download_compressed(b->shards[g], r.local, r.count, bytes_host + 32 * r.at));
        }
        return TRH_OK;
    }
    if (!n) return TRH_OK;
    TRH_ENTER_CTX(0, b->owner);
    DevTemp enc;
    TRH_HIP_TRY(hipMalloc(&enc.p, n * 32));
    TRH_TRY(points_compress_device(b->curve, (const char*)b->d_xy + offset * 64, enc.p, n, 0));
    const hipError_t e = hipMemcpy(bytes_host, enc.p, n * 32, hipMemcpyDeviceToHost);  // ordered behind the kernel on the null stream
    if (e != hipSuccess) { set_error("bases_download_compressed: %s", hipGetErrorString(e)); return TRH_EHIP; }
    return TRH_OK;
}

int trh_bases_wrap_device(int curve, const void* xy_dev, size_t n, trh_bases_t* out) {
    TRH_TRY(check_curve(curve));
    if (!out || (n && !xy_dev)) { set_error("bases_wrap_device: null pointer"); return TRH_EINVAL; }
    TRH_ENTER(0);
    trh_bases* b = new trh_bases{curve, (void*)xy_dev, n, false};
    b->owner = &ctx();
    *out = b;
    return TRH_OK;
}

int trh_bases_generate(int curve, uint64_t s0, uint64_t d, uint64_t first, size_t n, trh_bases_t* out) {
    TRH_TRY(require_init());
    TRH_TRY(check_curve(curve));
    if (!out) { set_error("bases_generate: null pointer"); return TRH_EINVAL; }
    if (use_group(n)) return sharded_create(curve, nullptr, s0, d, first, n, out);
    TRH_ENTER(0);
    return bases_create_local(curve, nullptr, s0, d, first, n, out);
}

int trh_bases_download(trh_bases_t b, size_t offset, size_t n, uint64_t* xy_host) {
    if (!b || !xy_host || offset + n > b->n) { set_error("bases_download: bad range"); return TRH_EINVAL; }
    if (!b->shards.empty()) {
        for (size_t g = 0; g < b->shards.size(); ++g) {
            const ShardRange r = shard_range(b, g, offset, n);
            if (r.count) TRH_TRY(trh_bases_download(b->shards[g], r.local, r.count, xy_host + 8 * r.at));
        }
        return TRH_OK;
    }
    TRH_ENTER_CTX(0, b->owner);
    TRH_HIP_TRY(hipMemcpy(xy_host, (const char*)b->d_xy + offset * 64, n * 64, hipMemcpyDeviceToHost));
    return TRH_OK;
}
const void* trh_bases_device_ptr(trh_bases_t b) { return b ? b->d_xy : nullptr; }
size_t trh_bases_len(trh_bases_t b) { return b ? b->n : 0; }
int trh_bases_shards(trh_bases_t b) { return b ? (b->shards.empty() ? 1 : (int)b->shards.size()) : 0; }
void trh_bases_destroy(trh_bases_t b) {
    if (!b) return;
    for (trh_bases* sh : b->shards) trh_bases_destroy(sh);
    if (b->owned && b->d_xy) (void)hipFree(b->d_xy);
    if (b->d_z) (void)hipFree(b->d_z);
    if (b->d_table) (void)hipFree(b->d_table);
    delete b;
}

int trh_bases_precompute(trh_bases_t b, int window_bits) {
    if (!b) { set_error("bases_precompute: null handle"); return TRH_EINVAL; }
    if (!b->owned) { set_error("bases_precompute: wrapped device memory may change under the table; create an owned set"); return TRH_EINVAL; }
    if (!b->shards.empty()) { set_error("bases_precompute: range-sharded sets keep the per-window path"); return TRH_EINVAL; }
    TRH_ENTER_CTX(0, b->owner);
    Range range("trh_bases_precompute");
    std::lock_guard<std::mutex> lk(b->mu);  // (an MSM that is already running over the old table from another context is the caller's to exclude: trh.h)
    if (b->d_table) { (void)hipFree(b->d_table); b->d_table = nullptr; b->fb = MsmFixedBase{nullptr, 0, 0}; }
    if (b->n == 0) return TRH_OK;
    int cb = window_bits;
    if (cb == 0) {  // wide windows: the single reduction costs 2^(c-1) additions per MSM against n * ceil(255 / c) mixed adds
        int l = 0;
        while (((size_t)2 << l) <= b->n) ++l;
        cb = l - 2 < 6 ? 6 : l - 2 > 17 ? 17 : l - 2;  // measured at 2^18 (batch 32): c = 16 beats 15 / 17
    }
    if (!msm_fixed_base_fits(b->n, cb)) { set_error("bases_precompute: window width %d with %zu bases is outside the fixed-base range (W * n <= 2^24, c <= 18)", cb, b->n); return TRH_EINVAL; }
    const int W = msm_fixed_base_windows(cb);
    void* t = nullptr;
    hipError_t e = hipMalloc(&t, (size_t)W * b->n * ZREC + ZREC);
    if (e != hipSuccess) { set_error("bases_precompute: hipMalloc(%zu): %s", (size_t)W * b->n * ZREC, hipGetErrorString(e)); return TRH_ENOMEM; }
    int rc = msm_build_table(b->curve, b->d_xy, b->n, cb, t, 0);
    if (rc == TRH_OK && hipStreamSynchronize(0) != hipSuccess) { set_error("bases_precompute: table kernel failed"); rc = TRH_EHIP; }
    if (rc != TRH_OK) { (void)hipFree(t); return rc; }
    b->d_table = t;
    b->fb = MsmFixedBase{t, cb, W};
    return TRH_OK;
}
int trh_bases_precomputed_window_bits(trh_bases_t b) { return b && b->d_table ? b->fb.c : 0; }

int trh_bases_reserve(trh_bases_t b, size_t n, size_t batch) {
    if (!b) { set_error("bases_reserve: null handle"); return TRH_EINVAL; }
    if (n == 0 || n > b->n || batch == 0) { set_error("bases_reserve: n = %zu, batch = %zu over a set of %zu bases", n, batch, b->n); return TRH_EINVAL; }
    if (!b->shards.empty()) return TRH_OK;  // every shard's context sizes itself at its first MSM
    TRH_ENTER(0);
    Range range("trh_bases_reserve");
    TRH_TRY(msm_ready(b, "bases_reserve"));
    Ctx& c = ctx();
    TRH_TRY(c.msm.tails.ensure(batch * 32));
    MsmFlags reserve;
    reserve.reserve_only = true;
    TRH_TRY(msm_launch(b, 0, b->d_xy /* never read */, n, batch, n, 1, nullptr, batch > 1 ? c.msm.tails.p : nullptr, reserve));
    // the shape of an IPA opening's round MSMs -- two rows over the whole of a tabled set of 2^k + 2 points (g || w || u): the opening's own buffers too
    if (batch == 2 && n == b->n && b->d_table && n > 2 && ((n - 2) & (n - 3)) == 0) {
        uint32_t k = 0;
        while (((size_t)1 << k) < n - 2) ++k;
        TRH_TRY(ipa_reserve(b->curve, b, k));
    }
    return TRH_OK;
}

}  // extern "C"
