// The MSM entries of the C ABI: trh_best_multiexp_* (host scalars and host bases, with the opt-in cache of base sets), trh_msm* and
// trh_commit_batch_* over a resident handle, the PCIe range-tiled MSM and the range-sharded MSM over the device group behind them.
#include <string.h>

#include <chrono>
#include <string>
#include <thread>

#include "bases.h"
#include "basescache.h"
#include "hostplan.h"

using namespace trh;

namespace trh {

int msm_idle(const char* what) {
    if (ctx().msm.pending_curve >= 0) { set_error("%s: this context has an enqueued MSM that was not finished", what); return TRH_EBUSY; }
    return TRH_OK;
}
static int single_device(trh_bases_t bases, const char* what) {
    if (!bases->shards.empty()) { set_error("%s: needs a base set on ONE device (this handle is range-sharded over %zu)", what, bases->shards.size()); return TRH_EINVAL; }
    if (bases->owner && bases->owner->device != ctx().device) { set_error("%s: the base set lives on device %d, the calling context on device %d", what, bases->owner->device, ctx().device); return TRH_EINVAL; }
    return TRH_OK;
}
int msm_ready(trh_bases_t bases, const char* what) {
    TRH_TRY(single_device(bases, what));
    return msm_idle(what);
}

namespace {

int msm_sharded(trh_bases* B, size_t offset, const void* scalars, bool scalars_on_host, size_t n, int mont, hipStream_t caller_stream, uint64_t* out);

// a synchronous entry point leaves no MSM "in flight" behind, whatever went wrong between its enqueue and its finish
// (otherwise every later call on the context would answer TRH_EBUSY).  Declared once the context is known to be idle.
struct PendingGuard {
    Ctx& c;
    ~PendingGuard() {
        if (c.msm.pending_curve < 0) return;
        (void)hipStreamSynchronize(c.msm.pending_stream);
        c.msm.pending_curve = -1;
        c.msm.tile_sum_valid = false;
    }
};

// One MSM with the scalars (and, for best_multiexp, the bases) in HOST memory.  The sum over pairs is cut into ranges: range
// t + 1 crosses PCIe (stage_h2d on the upload stream, two device buffers) while range t is computed; the range points are added
// on the host.  With the bases on the host the call is bound by the link (96 B per pair: 2^24 pairs = 1.6 GB = 28 ms at 57 GB/s
// against 17 ms of arithmetic), so the ranges are small (2^20 pairs) and only the last one's arithmetic is exposed; with resident
// bases (32 B per pair) it is bound by the arithmetic and the ranges are large (2^22), only the first upload is exposed.
int msm_host_tiled(int curve, const uint64_t* coeffs, const uint64_t* bases_host, trh_bases* res, size_t offset, size_t n, int mont, uint64_t* out) {
    Ctx& c = ctx();
    TRH_TRY(stage_begin(c));
    StageScope scope(c);
    Stage& st = c.stage;
    const std::vector<size_t> cut = hostplan::msm_host_cuts(bases_host != nullptr, n);  // range boundaries (hostplan.h)
    const size_t ntiles = cut.size() - 1;
    c.msm.host_ranges = ntiles;
    uint64_t acc[24];
    memset(acc, 0, sizeof(acc));
    // option trace, bit 0: where the call's time goes (microseconds since here, stderr)
    const bool tr_on = (opt().trace & 1) != 0;
    const auto tr_t0 = std::chrono::steady_clock::now();
    auto tr_mark = [&](const char* what) {
        if (tr_on) fprintf(stderr, "[trh msm] %9.1f us  %s\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tr_t0).count(), what);
    };
    for (size_t t = 0; t < ntiles; ++t) {  // both device buffers at their final size before anything is in flight (a growing DevBuf frees)
        size_t longest = 0;
        for (size_t u = t & 1; u < ntiles; u += 2) longest = cut[u + 1] - cut[u] > longest ? cut[u + 1] - cut[u] : longest;
        if (t < 2) { TRH_TRY(st.ring_in[t].ensure(longest * 32 + 32)); if (bases_host) TRH_TRY(st.ring_out[t].ensure(longest * 64 + 64)); }
    }
    for (size_t t = 0; t < ntiles; ++t) {
        const size_t slot = t & 1, off = cut[t], cur = cut[t + 1] - cut[t];
        // (only the call's first bytes gate anything: every later range streams behind the one before it, full slots throughout)
        // (zero_elide: a witness column is zero on three quarters of its rows -- the chunks of the transfer that are zero throughout become a
        //  device-side memset instead of a copy into the pinned ring and a DMA; a chunk of random scalars answers "not zero" at its first word)
        TRH_TRY(stage_h2d(c, st.ring_in[slot].p, coeffs + 4 * off, cur * 32, st.us, t > 0, true, ntiles > 1 || bases_host != nullptr));
        if (bases_host) {
            TRH_TRY(stage_h2d(c, st.ring_out[slot].p, bases_host + 8 * off, cur * 64, st.us, true));
        }
        TRH_HIP_TRY(hipEventRecord(st.ev_up[slot], st.us));
        tr_mark("scalars handed to the upload stream");
        if (t > 0) {  // the previous range finished under this upload
            TRH_TRY(msm_finish(curve, st.cs, acc + 12, 1));
            TRH_TRY(point_sum_host(curve, acc, 2, acc));
        }
        TRH_HIP_TRY(hipStreamWaitEvent(st.cs, st.ev_up[slot], 0));
        // resident bases: the fixed-base table covers whole sets of at most 2^24 / W pairs (W >= 15: about 2^20), which never split: the growing
        // ranges start above 3 * 2^21 pairs.  A call that does split therefore never finds a table (no range is the whole set), and every range
        // takes the per-window path
        if (bases_host) TRH_TRY(msm_enqueue(curve, st.ring_out[slot].p, nullptr, st.ring_in[slot].p, cur, 1, cur, mont, st.cs));
        else TRH_TRY(msm_launch(res, offset + off, st.ring_in[slot].p, cur, 1, cur, mont, st.cs));
        tr_mark("MSM enqueued");
    }
    TRH_TRY(msm_finish(curve, st.cs, acc + 12, 1));
    tr_mark("MSM finished");
    if (ntiles > 1) TRH_TRY(point_sum_host(curve, acc, 2, acc));
    memcpy(out, ntiles > 1 ? acc : acc + 12, 96);
    return scope.finish();
}

// the opt-in cache of base sets (option bases_cache): the policy is basescache.h's, the handles and the lock are kept here
std::mutex g_cache_mu;
BasesCache g_cache;

int best_multiexp_host(int curve, const uint64_t* coeffs, const uint64_t* bases, size_t n, uint64_t* out) {
    TRH_TRY(require_init());
    Range range(curve == TRH_PALLAS ? "trh_best_multiexp_pallas" : "trh_best_multiexp_vesta");
    if (!out || (n && (!coeffs || !bases))) { set_error("best_multiexp: null pointer"); return TRH_EINVAL; }
    if (n >= ((size_t)1 << 31)) { set_error("best_multiexp: n too large"); return TRH_EINVAL; }
    if (n == 0) { memset(out, 0, 96); return TRH_OK; }  // the empty sum: the identity (an empty Rust slice may carry any pointer)
    if (opt().bases_cache && n >= 1024) {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        const BasesCache::Key key{curve, bases, n, BasesCache::fingerprint(bases, n)};
        BasesCache::Entry* hit = g_cache.find(key);
        if (!hit && g_cache.sighting(key)) {
            trh_bases_destroy(g_cache.evict());
            trh_bases* h = nullptr;
            TRH_TRY(curve == TRH_PALLAS ? trh_bases_create_pallas(bases, n, &h) : trh_bases_create_vesta(bases, n, &h));
            hit = g_cache.insert(key, h);
        }
        if (hit) {
            if (g_cache.use(hit) && hit->h->shards.empty()) (void)trh_bases_precompute(hit->h, 0);  // outside the supported range: stays on the per-window path
            return trh_msm(hit->h, 0, coeffs, n, 1, out);
        }
    }
    if (use_group(n)) {  // device group: every GPU takes a range of the pairs
        trh_bases* h = nullptr;
        TRH_TRY(sharded_create(curve, bases, 0, 0, 0, n, &h));
        const BasesOwner owner(h);
        return msm_sharded(h, 0, coeffs, true, n, 1, nullptr, out);
    }
    TRH_ENTER(0);
    TRH_TRY(msm_idle("best_multiexp"));
    PendingGuard guard{ctx()};
    return msm_host_tiled(curve, coeffs, bases, nullptr, 0, n, 1, out);
}

int msm_args(trh_bases_t bases, size_t offset, const void* scalars, size_t n, size_t batch, void* out) {
    TRH_TRY(require_init());
    if (!bases || !out || (n && !scalars)) { set_error("msm: null pointer"); return TRH_EINVAL; }
    if (offset + n > bases->n || offset + n < offset) { set_error("msm: range [%zu, %zu) exceeds the %zu resident bases", offset, offset + n, bases->n); return TRH_EINVAL; }
    if (n >= ((size_t)1 << 31)) { set_error("msm: n too large"); return TRH_EINVAL; }
    if (batch == 0) { set_error("msm: batch == 0"); return TRH_EINVAL; }
    return TRH_OK;
}

int msm_sharded(trh_bases* B, size_t offset, const void* scalars, bool scalars_on_host, size_t n, int mont, hipStream_t caller_stream, uint64_t* out) {
    Range range("trh_msm[sharded]");
    const size_t G = B->shards.size();
    int src_device = -1;
    hipEvent_t ready = nullptr;
    if (!scalars_on_host && n) {  // device scalars live where the caller's context is: the shards copy their range over xGMI once the caller's stream got there
        Enter en;
        TRH_TRY(en.begin(caller_stream));
        src_device = ctx().device;
        ready = ctx().order_ev;  // recorded below on caller_stream; the context stays locked until the shard streams were told to wait for it
        TRH_HIP_TRY(hipEventRecord(ready, caller_stream));
        for (size_t g = 0; g < G; ++g) TRH_HIP_TRY(hipStreamWaitEvent(B->shards[g]->owner->own_stream, ready, 0));
        en.outermost = false;  // order_ev was just recorded by hand
        ctx().last_stream = caller_stream; ctx().last_stream_valid = true;
    }
    // lock the shard contexts in group order (every sharded call takes them in this order), enqueue everywhere, then collect.
    // The scopes nest, so they are left in REVERSE order on every path (each ~Enter restores the active context and the HIP device
    // it found: front-to-back destruction left the calling thread on shard G - 2's device); a shard whose MSM was
    // enqueued but not collected (an error in between) gets its in-flight state cleared, or the context would answer TRH_EBUSY forever
    struct HeldScopes {
        std::vector<std::unique_ptr<Enter>> v;
        explicit HeldScopes(size_t n) : v(n) {}
        ~HeldScopes() {
            while (!v.empty()) {
                if (v.back() && v.back()->c && v.back()->c->msm.pending_curve >= 0) {
                    (void)hipStreamSynchronize(v.back()->c->own_stream);
                    v.back()->c->msm.pending_curve = -1;
                }
                v.pop_back();
            }
        }
        std::unique_ptr<Enter>& operator[](size_t i) { return v[i]; }
    } held(G);
    std::vector<uint64_t> partial(12 * G, 0);
    std::vector<ShardRange> rg(G);  // count 0: the shard holds nothing of the range
    auto src = [&](size_t g) { return (const char*)scalars + rg[g].at * 32; };
    size_t n_active = 0;
    for (size_t g = 0; g < G; ++g) {
        rg[g] = shard_range(B, g, offset, n);
        if (!rg[g].count) continue;
        Ctx* sc = B->shards[g]->owner;
        held[g].reset(new Enter());
        TRH_TRY(held[g]->begin(sc->own_stream, sc));
        TRH_TRY(sc->msm.scalars.ensure(rg[g].count * 32 + 32));
        if (scalars_on_host) TRH_TRY(stage_ensure(*sc));  // rings and copy threads exist before the uploader threads start
        ++n_active;
    }
    // Host scalars: ONE uploader thread per shard, each feeding its device through that context's own pinned ring and copy threads (the
    // G links of a node run in parallel; one thread's memcpy stream -- 60-85 GB/s -- would be the limit of eight 57 GB/s links: a 2^26
    // MSM over 8 GPUs spent ~30 ms uploading against ~9 ms of arithmetic).  The calling thread holds every shard context's
    // lock and touches none of their stages meanwhile; it joins uploader g before it enqueues shard g's MSM, so the MSM of shard g starts
    // while the ranges of the later shards are still crossing.  Caller memory that is page-locked goes to the DMA engines directly.
    struct Upload { std::thread th; int rc = TRH_OK; std::string err; };
    std::vector<Upload> up(scalars_on_host ? G : 0);
    const bool threaded = scalars_on_host && n_active > 1;
    auto join_all = [&] { for (Upload& u : up) if (u.th.joinable()) u.th.join(); };
    if (threaded) {
        for (size_t g = 0; g < G; ++g) {
            if (!rg[g].count) continue;
            Ctx* sc = B->shards[g]->owner;
            Upload* u = &up[g];
            const char* from = src(g);
            const size_t bytes = rg[g].count * 32;
            u->th = std::thread([sc, u, from, bytes] {
                if (hipSetDevice(sc->device) != hipSuccess) { u->rc = TRH_EHIP; u->err = "hipSetDevice failed in an upload thread"; return; }
                u->rc = stage_h2d(*sc, sc->msm.scalars.p, from, bytes, sc->own_stream);
                if (u->rc != TRH_OK) u->err = trh_last_error();
            });
        }
    }
    for (size_t g = 0; g < G; ++g) {
        if (!rg[g].count) continue;
        trh_bases* sh = B->shards[g];
        Ctx* sc = sh->owner;
        const size_t bytes = rg[g].count * 32;
        Enter en;
        int rc = en.begin(sc->own_stream, sc);  // re-entrant: the context is held above, this makes it the active one (and its device current) again
        if (rc == TRH_OK) {
            if (threaded) {
                up[g].th.join();
                if (up[g].rc != TRH_OK) { set_error("%s", up[g].err.c_str()); rc = up[g].rc; }
            } else if (scalars_on_host) {
                rc = stage_h2d(*sc, sc->msm.scalars.p, src(g), bytes, sc->own_stream);
            } else if (opt().force_no_peer || (!trh_group_peer_access() && src_device != sc->device)) {
                // no peer access in the group (or forced): through the destination context's pinned ring, stream-ordered on both devices
                rc = stage_d2d_via_host(*sc, sc->msm.scalars.p, sc->own_stream, src(g), src_device, caller_stream, bytes);
            } else if (src_device == sc->device) {
                if (hipMemcpyAsync(sc->msm.scalars.p, src(g), bytes, hipMemcpyDeviceToDevice, sc->own_stream) != hipSuccess) { set_error("msm[sharded]: device copy failed"); rc = TRH_EHIP; }
            } else {
                if (hipMemcpyPeerAsync(sc->msm.scalars.p, sc->device, src(g), src_device, bytes, sc->own_stream) != hipSuccess) { set_error("msm[sharded]: peer copy failed: %s", hipGetErrorString(hipGetLastError())); rc = TRH_EHIP; }
            }
        }
        if (rc == TRH_OK) {
            // no sparse vote on a shard: the sampler ends in a host synchronisation behind this shard's upload / hand-over, which
            // would hold back the enqueues of the later shards; a range-sharded MSM is a full-size one
            // (its own flag: dense_hint also selects the quad-lane combine, which is for callers that vouch for full-size scalars -- ADVICE r05)
            MsmFlags no_vote;
            no_vote.no_sparse_vote = true;
            rc = msm_launch(sh, rg[g].local, sc->msm.scalars.p, rg[g].count, 1, rg[g].count, mont, sc->own_stream, nullptr, no_vote);
        }
        if (rc != TRH_OK) { join_all(); return rc; }
    }
    size_t cntp = 0;
    for (size_t g = 0; g < G; ++g) {
        if (!rg[g].count) continue;
        Ctx* sc = B->shards[g]->owner;
        Enter en;
        TRH_TRY(en.begin(sc->own_stream, sc));  // re-entrant: the context is still held above, this makes it the active one again
        TRH_TRY(msm_finish(B->curve, sc->own_stream, partial.data() + 12 * cntp, 1));
        ++cntp;
    }
    return point_sum_host(B->curve, partial.data(), cntp, out);
}

}  // namespace

void bases_cache_clear() {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    for (trh_bases* h : g_cache.clear()) trh_bases_destroy(h);
}

// trh_msm_dev; the flags are the self-test's way to the pipeline and the quad combine at a size the small kernel would take
int msm_dev_flagged(trh_bases_t bases, size_t offset, const void* scalars_dev, size_t n, int mont, void* stream, uint64_t out[12], MsmFlags flags) {
    TRH_TRY(msm_args(bases, offset, scalars_dev, n, 1, out));
    if (!bases->shards.empty()) return msm_sharded(bases, offset, scalars_dev, false, n, mont, (hipStream_t)stream, out);
    TRH_ENTER(stream);
    Range range("trh_msm_dev");
    TRH_TRY(msm_ready(bases, "msm_dev"));
    TRH_TRY(msm_launch(bases, offset, scalars_dev, n, 1, n, mont, (hipStream_t)stream, nullptr, flags));
    return msm_finish(bases->curve, (hipStream_t)stream, out, 1);
}
}  // namespace trh

extern "C" {

int trh_best_multiexp_pallas(const uint64_t* coeffs, const uint64_t* bases, size_t n, uint64_t out[12]) { return best_multiexp_host(TRH_PALLAS, coeffs, bases, n, out); }
int trh_best_multiexp_vesta(const uint64_t* coeffs, const uint64_t* bases, size_t n, uint64_t out[12]) { return best_multiexp_host(TRH_VESTA, coeffs, bases, n, out); }

int trh_msm(trh_bases_t bases, size_t offset, const uint64_t* scalars_host, size_t n, int mont, uint64_t out[12]) {
    TRH_TRY(msm_args(bases, offset, scalars_host, n, 1, out));
    if (!bases->shards.empty()) return msm_sharded(bases, offset, scalars_host, true, n, mont, nullptr, out);
    TRH_ENTER(0);
    Range range("trh_msm");
    TRH_TRY(msm_ready(bases, "msm"));
    PendingGuard guard{ctx()};
    return msm_host_tiled(bases->curve, scalars_host, nullptr, bases, offset, n, mont, out);
}

/* Params::commit / commit_lagrange for `batch` polynomials in HOST memory (one pointer per column, n scalars each): the columns
 * cross PCIe in chunks, chunk j + 1 while the batched MSM of chunk j runs. */
int trh_commit_batch_host(trh_bases_t bases, const uint64_t* const* polys_host, size_t n, size_t batch, const uint64_t* blinds_host, uint64_t* out) {
    TRH_TRY(msm_args(bases, 0, polys_host, n + 1, batch, out));
    if (!blinds_host) { set_error("commit_batch: null blinds"); return TRH_EINVAL; }
    if (bases->n != n + 1) { set_error("commit_batch: the handle must hold n + 1 = %zu bases (g or g_lagrange followed by w), it holds %zu", n + 1, bases->n); return TRH_EINVAL; }
    for (size_t i = 0; i < batch; ++i) if (!polys_host[i]) { set_error("commit_batch_host: column %zu is null", i); return TRH_EINVAL; }
    TRH_ENTER(0);
    Range range("trh_commit_batch_host");
    TRH_TRY(msm_ready(bases, "commit_batch_host"));
    Ctx& c = ctx();
    PendingGuard guard{c};
    TRH_TRY(stage_begin(c));
    StageScope scope(c);
    Stage& st = c.stage;
    size_t chunk = 16;  // 2^18-row columns: 128 MiB and ~7 ms of MSM per chunk
    while (chunk > 1 && chunk * n * 32 > ((size_t)256 << 20)) chunk >>= 1;
    if (chunk > batch) chunk = batch;
    const size_t nchunks = (batch + chunk - 1) / chunk;
    for (size_t j = 0; j < nchunks; ++j) {
        const size_t slot = j & 1, first = j * chunk, nb = first + chunk <= batch ? chunk : batch - first;
        TRH_TRY(st.ring_in[slot].ensure(chunk * n * 32 + chunk * 32 + 32));
        char* const tails = (char*)st.ring_in[slot].p + chunk * n * 32;
        for (size_t i = 0; i < nb; ++i) TRH_TRY(stage_h2d(c, (char*)st.ring_in[slot].p + i * n * 32, polys_host[first + i], n * 32, st.us, true));
        TRH_TRY(stage_h2d(c, tails, blinds_host + 4 * first, nb * 32, st.us));
        TRH_HIP_TRY(hipEventRecord(st.ev_up[slot], st.us));
        if (j > 0) TRH_TRY(msm_finish(bases->curve, st.cs, out + 12 * (first - chunk), chunk));
        TRH_HIP_TRY(hipStreamWaitEvent(st.cs, st.ev_up[slot], 0));
        TRH_TRY(msm_launch(bases, 0, st.ring_in[slot].p, n + 1, nb, n, 1, st.cs, tails));
    }
    {
        const size_t first = (nchunks - 1) * chunk;
        TRH_TRY(msm_finish(bases->curve, st.cs, out + 12 * first, batch - first));
    }
    return scope.finish();
}

int trh_msm_dev_enqueue(trh_bases_t bases, size_t offset, const void* scalars_dev, size_t n, int mont, void* stream) {
    uint64_t dummy;
    TRH_TRY(msm_args(bases, offset, scalars_dev, n, 1, &dummy));
    TRH_ENTER(stream);
    Range range("trh_msm_dev_enqueue");
    TRH_TRY(single_device(bases, "msm_dev_enqueue"));
    if (ctx().msm.pending_curve >= 0) { set_error("msm_dev_enqueue: this context already has an MSM in flight (finish it, or use a second context: trh_ctx_create)"); return TRH_EBUSY; }
    TRH_TRY(msm_launch(bases, offset, scalars_dev, n, 1, n, mont, (hipStream_t)stream));
    ctx().msm.pending_owner = bases;
    return TRH_OK;
}
int trh_msm_dev_finish(trh_bases_t bases, void* stream, uint64_t out[12]) {
    if (!bases || !out) { set_error("msm_dev_finish: null pointer"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    Range range("trh_msm_dev_finish");
    if (ctx().msm.pending_curve < 0 || ctx().msm.pending_owner != (const void*)bases) { set_error("msm_dev_finish: no MSM over this base set is in flight on the calling context"); return TRH_EINVAL; }
    return msm_finish(bases->curve, (hipStream_t)stream, out, 1);
}
int trh_msm_dev(trh_bases_t bases, size_t offset, const void* scalars_dev, size_t n, int mont, void* stream, uint64_t out[12]) {
    return msm_dev_flagged(bases, offset, scalars_dev, n, mont, stream, out, MsmFlags{});
}
int trh_msm_batch_dev(trh_bases_t bases, size_t offset, const void* scalars_dev, size_t n, size_t batch, int mont, void* stream, uint64_t* out) {
    TRH_TRY(msm_args(bases, offset, scalars_dev, n, batch, out));
    TRH_ENTER(stream);
    Range range("trh_msm_batch_dev");
    TRH_TRY(msm_ready(bases, "msm_batch_dev"));
    TRH_TRY(msm_launch(bases, offset, scalars_dev, n, batch, n, mont, (hipStream_t)stream));
    return msm_finish(bases->curve, (hipStream_t)stream, out, batch);
}
/* Params::commit / commit_lagrange for `batch` polynomials resident on the device: item b is the MSM of
 * polys[b] (n scalars) || blinds[b] over the n + 1 bases of the handle (g or g_lagrange followed by w) */
int trh_commit_batch_dev(trh_bases_t bases, const void* polys_dev, size_t n, size_t batch, const uint64_t* blinds_host, void* stream, uint64_t* out) {
    TRH_TRY(msm_args(bases, 0, polys_dev, n + 1, batch, out));
    if (!blinds_host) { set_error("commit_batch: null blinds"); return TRH_EINVAL; }
    if (bases->n != n + 1) { set_error("commit_batch: the handle must hold n + 1 = %zu bases (g or g_lagrange followed by w), it holds %zu", n + 1, bases->n); return TRH_EINVAL; }
    TRH_ENTER(stream);
    Range range("trh_commit_batch_dev");
    TRH_TRY(msm_ready(bases, "commit_batch_dev"));
    Ctx& c = ctx();
    hipStream_t s = (hipStream_t)stream;
    TRH_TRY(c.msm.tails.ensure(batch * 32));
    TRH_HIP_TRY(hipMemcpyAsync(c.msm.tails.p, blinds_host, batch * 32, hipMemcpyHostToDevice, s));
    TRH_HIP_TRY(hipStreamSynchronize(s));  // the caller's blinds may be reused
    TRH_TRY(msm_launch(bases, 0, polys_dev, n + 1, batch, n, 1, s, c.msm.tails.p));
    return msm_finish(bases->curve, s, out, batch);
}

int trh_msm_set_window_bits(int cbits) {
    if (cbits != 0 && (cbits < 2 || cbits > 18)) { set_error("window bits must be 0 or in [2, 18]"); return TRH_EINVAL; }
    TRH_TRY(require_init());
    if (on_group_default()) {  // the group's shards follow the default context
        for (Ctx* g : device_group()) { std::lock_guard<std::recursive_mutex> lk(g->mu); g->window_override = cbits; }
        return TRH_OK;
    }
    Ctx* c = thread_ctx();
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    c->window_override = cbits;
    return TRH_OK;
}

}  // extern "C"
