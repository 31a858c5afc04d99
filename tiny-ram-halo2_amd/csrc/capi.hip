// Context layer of libtrh.so's C ABI (include/trh.h): error text, options, the context registry and the device group, timing and events.
// The entries themselves live with their subject: bases.hip, msmapi.hip, elemops.hip, devalloc.hip and the files of the larger operations.
#include <dlfcn.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <set>

#include "bases.h"
#include "hosthelper.h"
#define TRH_TRANSCRIPT_ABI  // the trh_tr_* entries (host only) are defined by the header itself
#include "transcript.h"

#ifndef TRH_BUILD_ID
#define TRH_BUILD_ID "unknown"
#endif

struct trh_ctx : trh::Ctx {};

namespace trh {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- options (ctx.h Options): environment once, then trh_set_option while no context exists ------------------------------
namespace {
Options g_opt;
std::once_flag g_opt_once;
std::mutex g_opt_mu;                 // serialises trh_set_option calls; readers need none (nothing writes while a context is alive)
std::atomic<int> g_live_ctx{0};      // contexts alive: while > 0 the options are fixed
struct OptField { const char* name; int kind; void* p; long lo, hi; };  // kind 0: int, 1: long
const OptField* opt_fields(size_t* count) {
    static const OptField f[] = {
        {"pool_mb", 1, &g_opt.pool_mb, 0, 1 << 20},          {"stage_slot_mb", 1, &g_opt.stage_slot_mb, 1, 256}, {"copy_threads", 0, &g_opt.copy_threads, -1, 64},
        {"bases_cache", 0, &g_opt.bases_cache, 0, 1},        {"force_no_peer", 0, &g_opt.force_no_peer, 0, 1},   {"ipa_fold", 0, &g_opt.ipa_fold, 0, 10},
        {"trace", 0, &g_opt.trace, 0, 3},                    {"msm_chunk_gb", 1, &g_opt.msm_chunk_gb, 1, 256},   {"sparse", 0, &g_opt.sparse, 0, 1},
        {"reduce_q4", 0, &g_opt.reduce_q4, 0, 1},            {"bin_sort", 0, &g_opt.bin_sort, 0, 1},             {"selftest", 0, &g_opt.selftest, 0, 1},
    };
    *count = sizeof(f) / sizeof(f[0]);
    return f;
}
bool opt_assign(const OptField& f, const char* value) {
    char* end = nullptr;
    const long v = strtol(value, &end, 10);
    if (end == value || *end != 0 || v < f.lo || v > f.hi) return false;
    if (f.kind == 0) *(int*)f.p = (int)v; else *(long*)f.p = v;
    return true;
}
void opt_load_env() {  // TRH_<NAME> for every field; a value out of range is ignored (the default stays)
    size_t n = 0;
    const OptField* f = opt_fields(&n);
    for (size_t i = 0; i < n; ++i) {
        char env[64] = "TRH_";
        size_t k = 4;
        for (const char* q = f[i].name; *q && k + 1 < sizeof(env); ++q) env[k++] = (char)(*q >= 'a' && *q <= 'z' ? *q - 32 : *q);
        env[k] = 0;
        if (const char* e = getenv(env)) (void)opt_assign(f[i], e);
    }
}
}  // namespace
const Options& opt() {
    std::call_once(g_opt_once, opt_load_env);
    return g_opt;
}

// ---- context registry ------------------------------------------------------------------------------------------------
static std::mutex g_reg_mu;
static Ctx* g_default = nullptr;            // trh_init / trh_init_multi
static std::vector<Ctx*> g_group;           // trh_init_multi: g_group[0] == g_default
static size_t g_shard_min = (size_t)1 << 20;  // smaller base sets stay on the default device
static int g_peer_ok = 1;                     // every pair of distinct group devices has peer access enabled
static thread_local Ctx* t_bound = nullptr;   // trh_ctx_set_current
static thread_local Ctx* t_active = nullptr;  // innermost TRH_ENTER

Ctx* thread_ctx() { return t_bound ? t_bound : g_default; }
const std::vector<Ctx*>& device_group() { return g_group; }
bool on_group_default() { return g_group.size() > 1 && thread_ctx() == g_default; }
bool use_group(size_t n) { return on_group_default() && n >= g_shard_min; }

Ctx& ctx() {
    Ctx* c = t_active ? t_active : thread_ctx();
    if (!c) {  // unreachable through the C ABI (every entry point enters first); keep the failure loud
        fprintf(stderr, "libtrh: internal error: ctx() without a context\n");
        abort();
    }
    return *c;
}

static int usable(const Ctx* c) {
    if (c && c->inited) return TRH_OK;
    set_error("trh_init() has not succeeded: no HIP device bound (libtrh has no CPU fallback)");
    return TRH_ENODEV;
}
int require_init() { return usable(t_active ? t_active : thread_ctx()); }

int Enter::begin(hipStream_t stream, Ctx* explicit_ctx) {
    Ctx* cc = explicit_ctx ? explicit_ctx : thread_ctx();
    TRH_TRY(usable(cc));
    cc->mu.lock();
    locked = true;
    c = cc;
    prev_active = t_active;
    t_active = cc;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != cc->device) {  // hipSetDevice is per thread: a rayon worker never called trh_init
        prev_device = cur;
        TRH_HIP_TRY(hipSetDevice(cc->device));
    }
    if (prev_active != cc) {  // outermost entry into this context
        if (cc->last_stream_valid && cc->last_stream != stream) TRH_HIP_TRY(hipStreamWaitEvent(stream, cc->order_ev, 0));
        entered_stream = stream;
        outermost = true;
    }
    return TRH_OK;
}

Enter::~Enter() {
    if (!locked) return;
    if (outermost) {  // whatever this call enqueued is what the next stream entering the context has to wait for
        if (hipEventRecord(c->order_ev, entered_stream) == hipSuccess) { c->last_stream = entered_stream; c->last_stream_valid = true; }
        else c->last_stream_valid = false;
    }
    if (prev_device >= 0) (void)hipSetDevice(prev_device);
    t_active = prev_active;
    c->mu.unlock();
}

// ---- roctx ranges (rocprofv3 --marker-trace): resolved at first use, absent library = no-op -----------------------------
namespace {
typedef int (*roctx_push_fn)(const char*);
typedef int (*roctx_pop_fn)(void);
roctx_push_fn g_roctx_push = nullptr;
roctx_pop_fn g_roctx_pop = nullptr;
std::once_flag g_roctx_once;
void roctx_resolve() {
    void* h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return;
    g_roctx_push = (roctx_push_fn)dlsym(h, "roctxRangePushA");
    g_roctx_pop = (roctx_pop_fn)dlsym(h, "roctxRangePop");
    if (!g_roctx_push || !g_roctx_pop) { g_roctx_push = nullptr; g_roctx_pop = nullptr; }
}
}  // namespace
Range::Range(const char* name) {
    std::call_once(g_roctx_once, roctx_resolve);
    if (g_roctx_push) g_roctx_push(name);
}
Range::~Range() {
    if (g_roctx_pop) g_roctx_pop();
}

static int create_ctx(int device, Ctx** out) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { set_error("no HIP device (%s)", e == hipSuccess ? "count 0" : hipGetErrorString(e)); return TRH_ENODEV; }
    if (device < 0 || device >= n) { set_error("device %d out of range [0, %d)", device, n); return TRH_EINVAL; }
    hipDeviceProp_t prop;
    TRH_HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) { set_error("device %d is %s, libtrh is built for gfx950 only", device, prop.gcnArchName); return TRH_ENODEV; }
    DeviceScope on(device);
    if (on.err != hipSuccess) { set_error("hipSetDevice(device) failed: %s (%s:%d)", hipGetErrorString(on.err), __FILE__, __LINE__); return TRH_EHIP; }
    trh_ctx* h = new trh_ctx();
    Ctx* c = h;
    c->device = device;
    hipError_t e1 = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    hipError_t e2 = hipEventCreateWithFlags(&c->order_ev, hipEventDisableTiming);
    if (e1 != hipSuccess || e2 != hipSuccess) { delete h; set_error("context creation failed: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2)); return TRH_EHIP; }
    c->inited = true;
    g_live_ctx.fetch_add(1);
    *out = c;
    return TRH_OK;
}

static void destroy_ctx(Ctx* c) {
    if (!c) return;
    {
        Enter en;
        if (en.begin(nullptr, c) == TRH_OK) {
            (void)hipDeviceSynchronize();
            msm_release();
            lookup_release();
            ntt_release_tables();
            encoding_release();
            hashtocurve_release();
            c->ipa.release();
            c->io.release();
            stage_release(*c);
            c->factors.release();
            if (c->pinned_ring) { (void)hipHostFree(c->pinned_ring); c->pinned_ring = nullptr; c->pinned_slot = 0; }
            c->verdict.dev.release();  // the verdict words and where they land
            c->exechips_flag2.release();
            if (c->pinned_land) { (void)hipHostFree(c->pinned_land); c->pinned_land = nullptr; c->pinned_land_cap = 0; }
            c->pfft.release();
            c->scan.release(); c->scan2.release();
            c->last_stream_valid = false;
            en.outermost = false;  // nothing to order behind: the streams are drained
        }
    }
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c->helper; c->helper = nullptr;
    if (c->order_ev) (void)hipEventDestroy(c->order_ev);
    c->inited = false;
    if (t_bound == c) t_bound = nullptr;
    delete static_cast<trh_ctx*>(c);
    g_live_ctx.fetch_sub(1);
}

// selftest.hip: the known-answer test of the device arithmetic, once per device and process, on the context just created (made current
// for the calling thread while it runs).  On a mismatch the caller destroys the context and returns TRH_ESELFTEST.
int selftest_run();
static std::mutex g_selftest_mu;
static std::set<int> g_selftest_done;
static int selftest_once(Ctx* c) {
    if (!opt().selftest) return TRH_OK;
    std::lock_guard<std::mutex> lk(g_selftest_mu);
    if (g_selftest_done.count(c->device)) return TRH_OK;
    Ctx* prev = t_bound;
    t_bound = c;
    const int rc = selftest_run();
    t_bound = prev;
    if (rc == TRH_OK) g_selftest_done.insert(c->device);
    return rc;
}
// the calling thread's error text once more, behind "<name>: " (null: as it is), after `doomed` is destroyed -- which may replace the text
static void prefix_error(const char* name, Ctx* doomed = nullptr) {
    char msg[512];
    snprintf(msg, name ? 400 : sizeof(msg), "%s", g_err);
    destroy_ctx(doomed);
    if (name) set_error("%s: %s", name, msg); else set_error("%s", msg);
}
// create_ctx + self-test; a context that fails it never reaches the caller
static int create_checked_ctx(int device, Ctx** out) {
    Ctx* c = nullptr;
    TRH_TRY(create_ctx(device, &c));
    const int rc = selftest_once(c);
    if (rc != TRH_OK) { prefix_error(nullptr, c); return rc; }
    *out = c;
    return TRH_OK;
}

int check_curve(int curve) {
    if (curve != TRH_PALLAS && curve != TRH_VESTA) { set_error("unknown curve id %d", curve); return TRH_EINVAL; }
    return TRH_OK;
}
int check_field(int field) {
    if (field != TRH_FP && field != TRH_FQ) { set_error("unknown field id %d", field); return TRH_EINVAL; }
    return TRH_OK;
}

// TRH_FORCE_NO_PEER=1: the group behaves as if no pair of devices had peer access -- trh_init_multi enables none, and device-resident
// scalars reach EVERY shard (the one on the source device included) through the pinned-host hand-over that a box without peer access
// takes (msmapi.hip msm_sharded).  For exercising that path on a one-GPU box ({0, 0} groups).
static bool force_no_peer() { return opt().force_no_peer != 0; }

}  // namespace trh

using namespace trh;

extern "C" {

const char* trh_version(void) { return "trh 0.2.0 (gfx950, build " TRH_BUILD_ID ")"; }
const char* trh_last_error(void) { return g_err; }

int trh_set_option(const char* name, const char* value) {
    if (!name || !value) { set_error("trh_set_option: null pointer"); return TRH_EINVAL; }
    std::lock_guard<std::mutex> lk(g_opt_mu);
    (void)opt();  // the environment first: an explicit call overrides it
    if (g_live_ctx.load() > 0) { set_error("trh_set_option(%s): options are fixed while a context exists (call it before trh_init, or after trh_shutdown)", name); return TRH_EBUSY; }
    size_t n = 0;
    const OptField* f = opt_fields(&n);
    for (size_t i = 0; i < n; ++i)
        if (strcmp(f[i].name, name) == 0) {
            if (!opt_assign(f[i], value)) { set_error("trh_set_option(%s): value '%s' is not an integer in [%ld, %ld]", name, value, f[i].lo, f[i].hi); return TRH_EINVAL; }
            return TRH_OK;
        }
    set_error("trh_set_option: unknown option '%s'", name);
    return TRH_EINVAL;
}
int trh_get_option(const char* name, long* value) {
    if (!name || !value) { set_error("trh_get_option: null pointer"); return TRH_EINVAL; }
    (void)opt();
    size_t n = 0;
    const OptField* f = opt_fields(&n);
    for (size_t i = 0; i < n; ++i)
        if (strcmp(f[i].name, name) == 0) { *value = f[i].kind == 0 ? (long)*(int*)f[i].p : *(long*)f[i].p; return TRH_OK; }
    set_error("trh_get_option: unknown option '%s'", name);
    return TRH_EINVAL;
}

int trh_device_count(void) { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }

int trh_init(int device) {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    if (g_default) {
        if (g_default->device == device) return TRH_OK;
        set_error("trh_init: already bound to device %d", g_default->device);
        return TRH_EINVAL;
    }
    Ctx* c = nullptr;
    int rc = create_checked_ctx(device, &c);
    if (rc != TRH_OK) { prefix_error("trh_init"); return rc; }
    g_default = c;
    g_group.assign(1, c);
    return TRH_OK;
}

int trh_init_multi(const int* devices, int n_devices) {
    if (!devices || n_devices < 1 || n_devices > 64) { set_error("trh_init_multi: bad arguments"); return TRH_EINVAL; }
    std::lock_guard<std::mutex> lk(g_reg_mu);
    if (g_default) {
        bool same = g_group.size() == (size_t)n_devices;
        for (int i = 0; same && i < n_devices; ++i) same = g_group[i]->device == devices[i];
        if (same) return TRH_OK;
        // after a plain trh_init(devices[0]) the group grows around the existing default context
        if (g_group.size() != 1 || g_default->device != devices[0]) {
            set_error("trh_init_multi: already initialised with another device list (trh_shutdown first)");
            return TRH_EINVAL;
        }
    }
    std::vector<Ctx*> made;
    if (g_default) made.push_back(g_default);
    for (int i = (int)made.size(); i < n_devices; ++i) {  // the same device may be listed more than once: two lanes on one GPU
        Ctx* c = nullptr;
        const int rc = create_checked_ctx(devices[i], &c);
        if (rc != TRH_OK) {
            for (Ctx* m : made) if (m != g_default) destroy_ctx(m);
            prefix_error("trh_init_multi");
            return rc;
        }
        made.push_back(c);
    }
    // peer access for the hand-over of device-resident scalars.  Not fatal when it cannot be had (msm_sharded then hands the
    // ranges over through pinned host memory, stage_d2d_via_host), but not silent either: trh_group_peer_access() reports it and trh_last_error() names the first pair
    g_peer_ok = 1;
    if (force_no_peer()) {
        g_peer_ok = 0;
        set_error("trh_init_multi: TRH_FORCE_NO_PEER=1: no peer access enabled; device-resident scalars are handed over through pinned host memory");
    }
    for (int i = 0; i < n_devices && !force_no_peer(); ++i)
        for (int j = 0; j < n_devices; ++j)
            if (devices[i] != devices[j]) {
                int can = 0;
                hipError_t e = hipDeviceCanAccessPeer(&can, devices[i], devices[j]);
                if (e == hipSuccess && can) {
                    DeviceScope on(devices[i]);
                    e = on.err;
                    if (e == hipSuccess) {
                        e = hipDeviceEnablePeerAccess(devices[j], 0);
                        if (e == hipErrorPeerAccessAlreadyEnabled) { (void)hipGetLastError(); e = hipSuccess; }
                    }
                }
                if (e != hipSuccess || !can) {
                    if (g_peer_ok) set_error("trh_init_multi: no peer access from device %d to device %d (%s); device-resident scalars will be staged through the host",
                                             devices[i], devices[j], e != hipSuccess ? hipGetErrorString(e) : "hipDeviceCanAccessPeer says no");
                    (void)hipGetLastError();
                    g_peer_ok = 0;
                }
            }
    g_group = made;
    g_default = made[0];
    return TRH_OK;
}
int trh_group_size(void) { return (int)g_group.size(); }
int trh_group_peer_access(void) { return g_peer_ok; }
int trh_set_shard_min(size_t n_pairs) { g_shard_min = n_pairs ? n_pairs : 1; return TRH_OK; }

void trh_shutdown(void) {
    bases_cache_clear();  // before the registry lock: destroying a cached set enters its context
    pool_trim();
    std::lock_guard<std::mutex> lk(g_reg_mu);
    for (Ctx* c : g_group) destroy_ctx(c);
    g_group.clear();
    g_default = nullptr;
}

int trh_ctx_create(int device, trh_ctx_t* out) {
    if (!out) { set_error("ctx_create: null pointer"); return TRH_EINVAL; }
    Ctx* c = nullptr;
    TRH_TRY(create_checked_ctx(device, &c));
    *out = static_cast<trh_ctx*>(c);
    return TRH_OK;
}
void trh_ctx_destroy(trh_ctx_t c) { destroy_ctx(c); }
int trh_ctx_set_current(trh_ctx_t c) {
    if (c && !c->inited) { set_error("ctx_set_current: destroyed context"); return TRH_EINVAL; }
    t_bound = c;
    return TRH_OK;
}
void* trh_ctx_stream(trh_ctx_t c) {
    Ctx* cc = c ? (Ctx*)c : thread_ctx();
    return cc ? (void*)cc->own_stream : nullptr;
}
int trh_ctx_device(trh_ctx_t c) {
    Ctx* cc = c ? (Ctx*)c : thread_ctx();
    return cc ? cc->device : -1;
}

int trh_memcpy_h2d(void* dev, const void* host, size_t bytes) {
    TRH_ENTER(0);
    TRH_HIP_TRY(hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice));
    return TRH_OK;
}
int trh_memcpy_d2h(void* host, const void* dev, size_t bytes) {
    TRH_ENTER(0);
    TRH_HIP_TRY(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
    return TRH_OK;
}
int trh_stream_synchronize(void* stream) {
    TRH_ENTER(stream);
    TRH_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return TRH_OK;
}

/* GPU-side timing for hosts without a HIP toolchain of their own (the Rust shim, examples/replay.cpp): events recorded on a stream between
 * the steps, read afterwards -- the time the device spent, without a host synchronisation (and the idle gap and clock ramp it causes)
 * between the steps */
int trh_event_create(void** out) {
    if (!out) { set_error("event_create: null pointer"); return TRH_EINVAL; }
    TRH_ENTER(0);
    hipEvent_t e = nullptr;
    TRH_HIP_TRY(hipEventCreate(&e));
    *out = (void*)e;
    return TRH_OK;
}
int trh_event_record(void* event, void* stream) {
    if (!event) { set_error("event_record: null event"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    TRH_HIP_TRY(hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
    return TRH_OK;
}
int trh_event_elapsed_ms(void* start, void* end, float* ms) {
    if (!start || !end || !ms) { set_error("event_elapsed_ms: null pointer"); return TRH_EINVAL; }
    TRH_TRY(require_init());
    TRH_HIP_TRY(hipEventSynchronize((hipEvent_t)end));
    TRH_HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)end));
    return TRH_OK;
}
void trh_event_destroy(void* event) {
    if (event) (void)hipEventDestroy((hipEvent_t)event);
}

int trh_stat(const char* name, uint64_t* value) {
    if (!name || !value) { set_error("trh_stat: null pointer"); return TRH_EINVAL; }
    TRH_ENTER(0);
    const Ctx& c = ctx();
    const MsmScratch& m = c.msm;
    const struct { const char* name; uint64_t value; } counters[] = {
        {"msm_lean_retries", m.lean_retries}, {"msm_lean_sorts", m.lean_sorts}, {"msm_quad_combines", m.quad_combines}, {"msm_small_launches", m.small_launches}, {"msm_chunks", m.chunks}, {"msm_unit_chunks", m.unit_chunks},
        {"msm_host_ranges", m.host_ranges}, {"msm_range_tiles", m.range_tiles}, {"ntt_tableless_passes", c.ntt_tableless_passes},
        {"ipa_generator_collapses", c.ipa.collapses}, {"lookup_check_probes", c.lookup_check_probes},
        {"memtable_rows", c.memtable_rows}, {"memtable_sort_passes", c.memtable_sort_passes}, {"memtable_tiles", c.memtable_tiles},
        {"exetable_rows", c.exetable_rows}, {"exechips_rows", c.exechips_rows}};
    for (const auto& k : counters) if (strcmp(name, k.name) == 0) { *value = k.value; return TRH_OK; }
    if (strcmp(name, "msm_bin_sorted_windows") == 0) {  // synchronises the device: tests only
        *value = 0;
        if (!m.sort_flags) return TRH_OK;
        std::vector<u32> flags(m.sort_flag_count);
        TRH_HIP_TRY(hipDeviceSynchronize());
        TRH_HIP_TRY(hipMemcpy(flags.data(), m.sort_flags, flags.size() * 4, hipMemcpyDeviceToHost));
        for (u32 k = 0; k < m.sort_flag_count; ++k) *value += flags[k] == 0u;
        return TRH_OK;
    }
    if (strcmp(name, "exechips_flag2_rows") == 0) {  // synchronises the device: tests only
        *value = 0;
        if (!c.exechips_flag2.p) return TRH_OK;
        TRH_HIP_TRY(hipDeviceSynchronize());
        TRH_HIP_TRY(hipMemcpy(value, c.exechips_flag2.p, 8, hipMemcpyDeviceToHost));
        return TRH_OK;
    }
    set_error("trh_stat: unknown counter '%s'", name);
    return TRH_EINVAL;
}

int trh_set_timing(int enabled) {
    TRH_TRY(require_init());
    Ctx* c = thread_ctx();
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    c->timing = enabled;
    return TRH_OK;
}
int trh_last_timing(trh_timing_t* out) {
    if (!out) { set_error("last_timing: null pointer"); return TRH_EINVAL; }
    TRH_TRY(require_init());
    Ctx* c = thread_ctx();
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    *out = c->last;
    return TRH_OK;
}

}  // extern "C"
