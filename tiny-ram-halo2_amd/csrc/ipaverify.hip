// The arithmetic of the IPA verifier's accumulator: halo2_proofs 0.2.0 `poly::commitment::msm::MSM` and
// `poly::commitment::verifier::Guard::use_challenges` (reached from `plonk::verify_proof` / `BatchVerifier::finalize` after the
// proofs are made -- reference call site /root/reference/src/test_utils.rs:52-68).  The verifier's orchestration (transcript,
// challenges, compute_b, the multiopen verifier) stays on the host; this file holds the accumulator (trh_ipa_msm_t):
//   g_scalars   2^k scalars, resident here, optional as in msm.rs (None until add_constant_term / add_to_g_scalars / use_challenges)
//   w, u        one scalar each, on the host until eval
//   other       the appended (scalar, point) terms: S, L_j, R_j, the multiopen commitments
// use_challenges for P guards in ONE pass over the 2^k vector:
//   g[i] = alpha g[i] + sum_p weight_p neg_c_p prod_{j : bit (k - 1 - j) of i set} u_{p, j}          (compute_s's convention)
// P = 1 with alpha = weight = 1 is Guard::use_challenges; general P is BatchVerifier's scale(r) / add_msm chain, expanded.
// The products come from two tables per proof, over the low L = floor(k / 2) and the high H = ceil(k / 2) index bits
// (weight_p neg_c_p folded into the high one): one multiplication and one addition per element and proof.
// eval: ONE full-range MSM over the resident g || w [|| u] set through trh_msm_dev (fixed-base tables when attached), the appended
// terms through the existing small MSM (trh_best_multiexp_*), the points added on the host.
#include <string.h>

#include <vector>

#include "bases.h"
#include "devmem.h"

struct trh_ipa_msm {
    int curve;
    uint32_t k;
    size_t n;                 // 2^k
    trh_bases* set;           // g || w (n + 1 points) or g || w || u (n + 2)
    bool set_has_u;
    trh::Ctx* owner;          // the context that created it: every call must come from it (the buffers below are ordered by its streams)
    uint64_t u_xy[8], w_xy[8];
    trh::DevBuf scalars;      // set->n scalars: g [0, n), then the slots of w (and u) that eval writes
    bool has_g = false;
    uint64_t w_scalar[4] = {0, 0, 0, 0}, u_scalar[4] = {0, 0, 0, 0};
    std::vector<uint64_t> other_scalars, other_bases;  // 4 / 8 words per appended term
    trh::DevBuf tables;       // use_challenges: per proof 2^L low entries, then 2^H high entries
    trh::DevBuf params;       // use_challenges: count x k challenges, then count coefficients (weight neg_c)
    void* pinned = nullptr;   // host side of `params` (its last upload is `up_ev`)
    size_t pinned_cap = 0;
    hipEvent_t up_ev = nullptr;
    bool up_pending = false;
    hipStream_t stream = nullptr;  // the stream of the last call that named one: add_constant_term (no stream argument) enqueues there
};

namespace trh {
namespace {

struct Const1 { uint4 w[2]; };  // one scalar as a kernel argument
template <class F>
__device__ __forceinline__ Fe<F> ldc(const Const1& c) { return fe_load<F>(c.w[0].x, c.w[0].y, c.w[0].z, c.w[0].w, c.w[1].x, c.w[1].y, c.w[1].z, c.w[1].w); }

// tables of proof p = blockIdx.y: entry e < 2^L is prod over the set bits b of e of u[k - 1 - b] (the low index bits), entry 2^L + t is
// coef prod over the set bits b of t of u[k - 1 - (L + b)] (the high ones).  At most 13 multiplications per entry (k <= 26).
template <class F>
__global__ void __launch_bounds__(256) verify_tables_kernel(const uint4* __restrict__ u, const uint4* __restrict__ coef, u32 k, u32 lbits, u32 count,
                                                            uint4* __restrict__ tables) {
    const u32 p = blockIdx.y;
    const u32 lo_n = 1u << lbits, hbits = k - lbits, entries = lo_n + (1u << hbits);
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= count || e >= entries) return;
    const uint4* up = u + 2 * (size_t)p * k;
    const bool hi = e >= lo_n;
    const u32 t = hi ? e - lo_n : e, nb = hi ? hbits : lbits, shift = hi ? lbits : 0;
    Fe<F> r = hi ? load_fe<F>(coef + 2 * p) : fe_one<F>();
    for (u32 b = 0; b < nb; ++b)
        if ((t >> b) & 1u) r = fe_mul(r, load_fe<F>(up + 2 * (k - 1 - (shift + b))));
    store_fe<F>(tables + 2 * ((size_t)p * entries + e), r);
}

// g[i] = alpha g[i] + sum_p hi_p[i >> L] lo_p[i & (2^L - 1)] over [blockIdx.x * span, + span).  LDS: the low tables of all proofs are
// staged once per workgroup (the table entries a thread reads per element; the high entry is the same for 2^L consecutive i) when they
// fit the budget; otherwise they are read through L1 / L2, where every workgroup finds them.
// fresh: there is no g yet (msm.rs: g_scalars == None): written without being read; unit_alpha: no multiplication by alpha.
template <class F, bool LDS>
__global__ void __launch_bounds__(256) verify_apply_kernel(uint4* __restrict__ g, size_t n, u32 lbits, u32 count, const uint4* __restrict__ tables,
                                                           size_t span, int fresh, int unit_alpha, const Const1 alpha) {
    extern __shared__ uint4 lds_lo[];
    const u32 lo_n = 1u << lbits;
    const size_t entries = (size_t)lo_n + (n >> lbits);
    if (LDS) {
        for (u32 x = threadIdx.x; x < count * lo_n; x += blockDim.x) {
            const u32 p = x >> lbits, e = x & (lo_n - 1);
            const uint4* src = tables + 2 * ((size_t)p * entries + e);
            lds_lo[2 * x] = src[0];
            lds_lo[2 * x + 1] = src[1];
        }
        __syncthreads();
    }
    const size_t begin = (size_t)blockIdx.x * span;
    const size_t end = begin + span < n ? begin + span : n;
    for (size_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
        const u32 lo = (u32)(i & (lo_n - 1));
        const size_t hi = i >> lbits;
        Fe<F> acc = fe_zero<F>();
        for (u32 p = 0; p < count; ++p) {
            const uint4* tp = tables + 2 * (size_t)p * entries;
            const Fe<F> l = LDS ? load_fe<F>(lds_lo + 2 * ((size_t)p * lo_n + lo)) : load_fe<F>(tp + 2 * lo);
            acc = fe_add(acc, fe_mul(load_fe<F>(tp + 2 * (lo_n + hi)), l));
        }
        if (!fresh) {
            const Fe<F> old = load_fe<F>(g + 2 * i);
            acc = fe_add(acc, unit_alpha ? old : fe_mul(old, ldc<F>(alpha)));
        }
        store_fe<F>(g + 2 * i, acc);
    }
}

// MSM::scale on the g vector: g[i] *= f
template <class F>
__global__ void __launch_bounds__(256) verify_scale_kernel(uint4* __restrict__ g, size_t n, const Const1 f) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    store_fe<F>(g + 2 * i, fe_mul(load_fe<F>(g + 2 * i), ldc<F>(f)));
}
// MSM::add_to_g_scalars / add_msm: g[i] += h[i]
template <class F>
__global__ void __launch_bounds__(256) verify_add_kernel(uint4* __restrict__ g, const uint4* __restrict__ h, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    store_fe<F>(g + 2 * i, fe_add(load_fe<F>(g + 2 * i), load_fe<F>(h + 2 * i)));
}
// MSM::add_constant_term: g[0] += c
template <class F>
__global__ void verify_add_constant_kernel(uint4* __restrict__ g, const Const1 c) {
    if (threadIdx.x == 0) store_fe<F>(g, fe_add(load_fe<F>(g), ldc<F>(c)));
}

// the low tables go to LDS up to this size: two workgroups of the apply kernel per CU (160 KiB of LDS each)
constexpr size_t LDS_BUDGET = 64 * 1024;

Const1 const1(const uint64_t* v) {
    Const1 c;
    memcpy(&c, v, 32);
    return c;
}
unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

// host-side scalar arithmetic on 4 x u64 Montgomery words
template <class SF>
void host_mul(const uint64_t* a, const uint64_t* b, uint64_t* out) {
    FeMem x, y, r;
    memcpy(&x, a, 32); memcpy(&y, b, 32);
    fe_store(fe_mul(fe_load<SF>(x), fe_load<SF>(y)), r);
    memcpy(out, &r, 32);
}
template <class SF>
void host_add(uint64_t* acc, const uint64_t* b) {
    FeMem x, y, r;
    memcpy(&x, acc, 32); memcpy(&y, b, 32);
    fe_store(fe_add(fe_load<SF>(x), fe_load<SF>(y)), r);
    memcpy(acc, &r, 32);
}
void smul(int curve, const uint64_t* a, const uint64_t* b, uint64_t* out) {  // scalars of `curve`: pallas -> Fq, vesta -> Fp
    with_curve(curve, [&](auto cv) { host_mul<typename decltype(cv)::Scalar>(a, b, out); });
}
void sadd(int curve, uint64_t* acc, const uint64_t* b) {
    with_curve(curve, [&](auto cv) { host_add<typename decltype(cv)::Scalar>(acc, b); });
}
bool is_one_mont(int curve, const uint64_t* v) {
    FeMem one;
    with_curve(curve, [&](auto cv) { fe_store(fe_one<typename decltype(cv)::Scalar>(), one); });
    return memcmp(&one, v, 32) == 0;
}

// creates the g vector (all zero) when the accumulator has none yet
int ensure_g(trh_ipa_msm* m, hipStream_t s) {
    if (m->has_g) return TRH_OK;
    TRH_HIP_TRY(hipMemsetAsync(m->scalars.p, 0, m->n * 32, s));
    m->has_g = true;
    return TRH_OK;
}

// g += src (2^k scalars in device memory), or g = src when there is no g yet
int add_g(trh_ipa_msm* m, const void* src, hipStream_t s) {
    if (!m->has_g) {
        TRH_HIP_TRY(hipMemcpyAsync(m->scalars.p, src, m->n * 32, hipMemcpyDeviceToDevice, s));
        m->has_g = true;
        return TRH_OK;
    }
    with_curve(m->curve, [&](auto cv) { hipLaunchKernelGGL((verify_add_kernel<typename decltype(cv)::Scalar>), dim3(blocks_of(m->n)), dim3(256), 0, s, (uint4*)m->scalars.p, (const uint4*)src, m->n); });
    TRH_HIP_TRY(hipGetLastError());
    return TRH_OK;
}

int scale_g(trh_ipa_msm* m, const uint64_t* f, hipStream_t s) {
    if (!m->has_g) return TRH_OK;
    with_curve(m->curve, [&](auto cv) { hipLaunchKernelGGL((verify_scale_kernel<typename decltype(cv)::Scalar>), dim3(blocks_of(m->n)), dim3(256), 0, s, (uint4*)m->scalars.p, m->n, const1(f)); });
    TRH_HIP_TRY(hipGetLastError());
    return TRH_OK;
}

// host_params: count x k challenges, then count coefficients weight_p neg_c_p (Montgomery words)
template <class SF>
int use_challenges_t(trh_ipa_msm* m, size_t count, const uint64_t* host_params, const uint64_t* alpha, hipStream_t s) {
    const uint32_t k = m->k, lbits = k / 2, hbits = k - lbits;
    const size_t lo_n = (size_t)1 << lbits, entries = lo_n + ((size_t)1 << hbits);
    const size_t pbytes = count * (k + 1) * 32;
    TRH_TRY(m->params.ensure(pbytes));
    TRH_TRY(m->tables.ensure(count * entries * 32));
    // the challenges go up through a pinned buffer of the accumulator: its previous upload has to be complete before it is refilled
    if (m->up_pending) { TRH_HIP_TRY(hipEventSynchronize(m->up_ev)); m->up_pending = false; }
    if (m->pinned_cap < pbytes) {
        if (m->pinned) { (void)hipHostFree(m->pinned); m->pinned = nullptr; m->pinned_cap = 0; }
        TRH_HIP_TRY(hipHostMalloc(&m->pinned, pbytes, hipHostMallocDefault));
        m->pinned_cap = pbytes;
    }
    if (!m->up_ev) TRH_HIP_TRY(hipEventCreateWithFlags(&m->up_ev, hipEventDisableTiming));
    memcpy(m->pinned, host_params, pbytes);
    TRH_HIP_TRY(hipMemcpyAsync(m->params.p, m->pinned, pbytes, hipMemcpyHostToDevice, s));
    TRH_HIP_TRY(hipEventRecord(m->up_ev, s));
    m->up_pending = true;
    const uint4* d_u = m->params.as<uint4>();
    const uint4* d_coef = d_u + 2 * count * k;
    for (size_t p0 = 0; p0 < count; p0 += 65535) {  // grid.y limit
        const u32 pc = (u32)(count - p0 < 65535 ? count - p0 : 65535);
        hipLaunchKernelGGL((verify_tables_kernel<SF>), dim3(blocks_of(entries), pc), dim3(256), 0, s, d_u + 2 * p0 * k, d_coef + 2 * p0, k, lbits, pc,
                           m->tables.as<uint4>() + 2 * p0 * entries);
    }
    TRH_HIP_TRY(hipGetLastError());
    const int fresh = m->has_g ? 0 : 1;
    const int unit_alpha = (!alpha || is_one_mont(m->curve, alpha)) ? 1 : 0;
    const Const1 a = unit_alpha ? Const1{} : const1(alpha);
    const size_t lds = count * lo_n * 32;
    if (lds <= LDS_BUDGET) {
        // a workgroup covers `span` consecutive elements: up to 2 * 2^L (each staged entry read twice or more) while at least 256
        // workgroups remain (one per CU)
        size_t span = 256;
        while (span < 2 * lo_n && m->n / (2 * span) >= 256) span *= 2;
        hipLaunchKernelGGL((verify_apply_kernel<SF, true>), dim3((unsigned)((m->n + span - 1) / span)), dim3(256), lds, s, (uint4*)m->scalars.p, m->n, lbits,
                           (u32)count, m->tables.as<uint4>(), span, fresh, unit_alpha, a);
    } else {
        hipLaunchKernelGGL((verify_apply_kernel<SF, false>), dim3(blocks_of(m->n)), dim3(256), 0, s, (uint4*)m->scalars.p, m->n, lbits, (u32)count,
                           m->tables.as<uint4>(), (size_t)256, fresh, unit_alpha, a);
    }
    TRH_HIP_TRY(hipGetLastError());
    m->has_g = true;
    return TRH_OK;
}

int check_msm(trh_ipa_msm* m, const char* what) {
    if (&ctx() != m->owner) { set_error("%s: the accumulator belongs to another context than the calling thread's", what); return TRH_EINVAL; }
    return TRH_OK;
}

}  // namespace
}  // namespace trh

using namespace trh;

extern "C" {

int trh_ipa_msm_create(trh_bases_t g_w_u, uint32_t k, const uint64_t u_xy[8], trh_ipa_msm_t* out) {
    TRH_TRY(require_init());
    if (!g_w_u || !u_xy || !out) { set_error("ipa_msm_create: null pointer"); return TRH_EINVAL; }
    if (k == 0 || k > 26) { set_error("ipa_msm_create: k = %u is outside 1 .. 26", k); return TRH_EINVAL; }
    const size_t n = (size_t)1 << k;
    if (g_w_u->n != n + 1 && g_w_u->n != n + 2) {
        set_error("ipa_msm_create: the base set holds %zu points; it must be g || w (2^k + 1 = %zu) or g || w || u (2^k + 2)", g_w_u->n, n + 1);
        return TRH_EINVAL;
    }
    if (!g_w_u->shards.empty()) { set_error("ipa_msm_create: needs a base set on one device"); return TRH_EINVAL; }
    TRH_ENTER(0);
    Range range("trh_ipa_msm_create");
    if (g_w_u->owner && g_w_u->owner->device != ctx().device) { set_error("ipa_msm_create: the base set lives on another device than the calling context"); return TRH_EINVAL; }
    uint64_t tail[16];
    TRH_HIP_TRY(hipMemcpy(tail, (const char*)g_w_u->d_xy + n * 64, (g_w_u->n - n) * 64, hipMemcpyDeviceToHost));
    if (g_w_u->n == n + 2 && memcmp(tail + 8, u_xy, 64) != 0) { set_error("ipa_msm_create: the last point of a g || w || u base set differs from u"); return TRH_EINVAL; }
    trh_ipa_msm* m = new trh_ipa_msm();
    m->curve = g_w_u->curve;
    m->k = k;
    m->n = n;
    m->set = g_w_u;
    m->set_has_u = g_w_u->n == n + 2;
    m->owner = &ctx();
    memcpy(m->u_xy, u_xy, 64);
    memcpy(m->w_xy, tail, 64);
    const int rc = m->scalars.ensure(g_w_u->n * 32);
    if (rc != TRH_OK) { delete m; return rc; }
    *out = m;
    return TRH_OK;
}

void trh_ipa_msm_destroy(trh_ipa_msm_t m) {
    if (!m) return;
    if (m->up_pending) (void)hipEventSynchronize(m->up_ev);
    if (m->up_ev) (void)hipEventDestroy(m->up_ev);
    if (m->pinned) (void)hipHostFree(m->pinned);
    m->scalars.release();
    m->tables.release();
    m->params.release();
    delete m;
}

int trh_ipa_msm_append_term(trh_ipa_msm_t m, const uint64_t scalar[4], const uint64_t point_xy[8]) {
    TRH_TRY(require_init());
    if (!m || !scalar || !point_xy) { set_error("ipa_msm_append_term: null pointer"); return TRH_EINVAL; }
    m->other_scalars.insert(m->other_scalars.end(), scalar, scalar + 4);
    m->other_bases.insert(m->other_bases.end(), point_xy, point_xy + 8);
    return TRH_OK;
}

int trh_ipa_msm_add_constant_term(trh_ipa_msm_t m, const uint64_t c[4]) {
    TRH_TRY(require_init());
    if (!m || !c) { set_error("ipa_msm_add_constant_term: null pointer"); return TRH_EINVAL; }
    TRH_ENTER(m->stream);
    Range range("trh_ipa_msm_add_constant_term");
    TRH_TRY(check_msm(m, "ipa_msm_add_constant_term"));
    TRH_TRY(ensure_g(m, m->stream));
    with_curve(m->curve, [&](auto cv) { hipLaunchKernelGGL((verify_add_constant_kernel<typename decltype(cv)::Scalar>), dim3(1), dim3(64), 0, m->stream, (uint4*)m->scalars.p, const1(c)); });
    TRH_HIP_TRY(hipGetLastError());
    return TRH_OK;
}

int trh_ipa_msm_add_to_w_scalar(trh_ipa_msm_t m, const uint64_t s[4]) {
    TRH_TRY(require_init());
    if (!m || !s) { set_error("ipa_msm_add_to_w_scalar: null pointer"); return TRH_EINVAL; }
    sadd(m->curve, m->w_scalar, s);
    return TRH_OK;
}

int trh_ipa_msm_add_to_u_scalar(trh_ipa_msm_t m, const uint64_t s[4]) {
    TRH_TRY(require_init());
    if (!m || !s) { set_error("ipa_msm_add_to_u_scalar: null pointer"); return TRH_EINVAL; }
    sadd(m->curve, m->u_scalar, s);
    return TRH_OK;
}

int trh_ipa_msm_add_to_g_scalars_dev(trh_ipa_msm_t m, const void* scalars_dev, void* stream) {
    TRH_TRY(require_init());
    if (!m || !scalars_dev) { set_error("ipa_msm_add_to_g_scalars_dev: null pointer"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    Range range("trh_ipa_msm_add_to_g_scalars_dev");
    TRH_TRY(check_msm(m, "ipa_msm_add_to_g_scalars_dev"));
    m->stream = (hipStream_t)stream;
    return add_g(m, scalars_dev, (hipStream_t)stream);
}

int trh_ipa_msm_use_challenges(trh_ipa_msm_t m, size_t count, const uint64_t* u, const uint64_t* neg_c, const uint64_t* weights, const uint64_t alpha[4],
                               void* stream) {
    TRH_TRY(require_init());
    if (!m || !u || !neg_c) { set_error("ipa_msm_use_challenges: null pointer"); return TRH_EINVAL; }
    if (count == 0) { set_error("ipa_msm_use_challenges: no guards"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    Range range("trh_ipa_msm_use_challenges");
    TRH_TRY(check_msm(m, "ipa_msm_use_challenges"));
    hipStream_t s = (hipStream_t)stream;
    m->stream = s;
    // the challenges (count x k), then coef_p = weight_p neg_c_p: the host's share is `count` multiplications
    std::vector<uint64_t> hp(count * (m->k + 1) * 4);
    memcpy(hp.data(), u, count * m->k * 32);
    uint64_t* coef = hp.data() + count * m->k * 4;
    for (size_t p = 0; p < count; ++p) {
        if (weights) smul(m->curve, weights + 4 * p, neg_c + 4 * p, coef + 4 * p);
        else memcpy(coef + 4 * p, neg_c + 4 * p, 32);
    }
    return with_curve(m->curve, [&](auto cv) { return use_challenges_t<typename decltype(cv)::Scalar>(m, count, hp.data(), alpha, s); });
}

int trh_ipa_msm_scale(trh_ipa_msm_t m, const uint64_t factor[4], void* stream) {
    TRH_TRY(require_init());
    if (!m || !factor) { set_error("ipa_msm_scale: null pointer"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    Range range("trh_ipa_msm_scale");
    TRH_TRY(check_msm(m, "ipa_msm_scale"));
    m->stream = (hipStream_t)stream;
    TRH_TRY(scale_g(m, factor, (hipStream_t)stream));
    for (size_t i = 0; i < m->other_scalars.size(); i += 4) smul(m->curve, &m->other_scalars[i], factor, &m->other_scalars[i]);
    smul(m->curve, m->w_scalar, factor, m->w_scalar);
    smul(m->curve, m->u_scalar, factor, m->u_scalar);
    return TRH_OK;
}

int trh_ipa_msm_add_msm(trh_ipa_msm_t dst, trh_ipa_msm_t src, void* stream) {
    TRH_TRY(require_init());
    if (!dst || !src) { set_error("ipa_msm_add_msm: null accumulator"); return TRH_EINVAL; }
    if (dst->curve != src->curve) { set_error("ipa_msm_add_msm: the accumulators are over different curves"); return TRH_EINVAL; }
    if (dst->owner != src->owner) { set_error("ipa_msm_add_msm: the accumulators belong to different contexts"); return TRH_EINVAL; }
    if (dst->set != src->set || dst->k != src->k) { set_error("ipa_msm_add_msm: the accumulators are over different base sets"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    Range range("trh_ipa_msm_add_msm");
    TRH_TRY(check_msm(dst, "ipa_msm_add_msm"));
    hipStream_t s = (hipStream_t)stream;
    dst->stream = s;
    const std::vector<uint64_t> osc(src->other_scalars), obs(src->other_bases);  // (copies: src may be dst)
    dst->other_scalars.insert(dst->other_scalars.end(), osc.begin(), osc.end());
    dst->other_bases.insert(dst->other_bases.end(), obs.begin(), obs.end());
    if (src->has_g) TRH_TRY(add_g(dst, src->scalars.p, s));
    uint64_t w[4], u[4];
    memcpy(w, src->w_scalar, 32); memcpy(u, src->u_scalar, 32);
    sadd(dst->curve, dst->w_scalar, w);
    sadd(dst->curve, dst->u_scalar, u);
    return TRH_OK;
}

int trh_ipa_msm_eval(trh_ipa_msm_t m, void* stream, int* is_identity, uint64_t out_xyz[12]) {
    TRH_TRY(require_init());
    if (!m || !is_identity || !out_xyz) { set_error("ipa_msm_eval: null pointer"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    Range range("trh_ipa_msm_eval");
    TRH_TRY(check_msm(m, "ipa_msm_eval"));
    hipStream_t s = (hipStream_t)stream;
    m->stream = s;
    TRH_TRY(msm_idle("ipa_msm_eval"));
    // the small MSM: the appended terms, and w / u wherever the full-range MSM does not carry them
    std::vector<uint64_t> sc(m->other_scalars), bs(m->other_bases);
    auto push = [&](const uint64_t* scalar, const uint64_t* xy) { sc.insert(sc.end(), scalar, scalar + 4); bs.insert(bs.end(), xy, xy + 8); };
    if (!m->has_g) push(m->w_scalar, m->w_xy);
    if (!m->has_g || !m->set_has_u) push(m->u_scalar, m->u_xy);
    uint64_t pts[24];
    memset(pts, 0, sizeof(pts));
    size_t npts = 0;
    uint64_t tail[8];
    if (m->has_g) {  // one full-range MSM over the resident set: g, then the slots of w (and u)
        memcpy(tail, m->w_scalar, 32);
        memcpy(tail + 4, m->u_scalar, 32);
        TRH_HIP_TRY(hipMemcpyAsync((char*)m->scalars.p + m->n * 32, tail, (m->set->n - m->n) * 32, hipMemcpyHostToDevice, s));
        TRH_TRY(trh_msm_dev(m->set, 0, m->scalars.p, m->set->n, 1, stream, pts));  // returns after synchronising s: `tail` has been read
        ++npts;
    }
    if (!sc.empty()) {
        const size_t nterms = sc.size() / 4;
        TRH_TRY(m->curve == TRH_PALLAS ? trh_best_multiexp_pallas(sc.data(), bs.data(), nterms, pts + 12 * npts)
                                       : trh_best_multiexp_vesta(sc.data(), bs.data(), nterms, pts + 12 * npts));
        ++npts;
    }
    TRH_TRY(point_sum_host(m->curve, pts, npts, out_xyz));
    int zero = 1;
    for (int i = 0; i < 12; ++i) zero &= out_xyz[i] == 0 ? 1 : 0;
    *is_identity = zero;
    return TRH_OK;
}

const void* trh_ipa_msm_g_scalars_dev(trh_ipa_msm_t m) {
    if (require_init() != TRH_OK) return nullptr;
    if (!m) { set_error("ipa_msm_g_scalars_dev: null accumulator"); return nullptr; }
    return m->has_g ? m->scalars.p : nullptr;
}

}  // extern "C"
