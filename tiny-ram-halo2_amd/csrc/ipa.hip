// Device primitives of the inner-product-argument opening (halo2_proofs 0.2.0
// `poly::commitment::prover::create_proof`, reached through `poly::multiopen::create_proof` inside
// plonk::create_proof -- reference call site /root/reference/src/test_utils.rs:41-49; SURVEY.md
// section 8 row a7).  Per round j (half = 2^(k-j-1)) the Rust code does
//     L_j = <p'[half..], G'[..half]>          R_j = <p'[..half], G'[half..]>          (two MSMs)
//     value_l = <p'[half..], b[..half]>       value_r = <p'[..half], b[half..]>       (inner products)
//     p'[i] += u^-1 p'[i+half]      b[i] += u b[i+half]                               (folds)
//     G'[i] = G'[i] + u G'[i+half]   then batch_normalize                             (generator collapse)
// The MSMs run through msm.hip on the live G' buffer (trh_bases_wrap_device + offset); this file
// holds the rest: compute_inner_product, the folds (axpy), the generator collapse and the
// power vector b = (1, x, x^2, ...).
#include <string.h>

#include <chrono>
#include <initializer_list>
#include <utility>

#include "bases.h"
#include "devmem.h"
#include "hostcombine.h"
#include "hosthelper.h"
#include "hostplan.h"

namespace trh {
namespace {

// partial[block] = sum over the block's grid-stride share of a[i] * b[i]
template <class F>
__global__ void __launch_bounds__(256) inner_product_kernel(const uint4* __restrict__ a, const uint4* __restrict__ b, size_t n, uint4* __restrict__ partial) {
    __shared__ Fe<F> sh[256];
    Fe<F> acc = fe_zero<F>();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        acc = fe_add(acc, fe_mul(load_fe<F>(a + 2 * i), load_fe<F>(b + 2 * i)));
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = fe_add(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) store_fe<F>(partial + 2 * blockIdx.x, sh[0]);
}
template <class F>
__global__ void __launch_bounds__(256) sum_partials_kernel(const uint4* __restrict__ partial, u32 count, uint4* __restrict__ out) {
    __shared__ Fe<F> sh[256];
    Fe<F> acc = fe_zero<F>();
    for (u32 i = threadIdx.x; i < count; i += 256) acc = fe_add(acc, load_fe<F>(partial + 2 * i));
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = fe_add(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) store_fe<F>(out, sh[0]);
}

// evaluation of a batch of polynomials at one point: partial[poly][block] = sum over the block's share of a[poly][i] * pw[i]
template <class F>
__global__ void __launch_bounds__(256) eval_batch_kernel(const uint4* __restrict__ polys, const uint4* __restrict__ pw, size_t n, uint4* __restrict__ partial) {
    __shared__ Fe<F> sh[256];
    const uint4* a = polys + (size_t)blockIdx.y * n * 2;
    Fe<F> acc = fe_zero<F>();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        acc = fe_add(acc, fe_mul(load_fe<F>(a + 2 * i), load_fe<F>(pw + 2 * i)));
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = fe_add(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) store_fe<F>(partial + 2 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x), sh[0]);
}
template <class F>
__global__ void __launch_bounds__(256) sum_partials_batch_kernel(const uint4* __restrict__ partial, u32 count, uint4* __restrict__ out) {
    __shared__ Fe<F> sh[256];
    const uint4* p = partial + 2 * (size_t)blockIdx.x * count;
    Fe<F> acc = fe_zero<F>();
    for (u32 i = threadIdx.x; i < count; i += 256) acc = fe_add(acc, load_fe<F>(p + 2 * i));
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = fe_add(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) store_fe<F>(out + 2 * (size_t)blockIdx.x, sh[0]);
}

// y[i] += c * x[i]
template <class F>
__global__ void __launch_bounds__(256) axpy_kernel(uint4* __restrict__ y, const uint4* __restrict__ x, size_t n, const uint4* __restrict__ c) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    store_fe<F>(y + 2 * i, fe_add(load_fe<F>(y + 2 * i), fe_mul(load_fe<F>(x + 2 * i), load_fe<F>(c))));
}

// out[i] = x^i, pw[b] = x^(2^b)
template <class F>
__global__ void __launch_bounds__(256) powers_kernel(uint4* __restrict__ out, size_t n, const uint4* __restrict__ pw) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fe<F> r = fe_one<F>();
    for (int b = 0; b < 32; ++b)
        if ((i >> b) & 1u) r = fe_mul(r, load_fe<F>(pw + 2 * b));
    store_fe<F>(out + 2 * i, r);
}

// generator collapse: g_lo[i] = g_lo[i] + u * g_hi[i], normalised to affine
// (u given as canonical 32-bit words; double-and-add from the top set bit)
template <class BF>
__global__ void __launch_bounds__(256) bases_fold_kernel(AffineMem* __restrict__ g_lo, const AffineMem* __restrict__ g_hi, size_t half, const u32* __restrict__ u_words) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= half) return;
    const Affine<BF> hi = aff_load<BF>(g_hi[i]);
    XYZZ<BF> acc = xyzz_identity<BF>();
    for (int w = 7; w >= 0; --w) {
        const u32 word = u_words[w];  // wave-uniform
        for (int bit = 31; bit >= 0; --bit) {
            acc = xyzz_dbl(acc);
            if ((word >> bit) & 1u) xyzz_madd(acc, hi);
        }
    }
    xyzz_madd(acc, aff_load<BF>(g_lo[i]));
    aff_store(xyzz_to_affine(acc), g_lo[i]);
}

// ---- generator collapse without point arithmetic (native prover) ---------------------------
// The folded generators are linear combinations of the original ones,
//     G'_j[i] = sum over idx = i (mod n / 2^j) of wgt[idx] * G[idx],
// and a collapse with challenge u multiplies wgt[idx] by u on every index whose bit log2(half) is set.
// So L_j = <p'[half..], G'[..half]> and R_j = <p'[..half], G'[half..]> are MSMs over the ORIGINAL
// resident bases with the scalars below (zero outside their half), and G' is never materialised.
// a round's constants travel as kernel arguments (a staged copy is a blit kernel and ~20 us of queue idle per round on the trace)
struct IpaConsts { uint4 w[6]; };
template <class F>
__device__ __forceinline__ Fe<F> ipa_const(const IpaConsts& c, int k) { return fe_load<F>(c.w[2 * k].x, c.w[2 * k].y, c.w[2 * k].z, c.w[2 * k].w, c.w[2 * k + 1].x, c.w[2 * k + 1].y, c.w[2 * k + 1].z, c.w[2 * k + 1].w); }
// the folds of a round in one launch: p'[i] += u^-1 p'[i + half], b[i] += u b[i + half] (i < half) and the generators' weights
// (x u where bit log2(half) of the index is set); consts = (u^-1, u)
template <class F>
__global__ void __launch_bounds__(256) ipa_round_update_kernel(uint4* __restrict__ p, uint4* __restrict__ b, uint4* __restrict__ wgt, size_t n, size_t half, u32 bit,
                                                               const IpaConsts consts) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const Fe<F> u = ipa_const<F>(consts, 1);
    if ((idx >> bit) & 1u) store_fe<F>(wgt + 2 * idx, fe_mul(load_fe<F>(wgt + 2 * idx), u));
    if (idx < half) {
        store_fe<F>(p + 2 * idx, fe_add(load_fe<F>(p + 2 * idx), fe_mul(load_fe<F>(p + 2 * (half + idx)), ipa_const<F>(consts, 0))));
        store_fe<F>(b + 2 * idx, fe_add(load_fe<F>(b + 2 * idx), fe_mul(load_fe<F>(b + 2 * (half + idx)), u)));
    }
}

// The folds of round j - 1 and the scalar rows of round j in ONE launch (round 6; two launches before):
//   * the folds are applied ON THE FLY: p'_new[x] = p'[x] + u^-1 p'[hprev + x], b_new[x] = b[x] + u b[hprev + x] (x < hprev) are computed
//     where this round's scalar rows read them and written once to the OTHER buffer of a ping-pong pair (a thread's reads are other
//     threads' writes); the weights are updated in place (own index);
//   * scalars of L_j (row 0) and R_j (row 1) over the bases g || w || u: v = wgt[idx] p'_new[...] on the half of the indices the row
//     covers, 0 on the other.
// consts = (u_prev^-1, u_prev); first = 1 in round 0 (nothing to fold yet: p' and b are read as they are and stay where they are).
// (Measured and dropped: the two inner products and the tail scalars in the same launch behind a "last block" ticket -- every block's release
//  fence and the last block's acquire made it 33 - 67 us against 29 us for the four launches of round 5.)
// both inner products of an IPA round in one launch: partial[pair][block]
template <class F>
__global__ void __launch_bounds__(256) inner_product2_kernel(const uint4* __restrict__ a0, const uint4* __restrict__ b0, const uint4* __restrict__ a1, const uint4* __restrict__ b1, size_t n,
                                                             uint4* __restrict__ partial) {
    __shared__ Fe<F> sh[256];
    const uint4* a = blockIdx.y ? a1 : a0;
    const uint4* b = blockIdx.y ? b1 : b0;
    Fe<F> acc = fe_zero<F>();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        acc = fe_add(acc, fe_mul(load_fe<F>(a + 2 * i), load_fe<F>(b + 2 * i)));
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = fe_add(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) store_fe<F>(partial + 2 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x), sh[0]);
}

template <class F>
__global__ void __launch_bounds__(256) ipa_round_front_kernel(const uint4* __restrict__ p_old, const uint4* __restrict__ b_old, uint4* __restrict__ p_new, uint4* __restrict__ b_new,
                                                              uint4* __restrict__ wgt, uint4* __restrict__ lrsc, size_t n, size_t half, u32 bit, size_t stride, int first,
                                                              int wfresh /* the weights are all one and not in memory yet (rounds 0 and 1) */,
                                                              int canon /* the scalar rows leave in canonical form (the small-MSM kernel would convert every scalar in each of its 104 workgroups) */,
                                                              const IpaConsts consts) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const size_t hprev = half << 1;  // the previous round's half
    const Fe<F> uinv = ipa_const<F>(consts, 0), u = ipa_const<F>(consts, 1);
    auto pn = [&](size_t x) { return first ? load_fe<F>(p_old + 2 * x) : fe_add(load_fe<F>(p_old + 2 * x), fe_mul(load_fe<F>(p_old + 2 * (hprev + x)), uinv)); };  // x < hprev
    Fe<F> w;
    if (wfresh) {  // round 0 reads no weights, round 1 writes them all
        w = (!first && ((idx >> (bit + 1)) & 1u)) ? u : fe_one<F>();
        if (!first) store_fe<F>(wgt + 2 * idx, w);
    } else {
        w = load_fe<F>(wgt + 2 * idx);
        if (!first && ((idx >> (bit + 1)) & 1u)) { w = fe_mul(w, u); store_fe<F>(wgt + 2 * idx, w); }
    }
    const size_t i = idx & (half - 1);
    const bool hi = (idx >> bit) & 1u;
    Fe<F> v = fe_mul(w, pn(hi ? i : half + i));
    if (canon) v = fe_from_mont(v);
    const Fe<F> zero = fe_zero<F>();
    store_fe<F>(lrsc + 2 * idx, hi ? zero : v);
    store_fe<F>(lrsc + 2 * (stride + idx), hi ? v : zero);
    if (!first && idx < hprev) {  // the folded vectors, once
        store_fe<F>(p_new + 2 * idx, pn(idx));
        store_fe<F>(b_new + 2 * idx, fe_add(load_fe<F>(b_old + 2 * idx), fe_mul(load_fe<F>(b_old + 2 * (hprev + idx)), u)));
    }
}
// dst[i] = a[i] + x s[i] (s may be null: a plain copy) and the block sums of dst[i] b[i], one pass: the opening's s(X) -> s' and p + xi s -> p'
// with their values at x3 (consts = (x)).  ipa_fix_constant_kernel then subtracts the value from coefficient 0 -- on the device: the host never
// needs s(x3) or p'(x3) (round 6; each was a synchronisation and two 32-byte copies before).
template <class F>
__global__ void __launch_bounds__(256) ipa_combine_eval_kernel(const uint4* __restrict__ a, const uint4* __restrict__ sv, const uint4* __restrict__ b, uint4* __restrict__ dst, size_t n,
                                                               const IpaConsts consts, uint4* __restrict__ partial) {
    __shared__ Fe<F> sh[256];
    const Fe<F> x = ipa_const<F>(consts, 0);
    Fe<F> acc = fe_zero<F>();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        Fe<F> v = load_fe<F>(a + 2 * i);
        if (sv) v = fe_add(v, fe_mul(load_fe<F>(sv + 2 * i), x));
        store_fe<F>(dst + 2 * i, v);
        acc = fe_add(acc, fe_mul(v, load_fe<F>(b + 2 * i)));
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = fe_add(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) store_fe<F>(partial + 2 * blockIdx.x, sh[0]);
}
// one workgroup: vec[0] -= sum of the partials; with tail: vec[n] = consts[0] (the blind), vec[n + 1] = 0 (the scalar of u)
template <class F>
__global__ void __launch_bounds__(256) ipa_fix_constant_kernel(const uint4* __restrict__ partial, u32 count, uint4* __restrict__ vec, size_t n, int tail, const IpaConsts consts) {
    __shared__ Fe<F> sh[256];
    Fe<F> acc = fe_zero<F>();
    for (u32 i = threadIdx.x; i < count; i += 256) acc = fe_add(acc, load_fe<F>(partial + 2 * i));
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = fe_add(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        store_fe<F>(vec, fe_sub(load_fe<F>(vec), sh[0]));
        if (tail) { store_fe<F>(vec + 2 * n, ipa_const<F>(consts, 0)); store_fe<F>(vec + 2 * (n + 1), fe_zero<F>()); }
    }
}

template <class F>
__global__ void __launch_bounds__(256) ipa_round_tails_kernel(const uint4* __restrict__ partial, u32 count, const IpaConsts consts /* rand_l, rand_r, z */,
                                                              uint4* __restrict__ lrsc, size_t n, size_t stride, int canon /* as ipa_round_front_kernel */) {
    __shared__ Fe<F> sh[256];
    const u32 side = blockIdx.x;
    const uint4* p = partial + 2 * (size_t)side * count;
    Fe<F> acc = fe_zero<F>();
    for (u32 i = threadIdx.x; i < count; i += 256) acc = fe_add(acc, load_fe<F>(p + 2 * i));
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = fe_add(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        Fe<F> r = side ? ipa_const<F>(consts, 1) : ipa_const<F>(consts, 0), vz = fe_mul(sh[0], ipa_const<F>(consts, 2));
        if (canon) { r = fe_from_mont(r); vz = fe_from_mont(vz); }
        store_fe<F>(lrsc + 2 * (side * stride + n), r);
        store_fe<F>(lrsc + 2 * (side * stride + n + 1), vz);
    }
}

template <class F>
int inner_product_t(const void* a, const void* b, size_t n, hipStream_t s, u64* out) {
    Ctx& c = ctx();
    unsigned blocks = (unsigned)((n + 255) / 256);
    if (blocks > 1024) blocks = 1024;
    if (blocks == 0) blocks = 1;
    TRH_TRY(c.io.ensure((size_t)(blocks + 1) * 32));
    uint4* partial = c.io.as<uint4>();
    uint4* result = partial + 2 * blocks;
    hipLaunchKernelGGL((inner_product_kernel<F>), dim3(blocks), dim3(256), 0, s, (const uint4*)a, (const uint4*)b, n, partial);
    hipLaunchKernelGGL((sum_partials_kernel<F>), dim3(1), dim3(256), 0, s, partial, blocks, result);
    TRH_HIP_TRY(hipGetLastError());
    TRH_HIP_TRY(hipMemcpyAsync(out, result, 32, hipMemcpyDeviceToHost, s));
    TRH_HIP_TRY(hipStreamSynchronize(s));
    return TRH_OK;
}

// small device -> host read-back through the pinned landing area (callers hold the context lock)
int read_back(void* out, const void* dev, size_t bytes, hipStream_t s) {
    Ctx& c = ctx();
    if (bytes > 4096) {
        TRH_HIP_TRY(hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, s));
        TRH_HIP_TRY(hipStreamSynchronize(s));
        return TRH_OK;
    }
    TRH_TRY(host_land(c, 4096, nullptr));
    TRH_HIP_TRY(hipMemcpyAsync(c.pinned_land, dev, bytes, hipMemcpyDeviceToHost, s));
    TRH_HIP_TRY(hipStreamSynchronize(s));
    memcpy(out, c.pinned_land, bytes);
    return TRH_OK;
}

// small per-call constant staged in the factor ring (see trh_field_scale_rows_dev)
int stage_constant(const void* host, size_t bytes, hipStream_t s, void** dev) {
    Ctx& c = ctx();
    constexpr unsigned SLOTS = 64, SLOT_BYTES = 2048;
    if (bytes > SLOT_BYTES) { set_error("stage_constant: %zu bytes", bytes); return TRH_EINVAL; }
    TRH_TRY(c.factors.ensure(16 * 64 * 32 + SLOTS * SLOT_BYTES));  // the first 32 KiB belong to the scale kernels' ring
    if (!c.pinned_ring) TRH_HIP_TRY(hipHostMalloc(&c.pinned_ring, SLOTS * SLOT_BYTES, hipHostMallocDefault));
    const unsigned k = c.pinned_slot++ % SLOTS;
    if (k == 0 && c.pinned_slot > 1) TRH_HIP_TRY(hipDeviceSynchronize());  // wrap-around: every earlier upload (on whatever stream) has left the pinned slots
    char* hslot = (char*)c.pinned_ring + (size_t)k * SLOT_BYTES;
    char* dslot = (char*)c.factors.p + 16 * 64 * 32 + (size_t)k * SLOT_BYTES;
    memcpy(hslot, host, bytes);
    TRH_HIP_TRY(hipMemcpyAsync(dslot, hslot, bytes, hipMemcpyHostToDevice, s));
    *dev = dslot;
    return TRH_OK;
}

template <class F>
int powers_t(void* out, size_t n, const u64* x, hipStream_t s) {
    FeMem pw[32];
    memcpy(&pw[0], x, 32);
    for (int b = 1; b < 32; ++b) fe_store(fe_sqr(fe_load<F>(pw[b - 1])), pw[b]);
    void* d_pw;
    TRH_TRY(stage_constant(pw, sizeof(pw), s, &d_pw));
    hipLaunchKernelGGL((powers_kernel<F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (uint4*)out, n, (const uint4*)d_pw);
    TRH_HIP_TRY(hipGetLastError());
    return TRH_OK;
}

// poly::eval_polynomial for `batch` polynomials of n coefficients at one point: the powers x^i are built once
template <class F>
int eval_batch_t(const void* polys, size_t n, size_t batch, const u64* x, hipStream_t s, u64* out) {
    Ctx& c = ctx();
    unsigned blocks = (unsigned)((n + 2047) / 2048);  // eight elements per thread
    if (blocks > 64) blocks = 64;
    if (blocks == 0) blocks = 1;
    TRH_TRY(c.scan.ensure(n * 32 + 32));
    TRH_TRY(c.io.ensure((size_t)batch * (blocks + 1) * 32));
    TRH_TRY((powers_t<F>(c.scan.p, n, x, s)));
    uint4* partial = c.io.as<uint4>();
    uint4* result = partial + 2 * (size_t)batch * blocks;
    for (size_t b0 = 0; b0 < batch; b0 += 65535) {
        const unsigned nb = (unsigned)(batch - b0 < 65535 ? batch - b0 : 65535);
        hipLaunchKernelGGL((eval_batch_kernel<F>), dim3(blocks, nb), dim3(256), 0, s, (const uint4*)polys + b0 * n * 2, c.scan.as<uint4>(), n, partial + 2 * b0 * blocks);
        hipLaunchKernelGGL((sum_partials_batch_kernel<F>), dim3(nb), dim3(256), 0, s, partial + 2 * b0 * blocks, blocks, result + 2 * b0);
    }
    TRH_HIP_TRY(hipGetLastError());
    return read_back(out, result, batch * 32, s);
}

template <class SF, class BF>
int bases_fold_t(void* g_lo, const void* g_hi, size_t half, const u64* u_mont, hipStream_t s) {
    FeMem um, uc;
    memcpy(&um, u_mont, 32);
    fe_store(fe_from_mont(fe_load<SF>(um)), uc);  // scalar -> canonical bits (host)
    void* d_u;
    TRH_TRY(stage_constant(&uc, 32, s, &d_u));
    hipLaunchKernelGGL((bases_fold_kernel<BF>), dim3((unsigned)((half + 255) / 256)), dim3(256), 0, s, (AffineMem*)g_lo, (const AffineMem*)g_hi, half, (const u32*)d_u);
    TRH_HIP_TRY(hipGetLastError());
    return TRH_OK;
}

template <class F>
int axpy_t(void* y, const void* x, size_t n, const FeMem& c_mont, hipStream_t s) {
    if (!n) return TRH_OK;
    void* d_c;
    TRH_TRY(stage_constant(&c_mont, 32, s, &d_c));
    hipLaunchKernelGGL((axpy_kernel<F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (uint4*)y, (const uint4*)x, n, (const uint4*)d_c);
    TRH_HIP_TRY(hipGetLastError());
    return TRH_OK;
}

// ---------------------------------------------------------------------------------------
// The whole opening: poly::commitment::prover::create_proof with p', b and G' resident on the
// device.  Host-side scalar arithmetic uses the shared field code; the transcript and the prover's
// randomness are callbacks into the caller (BLAKE2b transcript and OsRng on the Rust side).
// Everything the opening decides from its shape is hostplan::ipa_plan's; the stages below run that plan.
// ---------------------------------------------------------------------------------------
static_assert(hostplan::ZREC_BYTES == ZREC && hostplan::FE_BYTES == sizeof(FeMem) && hostplan::AFFINE_BYTES == sizeof(AffineMem), "hostplan.h sizes the opening's buffers by these");

hostplan::IpaShape ipa_shape(const trh_bases* gw, uint32_t k) {
    return hostplan::IpaShape{k, gw->n, gw->d_table != nullptr, gw->fb.c, gw->fb.W, ctx().window_override, opt().ipa_fold, msm_small_max_pairs()};
}

template <class F>
FeMem fe_mem(const Fe<F>& v) { FeMem m; fe_store(v, m); return m; }
// up to three constants of a launch, as its kernel argument
template <class F>
IpaConsts ipa_consts(std::initializer_list<Fe<F>> v) {
    IpaConsts k{};
    int i = 0;
    for (const Fe<F>& e : v) { const FeMem m = fe_mem(e); memcpy(&k.w[2 * i++], &m, 32); }
    return k;
}
double ipa_now() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// One opening: the plan, the call, and what the rounds hand to each other.
template <class SF>
struct IpaRun {
    hostplan::IpaPlan p;
    int curve; const trh_bases* gw; hipStream_t s;
    const trh_transcript_t* tr; trh_rng_scalar_fn rng; void* rng_ctx;
    Ctx* c; IpaScratch* sc;
    const MsmFixedBase* fb;              // the set's table while the MSMs run over it: null without one, for a small set, and after the collapse
    const void* small_z;                 // a small tabled set: level 0 of its table, the bases in record form
    const void *round_xy, *round_z;      // bases of the round MSMs
    void *p_cur, *b_cur, *p_nxt, *b_nxt; // p' and b live in ping-pong pairs from round 1 on (a round reads the vectors the previous one left and writes their folds to the other buffer)
    Fe<SF> z, f, rnd[2], u_prev, u_prev_inv;
    u64 u_hist[16 * 4];                  // the challenges the collapse needs
    bool trace; double t_acc[5];         // TRH_TRACE bit 1: where the host's part of a round goes (sums over the rounds, microseconds)
};

// b = (1, x3, x3^2, ...); s'(X) = s(X) - s(x3), then its commitment over g ‖ w with the blind appended: one pass copies s and forms its value at
// x3, one workgroup subtracts it from coefficient 0 and appends the blind (and the zero scalar of u) -- no host turn before the MSM
template <class SF>
int commit_s_prime(IpaRun<SF>& r, const void* s_poly_dev, const Fe<SF>& s_blind, const Fe<SF>& x3) {
    const hostplan::IpaPlan& p = r.p; IpaScratch& sc = *r.sc; hipStream_t s = r.s;
    const FeMem x3m = fe_mem(x3);
    TRH_TRY((powers_t<SF>(sc.b.p, p.n, (const u64*)&x3m, s)));
    uint4* const partial = (uint4*)r.c->io.p;
    hipLaunchKernelGGL((ipa_combine_eval_kernel<SF>), dim3(p.eval_blocks), dim3(256), 0, s, (const uint4*)s_poly_dev, (const uint4*)nullptr, sc.b.as<const uint4>(), sc.sp.as<uint4>(), p.n,
                       IpaConsts{}, partial);
    hipLaunchKernelGGL((ipa_fix_constant_kernel<SF>), dim3(1), dim3(256), 0, s, (const uint4*)partial, p.eval_blocks, sc.sp.as<uint4>(), p.n, 1, ipa_consts({s_blind}));
    TRH_HIP_TRY(hipGetLastError());
    if (p.first_msm == hostplan::IPA_MSM_TABLE) {  // the scalar of u is zero: the full-range (table) path
        MsmFlags dense;
        dense.dense_hint = true;  // s(X) is uniformly random: no sparse classification
        TRH_TRY(msm_enqueue(r.curve, r.gw->d_xy, r.gw->d_z, sc.sp.p, p.first_pairs, 1, p.first_pairs, 1, s, r.fb, nullptr, dense));
    } else
        TRH_TRY(msm_enqueue(r.curve, r.gw->d_xy, r.small_z ? r.small_z : r.gw->d_z, sc.sp.p, p.first_pairs, 1, p.first_pairs, 1, s));
    u64 pt[12];
    TRH_TRY(msm_finish(r.curve, s, pt, 1));
    r.tr->write_point(r.tr->ctx, pt);
    return TRH_OK;
}

// p'(X) = p(X) + xi s'(X) - v, v its value at x3: the same two launches
template <class SF>
int form_p_prime(IpaRun<SF>& r, const void* p_poly_dev, const Fe<SF>& xi) {
    const hostplan::IpaPlan& p = r.p; IpaScratch& sc = *r.sc;
    uint4* const partial = (uint4*)r.c->io.p;
    hipLaunchKernelGGL((ipa_combine_eval_kernel<SF>), dim3(p.eval_blocks), dim3(256), 0, r.s, (const uint4*)p_poly_dev, sc.sp.as<const uint4>(), sc.b.as<const uint4>(), sc.pp.as<uint4>(), p.n,
                       ipa_consts({xi}), partial);
    hipLaunchKernelGGL((ipa_fix_constant_kernel<SF>), dim3(1), dim3(256), 0, r.s, (const uint4*)partial, p.eval_blocks, sc.pp.as<uint4>(), p.n, 0, IpaConsts{});
    TRH_HIP_TRY(hipGetLastError());
    return TRH_OK;
}

// the bases of the round MSMs are g (n points) followed by w and u, so that [rand] W + [value z] U ride in the same MSM as the main sum:
// the set itself where it holds u, otherwise a copy with u appended
template <class SF>
int bind_round_bases(IpaRun<SF>& r, const u64* u_xy) {
    const size_t n = r.p.n; IpaScratch& sc = *r.sc;
    r.round_xy = r.gw->d_xy;
    r.round_z = nullptr;
    if (!r.p.with_u) {
        TRH_HIP_TRY(hipMemcpyAsync(sc.gwu.p, r.gw->d_xy, (n + 1) * 64, hipMemcpyDeviceToDevice, r.s));
        TRH_HIP_TRY(hipMemcpy((char*)sc.gwu.p + (n + 1) * 64, u_xy, 64, hipMemcpyHostToDevice));
        TRH_TRY(msm_convert_bases(r.curve, sc.gwu.p, sc.gwuz.p, n + 2, r.s));
        r.round_xy = sc.gwu.p; r.round_z = sc.gwuz.p;
    } else if (!r.fb) {
        r.round_z = r.small_z ? r.small_z : r.gw->d_z;  // the handle's converted copy when it has one; otherwise the MSM converts per call
    }
    return TRH_OK;
}

// G'' || w || u from the table, after the challenges of rounds 0 .. r - 1; from here on the rounds are MSMs over m + 2 points
// (inline: on a stream of its own under the next full-size rounds the collapse gained nothing -- profiles/r06_ipa_fold_overlap_ab.txt)
template <class SF>
int collapse_generators(IpaRun<SF>& r) {
    const size_t n = r.p.n, m = r.p.m; IpaScratch& sc = *r.sc;
    TRH_TRY(ipa_fold_generators(r.curve, *r.fb, r.gw->n, r.p, r.u_hist, sc.gwu.p, sc.gwuz.p, r.s));
    TRH_HIP_TRY(hipMemcpyAsync((char*)sc.gwu.p + m * 64, (const char*)r.gw->d_xy + n * 64, 2 * 64, hipMemcpyDeviceToDevice, r.s));
    TRH_HIP_TRY(hipMemcpyAsync((char*)sc.gwuz.p + m * ZREC, (const char*)r.fb->table + n * ZREC, 2 * ZREC, hipMemcpyDeviceToDevice, r.s));  // level 0 of the table = the bases
    r.round_xy = sc.gwu.p; r.round_z = sc.gwuz.p; r.fb = nullptr;
    ++sc.collapses;
    return TRH_OK;
}

// per round three launches in front of the MSM (the previous round's folds applied on the fly + the scalar rows; both inner products; the tail
// scalars -- the round's constants travel as kernel arguments), then the MSM.  No host synchronisation before the MSM: the host
// never needs value_l / value_r.  (Round 5 had four launches here, the first version 14 small operations.)
template <class SF>
int enqueue_round(IpaRun<SF>& r, uint32_t j) {
    const hostplan::IpaRound g = r.p.round(j);
    IpaScratch& sc = *r.sc; hipStream_t s = r.s;
    FeMem tmp;
    r.rng(r.rng_ctx, (u64*)&tmp); r.rnd[0] = fe_load<SF>(tmp);
    r.rng(r.rng_ctx, (u64*)&tmp); r.rnd[1] = fe_load<SF>(tmp);
    hipLaunchKernelGGL((ipa_round_front_kernel<SF>), dim3(g.front_blocks), dim3(256), 0, s, (const uint4*)r.p_cur, (const uint4*)r.b_cur, (uint4*)r.p_nxt, (uint4*)r.b_nxt, sc.wgt.as<uint4>(),
                       sc.lrsc.as<uint4>(), g.gens, g.half, g.bit, g.stride, g.first, g.wfresh, g.canon, ipa_consts({r.u_prev_inv, r.u_prev}));
    if (j > 0) { std::swap(r.p_cur, r.p_nxt); std::swap(r.b_cur, r.b_nxt); }
    // value_l = <p'[half ..], b[.. half]>, value_r = <p'[.. half], b[half ..]> over the folded vectors, then the tail scalars [rand] W, [value z] U
    uint4* const partial = (uint4*)r.c->io.p;
    hipLaunchKernelGGL((inner_product2_kernel<SF>), dim3(g.sum_blocks, 2), dim3(256), 0, s, (const uint4*)((const char*)r.p_cur + g.half * 32), (const uint4*)r.b_cur, (const uint4*)r.p_cur,
                       (const uint4*)((const char*)r.b_cur + g.half * 32), g.half, partial);
    hipLaunchKernelGGL((ipa_round_tails_kernel<SF>), dim3(2), dim3(256), 0, s, partial, g.sum_blocks, ipa_consts({r.rnd[0], r.rnd[1], r.z}), sc.lrsc.as<uint4>(), g.gens, g.stride, g.canon);
    TRH_HIP_TRY(hipGetLastError());
    MsmFlags dense;
    dense.dense_hint = true;  // p' . w: full-size values on half the rows
    return msm_enqueue(r.curve, r.round_xy, r.round_z, sc.lrsc.p, g.gens + 2, 2, g.stride, g.canon ? 0 : 1, s, r.fb, nullptr, dense);
}

// L_j and R_j to the transcript, the challenge u_j and its inverse; t_round0: when the round began (trace)
template <class SF>
int finish_round(IpaRun<SF>& r, uint32_t j, double t_round0) {
    const double t_enq = r.trace ? ipa_now() : 0;
    u64 lrb[24];
    TRH_TRY(msm_finish(r.curve, r.s, lrb, 2));
    const double t_fin = r.trace ? ipa_now() : 0;
    FeMem tmp;
    r.tr->write_point(r.tr->ctx, lrb);
    r.tr->write_point(r.tr->ctx, lrb + 12);
    r.tr->squeeze_challenge_scalar(r.tr->ctx, (u64*)&tmp);
    const double t_tr = r.trace ? ipa_now() : 0;
    const Fe<SF> u_j = fe_load<SF>(tmp);
    if (fe_is_zero(u_j)) { set_error("ipa_create_proof: round %u challenge is zero (the Rust prover's u_j.invert().unwrap() panics here)", j); return TRH_EINVAL; }
    // u_j^-1 on the host's 4 x 64-bit Montgomery code (hostcombine.h): the nine-limb form the device code uses costs the host three times as much
    hostcombine::H uh;
    memcpy(&uh, &tmp, 32);
    const hostcombine::H uih = hostcombine::inv<SF>(uh);
    FeMem uim;
    memcpy(&uim, &uih, 32);
    const Fe<SF> u_inv = fe_load<SF>(uim);
    if (j < 16) memcpy(r.u_hist + 4 * j, &tmp, 32);
    r.u_prev = u_j; r.u_prev_inv = u_inv;  // folded into the next round's front launch (or by the launch behind the loop)
    r.f = fe_add(r.f, fe_add(fe_mul(r.rnd[0], u_inv), fe_mul(r.rnd[1], u_j)));
    if (r.trace) {
        const double t_end = ipa_now();
        r.t_acc[0] += t_enq - t_round0; r.t_acc[1] += t_fin - t_enq; r.t_acc[2] += t_tr - t_fin; r.t_acc[3] += t_end - t_tr; r.t_acc[4] += t_end - t_round0;
    }
    return TRH_OK;
}

// the last round's fold: p'[0] += u^-1 p'[1] (b and the weights are not read again, the kernel folds them too); then c = p'[0] and f leave
template <class SF>
int final_fold(IpaRun<SF>& r, u64* out_c, u64* out_f) {
    const uint32_t k = r.p.k;
    if (k > 0) {
        const size_t ncur = r.p.round(k - 1).gens;
        hipLaunchKernelGGL((ipa_round_update_kernel<SF>), dim3((unsigned)((ncur + 255) / 256)), dim3(256), 0, r.s, (uint4*)r.p_cur, (uint4*)r.b_cur, (uint4*)r.sc->wgt.p, ncur, (size_t)1, 0u,
                           ipa_consts({r.u_prev_inv, r.u_prev}));
        TRH_HIP_TRY(hipGetLastError());
    }
    if (r.trace)
        fprintf(stderr, "[trh ipa] k = %u, per round (us): enqueue %.1f, wait for the MSM (sync + host combine) %.1f, transcript callbacks %.1f, inversion + update launch %.1f, round %.1f\n",
                k, r.t_acc[0] / k, r.t_acc[1] / k, r.t_acc[2] / k, r.t_acc[3] / k, r.t_acc[4] / k);
    TRH_HIP_TRY(hipStreamSynchronize(r.s));
    FeMem cm;
    TRH_HIP_TRY(hipMemcpy(&cm, r.p_cur, 32, hipMemcpyDeviceToHost));
    const FeMem fm = fe_mem(r.f);
    r.tr->write_scalar(r.tr->ctx, (const u64*)&cm);
    r.tr->write_scalar(r.tr->ctx, (const u64*)&fm);
    if (out_c) memcpy(out_c, &cm, 32);
    if (out_f) memcpy(out_f, &fm, 32);
    return TRH_OK;
}

template <class SF, class BF>
int ipa_create_proof_t(int curve, const trh_bases* gw, const u64* u_xy, uint32_t k, const void* p_poly_dev, const u64* p_blind_m, const u64* x3_m,
                       const void* s_poly_dev, const u64* s_blind_m, const trh_transcript_t* tr, trh_rng_scalar_fn rng, void* rng_ctx,
                       hipStream_t s, u64* out_c, u64* out_f) {
    auto ld = [](const u64* p) { FeMem m; memcpy(&m, p, 32); return fe_load<SF>(m); };
    const Fe<SF> x3 = ld(x3_m), p_blind = ld(p_blind_m), s_blind = ld(s_blind_m);
    Ctx& c = ctx();
    IpaRun<SF> r{};
    r.p = hostplan::ipa_plan(ipa_shape(gw, k));
    r.curve = curve; r.gw = gw; r.s = s; r.tr = tr; r.rng = rng; r.rng_ctx = rng_ctx; r.c = &c; r.sc = &c.ipa;
    r.fb = r.p.first_msm == hostplan::IPA_MSM_TABLE ? &gw->fb : nullptr;
    r.small_z = r.p.first_msm == hostplan::IPA_MSM_SMALL_Z ? gw->fb.table : nullptr;
    r.trace = (opt().trace & 2) != 0;
    c.msm.lean_off_n = 0;  // a shape whose lean sort overflowed keeps the fallback launches for the rest of ITS opening only (msm.hip lean_sort)
    TRH_TRY(ipa_scratch_reserve(c, r.p, r.p.fold_list_words, s));

    TRH_TRY(commit_s_prime(r, s_poly_dev, s_blind, x3));
    FeMem tmp;
    tr->squeeze_challenge_scalar(tr->ctx, (u64*)&tmp);
    const Fe<SF> xi = fe_load<SF>(tmp);
    tr->squeeze_challenge_scalar(tr->ctx, (u64*)&tmp);
    r.z = fe_load<SF>(tmp);
    TRH_TRY(form_p_prime(r, p_poly_dev, xi));
    r.f = fe_add(fe_mul(s_blind, xi), p_blind);
    // the generators' weights inside the (virtual) folded ones are all ones at first: the front launch of round 0 takes them as such and round 1's writes them -- no fill
    TRH_TRY(bind_round_bases(r, u_xy));
    r.p_cur = c.ipa.pp.p; r.b_cur = c.ipa.b.p;
    r.p_nxt = c.ipa.pp2.p; r.b_nxt = c.ipa.b2.p;
    r.u_prev = fe_one<SF>(); r.u_prev_inv = fe_one<SF>();

    struct WindowGuard {
        int& slot; int saved;
        WindowGuard(int& s_, int v) : slot(s_), saved(s_) { if (!saved) slot = v; }
        ~WindowGuard() { slot = saved; }
    } window_guard(c.window_override, r.p.round_window);

    for (uint32_t j = 0; j < k; ++j) {
        const double t_round0 = r.trace ? ipa_now() : 0;
        if (r.p.fold_at && j == r.p.fold_at) TRH_TRY(collapse_generators(r));
        TRH_TRY(enqueue_round(r, j));
        TRH_TRY(finish_round(r, j, t_round0));
    }
    return final_fold(r, out_c, out_f);
}

}  // namespace

int ipa_scratch_reserve(Ctx& c, const hostplan::IpaPlan& p, size_t list_words, hipStream_t s) {
    IpaScratch& sc = c.ipa;
    TRH_TRY(sc.b.ensure(p.bytes.b)); TRH_TRY(sc.sp.ensure(p.bytes.sp)); TRH_TRY(sc.pp.ensure(p.bytes.pp)); TRH_TRY(sc.wgt.ensure(p.bytes.wgt)); TRH_TRY(sc.lrsc.ensure(p.bytes.lrsc));
    TRH_TRY(sc.pp2.ensure(p.bytes.pp2)); TRH_TRY(sc.b2.ensure(p.bytes.b2));
    TRH_TRY(sc.gwu.ensure(p.bytes.gwu)); TRH_TRY(sc.gwuz.ensure(p.bytes.gwuz));
    TRH_TRY(c.io.ensure(p.bytes.io));
    if (!p.fold_at) return TRH_OK;
    TRH_TRY(sc.fold_buckets.ensure(p.bytes.fold_buckets));
    TRH_TRY(sc.fold_lists.ensure(list_words * 4));
    if (sc.fold_pinned_cap < list_words * 4) {
        if (sc.fold_pinned) { TRH_HIP_TRY(hipStreamSynchronize(s)); (void)hipHostFree(sc.fold_pinned); sc.fold_pinned = nullptr; sc.fold_pinned_cap = 0; }
        const size_t want = list_words * 4 + 4096;
        TRH_HIP_TRY(hipHostMalloc(&sc.fold_pinned, want, hipHostMallocDefault));
        sc.fold_pinned_cap = want;
    }
    return TRH_OK;
}

// what an opening over this base set allocates, at setup time (trh_bases_reserve): the first proof of a process then finds its vectors, the
// collapse's buckets and the small MSM's landing area in place
int ipa_reserve(int curve, const trh_bases* gw, uint32_t k) {
    Ctx& c = ctx();
    const hostplan::IpaPlan p = hostplan::ipa_plan(ipa_shape(gw, k));
    TRH_TRY(ipa_scratch_reserve(c, p, p.fold_list_words, nullptr));
    if (!p.fold_at) return TRH_OK;
    if (!c.helper && !c.helper_failed) {  // msm_finish's second Horner thread
        try { c.helper = new HostHelper(); } catch (...) { c.helper_failed = true; }
    }
    const hostplan::IpaRound g = p.round(p.fold_at);  // the rounds behind the collapse
    MsmFlags reserve;
    reserve.reserve_only = true;
    return msm_enqueue(curve, c.ipa.gwu.p, c.ipa.gwuz.p, c.ipa.lrsc.p, g.gens + 2, 2, g.stride, 1, nullptr, nullptr, nullptr, reserve);
}

int field_powers_device(int field, void* out_dev, size_t n, const u64 x_mont[4], hipStream_t s) {
    if (!n) return TRH_OK;
    return with_field(field, [&](auto f) { return powers_t<decltype(f)>(out_dev, n, x_mont, s); });
}
}  // namespace trh

using namespace trh;

extern "C" {

int trh_poly_eval_batch_dev(int field, const void* polys_dev, size_t n, size_t batch, const uint64_t point[4], void* stream, uint64_t* out) {
    TRH_TRY(require_init());
    TRH_TRY(check_field(field));
    if (!out || !point || (n && batch && !polys_dev)) { set_error("poly_eval: null pointer"); return TRH_EINVAL; }
    if (!batch) return TRH_OK;
    if (!n) { memset(out, 0, batch * 32); return TRH_OK; }
    TRH_ENTER(stream);
    Range range("trh_poly_eval_batch_dev");
    return with_field(field, [&](auto f) { return eval_batch_t<decltype(f)>(polys_dev, n, batch, point, (hipStream_t)stream, out); });
}

int trh_field_inner_product_dev(int field, const void* a_dev, const void* b_dev, size_t n, void* stream, uint64_t out[4]) {
    TRH_TRY(require_init());
    TRH_TRY(check_field(field));
    if (!out || (n && (!a_dev || !b_dev))) { set_error("inner_product: null pointer"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    Range range("trh_field_inner_product_dev");
    return with_field(field, [&](auto f) { return inner_product_t<decltype(f)>(a_dev, b_dev, n, (hipStream_t)stream, out); });
}

int trh_field_axpy_dev(int field, void* y_dev, const void* x_dev, size_t n, const uint64_t c_mont[4], void* stream) {
    TRH_TRY(require_init());
    TRH_TRY(check_field(field));
    if (!c_mont || (n && (!y_dev || !x_dev))) { set_error("axpy: null pointer"); return TRH_EINVAL; }
    if (!n) return TRH_OK;
    TRH_ENTER(stream);
    Range range("trh_field_axpy_dev");
    FeMem cm;
    memcpy(&cm, c_mont, 32);
    return with_field(field, [&](auto f) { return axpy_t<decltype(f)>(y_dev, x_dev, n, cm, (hipStream_t)stream); });
}

int trh_field_powers_dev(int field, void* out_dev, size_t n, const uint64_t x_mont[4], void* stream) {
    TRH_TRY(require_init());
    TRH_TRY(check_field(field));
    if (!x_mont || (n && !out_dev)) { set_error("powers: null pointer"); return TRH_EINVAL; }
    if (!n) return TRH_OK;
    TRH_ENTER(stream);
    Range range("trh_field_powers_dev");
    return with_field(field, [&](auto f) { return powers_t<decltype(f)>(out_dev, n, x_mont, (hipStream_t)stream); });
}

int trh_bases_fold_dev(int curve, void* g_lo_dev, const void* g_hi_dev, size_t half, const uint64_t u_mont[4], void* stream) {
    TRH_TRY(require_init());
    TRH_TRY(check_curve(curve));
    if (!u_mont || (half && (!g_lo_dev || !g_hi_dev))) { set_error("bases_fold: null pointer"); return TRH_EINVAL; }
    if (!half) return TRH_OK;
    TRH_ENTER(stream);
    Range range("trh_bases_fold_dev");
    return with_curve(curve, [&](auto cv) { return bases_fold_t<typename decltype(cv)::Scalar, typename decltype(cv)::Base>(g_lo_dev, g_hi_dev, half, u_mont, (hipStream_t)stream); });
}

int trh_ipa_create_proof(trh_bases_t g_w, const uint64_t u_xy[8], uint32_t k, const void* p_poly_dev, const uint64_t p_blind[4], const uint64_t x3[4],
                         const void* s_poly_dev, const uint64_t s_blind[4], const trh_transcript_t* transcript, trh_rng_scalar_fn rng, void* rng_ctx,
                         void* stream, uint64_t out_c[4], uint64_t out_f[4]) {
    TRH_TRY(require_init());
    if (!g_w || !u_xy || !p_poly_dev || !p_blind || !x3 || !s_poly_dev || !s_blind || !transcript || !rng ||
        !transcript->write_point || !transcript->write_scalar || !transcript->squeeze_challenge_scalar) { set_error("ipa_create_proof: null pointer"); return TRH_EINVAL; }
    if (k > 26 || (g_w->n != ((size_t)1 << k) + 1 && g_w->n != ((size_t)1 << k) + 2)) { set_error("ipa_create_proof: bases must hold g (2^k points) followed by w (and optionally u)"); return TRH_EINVAL; }
    if (!g_w->shards.empty()) { set_error("ipa_create_proof: needs a base set on one device (the rounds are sequential: SURVEY 8e)"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    Range range("trh_ipa_create_proof");
    if (g_w->owner && g_w->owner->device != ctx().device) { set_error("ipa_create_proof: the base set lives on another device than the calling context"); return TRH_EINVAL; }
    TRH_TRY(msm_idle("ipa_create_proof"));
    if (g_w->n == ((size_t)1 << k) + 2) {  // g || w || u: the resident u must be the caller's
        uint64_t last[8];
        TRH_HIP_TRY(hipMemcpy(last, (const char*)g_w->d_xy + (g_w->n - 1) * 64, 64, hipMemcpyDeviceToHost));
        if (memcmp(last, u_xy, 64) != 0) { set_error("ipa_create_proof: the last point of a g || w || u base set differs from u"); return TRH_EINVAL; }
    }
    return with_curve(g_w->curve, [&](auto cv) {
        return ipa_create_proof_t<typename decltype(cv)::Scalar, typename decltype(cv)::Base>(g_w->curve, g_w, u_xy, k, p_poly_dev, p_blind, x3, s_poly_dev, s_blind, transcript, rng, rng_ctx, (hipStream_t)stream, out_c, out_f);
    });
}

}  // extern "C"
