// Elementwise entries of the C ABI: one field or point operation per element (what the self-test and the golden vectors run), the scale
// entries, the plain NTT entries (device, and best_fft over hostio.hip) and the host point sum.
#include "ctx.h"
#include "curve_q4.h"

using namespace trh;

namespace trh {

int field_scale_periodic(int field, void* a_dev, size_t rows, size_t row_len, size_t active_len, const void* factors_dev, u32 period, hipStream_t s);  // ntt.hip

namespace {

template <class F>
__global__ void __launch_bounds__(256) field_op_kernel(int op, const uint4* __restrict__ a, const uint4* __restrict__ b, uint4* __restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fe<F> x, y = fe_zero<F>(), r;
    {
        uint4 lo = a[2 * i], hi = a[2 * i + 1];
        x = fe_load<F>(lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w);
    }
    if (b) {
        uint4 lo = b[2 * i], hi = b[2 * i + 1];
        y = fe_load<F>(lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w);
    }
    switch (op) {
        case 0: r = fe_add(x, y); break;
        case 1: r = fe_sub(x, y); break;
        case 2: r = fe_mul(x, y); break;
        case 3: r = fe_sqr(x); break;
        case 4: r = fe_neg(x); break;
        case 5: r = fe_inv(x); break;
        case 6: r = fe_to_mont(x); break;
        default: r = fe_from_mont(x); break;
    }
    u32 w[8];
    fe_store(r, w);
    out[2 * i] = make_uint4(w[0], w[1], w[2], w[3]);
    out[2 * i + 1] = make_uint4(w[4], w[5], w[6], w[7]);
}

template <class F>
__global__ void __launch_bounds__(64) point_op_kernel(int op, const JacobianMem* __restrict__ p, const void* __restrict__ q, JacobianMem* __restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    XYZZ<F> a = xyzz_from_jacobian(jac_load<F>(p[i])), r;
    if (op == 0) {
        r = xyzz_add(a, xyzz_from_jacobian(jac_load<F>(((const JacobianMem*)q)[i])));
    } else if (op == 1) {
        r = a;
        xyzz_madd(r, aff_load<F>(((const AffineMem*)q)[i]));
    } else {
        r = xyzz_dbl(a);
    }
    jac_store(jac_from_affine(xyzz_to_affine(r)), out[i]);
}

// ops 3 / 4: the same addition / doubling through the quad-lane arithmetic of curve_q4.h (four lanes per pair: lane q carries coordinate q in
// the lazy domain), so that the golden vectors and the edge cases (identity operands, P + P, P - P) test it directly
template <class F>
__global__ void __launch_bounds__(64) point_op_q4_kernel(int op, const JacobianMem* __restrict__ p, const void* __restrict__ q_in, JacobianMem* __restrict__ out, size_t n) {
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    const int q = threadIdx.x & 3;
    if (i >= n) return;  // n is padded to whole quads by construction: the four lanes of a pair share i
    auto coord = [&](const XYZZz<F>& v) { return q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.zz : v.zzz; };
    const Fy<F> a = coord(xyzzz_from_canonical(xyzz_from_jacobian(jac_load<F>(p[i]))));
    Fy<F> r;
    if (op == 3) r = q4_add(a, coord(xyzzz_from_canonical(xyzz_from_jacobian(jac_load<F>(((const JacobianMem*)q_in)[i])))), q);
    else r = q4_dbl(a, q);
    XYZZz<F> full;
    full.x = q4_perm<F, 0, 0, 0, 0>(r); full.y = q4_perm<F, 1, 1, 1, 1>(r); full.zz = q4_perm<F, 2, 2, 2, 2>(r); full.zzz = q4_perm<F, 3, 3, 3, 3>(r);
    if (q == 0) jac_store(jac_from_affine(xyzz_to_affine(xyzzz_to_canonical(full))), out[i]);
}

}  // namespace
}  // namespace trh

extern "C" {

int trh_point_sum(int curve, const uint64_t* pts, size_t count, uint64_t out[12]) {
    TRH_TRY(check_curve(curve));
    if (!out || (count && !pts)) { set_error("point_sum: null pointer"); return TRH_EINVAL; }
    return point_sum_host(curve, pts, count, out);
}

int trh_best_fft_fp(uint64_t* a, const uint64_t omega[4], uint32_t log_n) { return best_fft_host(TRH_FP, a, omega, log_n); }
int trh_best_fft_fq(uint64_t* a, const uint64_t omega[4], uint32_t log_n) { return best_fft_host(TRH_FQ, a, omega, log_n); }

int trh_ntt_dev(int field, void* a_dev, uint32_t log_n, const uint64_t omega[4], size_t batch, void* stream) {
    TRH_TRY(check_field(field));
    if (!a_dev || !omega) { set_error("ntt_dev: null pointer"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    Range range("trh_ntt_dev");
    return ntt_device(field, a_dev, log_n, omega, batch, (hipStream_t)stream);
}

int trh_field_scale_rows_dev(int field, void* a_dev, size_t rows, size_t row_len, size_t active_len, const uint64_t* factors, uint32_t period, void* stream) {
    TRH_TRY(check_field(field));
    if (!a_dev || !factors || period == 0 || period > 64 || active_len > row_len) { set_error("field_scale: bad arguments"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    Ctx& c = ctx();
    // factors are staged in a small ring so that back-to-back calls on one stream do not overwrite
    // a table a queued kernel still reads
    TRH_TRY(c.factors.ensure(16 * 64 * 32));
    char* slot = (char*)c.factors.p + (size_t)(c.factor_slot++ & 15) * 64 * 32;
    TRH_HIP_TRY(hipMemcpyAsync(slot, factors, (size_t)period * 32, hipMemcpyHostToDevice, (hipStream_t)stream));
    TRH_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // `factors` is caller memory
    return field_scale_periodic(field, a_dev, rows, row_len, active_len, slot, period, (hipStream_t)stream);
}
int trh_field_scale_periodic_dev(int field, void* a_dev, size_t n, const uint64_t* factors, uint32_t period, void* stream) {
    return trh_field_scale_rows_dev(field, a_dev, 1, n, n, factors, period, stream);
}
int trh_field_scale_dev(int field, void* a_dev, size_t n, const uint64_t factor[4], void* stream) {
    return trh_field_scale_periodic_dev(field, a_dev, n, factor, 1, stream);
}

int trh_field_op_dev(int field, int op, const void* a, const void* b, void* out, size_t n, void* stream) {
    TRH_TRY(check_field(field));
    TRH_ENTER(stream);
    if (!n) return TRH_OK;
    const unsigned gb = (unsigned)((n + 255) / 256);
    with_field(field, [&](auto f) { hipLaunchKernelGGL((field_op_kernel<decltype(f)>), dim3(gb), dim3(256), 0, (hipStream_t)stream, op, (const uint4*)a, (const uint4*)b, (uint4*)out, n); });
    TRH_HIP_TRY(hipGetLastError());
    return TRH_OK;
}
int trh_point_op_dev(int curve, int op, const void* p, const void* q, void* out, size_t n, void* stream) {
    TRH_TRY(check_curve(curve));
    TRH_ENTER(stream);
    if (!n) return TRH_OK;
    const unsigned gq = (unsigned)((n * 4 + 63) / 64), gb = (unsigned)((n + 63) / 64);
    if (op == 3 || op == 4) with_curve(curve, [&](auto cv) { hipLaunchKernelGGL((point_op_q4_kernel<typename decltype(cv)::Base>), dim3(gq), dim3(64), 0, (hipStream_t)stream, op, (const JacobianMem*)p, q, (JacobianMem*)out, n); });
    else with_curve(curve, [&](auto cv) { hipLaunchKernelGGL((point_op_kernel<typename decltype(cv)::Base>), dim3(gb), dim3(64), 0, (hipStream_t)stream, op, (const JacobianMem*)p, q, (JacobianMem*)out, n); });
    TRH_HIP_TRY(hipGetLastError());
    return TRH_OK;
}

}  // extern "C"
