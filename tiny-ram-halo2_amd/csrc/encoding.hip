// ff::Field::sqrt and GroupEncoding (the 32-byte compressed points of pasta_curves 0.4.1: `to_bytes` / `from_bytes`) on the device, and the
// host-side single-point forms a transcript needs.  What they serve: `Params::read` (halo2_proofs 0.2.0 poly/commitment.rs) decodes
// 2 * 2^k + 2 compressed points -- one square root each in a field of two-adicity 32 -- before a single base can be uploaded; here the 32-byte
// encodings cross the link and one kernel turns them into the resident 64-byte PODs (bases.hip trh_bases_create_compressed).
// The arithmetic is csrc/fieldsqrt.h (fixed schedule: no lane of a wavefront waits for another's Tonelli-Shanks rounds); one thread per
// element, grid-stride; the decompression's smallest invalid index is a verdict of one min word (verdict.h).  The per-field table of fieldsqrt.h lives in the context.
#include <string.h>

#include "ctx.h"
#include "fieldsqrt.h"
#include "verdict.h"

namespace trh {
namespace {

constexpr unsigned ENC_BLOCK = 256, ENC_MAX_BLOCKS = 4096;

template <class F>
__global__ void __launch_bounds__(ENC_BLOCK) sqrt_kernel(const uint4* __restrict__ a, uint4* __restrict__ out, unsigned char* __restrict__ flags, size_t n,
                                                         const SqrtTable<F>* __restrict__ tab) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint4 lo = a[2 * i], hi = a[2 * i + 1];
        bool sq;
        const Fe<F> r = fe_sqrt(fe_load<F>(lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w), &sq, tab);
        u32 w[8];
        fe_store(r, w);
        out[2 * i] = make_uint4(w[0], w[1], w[2], w[3]);
        out[2 * i + 1] = make_uint4(w[4], w[5], w[6], w[7]);
        flags[i] = sq ? 1 : 0;
    }
}

// enc: n x 8 words; out: n x 64 B PODs (invalid: all zero); ok: n bytes or null; first_bad: lowered to the smallest invalid index
template <class F>
__global__ void __launch_bounds__(ENC_BLOCK) decompress_kernel(const u32* __restrict__ enc, uint4* __restrict__ out, unsigned char* __restrict__ ok,
                                                               unsigned long long* __restrict__ first_bad, size_t n, const SqrtTable<F>* __restrict__ tab) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        u32 e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) e[k] = enc[8 * i + k];
        Fe<F> x, y;
        const bool valid = point_decode(e, x, y, tab);
        u32 wx[8], wy[8];
        fe_store(x, wx);
        fe_store(y, wy);
        out[4 * i] = make_uint4(wx[0], wx[1], wx[2], wx[3]);
        out[4 * i + 1] = make_uint4(wx[4], wx[5], wx[6], wx[7]);
        out[4 * i + 2] = make_uint4(wy[0], wy[1], wy[2], wy[3]);
        out[4 * i + 3] = make_uint4(wy[4], wy[5], wy[6], wy[7]);
        if (ok) ok[i] = valid ? 1 : 0;
        if (!valid) atomicMin(first_bad, (unsigned long long)i);
    }
}

template <class F>
__global__ void __launch_bounds__(ENC_BLOCK) compress_kernel(const uint4* __restrict__ xy, u32* __restrict__ enc, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint4 a = xy[4 * i], b = xy[4 * i + 1], c = xy[4 * i + 2], d = xy[4 * i + 3];
        u32 e[8];
        point_encode(fe_load<F>(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w), fe_load<F>(c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w), e);
#pragma unroll
        for (int k = 0; k < 8; ++k) enc[8 * i + k] = e[k];
    }
}

unsigned enc_grid(size_t n) {
    const size_t b = (n + ENC_BLOCK - 1) / ENC_BLOCK;
    return (unsigned)(b < ENC_MAX_BLOCKS ? b : ENC_MAX_BLOCKS);
}

// the context's copy of the field's table (built on the host by fieldsqrt.h itself)
template <class F> int sqrt_table_dev(const SqrtTable<F>** out) {
    DevBuf& d = ctx().sqrt_tab[F::ID];
    if (!d.p) {
        TRH_TRY(d.ensure(sizeof(SqrtTable<F>)));
        hipError_t e = hipMemcpy(d.p, sqrt_table_host<F>(), sizeof(SqrtTable<F>), hipMemcpyHostToDevice);
        if (e != hipSuccess) { d.release(); set_error("sqrt table upload: %s", hipGetErrorString(e)); return TRH_EHIP; }
    }
    *out = d.as<const SqrtTable<F>>();
    return TRH_OK;
}

template <class F> int field_sqrt_t(const void* a, void* out, void* flags, size_t n, hipStream_t s) {
    const SqrtTable<F>* tab;
    TRH_TRY(sqrt_table_dev<F>(&tab));
    hipLaunchKernelGGL((sqrt_kernel<F>), dim3(enc_grid(n)), dim3(ENC_BLOCK), 0, s, (const uint4*)a, (uint4*)out, (unsigned char*)flags, n, tab);
    TRH_HIP_TRY(hipGetLastError());
    return TRH_OK;
}

template <class F> int decompress_t(const void* bytes, void* xy, void* ok, size_t n, hipStream_t s, u64* first_bad) {
    Ctx& c = ctx();
    const SqrtTable<F>* tab;
    TRH_TRY(sqrt_table_dev<F>(&tab));
    unsigned long long* d_min;  // the verdict: the smallest invalid index
    TRH_TRY(verdict_begin(c, 0, 1, s, nullptr, &d_min));
    hipLaunchKernelGGL((decompress_kernel<F>), dim3(enc_grid(n)), dim3(ENC_BLOCK), 0, s, (const u32*)bytes, (uint4*)xy, (unsigned char*)ok, d_min, n, tab);
    TRH_HIP_TRY(hipGetLastError());
    if (first_bad) {  // without it the verdict is never read: no synchronisation
        const u64* min;
        TRH_TRY(verdict_read(c, s, nullptr, &min));
        *first_bad = min_or(min[0], n);
    }
    return TRH_OK;
}

template <class F> void point_to_bytes_t(const uint64_t* xyz, uint8_t* out) {
    JacobianMem j;
    memcpy(&j, xyz, 96);
    const Affine<F> a = xyzz_to_affine(xyzz_from_jacobian(jac_load<F>(j)));
    u32 e[8];
    point_encode(a.x, a.y, e);
    memcpy(out, e, 32);
}
template <class F> bool point_from_bytes_t(const uint8_t* in, uint64_t* out_xy) {
    u32 e[8];
    memcpy(e, in, 32);
    Affine<F> a;
    const bool valid = point_decode(e, a.x, a.y, sqrt_table_host<F>());
    AffineMem m;
    aff_store(a, m);
    memcpy(out_xy, &m, 64);
    return valid;
}

}  // namespace

int points_decompress_device(int curve, const void* bytes_dev, void* xy_dev, void* ok_dev, size_t n, hipStream_t s, u64* first_bad) {
    if (!n) { if (first_bad) *first_bad = 0; return TRH_OK; }
    return with_curve(curve, [&](auto cv) { return decompress_t<typename decltype(cv)::Base>(bytes_dev, xy_dev, ok_dev, n, s, first_bad); });
}
int points_compress_device(int curve, const void* xy_dev, void* bytes_dev, size_t n, hipStream_t s) {
    if (!n) return TRH_OK;
    with_curve(curve, [&](auto cv) { hipLaunchKernelGGL((compress_kernel<typename decltype(cv)::Base>), dim3(enc_grid(n)), dim3(ENC_BLOCK), 0, s, (const uint4*)xy_dev, (u32*)bytes_dev, n); });
    TRH_HIP_TRY(hipGetLastError());
    return TRH_OK;
}
int sqrt_table_device(int field_id, const void** out) {
    if (field_id == FpParams::ID) {
        const SqrtTable<FpParams>* t = nullptr;
        TRH_TRY(sqrt_table_dev<FpParams>(&t));
        *out = t;
    } else {
        const SqrtTable<FqParams>* t = nullptr;
        TRH_TRY(sqrt_table_dev<FqParams>(&t));
        *out = t;
    }
    return TRH_OK;
}
void encoding_release() { ctx().sqrt_tab[0].release(); ctx().sqrt_tab[1].release(); }

}  // namespace trh

using namespace trh;

extern "C" {

int trh_field_sqrt_dev(int field, const void* a_dev, void* out_dev, void* is_square_dev, size_t n, void* stream) {
    TRH_TRY(check_field(field));
    if (n && (!a_dev || !out_dev || !is_square_dev)) { set_error("field_sqrt_dev: null pointer"); return TRH_EINVAL; }
    if ((((uintptr_t)a_dev | (uintptr_t)out_dev) & 15) != 0) { set_error("field_sqrt_dev: elements must be 16-byte aligned"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    if (!n) return TRH_OK;
    Range range("trh_field_sqrt_dev");
    return with_field(field, [&](auto f) { return field_sqrt_t<decltype(f)>(a_dev, out_dev, is_square_dev, n, (hipStream_t)stream); });
}

int trh_points_compress_dev(int curve, const void* xy_dev, void* bytes_dev, size_t n, void* stream) {
    TRH_TRY(check_curve(curve));
    if (n && (!xy_dev || !bytes_dev)) { set_error("points_compress_dev: null pointer"); return TRH_EINVAL; }
    if (((uintptr_t)xy_dev & 15) != 0 || ((uintptr_t)bytes_dev & 3) != 0) { set_error("points_compress_dev: points must be 16-byte, encodings 4-byte aligned"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    Range range("trh_points_compress_dev");
    return points_compress_device(curve, xy_dev, bytes_dev, n, (hipStream_t)stream);
}

int trh_points_decompress_dev(int curve, const void* bytes_dev, void* xy_dev, void* ok_dev_or_null, size_t n, void* stream, uint64_t* first_bad_or_null) {
    TRH_TRY(check_curve(curve));
    if (n && (!xy_dev || !bytes_dev)) { set_error("points_decompress_dev: null pointer"); return TRH_EINVAL; }
    if (((uintptr_t)xy_dev & 15) != 0 || ((uintptr_t)bytes_dev & 3) != 0) { set_error("points_decompress_dev: points must be 16-byte, encodings 4-byte aligned"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    Range range("trh_points_decompress_dev");
    return points_decompress_device(curve, bytes_dev, xy_dev, ok_dev_or_null, n, (hipStream_t)stream, first_bad_or_null);
}

int trh_point_to_bytes(int curve, const uint64_t xyz[12], uint8_t out[32]) {
    TRH_TRY(check_curve(curve));
    if (!xyz || !out) { set_error("point_to_bytes: null pointer"); return TRH_EINVAL; }
    with_curve(curve, [&](auto cv) { point_to_bytes_t<typename decltype(cv)::Base>(xyz, out); });
    return TRH_OK;
}

int trh_point_from_bytes(int curve, const uint8_t in[32], uint64_t out_xy[8]) {
    TRH_TRY(check_curve(curve));
    if (!in || !out_xy) { set_error("point_from_bytes: null pointer"); return TRH_EINVAL; }
    const bool valid = with_curve(curve, [&](auto cv) { return point_from_bytes_t<typename decltype(cv)::Base>(in, out_xy); });
    if (!valid) { set_error("point_from_bytes: not the encoding of a point"); return TRH_EINVAL; }
    return TRH_OK;
}

}  // extern "C"
