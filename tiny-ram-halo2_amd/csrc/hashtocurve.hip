// Params::new on the device: trh_hash_to_field_indexed_dev, trh_map_to_curve_dev, trh_hash_to_curve_indexed_dev and the host-side
// trh_hash_to_curve (include/trh.h) over csrc/blake2b.h and csrc/hashtocurve.h.
// What they serve: halo2_proofs 0.2.0 `Params::new(k)` calls `C::hash_to_curve("Halo2-Parameters")` for each of its 2^k generators on
// the host -- three BLAKE2b hashes of two blocks, two simplified-SWU maps with a square root each, an addition and a 3-isogeny per point
// -- before the first base can be uploaded.  The points are independent and every one takes the same instructions, so they are made
// where they are used: one index per lane.
// Two kernels, because their register needs have nothing in common: the hash keeps 16 + 16 + 8 64-bit words of BLAKE2b state and no field
// element until its last step, the map keeps a dozen nine-limb elements and no hash state.  The fused entry runs them back to back over
// a scratch buffer of the context (64 bytes per point, in chunks of H2C_CHUNK points), on the caller's stream.
// No LDS, no cross-lane work.  What every lane shares -- b0's first chaining value, DST' -- travels in the hash kernel's arguments
// (H2cPlan); the square-root table is the context's (encoding.hip).
#include <string.h>

#include "ctx.h"
#include "devmem.h"
#include "hashtocurve.h"

namespace trh {
namespace {

constexpr unsigned H2C_BLOCK = 256;
constexpr size_t H2C_CHUNK = (size_t)1 << 18;  // points per pair of launches of the fused entry: 16 MiB of scratch

// u[2 i], u[2 i + 1] = hash_to_field(tag || le32(first + i)); first + n <= 2^32, so the index does not wrap
template <class F>
__global__ void __launch_bounds__(H2C_BLOCK) h2c_hash_kernel(uint4* __restrict__ u, size_t n, u32 first, const H2cPlan plan) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fe<F> u0, u1;
    h2c_hash_to_field_indexed<F>(plan, first + (u32)i, u0, u1);
    store_fe(u + 4 * i, u0);
    store_fe(u + 4 * i + 2, u1);
}

// xy[i] = iso_map(sum over j < per_point of swu(u[i per_point + j])), affine, the identity as the all-zero POD
template <class F>
__global__ void __launch_bounds__(H2C_BLOCK) h2c_map_kernel(const uint4* __restrict__ u, uint4* __restrict__ xy, size_t n, int per_point,
                                                            const SqrtTable<F>* __restrict__ tab) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    XYZZ<F> acc = xyzz_identity<F>();
#pragma unroll 1
    for (int j = 0; j < per_point; ++j) h2c_accumulate(acc, load_fe<F>(u + 2 * (i * per_point + j)), tab);
    const Affine<F> p = xyzz_to_affine(acc);
    store_fe(xy + 4 * i, p.x);
    store_fe(xy + 4 * i + 2, p.y);
}

int h2c_grid(const char* who, size_t n, unsigned* blocks) {
    const size_t b = (n + H2C_BLOCK - 1) / H2C_BLOCK;
    if (b > 0x7fffffffu) { set_error("%s: %zu elements exceed one launch", who, n); return TRH_EINVAL; }
    *blocks = (unsigned)b;
    return TRH_OK;
}

// prefix: NUL-terminated, at most H2C_MAX_PREFIX bytes
int h2c_dst(const char* who, int curve, const char* prefix, uint8_t dstp[H2C_MAX_DSTP], size_t* dstp_len) {
    if (!prefix) { set_error("%s: null pointer", who); return TRH_EINVAL; }
    const size_t len = strnlen(prefix, H2C_MAX_PREFIX + 1);
    if (len > H2C_MAX_PREFIX) { set_error("%s: the prefix is longer than %zu bytes", who, H2C_MAX_PREFIX); return TRH_EINVAL; }
    *dstp_len = h2c_dst_prime(curve == TRH_PALLAS, prefix, len, dstp);
    return TRH_OK;
}
int h2c_range(const char* who, u32 first, size_t n) {
    if ((u64)n > ((u64)1 << 32) - (u64)first) { set_error("%s: indices [%u, %u + %zu) pass 2^32", who, first, first, n); return TRH_EINVAL; }
    return TRH_OK;
}

template <class F> int hash_launch(const H2cPlan& plan, u32 first, size_t n, void* u_dev, hipStream_t s) {
    unsigned blocks = 0;
    TRH_TRY(h2c_grid("hash_to_field_indexed_dev", n, &blocks));
    hipLaunchKernelGGL((h2c_hash_kernel<F>), dim3(blocks), dim3(H2C_BLOCK), 0, s, (uint4*)u_dev, n, first, plan);
    TRH_HIP_TRY(hipGetLastError());
    return TRH_OK;
}
template <class F> int map_launch(const void* u_dev, size_t n, int per_point, void* xy_dev, hipStream_t s) {
    unsigned blocks = 0;
    TRH_TRY(h2c_grid("map_to_curve_dev", n, &blocks));
    const void* tab = nullptr;
    TRH_TRY(sqrt_table_device(F::ID, &tab));
    hipLaunchKernelGGL((h2c_map_kernel<F>), dim3(blocks), dim3(H2C_BLOCK), 0, s, (const uint4*)u_dev, (uint4*)xy_dev, n, per_point, (const SqrtTable<F>*)tab);
    TRH_HIP_TRY(hipGetLastError());
    return TRH_OK;
}

template <class F> void hash_to_curve_host_t(const uint8_t* dstp, size_t dstp_len, const uint8_t* msg, size_t msg_len, uint64_t* out_xy) {
    Fe<F> u0, u1;
    h2c_hash_to_field_bytes<F>(dstp, dstp_len, msg, msg_len, u0, u1);
    XYZZ<F> acc = xyzz_identity<F>();
    h2c_accumulate(acc, u0, sqrt_table_host<F>());
    h2c_accumulate(acc, u1, sqrt_table_host<F>());
    AffineMem m;
    aff_store(xyzz_to_affine(acc), m);
    memcpy(out_xy, &m, 64);
}

}  // namespace

void hashtocurve_release() { ctx().h2c_u.release(); }

}  // namespace trh

using namespace trh;

extern "C" {

int trh_hash_to_curve(int curve, const char* prefix, const uint8_t* msg, size_t msg_len, uint64_t out_xy[8]) {
    TRH_TRY(check_curve(curve));
    if (!out_xy || (msg_len && !msg)) { set_error("hash_to_curve: null pointer"); return TRH_EINVAL; }
    uint8_t dstp[H2C_MAX_DSTP];
    size_t dstp_len = 0;
    TRH_TRY(h2c_dst("hash_to_curve", curve, prefix, dstp, &dstp_len));
    with_curve(curve, [&](auto cv) { hash_to_curve_host_t<typename decltype(cv)::Base>(dstp, dstp_len, msg, msg_len, out_xy); });
    return TRH_OK;
}

int trh_hash_to_field_indexed_dev(int curve, const char* prefix, uint8_t tag, uint32_t first, size_t n, void* u_dev, void* stream) {
    TRH_TRY(check_curve(curve));
    uint8_t dstp[H2C_MAX_DSTP];
    size_t dstp_len = 0;
    TRH_TRY(h2c_dst("hash_to_field_indexed_dev", curve, prefix, dstp, &dstp_len));
    TRH_TRY(h2c_range("hash_to_field_indexed_dev", first, n));
    if (n && !u_dev) { set_error("hash_to_field_indexed_dev: null pointer"); return TRH_EINVAL; }
    if (((uintptr_t)u_dev & 15) != 0) { set_error("hash_to_field_indexed_dev: elements must be 16-byte aligned"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    if (!n) return TRH_OK;
    Range range("trh_hash_to_field_indexed_dev");
    H2cPlan plan;
    h2c_plan_build(plan, dstp, dstp_len, tag);
    return with_curve(curve, [&](auto cv) { return hash_launch<typename decltype(cv)::Base>(plan, first, n, u_dev, (hipStream_t)stream); });
}

int trh_map_to_curve_dev(int curve, const void* u_dev, size_t n, int per_point, void* xy_dev, void* stream) {
    TRH_TRY(check_curve(curve));
    if (per_point != 1 && per_point != 2) { set_error("map_to_curve_dev: per_point %d is neither 1 nor 2", per_point); return TRH_EINVAL; }
    if (n && (!u_dev || !xy_dev)) { set_error("map_to_curve_dev: null pointer"); return TRH_EINVAL; }
    if ((((uintptr_t)u_dev | (uintptr_t)xy_dev) & 15) != 0) { set_error("map_to_curve_dev: elements and points must be 16-byte aligned"); return TRH_EINVAL; }
    if (n > ((size_t)-1 >> 7)) { set_error("map_to_curve_dev: n out of range"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    if (!n) return TRH_OK;
    Range range("trh_map_to_curve_dev");
    return with_curve(curve, [&](auto cv) { return map_launch<typename decltype(cv)::Base>(u_dev, n, per_point, xy_dev, (hipStream_t)stream); });
}

int trh_hash_to_curve_indexed_dev(int curve, const char* prefix, uint8_t tag, uint32_t first, size_t n, void* xy_dev, void* stream) {
    TRH_TRY(check_curve(curve));
    uint8_t dstp[H2C_MAX_DSTP];
    size_t dstp_len = 0;
    TRH_TRY(h2c_dst("hash_to_curve_indexed_dev", curve, prefix, dstp, &dstp_len));
    TRH_TRY(h2c_range("hash_to_curve_indexed_dev", first, n));
    if (n && !xy_dev) { set_error("hash_to_curve_indexed_dev: null pointer"); return TRH_EINVAL; }
    if (((uintptr_t)xy_dev & 15) != 0) { set_error("hash_to_curve_indexed_dev: points must be 16-byte aligned"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    if (!n) return TRH_OK;
    Range range("trh_hash_to_curve_indexed_dev");
    DevBuf& scratch = ctx().h2c_u;
    TRH_TRY(scratch.ensure((n < H2C_CHUNK ? n : H2C_CHUNK) * 64));
    H2cPlan plan;
    h2c_plan_build(plan, dstp, dstp_len, tag);
    // chunk by chunk on one stream: the map of a chunk has read the scratch before the next chunk's hash writes it
    for (size_t done = 0; done < n; done += H2C_CHUNK) {
        const size_t cnt = n - done < H2C_CHUNK ? n - done : H2C_CHUNK;
        TRH_TRY(with_curve(curve, [&](auto cv) {
            typedef typename decltype(cv)::Base F;
            TRH_TRY(hash_launch<F>(plan, first + (u32)done, cnt, scratch.p, (hipStream_t)stream));
            return map_launch<F>(scratch.p, cnt, 2, (char*)xy_dev + done * 64, (hipStream_t)stream);
        }));
    }
    return TRH_OK;
}

}  // extern "C"
