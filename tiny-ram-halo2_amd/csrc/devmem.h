// How the kernels move field elements and points between device memory and registers: the one definition of each accessor.
//
// Memory holds a field element as eight 32-bit words (canonical Montgomery form, FeMem) and the kernels read and write it as two uint4, so
// that every access is a 16-byte one.  The points follow: AffineMem is four uint4, XYZZMem eight, and XYZZzMem -- the raw limbs of a point
// of the lazy domain, scratch between two kernels and never seen by a caller -- nine.  curve.h's aff_load / xyzz_load take the same records
// by struct reference and word by word; which of the two forms a kernel uses decides the width of its loads, so they are not interchangeable.
// Layouts that belong to one kernel family stay with it (ntt.hip's split LDS planes, expr.hip's ldg_column, msm.hip's ZREC records).
#pragma once
#include "curve.h"

namespace trh {

template <class F>
__device__ __forceinline__ Fe<F> load_fe(const uint4* p) {
    uint4 a = p[0], b = p[1];
    return fe_load<F>(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w);
}
template <class F>
__device__ __forceinline__ void store_fe(uint4* p, const Fe<F>& v) {
    u32 w[8];
    fe_store(v, w);
    p[0] = make_uint4(w[0], w[1], w[2], w[3]);
    p[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// the field's zero: the same eight words in both fields
__device__ __forceinline__ void store_zero(uint4* p) {
    p[0] = make_uint4(0u, 0u, 0u, 0u);
    p[1] = make_uint4(0u, 0u, 0u, 0u);
}
// canonical Montgomery words -> the lazy domain (fy_load)
template <class F>
__device__ __forceinline__ Fy<F> load_fy(const uint4* p) {
    uint4 a = p[0], b = p[1];
    return fy_load<F>(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w);
}

template <class BF>
__device__ __forceinline__ Affine<BF> load_affine(const uint4* __restrict__ bases, u32 idx) {
    const uint4* p = bases + (size_t)idx * 4;
    uint4 a = p[0], b = p[1], c = p[2], d = p[3];
    Affine<BF> r;
    r.x = fe_load<BF>(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w);
    r.y = fe_load<BF>(c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w);
    return r;
}
template <class BF>
__device__ __forceinline__ void store_xyzz(XYZZMem* dst, const XYZZ<BF>& v) {
    uint4* p = (uint4*)dst;
    store_fe(p, v.x); store_fe(p + 2, v.y); store_fe(p + 4, v.zz); store_fe(p + 6, v.zzz);
}
template <class BF>
__device__ __forceinline__ XYZZ<BF> load_xyzz(const XYZZMem* src) {
    const uint4* p = (const uint4*)src;
    XYZZ<BF> v;
    v.x = load_fe<BF>(p); v.y = load_fe<BF>(p + 2); v.zz = load_fe<BF>(p + 4); v.zzz = load_fe<BF>(p + 6);
    return v;
}

// a point of the lazy domain, limbs as they are
template <class BF>
__device__ __forceinline__ void store_raw(XYZZzMem* dst, const XYZZz<BF>& v) {
    uint4* p = (uint4*)dst;
    const u32* w = (const u32*)&v;
#pragma unroll
    for (int k = 0; k < 9; ++k) p[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}
template <class BF>
__device__ __forceinline__ XYZZz<BF> load_raw(const XYZZzMem* src) {
    const uint4* p = (const uint4*)src;
    XYZZz<BF> v;
    u32* w = (u32*)&v;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        uint4 q = p[k];
        w[4 * k] = q.x; w[4 * k + 1] = q.y; w[4 * k + 2] = q.z; w[4 * k + 3] = q.w;
    }
    return v;
}
// lane i receives the point of lane i + off (inside groups of `width` lanes)
template <class BF>
__device__ __forceinline__ XYZZz<BF> shfl_down_point(const XYZZz<BF>& v, int off, int width) {
    XYZZz<BF> o;
#pragma unroll
    for (int l = 0; l < NLIMBS; ++l) {
        o.x.l[l] = __shfl_down(v.x.l[l], off, width); o.y.l[l] = __shfl_down(v.y.l[l], off, width);
        o.zz.l[l] = __shfl_down(v.zz.l[l], off, width); o.zzz.l[l] = __shfl_down(v.zzz.l[l], off, width);
    }
    return o;
}

}  // namespace trh
