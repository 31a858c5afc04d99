// One segment of the MSM's accumulation (msm_accumulate_seg_kernel, csrc/msm.hip) outside the library: one wave, 64 lanes, each running
// SEG = 128 consecutive mixed additions (xyzzz_madd_main, csrc/curve.h) onto ONE accumulator that lives in registers across the loop,
// with the accumulation's own handling of the lanes that meet p = acc (doubling) and p = -acc (the identity, then a fresh start).
// The same step runs through the plain C++ host branch of the headers in this binary.  After EVERY addition the 36 accumulator limbs
// and a code (0 generic, 1 doubled, 2 identity, 3 fresh start) are recorded; both traces are written (device first, then host) and
// tests/test_gpu_lazy29_segment.py compares them limb for limb and the end of every lane with the oracle's affine sum.
// Every HIP call is checked: the first error ends the program with a non-zero status and nothing further is launched.
//   usage: lazy29_segment_test <fp|fq> <point file> <trace file>
// Point file: LANES x (SEG + 1) affine points of the lazy domain, 18 signed limbs each (x, y), lane-major; a lane's first point starts
// its accumulator.  Trace file: 2 x LANES x SEG records of 37 words.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../tiny-ram-halo2_amd/csrc/curve.h"

using namespace trh;

#define HIP_OK(call)                                                                                                  \
    do {                                                                                                              \
        const hipError_t e_ = (call);                                                                                 \
        if (e_ != hipSuccess) {                                                                                       \
            std::fprintf(stderr, "lazy29_segment: %s -> %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            std::exit(2);                                                                                             \
        }                                                                                                             \
    } while (0)

constexpr int LANES = 64, SEG = 128, PT_WORDS = 2 * NLIMBS, REC_WORDS = 4 * NLIMBS + 1;

template <class F> TRH_HD AffineZ<F> load_point(const i32* w) {
    AffineZ<F> p;
#pragma unroll
    for (int i = 0; i < NLIMBS; ++i) { p.x.l[i] = w[i]; p.y.l[i] = w[NLIMBS + i]; }
    return p;
}
template <class F> TRH_HD void store_rec(i32* w, const XYZZz<F>& a, u32 code) {
#pragma unroll
    for (int i = 0; i < NLIMBS; ++i) { w[i] = a.x.l[i]; w[NLIMBS + i] = a.y.l[i]; w[2 * NLIMBS + i] = a.zz.l[i]; w[3 * NLIMBS + i] = a.zzz.l[i]; }
    w[4 * NLIMBS] = (i32)code;
}
// one step of the accumulation loop
template <class F> TRH_HD u32 seg_step(XYZZz<F>& acc, bool& fresh, const AffineZ<F>& p) {
    if (fresh) {
        acc.x = p.x; acc.y = p.y; acc.zz = fy_one<F>(); acc.zzz = fy_one<F>();
        fresh = false;
        return 3;
    }
    Fy<F> R;
    const bool same_x = xyzzz_madd_main(acc, p, R);
    if (same_x) {
        if (fy_is_zero_mod(R)) { acc = xyzzz_dbl_affine(p); return 1; }
        acc = xyzzz_identity<F>();
        fresh = true;
        return 2;
    }
    return 0;
}
template <class F> TRH_HD void run_lane(const i32* pts, i32* trace, int lane) {
    const i32* mine = pts + (size_t)lane * (SEG + 1) * PT_WORDS;
    XYZZz<F> acc;
    bool fresh = true;
    seg_step(acc, fresh, load_point<F>(mine));
    for (int s = 0; s < SEG; ++s) {
        const u32 code = seg_step(acc, fresh, load_point<F>(mine + (size_t)(s + 1) * PT_WORDS));
        store_rec(trace + ((size_t)lane * SEG + s) * REC_WORDS, acc, code);
    }
}
// one wave: lane = threadIdx.x < LANES; pts holds LANES x (SEG + 1) points, trace LANES x SEG records
template <class F> __global__ __launch_bounds__(64) void segment_kernel(const i32* __restrict__ pts, i32* __restrict__ trace) {
    if (threadIdx.x < LANES && blockIdx.x == 0) run_lane<F>(pts, trace, (int)threadIdx.x);
}

int main(int argc, char** argv) {
    if (argc != 4 || (std::strcmp(argv[1], "fp") != 0 && std::strcmp(argv[1], "fq") != 0)) {
        std::fprintf(stderr, "usage: %s <fp|fq> <point file> <trace file>\n", argv[0]);
        return 1;
    }
    const bool fp = std::strcmp(argv[1], "fp") == 0;
    const size_t n_pts = (size_t)LANES * (SEG + 1) * PT_WORDS, n_trace = (size_t)LANES * SEG * REC_WORDS;
    std::vector<i32> pts(n_pts), dev(n_trace), host(n_trace);
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f || std::fread(pts.data(), 4, n_pts, f) != n_pts || std::fgetc(f) != EOF) { std::fprintf(stderr, "%s: not a point file\n", argv[2]); return 1; }
    std::fclose(f);
    i32 *d_pts = nullptr, *d_trace = nullptr;
    HIP_OK(hipMalloc(&d_pts, n_pts * 4));
    HIP_OK(hipMalloc(&d_trace, n_trace * 4));
    HIP_OK(hipMemcpy(d_pts, pts.data(), n_pts * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_trace, 0xff, n_trace * 4));  // a record the kernel did not write cannot pass for a result
    if (fp) hipLaunchKernelGGL(segment_kernel<FpParams>, dim3(1), dim3(64), 0, 0, d_pts, d_trace);
    else hipLaunchKernelGGL(segment_kernel<FqParams>, dim3(1), dim3(64), 0, 0, d_pts, d_trace);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(dev.data(), d_trace, n_trace * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_pts));
    HIP_OK(hipFree(d_trace));
    for (int lane = 0; lane < LANES; ++lane) {
        if (fp) run_lane<FpParams>(pts.data(), host.data(), lane); else run_lane<FqParams>(pts.data(), host.data(), lane);
    }
    f = std::fopen(argv[3], "wb");
    if (!f) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 1; }
    const bool ok = std::fwrite(dev.data(), 4, n_trace, f) == n_trace && std::fwrite(host.data(), 4, n_trace, f) == n_trace;
    if (std::fclose(f) != 0 || !ok) return 1;
    std::printf("lazy29_segment: %d lanes x %d additions ok\n", LANES, SEG);
    return 0;
}
