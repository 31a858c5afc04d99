// In-place and shared operands of the lazy domain's product forms (csrc/field.h: fy_mul, fy_mul_nonneg, fy_sqr, fy_mul2, fy_mul_sub,
// fy_sqr_sub_sub2).  The records of lazy29_dev_test keep every operand and the result in slots of their own; here the result is
// written over each operand in turn, and one value sits in several operand slots -- the calls at which a wrong constraint of the
// column blocks (a missing early clobber, a tied operand) would let a result limb land in a register whose operand limb is still to be
// read.  One kernel instantiation per (shape, field), one thread per record, then the host branch of the same headers in this
// binary; both result sets are written (device first, then host) and tests/test_gpu_lazy29_alias.py compares them limb for limb.
// Every HIP call is checked: the first error ends the program with a non-zero status and nothing further is launched.
//   usage: lazy29_alias_test <case file> <result file>
// Case file: records of lazy29_cases.h (op = shape below, field, operand slots a, b, c, d); result: slots 0 .. 3 = a, b, c, d after the call.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "lazy29_cases.h"

using namespace lz;

#define HIP_OK(call)                                                                                                \
    do {                                                                                                            \
        const hipError_t e_ = (call);                                                                               \
        if (e_ != hipSuccess) {                                                                                     \
            std::fprintf(stderr, "lazy29_alias: %s -> %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            std::exit(2);                                                                                           \
        }                                                                                                           \
    } while (0)

enum Shape : int {
    MUL_A = 0, MUL_B, MUL_AA,                            // a = mul(a, b); b = mul(a, b); a = mul(a, a)
    NONNEG_A, NONNEG_B, NONNEG_AA,
    SQR_A,                                               // a = sqr(a)
    MUL2_A, MUL2_B, MUL2_C, MUL2_D, MUL2_ABAB,           // x = mul2(a, b, c, d) for each x; a = mul2(a, b, a, b)
    MUL_SUB_A, MUL_SUB_B, MUL_SUB_S, MUL_SUB_AAA,        // x = mul_sub(a, b, c) for each x; a = mul_sub(a, a, a)
    SQR_SUB_A, SQR_SUB_S1, SQR_SUB_S2, SQR_SUB_AAA,      // x = sqr_sub_sub2(a, b, c) for each x; a = sqr_sub_sub2(a, a, a)
    SHAPE_COUNT
};

template <int S, class F> TRH_HD void run_shape(const In& in, Out& o) {
    Fy<F> a = get<F>(in, 0), b = get<F>(in, 1), c = get<F>(in, 2), d = get<F>(in, 3);
    if constexpr (S == MUL_A) a = fy_mul(a, b);
    else if constexpr (S == MUL_B) b = fy_mul(a, b);
    else if constexpr (S == MUL_AA) a = fy_mul(a, a);
    else if constexpr (S == NONNEG_A) a = fy_mul_nonneg(a, b);
    else if constexpr (S == NONNEG_B) b = fy_mul_nonneg(a, b);
    else if constexpr (S == NONNEG_AA) a = fy_mul_nonneg(a, a);
    else if constexpr (S == SQR_A) a = fy_sqr(a);
    else if constexpr (S == MUL2_A) a = fy_mul2(a, b, c, d);
    else if constexpr (S == MUL2_B) b = fy_mul2(a, b, c, d);
    else if constexpr (S == MUL2_C) c = fy_mul2(a, b, c, d);
    else if constexpr (S == MUL2_D) d = fy_mul2(a, b, c, d);
    else if constexpr (S == MUL2_ABAB) a = fy_mul2(a, b, a, b);
    else if constexpr (S == MUL_SUB_A) a = fy_mul_sub(a, b, c);
    else if constexpr (S == MUL_SUB_B) b = fy_mul_sub(a, b, c);
    else if constexpr (S == MUL_SUB_S) c = fy_mul_sub(a, b, c);
    else if constexpr (S == MUL_SUB_AAA) a = fy_mul_sub(a, a, a);
    else if constexpr (S == SQR_SUB_A) a = fy_sqr_sub_sub2(a, b, c);
    else if constexpr (S == SQR_SUB_S1) b = fy_sqr_sub_sub2(a, b, c);
    else if constexpr (S == SQR_SUB_S2) c = fy_sqr_sub_sub2(a, b, c);
    else if constexpr (S == SQR_SUB_AAA) a = fy_sqr_sub_sub2(a, a, a);
#pragma unroll
    for (int i = 0; i < NLIMBS; ++i) o.r[4][i] = 0;
    o.flag = 0;
    put(o, 0, a); put(o, 1, b); put(o, 2, c); put(o, 3, d);
}

template <int S, class F>
__global__ __launch_bounds__(256) void shape_kernel(const Rec* __restrict__ recs, Out* __restrict__ outs, u32 first, u32 count) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;  // first + i < first + count <= number of records: both arrays hold that many
    const In in = recs[first + i].in;
    Out o;
    run_shape<S, F>(in, o);
    outs[first + i] = o;
}

template <int S = 0> static void launch(u32 shape, u32 field, const Rec* recs, Out* outs, u32 first, u32 count) {
    if constexpr (S < SHAPE_COUNT) {
        if ((int)shape != S) return launch<S + 1>(shape, field, recs, outs, first, count);
        const dim3 grid((count + 255u) / 256u), block(256);
        if (field == 0) hipLaunchKernelGGL((shape_kernel<S, FpParams>), grid, block, 0, 0, recs, outs, first, count);
        else hipLaunchKernelGGL((shape_kernel<S, FqParams>), grid, block, 0, 0, recs, outs, first, count);
    }
}
template <int S = 0> static void host_shape(const Rec& r, Out& o) {
    if constexpr (S < SHAPE_COUNT) {
        if ((int)r.op != S) return host_shape<S + 1>(r, o);
        if (r.field == 0) run_shape<S, FpParams>(r.in, o); else run_shape<S, FqParams>(r.in, o);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s <case file> <result file>\n", argv[0]); return 1; }
    static_assert((int)SHAPE_COUNT <= (int)OP_COUNT, "read_cases bounds the op word by OP_COUNT");
    std::vector<Rec> recs;
    if (!read_cases(argv[1], recs)) return 1;
    const size_t n = recs.size();
    for (size_t i = 0; i < n; ++i)
        if (recs[i].op >= (u32)SHAPE_COUNT) { std::fprintf(stderr, "record %zu: no such shape\n", i); return 1; }
    std::vector<Out> dev(n), host(n);
    if (n) {
        Rec* d_recs = nullptr;
        Out* d_outs = nullptr;
        HIP_OK(hipMalloc(&d_recs, n * sizeof(Rec)));
        HIP_OK(hipMalloc(&d_outs, n * sizeof(Out)));
        HIP_OK(hipMemcpy(d_recs, recs.data(), n * sizeof(Rec), hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_outs, 0xff, n * sizeof(Out)));  // a record no kernel wrote cannot pass for a result
        for (size_t i = 0; i < n;) {
            const size_t j = run_end(recs, i);
            launch(recs[i].op, recs[i].field, d_recs, d_outs, (u32)i, (u32)(j - i));
            HIP_OK(hipGetLastError());
            HIP_OK(hipDeviceSynchronize());  // a fault is reported at its own shape, before the next one starts
            i = j;
        }
        HIP_OK(hipMemcpy(dev.data(), d_outs, n * sizeof(Out), hipMemcpyDeviceToHost));
        HIP_OK(hipFree(d_recs));
        HIP_OK(hipFree(d_outs));
    }
    for (size_t i = 0; i < n; ++i) host_shape(recs[i], host[i]);
    if (!write_results(argv[2], dev, &host)) return 1;
    std::printf("lazy29_alias: %zu records ok\n", n);
    return 0;
}
