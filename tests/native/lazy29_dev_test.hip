// Device driver of the lazy-domain case runner (lazy29_cases.h): reads a case file, runs every record on the device -- one thread per
// record, one kernel instantiation per (op, field) so that each operation is compiled as it is inside the library's kernels (the
// v_mad_i64_i32 blocks of field.h, not its plain C++) -- and through the host branch of the same headers in this binary, and
// writes both result sets (device first, then host).  tests/test_gpu_lazy29.py compares them limb for limb and against big integers.
// Every HIP call is checked: the first error ends the program with a non-zero status and nothing further is launched.
//   usage: lazy29_dev_test <case file> <result file>
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "lazy29_cases.h"

using namespace lz;

#define HIP_OK(call)                                                                                              \
    do {                                                                                                          \
        const hipError_t e_ = (call);                                                                             \
        if (e_ != hipSuccess) {                                                                                   \
            std::fprintf(stderr, "lazy29_dev: %s -> %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            std::exit(2);                                                                                         \
        }                                                                                                         \
    } while (0)

template <int OP, class F>
__global__ __launch_bounds__(256) void case_kernel(const Rec* __restrict__ recs, Out* __restrict__ outs, u32 first, u32 count) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const In in = recs[first + i].in;
    Out o;
    run_case<OP, F>(in, o);
    outs[first + i] = o;
}

template <int OP> static void launch_one(u32 field, const Rec* recs, Out* outs, u32 first, u32 count) {
    const dim3 grid((count + 255u) / 256u), block(256);
    if (field == 0) hipLaunchKernelGGL((case_kernel<OP, FpParams>), grid, block, 0, 0, recs, outs, first, count);
    else hipLaunchKernelGGL((case_kernel<OP, FqParams>), grid, block, 0, 0, recs, outs, first, count);
}
template <int OP = 0> static void launch(u32 op, u32 field, const Rec* recs, Out* outs, u32 first, u32 count) {
    if constexpr (OP < OP_COUNT) {
        if ((int)op == OP) launch_one<OP>(field, recs, outs, first, count); else launch<OP + 1>(op, field, recs, outs, first, count);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s <case file> <result file>\n", argv[0]); return 1; }
    std::vector<Rec> recs;
    if (!read_cases(argv[1], recs)) return 1;
    const size_t n = recs.size();
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
            HIP_OK(hipDeviceSynchronize());  // a fault is reported at its own operation, before the next one starts
            i = j;
        }
        HIP_OK(hipMemcpy(dev.data(), d_outs, n * sizeof(Out), hipMemcpyDeviceToHost));
        HIP_OK(hipFree(d_recs));
        HIP_OK(hipFree(d_outs));
    }
    for (size_t i = 0; i < n; ++i) host_case(recs[i], host[i]);
    if (!write_results(argv[2], dev, &host)) return 1;
    std::printf("lazy29_dev: %zu records ok\n", n);
    return 0;
}
