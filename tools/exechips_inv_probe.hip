// The inversion kernel of trh_exe_chips_dev (csrc/exechips_inv.h) on its own, at strips of B = 1 (a plain fe_inv per row), 4 and 8 rows per
// lane: tools/exechips_inv_probe [log2 rows, default 18] [reps, default 9]   (make tools/exechips_inv_probe; tools/exechips_probe.py runs it)
// One column of 2^k - 1 rows of Fp, every second opcode drawn with the flag2 bit -- about half the rows, as in a trace at k = 18 -- and
// non-zero denominators on them.  Device events around the kernel alone (the column is restored before each run, outside the window),
// medians of `reps` after one untimed run each, alternating; hipMemsetAsync of the same column is the fill next to it.  Before anything is
// timed the three results are compared word for word, and B = 1's is checked to be the inverse (x * x^-1 = 1 through the same fe_mul on
// the host).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tiny-ram-halo2_amd/csrc/exechips_inv.h"

using namespace trh;
using namespace trh::exetable;

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <u32 B>
static void launch(const u32* inst, size_t m, const Selection& chips, uint4* column, unsigned long long* count, hipStream_t s) {
    hipLaunchKernelGGL((exe_chips_inverse_kernel<FpParams, B>), dim3(exe_chips_inverse_blocks(m, B)), dim3(EXE_THREADS), 0, s, inst, m, chips, column, count);
}

int main(int argc, char** argv) {
    const int k = argc > 1 ? std::atoi(argv[1]) : 18, reps = argc > 2 ? std::atoi(argv[2]) : 9;
    if (k < 8 || k > 24 || reps < 1) { std::fprintf(stderr, "usage: exechips_inv_probe [log2 rows 8 .. 24] [reps]\n"); return 2; }
    const size_t n = (size_t)1 << k, m = n - 1;
    u64 x = 0x9e3779b97f4a7c15ull;
    auto next = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    Selection chips;
    for (u32 o = 0; o < OPCODES; ++o) chips.e[o] = o & 1u ? (u32)TRH_CHIP_FLAG2 : 0u;
    std::vector<u32> inst(m), column(n * 8, 0u);
    size_t flag2 = 0;
    for (size_t r = 0; r < m; ++r) {
        inst[r] = (u32)(next() & 31u);
        if (!(inst[r] & 1u)) continue;
        ++flag2;
        for (int w = 0; w < 8; ++w) column[r * 8 + w] = (u32)next();
        column[r * 8 + 7] &= 0x3fffffffu;  // below the modulus (2^254 + ...): a canonical element, non-zero
    }
    u32 *d_inst; uint4 *d_pristine, *d_column; unsigned long long* d_count;
    HIP_OK(hipMalloc(&d_inst, m * 4)); HIP_OK(hipMalloc(&d_pristine, n * 32)); HIP_OK(hipMalloc(&d_column, n * 32)); HIP_OK(hipMalloc(&d_count, 8));
    HIP_OK(hipMemcpy(d_inst, inst.data(), m * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_pristine, column.data(), n * 32, hipMemcpyHostToDevice));
    hipStream_t s = nullptr;
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
    const char* names[4] = {"B = 1 (fe_inv per row)", "B = 4", "B = 8", "hipMemsetAsync of the column"};
    auto run = [&](int which, float* ms) -> int {
        HIP_OK(hipMemcpyAsync(d_column, d_pristine, n * 32, hipMemcpyDeviceToDevice, s));
        HIP_OK(hipMemsetAsync(d_count, 0, 8, s));
        HIP_OK(hipEventRecord(e0, s));
        if (which == 0) launch<1>(d_inst, m, chips, d_column, d_count, s);
        else if (which == 1) launch<4>(d_inst, m, chips, d_column, d_count, s);
        else if (which == 2) launch<8>(d_inst, m, chips, d_column, d_count, s);
        else HIP_OK(hipMemsetAsync(d_column, 0, n * 32, s));
        HIP_OK(hipGetLastError());
        HIP_OK(hipEventRecord(e1, s));
        HIP_OK(hipEventSynchronize(e1));
        HIP_OK(hipEventElapsedTime(ms, e0, e1));
        return 0;
    };
    // the untimed runs, compared with each other
    std::vector<u32> got[3];
    float ms = 0;
    for (int which = 0; which < 3; ++which) {
        if (run(which, &ms)) return 1;
        got[which].resize(n * 8);
        HIP_OK(hipMemcpy(got[which].data(), d_column, n * 32, hipMemcpyDeviceToHost));
        unsigned long long counted = 0;
        HIP_OK(hipMemcpy(&counted, d_count, 8, hipMemcpyDeviceToHost));
        if (counted != flag2) { std::fprintf(stderr, "%s counted %llu flag2 rows of %zu\n", names[which], counted, flag2); return 1; }
    }
    if (got[0] != got[1] || got[0] != got[2]) { std::fprintf(stderr, "the strips disagree\n"); return 1; }
    for (size_t r = 0; r < m; r += 997) {
        const Fe<FpParams> a = fe_load<FpParams>(&column[r * 8]), b = fe_load<FpParams>(&got[0][r * 8]);
        const bool ok = inst[r] & 1u ? fe_eq(fe_mul(a, b), fe_one<FpParams>()) : std::memcmp(&column[r * 8], &got[0][r * 8], 32) == 0;
        if (!ok) { std::fprintf(stderr, "row %zu is not the inverse\n", r); return 1; }
    }
    if (run(3, &ms)) return 1;
    std::vector<float> times[4];
    for (int rep = 0; rep < reps; ++rep)
        for (int which = 0; which < 4; ++which) {
            if (run(which, &ms)) return 1;
            times[which].push_back(ms);
        }
    std::printf("inversion kernel alone, Fp, k = %d: %zu rows, %zu with flag2 (%.0f MB read and written); the three strips agree word for word\n", k, m, flag2,
                2.0 * flag2 * 32 / 1e6);
    float med[4];
    for (int which = 0; which < 4; ++which) {
        std::sort(times[which].begin(), times[which].end());
        med[which] = times[which][times[which].size() / 2];
        std::printf("   %-44s: median %9.3f ms, min %9.3f, max %9.3f\n", names[which], med[which], times[which].front(), times[which].back());
    }
    std::printf("   B = 1 / fill = %.1f; B = 4 / fill = %.1f; B = 8 / fill = %.1f; B = 1 / B = 4 = %.2f; B = 4 / B = 8 = %.2f\n", med[0] / med[3], med[1] / med[3], med[2] / med[3],
                med[0] / med[1], med[1] / med[2]);
    (void)hipFree(d_inst); (void)hipFree(d_pristine); (void)hipFree(d_column); (void)hipFree(d_count);
    return 0;
}
