// Host-side shape decisions of the two headline operations, free of HIP types so that a plain C++ test can check them
// (tests/native/hostplan_test.cpp): where msm_host_tiled (capi.hip) cuts an MSM with host scalars into ranges, and how
// ntt.hip splits a transform into passes.
#pragma once
#include <cstddef>
#include <vector>

namespace trh {
namespace hostplan {

constexpr size_t MSM_HOST_BASES_SPLIT = (size_t)1 << 21;      // host bases: one range up to here, equal ranges of about 2^20 pairs above
constexpr size_t MSM_HOST_BASES_RANGE = (size_t)1 << 20;
constexpr size_t MSM_RESIDENT_SPLIT = (size_t)3 << 21;        // resident bases: one range up to here, then 2^21, 2^22, the rest

// range boundaries of one MSM over n pairs whose scalars (host_bases: and bases) cross PCIe: cut[0] = 0 < cut[1] < ... < cut.back() = n
// (n == 0: the one empty range {0, 0} -- the callers answer the empty sum before they get here)
inline std::vector<size_t> msm_host_cuts(bool host_bases, size_t n) {
    std::vector<size_t> cut(1, 0);
    if (host_bases && n > MSM_HOST_BASES_SPLIT) {  // equal ranges
        const size_t want = MSM_HOST_BASES_RANGE, nt = (n + want - 1) / want, len = (n + nt - 1) / nt;
        for (size_t o = len; o < n; o += len) cut.push_back(o);
    } else if (!host_bases && n > MSM_RESIDENT_SPLIT) {
        // growing ranges: 2^21, 2^22, then the rest -- the first upload is short, every later one hides under the range before it
        // (32 B per pair cross the link ~2x faster than they are multiplied), and most pairs run as one large MSM at the full rate
        cut.push_back((size_t)1 << 21);
        cut.push_back((size_t)3 << 21);
    }
    cut.push_back(n);
    return cut;
}

constexpr int NTT_TILE_LOG = 11;      // elements per workgroup tile of the NTT passes, log2
constexpr int NTT_MAX_PASS_LOG = 9;   // stages per pass at most

// pass plan: log_n split into passes of <= NTT_MAX_PASS_LOG stages on 2^tile_log-element tiles
inline void ntt_plan_passes(int log_n, int* sizes, int* n_passes, int* tile_log) {
    // (a 4096-element tile -- two passes for 2^19..2^22, all 160 KiB of LDS, one workgroup per CU -- measured equal: removed.  Round 6: 2^22 as
    //  two 11-stage passes on the 2048-element tile, pass 0 reading 64-KiB-strided columns: 0.83 ms against 0.47 for 8 + 7 + 7, the fabric
    //  fetches 4.8 x the bytes -- profiles/r06_ntt_11_11_ab.txt.)
    int P = 0;
    if (log_n <= NTT_TILE_LOG) { sizes[P++] = log_n; }
    else {
        P = (log_n + NTT_MAX_PASS_LOG - 1) / NTT_MAX_PASS_LOG;
        if (P < 2) P = 2;
        int rem = log_n;
        for (int p = 0; p < P; ++p) { sizes[p] = (rem + (P - p) - 1) / (P - p); rem -= sizes[p]; }
    }
    *n_passes = P; *tile_log = NTT_TILE_LOG;
}

}  // namespace hostplan
}  // namespace trh
