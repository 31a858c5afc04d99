// csrc/hostplan.h without a device: the range boundaries msm_host_tiled (capi.hip) cuts an MSM with host scalars at, in both modes
// (host bases: equal ranges of ceil(n / ceil(n / 2^20)) pairs above 2^21; resident bases: 2^21, 2^22, the rest above 3 * 2^21), and the
// pass plan of the NTT for every accepted size.  The range counts asserted here are the ones the GPU tests expect from trh_stat
// "msm_host_ranges" (tests/test_gpu_dropin.py, tests/test_gpu_realsize.py).  Plain C++, run by tests/test_hostcombine.py.
#include <cstdio>

#include "../../tiny-ram-halo2_amd/csrc/hostplan.h"

int main() {
    using namespace trh::hostplan;
    int bad = 0;
    auto expect = [&](bool ok, const char* what, unsigned long long a, unsigned long long b) {
        if (!ok) { std::printf("hostplan: FAILED %s (%llu, %llu)\n", what, a, b); ++bad; }
    };
    const size_t M = (size_t)1 << 20;
    const size_t sizes[] = {0, 1, 2 * M, 2 * M + 1, 2 * M + M + 13, 16 * M, 6 * M, 6 * M + 1, 6 * M + 5, 32 * M + 3, 38 * M + 3, ((size_t)1 << 31) - 1};
    for (int host_bases = 0; host_bases < 2; ++host_bases) {
        for (size_t n : sizes) {
            const std::vector<size_t> cut = msm_host_cuts(host_bases != 0, n);
            expect(cut.size() >= 2, "at least one range", n, cut.size());
            if (cut.size() < 2) continue;
            expect(cut.front() == 0, "first boundary is 0", n, cut.front());
            expect(cut.back() == n, "last boundary is n", n, cut.back());
            if (n == 0) { expect(cut.size() == 2, "the empty sum is one (empty) range", n, cut.size()); continue; }
            size_t longest = 0;
            for (size_t t = 0; t + 1 < cut.size(); ++t) {
                expect(cut[t] < cut[t + 1], "boundaries strictly increasing: no empty range", n, t);
                if (cut[t + 1] - cut[t] > longest) longest = cut[t + 1] - cut[t];
            }
            const size_t ranges = cut.size() - 1;
            if (host_bases) {
                if (n <= 2 * M) expect(ranges == 1, "host bases: one range up to 2^21", n, ranges);
                else {
                    const size_t nt = (n + M - 1) / M, len = (n + nt - 1) / nt;
                    expect(ranges == (n + len - 1) / len, "host bases: ceil(n / len) ranges", n, ranges);
                    expect(longest == len && len <= M + 1, "host bases: ranges of ceil(n / ceil(n / 2^20)) <= 2^20 + 1 pairs", n, longest);
                    for (size_t t = 0; t + 2 < cut.size(); ++t) expect(cut[t + 1] - cut[t] == len, "host bases: equal ranges before the last", n, t);
                }
            } else {
                if (n <= 6 * M) expect(ranges == 1, "resident bases: one range up to 3 * 2^21", n, ranges);
                else expect(ranges == 3 && cut[1] == 2 * M && cut[2] == 6 * M, "resident bases: 2^21, 2^22, the rest", n, ranges);
            }
        }
    }
    // the counts the GPU tests assert
    auto ranges = [](bool hb, size_t n) { return msm_host_cuts(hb, n).size() - 1; };
    expect(ranges(true, 2 * M) == 1, "host bases 2^21", 2 * M, ranges(true, 2 * M));
    expect(ranges(true, 2 * M + 1) == 3, "host bases 2^21 + 1", 2 * M + 1, ranges(true, 2 * M + 1));
    {
        const std::vector<size_t> cut = msm_host_cuts(true, 3 * M + 13);
        expect(cut.size() == 5 && cut[1] == 786436 && cut[2] == 2 * 786436 && cut[3] == 3 * 786436 && cut[4] - cut[3] == 786433, "host bases 2^21 + 2^20 + 13: 3 x 786436 + 786433",
               3 * M + 13, cut.size() - 1);
    }
    expect(ranges(true, 16 * M) == 16, "host bases 2^24", 16 * M, ranges(true, 16 * M));
    expect(ranges(false, 6 * M) == 1 && ranges(false, 6 * M + 1) == 3 && ranges(false, 6 * M + 5) == 3 && ranges(false, 32 * M + 3) == 3, "resident bases around 3 * 2^21", 6 * M,
           ranges(false, 6 * M + 1));
    expect(msm_host_cuts(false, 6 * M + 5)[3] - msm_host_cuts(false, 6 * M + 5)[2] == 5, "resident bases 3 * 2^21 + 5: a last range of 5 pairs", 6 * M + 5, 0);
    expect(msm_host_cuts(false, 32 * M + 3)[3] - msm_host_cuts(false, 32 * M + 3)[2] == 27262979, "resident bases 2^25 + 3: a last range of 27262979 pairs", 32 * M + 3, 0);
    expect(ranges(false, 38 * M + 3) == 3 && msm_host_cuts(false, 38 * M + 3)[3] - msm_host_cuts(false, 38 * M + 3)[2] == 32 * M + 3,
           "resident bases 3 * 2^21 + 2^25 + 3: a last range above 2^25 pairs", 38 * M + 3, 0);

    // NTT pass plan
    for (int log_n = 1; log_n <= 27; ++log_n) {
        int s[8] = {0, 0, 0, 0, 0, 0, 0, 0}, P = 0, tlog = 0;
        ntt_plan_passes(log_n, s, &P, &tlog);
        int sum = 0;
        for (int p = 0; p < P; ++p) sum += s[p];
        expect(P >= 1 && P <= 3 && sum == log_n, "pass sizes sum to log_n", log_n, sum);
        expect(tlog == NTT_TILE_LOG, "tile size", log_n, tlog);
        if (log_n <= NTT_TILE_LOG) expect(P == 1, "one pass up to a tile", log_n, P);
        else {
            expect(P == (log_n <= 18 ? 2 : 3), "two passes for 12..18, three for 19..27", log_n, P);
            for (int p = 0; p < P; ++p) {
                expect(s[p] >= 2 && s[p] <= NTT_MAX_PASS_LOG, "2..9 stages per pass", log_n, s[p]);
                if (p) expect(s[p] <= s[p - 1] && s[p - 1] - s[p] <= 1, "passes differ by at most one stage, longest first", log_n, p);
            }
        }
    }
    {   // the shapes the GPU tests name
        int s[8], P, tlog;
        ntt_plan_passes(18, s, &P, &tlog); expect(P == 2 && s[0] == 9 && s[1] == 9, "2^18 is 9 + 9", 18, P);
        ntt_plan_passes(25, s, &P, &tlog); expect(P == 3 && s[0] == 9 && s[1] == 8 && s[2] == 8, "2^25 is 9 + 8 + 8", 25, P);
        ntt_plan_passes(26, s, &P, &tlog); expect(P == 3 && s[0] == 9 && s[1] == 9 && s[2] == 8, "2^26 is 9 + 9 + 8", 26, P);
        ntt_plan_passes(27, s, &P, &tlog); expect(P == 3 && s[0] == 9 && s[1] == 9 && s[2] == 9, "2^27 is 9 + 9 + 9", 27, P);
    }
    std::printf(bad ? "hostplan: FAILED (%d)\n" : "hostplan: ok\n", bad);
    return bad ? 1 : 0;
}
