// csrc/hostplan.h without a device: the range boundaries msm_host_tiled (msmapi.hip) cuts an MSM with host scalars at, in both modes
// (host bases: equal ranges of ceil(n / ceil(n / 2^20)) pairs above 2^21; resident bases: 2^21, 2^22, the rest above 3 * 2^21), and the
// pass plan of the NTT for every accepted size and the number of transforms its lazy passes run per launch set (ntt_lazy_chunk: the invariants
// over log_n 12..27 and the block counts in use, and the literal values tests/test_gpu_domain_chunks.py builds its cases on).  The range counts asserted here are the ones the GPU tests expect from trh_stat
// "msm_host_ranges" (tests/test_gpu_dropin.py, tests/test_gpu_realsize.py).  Then the launch plan of an MSM on the device (msm_route, msm_plan):
// the invariants the kernels of msm.hip rely on over a sweep of shapes, the routes at their edges and the geometry of named shapes.
// Then the plan of an IPA opening (ipa_plan): the invariants of every shape the entry accepts (k = 1..26, both set forms, no table and tables of 10..18 bits,
// the values of option ipa_fold, with and without a window override), the counts tests/test_gpu_realsize.py asserts through trh_stat and the byte
// size of every scratch buffer at k = 10, 14 and 18 as literals.
// Plain C++, run by tests/test_hostcombine.py.
#include <cstdio>
#include <utility>

#include "../../tiny-ram-halo2_amd/csrc/foldplan.h"
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

    // transforms per launch set of the lazy passes (log_n >= 12): the rule ntt_device_t runs by and ntt_prepare sizes the scratch by
    {
        const size_t cap = (size_t)2 << 30;
        const size_t block_counts[] = {0, 1, 3, 5, 8};
        for (int log_n = 12; log_n <= 27; ++log_n) for (size_t blocks : block_counts) {
            const size_t fit = cap / ((size_t)72 << log_n), unit = blocks ? blocks : 1;
            // batches (whole polynomials) below, at and above what fits, and far above
            const size_t polys[] = {1, 2, 7, fit / unit, fit / unit + 1, 2 * (fit / unit) + 3, 100000};
            for (size_t p : polys) {
                if (p == 0) continue;
                const size_t batch = p * unit, chunk = ntt_lazy_chunk(log_n, blocks, batch);
                expect(chunk >= 1 && chunk <= batch, "1 <= chunk <= batch", log_n, chunk);
                if (blocks) expect(chunk % blocks == 0, "whole polynomials per launch set", log_n, chunk);
                const bool raised = fit < unit;  // (from 2^25 not even one transform's two planes fit: it runs alone)
                if (raised) expect(chunk == unit, "fewer than one polynomial fits: one polynomial", log_n, chunk);
                else expect(2 * chunk * ((size_t)36 << log_n) <= cap, "both raw planes within 2 GiB", log_n, chunk);
                // nothing larger would do: the next whole polynomial is beyond the batch or beyond the scratch
                if (!raised && chunk + unit <= batch) expect(2 * (chunk + unit) * ((size_t)36 << log_n) > cap, "the largest set that fits", log_n, chunk);
            }
        }
        const size_t big = 1000000 * 120;  // a multiple of 3, 5 and 8
        expect(ntt_lazy_chunk(12, 0, big) == 7281, "2^12: 7281", 12, ntt_lazy_chunk(12, 0, big));
        expect(ntt_lazy_chunk(18, 0, big) == 113, "2^18: 113", 18, ntt_lazy_chunk(18, 0, big));
        expect(ntt_lazy_chunk(21, 0, big) == 14, "2^21: 14", 21, ntt_lazy_chunk(21, 0, big));
        expect(ntt_lazy_chunk(22, 0, big) == 7, "2^22: 7", 22, ntt_lazy_chunk(22, 0, big));
        expect(ntt_lazy_chunk(18, 5, big) == 110, "2^18, 5 blocks: 110", 18, ntt_lazy_chunk(18, 5, big));
        expect(ntt_lazy_chunk(18, 8, big) == 112, "2^18, 8 blocks: 112", 18, ntt_lazy_chunk(18, 8, big));
        expect(ntt_lazy_chunk(18, 3, big) == 111, "2^18, 3 blocks: 111", 18, ntt_lazy_chunk(18, 3, big));
        expect(ntt_lazy_chunk(12, 5, big) == 7280, "2^12, 5 blocks: 7280", 12, ntt_lazy_chunk(12, 5, big));
        expect(ntt_lazy_chunk(22, 8, big) == 8, "2^22, 8 blocks: 7 raised to 8", 22, ntt_lazy_chunk(22, 8, big));
        expect(ntt_lazy_chunk(22, 8, 24) == 8 && ntt_lazy_chunk(18, 5, 160) == 110 && ntt_lazy_chunk(18, 5, 105) == 105, "capped at the batch", 18, ntt_lazy_chunk(18, 5, 105));
    }

    // MSM launch plan: invariants over the sweep
    {
        std::vector<size_t> ns = {1, 2, 255, 256, 8448, 8449};
        for (int k = 9; k <= 31; ++k) { ns.push_back(((size_t)1 << k) - 1); ns.push_back((size_t)1 << k); ns.push_back(((size_t)1 << k) + 1); }
        const size_t batches[] = {1, 2, 4, 5, 7, 8, 64, 65, 200};
        const int tables[] = {0, 4, 14, 15, 18}, overrides[] = {0, 2, 13, 18};
        const unsigned gbs[] = {1, 4};
        for (size_t n : ns) for (size_t batch : batches) for (int fc : tables) for (int ov : overrides) for (unsigned gb : gbs) {
            if (fc && !msm_fixed_base_fits(n, fc)) continue;
            const MsmPlan p = msm_plan(MsmShape{n, batch, fc, ov, gb});
            expect(p.k1 + p.k2 == p.c - 1, "k1 + k2 == c - 1", n, batch);
            expect(p.idx_bits + p.k2 <= 31, "index and low bucket bits fit the entry", n, batch);
            expect(p.nbins <= 2048 && p.nbins == 1u << p.k1, "at most 2048 level-1 bins (LDS of the partition)", n, p.nbins);
            expect((size_t)p.slice * p.tpw == p.nbk, "slice * tpw == nbk", n, batch);
            expect(p.chunk >= 1 && p.chunk <= 64, "1 <= chunk <= 64", n, p.chunk);
            expect(p.tpw <= 256 || (size_t)p.Ws * p.tpw * p.chunk <= ((size_t)1 << 16) || p.tpw == p.nbk, "reduction within 2^16 threads", n, p.tpw);
            expect(p.seg_len0 == 16 || p.seg_len0 == 32 || p.seg_len0 == 64 || p.seg_len0 == 128, "segment length", n, p.seg_len0);
            expect((size_t)p.nseg0 * p.seg_len0 >= p.ns, "the segments cover the slots", n, p.nseg0);
            if (p.use_bin_shape) expect(p.bin_cap % 1024 == 0 && p.bin_cap <= BIN_CAP_MAX && p.avg_bin >= 4096, "LDS bin sort: capacity and bin size", n, p.bin_cap);
            // counts: [bin counts][tile flags][oversize flags][entry totals], 16 bytes of slack
            expect(p.tile_flags_off() == p.bins_bytes(p.chunk) && p.oversize_off() == p.tile_flags_off() + p.flag_bytes && p.totals_off() == p.oversize_off() + p.chunk * p.Ws * 4 &&
                   p.counts_bytes() == p.totals_off() + p.chunk * p.Ws * 4 + 16, "counts: four disjoint regions, then 16 bytes", n, batch);
            expect(p.tile_flags_off() % 4 == 0 && p.oversize_off() % 4 == 0 && p.totals_off() % 4 == 0, "counts: regions 4-byte aligned", n, batch);
            expect((fc != 0) == (p.flag_bytes != 0) && p.flag_bytes >= (fc ? p.chunk * p.part_tiles : 0), "tile flags: one byte per (item, partition tile) of a tabled set", n, p.flag_bytes);
            expect((p.recode_use_lds != 0) == ((size_t)p.Ws * p.nbins * 4 <= 65536), "recode histogram in LDS up to 64 KiB", n, p.recode_lds);
        }
    }
    // routes at their edges (no table, no override)
    {
        const size_t T = (size_t)1 << 25;
        auto route = [](size_t n, size_t batch, int ov, bool in_tile, size_t* tiles, size_t* len) { return msm_route(MsmShape{n, batch, 0, ov, 4}, in_tile, false, tiles, len); };
        size_t tiles = 0, len = 0;
        expect(route(8448, 4, 0, false, &tiles, &len) == MSM_ROUTE_SMALL, "(8448, 4) is one launch", 8448, 4);
        expect(route(8449, 4, 0, false, &tiles, &len) == MSM_ROUTE_PIPELINE, "(8449, 4) is the pipeline", 8449, 4);
        expect(route(8448, 5, 0, false, &tiles, &len) == MSM_ROUTE_PIPELINE, "(8448, 5) is the pipeline", 8448, 5);
        expect(route(T, 1, 0, false, &tiles, &len) == MSM_ROUTE_PIPELINE, "(2^25, 1) is the pipeline", T, 1);
        expect(route(T + 1, 1, 0, false, &tiles, &len) == MSM_ROUTE_TILED && tiles == 2 && len == T / 2 + 1, "(2^25 + 1, 1): 2 tiles of 2^24 + 1", tiles, len);
        // the count tests/test_gpu_realsize.py expects from trh_stat "msm_range_tiles"
        expect(route(T + 3, 1, 0, false, &tiles, &len) == MSM_ROUTE_TILED && tiles == 2, "(2^25 + 3, 1): 2 tiles", tiles, len);
        expect(route(T + 1, 2, 0, false, &tiles, &len) == MSM_ROUTE_PIPELINE, "(2^25 + 1, 2) is the pipeline", T + 1, 2);
        expect(route(T + 1, 1, 16, false, &tiles, &len) == MSM_ROUTE_PIPELINE, "(2^25 + 1, 1) with a window override is the pipeline", T + 1, 16);
        expect(route(T + 1, 1, 0, true, &tiles, &len) == MSM_ROUTE_PIPELINE, "(2^25 + 1, 1) in a tile is the pipeline", T + 1, 1);
    }
    // named shapes.  The 256 bins and BIN_CAP = 5120 that tests/test_gpu_msm_sort.py hard-codes are the (2^20, 1) row.
    {
        const struct { size_t n, batch; int fc, c, W, Ws, k2; unsigned nbins; size_t chunk; unsigned tpw, slice, seg_len0, nseg0, bin_cap; bool use_bin; } rows[] = {
            {8449u, 1, 0, 8, 32, 32, 7, 1, 1, 128, 1, 16, 529, 10240, true},
            {65536u, 64, 0, 10, 26, 26, 7, 4, 64, 256, 2, 128, 512, 18432, true},
            {262144u, 1, 0, 15, 18, 18, 7, 128, 1, 2048, 8, 16, 16384, 3072, false},
            {1048576u, 1, 0, 16, 16, 16, 7, 256, 1, 4096, 8, 64, 16384, 5120, true},
            {1048576u, 4, 0, 16, 16, 16, 7, 256, 4, 1024, 32, 128, 8192, 5120, true},
            {16777216u, 1, 0, 17, 16, 16, 7, 512, 1, 4096, 16, 128, 131072, 35840, true},
            {33554432u, 1, 0, 17, 16, 16, 6, 1024, 1, 4096, 16, 128, 262144, 35840, true},
            {268435456u, 1, 0, 15, 18, 18, 3, 2048, 1, 2048, 8, 128, 2097152, 0 /* beyond BIN_CAP_MAX */, false},
            {2147483648u, 1, 0, 12, 22, 22, 0, 2048, 1, 2048, 1, 128, 16777216, 0 /* beyond BIN_CAP_MAX */, false},
            {4194304u, 200, 0, 16, 16, 16, 7, 256, 5, 512, 64, 128, 32768, 18432, true},
            {65538u, 2, 14, 14, 19, 1, 7, 64, 2, 8192, 1, 16, 77827, 21504, true},
            {262146u, 2, 15, 15, 18, 1, 7, 128, 2, 16384, 1, 32, 147458, 39936, false},
            {262145u, 100, 15, 15, 18, 1, 7, 128, 64, 1024, 16, 128, 36865, 39936, false},
        };
        for (const auto& r : rows) {
            const MsmPlan p = msm_plan(MsmShape{r.n, r.batch, r.fc, 0, 4});
            expect(p.c == r.c && p.W == r.W && p.Ws == r.Ws && p.k2 == r.k2 && p.nbins == r.nbins, "named shape: window bits, windows, bucket sets, k2, bins", r.n, r.batch);
            expect(p.chunk == r.chunk && p.tpw == r.tpw && p.slice == r.slice, "named shape: chunk, reduce geometry", r.n, r.batch);
            expect(p.seg_len0 == r.seg_len0 && p.nseg0 == r.nseg0, "named shape: segments", r.n, r.batch);
            expect(r.bin_cap ? p.bin_cap == r.bin_cap : p.bin_cap > BIN_CAP_MAX, "named shape: bin capacity", r.n, p.bin_cap);
            expect(p.use_bin_shape == r.use_bin, "named shape: LDS bin sort", r.n, r.batch);
        }
    }
    // chunk shapes: the batches tests/test_gpu_msm_chunks.py runs past one launch set.  chunk = min(batch, 64, floor((chunk_gb << 30) / per_item))
    // with per_item = W * n * 12 + 1; the GPU tests assert ceil(batch / chunk) through trh_stat "msm_chunks" and build their items on the
    // window width, the adaptive flag and (the read-back of size_segments, msm.hip) on whether nb * Ws * 4 fits the 4 KiB landing area.
    {
        const struct { size_t n, batch; int fc; unsigned gb; int c, W, Ws; size_t chunk, chunks; bool adaptive, use_bin, sparse_ok; } rows[] = {
            // 32 windows of 8 bits, per_item = 32 * 1500 * 12 + 1 = 576001: the budget allows 7456 items, the cap of 64 cuts
            {1500, 65, 0, 4, 8, 32, 32, 64, 2, true, false, false},
            {1500, 96, 0, 4, 8, 32, 32, 64, 2, true, false, false},
            {1500, 97, 0, 4, 8, 32, 32, 64, 2, true, false, false},
            {1500, 129, 0, 4, 8, 32, 32, 64, 3, true, false, false},
            // 64 windows of 4 bits; 256 is the last batch whose Horners msm_finish_t splits with the helper thread, 257 the first beyond
            {300, 256, 0, 4, 4, 64, 64, 64, 4, true, false, false},
            {300, 257, 0, 4, 4, 64, 64, 64, 5, true, false, false},
            // one GiB: per_item = 18 * 2^18 * 12 + 1 = 56623105, floor(2^30 / 56623105) = 18 -> 18 + 2; four GiB hold all 20
            {(size_t)1 << 18, 20, 0, 1, 15, 18, 18, 18, 2, true, false, false},
            {(size_t)1 << 18, 20, 0, 4, 15, 18, 18, 20, 1, true, false, false},
            // per_item = 16 * 2^20 * 12 + 1 = 201326593, floor(2^30 / 201326593) = 5 -> 5 + 1, not adaptive (fused zeroing), LDS bin sort
            {(size_t)1 << 20, 6, 0, 1, 16, 16, 16, 5, 2, false, true, false},
            {(size_t)1 << 20, 6, 0, 4, 16, 16, 16, 6, 1, false, true, false},
            // the table trh_bases_precompute(0) attaches to 2^14 + 1 bases has 12-bit windows (bases.hip: floor(log2 n) - 2, a COPY of that rule: the
            // GPU test asserts the width the entry returns): one bucket set, the sampler is asked
            {((size_t)1 << 14) + 1, 70, 12, 4, 12, 22, 1, 64, 2, true, true, true},
        };
        for (const auto& r : rows) {
            const MsmShape sh{r.n, r.batch, r.fc, 0, r.gb};
            const MsmPlan p = msm_plan(sh);
            expect(msm_route(sh, false, false) == MSM_ROUTE_PIPELINE, "chunk shape: the pipeline", r.n, r.batch);
            expect(p.c == r.c && p.W == r.W && p.Ws == r.Ws, "chunk shape: window bits, windows, bucket sets", r.n, r.batch);
            const size_t per_item = (size_t)p.W * r.n * 12 + 1, cap = ((size_t)r.gb << 30) / per_item;
            expect(p.chunk == r.chunk && p.chunk == (r.batch < 64 ? (r.batch < cap ? r.batch : cap) : (cap < 64 ? cap : 64)), "chunk shape: items per launch set", r.n, p.chunk);
            expect((r.batch + p.chunk - 1) / p.chunk == r.chunks, "chunk shape: launch sets", r.n, r.batch);
            expect(p.adaptive == r.adaptive && p.use_bin_shape == r.use_bin && p.sparse_shape_ok == r.sparse_ok, "chunk shape: adaptive, LDS bin sort, sampler", r.n, r.batch);
            expect(!r.fc || msm_fixed_base_fits(r.n, r.fc), "chunk shape: the table fits", r.n, r.fc);
        }
        // the 4 KiB landing area of the adaptive read-back at c = 8 (Ws = 32): a chunk of 32 fills it to its last byte, 33 is one item over, 64 twice over
        const MsmPlan p8 = msm_plan(MsmShape{1500, 97, 0, 0, 4});
        expect((size_t)32 * p8.Ws * 4 == 4096 && (size_t)33 * p8.Ws * 4 > 4096 && (size_t)64 * p8.Ws * 4 == 8192, "chunk shape: 32 items x 32 windows x 4 B == 4096", p8.Ws, 0);
        // all scalars of an item equal: one bucket of 1500 entries per window, ceil(1500 / 16) = 94 segments -- beyond HEAVY_PIECES; at 300 pairs no bucket can be
        expect(p8.seg_len0 == 16 && p8.nseg0 == 94 && p8.nseg0 - 1 > HEAVY_PIECES, "chunk shape: a 1500-entry bucket is heavy", p8.nseg0, HEAVY_PIECES);
        expect(msm_plan(MsmShape{300, 256, 0, 0, 4}).nseg0 == 19, "chunk shape: 300 pairs are 19 segments", 300, 0);
        // what a lone item and a last chunk of up to four items run as when they are sent on their own
        expect(msm_route(MsmShape{1500, 1, 0, 0, 4}, false, false) == MSM_ROUTE_SMALL && msm_route(MsmShape{1500, 32, 0, 0, 4}, false, false) == MSM_ROUTE_PIPELINE &&
               msm_route(MsmShape{300, 64, 0, 0, 4}, false, false) == MSM_ROUTE_PIPELINE, "chunk shape: a lone item is one launch, a last chunk alone the pipeline", 1500, 1);
    }
    // collision shapes: the plan numbers tests/msm_collision_cases.py (SHAPES) builds the cases of tests/test_gpu_msm_collisions.py on -- which
    // segment offset a bucket starts at, how many pieces the combine adds with how many lanes, which buckets share a reduce slice, which
    // slices meet in a workgroup's tree.  A plan change that fails here means those cases no longer aim where their names say.
    {
        const struct { size_t n_lo, n_hi, batch; int fc, ov, c; unsigned seg_len0, nbk, tpw, slice, rblocks, lanes; } rows[] = {
            {64, 2400, 1, 0, 8, 8, 16, 128, 128, 1, 1, 1},              // "c8": one lane per bucket (fewer than three pieces)
            {64, 2400, 2, 0, 8, 8, 16, 128, 128, 1, 1, 1},
            {1024, 2048, 1, 0, 3, 3, 16, 4, 4, 1, 1, 4},                // "c3": 16 / 32 pieces per bucket, four lanes
            {512, 512, 1, 0, 15, 15, 16, 16384, 2048, 8, 8, 1},         // "c15": slices of 8, running sums
            {512, 512, 1, 0, 17, 17, 16, 65536, 4096, 16, 16, 1},       // "c17", "c18": slices of 16 and 32, the live-bucket branch
            {512, 512, 1, 0, 18, 18, 16, 131072, 4096, 32, 16, 1},
            {512, 512, 1, 16, 0, 16, 16, 32768, 16384, 2, 64, 1},       // "table16": one bucket set, slices of 2
            {512, 6143, 8, 0, 0, 8, 16, 128, 128, 1, 1, 1},             // eight items: the plan's own c = 8, adaptive segments
            {16386, 16386, 1, 12, 0, 12, 16, 2048, 2048, 1, 8, 4},      // "ipa14" (tests/ipa_collision_cases.py): the opening's commitment to s' at k = 14 ...
            {16386, 16386, 2, 12, 0, 12, 16, 2048, 2048, 1, 8, 4},      // ... and its rounds 0 and 1: one set of 2048 buckets, slices of one bucket
        };
        for (const auto& r : rows) for (size_t n : {r.n_lo, (r.n_lo + r.n_hi) / 2, r.n_hi}) {
            const MsmShape sh{n, r.batch, r.fc, r.ov, 4};
            const MsmPlan p = msm_plan(sh);
            expect(msm_route(sh, false, false) == MSM_ROUTE_PIPELINE, "collision shape: the pipeline", n, r.c);
            expect(p.c == r.c && p.Ws == (r.fc ? 1 : num_windows(r.c)) && p.nbk == r.nbk, "collision shape: window bits, bucket sets, buckets", n, r.c);
            expect(p.seg_len0 == r.seg_len0, "collision shape: segments of 16 entries", n, p.seg_len0);
            expect(p.tpw == r.tpw && p.slice == r.slice && p.rblocks == r.rblocks, "collision shape: reduce geometry", n, p.slice);
            // The next two rules are COPIES: the lanes per bucket are decided in stage_accumulate and the quad / thread form of the reduction in
            // stage_reduce (msm.hip), not by a function of hostplan.h.  What is asserted here is that the plan numbers those rules read give the
            // form the cases are built for; a change of the rules themselves in msm.hip must be carried over to these lines by hand.
            const size_t pieces = p.ns / ((size_t)p.nbk * p.seg_len0);  // stage_accumulate: four lanes per bucket from three expected pieces
            expect((pieces >= 3 && p.nbk >= 4 ? 4u : 1u) == r.lanes, "collision shape: lanes per bucket of the combine", n, pieces);
            expect(p.adaptive == (r.batch >= 8), "collision shape: adaptive segments for eight items", n, r.batch);
            if (p.adaptive) expect(msm_segments_counted(p, n, (uint32_t)n).seg_len == 16, "collision shape: counted segments of 16", n, r.batch);
            if (r.fc) {  // the quad reduction takes this shape: 16384 quads of 2 buckets, 256 workgroups of 64 quads
                expect((size_t)p.tpw * 4 * p.Ws <= ((size_t)1 << 16) && p.nbk % p.tpw == 0 && p.tpw >= 64, "collision shape: the table shape passes the quad gate at tpw", n, p.tpw);
            } else expect(p.Ws > 8, "collision shape: more than 8 bucket sets keep the thread-per-slice reduction", n, p.Ws);
        }
        // "ipa14", what the dense route of the opening decides from the plan (COPIES of stage_accumulate's and enqueue_pipeline's rules, as above): the
        // quad combine needs three expected pieces per bucket and at most 8 bucket sets in the launch, the lean sort the LDS bin sort
        for (size_t batch : {(size_t)1, (size_t)2}) {
            const MsmPlan p = msm_plan(MsmShape{16386, batch, 12, 0, 4});
            expect(p.W == 22 && p.ns == (size_t)22 * 16386 && p.chunk == batch, "ipa14: 22 table levels in one list, one launch set", batch, p.W);
            expect(p.ns / ((size_t)p.nbk * p.seg_len0) == 11 && p.ns / ((size_t)p.nbk * p.seg_len0) >= 3, "ipa14: eleven expected pieces per bucket", batch, p.ns);
            expect((size_t)p.Ws * batch <= 8, "ipa14: at most 8 bucket sets per launch (the quad combine, the quad reduction)", batch, p.Ws);
            expect(p.use_bin_shape && p.bin_cap == 24576 && p.nbins == 16 && p.k2 == 7, "ipa14: the LDS bin sort, 16 bins of 128 buckets, 24576 entries each at most", batch, p.bin_cap);
            expect((size_t)p.tpw * 4 * p.Ws * batch <= ((size_t)1 << 16) && p.nbk % p.tpw == 0, "ipa14: the quad reduction, one bucket per quad", batch, p.tpw);
            expect(1100 / p.seg_len0 > HEAVY_PIECES && !p.adaptive, "ipa14: a bucket of 1100 entries spans more than HEAVY_PIECES segments of the plan's own length", batch, p.seg_len0);
        }
        {   // the openings of tests/test_gpu_ipa_collisions.py: small (level 0 of the table) up to k = 13, the table pipeline with one collapse to 2^12 at k = 14
            const IpaPlan small = ipa_plan(IpaShape{13, ((size_t)1 << 13) + 2, true, 11, 24, 0, 1, SMALL_MAX_N});
            const IpaPlan p14 = ipa_plan(IpaShape{14, ((size_t)1 << 14) + 2, true, 12, 22, 0, 1, SMALL_MAX_N});
            expect(small.first_msm == IPA_MSM_SMALL_Z && small.fold_at == 0, "k = 13 with a table: msm_small_kernel over level 0", 13, small.fold_at);
            expect(p14.first_msm == IPA_MSM_TABLE && p14.fold_at == 2 && p14.m == 4096 && p14.round(1).table && !p14.round(2).table && p14.round(2).canon == 1,
                   "k = 14 with a table: rounds 0 and 1 over the table, then 12 small rounds over 2^12 + 2 points", 14, p14.fold_at);
        }
        // 2048 entries in one bucket at c = 3: 128 segments, beyond HEAVY_PIECES
        expect(msm_plan(MsmShape{2048, 1, 0, 3, 4}).nseg0 == 128 && 128 - 1 > HEAVY_PIECES, "collision shape: a 2048-entry bucket is heavy", 2048, HEAVY_PIECES);
        // the small kernel's cases
        expect(msm_route(MsmShape{2, 1, 0, 0, 4}, false, false) == MSM_ROUTE_SMALL && msm_route(MsmShape{400, 2, 0, 0, 4}, false, false) == MSM_ROUTE_SMALL && SMALL_C == 5,
               "collision shape: one launch, c = 5", 400, SMALL_C);
        // tests/test_gpu_parity.py test_msm_all_same_base_skewed and its twin under the override
        expect(msm_route(MsmShape{5000, 1, 0, 0, 4}, false, false) == MSM_ROUTE_SMALL && msm_route(MsmShape{5000, 1, 0, 8, 4}, false, false) == MSM_ROUTE_PIPELINE,
               "5000 pairs: one launch; the pipeline under a window override", 5000, 8);
    }
    // The plan of an IPA opening (ipa_plan): invariants over every shape the entry accepts
    {
        const int folds[] = {0, 1, 2, 4, 7, 8, 10}, overrides[] = {0, 12};
        for (uint32_t k = 1; k <= 26; ++k) for (int with_u = 0; with_u < 2; ++with_u) for (int c = 9; c <= 18; ++c) for (int fold : folds) for (int ov : overrides) {
            const bool table = c >= 10;  // c = 9 stands for "no table"
            const size_t n = (size_t)1 << k;
            const int W = table ? num_windows(c) : 0;
            const IpaPlan p = ipa_plan(IpaShape{k, n + 1 + with_u, table, table ? c : 0, W, ov, fold, SMALL_MAX_N});
            const unsigned long long id = (unsigned long long)k * 1000 + with_u * 100 + c, id2 = (unsigned long long)fold * 100 + ov;
            expect(p.k == k && p.n == n && p.with_u == (with_u != 0), "ipa: the shape", id, id2);
            // the first MSM
            const bool tabled = with_u && table, small = n + 2 <= SMALL_MAX_N && ov == 0;
            expect(p.first_msm == (!tabled ? IPA_MSM_PLAIN : small ? IPA_MSM_SMALL_Z : IPA_MSM_TABLE), "ipa: form of the first MSM", id, id2);
            expect(p.first_pairs == (tabled ? n + 2 : n + 1), "ipa: pairs of the first MSM", id, id2);
            if (with_u && n + 2 <= SMALL_MAX_N && ov == 0) expect(p.first_msm != IPA_MSM_TABLE && p.fold_at == 0, "ipa: a set within the small kernel never uses its table and never collapses", id, id2);
            if (p.first_msm == IPA_MSM_SMALL_Z) expect(msm_route(MsmShape{p.first_pairs, 1, 0, ov, 4}, false, false) == MSM_ROUTE_SMALL, "ipa: small_z is one launch", id, id2);
            expect(p.bytes.sp >= p.first_pairs * 32 && p.bytes.sp >= (n + 2) * 32, "ipa: s' holds the first MSM's scalars, blind and the scalar of u", id, id2);
            expect(p.bytes.b >= n * 32 && p.bytes.pp >= n * 32 && p.eval_blocks >= 1 && p.eval_blocks <= 512 && p.bytes.io >= (size_t)p.eval_blocks * 32, "ipa: the evaluation launches", id, id2);
            // the collapse
            if (p.fold_at) {
                const uint32_t r = p.fold_at;
                expect(with_u && table && k >= 14 && ipa_fold_supported(true, c, W, k, r) && p.first_msm == IPA_MSM_TABLE, "ipa: a collapse needs g || w || u, a table, k >= 14 and a supported shape", id, id2);
                expect(r == (uint32_t)(fold == 1 ? k - 12 : fold) && r >= 2 && r <= 10 && r + 8 <= k, "ipa: the collapse round is the option's (1: k - 12)", id, r);
                expect(p.m == n >> r && p.m >= 256 && p.m % 256 == 0, "ipa: whole workgroups of collapsed generators", id, p.m);
                if (fold == 1) expect(p.m == 4096, "ipa: the library's choice collapses to 2^12 generators", id, p.m);
                expect(p.fold_w0 + p.fold_w1 == (uint32_t)c && p.fold_w0 >= p.fold_w1 && p.fold_w1 >= 5 && p.fold_w0 <= 9, "ipa: two sub-digits of 5 .. 9 bits per window", id, p.fold_w0);
                expect(p.fold_nbk == (1u << (p.fold_w0 - 1)) + (1u << (p.fold_w1 - 1)), "ipa: buckets of the collapse", id, p.fold_nbk);
                expect(p.bytes.fold_buckets == (size_t)(p.fold_nbk + 1) * p.m * 144, "ipa: buckets and the m sums behind them", id, p.bytes.fold_buckets);
                expect(p.fold_list_words == (size_t)p.fold_nbk + 1 + ((size_t)2 << r) * W, "ipa: offsets + two entries per scalar and window", id, p.fold_list_words);
                // the stand-alone collapse of the same shape sizes the same buffers and nothing else
                const IpaPlan q = ipa_collapse_plan(c, W, k, r);
                expect(q.fold_at == r && q.m == p.m && q.fold_nbk == p.fold_nbk && q.fold_w0 == p.fold_w0 && q.fold_w1 == p.fold_w1 && q.bytes.fold_buckets == p.bytes.fold_buckets &&
                       q.fold_list_words == p.fold_list_words, "ipa: the collapse alone plans as the opening's", id, id2);
                expect(q.bytes.b + q.bytes.sp + q.bytes.pp + q.bytes.wgt + q.bytes.lrsc + q.bytes.gwu + q.bytes.gwuz + q.bytes.pp2 + q.bytes.b2 + q.bytes.io == 0, "ipa: the collapse alone has no vectors", id, id2);
            } else {
                const uint32_t want = fold == 1 ? (k >= 14 ? k - 12 : 0) : (uint32_t)fold;
                expect(!(p.first_msm == IPA_MSM_TABLE && k >= 14 && ipa_fold_supported(true, c, W, k, want)), "ipa: a supported collapse is taken", id, id2);
                expect(p.bytes.fold_buckets == 0 && p.fold_list_words == 0, "ipa: no collapse, no buffers for one", id, id2);
            }
            // the rounds' window override: k - 8 for k = 16..18 unless the MSMs run over the table
            expect(p.round_window == ((p.first_msm != IPA_MSM_TABLE && k >= 16 && k <= 18) ? (int)k - 8 : 0), "ipa: window override of the rounds", id, p.round_window);
            const int live_ov = ov ? ov : p.round_window;  // what msm_enqueue finds in the context during the rounds (WindowGuard)
            // own copy of the round bases: the whole set with u appended, or the collapsed generators
            expect(p.bytes.gwu == (!with_u ? (n + 2) * 64 : p.fold_at ? (p.m + 2) * 64 : 0) && p.bytes.gwuz == 2 * p.bytes.gwu, "ipa: the opening's own round bases", id, p.bytes.gwu);
            size_t small_msms = p.first_msm == IPA_MSM_SMALL_Z ? 1 : 0;
            for (uint32_t j = 0; j < k; ++j) {
                const IpaRound g = p.round(j);
                const bool folded = p.fold_at && j >= p.fold_at;
                expect(g.gens == (folded ? p.m : n) && g.stride == g.gens + 2, "ipa round: generators and stride", id, j);
                expect(g.bit == k - j - 1 && g.half == (size_t)1 << g.bit && 2 * g.half <= g.gens, "ipa round: half", id, j);
                expect(g.table == (p.first_msm == IPA_MSM_TABLE && !folded), "ipa round: over the table until the collapse", id, j);
                if (folded) expect(g.gens + 2 == p.m + 2 && g.canon == (ov == 0 && p.m + 2 <= SMALL_MAX_N ? 1 : 0), "ipa round: m + 2 pairs behind a collapse, the small kernel's where they fit", id, j);
                if (folded && fold == 1 && ov == 0) expect(g.canon == 1, "ipa round: canonical rows behind the library's collapse", id, j);
                // canon says which kernel takes the MSM: it must be msm_enqueue's own route for the call
                expect((g.canon != 0) == (msm_route(MsmShape{g.gens + 2, 2, g.table ? c : 0, live_ov, 4}, false, false) == MSM_ROUTE_SMALL), "ipa round: canon is the MSM's route", id, j);
                small_msms += g.canon ? 1 : 0;
                expect(g.first == (j == 0) && g.wfresh == (j <= 1 || (p.fold_at && (j == p.fold_at || j == p.fold_at + 1)) ? 1 : 0), "ipa round: flags of the front launch", id, j);
                expect(g.front_blocks == (g.gens + 255) / 256 && g.sum_blocks >= 1 && g.sum_blocks <= 512 && g.sum_blocks == ((g.half + 255) / 256 < 512 ? (g.half + 255) / 256 : 512),
                       "ipa round: workgroups", id, j);
                // every buffer holds the round's use of it
                expect(p.bytes.wgt >= g.gens * 32, "ipa round: weights", id, j);
                expect(p.bytes.lrsc >= (g.stride + g.gens + 2) * 32, "ipa round: two scalar rows with their tails", id, j);
                expect(p.bytes.io >= ((size_t)2 * g.sum_blocks) * 32, "ipa round: partial sums of both sides", id, j);
                // round j reads p' / b of 2^(k - j) entries (j >= 1: both halves of the previous round's, 2^(k - j + 1)) and writes the folds, 2^(k - j):
                // rounds 0 and 1 read the first buffers, then the pairs alternate -- odd rounds write the second buffers
                const size_t reads = j ? 4 * g.half : 2 * g.half, writes = j ? 2 * g.half : 0;
                const size_t read_buf = (j <= 1 || j % 2 == 1) ? p.bytes.pp : p.bytes.pp2, write_buf = j % 2 == 1 ? p.bytes.pp2 : p.bytes.pp;
                expect(read_buf >= reads * 32 && write_buf >= writes * 32 && p.bytes.b2 == p.bytes.pp2 && p.bytes.b == p.bytes.pp, "ipa round: the ping-pong pairs", id, j);
                if (folded || !with_u) expect(p.bytes.gwu >= (g.gens + 2) * 64 && p.bytes.gwuz >= (g.gens + 2) * 128, "ipa round: own bases", id, j);
            }
            // the counts tests/test_gpu_realsize.py::_ipa_case asserts through trh_stat "msm_small_launches" and "ipa_generator_collapses"
            // (for every table that can exist -- W (n + 2) <= 2^24, so k <= 20; from k = 23 the choice k - 12 is beyond the ten rounds a collapse takes)
            if (tabled && fold == 1 && ov == 0 && msm_fixed_base_fits(n + 2, c)) {
                expect(small_msms == (k <= 13 ? k + 1 : 12), "ipa: k + 1 small MSMs up to k = 13, the 12 rounds behind the collapse from 14", id, small_msms);
                expect((p.fold_at != 0) == (k >= 14), "ipa: one collapse from k = 14", id, p.fold_at);
            }
            if (ov == 0) expect((p.round_window != 0) == (!tabled && k >= 16 && k <= 18) && (!p.round_window || p.round_window == (int)k - 8), "ipa: k - 8 exactly for untabled k = 16..18", id, p.round_window);
        }
        // the bucket count is the one the bucket lists are built with (foldplan.h)
        for (int c = 10; c <= 18; ++c) {
            const IpaPlan q = ipa_collapse_plan(c, num_windows(c), 14, 2);
            std::vector<trh::hostcombine::H> one(4, trh::hostcombine::H{{1, 0, 0, 0}});
            std::vector<uint32_t> lists;
            uint32_t nbk = 0;
            expect(trh::foldplan::fold_plan(one, c, num_windows(c), q.fold_w0, q.fold_w1, lists, nbk) == trh::foldplan::FOLD_PLAN_OK && nbk == q.fold_nbk && lists.size() <= q.fold_list_words,
                   "ipa: the plan's buckets are the bucket lists'", c, nbk);
        }
        // an unsupported collapse alone keeps its (k, r) for the refusal and sizes nothing
        for (const auto& kr : {std::pair<uint32_t, uint32_t>{10, 1}, {10, 3}, {9, 2}, {10, 11}, {10, 200}}) {
            const IpaPlan q = ipa_collapse_plan(12, num_windows(12), kr.first, kr.second);
            expect(q.k == kr.first && q.fold_at == kr.second && q.bytes.fold_buckets == 0 && q.fold_list_words == 0, "ipa: an unsupported collapse sizes nothing", kr.first, kr.second);
        }
        expect(ipa_collapse_plan(9, num_windows(9), 10, 2).bytes.fold_buckets == 0, "ipa: a 9-bit table has no collapse", 9, 0);
        // the byte sizes, restated from the expressions of the opening before the plan existed (n = 2^k):
        //   b, p', weights n * 32; s' (n + 2) * 32; rows 2 * (n + 2) * 32; second halves n * 16 + 32; partial sums (2 * 512 + 2) * 32;
        //   own bases (points) * 64 and * 128; buckets (nbk + 1) * m * 144; lists nbk + 1 + (2 << r) * W words
        const struct { uint32_t k; int with_u, c, W; size_t b, sp, lrsc, pp2, gwu, gwuz, buckets, words; uint32_t fold_at; } rows[] = {
            {10, 1, 12, 22, 32768, 32832, 65664, 16416, 0, 0, 0, 0, 0},
            {10, 0, 0, 0, 32768, 32832, 65664, 16416, 65664, 131328, 0, 0, 0},
            {14, 1, 14, 19, 524288, 524352, 1048704, 262176, 262272, 524544, 76087296, 281, 2},
            {14, 0, 0, 0, 524288, 524352, 1048704, 262176, 1048704, 2097408, 0, 0, 0},
            {18, 1, 16, 16, 8388608, 8388672, 16777344, 4194336, 262272, 524544, 151584768, 2305, 6},
            {18, 1, 15, 18, 8388608, 8388672, 16777344, 4194336, 262272, 524544, 113836032, 2497, 6},
            {18, 0, 0, 0, 8388608, 8388672, 16777344, 4194336, 16777344, 33554688, 0, 0, 0},
        };
        for (const auto& r : rows) {
            const IpaPlan p = ipa_plan(IpaShape{r.k, ((size_t)1 << r.k) + 1 + r.with_u, r.c != 0, r.c, r.W, 0, 1, SMALL_MAX_N});
            expect(p.bytes.b == r.b && p.bytes.pp == r.b && p.bytes.wgt == r.b && p.bytes.sp == r.sp && p.bytes.lrsc == r.lrsc && p.bytes.pp2 == r.pp2 && p.bytes.b2 == r.pp2, "ipa sizes: the vectors", r.k, r.c);
            expect(p.bytes.io == 32832, "ipa sizes: partial sums", r.k, p.bytes.io);
            expect(p.bytes.gwu == r.gwu && p.bytes.gwuz == r.gwuz, "ipa sizes: own bases", r.k, p.bytes.gwu);
            expect(p.fold_at == r.fold_at && p.bytes.fold_buckets == r.buckets && p.fold_list_words == r.words, "ipa sizes: the collapse", r.k, p.bytes.fold_buckets);
        }
    }
    std::printf(bad ? "hostplan: FAILED (%d)\n" : "hostplan: ok\n", bad);
    return bad ? 1 : 0;
}
