// Host-side shape decisions of the two headline operations, free of HIP types so that a plain C++ test can check them
// (tests/native/hostplan_test.cpp): where msm_host_tiled (msmapi.hip) cuts an MSM with host scalars into ranges, how
// ntt.hip splits a transform into passes and a batch into launch sets, the launch plan of an MSM on the device (msm.hip: route, Pippenger geometry,
// scratch layout) as a pure function of its shape, and the plan of an IPA opening (ipa.hip, ipafold.hip: the form of its MSMs, the generator
// collapse, every round's geometry, the size of every scratch buffer) likewise.
#pragma once
#include <cstddef>
#include <cstdint>
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

constexpr size_t NTT_MAX_SCRATCH = (size_t)2 << 30;  // raw scratch of one call of the lazy passes at most
constexpr size_t NTT_RAW_BYTES = 36;                  // a raw nine-limb element; the passes alternate between two such planes per transform

// transforms per launch set of the lazy passes (ntt_device_t runs by it, ntt_prepare sizes the scratch by it): what fits 2 GiB of raw
// scratch at 72 B per element, at least one; with coset blocks (blocks != 0: the kernel takes the block as index % blocks inside a
// launch) whole polynomials only -- a multiple of `blocks`, and `blocks` where fewer would fit; never more than the batch
inline size_t ntt_lazy_chunk(int log_n, size_t blocks, size_t batch) {
    size_t chunk = NTT_MAX_SCRATCH / (((size_t)1 << log_n) * 2 * NTT_RAW_BYTES);
    if (chunk < 1) chunk = 1;
    if (blocks) chunk = chunk < blocks ? blocks : chunk - chunk % blocks;
    if (chunk > batch) chunk = batch;
    return chunk;
}

// ---------------------------------------------------------------------------------------
// The launch plan of one MSM on the device (msm.hip): which route msm_enqueue takes, the Pippenger geometry of the pipeline and the
// layout of its scratch, all integer functions of the shape.  No HIP types, no context, no options, no heap: it runs on every MSM.
// The constants are the ones the kernels of msm.hip are built with (each is described where its kernel is).
// ---------------------------------------------------------------------------------------
constexpr int MAX_C = 18;
constexpr int MAX_C_FIXED = 18;  // fixed-base tables: one bucket set per MSM, so wider windows pay
// Above 2^25 pairs the entry index squeezes the second sort level (31 bits = index + low bucket bits) and the rate drops
// (2^25: 815 M pairs/s, 2^26: 740, 2^27: 490, 2^28: 410): larger MSMs run as equal range tiles of at most 2^25 pairs, each
// at the full rate; the tiles' points are added on the host (the same sum the range-sharded multi-GPU path forms).
constexpr size_t MSM_TILE = (size_t)1 << 25;
constexpr int SMALL_C = 5;                  // msm_small_kernel
constexpr uint32_t SMALL_MAX_N = 8448;      // LDS: one byte + one u16 per scalar
constexpr int PART_TILE = 16384;            // msm_partition_kernel: digits per workgroup tile
constexpr int BIN_THREADS = 1024;           // msm_bin_sort_kernel
constexpr int BIN_PER_MAX = 36;                             // entries per thread, kept in registers from the load to the last pass
constexpr uint32_t BIN_CAP_MAX = BIN_THREADS * BIN_PER_MAX; // 36864 entries
constexpr int RANGE_BLOCK = 1024;           // msm_bucket_block_sums_kernel / msm_bucket_ranges_kernel
constexpr uint32_t HEAVY_PIECES = 64;       // msm_combine_heavy_kernel
constexpr int SP_LISTS = 16;              // compact lists per column (one counter each: a single counter per column would serialise its 1025 workgroups)
constexpr int SP_CNT = 2 * SP_LISTS;      // counters per column: the SP_LISTS digit lists, then the SP_LISTS unit lists
constexpr uint32_t SP_PAD = 32;           // u32 words between two list counters (one 128-byte line each)
constexpr int SP_PARTS = SP_LISTS + 1;    // partial sums per column: one per unit list, one for the digit entries of a tiny column
constexpr size_t SP_MAX_CHUNK = 256;      // items per launch set the pinned read-back area is sized for
constexpr size_t XYZZ_BYTES = 128;        // a window sum (XYZZMem)
constexpr size_t RAW_POINT_BYTES = 144;   // a raw lazy point of the accumulate -> combine -> reduce scratch (XYZZzMem)

inline int ilog2_floor(size_t n) {
    int l = 0;
    while ((n >> (l + 1)) != 0) ++l;
    return l;
}

inline int choose_window_bits(size_t n, int window_override) {
    const int o = window_override;
    if (o >= 2 && o <= MAX_C) return o;
    // measured on MI355X (tools/window_sweep.py): below 2^15 pairs an MSM is latency-bound and the width
    // hardly matters; from 2^16 the wide windows win (fewer mixed adds, more level-1 sort bins)
    const int l = ilog2_floor(n ? n : 1);
    // 2^24 / 2^25: c = 17 (15 full windows + an almost always empty carry window) beats 16 by 3 %; from 2^26 the index
    // takes 26 of the 31 entry bits, which leaves 5 low bucket bits for the second sort level, and 16 wins again
    return l < 9 ? 4 : l < 15 ? 8 : l == 15 ? 11 : l == 16 ? 10 : l == 17 ? 12 : l < 20 ? 15 : l < 24 ? 16 : l < 26 ? 17 : 16;
}
inline int num_windows(int c) { return 255 / c + 1; }
// the partitioned entries pack 7 low bucket bits above the flat table index
inline bool msm_fixed_base_fits(size_t n, int c) {
    if (c < 2 || c > MAX_C_FIXED) return false;
    return (size_t)num_windows(c) * n <= ((size_t)1 << 24);
}

struct MsmShape {
    size_t n, batch;       // pairs per item, items
    int fb_c;              // window bits of the fixed-base table the MSM runs over, 0: no table
    int window_override;   // the context's override, 0: none
    unsigned chunk_gb;     // option msm_chunk_gb
};

enum MsmRoute { MSM_ROUTE_TILED, MSM_ROUTE_SMALL, MSM_ROUTE_PIPELINE };
// TILED: range tiles of `len` pairs (the last one shorter), each through msm_route again with in_tile; SMALL: one launch (msm_small_kernel)
inline MsmRoute msm_route(const MsmShape& sh, bool in_tile, bool force_fallback, size_t* tiles = nullptr, size_t* len = nullptr) {
    if (!sh.fb_c && sh.batch == 1 && sh.n > MSM_TILE && !in_tile && sh.window_override == 0) {
        const size_t t = (sh.n + MSM_TILE - 1) / MSM_TILE;
        if (tiles) *tiles = t;
        if (len) *len = (sh.n + t - 1) / t;
        return MSM_ROUTE_TILED;
    }
    if (!sh.fb_c && sh.n != 0 && sh.n <= SMALL_MAX_N && sh.batch <= 4 && sh.window_override == 0 && !in_tile && !force_fallback) return MSM_ROUTE_SMALL;
    return MSM_ROUTE_PIPELINE;
}

// segments of the sorted lists (one thread of msm_accumulate_seg_kernel each) and the heavy-bucket list that goes with them
struct MsmSegments { uint32_t seg_len, nseg, heavy_stride; unsigned heavy_blocks; };
// a heavy bucket spans > HEAVY_PIECES segments, so there are fewer than W * nseg / HEAVY_PIECES of them
inline size_t msm_max_heavy(int Ws, uint32_t nseg) { return (size_t)Ws * nseg / HEAVY_PIECES + 1; }
inline MsmSegments msm_segments(int Ws, uint32_t seg_len, uint32_t nseg) {
    const size_t mh = msm_max_heavy(Ws, nseg);
    return MsmSegments{seg_len, nseg, (uint32_t)(mh + 1), (unsigned)(mh < 256 ? mh : 256)};
}

struct MsmPlan {
    size_t n, batch;
    bool fb;                 // fixed-base mode (a table): one bucket set per item
    int c, W, Ws;            // window bits, windows of the recoding, bucket sets per item
    size_t ns;               // slots per item and bucket set
    uint32_t nbk, nb1;       // buckets per set, + 1
    int idx_bits, k1, k2;    // sort geometry (see msm_plan)
    uint32_t nbins;
    size_t recode_lds; int recode_use_lds;
    size_t chunk;            // items per launch set
    uint32_t tpw, slice, rblocks;  // reduce geometry: threads per window, buckets per thread, workgroups
    uint32_t seg_len0, nseg0;  // the segments every launch starts from (run_chunk resizes them for dense and counted chunks)
    size_t max_heavy; uint32_t heavy_stride0; unsigned heavy_blocks0;
    uint32_t part_tiles; size_t flag_bytes;
    unsigned range_blocks;
    size_t avg_bin; uint32_t bin_cap;
    bool use_bin_shape;      // the shape half of "LDS bin sort" (option bin_sort is the other)
    bool adaptive;
    uint32_t sp_subcap, sp_cap;
    bool sparse_shape_ok;    // the shape half of "ask the sparse sampler" (option, table and the call's flags are the other)

    MsmSegments seg0() const { return MsmSegments{seg_len0, nseg0, heavy_stride0, heavy_blocks0}; }
    // ---- scratch layout: every size msm.hip reserves, zeroes or offsets by, once
    size_t entries_bytes() const { return chunk * W * n * 4 + 16; }                     // digits, parted, sorted
    // counts: [bin counts][fixed-base mode: one byte per (item, partition tile)][oversize-bin flags of the LDS bin sort][entry totals per item and window]
    size_t bins_bytes(size_t items) const { return items * Ws * nbins * 4; }            // (also bin_starts, for `chunk` items)
    size_t tile_flags_off() const { return bins_bytes(chunk); }
    size_t oversize_off() const { return tile_flags_off() + flag_bytes; }
    size_t set_words_bytes() const { return chunk * Ws * 4; }                           // one u32 per (item, bucket set)
    size_t totals_off() const { return oversize_off() + set_words_bytes(); }
    size_t counts_used() const { return totals_off() + set_words_bytes(); }
    size_t counts_bytes() const { return counts_used() + 16; }
    size_t ranges_bytes(size_t items) const { return items * Ws * nb1 * 4; }            // starts, ends, bucket_cnt (+ 16)
    size_t seg_bucket_bytes() const { return chunk * Ws * range_blocks * 4 + 16; }      // block totals of the chunked passes' range scan
    size_t pieces_bytes(uint32_t nseg) const { return chunk * Ws * nseg * RAW_POINT_BYTES; }  // first, last
    size_t direct_bytes() const { return chunk * Ws * nb1 * RAW_POINT_BYTES; }
    size_t heavy_bytes(size_t items, uint32_t heavy_stride) const { return items * heavy_stride * 4; }
    size_t buckets_bytes() const { return chunk * Ws * nbk * RAW_POINT_BYTES; }
    size_t partials_bytes(uint32_t blocks) const { return chunk * Ws * blocks * RAW_POINT_BYTES; }
    // sparse: [counters: chunk x SP_CNT lines][partial sums: chunk x SP_PARTS raw points]
    size_t sparse_counter_words() const { return chunk * SP_CNT * SP_PAD; }
    size_t sparse_bytes() const { return sparse_counter_words() * 4 + chunk * SP_PARTS * RAW_POINT_BYTES + 64; }
    // window sums: batch x Ws XYZZ, then (lean sort) one overflow flag per (item, bucket set)
    size_t sum_flags_off() const { return batch * Ws * XYZZ_BYTES; }
    size_t sums_bytes(bool lean_sort) const { return sum_flags_off() + (lean_sort ? batch * Ws * 4 : 0); }
};

inline MsmPlan msm_plan(const MsmShape& sh) {
    MsmPlan p{};
    const size_t n = sh.n, batch = sh.batch;
    p.n = n; p.batch = batch; p.fb = sh.fb_c != 0;
    int cb = p.fb ? sh.fb_c : choose_window_bits(n, sh.window_override);
    if (!p.fb) {
        // beyond 2^27 pairs the index leaves fewer than 4 entry bits for the second sort level; the first level has at most
        // 2^11 bins (LDS of the partition), so the window narrows with n (15 bits up to 2^28 pairs ... 12 up to 2^31)
        int ib = 1;
        while (((size_t)1 << ib) < n) ++ib;
        const int k2max = 31 - ib < 7 ? 31 - ib : 7;
        if (cb - 1 - k2max > 11) cb = 12 + k2max;
    }
    p.c = cb;
    const int W = p.W = num_windows(cb);  // windows of the recoding
    // fixed-base mode: the W x n digits are one flat list over the W x n table entries -> ONE bucket set
    const int Ws = p.Ws = p.fb ? 1 : W;
    const size_t ns = p.ns = p.fb ? (size_t)W * n : n;
    const uint32_t nbk = p.nbk = 1u << (cb - 1);
    p.nb1 = nbk + 1;
    // sort geometry: bucket - 1 = bin << k2 | sub; the partitioned entry packs sub above the index
    int idx_bits = 1;
    while (((size_t)1 << idx_bits) < ns) ++idx_bits;
    int k2 = cb - 1 < 7 ? cb - 1 : 7;
    if (k2 > 31 - idx_bits) k2 = 31 - idx_bits;
    p.idx_bits = idx_bits; p.k2 = k2; p.k1 = cb - 1 - k2;
    const uint32_t nbins = p.nbins = 1u << p.k1;
    p.recode_lds = (size_t)Ws * nbins * 4;
    p.recode_use_lds = p.recode_lds <= 64 * 1024;
    // independent batch items (one MSM per column of create_proof, same bases) are processed
    // `chunk` at a time by the SAME launches (blockIdx.z = item), so the latency-bound sort and
    // reduction phases of one item are hidden behind the work of the others
    size_t chunk = batch;
    {
        const size_t per_item = (size_t)W * n * 12 + 1;  // digits + parted + sorted dominate
        // at most 64 items per launch set, inside the scratch budget (option msm_chunk_gb, default 4 GiB per digit array set)
        const size_t cap = ((size_t)sh.chunk_gb << 30) / per_item;
        if (chunk > cap) chunk = cap ? cap : 1;
        if (chunk > 64) chunk = 64;
        static_assert(64 <= SP_MAX_CHUNK, "chunk size against the pinned read-back area");
    }
    p.chunk = chunk;
    // reduce geometry: each thread owns a slice of buckets and pays one short scalar multiplication for
    // the slice offset, so long slices do less work per bucket but are a long serial chain: a lone MSM
    // (latency-bound) gets 2048-4096 threads per window, a batch (throughput-bound) as few as 256
    uint32_t tpw = nbk >= (1u << 15) ? 4096 : 2048;  // slices of >= 8 buckets (measured: 2^20..2^24 pairs gain 0.07-0.16 ms, 2^18 loses with 4096)
    if (p.fb) tpw = 16384;  // one flat window per item: slices of 2 buckets while the batch is small (the cap below takes over for batches) -- the
                            // opening's rounds are two such items each: reduce 240 -> 190 us per round, k = 18 opening 15.4 -> 14.6 ms
    while (tpw > 256 && (size_t)Ws * tpw * chunk > ((size_t)1 << 16)) tpw >>= 1;  // 2^16 threads = one wave per SIMD (batch of 64 commits: 0.79 -> 0.62 ms)
    if (tpw > nbk) tpw = nbk;
    p.tpw = tpw;
    p.slice = nbk / tpw;
    p.rblocks = (tpw + 255) / 256;
    // segment length: enough segments to fill the chip (>= ~2^18 threads) but at most 128 entries each
    uint32_t seg_len0 = 128;
    // (2^18, round 6: an opening's full-size round -- 2 x 4.2 M digit slots, half of them empty -- takes segments of 32 instead of 16: four pieces per
    //  bucket for the combine instead of eight, k = 18 opening 8.2 -> 8.0 ms; 2^20 .. 2^22 MSMs and lone commitments unchanged; 2^17 loses: 9.0 ms)
    while (seg_len0 > 16 && (size_t)W * n * chunk / seg_len0 < ((size_t)1 << 18)) seg_len0 >>= 1;  // W * n == Ws * ns
    const MsmSegments s0 = msm_segments(Ws, seg_len0, (uint32_t)((ns + seg_len0 - 1) / seg_len0));
    p.seg_len0 = s0.seg_len; p.nseg0 = s0.nseg; p.heavy_stride0 = s0.heavy_stride; p.heavy_blocks0 = s0.heavy_blocks;
    p.max_heavy = msm_max_heavy(Ws, p.nseg0);
    p.part_tiles = (uint32_t)((ns + PART_TILE - 1) / PART_TILE);
    p.flag_bytes = p.fb ? ((size_t)chunk * p.part_tiles + 3) / 4 * 4 : 0;
    // Batched commitments of WITNESS columns (flags, small words: a few 10^4 entries per column, most of them in a handful of buckets)
    // leave the sorted lists almost empty, and fixed 128-entry segments then mean a few hundred threads each walking a serial chain of 128
    // mixed additions (3 ms per batch of 64 flag columns at k = 18, the chip idle).  For batches the entry counts are read back after the
    // histogram scan (one synchronisation per chunk, ~20 us) and the segment length is sized to the entries that exist.
    p.adaptive = batch >= 8;
    // LDS bin sort when the bins are big enough to fill a 1024-thread workgroup and fit with 6 % + 512 entries of slack
    // (uniform digits: the largest of 8192 bins of 2^15 entries is 4.5 sigma = 800 entries above the mean)
    const size_t avg_bin = p.avg_bin = ns / nbins;
    p.bin_cap = (uint32_t)(((avg_bin + avg_bin / 16 + 512 + 1023) / 1024) * 1024);
    p.use_bin_shape = avg_bin >= 4096 && p.bin_cap <= BIN_CAP_MAX;
    p.range_blocks = (p.nb1 + RANGE_BLOCK - 1) / RANGE_BLOCK;  // <= 2^17 / 1024 + 1 = 129 < RANGE_BLOCK threads
    p.sp_subcap = (uint32_t)(ns / 8 / SP_LISTS); p.sp_cap = p.sp_subcap * SP_LISTS;  // a column with more than W n / 8 entries is dense
    p.sparse_shape_ok = p.fb && n >= 4096 && ns / 8 / SP_LISTS >= 1024 && sh.window_override == 0;
    return p;
}

// full-size columns of a sparse chunk (nb of them): the slot count is the entry count
inline MsmSegments msm_segments_dense(const MsmPlan& p, unsigned nb) {
    uint32_t seg_len = 128;
    while (seg_len > 16 && (size_t)p.W * p.n * nb / seg_len < ((size_t)1 << 19)) seg_len >>= 1;
    return msm_segments(p.Ws, seg_len, (uint32_t)((p.ns + seg_len - 1) / seg_len));
}
// lists whose entry counts are known (compact lists, adaptive batches): `sum` entries in all, `most` in the longest list
inline MsmSegments msm_segments_counted(const MsmPlan& p, size_t sum, uint32_t most) {
    // segments for >= 2^17 live threads (round 4, compact lists: 2^16 2.67 / 1.84 / 2.13 / 2.96 / 2.85 ms for the five sparse batches of the k = 18
    // proof, 2^17 2.37 / 1.85 / 2.03 / 2.88 / 2.88, 2^18 2.34 / 1.71 / 2.06 / 2.98 / 3.05: shorter segments shorten the accumulation's chains and
    // lengthen the combine's)
    constexpr int target_log = 17;
    uint32_t seg_len = 128;
    while (seg_len > 16 && sum / seg_len < ((size_t)1 << target_log)) seg_len >>= 1;
    uint32_t nseg = (most + seg_len - 1) / seg_len;  // segments beyond the longest list would find nothing
    if (nseg == 0) nseg = 1;
    return msm_segments(p.Ws, seg_len, nseg);
}

// ---------------------------------------------------------------------------------------
// The plan of one IPA opening (ipa.hip; the generator collapse: ipafold.hip): everything trh_ipa_create_proof decides from its shape --
// the form of its MSMs, the round at which the generators collapse, every round's geometry and the size of every scratch buffer -- as a
// pure function of that shape.  Same constraints as msm_plan.  IpaScratch (ctx.h) is sized from it and from nothing else.
// ---------------------------------------------------------------------------------------
constexpr size_t FE_BYTES = 32;             // a field element
constexpr size_t AFFINE_BYTES = 64;         // an affine base
constexpr size_t ZREC_BYTES = 128;          // a base in the accumulation's record format (ctx.h ZREC)
constexpr unsigned IPA_SUM_BLOCKS = 512;    // workgroups of the opening's evaluation and inner-product launches at most

struct IpaShape {
    uint32_t k;
    size_t set_len;           // points of the base set: 2^k + 1 (g || w) or 2^k + 2 (g || w || u)
    bool table;               // the set has a fixed-base table of fb_W windows of fb_c bits
    int fb_c, fb_W;
    int window_override;      // the context's override, 0: none
    int ipa_fold;             // option ipa_fold
    size_t small_max;         // the largest MSM msm_small_kernel takes (SMALL_MAX_N)
};

// two sub-digits of 5 .. 9 bits per table window (sixteen slices of >= 1 bucket); t and the table level share an entry word; whole workgroups of generators
inline bool ipa_fold_supported(bool table, int c, int W, uint32_t k, uint32_t r) {
    return table && c >= 10 && c <= 18 && W < 0x8000 && r >= 2 && r <= 10 && k >= r + 8;
}
// the round after which the generators are collapsed (0: never -- no table, a small opening, or option ipa_fold = 0).  Option 1 = the measured
// choice: after six rounds, later where the collapsed set would not fit msm_small_kernel (k = 18: 5 / 6 / 7 / 8 rounds -> 9.3 / 9.0 / 9.2 / 9.6 ms)
inline uint32_t ipa_fold_level(bool table, int c, int W, uint32_t k, int ipa_fold) {
    uint32_t r = (uint32_t)ipa_fold;
    if (r == 1) r = k >= 14 ? k - 12 : 0;  // down to 2^12 generators
    return (r > 0 && k >= 14 && ipa_fold_supported(table, c, W, k, r)) ? r : 0;
}

enum IpaFirstMsm {
    IPA_MSM_TABLE,    // over the table, all 2^k + 2 pairs (the scalar of u is zero)
    IPA_MSM_SMALL_Z,  // 2^k + 2 pairs through msm_small_kernel, level 0 of the table as its bases: the table is left alone
    IPA_MSM_PLAIN,    // g || w alone, 2^k + 1 pairs
};
struct IpaRound {
    size_t gens, stride;      // generators of the round's MSM (gens + 2 pairs: then w and u); elements between its two scalar rows
    size_t half; uint32_t bit;
    bool table;               // the MSM runs over the set's table
    int canon;                // the MSM is msm_small_kernel's: the scalar rows leave in canonical form
    int first, wfresh;        // ipa_round_front_kernel's flags: nothing to fold yet; the weights are all one and not in memory yet
    unsigned front_blocks, sum_blocks;  // workgroups of the front launch and (per side) of the inner products
};
struct IpaPlan {
    uint32_t k; size_t n;
    bool with_u;              // the set is g || w || u
    IpaFirstMsm first_msm; size_t first_pairs;  // the commitment to s'; the rounds before a collapse run over the same bases
    uint32_t fold_at; size_t m;                 // the generators collapse in front of round fold_at (0: never) to m = 2^(k - fold_at)
    uint32_t fold_w0, fold_w1, fold_nbk;        // the collapse's two sub-digit widths per table window and its buckets
    int round_window;         // window override of the rounds where the context has none, 0: none
    int window_override; size_t small_max;      // (of the shape)
    unsigned eval_blocks;     // workgroups of the two evaluation launches
    // ---- scratch: the bytes of every buffer of IpaScratch and of the partial sums in Ctx::io, once
    struct {
        size_t b, sp, pp, wgt;   // b = powers of x3, s', p', weights: n elements (s' with the blind and the scalar of u behind it)
        size_t lrsc;             // the two scalar rows of a round's MSM
        size_t gwu, gwuz;        // g || w || u where the set lacks u, G'' || w || u after a collapse: affine and record form; else none
        size_t pp2, b2;          // second halves of the p' / b ping-pong pairs: the folded vectors have at most n / 2 entries
        size_t io;               // partial sums: two sides of IPA_SUM_BLOCKS and two results
        size_t fold_buckets;     // the collapse's buckets + the m sums between the reduction and the inversion
    } bytes;
    size_t fold_list_words;   // bound on the collapse's bucket lists: offsets, then two entries per scalar and window

    IpaRound round(uint32_t j) const {
        IpaRound r{};
        const bool folded = fold_at && j >= fold_at;
        r.gens = folded ? m : n; r.stride = r.gens + 2;
        r.bit = k - j - 1; r.half = (size_t)1 << r.bit;
        r.table = first_msm == IPA_MSM_TABLE && !folded;
        r.canon = (!r.table && r.gens + 2 <= small_max && window_override == 0) ? 1 : 0;
        r.first = j == 0 ? 1 : 0;
        r.wfresh = (j <= 1 || (fold_at && (j == fold_at || j == fold_at + 1))) ? 1 : 0;  // a collapse starts the weights afresh
        r.front_blocks = (unsigned)((r.gens + 255) / 256);
        r.sum_blocks = (unsigned)((r.half + 255) / 256);
        if (r.sum_blocks > IPA_SUM_BLOCKS) r.sum_blocks = IPA_SUM_BLOCKS;
        return r;
    }
};

// the collapse's part of a plan: r rounds at once over a table of W windows of c bits (ipafold.hip); ipa_fold_supported(.., k, r) holds
inline void ipa_collapse_geometry(IpaPlan& p, int c, int W, uint32_t r) {
    p.fold_at = r; p.m = (size_t)1 << (p.k - r);
    p.fold_w0 = (uint32_t)(c + 1) / 2; p.fold_w1 = (uint32_t)c / 2;
    p.fold_nbk = (1u << (p.fold_w0 - 1)) + (1u << (p.fold_w1 - 1));
    p.bytes.fold_buckets = (size_t)(p.fold_nbk + 1) * p.m * RAW_POINT_BYTES;
    p.fold_list_words = (size_t)p.fold_nbk + 1 + ((size_t)2 << r) * W;
}
// a collapse alone (trh_ipa_collapse_generators_dev, any supported (k, r)): its own buffers, the generators go to the caller's
inline IpaPlan ipa_collapse_plan(int c, int W, uint32_t k, uint32_t r) {
    IpaPlan p{};
    p.k = k; p.n = (size_t)1 << k; p.fold_at = r;
    if (ipa_fold_supported(true, c, W, k, r)) ipa_collapse_geometry(p, c, W, r);  // (otherwise ipa_fold_generators refuses the plan)
    return p;
}

inline IpaPlan ipa_plan(const IpaShape& sh) {
    IpaPlan p{};
    const uint32_t k = p.k = sh.k;
    const size_t n = p.n = (size_t)1 << k;
    p.window_override = sh.window_override; p.small_max = sh.small_max;
    // A base set that holds g || w || u (n + 2 points) with fixed-base tables attached (trh_bases_precompute: Params are fixed for
    // the life of a proving key) lets every MSM of the opening run in fixed-base mode: one bucket set instead of one per window,
    // wide windows, no heavy top-window buckets and no Horner over windows on the host between two rounds.
    p.with_u = sh.set_len == n + 2;
    const bool tabled = p.with_u && sh.table;
    // A set small enough for msm_small_kernel does not use its table: one launch + a host Horner beats the fixed-base pipeline's chain of ten
    // launches (k = 10: 3.3 -> 2.1 ms per opening, k = 13: 5.4 -> 3.7); level 0 of the table is the set in the accumulation's record format
    const bool small_z = tabled && n + 2 <= sh.small_max && sh.window_override == 0;
    p.first_msm = !tabled ? IPA_MSM_PLAIN : small_z ? IPA_MSM_SMALL_Z : IPA_MSM_TABLE;
    p.first_pairs = tabled ? n + 2 : n + 1;
    // the round MSMs are batches of two with half of the scalars zero: their time is the latency of the sort / reduction chain,
    // which narrow windows shorten (measured: k = 18 -> c = 10 gives 24.4 ms against 26.7 at the table's 15; k = 14 -> 8);
    // k = 20: the table's 15 is better again (60 vs 68 ms)
    p.round_window = (p.first_msm != IPA_MSM_TABLE && k >= 16 && k <= 18) ? (int)k - 8 : 0;
    p.eval_blocks = (unsigned)((n + 255) / 256);
    if (p.eval_blocks > IPA_SUM_BLOCKS) p.eval_blocks = IPA_SUM_BLOCKS;
    p.bytes.b = p.bytes.pp = p.bytes.wgt = n * FE_BYTES;
    p.bytes.sp = (n + 2) * FE_BYTES;
    p.bytes.lrsc = 2 * (n + 2) * FE_BYTES;
    p.bytes.pp2 = p.bytes.b2 = n * (FE_BYTES / 2) + FE_BYTES;
    p.bytes.io = (size_t)(2 * IPA_SUM_BLOCKS + 2) * FE_BYTES;
    // Hybrid (ipafold.hip): the first r rounds run over the 2^k original bases with the folds as weights (a full-size fixed-base MSM each); then
    // the generators are collapsed for real -- r folds at once from the table -- and the remaining k - r rounds are MSMs over m + 2 = 2^(k - r) + 2
    // points, a fraction of a full-size round each.  Only worth it where a full-size round costs much more than a small one.
    const uint32_t r = ipa_fold_level(p.first_msm == IPA_MSM_TABLE, sh.fb_c, sh.fb_W, k, sh.ipa_fold);
    if (r) ipa_collapse_geometry(p, sh.fb_c, sh.fb_W, r);
    const size_t own = !p.with_u ? n + 2 : r ? p.m + 2 : 0;  // points of the opening's own copy of the round bases
    p.bytes.gwu = own * AFFINE_BYTES; p.bytes.gwuz = own * ZREC_BYTES;
    return p;
}

}  // namespace hostplan
}  // namespace trh
