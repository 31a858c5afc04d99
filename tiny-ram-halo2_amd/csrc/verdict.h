// Verdicts: how a kernel that judges its input reports and how the host reads the report -- the one definition, for every entry point.
// A verdict is n_sums u64 words that kernels only add to (seeded 0), then n_mins u64 words that kernels only lower (seeded ~0: "none"), in
// one grow-only buffer of the context; they come back through its pinned landing area (host_land).  Kernels whose lanes hold consecutive
// indices end in wave_verdict; one that only lowers a minimum, or strides over its rows, uses a bare atomic on its words.
// The rule: ONE verdict is open per context at a time.  An entry that opens one holds the context lock from verdict_begin to its last
// read and calls no entry that opens another (trh_bases_create_compressed calls the decompression, but opens none itself).  The words are
// context scratch like Ctx::scan: TRH_ENTER orders a stream behind the context's previous one, nothing else is needed.
#pragma once
#include "ctx.h"
namespace trh {
// The ballot tail, called by every lane of a wave whose lane l holds index (lane 0's index) + l.  Returns the wave's ballot of `bad`; a wave
// with a bad lane adds their number to *sum and lowers *min to the smallest bad index: one pair of atomics from lane 0, else none.
__device__ __forceinline__ unsigned long long wave_verdict(bool bad, size_t index, unsigned long long* sum, unsigned long long* min) {
    const unsigned long long ballot = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && ballot) {
        atomicAdd(sum, (unsigned long long)__popcll(ballot));
        atomicMin(min, (unsigned long long)(index + (size_t)(__ffsll((long long)ballot) - 1)));
    }
    return ballot;
}
// sizes the words (and the landing area, before anything is in flight towards it) and seeds the two planes on s; sums_dev may be null, mins_dev not
inline int verdict_begin(Ctx& c, size_t n_sums, size_t n_mins, hipStream_t s, unsigned long long** sums_dev, unsigned long long** mins_dev) {
    TRH_TRY(host_land(c, (n_sums + n_mins) * 8, nullptr));
    TRH_TRY(c.verdict.dev.ensure((n_sums + n_mins) * 8));
    c.verdict.n_sums = n_sums; c.verdict.n_mins = n_mins;
    unsigned long long* w = c.verdict.dev.as<unsigned long long>();
    if (n_sums) TRH_HIP_TRY(hipMemsetAsync(w, 0, n_sums * 8, s));
    if (n_mins) TRH_HIP_TRY(hipMemsetAsync(w + n_sums, 0xff, n_mins * 8, s));
    if (sums_dev) *sums_dev = w;
    *mins_dev = w + n_sums;
    return TRH_OK;
}
inline int verdict_fetch(Ctx& c, hipStream_t s) {  // queues the copy of all words into the landing area as verdict_begin sized it
    TRH_HIP_TRY(hipMemcpyAsync(c.pinned_land, c.verdict.dev.p, (c.verdict.n_sums + c.verdict.n_mins) * 8, hipMemcpyDeviceToHost, s));
    return TRH_OK;
}
// fetch, then wait for s; sums_host may be null, mins_host not.  The pointers hold until the context's next verdict_begin or a host_land that has to grow the area
inline int verdict_read(Ctx& c, hipStream_t s, const u64** sums_host, const u64** mins_host) {
    TRH_TRY(verdict_fetch(c, s));
    TRH_HIP_TRY(hipStreamSynchronize(s));
    if (sums_host) *sums_host = (const u64*)c.pinned_land;
    *mins_host = (const u64*)c.pinned_land + c.verdict.n_sums;
    return TRH_OK;
}
// what a min word says: whether a kernel lowered it (where a count exists, it is non-zero exactly then), and its value or `none`
inline bool lowered(u64 min) { return min != ~0ull; }
inline u64 min_or(u64 min, u64 none) { return lowered(min) ? min : none; }
}  // namespace trh
