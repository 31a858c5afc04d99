// The bucket lists of the IPA generator collapse (ipafold.hip), free of HIP types so that a plain C++ test can check them
// (tests/native/foldplan_test.cpp): the signed sub-digit recoding of the 2^r shared scalars and the counting sort of its entries.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "hostcombine.h"

namespace trh {
namespace foldplan {

constexpr uint32_t FOLD_SIGN = 0x80000000u;
enum { FOLD_PLAN_OK = 0, FOLD_PLAN_NO_FIT = 1 };  // NO_FIT: a scalar carries out of the table's W windows of c bits

// the bucket lists of the 2^r shared scalars (canonical 4 x 64-bit words each): offsets[nbk + 1], then the entries bucket by bucket.
// Each window of c bits is two signed sub-digits of w0 (low) and w1 (high) bits, w0 + w1 = c; a sub-digit above 2^(w-1) becomes
// d - 2^w and carries one into the next sub-window.  Bucket (s, |d|) is row (s ? 2^(w0-1) : 0) + |d| - 1; an entry is
// level j << 16 | t | sign << 31, and within a bucket the entries keep the order they were made in: (t, j) ascending.
inline int fold_plan(const std::vector<hostcombine::H>& sc, int c, int W, uint32_t w0, uint32_t w1, std::vector<uint32_t>& plan, uint32_t& nbk) {
    typedef uint32_t u32;
    const u32 nb0 = 1u << (w0 - 1), nb1 = 1u << (w1 - 1);
    nbk = nb0 + nb1;
    std::vector<u32> bucket, entry;
    bucket.reserve(sc.size() * W * 2); entry.reserve(sc.size() * W * 2);
    std::vector<u32> count(nbk + 1, 0);
    auto bits = [](const hostcombine::H& v, u32 o, u32 w) -> u32 {
        if (o >= 256) return 0;
        uint64_t x = v.l[o >> 6] >> (o & 63);
        if ((o & 63) + w > 64 && (o >> 6) + 1 < 4) x |= v.l[(o >> 6) + 1] << (64 - (o & 63));
        return (u32)(x & ((1ull << w) - 1));
    };
    for (size_t t = 0; t < sc.size(); ++t) {
        u32 carry = 0;
        for (int j = 0; j < W; ++j)
            for (u32 s = 0; s < 2; ++s) {
                const u32 w = s ? w1 : w0;
                int d = (int)(bits(sc[t], (u32)(c * j) + (s ? w0 : 0), w) + carry);
                if (d > (1 << (w - 1))) { d -= 1 << w; carry = 1; } else carry = 0;
                if (!d) continue;
                const u32 mag = (u32)(d < 0 ? -d : d);
                const u32 b = (s ? nb0 : 0) + mag - 1;
                bucket.push_back(b);
                entry.push_back(((u32)j << 16) | (u32)t | (d < 0 ? FOLD_SIGN : 0u));
                ++count[b];
            }
        if (carry) return FOLD_PLAN_NO_FIT;
    }
    plan.assign(nbk + 1 + entry.size(), 0);
    u32 run = 0;
    for (u32 b = 0; b < nbk; ++b) { plan[b] = run; run += count[b]; }
    plan[nbk] = run;
    std::vector<u32> cur(plan.begin(), plan.begin() + nbk);
    for (size_t e = 0; e < entry.size(); ++e) plan[nbk + 1 + cur[bucket[e]]++] = entry[e];
    return FOLD_PLAN_OK;
}

}  // namespace foldplan
}  // namespace trh
