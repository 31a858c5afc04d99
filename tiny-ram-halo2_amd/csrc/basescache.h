// Policy of the opt-in cache of base sets seen by the host-pointer MSM entries (msmapi.hip best_multiexp_host; option bases_cache).  No HIP
// in here: handles are opaque pointers, and tests/native/basescache_test.cpp compiles and runs the policy on its own with made-up ones.
//
// `best_multiexp(coeffs, bases)` is called ~500 times per proof with the SAME `Params.g_lagrange` / `Params.g` slices.  The plain
// two-function shim passes host pointers every time; re-uploading 64 B per base would cost as much as the
// MSM.  A set is recognised by (curve, pointer, length, FNV-1a hash of ALL n points -- recomputed on every call, so a base changed in
// place is never served from the stale copy) and only becomes resident at its SECOND identical sighting, which keeps the once-per-proof
// IPA slices out of the 8-entry LRU; at its fourth use a set also gets the fixed-base tables.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

struct trh_bases;

namespace trh {

struct BasesCache {
    static constexpr size_t CANDIDATES = 16, RESIDENT = 8;
    static constexpr unsigned TABLE_AT_USE = 4;
    struct Key {
        int curve;
        const void* host;
        size_t n;
        uint64_t fp;
        bool operator==(const Key& o) const { return curve == o.curve && host == o.host && n == o.n && fp == o.fp; }
    };
    struct Entry { Key key; trh_bases* h; uint64_t stamp; unsigned uses; };
    std::vector<Entry> resident;
    Key seen[CANDIDATES] = {};
    unsigned seen_next = 0;
    uint64_t stamp = 0;

    static uint64_t fingerprint(const uint64_t* bases, size_t n) {  // n points of eight words each
        uint64_t h = 0xcbf29ce484222325ull ^ (uint64_t)n;
        for (size_t k = 0; k < n * 8; ++k) { h ^= bases[k]; h *= 0x100000001b3ull; }
        return h;
    }
    Entry* find(const Key& k) {
        for (Entry& e : resident) if (e.key == k) return &e;
        return nullptr;
    }
    // a set that is not resident: true at a repeated sighting (the caller makes it resident: evict, then insert); a first sighting is
    // remembered in the ring, over the oldest candidate
    bool sighting(const Key& k) {
        for (const Key& c : seen) if (c == k) return true;
        seen[seen_next++ % CANDIDATES] = k;
        return false;
    }
    // room for one more resident set: the handle of the least recently used one, removed from the cache and now the caller's to
    // destroy, or null while there is room
    trh_bases* evict() {
        if (resident.size() < RESIDENT) return nullptr;
        size_t victim = 0;
        for (size_t i = 1; i < resident.size(); ++i) if (resident[i].stamp < resident[victim].stamp) victim = i;
        trh_bases* h = resident[victim].h;
        resident.erase(resident.begin() + victim);
        return h;
    }
    Entry* insert(const Key& k, trh_bases* h) {
        resident.push_back(Entry{k, h, 0, 0});
        return &resident.back();
    }
    // one MSM over a resident set; true exactly once, at the use from which the set is worth a fixed-base table
    bool use(Entry* e) {
        e->stamp = ++stamp;
        return ++e->uses == TABLE_AT_USE;
    }
    // forgets everything; the handles of the resident sets are the caller's to destroy
    std::vector<trh_bases*> clear() {
        std::vector<trh_bases*> out;
        for (const Entry& e : resident) out.push_back(e.h);
        resident.clear();
        for (Key& c : seen) c = Key{};
        return out;
    }
};

}  // namespace trh
