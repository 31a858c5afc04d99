// The policy of the opt-in bases cache (csrc/basescache.h) with made-up host pointers and handles: candidates and promotion, the ring of
// 16, the LRU of 8, the one "precompute now", clear, and the fingerprint against a value computed independently.  Plain C++, never loads
// the library; run by tests/test_hostcombine.py.
#include <cstdint>
#include <cstdio>
#include <set>

#include "../../tiny-ram-halo2_amd/csrc/basescache.h"

int main() {
    using trh::BasesCache;
    typedef BasesCache::Key Key;
    int bad = 0;
    auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("basescache: FAILED %s\n", what); ++bad; } };
    static char host[64];                                                        // made-up base arrays: only their addresses are used
    auto handle = [](size_t i) { return (trh_bases*)(uintptr_t)(0x1000 + 16 * i); };  // made-up handles, never dereferenced
    auto key = [&](size_t i, uint64_t fp = 7) { return Key{0, &host[i], 1024, fp}; };

    {   // candidates and promotion
        BasesCache c;
        expect(!c.find(key(0)) && !c.sighting(key(0)), "a first sighting is a candidate");
        expect(!c.find(key(0)) && c.resident.empty(), "and no resident set");
        expect(!c.sighting(key(0, 8)), "the same pointer and length with another fingerprint is another set");
        expect(!c.sighting(Key{1, &host[0], 1024, 7}) && !c.sighting(Key{0, &host[0], 1025, 7}), "so is another curve, another length");
        expect(c.sighting(key(0)), "the second identical sighting promotes");
        expect(c.evict() == nullptr, "nothing to evict below 8 sets");
        BasesCache::Entry* e = c.insert(key(0), handle(0));
        expect(c.find(key(0)) == e && e->h == handle(0) && !c.find(key(0, 8)), "the promoted set is found by its whole key");
        expect(!c.use(e) && !c.use(e) && !c.use(e), "uses 1 to 3: no table");
        expect(c.use(e), "the fourth use says precompute");
        bool again = false;
        for (int i = 0; i < 40; ++i) again |= c.use(e);
        expect(!again && e->uses == 44, "and no later use does");
    }
    {   // the ring holds 16 candidates
        BasesCache c;
        for (size_t i = 0; i < 16; ++i) expect(!c.sighting(key(i)), "16 distinct candidates");
        expect(c.sighting(key(0)) && c.sighting(key(15)), "all 16 are remembered");
        expect(!c.sighting(key(16)), "the 17th is new");
        expect(c.sighting(key(16)) && c.sighting(key(1)), "it is remembered, and so is the second");
        expect(!c.sighting(key(0)), "it took the place of the first");
    }
    {   // 8 resident sets, least recently used out
        BasesCache c;
        for (size_t i = 0; i < 8; ++i) {
            expect(c.evict() == nullptr, "room for 8");
            c.use(c.insert(key(i), handle(i)));
        }
        c.use(c.find(key(0)));  // 1 is now the least recently used
        std::multiset<trh_bases*> returned;
        trh_bases* v = c.evict();
        returned.insert(v);
        expect(v == handle(1) && c.resident.size() == 7 && !c.find(key(1)), "the ninth promotion evicts the least recently used set");
        expect(c.evict() == nullptr, "and hands over one handle only");
        c.use(c.insert(key(8), handle(8)));
        v = c.evict();
        returned.insert(v);
        expect(v == handle(2), "then the next one");
        c.insert(key(9), handle(9));   // never used: stamp 0
        expect(c.resident.size() == 8, "eight again");
        for (trh_bases* h : c.clear()) returned.insert(h);
        bool once = returned.size() == 10;
        for (size_t i = 0; i < 10; ++i) once = once && returned.count(handle(i)) == 1;
        expect(once, "eviction and clear together return every handle exactly once");
        expect(c.resident.empty() && c.clear().empty(), "clear leaves nothing behind");
        expect(!c.find(key(0)) && !c.sighting(key(0)), "nor a candidate");
    }
    {   // FNV-1a over the 64-bit words, seeded with the length: the literal is from a Python loop over the same 128 bytes (little-endian words)
        uint64_t two[16];
        for (uint64_t k = 0; k < 16; ++k) two[k] = 0x0123456789abcdefull * (k + 1);
        expect(BasesCache::fingerprint(two, 2) == 0xdb78a4b0df05e257ull, "fingerprint of a fixed 2-point input");
        two[15] ^= 1;
        expect(BasesCache::fingerprint(two, 2) != 0xdb78a4b0df05e257ull, "one changed bit changes it");
        expect(BasesCache::fingerprint(two, 1) != BasesCache::fingerprint(two, 2), "so does the length");
    }
    std::printf(bad ? "basescache: FAILED (%d)\n" : "basescache: ok\n", bad);
    return bad ? 1 : 0;
}
