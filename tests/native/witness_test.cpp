// Native test of the packed witness intake over include/trh.hpp (compiled host, no Python in the process): one trh::columns_from_ints from
// host vectors (unsigned and signed), one trh::even_odd_split of resident words and one trh::even_bits_table per field, each brought back
// through the ABI's from_mont (trh_field_op_dev op 7) and compared with values computed here with 128-bit integers.  Prints one JSON line;
// tests/test_gpu_witness.py runs it.
#include <cstdio>
#include <vector>

#include "../../include/trh.hpp"

using namespace trh;

// dev: count elements in Montgomery form -> their canonical values
static std::vector<Limbs> canonical(Field f, DeviceBuffer& dev, size_t count) {
    DeviceBuffer plain(count * 32);
    check(trh_field_op_dev((int)f, 7, dev.data(), nullptr, plain.data(), count, nullptr), "from_mont");
    check(trh_stream_synchronize(nullptr), "sync");
    std::vector<Limbs> out(count);
    plain.download(out.data(), count * 32);
    return out;
}
// v as a canonical element: m - |v| for v < 0, the borrow carried through the four words as 128-bit differences
static Limbs canonical_of(Field f, __int128 v) {
    if (v >= 0) return Limbs{(uint64_t)v, (uint64_t)((unsigned __int128)v >> 64), 0, 0};
    const unsigned __int128 mag = (unsigned __int128)(-v);
    return host::sub_raw(host::modulus(f), Limbs{(uint64_t)mag, (uint64_t)(mag >> 64), 0, 0});
}

int main() {
    int failed = 0, checks = 0;
    std::printf("{\"test\": \"witness\"");
    try {
        check(trh_init(0), "trh_init");
        for (Field f : {Field::Fp, Field::Fq}) {
            uint64_t x = 0x9e3779b97f4a7c15ull;
            auto next = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
            // unsigned words from a host vector, zero behind them
            std::vector<uint64_t> words = {0, 1, 0xffffffffull, 1ull << 63, ~0ull};
            for (int i = 0; i < 300; ++i) words.push_back(next());
            const size_t n = words.size() + 7;
            DeviceBuffer d(n * 32);
            columns_from_ints(f, words, d.data(), n);
            std::vector<Limbs> got = canonical(f, d, n);
            for (size_t i = 0; i < n; ++i, ++checks) if (got[i] != (i < words.size() ? canonical_of(f, (__int128)words[i]) : Limbs{0, 0, 0, 0})) ++failed;
            // signed words
            std::vector<int64_t> sw = {0, -1, 1ll << 31, -(1ll << 31), INT64_MAX, INT64_MIN};
            for (int i = 0; i < 300; ++i) sw.push_back((int64_t)next());
            const size_t ns = sw.size() + 1;
            DeviceBuffer ds(ns * 32);
            columns_from_ints(f, sw, ds.data(), ns);
            got = canonical(f, ds, ns);
            for (size_t i = 0; i < ns; ++i, ++checks) if (got[i] != (i < sw.size() ? canonical_of(f, (__int128)sw[i]) : Limbs{0, 0, 0, 0})) ++failed;
            // the split of resident u32 words
            std::vector<uint32_t> w32 = {0, ~0u, 0xaaaaaaaau, 0x55555555u};
            for (int i = 0; i < 300; ++i) w32.push_back((uint32_t)next());
            const size_t nw = w32.size() + 3;
            DeviceBuffer src(w32.size() * 4), even(nw * 32), odd(nw * 32);
            src.upload(w32.data(), w32.size() * 4);
            even_odd_split(f, IntKind::U32, src.data(), w32.size(), 1, w32.size(), even.data(), odd.data(), nw);
            const std::vector<Limbs> ge = canonical(f, even, nw), go = canonical(f, odd, nw);
            for (size_t i = 0; i < nw; ++i, ++checks) {
                const uint64_t w = i < w32.size() ? w32[i] : 0;
                if (ge[i] != Limbs{w & 0x55555555ull, 0, 0, 0} || go[i] != Limbs{(w >> 1) & 0x55555555ull, 0, 0, 0}) ++failed;
            }
            // the even-bits table of 8-bit words in a column of 64 rows
            DeviceBuffer tab(64 * 32);
            even_bits_table(f, 8, tab.data(), 64);
            const std::vector<Limbs> gt = canonical(f, tab, 64);
            for (uint64_t i = 0; i < 64; ++i, ++checks) {
                uint64_t s = 0;
                for (int j = 0; j < 4; ++j) s |= ((i >> j) & 1) << (2 * j);
                if (gt[i] != Limbs{i < 16 ? s : 0, 0, 0, 0}) ++failed;
            }
        }
        trh_shutdown();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        ++failed;
    }
    std::printf(", \"checks\": %d, \"checks_failed\": %d}\n", checks, failed);
    return failed ? 1 : 0;
}
