// Native test of Params::write / Params::read over include/trh.hpp (compiled host, no Python in the process): Params over synthetic points at
// k = 10 are written, the bytes are read back through the device decoder, and the two must agree point for point, on w and u, and on the
// commitments of one column through both base sets -- with fixed-base tables attached on both sides.  A corrupted or shortened file must
// throw.  Prints one JSON line; run by tests/test_gpu_encoding.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/trh.hpp"

using namespace trh;

static int failed = 0;
#define CHECK(cond) do { if (!(cond)) { ++failed; std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

static bool same(const std::vector<Affine>& a, const std::vector<Affine>& b) { return a.size() == b.size() && !std::memcmp(a.data(), b.data(), a.size() * sizeof(Affine)); }

template <class Fn> static bool throws(Fn fn) {
    try { fn(); } catch (const Error&) { return true; }
    return false;
}

int main() {
    try {
        check(trh_init(0), "trh_init");
        const uint32_t k = 10;
        for (Curve c : {Curve::Pallas, Curve::Vesta}) {
            // g, g_lagrange, w, u as a Params file has them: both resident sets end in the same w (the synthetic constructor's do not)
            std::vector<Affine> g = Bases::generate(c, 1000, 3, ((size_t)1 << k) + 1).download();
            const Affine w = g.back();
            g.pop_back();
            Params a(c, k, g, Bases::generate(c, 1077, 5, (size_t)1 << k).download(), w, Bases::generate(c, 4242, 1, 1).download()[0]);
            const std::vector<uint8_t> file = a.write();
            CHECK(file.size() == 4 + 32 * (2 * a.n + 2));
            Params b = Params::read(c, file);
            CHECK(b.k == k && b.n == a.n);
            CHECK(same(a.g().download(), b.g().download()));
            CHECK(same(a.g_lagrange().download(), b.g_lagrange().download()));
            CHECK(!std::memcmp(&a.w, &b.w, sizeof(Affine)) && !std::memcmp(&a.u, &b.u, sizeof(Affine)));
            CHECK(b.ipa_bases().len() == a.n + 2 && same(a.ipa_bases().download(), b.ipa_bases().download()));
            CHECK(b.write() == file);
            std::vector<Limbs> poly(a.n);
            uint64_t s = 0x9e3779b97f4a7c15ull;
            for (Limbs& v : poly) for (int i = 0; i < 4; ++i) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; v[i] = i == 3 ? s >> 2 : s; }
            const Limbs blind = poly[7];
            const Point pa = a.commit(poly, blind), pb = b.commit(poly, blind), la = a.commit_lagrange(poly, blind), lb = b.commit_lagrange(poly, blind);
            CHECK(!std::memcmp(&pa, &pb, sizeof(Point)) && !std::memcmp(&la, &lb, sizeof(Point)));
            std::vector<uint8_t> bad = file;
            bad[4 + 32 * 5] ^= 1;  // g[5]: another x -- if that x happens to be on the curve the points differ instead
            bool differs = false;
            const bool threw = throws([&] { Params q = Params::read(c, bad, false); differs = !same(q.g().download(), a.g().download()); });
            CHECK(threw || differs);
            std::vector<uint8_t> high = file;
            std::memset(&high[4 + 32 * 9], 0xff, 32);  // x = 2^255 - 1 >= the modulus
            CHECK(throws([&] { Params::read(c, high, false); }));
            std::vector<uint8_t> cut(file.begin(), file.end() - 1);
            CHECK(throws([&] { Params::read(c, cut, false); }));
        }
        trh_shutdown();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        ++failed;
    }
    std::printf("{\"test\": \"params_io\", \"checks_failed\": %d}\n", failed);
    return failed ? 1 : 0;
}
