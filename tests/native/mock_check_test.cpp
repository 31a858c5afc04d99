// Native test of trh::GateEvaluator::check and trh::lookup_check over include/trh.hpp (compiled host, no Python in the process): a fixed
// 2^6-row system with 58 usable rows, built here and restated by tests/test_gpu_mock.py, which compares the JSON line printed below with the
// verdicts of the Python layer and of its own model.
//   columns  a[r] = r + 1, b[r] = 2 r + 3, c[r] = a[r] b[r]; then c[5] += 1, c[40] += 1 and a[58] += 1 (row 58 is the first blinding row)
//   gates    p0 = a b - c          bad on rows 5 and 40
//            p1 = a(+1) - a - 1    bad on row 57, which reads the blinding row through its rotation
//   lookup   width 2, table row t = (t, 3 t + 1); input row r = table row 5 r mod 58, but row 0 = (1, 1) and row 57 = table row 60 (a tuple
//            that only rows beyond the usable ones hold): bad on rows 0 and 57
//   usage: mock_check_test <fp|fq>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/trh.hpp"

using namespace trh;

static DeviceBuffer upload(const std::vector<Limbs>& col) {
    DeviceBuffer d(col.size() * 32);
    d.upload(col.data(), col.size() * 32);
    return d;
}

int main(int argc, char** argv) {
    int failed = 0;
    std::printf("{\"test\": \"mock_check\"");
    try {
        require(argc == 2, "usage: mock_check_test <fp|fq>");
        const Field f = std::strcmp(argv[1], "fp") == 0 ? Field::Fp : Field::Fq;
        const uint32_t k = 6;
        const size_t n = (size_t)1 << k, usable = n - 6;
        check(trh_init(0), "trh_init");

        std::vector<Limbs> a(n), b(n), c(n);
        for (size_t r = 0; r < n; ++r) { a[r] = host::from_u64(f, r + 1); b[r] = host::from_u64(f, 2 * r + 3); c[r] = host::mul(f, a[r], b[r]); }
        const Limbs one = host::one(f);
        c[5] = host::add(f, c[5], one);
        c[40] = host::add(f, c[40], one);
        a[usable] = host::add(f, a[usable], one);
        const DeviceBuffer da = upload(a), db = upload(b), dc = upload(c);
        const Expr p0 = advice(0) * advice(1) - advice(2);
        const Expr p1 = advice(0, 1) - advice(0) - constant(one);
        GateEvaluator ev(compile_outputs(f, {p0, p1}), 2);
        std::vector<const void*> cols;
        for (const auto& key : ev.program.columns) cols.push_back(key.second == 0 ? da.data() : key.second == 1 ? db.data() : dc.data());
        DeviceBuffer words(2 * 8);
        const uint64_t fill[2] = {~0ull, ~0ull};  // every word is written, zeros included
        words.upload(fill, sizeof(fill));
        const GateEvaluator::Check g = ev.check(cols, k, usable, words.data());
        uint64_t gw[2];
        words.download(gw, sizeof(gw));
        std::printf(", \"gate_n_bad\": [%llu, %llu], \"gate_first_bad_row\": [%llu, %llu], \"gate_bitmap\": [\"%016llx\", \"%016llx\"]", (unsigned long long)g.n_bad[0],
                    (unsigned long long)g.n_bad[1], (unsigned long long)g.first_bad_row[0], (unsigned long long)g.first_bad_row[1], (unsigned long long)gw[0], (unsigned long long)gw[1]);
        const GateEvaluator::Check plain = ev.check(cols, k, usable);  // without a bitmap: the same counts
        if (plain.n_bad != g.n_bad || plain.first_bad_row != g.first_bad_row) ++failed;

        std::vector<Limbs> t0(n), t1(n), i0(n), i1(n);
        for (size_t t = 0; t < n; ++t) { t0[t] = host::from_u64(f, t); t1[t] = host::from_u64(f, 3 * t + 1); }
        for (size_t r = 0; r < n; ++r) { i0[r] = t0[5 * r % usable]; i1[r] = t1[5 * r % usable]; }
        i0[0] = one; i1[0] = one;
        i0[usable - 1] = t0[60]; i1[usable - 1] = t1[60];
        const DeviceBuffer dt0 = upload(t0), dt1 = upload(t1), di0 = upload(i0), di1 = upload(i1);
        DeviceBuffer lw(8);
        lw.upload(fill, 8);
        const LookupCheck l = lookup_check(f, {di0.data(), di1.data()}, {dt0.data(), dt1.data()}, usable, lw.data());
        uint64_t lword = 0, probes = 0;
        lw.download(&lword, 8);
        check(trh_stat("lookup_check_probes", &probes), "trh_stat");
        std::printf(", \"lookup_n_bad\": %llu, \"lookup_first_bad_row\": %llu, \"lookup_bitmap\": \"%016llx\", \"lookup_probes\": %llu", (unsigned long long)l.n_bad,
                    (unsigned long long)l.first_bad_row, (unsigned long long)lword, (unsigned long long)probes);
        bool refused = false;  // usable_rows beyond the domain throws
        try { (void)ev.check(cols, k, n + 1); } catch (const Error&) { refused = true; }
        if (!refused) ++failed;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        ++failed;
    }
    trh_shutdown();
    std::printf(", \"checks_failed\": %d}\n", failed);
    return failed ? 1 : 0;
}
