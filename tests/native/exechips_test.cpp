// Native test of the Exe chips over include/trh.hpp (compiled host, no Python in the process): one trh::exe_chips per field on 1100 steps of
// six opcodes (and, add, udiv, shl, cmpg and the closing answer; immediates and register operands alternate; W = 32, R = 8) -- past one
// strip of the inversion kernel -- brought back through the ABI's from_mont (trh_field_op_dev op 7) and compared with cells made here from
// the default tables written out by hand: Out, the changed flags, a's and b's halves, es_word / os_word, r_word, a_shift, a_power, lsb_b,
// b_flag, sg_a_msb, sg_a_sigma, and zero in every other cell of these opcodes that the list below names.  a_flag is checked by what it
// means: times c + flag' (trh_field_op_dev op 2) it is 1, or both are 0.  A step with an opcode the tables do not know is refused by its
// index with the destination untouched, a chips table that sets flag3 and shift together by its opcode, and trh_stat reports the steps and
// the flag2 rows.  Prints one JSON line; tests/test_gpu_exechips.py runs it.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/trh.hpp"

using namespace trh;

static std::vector<Limbs> canonical(Field f, const void* dev, size_t count) {
    DeviceBuffer plain(count * 32);
    check(trh_field_op_dev((int)f, 7, dev, nullptr, plain.data(), count, nullptr), "from_mont");
    check(trh_stream_synchronize(nullptr), "sync");
    std::vector<Limbs> out(count);
    plain.download(out.data(), count * 32);
    return out;
}
static uint64_t even_of(uint64_t w) { return w & 0x5555555555555555ull; }
static uint64_t odd_of(uint64_t w) { return (w >> 1) & 0x5555555555555555ull; }

int main() {
    int failed = 0, checks = 0;
    std::printf("{\"test\": \"exechips\"");
    try {
        check(trh_init(0), "trh_init");
        uint64_t x = 0x9e3779b97f4a7c15ull;
        auto next = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
        const uint32_t W = 32, R = 8;
        const size_t m = 1100, n = 2048, ncols = exe_chip_columns(R);
        const uint32_t ops[5] = {0, 4, 9, 11, 16};
        std::vector<uint32_t> pc(m), inst(m), a(m), value(m, 0), regs(m * R), bits((m + 31) / 32, 0);
        for (size_t i = 0; i < m; ++i) {
            const bool a_is_reg = (i & 1) != 0;
            const uint32_t op = i + 1 == m ? 31u : ops[next() % 5];
            pc[i] = i ? (uint32_t)next() : 0u;
            a[i] = a_is_reg ? (uint32_t)(next() % R) : (i % 3 == 0 ? (uint32_t)(next() % 40) : (uint32_t)next());
            inst[i] = exe_encode(op, (uint32_t)(next() % R), (uint32_t)(next() % R), a_is_reg);
            for (uint32_t k = 0; k < R; ++k) regs[i * R + k] = i ? (next() % 5 ? (uint32_t)next() : 0u) : 0u;
            if (i && (next() & 1)) bits[i >> 5] |= 1u << (i & 31);
        }
        // the columns by name (R = 8)
        const size_t CH_REG = 13, CH_PC = 13 + R, CH_FLAG = 14 + R, CELL = 15 + R;
        const size_t A_EVEN = CELL, A_ODD = CELL + 1, B_EVEN = CELL + 2, B_ODD = CELL + 3, ES_WORD = CELL + 8, OS_WORD = CELL + 11, SG_A_MSB = CELL + 14, SG_A_SIGMA = CELL + 15,
                     R_WORD = CELL + 29, A_SHIFT = CELL + 32, A_POWER = CELL + 33, A_FLAG = CELL + 34, LSB_B = CELL + 35, B_FLAG = CELL + 36;
        const std::vector<size_t> checked = {A_EVEN, A_ODD, B_EVEN, B_ODD, ES_WORD, OS_WORD, SG_A_MSB, SG_A_SIGMA, R_WORD, A_SHIFT, A_POWER, LSB_B, B_FLAG};
        std::vector<std::vector<uint64_t>> want(ncols, std::vector<uint64_t>(n, 0));
        std::vector<uint64_t> denominator(n * 4, 0);  // c + flag' on flag2 rows, as canonical limbs
        uint64_t flag2_rows = 0;
        for (size_t i = 0; i < m; ++i) {
            const uint32_t op = inst[i] & 31, ri = (inst[i] >> 8) & 15, rj = (inst[i] >> 12) & 15;
            const bool a_is_reg = (inst[i] >> 16) & 1;
            const uint32_t* now = &regs[i * R];
            const uint64_t A = a_is_reg ? now[a[i]] : a[i], RJ = now[rj], RI = now[ri];
            const uint64_t ri_next = i + 1 < m ? regs[(i + 1) * R + ri] : 0, flag_next = i + 1 < m ? (bits[(i + 1) >> 5] >> ((i + 1) & 31)) & 1 : 0;
            auto out = [&](size_t bit) { want[bit][i] = 1; };
            auto halves = [&](size_t even, uint64_t w) { want[even][i] = even_of(w); want[even + 1][i] = odd_of(w); };
            auto flag2 = [&](uint64_t c) { denominator[i * 4] = c + flag_next; ++flag2_rows; };
            switch (op) {
            case 0:   // and: a = A, b = RJ, c = ri'
                out(0); out(9); out(10); want[CH_REG + ri][i] = 1; want[CH_FLAG][i] = 1;
                halves(A_EVEN, A); halves(B_EVEN, RJ); want[ES_WORD][i] = even_of(A) + even_of(RJ); want[OS_WORD][i] = odd_of(A) + odd_of(RJ); flag2(ri_next);
                break;
            case 4:   // add: b = RJ is decomposed
                out(3); want[CH_REG + ri][i] = 1; want[CH_FLAG][i] = 1; halves(B_EVEN, RJ);
                break;
            case 9: { // udiv: a = RJ mod A, b = ri', c = A
                out(7); out(9); out(10); out(11); want[CH_REG + ri][i] = 1; want[CH_FLAG][i] = 1;
                const uint64_t rem = A ? RJ % A : 0;
                halves(A_EVEN, rem); halves(B_EVEN, ri_next); want[R_WORD][i] = A ? A - rem - 1 : 0; flag2(A);
                break;
            }
            case 11:  // shl: a = A, b = RJ
                out(8); out(12); want[CH_REG + ri][i] = 1; want[CH_FLAG][i] = 1;
                halves(B_EVEN, RJ); want[R_WORD][i] = A > W ? 0 : W - A; want[A_SHIFT][i] = A > W; want[A_POWER][i] = 1ull << (A < W ? A : W);
                want[LSB_B][i] = RJ & 1; want[B_FLAG][i] = 1;
                break;
            case 16:  // cmpg: a = RI, b = the comparison's advice (decomposed, not checked here), c = A
                out(5); want[CH_FLAG][i] = 1; halves(A_EVEN, RI);
                want[SG_A_MSB][i] = RI >> 31; want[SG_A_SIGMA][i] = RI >> 31 ? (1ull << 32) - RI : RI;
                want[B_EVEN][i] = want[B_ODD][i] = ~0ull;  // not compared
                break;
            default: break;  // answer: nothing
            }
        }
        (void)CH_PC;
        DeviceBuffer d_pc(4 * m), d_inst(4 * m), d_a(4 * m), d_value(4 * m), d_regs(4 * m * R), d_bits(4 * bits.size()), d_den(32 * n), d_prod(32 * n);
        d_pc.upload(pc.data(), 4 * m); d_inst.upload(inst.data(), 4 * m); d_a.upload(a.data(), 4 * m); d_value.upload(value.data(), 4 * m);
        d_regs.upload(regs.data(), 4 * m * R); d_bits.upload(bits.data(), 4 * bits.size());
        auto u32p = [](DeviceBuffer& b) { return (const uint32_t*)b.data(); };
        for (Field f : {Field::Fp, Field::Fq}) {
            DeviceBuffer dst(ncols * n * 32);
            exe_chips(f, W, R, u32p(d_pc), u32p(d_inst), u32p(d_a), u32p(d_value), u32p(d_regs), u32p(d_bits), m, dst.data(), n);
            const std::vector<Limbs> cells = canonical(f, dst.data(), ncols * n);
            auto compare = [&](size_t c) {
                for (size_t r = 0; r < n; ++r) {
                    if (want[c][r] == ~0ull) continue;
                    ++checks;
                    if (cells[c * n + r] != Limbs{want[c][r], 0, 0, 0}) ++failed;
                }
            };
            for (size_t c = 0; c < CELL; ++c) compare(c);
            for (size_t c : checked) compare(c);
            for (size_t c = 0; c < ncols; ++c)  // behind the trace every column is zero
                for (size_t r = m; r < n; ++r, ++checks)
                    if (cells[c * n + r] != Limbs{0, 0, 0, 0}) ++failed;
            // a_flag (c + flag') = 1 where c + flag' != 0, and a_flag = 0 elsewhere
            d_den.upload(denominator.data(), 32 * n);
            check(trh_field_op_dev((int)f, 6, d_den.data(), nullptr, d_den.data(), n, nullptr), "to_mont");
            check(trh_field_op_dev((int)f, 2, d_den.data(), (const char*)dst.data() + A_FLAG * n * 32, d_prod.data(), n, nullptr), "mul");
            const std::vector<Limbs> product = canonical(f, d_prod.data(), n);
            size_t inverted = 0;
            for (size_t r = 0; r < n; ++r, ++checks) {
                const uint64_t one = denominator[r * 4] ? 1 : 0;
                inverted += one;
                if (product[r] != Limbs{one, 0, 0, 0}) ++failed;
                if (!one && cells[A_FLAG * n + r] != Limbs{0, 0, 0, 0}) ++failed;
            }
            ++checks; if (inverted < 100 || inverted == flag2_rows) ++failed;  // both kinds of flag2 row are present
            uint64_t rows = 0, counted = 0;
            check(trh_stat("exechips_rows", &rows), "trh_stat");
            check(trh_stat("exechips_flag2_rows", &counted), "trh_stat");
            ++checks; if (rows != m) ++failed;
            ++checks; if (counted != flag2_rows) ++failed;
        }
        const std::vector<uint64_t> sentinel(ncols * n * 4, 0xA5A5A5A5A5A5A5A5ull);
        std::vector<uint64_t> after(sentinel.size());
        DeviceBuffer dst(ncols * n * 32);
        dst.upload(sentinel.data(), ncols * n * 32);
        // a chips table whose udiv sets shift next to flag3: refused by the opcode
        ExeChips faulty = exe_default_chips();
        faulty[9] |= TRH_CHIP_SHIFT;
        bool refused = false;
        try { exe_chips(Field::Fq, W, R, u32p(d_pc), u32p(d_inst), u32p(d_a), u32p(d_value), u32p(d_regs), u32p(d_bits), m, dst.data(), n, exe_default_selection(), faulty); }
        catch (const Error& e) { refused = std::strstr(e.what(), "chips[9]") != nullptr; }
        ++checks; if (!refused) ++failed;
        // an opcode the tables do not know: refused by the step's index, the destination as it was
        inst[123] = exe_encode(23, 0, 0, false);
        inst[900] = exe_encode(30, 0, 0, false);
        d_inst.upload(inst.data(), 4 * m);
        refused = false;
        try { exe_chips(Field::Fp, W, R, u32p(d_pc), u32p(d_inst), u32p(d_a), u32p(d_value), u32p(d_regs), u32p(d_bits), m, dst.data(), n); }
        catch (const Error& e) { refused = std::strstr(e.what(), "step 123 ") != nullptr; }
        check(trh_stream_synchronize(nullptr), "sync");
        dst.download(after.data(), ncols * n * 32);
        ++checks; if (!refused) ++failed;
        ++checks; if (after != sentinel) ++failed;
        trh_shutdown();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        ++failed;
    }
    std::printf(", \"checks\": %d, \"checks_failed\": %d}\n", checks, failed);
    return failed ? 1 : 0;
}
