// Native test of the Exe table over include/trh.hpp (compiled host, no Python in the process): one trh::exe_table per field on 700 steps of
// six opcodes (add, sub, mull, shl, cjmp and the closing answer; immediates and register operands alternate; W = 32, R = 8) -- past two
// workgroups of rows -- brought back through the ABI's from_mont (trh_field_op_dev op 7) and compared cell by cell with a table made here
// from the default selection written out by hand; a step with an opcode the table does not know is refused by its index with the
// destination untouched, and trh_stat reports the steps.  Prints one JSON line; tests/test_gpu_exetable.py runs it.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/trh.hpp"

using namespace trh;

static std::vector<Limbs> canonical(Field f, DeviceBuffer& dev, size_t count) {
    DeviceBuffer plain(count * 32);
    check(trh_field_op_dev((int)f, 7, dev.data(), nullptr, plain.data(), count, nullptr), "from_mont");
    check(trh_stream_synchronize(nullptr), "sync");
    std::vector<Limbs> out(count);
    plain.download(out.data(), count * 32);
    return out;
}

int main() {
    int failed = 0, checks = 0;
    std::printf("{\"test\": \"exetable\"");
    try {
        check(trh_init(0), "trh_init");
        uint64_t x = 0x9e3779b97f4a7c15ull;
        auto next = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
        const uint32_t W = 32, R = 8;
        const size_t m = 700, n = 1024, ncols = exe_columns(R);
        const uint32_t ops[5] = {4, 5, 6, 11, 21};
        std::vector<uint32_t> pc(m), inst(m), a(m), value(m, 0), regs(m * R), bits((m + 31) / 32, 0);
        for (size_t i = 0; i < m; ++i) {
            const bool a_is_reg = (i & 1) != 0;
            const uint32_t op = i + 1 == m ? 31u : ops[next() % 5];
            pc[i] = i ? (uint32_t)next() : 0u;
            a[i] = a_is_reg ? (uint32_t)(next() % R) : (i % 7 == 0 ? (uint32_t)(next() % 40) : (uint32_t)next());
            inst[i] = exe_encode(op, (uint32_t)(next() % R), (uint32_t)(next() % R), a_is_reg);
            for (uint32_t k = 0; k < R; ++k) regs[i * R + k] = i ? (uint32_t)next() : 0u;
            if (i && (next() & 1)) bits[i >> 5] |= 1u << (i & 31);
        }
        // the expected table, the default selection written out: columns of R = 8 by name
        const size_t SA = 10 + R, SB = SA + 2 * R + 3, SC = SB + 2 * R + 5, SD = SC + 2 * R + 2, ND = SD + 2 * R + 4;
        std::vector<std::vector<uint64_t>> want(ncols, std::vector<uint64_t>(n, 0));
        for (size_t i = 0; i < m; ++i) {
            const uint32_t op = inst[i] & 31, ri = (inst[i] >> 8) & 15, rj = (inst[i] >> 12) & 15;
            const bool a_is_reg = (inst[i] >> 16) & 1;
            const uint32_t* now = &regs[i * R];
            const uint64_t A = a_is_reg ? now[a[i]] : a[i], RJ = now[rj];
            const uint64_t pc_next = i + 1 < m ? pc[i + 1] : 0, ri_next = i + 1 < m ? regs[(i + 1) * R + ri] : 0;
            want[0][i] = 1; want[1][i] = pc[i]; want[2][i] = (bits[i >> 5] >> (i & 31)) & 1;
            for (uint32_t k = 0; k < R; ++k) want[3 + k][i] = now[k];
            want[3 + R][i] = op; want[4 + R][i] = a_is_reg ? 0 : a[i]; want[5 + R][i] = 0;
            uint64_t* tv[4] = {&want[6 + R][i], &want[7 + R][i], &want[8 + R][i], &want[9 + R][i]};
            // where operand A's selector stands in a family whose `reg` block starts at reg0 and whose `a` column is a_col
            auto sel_a = [&](size_t reg0, size_t a_col) { want[a_is_reg ? reg0 + a[i] : a_col][i] = 1; };
            const uint64_t s = A < W ? A : W;
            switch (op) {
            case 4:  *tv[0] = A; sel_a(SA + 1, SA + 1 + 2 * R); *tv[1] = RJ; want[SB + 3 + rj][i] = 1; *tv[2] = ri_next; want[SC + R + ri][i] = 1; want[SD + 2 + 2 * R][i] = 1; break;
            case 5:  *tv[0] = A; sel_a(SA + 1, SA + 1 + 2 * R); *tv[1] = ri_next; want[SB + 3 + R + ri][i] = 1; *tv[2] = RJ; want[SC + rj][i] = 1; want[SD + 2 + 2 * R][i] = 1; break;
            case 6:  *tv[0] = A; sel_a(SA + 1, SA + 1 + 2 * R); *tv[1] = RJ; want[SB + 3 + rj][i] = 1; *tv[2] = (RJ * A) >> W; want[ND + 2][i] = 1; *tv[3] = ri_next; want[SD + 1 + R + ri][i] = 1; break;
            case 11: *tv[0] = A; sel_a(SA + 1, SA + 1 + 2 * R); *tv[1] = RJ; want[SB + 3 + rj][i] = 1; *tv[2] = (RJ << s) >> W; want[ND + 2][i] = 1; *tv[3] = ri_next; want[SD + 1 + R + ri][i] = 1; break;
            case 21: *tv[0] = pc_next; want[SA][i] = 1; *tv[1] = A; sel_a(SB + 3, SB + 3 + 2 * R); want[SC + 2 * R + 1][i] = 1; *tv[3] = (uint64_t)pc[i] + 1; want[ND + 3][i] = 1; break;
            default: *tv[0] = A; sel_a(SA + 1, SA + 1 + 2 * R); *tv[1] = pc[i]; want[SB][i] = 1; want[SC + 2 * R + 1][i] = 1; want[SD + 2 + 2 * R][i] = 1; break;
            }
        }
        DeviceBuffer d_pc(4 * m), d_inst(4 * m), d_a(4 * m), d_value(4 * m), d_regs(4 * m * R), d_bits(4 * bits.size());
        d_pc.upload(pc.data(), 4 * m); d_inst.upload(inst.data(), 4 * m); d_a.upload(a.data(), 4 * m); d_value.upload(value.data(), 4 * m);
        d_regs.upload(regs.data(), 4 * m * R); d_bits.upload(bits.data(), 4 * bits.size());
        auto u32p = [](DeviceBuffer& b) { return (const uint32_t*)b.data(); };
        for (Field f : {Field::Fp, Field::Fq}) {
            DeviceBuffer dst(ncols * n * 32);
            exe_table(f, W, R, u32p(d_pc), u32p(d_inst), u32p(d_a), u32p(d_value), u32p(d_regs), u32p(d_bits), m, dst.data(), n);
            const std::vector<Limbs> cells = canonical(f, dst, ncols * n);
            for (size_t c = 0; c < ncols; ++c)
                for (size_t r = 0; r < n; ++r, ++checks)
                    if (cells[c * n + r] != Limbs{want[c][r], 0, 0, 0}) ++failed;
            uint64_t rows = 0;
            check(trh_stat("exetable_rows", &rows), "trh_stat");
            ++checks; if (rows != m) ++failed;
        }
        // an opcode the table does not know: refused by the step's index, the destination as it was
        inst[123] = exe_encode(23, 0, 0, false);
        inst[500] = exe_encode(30, 0, 0, false);
        d_inst.upload(inst.data(), 4 * m);
        const std::vector<uint64_t> sentinel(ncols * n * 4, 0xA5A5A5A5A5A5A5A5ull);
        std::vector<uint64_t> after(sentinel.size());
        DeviceBuffer dst(ncols * n * 32);
        dst.upload(sentinel.data(), ncols * n * 32);
        bool refused = false;
        try { exe_table(Field::Fp, W, R, u32p(d_pc), u32p(d_inst), u32p(d_a), u32p(d_value), u32p(d_regs), u32p(d_bits), m, dst.data(), n); }
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
