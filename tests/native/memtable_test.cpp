// Native test of the memory-consistency table over include/trh.hpp (compiled host, no Python in the process): one trh::mem_table per field
// on a log of 5003 records over 37 addresses and a tape of three words -- past one sort tile and one scan tile -- brought back through the
// ABI's from_mont (trh_field_op_dev op 7) and compared with a table made here by std::stable_sort and a walk down the runs; one wrong load
// is reported, a log with a repeated time and one that is too long are refused.  Prints one JSON line; tests/test_gpu_memtable.py runs it.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/trh.hpp"

using namespace trh;

static const int NCOL = 13;

static std::vector<Limbs> canonical(Field f, DeviceBuffer& dev, size_t count) {
    DeviceBuffer plain(count * 32);
    check(trh_field_op_dev((int)f, 7, dev.data(), nullptr, plain.data(), count, nullptr), "from_mont");
    check(trh_stream_synchronize(nullptr), "sync");
    std::vector<Limbs> out(count);
    plain.download(out.data(), count * 32);
    return out;
}

struct Access { uint32_t address, time, value; bool store; };

int main() {
    int failed = 0, checks = 0;
    std::printf("{\"test\": \"memtable\"");
    try {
        check(trh_init(0), "trh_init");
        uint64_t x = 0x9e3779b97f4a7c15ull;
        auto next = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
        const uint32_t word_bits = 32;
        const std::vector<uint32_t> tape = {7, 0xFFFFFFFFu, 9};  // addresses 0, 4, 8
        std::vector<uint32_t> pool = {0, 4, 5, 0xFFFFFFFFu, 0xFFFFFFFEu, 0x01000000u, 0x00010000u, 0x00000100u};
        while (pool.size() < 37) pool.push_back((uint32_t)next());
        const size_t m = 5003, wrong_at = 4990;
        std::vector<Access> log(m);
        uint32_t now = 0;
        for (size_t i = 0; i < m; ++i) {
            now += 1 + (uint32_t)(next() % 700000);
            log[i] = Access{pool[next() % pool.size()], now, (uint32_t)next(), (next() & 1) != 0};
        }
        // the expected table: records (tape first) stably sorted by address, a walk down the runs
        struct Rec { uint32_t address; long index; };
        std::vector<Rec> recs;
        for (size_t i = 0; i < tape.size(); ++i) recs.push_back(Rec{(uint32_t)(4 * i), -1 - (long)i});
        for (size_t i = 0; i < m; ++i) recs.push_back(Rec{log[i].address, (long)i});
        std::stable_sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) { return a.address < b.address; });
        std::vector<std::vector<uint64_t>> want;
        std::vector<uint32_t> want_src;
        uint64_t prev_run = 0, carried = 0, prev_time = 0, addr_inc = 0;
        bool have_run = false;
        uint32_t run_address = 0;
        auto push = [&](uint32_t address, uint64_t time, int kind, uint64_t time_inc, uint32_t src) {
            want.push_back({1, address, time, (uint64_t)(kind == 0), (uint64_t)(kind == 1), (uint64_t)(kind == 2), carried, addr_inc, time_inc, addr_inc & 0x55555555u,
                            (addr_inc >> 1) & 0x55555555u, time_inc & 0x55555555u, (time_inc >> 1) & 0x55555555u});
            want_src.push_back(src);
        };
        for (const Rec& r : recs) {
            if (!have_run || r.address != run_address) {
                if (have_run) prev_run = run_address;
                have_run = true;
                run_address = r.address;
                addr_inc = (uint64_t)r.address > prev_run ? (uint64_t)r.address - prev_run - 1 : 0;
                carried = r.index < 0 ? tape[-1 - r.index] : 0;
                prev_time = 0;
                push(r.address, 0, 0, 0, 0xFFFFFFFFu);
                if (r.index < 0) continue;
            }
            Access& a = log[r.index];
            if (a.store) carried = a.value;
            else if ((size_t)r.index != wrong_at) a.value = (uint32_t)carried;  // loads claim what the table holds, but one
            else a.value = (uint32_t)carried + 1;
            push(a.address, a.time, a.store ? 1 : 2, a.time - prev_time, (uint32_t)r.index);
            prev_time = a.time;
        }
        const size_t rows = want.size(), n = rows + 9;
        std::vector<uint32_t> address(m), time(m), value(m), bits((m + 31) / 32, 0);
        for (size_t i = 0; i < m; ++i) {
            address[i] = log[i].address; time[i] = log[i].time; value[i] = log[i].value;
            if (log[i].store) bits[i >> 5] |= 1u << (i & 31);
        }
        DeviceBuffer d_address(4 * m), d_time(4 * m), d_value(4 * m), d_bits(4 * bits.size()), d_tape(4 * tape.size()), d_src(4 * n);
        d_address.upload(address.data(), 4 * m); d_value.upload(value.data(), 4 * m); d_bits.upload(bits.data(), 4 * bits.size());
        d_time.upload(time.data(), 4 * m); d_tape.upload(tape.data(), 4 * tape.size());
        for (Field f : {Field::Fp, Field::Fq}) {
            DeviceBuffer dst(NCOL * n * 32);
            const MemTableResult got = mem_table(f, word_bits, (const uint32_t*)d_address.data(), (const uint32_t*)d_time.data(), (const uint32_t*)d_value.data(),
                                                 (const uint32_t*)d_bits.data(), m, (const uint32_t*)d_tape.data(), tape.size(), dst.data(), n, n, (uint32_t*)d_src.data());
            ++checks; if (got.rows != rows) ++failed;
            ++checks; if (got.n_inconsistent != (log[wrong_at].store ? 0u : 1u) || got.first_inconsistent != (log[wrong_at].store ? m : wrong_at)) ++failed;
            const std::vector<Limbs> cells = canonical(f, dst, NCOL * n);
            for (int c = 0; c < NCOL; ++c)
                for (size_t r = 0; r < n; ++r, ++checks)
                    if (cells[c * n + r] != Limbs{r < rows ? want[r][c] : 0, 0, 0, 0}) ++failed;
            std::vector<uint32_t> src(n);
            d_src.download(src.data(), 4 * n);
            for (size_t r = 0; r < n; ++r, ++checks) if (src[r] != (r < rows ? want_src[r] : 0xFFFFFFFFu)) ++failed;
            // one row too many for max_rows: refused with the rows reported
            trh_mem_table_args_t a{word_bits, (const uint32_t*)d_address.data(), (const uint32_t*)d_time.data(), (const uint32_t*)d_value.data(), (const uint32_t*)d_bits.data(), m,
                                   (const uint32_t*)d_tape.data(), tape.size(), dst.data(), n, rows - 1, nullptr, nullptr, 0, 0, 0};
            ++checks; if (trh_mem_table_dev((int)f, &a) != TRH_EINVAL || a.rows != rows) ++failed;
        }
        // a repeated time: the log is refused at that index
        time[4000] = time[3999];
        d_time.upload(time.data(), 4 * m);
        DeviceBuffer dst(NCOL * n * 32);
        trh_mem_table_args_t a{word_bits, (const uint32_t*)d_address.data(), (const uint32_t*)d_time.data(), (const uint32_t*)d_value.data(), (const uint32_t*)d_bits.data(), m,
                               (const uint32_t*)d_tape.data(), tape.size(), dst.data(), n, n, nullptr, nullptr, 0, 0, 0};
        ++checks; if (trh_mem_table_dev((int)Field::Fp, &a) != TRH_EINVAL || !std::strstr(trh_last_error(), "record 4000 ")) ++failed;
        trh_shutdown();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        ++failed;
    }
    std::printf(", \"checks\": %d, \"checks_failed\": %d}\n", checks, failed);
    return failed ? 1 : 0;
}
