// Host test of csrc/tuplehash.h (the set behind trh_lookup_check_dev), compiled with address + undefined sanitizers: builds the set
// sequentially with the header's own insert and probe code -- the code the device kernels run -- over the cases tests/test_mock_host.py
// wrote, and prints one JSON line per case: the verdict (bad rows, smallest bad row, the bitmap as hex words), the slots visited by all
// inserts and probes, whether that total is within 4 * (table rows + input rows), and how many rows disagree with a std::set of the table's
// tuples.  The Python side compares the verdict with its own model.
//   file (binary, little endian u64): width, usable_rows, rows; then `width` input columns and `width` table columns of rows x 4 u64
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "../../tiny-ram-halo2_amd/csrc/tuplehash.h"

using namespace trh::tuplehash;

static int run(const char* path) {
    FILE* in = std::fopen(path, "rb");
    if (!in) { std::fprintf(stderr, "%s does not open\n", path); return 1; }
    uint64_t head[3];
    if (std::fread(head, 8, 3, in) != 3) { std::fprintf(stderr, "%s: header\n", path); return 1; }
    const uint32_t width = (uint32_t)head[0];
    const size_t usable = (size_t)head[1], rows = (size_t)head[2];
    if (width == 0 || width > MAX_WIDTH || usable == 0 || usable > rows) { std::fprintf(stderr, "%s: bad shape\n", path); return 1; }
    std::vector<std::vector<Words8>> cols(2 * width, std::vector<Words8>(rows));
    for (auto& c : cols)
        if (std::fread(c.data(), sizeof(Words8), rows, in) != rows) { std::fprintf(stderr, "%s: short column\n", path); return 1; }
    std::fclose(in);
    std::vector<const void*> ptrs;
    for (auto& c : cols) ptrs.push_back(c.data());
    const void* const* inputs = ptrs.data();
    const void* const* tables = ptrs.data() + width;

    const uint64_t capacity = capacity_for(usable);
    std::vector<uint32_t> slots(capacity, EMPTY);
    uint64_t probes = 0;
    auto claim = [](uint32_t* slot, uint32_t row) { const uint32_t seen = *slot; if (seen == EMPTY) *slot = row; return seen; };
    for (size_t t = 0; t < usable; ++t) probes += insert_row(slots.data(), capacity, tables, width, (uint32_t)t, claim);

    auto tuple_of = [&](const void* const* c, size_t r) {
        std::vector<uint32_t> t;
        for (uint32_t j = 0; j < width; ++j) { const Words8 e = load_elem(c[j], r); t.insert(t.end(), e.w, e.w + 8); }
        return t;
    };
    std::set<std::vector<uint32_t>> reference;
    for (size_t t = 0; t < usable; ++t) reference.insert(tuple_of(tables, t));

    std::vector<uint64_t> bitmap((usable + 63) / 64, 0);
    uint64_t n_bad = 0, first_bad = usable, mismatches = 0;
    for (size_t r = 0; r < usable; ++r) {
        uint32_t visited = 0;
        const bool found = probe_row(slots.data(), capacity, inputs, tables, width, r, &visited);
        probes += visited;
        if (found != (reference.count(tuple_of(inputs, r)) != 0)) ++mismatches;
        if (!found) {
            bitmap[r / 64] |= (uint64_t)1 << (r % 64);
            if (!n_bad) first_bad = r;
            ++n_bad;
        }
    }
    const bool within = probes <= 4 * (uint64_t)(usable + usable);
    std::printf("{\"width\": %u, \"usable_rows\": %zu, \"n_bad\": %llu, \"first_bad_row\": %llu, \"probes\": %llu, \"within_cap\": %s, \"set_mismatches\": %llu, \"bitmap\": \"",
                width, usable, (unsigned long long)n_bad, (unsigned long long)first_bad, (unsigned long long)probes, within ? "true" : "false", (unsigned long long)mismatches);
    for (uint64_t w : bitmap) std::printf("%016llx", (unsigned long long)w);
    std::printf("\"}\n");
    return (within && mismatches == 0) ? 0 : 1;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: tuplehash_test <case file>...\n"); return 2; }
    int failed = 0;
    for (int i = 1; i < argc; ++i) failed += run(argv[i]);
    return failed ? 1 : 0;
}
