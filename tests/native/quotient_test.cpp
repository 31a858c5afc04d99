// Native test of trh::QuotientTerms over include/trh.hpp (compiled host, no Python in the process).  tests/test_gpu_quotient.py writes the
// input file, runs this program and compares the output file with its model bit for bit.
//   input   eight u32: field (0 fp, 1 fq), j, k, n_perm_columns, chunk_len, n_lookups, blinding_factors, n_blocks (0: flat layout);
//           beta, gamma, y (32 bytes each, Montgomery); then the columns, rows x 32 bytes each (rows = 2^extended_k or n_blocks 2^k):
//           values, sigmas, the product columns, the lookups' A, S, A', S', z, then l0, l_blind, l_last and the starting acc
//   output  acc after the terms, rows x 32 bytes
//   usage: quotient_test <input> <output>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/trh.hpp"

using namespace trh;

int main(int argc, char** argv) {
    int failed = 0;
    try {
        require(argc == 3, "usage: quotient_test <input> <output>");
        FILE* in = std::fopen(argv[1], "rb");
        require(in != nullptr, "cannot open the input file");
        uint32_t h[8];
        Limbs ch[3];
        require(std::fread(h, 4, 8, in) == 8 && std::fread(ch, 32, 3, in) == 3, "short header");
        const uint32_t j = h[1], k = h[2], n_columns = h[3], chunk_len = h[4], n_lookups = h[5], blinding = h[6], n_blocks = h[7];
        require(h[0] <= 1 && j >= 2 && j <= 9 && k <= 12 && n_columns <= 64 && chunk_len >= 1 && n_lookups <= 16, "header out of the test's range");
        check(trh_init(0), "trh_init");
        {
            EvaluationDomain dom(h[0] == 0 ? Field::Fp : Field::Fq, j, k);
            require(n_blocks <= (1u << (dom.extended_k - k)), "n_blocks beyond the extended domain");
            const size_t rows = n_blocks ? (size_t)n_blocks << k : dom.extended_len();
            QuotientTerms terms(dom, n_columns, chunk_len, n_lookups, blinding);
            const size_t n_in = 2 * (size_t)n_columns + terms.n_sets() + 5 * (size_t)n_lookups + 3;
            std::vector<std::unique_ptr<DeviceBuffer>> cols;
            std::vector<Limbs> buf(rows);
            for (size_t c = 0; c < n_in + 1; ++c) {
                require(std::fread(buf.data(), 32, rows, in) == rows, "short column");
                cols.emplace_back(new DeviceBuffer(rows * 32));
                cols.back()->upload(buf.data(), rows * 32);
            }
            std::fclose(in);
            QuotientTerms::Columns q;
            size_t at = 0;
            for (uint32_t c = 0; c < n_columns; ++c) q.values.push_back(cols[at++]->data());
            for (uint32_t c = 0; c < n_columns; ++c) q.sigmas.push_back(cols[at++]->data());
            for (size_t c = 0; c < terms.n_sets(); ++c) q.zs.push_back(cols[at++]->data());
            for (size_t c = 0; c < 5 * (size_t)n_lookups; ++c) q.lookups.push_back(cols[at++]->data());
            q.l0 = cols[at++]->data(); q.l_blind = cols[at++]->data(); q.l_last = cols[at++]->data();
            DeviceBuffer& acc = *cols[at];
            terms.eval(acc.data(), q, ch[0], ch[1], ch[2], n_blocks);
            bool refused = false;  // a wrong number of columns is refused by the wrapper, acc as an input by the library
            try { QuotientTerms::Columns bad = q; bad.l0 = acc.data(); terms.eval(acc.data(), bad, ch[0], ch[1], ch[2], n_blocks); } catch (const Error&) { refused = true; }
            if (!refused) ++failed;
            acc.download(buf.data(), rows * 32);
            FILE* out = std::fopen(argv[2], "wb");
            require(out != nullptr, "cannot open the output file");
            require(std::fwrite(buf.data(), 32, rows, out) == rows, "short write");
            std::fclose(out);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        ++failed;
    }
    trh_shutdown();
    std::printf("{\"test\": \"quotient_terms\", \"checks_failed\": %d}\n", failed);
    return failed ? 1 : 0;
}
