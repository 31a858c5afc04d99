// The permutation argument's keygen assembly on the host: which cell every cell of the equality-enabled columns maps to after the circuit's
// copy constraints.  A restatement of halo2_proofs 0.2.0 plonk/permutation/keygen.rs `Assembly` { mapping, aux, sizes } and its `copy`.
// [UPSTREAM-RECALL]: the crate's source is not at hand; the algorithm below is written from memory of that file (and of the book's
// design/permutation.md, which it cites) and is checked by tests/test_permkeygen_host.py against an independent statement of what it must
// produce -- the cycles of the mapping are the connected components of the copy graph -- besides a line-by-line Python model.
//
// A cell is ONE u32: cell = column * n + row, n = 2^k, where upstream keeps (column, row) pairs.  `mapping` is the permutation itself
// (sigma column c, row r holds delta^(m / n) omega^(m % n) for m = mapping[c * n + r]; permutation.hip), `aux` names the representative
// of the cycle a cell belongs to and `sizes` holds, at a representative, the length of its cycle.  copy() merges the smaller cycle into the
// larger (a tie keeps the left one) and then swaps the mapping of the caller's two cells -- the order of the merges decides the mapping, the
// mapping decides the sigma commitments of the verifying key, so none of this is free to differ from upstream.
// Plain C++17, no HIP: tests/native/permkeygen_test.cpp compiles it alone, under the address and undefined-behaviour sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <new>
#include <utility>
#include <vector>

#include "../../include/trh.h"

namespace trh {

struct PermAssembly {
    uint32_t n_columns = 0, k = 0;
    size_t n = 0, cells = 0;
    std::vector<uint32_t> mapping, aux, sizes;

    // a cell index must fit a u32: n_columns * 2^k <= 2^32
    static bool shape_ok(uint32_t n_columns, uint32_t k) { return n_columns != 0 && k <= 27 && (uint64_t)n_columns << k <= (uint64_t)1 << 32; }

    int init(uint32_t columns, uint32_t log_n) {
        if (!shape_ok(columns, log_n)) return TRH_EINVAL;
        n_columns = columns; k = log_n;
        n = (size_t)1 << k;
        cells = (size_t)columns << k;
        try {
            mapping.resize(cells); aux.resize(cells);
            sizes.assign(cells, 1u);
        } catch (const std::bad_alloc&) {
            return TRH_ENOMEM;
        }
        for (size_t i = 0; i < cells; ++i) mapping[i] = aux[i] = (uint32_t)i;
        return TRH_OK;
    }

    bool in_range(uint32_t column, uint32_t row) const { return column < n_columns && row < n; }
    uint32_t cell(uint32_t column, uint32_t row) const { return (uint32_t)(((size_t)column << k) + row); }

    // Assembly::copy.  An out-of-range cell is refused before anything is touched (upstream: Error::BoundsFailure).
    int copy(uint32_t left_column, uint32_t left_row, uint32_t right_column, uint32_t right_row) {
        if (!in_range(left_column, left_row) || !in_range(right_column, right_row)) return TRH_EINVAL;
        const uint32_t left = cell(left_column, left_row), right = cell(right_column, right_row);
        uint32_t lc = aux[left], rc = aux[right];
        if (lc == rc) return TRH_OK;  // already in one cycle: a self-copy, a repeated copy
        if (sizes[lc] < sizes[rc]) std::swap(lc, rc);
        sizes[lc] += sizes[rc];  // 2^32 cells in one cycle wrap this to 0, and no merge can follow that one
        uint32_t i = rc;
        do {
            aux[i] = lc;
            i = mapping[i];
        } while (i != rc);
        std::swap(mapping[left], mapping[right]);  // the caller's two cells, not the representatives
        return TRH_OK;
    }
};

}  // namespace trh
