"""The permutation and lookup terms of the quotient's numerator on resident extended columns (csrc/quotient.hip, trh_quotient_*): what
halo2_proofs 0.2.0 plonk/permutation/prover.rs `Committed::construct` and plonk/lookup/prover.rs `Committed::construct` contribute to h(X)
in `plonk::create_proof`, folded with the challenge y behind the custom gates (expr.GateEvaluator):

    QuotientTerms(domain, n_perm_columns, chunk_len, n_lookups, blinding_factors)
        .eval(acc, values, sigmas, zs, lookups, l0, l_blind, l_last, beta, gamma, y, n_blocks=None)
    lagrange_basis_columns(domain, blinding_factors, n_blocks=None)      keygen_pk's l0 / l_blind / l_last on the extended domain

Columns are device tensors in either layout of the extended domain: (2^extended_k, 4), or (n_blocks, 2^k, 4) coset blocks
(EvaluationDomain.coeff_to_extended_blocks)."""
from __future__ import annotations

import ctypes

import numpy as np

from . import api
from .poly import EvaluationDomain, _mont


def lagrange_basis_columns(domain: EvaluationDomain, blinding_factors: int, n_blocks: int | None = None):
    """keygen_pk's l0, l_blind, l_last (plonk/keygen.rs): the Lagrange basis polynomial of row 0, the sum of those of the blinding_factors
    rows behind the last usable one, and that of row n - (blinding_factors + 1), as device tensors on the extended domain: (3, 2^extended_k, 4),
    or (3, n_blocks, 2^k, 4) coset blocks.  Order: l0, l_blind, l_last"""
    import torch
    n = domain.n
    u = n - (blinding_factors + 1)
    assert blinding_factors + 2 <= n
    one = _mont(domain.field, 1)
    cols = np.zeros((3, n, 4), dtype=np.uint64)
    cols[0, 0] = one
    cols[1, u + 1:] = one
    cols[2, u] = one
    dev = torch.device("cuda", max(int(api.lib().trh_ctx_device(None)), 0))
    coeff = domain.lagrange_to_coeff(torch.from_numpy(cols.view(np.int64)).to(dev))
    return domain.coeff_to_extended(coeff) if not n_blocks else domain.coeff_to_extended_blocks(coeff, n_blocks)


class QuotientTerms:
    """the shape of the two arguments, resident on the device: n_perm_columns equality-enabled columns in sets of chunk_len (one product
    column each), n_lookups lookups of five columns (A, S, A', S', z)"""

    def __init__(self, domain: EvaluationDomain, n_perm_columns: int, chunk_len: int, n_lookups: int, blinding_factors: int):
        for v in (n_perm_columns, chunk_len, n_lookups, blinding_factors):
            if not 0 <= v < 1 << 32:
                raise api.TrhError(f"QuotientTerms: {v} does not fit the entry's 32-bit counts")
        self.domain, self.n_perm_columns, self.chunk_len, self.n_lookups, self.blinding_factors = domain, n_perm_columns, chunk_len, n_lookups, blinding_factors
        self.handle = api._vp()
        api._check(api.lib().trh_quotient_create(domain.handle(), n_perm_columns, chunk_len, n_lookups, blinding_factors, ctypes.byref(self.handle)))
        self.n_sets = -(-n_perm_columns // chunk_len)

    def rows(self, n_blocks: int | None = None) -> int:
        return n_blocks << self.domain.k if n_blocks else 1 << self.domain.extended_k

    def eval(self, acc, values, sigmas, zs, lookups, l0, l_blind, l_last, beta: int, gamma: int, y: int, n_blocks: int | None = None, stream=None):
        """acc: device tensor with the fold so far (the gates' output for the same y, or zeros), overwritten with acc * y + t over every
        term t; values / sigmas: n_perm_columns columns each, zs: one per set, lookups: n_lookups sequences (A, S, A', S', z).  beta, gamma,
        y: integers.  n_blocks: None or 0 for the flat layout.  Returns acc, complete (the entry synchronises the stream)"""
        import torch
        rows = self.rows(n_blocks)
        flat_lookups = [c for l in lookups for c in l]
        assert len(values) == self.n_perm_columns and len(sigmas) == self.n_perm_columns and len(zs) == self.n_sets and len(flat_lookups) == 5 * self.n_lookups
        for t in list(values) + list(sigmas) + list(zs) + flat_lookups + [l0, l_blind, l_last, acc]:
            assert t.is_contiguous() and t.numel() == rows * 4, "a column of another layout"

        def table(cols):
            return (ctypes.c_void_p * max(1, len(cols)))(*[t.data_ptr() for t in cols])
        tv, ts, tz, tl = table(values), table(sigmas), table(zs), table(flat_lookups)
        field = self.domain.field
        a = api.QuotientArgs()
        a.perm_values, a.perm_sigmas, a.perm_z, a.lookups = tv, ts, tz, tl
        a.l0, a.l_blind, a.l_last, a.acc = l0.data_ptr(), l_blind.data_ptr(), l_last.data_ptr(), acc.data_ptr()
        a.beta[:], a.gamma[:], a.y[:] = [[int(w) for w in _mont(field, v)] for v in (beta, gamma, y)]
        a.n_blocks = n_blocks or 0
        a.stream = stream if stream is not None else torch.cuda.current_stream(acc.device).cuda_stream
        api._check(api.lib().trh_quotient_terms_dev(self.handle, ctypes.byref(a)))
        return acc

    def destroy(self):
        if self.handle:
            api.lib().trh_quotient_destroy(self.handle)
            self.handle = api._vp()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
