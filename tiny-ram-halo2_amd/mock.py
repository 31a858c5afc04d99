"""halo2_proofs 0.2.0 `dev::MockProver::verify` for a witness that is resident on the device: which gate, which row, which lookup.

The reference develops its circuit almost entirely against MockProver (SURVEY.md sections 3.3 / 4).  verify has three parts, and each is one
device check here, none of which writes anything the size of a column back to the host:

    gates        every gate polynomial is zero on every usable row       expr.GateEvaluator.check   (trh_expr_check_dev)
    lookups      every input tuple occurs among its table's rows         lookup_check               (trh_lookup_check_dev)
    permutation  the copy constraints hold                               permutation.Assembly.check (trh_perm_check_dev)

The gate and lookup checks return a bitmap of bad rows per polynomial / lookup; `decode_failures` turns bitmaps into failure records and is a
pure function of host arrays.  Columns are plain values: cell poisoning and CellNotAssigned (region bookkeeping of the Rust host) are not
modelled.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import api, expr


@dataclass(frozen=True)
class ConstraintNotSatisfied:
    """VerifyFailure::ConstraintNotSatisfied: polynomial `poly_index` of gate `gate_index` is non-zero on `row`"""
    gate_index: int
    poly_index: int
    name: str
    row: int


@dataclass(frozen=True)
class Lookup:
    """VerifyFailure::Lookup: the input tuple of `row` is not among the table's rows"""
    lookup_index: int
    name: str
    row: int


@dataclass(frozen=True)
class Permutation:
    """VerifyFailure::Permutation, summarised: `n_bad` cells differ from the cell they map to, the smallest is cell = (column, row) -- column
    counted among the assembly's columns"""
    cell: tuple
    n_bad: int


def bitmap_rows(words, limit: int | None = None) -> list:
    """the set bits of a bitmap (u64 words, bit r % 64 of word r // 64 stands for row r) as ascending row numbers, at most `limit` of them"""
    w = np.ascontiguousarray(words).reshape(-1).view(np.uint64).astype("<u8")
    rows = np.flatnonzero(np.unpackbits(w.view(np.uint8), bitorder="little"))
    return [int(r) for r in (rows if limit is None else rows[:max(limit, 0)])]


def decode_failures(gate_polys, gate_bitmaps, lookup_names, lookup_bitmaps, max_failures: int = 64) -> list:
    """Bitmaps -> failure records.  gate_polys: (gate_index, poly_index, name) per output of the gate program, gate_bitmaps: one row of
    words per output (or None where nothing failed); lookup_names / lookup_bitmaps: the same per lookup.  The records are ordered as
    MockProver orders them -- ConstraintNotSatisfied by (gate, poly, row), then Lookup by (lookup, row) -- and at most max_failures of
    them are made: a broken selector fails every row of every polynomial"""
    out = []
    for (gate_index, poly_index, name), words in sorted(zip(gate_polys, gate_bitmaps), key=lambda t: t[0][:2]):
        if words is None or len(out) >= max_failures:
            continue
        out += [ConstraintNotSatisfied(gate_index, poly_index, name, r) for r in bitmap_rows(words, max_failures - len(out))]
    for li, (name, words) in enumerate(zip(lookup_names, lookup_bitmaps)):
        if words is None or len(out) >= max_failures:
            continue
        out += [Lookup(li, name, r) for r in bitmap_rows(words, max_failures - len(out))]
    return out


def lookup_check(field: str, inputs, tables, usable_rows: int, bitmap: bool = False):
    """The lookup part of MockProver::verify (trh_lookup_check_dev): inputs / tables are equally long lists of 1 .. 16 device columns
    (rows, 4) with rows >= usable_rows; input row r < usable_rows is bad when its tuple of elements equals the tuple of no table row
    t < usable_rows (exact membership, not the theta compression).  Returns (n_bad, first_bad_row) -- first_bad_row = usable_rows when
    there is none -- and, with bitmap=True, a device tensor of ceil(usable_rows / 64) int64 words, one bit per row.  Takes no stream: see
    GateEvaluator.check"""
    import torch
    width = len(inputs)
    assert width == len(tables) and width >= 1
    for t in list(inputs) + list(tables):
        assert t.is_contiguous() and t.shape[-1] == 4 and t.shape[-2] >= usable_rows
    in_ptrs = (ctypes.c_void_p * width)(*[t.data_ptr() for t in inputs])
    tab_ptrs = (ctypes.c_void_p * width)(*[t.data_ptr() for t in tables])
    n_bad, first_bad = ctypes.c_uint64(0), ctypes.c_uint64(0)
    words = torch.empty(((usable_rows + 63) // 64,), dtype=torch.int64, device=inputs[0].device) if bitmap else None
    api._check(api.lib().trh_lookup_check_dev(api.FIELD_ID[field], in_ptrs, tab_ptrs, width, usable_rows, ctypes.byref(n_bad), ctypes.byref(first_bad),
                                              words.data_ptr() if bitmap else None))
    return (int(n_bad.value), int(first_bad.value), words) if bitmap else (int(n_bad.value), int(first_bad.value))


class MockProver:
    """MockProver::verify over device columns.

    field, k, usable_rows: the circuit's field, its 2^k rows and how many of them are usable (the rest are blinding rows: they are read
    through rotations only);
    gates: [(name, [Expression, ...])] -- every polynomial must vanish on every usable row;
    lookups: [(name, [input Expression, ...], [table Expression, ...])];
    permutation, permutation_columns: a permutation.Assembly and the (kind, column) key of each of its columns, in its column order.
    Everything is compiled once: one program with one output per gate polynomial, and one per lookup whose outputs are the input
    expressions followed by the table expressions."""

    def __init__(self, field: str, k: int, usable_rows: int, gates=(), lookups=(), permutation=None, permutation_columns=None):
        assert 1 <= usable_rows <= 1 << k
        self.field, self.k, self.n, self.usable_rows = field, k, 1 << k, usable_rows
        self.gate_polys = [(gi, pi, name) for gi, (name, polys) in enumerate(gates) for pi in range(len(polys))]
        flat = [p for _, polys in gates for p in polys]
        self.gate_ev = expr.GateEvaluator(expr.compile_outputs(field, flat), n_outputs=len(flat)) if flat else None
        self.lookup_names, self.lookup_ev = [], []
        for name, inputs, tables in lookups:
            assert len(inputs) == len(tables) and 1 <= len(inputs) <= 16, name
            self.lookup_names.append(name)
            self.lookup_ev.append(expr.GateEvaluator(expr.compile_outputs(field, list(inputs) + list(tables)), n_outputs=2 * len(inputs)))
        assert (permutation is None) == (permutation_columns is None)
        if permutation is not None:
            assert permutation.k == k and permutation.field == field and len(permutation_columns) == permutation.n_columns
        self.permutation, self.permutation_columns = permutation, permutation_columns

    def verify(self, columns: dict, max_failures: int = 64) -> list:
        """columns: {(kind, column): device tensor (2^k, 4)}.  Returns the failure records: ConstraintNotSatisfied ordered by (gate, poly,
        row), then Lookup by (lookup, row) -- max_failures caps these two kinds together -- then one Permutation record when a copy
        constraint is broken.  An empty list: the witness satisfies the system"""
        gate_bitmaps = [None] * len(self.gate_polys)
        if self.gate_ev is not None:
            cols = {key: columns[key] for key in self.gate_ev.program.columns}
            n_bad, _, words = self.gate_ev.check(cols, self.k, self.usable_rows, bitmap=True)
            if n_bad.any():
                host = words.cpu().numpy()
                gate_bitmaps = [host[a] if n_bad[a] else None for a in range(len(self.gate_polys))]
        lookup_bitmaps = []
        for ev in self.lookup_ev:
            width = ev.n_outputs // 2
            values = ev.eval({key: columns[key] for key in ev.program.columns}, self.k, 1).reshape(2 * width, self.n, 4)
            n_bad, _, words = lookup_check(self.field, [values[j] for j in range(width)], [values[width + j] for j in range(width)], self.usable_rows, bitmap=True)
            lookup_bitmaps.append(words.cpu().numpy() if n_bad else None)
        out = decode_failures(self.gate_polys, gate_bitmaps, self.lookup_names, lookup_bitmaps, max_failures)
        if self.permutation is not None:
            n_bad, first = self.permutation.check([columns[key] for key in self.permutation_columns])
            if n_bad:
                out.append(Permutation(first, n_bad))
        return out
