"""GPU tests (-m gpu) of the lookup permutation (csrc/lookup.hip) past one scan block and one 32-lookup chunk: the cases of
tests/lookup_cases.py through permutation.lookup_permute / lookup_permute_batch, A' and S' compared word for word with the step-by-step
oracle (oracle/pasta.py::permute_expression_pair).  What each case reaches -- the carries of radix_scan_kernel and scan_sums_kernel at
526 337 rows, the chunk offsets at 67 lookups, the identity steps and the trimmed masks of the sort, ties in one column only, both miss
branches, the order in which failures are reported -- is asserted without a GPU by tests/test_lookup_cases.py.

A wrong carry or chunk offset gives columns that are still permutations and often still sorted: only the bit-exact comparison sees it."""
import functools

import numpy as np
import pytest
import torch

import cpu_ref
import lookup_cases as lc
import pasta as o
from tiny_ram_halo2_amd import api, permutation

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


def mont(field, vals):
    """canonical integers -> (len, 4) uint64 Montgomery limbs, through the C++ oracle (a list comprehension over f.limbs takes seconds at 2^19)"""
    raw = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4)
    out = cpu_ref.field_op(field, "to_mont", raw)
    assert not len(vals) or out[0].tolist() == o.FIELDS[field].limbs(vals[0])
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.contiguous().cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def prepared(name):
    """(case, inputs (batch, rows, 4), tables, wanted A' (batch, usable_rows, 4) or None, wanted S'): built once, shared, never written to"""
    c = lc.case(name)
    want, _ = lc.expected(name)
    inputs = np.stack([mont(c.field, col) for col in c.inputs])
    tables = np.stack([mont(c.field, col) for col in c.tables])
    if want is None:
        return c, inputs, tables, None, None
    return c, inputs, tables, np.stack([mont(c.field, a) for a, _ in want]), np.stack([mont(c.field, s) for _, s in want])


def run(name):
    """the case on the device -> (A', S') as (batch, usable_rows, 4) host arrays; a batch call's rows behind usable_rows must be zero"""
    c, inputs, tables, _, _ = prepared(name)
    n = c.usable_rows
    if c.call == "single":
        a, s = permutation.lookup_permute(c.field, dev(inputs[0]), dev(tables[0]), n)
        a, s = host(a)[None], host(s)[None]
        assert a.shape == s.shape == (1, n, 4)
        return a, s
    a, s = permutation.lookup_permute_batch(c.field, dev(inputs), dev(tables), n)
    a, s = host(a), host(s)
    assert a.shape == s.shape == inputs.shape
    assert not a[:, n:].any() and not s[:, n:].any()
    return a[:, :n], s[:, :n]


def first_bad(got, want):
    bad = np.argwhere(~(got == want).all(axis=-1))
    return None if not bad.size else {"lookup": int(bad[0][0]), "row": int(bad[0][1]), "tile": int(bad[0][1]) // lc.TILE}


def check(name):
    _, _, _, want_a, want_s = prepared(name)
    a, s = run(name)
    assert first_bad(a, want_a) is None, ("A'", name, first_bad(a, want_a))
    assert first_bad(s, want_s) is None, ("S'", name, first_bad(s, want_s))
    return a, s


FAILING = [nm for nm in lc.NAMES if nm.startswith(("missing-order-", "input-only-tie-")) or (nm.startswith("missing-") and not nm.endswith("-input-tail"))]
GOOD_SMALL = [nm for nm in lc.NAMES if nm not in FAILING and nm not in ("big", "chunks")]
AFTER_ERROR = "sizes-fp-2049-wide"  # the good call that follows a failing one


def test_case_lists_cover_every_case():
    assert sorted(GOOD_SMALL + FAILING + ["big", "chunks"]) == sorted(lc.NAMES)
    assert all(lc.case(nm).error is None for nm in GOOD_SMALL) and all(lc.case(nm).error is not None for nm in FAILING)
    assert len(FAILING) == 2 * 4 + 2 + 4 and AFTER_ERROR in GOOD_SMALL


@pytest.mark.parametrize("name", GOOD_SMALL)
def test_small_cases_match_oracle(name):
    """tile edges (2047 .. 4097 rows), no repeated row at all, columns that vary in some limbs only, sparse and trimmed key masks, a tie in the
    table column alone, a stray input value behind usable_rows"""
    check(name)


def test_big_matches_oracle():
    """526 337 rows, three lookups: the smallest size at which radix_scan_kernel and scan_sums_kernel both carry between blocks"""
    check("big")


def test_chunks_match_oracle():
    """67 lookups in one call: three chunks, ties redone at the chunk edges"""
    check("chunks")


@pytest.mark.parametrize("name", FAILING)
def test_missing_value_names_first_lookup(name):
    """a call with an input value missing from its table fails and names the first such lookup of the call, whichever way each is found
    (first pass, or the redo of a tied lookup), in whichever chunk; the next call in the same process is not affected"""
    c = lc.case(name)
    with pytest.raises(api.TrhError, match=rf"lookup {c.error}\b"):
        run(name)
    check(AFTER_ERROR)


def test_scratch_reuse_across_sizes():
    """one context, in this order: 67 x 2349 rows, 3 x 526 337, one lookup of 7 rows, 67 x 2349 again -- every call after the first finds the
    histogram, tile sums, pass sides and row lists of a call of another shape in the scratch"""
    first_a, first_s = check("chunks")
    check("big")
    f = o.FIELDS["fq"]
    inp, table = [3, 1, 3, 3, 2, 1, 1], [1, 2, 3, 9, 9, 1, 4]
    want_a, want_s = o.permute_expression_pair(inp, table, 7)
    a, s = permutation.lookup_permute("fq", dev(mont("fq", inp)), dev(mont("fq", table)))
    assert [f.from_limbs(r) for r in host(a)] == want_a and [f.from_limbs(r) for r in host(s)] == want_s
    again_a, again_s = check("chunks")
    assert (again_a == first_a).all() and (again_s == first_s).all()


def test_entry_refusals():
    """trh_lookup_permute_batch_dev refuses, before any launch: outputs that alias the inputs or each other, a row stride below usable_rows,
    usable_rows >= 2^31, null pointers, an unknown field; and returns TRH_OK without touching the outputs for usable_rows = 0 or batch = 0"""
    lib = api.lib()
    _, inputs, tables, want_a, want_s = prepared(AFTER_ERROR)
    n = inputs.shape[1]
    d_in, d_tab = dev(inputs[0]), dev(tables[0])
    sentinel = 0x5A5A5A5A5A5A5A5A
    out_a, out_s = torch.full_like(d_in, sentinel), torch.full_like(d_in, sentinel)
    p = api._devptr
    call = lambda field, i, t, usable, stride, batch, oa, os_: lib.trh_lookup_permute_batch_dev(field, i, t, usable, stride, batch, oa, os_, None)  # noqa: E731
    EINVAL = -1
    refused = [
        ("alias", (api.FP, p(d_in), p(d_tab), n, n, 1, p(d_in), p(out_s))),
        ("alias", (api.FP, p(d_in), p(d_tab), n, n, 1, p(out_a), p(d_tab))),
        ("alias", (api.FP, p(d_in), p(d_tab), n, n, 1, p(out_a), p(out_a))),
        ("stride", (api.FP, p(d_in), p(d_tab), n, n - 1, 1, p(out_a), p(out_s))),
        ("stride", (api.FP, p(d_in), p(d_tab), 1 << 31, 1 << 31, 1, p(out_a), p(out_s))),
        ("null pointer", (api.FP, None, p(d_tab), n, n, 1, p(out_a), p(out_s))),
        ("null pointer", (api.FP, p(d_in), p(d_tab), n, n, 1, p(out_a), None)),
        ("unknown field", (7, p(d_in), p(d_tab), n, n, 1, p(out_a), p(out_s))),
    ]
    for text, args in refused:
        assert call(*args) == EINVAL, args
        assert text in lib.trh_last_error().decode(), (text, lib.trh_last_error())
    assert lib.trh_lookup_permute_dev(api.FP, p(d_in), p(d_tab), n, p(d_in), p(out_s), None) == EINVAL
    # nothing to do: TRH_OK, the outputs as they were (2^31 - 1 rows pass the range check; with batch = 0 nothing is read)
    for usable, stride, batch in ((0, n, 1), (n, n, 0), (0, 0, 0), ((1 << 31) - 1, 1 << 31, 0)):
        assert call(api.FP, p(d_in), p(d_tab), usable, stride, batch, p(out_a), p(out_s)) == 0
    torch.cuda.synchronize()
    assert bool((out_a == sentinel).all()) and bool((out_s == sentinel).all())
    # and the entry still works on the same buffers
    assert call(api.FP, p(d_in), p(d_tab), n, n, 1, p(out_a), p(out_s)) == 0
    assert (host(out_a) == want_a[0]).all() and (host(out_s) == want_s[0]).all()
