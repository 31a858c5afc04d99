"""The cases of tests/lookup_cases.py, without a GPU: the oracle (oracle/pasta.py::permute_expression_pair) accepts or refuses each as the
case says, its result satisfies the constraints that define the lookup argument's permuted columns, and every case reaches the part of
csrc/lookup.hip it was written for -- computed here from the rules that file documents (lookup_cases.varies / fast_key / tied), so that
tests/test_gpu_lookup_sizes.py cannot pass without having gone there."""
import bisect
from collections import Counter

import pytest

import lookup_cases as lc


def columns(c, l):
    return c.inputs[l][:c.usable_rows], c.tables[l][:c.usable_rows]


@pytest.mark.parametrize("name", lc.NAMES)
def test_oracle_verdict_and_constraints(name):
    """the oracle succeeds, or fails at exactly the lookup the case names; A' is a permutation of the inputs, S' of the table, and on every
    row A'[r] == S'[r] or A'[r] == A'[r - 1]"""
    c = lc.case(name)
    want, failed_at = lc.expected(name)
    assert failed_at == c.error
    if c.error is not None:
        # every lookup before the named one is sound: the named one is the first
        for l in range(c.error):
            inp, table = columns(c, l)
            assert set(inp) <= set(table)
        inp, table = columns(c, c.error)
        assert set(inp) - set(table)
        return
    assert len(want) == len(c.inputs)
    for l, (a, s) in enumerate(want):
        inp, table = columns(c, l)
        assert len(a) == len(s) == c.usable_rows
        assert Counter(a) == Counter(inp) and Counter(s) == Counter(table), l
        assert a[0] == s[0] and all(a[r] == s[r] or a[r] == a[r - 1] for r in range(1, len(a))), l


def tie_kind(c, l):
    inp, table = columns(c, l)
    ti, tt = lc.tied(inp), lc.tied(table)
    return {(False, False): None, (True, False): "input-only", (False, True): "table-only", (True, True): "both"}[(ti, tt)]


@pytest.mark.parametrize("name", lc.NAMES)
def test_case_reaches_what_it_claims(name):
    c = lc.case(name)
    n, reach = c.usable_rows, dict(c.reach)
    assert c.rows >= n and (c.call == "batch" or len(c.inputs) == 1)
    if "tiles" in reach:
        assert lc.tiles(n) == reach.pop("tiles")
    if "radix_scan_trips" in reach:  # radix_scan_kernel: RADIX words per tile, RADIX_SCAN_BLOCK per trip
        words = lc.RADIX * lc.tiles(n)
        assert -(-words // lc.RADIX_SCAN_BLOCK) == reach.pop("radix_scan_trips") and words % lc.RADIX_SCAN_BLOCK
    if "sums_scan_trips" in reach:   # scan_sums_kernel: one sum per tile, SUMS_SCAN_BLOCK per trip
        assert -(-lc.tiles(n) // lc.SUMS_SCAN_BLOCK) == reach.pop("sums_scan_trips") and lc.tiles(n) > 256
    if "batch_gt" in reach:
        assert len(c.inputs) > reach.pop("batch_gt") and len(c.inputs) % lc.CHUNK
    for l, kind in reach.pop("tied", {}).items():
        got = tie_kind(c, l)
        assert got is not None and (kind == "some" or got == kind), (l, kind, got)
    for l in reach.pop("untied", []):
        assert tie_kind(c, l) is None, l
    for l, limbs in reach.pop("varying_limbs", {}).items():
        for col in columns(c, l):
            assert tuple(k for k, v in enumerate(lc.varies(col)) if v) == limbs, l
            assert all((col[0] >> (64 * k)) & lc.M64 for k in range(4) if k not in limbs)  # the constant limbs are not zero
    for l, key in reach.pop("key", {}).items():
        for col in columns(c, l):
            assert lc.fast_key(lc.varies(col)) == key, l
    for l, count in reach.pop("digit_values", {}).items():
        for col in columns(c, l):
            seen = lc.digits_seen(col)
            assert len(seen) == lc.PASSES and all(len(d) == count for d in seen.values()), l
    for l in reach.pop("all_digits", []):
        for col in columns(c, l):
            assert any(len(d) == lc.RADIX for d in lc.digits_seen(col).values()), l
    high = 256 * lc.TILE
    for l in reach.pop("high_tile", []):
        # a repeated row of A' and a left-over position of the sorted table (not the first instance of an input value) in tile 256 or above:
        # their compacted indices need the carry of scan_sums_kernel
        inp, table = columns(c, l)
        a, s, present = sorted(inp), sorted(table), set(inp)
        assert any(a[r] == a[r - 1] for r in range(high, n)), l
        assert any(s[r] == s[r - 1] or s[r] not in present for r in range(high, n)), l
        assert any(a[r] != a[r - 1] for r in range(high, n)), l  # and a run start, whose table instance is searched for
    if "n_rep" in reach:
        inp, table = columns(c, 0)
        assert reach.pop("n_rep") == 0 and len(set(inp)) == n and sorted(inp) == sorted(table)
        a, s = lc.expected(name)[0][0]
        assert a == s
    for l, branch in reach.pop("miss_branch", {}).items():
        inp, table = columns(c, l)
        (absent,) = set(inp) - set(table)
        lo = bisect.bisect_left(sorted(table), absent)
        assert (lo == n) == (branch == "above") and (branch != "inside" or lo < n), (l, lo)
    reach.pop("kinds", None)
    assert not reach, f"reach properties nobody checked: {sorted(reach)}"


def test_missing_reaches_every_place():
    """the three places an absent value can fall, per field: lower bound 0, strictly inside, n"""
    for field in ("fp", "fq"):
        los = []
        for where in ("below", "between", "above"):
            c = lc.case(f"missing-{field}-{where}")
            inp, table = columns(c, 0)
            (absent,) = set(inp) - set(table)
            los.append(bisect.bisect_left(sorted(table), absent))
        assert los[0] == 0 and 0 < los[1] < c.usable_rows and los[2] == c.usable_rows
        # behind usable_rows: the value is in the whole table column and not in its usable part; the stray input is behind the usable part
        c = lc.case(f"missing-{field}-table-tail")
        (absent,) = set(c.inputs[0][:c.usable_rows]) - set(c.tables[0][:c.usable_rows])
        assert absent in c.tables[0][c.usable_rows:]
        c = lc.case(f"missing-{field}-input-tail")
        assert set(c.inputs[0]) - set(c.tables[0]) and not set(c.inputs[0][:c.usable_rows]) - set(c.tables[0][:c.usable_rows])


def test_chunk_boundaries_and_order_cases():
    c = lc.case("chunks")
    assert len(c.inputs) == 67 and set(lc.CHUNKS_TIED) == {31, 32, 40, 66} and set(c.reach["kinds"]) == set(lc.KINDS)
    assert all(i in c.reach["tied"] for i in lc.CHUNKS_TIED)
    assert c.usable_rows == 2049 + 300 and c.rows > c.usable_rows
    for variant, first, later in (("3+5", 3, 5), ("35+37", 35, 37)):
        c = lc.case(f"missing-order-{variant}")
        assert c.error == first and first // lc.CHUNK == later // lc.CHUNK
        assert set(c.inputs[later][:c.usable_rows]) - set(c.tables[later][:c.usable_rows])  # the later one fails too, and is not tied
        assert tie_kind(c, later) is None and tie_kind(c, first) is not None
    assert lc.case("missing-order-40").error == 40 and len(lc.case("missing-order-40").inputs) == 41
    assert lc.case("missing-order-37").error == 37 and tie_kind(lc.case("missing-order-37"), 37) is None


def test_no_valid_lookup_ties_in_the_input_alone():
    """lookup_cases' docstring: where every input value is in the table, a tie of the input column is one of the table column too"""
    for name in lc.NAMES:
        c = lc.case(name)
        if name == "big":
            continue  # its tied lookup is checked above; the rule is about the mask, not the size
        for l in range(len(c.inputs)):
            inp, table = columns(c, l)
            if set(inp) <= set(table):
                assert tie_kind(c, l) != "input-only", (name, l)
