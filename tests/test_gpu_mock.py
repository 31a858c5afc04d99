"""MockProver::verify on the device (tiny_ram_halo2_amd/mock.py; trh_expr_check_dev, trh_lookup_check_dev, trh_perm_check_dev).

Expected values never come from the device: gate polynomials are evaluated row by row with oracle.pasta.evaluate_expression, lookups are
decided by a Python set of tuples (tests/mock_cases.py, the inputs tests/test_mock_host.py runs through the host build of the same set).

  gate check     a system of five outputs -- four STORE_TOP, one STORE_ACC over two folded polynomials -- with rotations -1 and +1 and one
                 expression deep enough to spill to LDS; 2^5 rows (less than one wave: W = 1), 2^6 and 2^8 (one workgroup; 2^8 with every row
                 usable), 2^9 with 2^9 - 6 usable rows (the last wave partly masked); one cell corrupted at row 0, 63, 64, usable_rows - 1
                 and at usable_rows itself, a blinding row that shows only through its neighbour's rotation
  lookup check   widths 1, 2, 5 over the tables and planted misses of mock_cases; counts, first row, bitmap, and the probe cap
  ordering       a column scaled on a non-blocking stream and checked straight after, with no synchronisation in between
  MockProver     the logic chip's constraint system (tests/test_gpu_logic_chip.py's docstring, WORD_BITS 8, k = 9) plus two copy constraints
  native         tests/native/mock_check_test over include/trh.hpp against the Python layer and the model"""
import ctypes
import functools
import json
import os
import random
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import mock_cases as mc
from common import expr_to_tuple
from oracle import pasta as o
from tiny_ram_halo2_amd import api, expr, mock, permutation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLINDING = 6


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


def to_dev(f, col):
    return torch.from_numpy(np.array([f.limbs(v) for v in col], dtype=np.uint64).view(np.int64)).cuda()


def words_of(t):
    return t.cpu().numpy().view(np.uint64)


def bitmap_of(n_words, rows):
    w = np.zeros(n_words, dtype=np.uint64)
    for r in rows:
        w[r // 64] |= np.uint64(1) << np.uint64(r % 64)
    return w


# ---- gate check --------------------------------------------------------------------------------------------------------------------------
# advice 0 .. 3: free values; advice 4 .. 9: the value each expression takes, so that p_i = s (E_i - c_i) vanishes on the witness whatever
# E_i queries; selector 0: one on every usable row
Y = 0x7E57AB1E0DDC0FFEE
A = [expr.Advice(i) for i in range(10)]
S = expr.Selector(0)
GATE_SIZES = {5: (1 << 5) - BLINDING, 6: (1 << 6) - BLINDING, 8: 1 << 8, 9: (1 << 9) - BLINDING}   # log_n -> usable_rows


def gate_expressions():
    r = lambda c, rot: expr.Advice(c, rot)   # noqa: E731
    return [A[0] + A[1] * 3 - A[2],
            r(1, 1) * A[0] - r(3, -1),
            ((A[0] * A[1]) + (A[2] * A[3])) * ((A[0] + A[2]) * (A[1] + A[3])),      # four stack entries: two of them in LDS
            r(2, 1) - r(2, -1),
            A[3] * A[3],                                                              # the two folded polynomials
            r(0, -1) + A[1]]


def gate_polys():
    return [S * (e - A[4 + i]) for i, e in enumerate(gate_expressions())]


def gate_program(field):
    """outputs 0 .. 3: STORE_TOP of p_0 .. p_3; output 4: STORE_ACC of p_4 y + p_5"""
    polys = gate_polys()
    lo = expr._Lowering(field, first_const=Y)
    for i, p in enumerate(polys[:4]):
        lo.emit(p)
        lo.insns.append((expr.OP["STORE_TOP"], i, 0))
    for p in polys[4:]:
        lo.emit(p)
        lo.insns.append((expr.OP["FOLD"], 0, 0))
    lo.insns.append((expr.OP["STORE_ACC"], 4, 0))
    return lo.program(field, max(p.degree() for p in polys))


@functools.lru_cache(maxsize=None)
def gate_evaluator(field):
    ev = expr.GateEvaluator(gate_program(field), n_outputs=5)
    assert ev.lds_slots() > 0
    return ev


def gate_model(f, ints, n, usable):
    """-> the bad rows of each of the five outputs, from the oracle row by row"""
    tuples = [expr_to_tuple(p) for p in gate_polys()]
    bad = [[] for _ in range(5)]
    for row in range(usable):
        v = [o.evaluate_expression(f, t, ints, row, n, 1) for t in tuples]
        for a in range(4):
            if v[a]:
                bad[a].append(row)
        if (v[4] * Y + v[5]) % f.m:
            bad[4].append(row)
    return bad


@functools.lru_cache(maxsize=None)
def gate_witness(field, log_n):
    """integer columns of a satisfying witness (computed once per shape and never changed: corruptions work on copies)"""
    f = o.FIELDS[field]
    n, usable = 1 << log_n, GATE_SIZES[log_n]
    rng = random.Random(0x90C7 + 64 * log_n + (field == "fq"))
    ints = {("advice", c): [rng.randrange(f.m) for _ in range(n)] for c in range(10)}
    ints[("selector", 0)] = [1 if r < usable else rng.randrange(f.m) for r in range(n)]
    for i, e in enumerate(gate_expressions()):
        t = expr_to_tuple(e)
        for row in range(usable):
            ints[("advice", 4 + i)][row] = o.evaluate_expression(f, t, ints, row, n, 1)
    assert gate_model(f, ints, n, usable) == [[]] * 5
    return ints


def check_against_model(field, log_n, ints, dev):
    f = o.FIELDS[field]
    n, usable = 1 << log_n, GATE_SIZES[log_n]
    W = max(1, n // 64)
    ev = gate_evaluator(field)
    want = gate_model(f, ints, n, usable)
    n_bad, first, words = ev.check(dev, log_n, usable, bitmap=True)
    assert [int(v) for v in n_bad] == [len(b) for b in want]
    assert [int(v) for v in first] == [b[0] if b else usable for b in want]
    assert words.shape == (5, W)
    assert (words_of(words) == np.stack([bitmap_of(W, b) for b in want])).all()
    plain = ev.check(dev, log_n, usable)                                   # without a bitmap: the same counts
    assert (plain[0] == n_bad).all() and (plain[1] == first).all()
    # the bitmap is eval(...) != 0 on the usable rows
    values = ev.eval(dev, log_n, 1)
    torch.cuda.synchronize()
    nonzero = values.ne(0).any(dim=-1).cpu().numpy()
    assert [list(np.flatnonzero(nonzero[a][:usable])) for a in range(5)] == want
    return want


@pytest.mark.parametrize("field", ["fp", "fq"])
@pytest.mark.parametrize("log_n", sorted(GATE_SIZES))
def test_gate_check_equals_the_model(field, log_n):
    f = o.FIELDS[field]
    n, usable = 1 << log_n, GATE_SIZES[log_n]
    ints = gate_witness(field, log_n)
    dev = {k: to_dev(f, col) for k, col in ints.items()}
    assert check_against_model(field, log_n, ints, dev) == [[]] * 5
    # every word is written, zeros included: a bitmap full of ones comes back clear
    ev = gate_evaluator(field)
    ptrs = (ctypes.c_void_p * len(ev.program.columns))(*[dev[k].data_ptr() for k in ev.program.columns])
    ones = torch.full((5, max(1, n // 64)), -1, dtype=torch.int64, device="cuda")
    n_bad, first = np.zeros(5, np.uint64), np.zeros(5, np.uint64)
    api._check(api.lib().trh_expr_check_dev(ev.handle, ptrs, log_n, usable, api._p(n_bad), api._p(first), ones.data_ptr()))
    assert not words_of(ones).any() and not n_bad.any() and (first == usable).all()
    # one corrupted cell of advice 2 (queried at rotations 0, -1 and +1)
    seen_through_rotation = False
    for row in sorted({r for r in (0, 63, 64, usable - 1, usable) if r < n}):
        bad = dict(ints)
        bad[("advice", 2)] = list(ints[("advice", 2)])
        bad[("advice", 2)][row] = (bad[("advice", 2)][row] + 1) % f.m
        bad_dev = dict(dev)
        bad_dev[("advice", 2)] = to_dev(f, bad[("advice", 2)])
        want = check_against_model(field, log_n, bad, bad_dev)
        assert any(want), row
        if row >= usable:   # a blinding row: only p_3's rotations reach it
            assert want[0] == [] and want[2] == [] and want[3] == sorted({(row - 1) % n, (row + 1) % n} & set(range(usable)))
            seen_through_rotation = True
    assert seen_through_rotation == (usable < n)


def test_gate_check_with_more_outputs_than_one_landing_area_holds():
    """300 outputs are 600 verdict words, 4800 bytes: more than the 4 KiB the context's pinned landing area starts with.  In a fresh context
    the five-output check comes first and allocates the area at 4 KiB; the 300-output check behind it has to GROW it (the old area is freed
    while the context lives on); then the five-output check again, which asks for less than is there, and the 300 outputs once more through
    the area as it stands.  300 gates of expr.synthetic_gates, one output each, at log_n = 7 with 100 usable rows: the advice is random and
    every selector zero, so every output vanishes -- except that three gates which share their selector with no other gate have it set on
    one row each: rows 0, 63 (the last lane of the first wave) and 99 (the last usable row).  The expected verdict is the oracle's, row by
    row."""
    field, log_n, usable, n_gates = "fp", 7, 100, 300
    f, n = o.FIELDS[field], 1 << log_n
    gates = expr.synthetic_gates(12, 4096, n_gates, seed=0x4B1D)
    selector_of = [g.a.column for g in gates]                                  # a gate is Selector * body
    assert all(isinstance(g.a, expr.Selector) for g in gates)
    lone = [a for a, c in enumerate(selector_of) if selector_of.count(c) == 1]
    chosen = {lone[0]: 0, lone[len(lone) // 2]: 63, lone[-1]: 99}
    assert len(chosen) == 3
    ev = expr.GateEvaluator(expr.compile_outputs(field, gates), n_outputs=n_gates)
    rng = random.Random(0x1A4D)
    ints = {key: [rng.randrange(f.m) for _ in range(n)] if key[0] == "advice" else [0] * n for key in ev.program.columns}
    for a, row in chosen.items():
        ints[("selector", selector_of[a])][row] = 1
    tuples = [expr_to_tuple(g) for g in gates]
    want = [[row for row in range(usable) if o.evaluate_expression(f, t, ints, row, n, 1)] for t in tuples]
    assert {a: b for a, b in enumerate(want) if b} == {a: [row] for a, row in chosen.items()}
    zeros = to_dev(f, [0] * n)
    dev = {key: to_dev(f, col) if any(col) else zeros for key, col in ints.items()}
    # the five-gate system at log_n = 6, satisfied and with one corrupted cell
    ints5 = gate_witness(field, 6)
    dev5 = {k: to_dev(f, col) for k, col in ints5.items()}
    bad5 = dict(ints5)
    bad5[("advice", 2)] = list(ints5[("advice", 2)])
    bad5[("advice", 2)][57] = (bad5[("advice", 2)][57] + 1) % f.m
    bad_dev5 = dict(dev5)
    bad_dev5[("advice", 2)] = to_dev(f, bad5[("advice", 2)])

    def five_outputs():
        assert check_against_model(field, 6, ints5, dev5) == [[]] * 5
        assert any(check_against_model(field, 6, bad5, bad_dev5))

    def three_hundred_outputs():
        W = n // 64
        n_bad, first, words = ev.check(dev, log_n, usable, bitmap=True)
        assert [int(v) for v in n_bad] == [len(b) for b in want]
        assert [int(v) for v in first] == [b[0] if b else usable for b in want]
        assert words.shape == (n_gates, W) and (words_of(words) == np.stack([bitmap_of(W, b) for b in want])).all()
        plain = ev.check(dev, log_n, usable)
        assert (plain[0] == n_bad).all() and (plain[1] == first).all()

    fresh = api.Context(0)                                                     # whatever ran before this test: this context has no landing area yet
    try:
        with fresh:
            five_outputs()            # allocates the area at 4 KiB
            three_hundred_outputs()   # grows it
            five_outputs()            # asks for less than is there
            three_hundred_outputs()
    finally:
        fresh.destroy()


def test_gate_check_refusals():
    field, log_n = "fp", 6
    f = o.FIELDS[field]
    ints = gate_witness(field, log_n)
    dev = {k: to_dev(f, col) for k, col in ints.items()}
    ev = gate_evaluator(field)
    lib = api.lib()
    ptrs = (ctypes.c_void_p * len(ev.program.columns))(*[dev[k].data_ptr() for k in ev.program.columns])
    n_bad, first = np.zeros(5, np.uint64), np.zeros(5, np.uint64)
    nb, fb = api._p(n_bad), api._p(first)
    assert lib.trh_expr_check_dev(ev.handle, ptrs, log_n, 0, nb, fb, None) == -1 and b"usable_rows" in lib.trh_last_error()
    assert lib.trh_expr_check_dev(ev.handle, ptrs, log_n, (1 << log_n) + 1, nb, fb, None) == -1 and b"usable_rows" in lib.trh_last_error()
    assert lib.trh_expr_check_dev(ev.handle, ptrs, 31, 1, nb, fb, None) == -1 and b"log_n" in lib.trh_last_error()
    assert lib.trh_expr_check_dev(None, ptrs, log_n, 58, nb, fb, None) == -1 and b"null" in lib.trh_last_error()
    assert lib.trh_expr_check_dev(ev.handle, None, log_n, 58, nb, fb, None) == -1 and b"null" in lib.trh_last_error()
    assert lib.trh_expr_check_dev(ev.handle, ptrs, log_n, 58, None, fb, None) == -1 and b"null" in lib.trh_last_error()
    assert lib.trh_expr_check_dev(ev.handle, ptrs, log_n, 58, nb, None, None) == -1 and b"null" in lib.trh_last_error()
    holed = (ctypes.c_void_p * len(ev.program.columns))(*ptrs)
    holed[1] = None
    assert lib.trh_expr_check_dev(ev.handle, holed, log_n, 58, nb, fb, None) == -1 and b"column 1" in lib.trh_last_error()
    assert lib.trh_expr_check_dev(ev.handle, ptrs, log_n, 58, nb, fb, None) == 0 and not n_bad.any()


# ---- lookup check ------------------------------------------------------------------------------------------------------------------------
def dev_columns(cols):
    return [torch.from_numpy(np.ascontiguousarray(c).view(np.int64)).cuda() for c in cols]


@pytest.mark.parametrize("field", ["fp", "fq"])
@pytest.mark.parametrize("kind", mc.TABLES)
@pytest.mark.parametrize("width", [1, 2, 5])
def test_lookup_check_equals_the_model_within_the_probe_cap(field, kind, width):
    for usable in mc.sizes(kind):
        for bad in (False, True):
            inputs, tables = mc.lookup_case(kind, width, usable, bad)
            want_n, want_first, want_words = mc.lookup_model(inputs, tables, usable)
            assert (want_n > 0) == bad
            d_in, d_tab = dev_columns(inputs), dev_columns(tables)
            n_bad, first, words = mock.lookup_check(field, d_in, d_tab, usable, bitmap=True)
            probes = api.stat("lookup_check_probes")
            what = (kind, width, usable, bad)
            print(what, "probes", probes, "cap", mc.PROBE_CAP * 2 * usable)
            assert (n_bad, first) == (want_n, want_first), what
            assert (words_of(words) == want_words).all(), what
            assert mock.lookup_check(field, d_in, d_tab, usable) == (want_n, want_first), what
            assert 2 * usable <= probes <= mc.PROBE_CAP * (usable + usable), (what, probes)   # table rows + input rows, both usable_rows
            if kind == "same" and not bad:
                assert probes == 2 * usable, what                              # the duplicates were dropped at the first slot


def test_lookup_check_writes_every_bitmap_word_and_refuses_bad_arguments():
    usable = 65
    inputs, tables = mc.lookup_case("range", 2, usable, False)
    d_in, d_tab = dev_columns(inputs), dev_columns(tables)
    lib = api.lib()
    ip = (ctypes.c_void_p * 2)(*[t.data_ptr() for t in d_in])
    tp = (ctypes.c_void_p * 2)(*[t.data_ptr() for t in d_tab])
    n_bad, first = ctypes.c_uint64(9), ctypes.c_uint64(9)
    nb, fb = ctypes.byref(n_bad), ctypes.byref(first)
    ones = torch.full((3,), -1, dtype=torch.int64, device="cuda")              # two words belong to the bitmap, the third is not its
    assert lib.trh_lookup_check_dev(api.FP, ip, tp, 2, usable, nb, fb, ones.data_ptr()) == 0
    assert (n_bad.value, first.value) == (0, usable) and list(words_of(ones)) == [0, 0, 0xFFFFFFFFFFFFFFFF]
    for args, text in (((api.FP, ip, tp, 0, usable, nb, fb, None), b"width"), ((api.FP, ip, tp, 17, usable, nb, fb, None), b"width"),
                       ((api.FP, ip, tp, 2, 0, nb, fb, None), b"usable_rows"), ((api.FP, ip, tp, 2, (1 << 30) + 1, nb, fb, None), b"usable_rows"),
                       ((api.FP, None, tp, 2, usable, nb, fb, None), b"null"), ((api.FP, ip, None, 2, usable, nb, fb, None), b"null"),
                       ((api.FP, ip, tp, 2, usable, None, fb, None), b"null"), ((api.FP, ip, tp, 2, usable, nb, None, None), b"null"),
                       ((7, ip, tp, 2, usable, nb, fb, None), b"unknown field id 7")):
        assert lib.trh_lookup_check_dev(*args) == -1 and text in lib.trh_last_error(), text
    assert lib.trh_last_error() == b"unknown field id 7"                       # the id is refused as everywhere else, and the context stays usable
    assert lib.trh_lookup_check_dev(api.FQ, ip, tp, 2, usable, nb, fb, None) == 0 and (n_bad.value, first.value) == (0, usable)
    holed = (ctypes.c_void_p * 2)(d_tab[0].data_ptr(), None)
    assert lib.trh_lookup_check_dev(api.FP, ip, holed, 2, usable, nb, fb, None) == -1 and b"table column 1" in lib.trh_last_error()
    odd = (ctypes.c_void_p * 2)(d_in[0].data_ptr() + 8, d_in[1].data_ptr())
    assert lib.trh_lookup_check_dev(api.FP, odd, tp, 2, usable, nb, fb, None) == -1 and b"aligned" in lib.trh_last_error()


# ---- ordering ----------------------------------------------------------------------------------------------------------------------------
def test_checks_follow_a_call_on_a_non_blocking_stream():
    """A column produced by trh_field_scale_dev on a non-blocking stream is checked straight after, with no synchronisation in between:
    both checks open with TRH_ENTER(0), which makes the null stream wait for the context's previous call.  The verdict must be that of the
    scaled data.  Without a delay window in front of the scaling (tests/test_gpu_streams.py's method) this is not decisive: the scaling
    kernel may simply have finished before the check starts, ordered or not."""
    field, log_n = "fq", 9
    f = o.FIELDS[field]
    n, usable = 1 << log_n, (1 << log_n) - BLINDING
    rng = random.Random(0x0D3)
    x = [rng.randrange(f.m) for _ in range(n)]
    three_x = [3 * v % f.m for v in x]
    ev = expr.GateEvaluator(expr.compile_outputs(field, [A[0] - A[1]]), n_outputs=1)
    side = torch.cuda.Stream()
    want = to_dev(f, three_x)
    col = to_dev(f, x)
    torch.cuda.synchronize()
    assert int(ev.check({("advice", 0): col, ("advice", 1): want}, log_n, usable)[0][0]) == usable          # x != 3 x on every row
    api.field_scale_dev(field, col, n, expr._limbs(field, 3), stream=side.cuda_stream)
    n_bad, first = ev.check({("advice", 0): col, ("advice", 1): want}, log_n, usable)
    assert (int(n_bad[0]), int(first[0])) == (0, usable)
    col2 = to_dev(f, x)
    torch.cuda.synchronize()
    assert mock.lookup_check(field, [want], [col2], usable)[0] == usable
    api.field_scale_dev(field, col2, n, expr._limbs(field, 3), stream=side.cuda_stream)
    assert mock.lookup_check(field, [want], [col2], usable) == (0, usable)


# ---- MockProver.verify on the logic chip ---------------------------------------------------------------------------------------------------
# The constraint system of tests/test_gpu_logic_chip.py's docstring (even_bits.rs:143-170, logic.rs:125-185 of the reference; WORD_BITS = 8,
# k = 9), restated: every decomposed word has its gate and two lookups into the even-bits table, then l_add, and, xor, or.  One more advice
# column, `cp`, carries two copies: cp[3] = a[3] and cp[7] = res[5].
WORD_BITS, K, USED = 8, 9, 400
ADV = ["s_and", "s_xor", "s_or", "a", "a_e", "a_o", "b", "b_e", "b_o", "es", "es_e", "es_o", "os", "os_e", "os_o", "res", "cp"]
Q = {name: expr.Advice(i) for i, name in enumerate(ADV)}
S_TABLE = expr.Selector(0)
T_EVEN = expr.Fixed(1)
DECOMPOSED = [("a", "a_e", "a_o"), ("b", "b_e", "b_o"), ("es", "es_e", "es_o"), ("os", "os_e", "os_o")]
PERM_COLUMNS = [("advice", ADV.index("a")), ("advice", ADV.index("res")), ("advice", ADV.index("cp"))]


def logic_system():
    s = S_TABLE * (Q["s_and"] + Q["s_xor"] + Q["s_or"])
    two = expr.Constant(2)
    gates, lookups = [], []
    for word, even, odd in DECOMPOSED:
        gates.append((f"decompose {word}", [s * (Q[even] + two * Q[odd] - Q[word])]))
        lookups.append((f"{even} even bits", [s * Q[even]], [T_EVEN]))
        lookups.append((f"{odd} even bits", [s * Q[odd]], [T_EVEN]))
    gates.append(("l_add", [s * (Q["a_e"] + Q["b_e"] - Q["es"]), s * (Q["a_o"] + Q["b_o"] - Q["os"])]))
    and_ = Q["es_o"] + two * Q["os_o"]
    xor = Q["es_e"] + two * Q["os_e"]
    gates.append(("and", [S_TABLE * Q["s_and"] * (and_ - Q["res"])]))
    gates.append(("xor", [S_TABLE * Q["s_xor"] * (xor - Q["res"])]))
    gates.append(("or", [S_TABLE * Q["s_or"] * (xor + and_ - Q["res"])]))
    return gates, lookups


def logic_witness(n, seed):
    rng = random.Random(seed)
    dec = lambda w: (w & 0x55, (w >> 1) & 0x55)   # noqa: E731
    cols = {name: [0] * n for name in ADV}
    s_table = [0] * n
    for row in range(USED):
        s_table[row] = 1
        op = ("and", "xor", "or", "none")[row % 4] if row < 8 else rng.choice(("and", "xor", "or", "none"))
        a, b = rng.randrange(1 << WORD_BITS), rng.randrange(1 << WORD_BITS)
        if op == "none":
            cols["a"][row], cols["res"][row] = a, rng.randrange(1 << 20)
            continue
        cols["s_" + op][row] = 1
        (ae, ao), (be, bo) = dec(a), dec(b)
        es, os_ = ae + be, ao + bo
        (ese, eso), (ose, oso) = dec(es), dec(os_)
        res = {"and": a & b, "xor": a ^ b, "or": a | b}[op]
        for name, v in (("a", a), ("a_e", ae), ("a_o", ao), ("b", b), ("b_e", be), ("b_o", bo), ("es", es), ("es_e", ese), ("es_o", eso),
                        ("os", os_), ("os_e", ose), ("os_o", oso), ("res", res)):
            cols[name][row] = v
    cols["cp"][3], cols["cp"][7] = cols["a"][3], cols["res"][5]
    spread = lambda v: sum(((v >> b) & 1) << (2 * b) for b in range(WORD_BITS // 2))   # noqa: E731
    table = [spread(i) if i < (1 << (WORD_BITS // 2)) else 0 for i in range(n)]
    return cols, s_table, table


def logic_ints(cols, s_table, table):
    d = {("advice", i): cols[name] for i, name in enumerate(ADV)}
    d[("selector", 0)] = s_table
    d[("fixed", 1)] = table
    return d


def logic_model(f, gates, lookups, ints, n, usable):
    """MockProver's verdict from the oracle: gate polynomials row by row, lookups through a set of table tuples"""
    out = []
    for gi, (name, polys) in enumerate(gates):
        for pi, p in enumerate(polys):
            t = expr_to_tuple(p)
            out += [mock.ConstraintNotSatisfied(gi, pi, name, r) for r in range(usable) if o.evaluate_expression(f, t, ints, r, n, 1)]
    for li, (name, inputs, tables) in enumerate(lookups):
        ev = lambda es, r: tuple(o.evaluate_expression(f, expr_to_tuple(e), ints, r, n, 1) for e in es)   # noqa: E731
        table = {ev(tables, r) for r in range(usable)}
        out += [mock.Lookup(li, name, r) for r in range(usable) if ev(inputs, r) not in table]
    return out


def test_mock_prover_verify_on_the_logic_chip():
    field = "fp"
    f = o.FIELDS[field]
    n, usable = 1 << K, (1 << K) - BLINDING
    gates, lookups = logic_system()
    asm = permutation.Assembly(field, K, len(PERM_COLUMNS))
    asm.copy(2, 3, 0, 3)       # cp[3] = a[3]
    asm.copy(2, 7, 1, 5)       # cp[7] = res[5]
    prover = mock.MockProver(field, K, usable, gates, lookups, permutation=asm, permutation_columns=PERM_COLUMNS)
    cols, s_table, table = logic_witness(n, 0x10C)
    ints = logic_ints(cols, s_table, table)
    assert logic_model(f, gates, lookups, ints, n, usable) == []
    dev = {k: to_dev(f, c) for k, c in ints.items()}
    assert prover.verify(dev) == []

    def corrupted(changes):
        bad = {name: list(c) for name, c in cols.items()}
        for name, row, delta in changes:
            bad[name][row] += delta
        bad_ints = logic_ints(bad, s_table, table)
        bad_dev = dict(dev)
        for name in {c[0] for c in changes}:
            key = ("advice", ADV.index(name))
            bad_dev[key] = to_dev(f, bad[name])
        return bad_ints, bad_dev

    # a gate row: a wrong xor result
    row = next(r for r in range(8, USED) if cols["s_xor"][r])
    bad_ints, bad_dev = corrupted([("res", row, 1)])
    want = [mock.ConstraintNotSatisfied([g[0] for g in gates].index("xor"), 0, "xor", row)]
    assert logic_model(f, gates, lookups, bad_ints, n, usable) == want
    assert prover.verify(bad_dev) == want
    # an even part that is not an even-bits value, with every gate still satisfied: on an xor row the odd part of even_sum is in no gate but
    # its own decomposition, so a_e + 2, a + 2, es + 2, es_o + 1 keeps the polynomials at zero -- only the lookup of a_e can object
    row = next(r for r in range(8, USED) if cols["s_xor"][r] and not cols["es_o"][r] & 1)
    bad_ints, bad_dev = corrupted([("a_e", row, 2), ("a", row, 2), ("es", row, 2), ("es_o", row, 1)])
    want = [mock.Lookup(0, "a_e even bits", row)]
    assert logic_model(f, gates, lookups, bad_ints, n, usable) == want
    assert prover.verify(bad_dev) == want
    # a broken copy: cp[7] no longer equals res[5]; both cells of the cycle differ from the cell they map to
    bad_ints, bad_dev = corrupted([("cp", 7, 1)])
    assert logic_model(f, gates, lookups, bad_ints, n, usable) == []
    assert prover.verify(bad_dev) == [mock.Permutation((1, 5), 2)]
    # everything at once, and the cap on the row records
    bad_ints, bad_dev = corrupted([("res", row, 1), ("cp", 7, 1), ("a_e", row, 2), ("a", row, 2), ("es", row, 2), ("es_o", row, 1)])
    rows = logic_model(f, gates, lookups, bad_ints, n, usable)
    assert len(rows) == 2 and prover.verify(bad_dev) == rows + [mock.Permutation((1, 5), 2)]
    assert prover.verify(bad_dev, max_failures=1) == rows[:1] + [mock.Permutation((1, 5), 2)]


# ---- the C++ wrappers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["fp", "fq"])
def test_native_mock_check_matches_python(field):
    """tests/native/mock_check_test (trh::GateEvaluator::check, trh::lookup_check) on its 2^6-row system, restated here"""
    exe = os.path.join(ROOT, "tests", "native", "mock_check_test")
    assert os.path.exists(exe), "tests/native/mock_check_test is missing: run `make`"
    r = subprocess.run([exe, field], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    f = o.FIELDS[field]
    k, n, usable = 6, 64, 58
    a = [r_ + 1 for r_ in range(n)]
    b = [2 * r_ + 3 for r_ in range(n)]
    c = [x * y for x, y in zip(a, b)]
    c[5] += 1
    c[40] += 1
    a[usable] += 1
    ints = {("advice", 0): a, ("advice", 1): b, ("advice", 2): c}
    polys = [A[0] * A[1] - A[2], expr.Advice(0, 1) - A[0] - expr.Constant(1)]
    want = [[r_ for r_ in range(usable) if o.evaluate_expression(f, expr_to_tuple(p), ints, r_, n, 1)] for p in polys]
    assert want == [[5, 40], [57]]
    ev = expr.GateEvaluator(expr.compile_outputs(field, polys), n_outputs=2)
    n_bad, first, words = ev.check({key: to_dev(f, col) for key, col in ints.items()}, k, usable, bitmap=True)
    assert got["gate_n_bad"] == [int(v) for v in n_bad] == [2, 1]
    assert got["gate_first_bad_row"] == [int(v) for v in first] == [5, 57]
    assert got["gate_bitmap"] == [f"{int(w):016x}" for w in words_of(words).reshape(-1)] == [f"{int(bitmap_of(1, w)[0]):016x}" for w in want]
    t0, t1 = list(range(n)), [3 * t + 1 for t in range(n)]
    i0, i1 = [t0[5 * r_ % usable] for r_ in range(n)], [t1[5 * r_ % usable] for r_ in range(n)]
    i0[0], i1[0] = 1, 1
    i0[usable - 1], i1[usable - 1] = t0[60], t1[60]
    table = {(t0[t], t1[t]) for t in range(usable)}
    bad = [r_ for r_ in range(usable) if (i0[r_], i1[r_]) not in table]
    assert bad == [0, 57]
    l_bad, l_first, l_words = mock.lookup_check(field, [to_dev(f, i0), to_dev(f, i1)], [to_dev(f, t0), to_dev(f, t1)], usable, bitmap=True)
    assert (got["lookup_n_bad"], got["lookup_first_bad_row"]) == (l_bad, l_first) == (2, 0)
    assert got["lookup_bitmap"] == f"{int(words_of(l_words)[0]):016x}" == f"{int(bitmap_of(1, bad)[0]):016x}"
    assert got["lookup_probes"] == api.stat("lookup_check_probes") <= mc.PROBE_CAP * 2 * usable
    assert got["checks_failed"] == 0
