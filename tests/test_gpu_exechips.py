"""trh_exe_chips_dev on the device: the Out selectors, the changed flags and the sub-chips' advice of a trace's steps, against
tests/exechips_model.py.  T = 256 rows per workgroup, B = exetable.INVERSE_STRIP rows per lane of the inversion kernel.

  word for word  drawn steps at W = 16, R = 8, both fields, every cell (a_flag against Python's modular inverse): m = 1, 2, 31, 32, 33 (the
                 flag bitmap's word), T - 1, T, T + 1, 2 T + 1 (the successor across a workgroup), T B - 1, T B, T B + 1 (the strip's edges),
                 n the next power of two, and m = n - 1; flag2 rows whose c + flag' is zero on all but one (the product skips zeros); no
                 flag2 row at all; trh_stat "exechips_flag2_rows" is the model's count
  extremes       W = 32, R = 1 and 16, extreme_steps(R, T + 1): inputs that are no words (pc + 1 = 2^32 as b, a negative SHR_LO as d) give
                 zero groups, a_power = 2^32, check at both signs
  the gates      both entries' columns of an interpreter's trace of 991 steps at n = 1024: every gate of exechips_model.System through
                 expr.compile_gates / GateEvaluator is zero on every row; one corrupted a_flag, r_odd or sg_c_sigma cell gives its row
  the circuit    k = 9, W = 16, tables of 256 rows: the gates, the even-bits lookups and the pow lookup under mock.MockProver; one whole proof
                 accepted by the package's verifier and by tests/plonk_model.py; a wrong a_power is found by MockProver (the shift gate and
                 the pow lookup, on its row), refused by the prover's lookup argument and, proved all the same, by both verifiers
  another table  sub's Out bit moved from sum to ssum: the model's columns for that table
  refusals       odd word_bits, a chips entry with flag3 and shift, one known to chips alone, a bad step: each names its cause and leaves a
                 sentinel-filled destination as it was
  the rest       the caller's non-blocking stream behind a delay, AdviceBuilder.exe_chips, tests/native/exechips_test.cpp over trh.hpp"""
import functools
import json
import os
import random
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import exechips_model as cm
import exetable_model as em
import pasta as o
import transcript_model as tm
from common import expr_from_json as from_json, expr_to_tuple as to_tuple
from plonk_circuits import Circuit
from tiny_ram_halo2_amd import api, exetable, expr, mock, plonk, poly, witness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, B = exetable.ROWS_PER_WORKGROUP, exetable.INVERSE_STRIP
FIELDS = ["fp", "fq"]
FILL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def arrays(steps, R):
    """-> pc, inst, a, regs (m, R), flags (bool), value"""
    u = lambda xs: np.array(xs, dtype=np.uint32)  # noqa: E731
    inst = [s.op | s.ri << 8 | s.rj << 12 | (1 << 16 if s.a_is_reg else 0) for s in steps]
    return (u([s.pc for s in steps]), u(inst), u([s.a for s in steps]), u([s.regs for s in steps]).reshape(len(steps), R),
            np.array([s.flag for s in steps], dtype=np.bool_), u([s.value for s in steps]))


def device_chips(field, W, R, steps, n=None, **kw):
    pc, inst, a, regs, flags, value = arrays(steps, R)
    return exetable.build_chips(field, W, R, pc, inst, a, regs, flags, value, n=n, **kw)


def expected_limbs(field, cols, n):
    """(columns, n, 4) uint64: the model's columns as Montgomery limbs, negative values as m - |v|; each distinct value is converted once"""
    f, cache = o.FIELDS[field], {}
    out = np.zeros((len(cols), n, 4), dtype=np.uint64)
    for c, col in enumerate(cols):
        for r, v in enumerate(col):
            if v:
                if v not in cache:
                    cache[v] = f.limbs(v % f.m)
                out[c, r] = cache[v]
    return out


def compare(field, W, R, steps, n, got=None, chips=None, model_chips=cm.DEFAULT):
    """the device's columns against the model's, every cell; -> (the model's columns by name, the device tensor)"""
    cols = cm.build(W, R, steps, n, o.FIELDS[field].m, chips=model_chips)
    got = device_chips(field, W, R, steps, n, chips=chips) if got is None else got
    assert api.stat("exechips_rows") == len(steps)
    cells, want = host(got).view(np.uint64), expected_limbs(field, cols, n)
    assert cells.shape == want.shape == (52 + R, n, 4)
    if not (cells == want).all():
        c, r = [int(x[0]) for x in np.nonzero((cells != want).any(axis=2))]
        raise AssertionError(f"column {cm.columns(R)[c]}, row {r} of {len(steps)} (n = {n}), step {steps[r] if r < len(steps) else None}: {cells[c, r]} for {want[c, r]} = {cols[c][r]}")
    return dict(zip(cm.columns(R), cols)), got


@functools.lru_cache(maxsize=None)
def drawn(W, R, m, seed=0):
    return em.random_steps(random.Random(1000 * W + 10 * R + m + seed), W, R, m)


SIZES = [(m, 1 << m.bit_length()) for m in (1, 2, 31, 32, 33, T - 1, T, T + 1, 2 * T + 1, T * B - 1, T * B, T * B + 1)] + [(127, 128)]


# ---- word for word -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("m,n", SIZES)
def test_word_for_word_against_the_model(field, m, n):
    assert m < n and (n == m + 1 or n & (n - 1) == 0)
    steps = drawn(16, 8, m)
    cols, _ = compare(field, 16, 8, steps, n)
    assert api.stat("exechips_flag2_rows") == cm.flag2_rows(steps) == sum(cols["out_flag2"])
    if m > 60:  # there is something to invert (the rows whose denominator is zero have a test of their own)
        assert any(cols["a_flag"])


@pytest.mark.parametrize("field", FIELDS)
def test_flag2_rows_that_are_all_zero_but_one_and_none_at_all(field):
    """cmpe of unequal words: c = RI xor A != 0, flag' = 0.  With equal words c = 0 and flag' = 0 behind them (drawn: no machine sets it),
    so c + flag' = 0: a strip's product must skip them"""
    m, n = T * B + 5, 2 * T * B
    zero = em.Step(3, em.OPCODES["cmpe"], 1, 0, 9, False, (0, 9, 0, 0, 0, 0, 0, 0), False, 0)
    steps = [zero._replace(pc=0, regs=(0,) * 8, a=0)] + [zero] * (m - 2) + [em.Step(4, em.OPCODES["answer"], 0, 0, 0, False, (0,) * 8, False, 0)]
    live = T + 70  # one lane's strip holds this row and B - 1 zeros
    steps[live] = zero._replace(a=12)
    cols, _ = compare(field, 16, 8, steps, n)
    f = o.FIELDS[field]
    assert [r for r in range(n) if cols["a_flag"][r]] == [live] and cols["a_flag"][live] == pow(9 ^ 12, -1, f.m)
    assert api.stat("exechips_flag2_rows") == m - 1
    # no flag2 row at all: add, sub and mov only
    plain = [s._replace(op=em.OPCODES[("add", "sub", "mov")[i % 3]]) for i, s in enumerate(drawn(16, 8, T + 9)[:-1])] + [drawn(16, 8, T + 9)[-1]]
    cols, _ = compare(field, 16, 8, plain, 2 * T)
    assert not any(cols["a_flag"]) and not any(cols["out_flag2"]) and api.stat("exechips_flag2_rows") == 0


@pytest.mark.parametrize("field,R", [("fp", 1), ("fq", 16)])
def test_the_extreme_words_at_32_bits(field, R):
    steps = em.extreme_steps(R, T + 1)
    assert len(steps) == T + 1
    cols, _ = compare(field, 32, R, steps, 2 * T)
    tv = dict(zip(em.columns(R), em.build(32, R, steps, 2 * T)))
    rows = range(len(steps))
    name = lambda r: em.NAMES[steps[r].op]  # noqa: E731
    # inputs that are no words give zero groups: b = pc + 1 = 2^32 under mod (cnjmp), d = a negative SHR_LO under a table that decomposes it
    assert any(name(r) == "cnjmp" and tv["tv_b"][r] == 1 << 32 and cols["b_even"][r] == cols["b_odd"][r] == 0 for r in rows)
    assert any(name(r) == "cnjmp" and tv["tv_b"][r] < 1 << 32 and cols["b_even"][r] + 2 * cols["b_odd"][r] == tv["tv_b"][r] > 0 for r in rows)
    assert any(name(r) == "shl" and cols["a_power"][r] == 1 << 32 and cols["a_shift"][r] == 0 and cols["r_word"][r] == 0 for r in rows)   # A == W
    assert any(name(r) == "shr" and cols["a_power"][r] == 1 << 32 and cols["a_shift"][r] == 1 for r in rows)                               # A > W
    assert any(name(r) == "smulh" and cols["sg_a_msb"][r] == 1 and cols["sg_a_check"][r] < 1 << 30 for r in rows)
    assert any(name(r) == "smulh" and cols["sg_a_msb"][r] == 0 and cols["sg_a_check"][r] >= 1 << 30 for r in rows)
    moved = dict(cm.DEFAULT, shr=cm.DEFAULT["shr"] | cm.PROD)  # prod decomposes d: SHR_LO, negative for a shift below W
    chips = dict(exetable.DEFAULT_CHIPS, shr=exetable.DEFAULT_CHIPS["shr"] | exetable.PROD)
    cols, _ = compare(field, 32, R, steps, 2 * T, chips=chips, model_chips=moved)
    assert any(name(r) == "shr" and tv["tv_d"][r] < 0 and cols["d_even"][r] == cols["d_odd"][r] == 0 and cols["out_prod"][r] == 1 for r in rows)
    if R > 1:  # with one register rj = ri = the operand's register: no drawn shr leaves a small positive d
        assert any(name(r) == "shr" and 0 < tv["tv_d"][r] < 1 << 32 and cols["d_even"][r] + 2 * cols["d_odd"][r] == tv["tv_d"][r] for r in rows)


# ---- the gates on the device ------------------------------------------------------------------------------------------------------------------------
W, R = 16, 8
EXE_COLS, CHIP_COLS = 28 + 9 * R, 52 + R
INDEX = {name: i for i, name in enumerate(list(em.columns(R)) + cm.columns(R))}
assert len(INDEX) == EXE_COLS + CHIP_COLS


@functools.lru_cache(maxsize=None)
def system():
    return cm.System(W, R, to_tuple, from_json)


def column_expr(name, rot=0):
    """a column of the model's gates over: Fixed(0) = s_table, the selectors that are sums of Out cells, advice = exe columns then chip columns"""
    if name == "s_table":
        return expr.Fixed(0)
    if name in cm.System.SELECTORS:
        terms = [expr.Advice(INDEX[x], rot) for x in cm.System.out_names(cm.System.SELECTORS[name])]
        return functools.reduce(lambda x, y: x + y, terms)
    return expr.Advice(INDEX[name], rot)


def as_expr(e):
    tag = e[0]
    if tag == "const":
        return expr.Constant(e[1])
    if tag == "col":
        return column_expr(e[1], e[2])
    if tag == "neg":
        return expr.Negated(as_expr(e[1]))
    if tag == "scaled":
        return expr.Scaled(as_expr(e[1]), e[2])
    return {"sum": expr.Sum, "prod": expr.Product}[tag](as_expr(e[1]), as_expr(e[2]))


def long_program(iterations=22):
    """a loop whose body is straight-line code over every opcode but the jumps (registers 0 .. 6; r7 counts), shifts by W - 1, W, W + 1 and by
    a register among them: 45 steps a turn"""
    rnd = random.Random(0x10C)
    ops = [op for op in em.OPCODES if op not in ("jmp", "cjmp", "cnjmp", "answer")]
    body = [("shl", 4, 0, W - 1, False), ("shr", 5, 1, W, False), ("shl", 6, 2, W + 1, False), ("shr", 3, 3, W + 1, False), ("shl", 4, 1, W, False), ("shr", 5, 2, 5, True)]
    while len(body) < 42:
        op = ops[len(body) - 6] if len(body) - 6 < len(ops) else rnd.choice(ops)  # each once, then drawn
        a_is_reg = rnd.random() < 0.5
        a = rnd.randrange(R) if a_is_reg else rnd.choice((0, 1, rnd.randrange(1 << W), (1 << W) - 1, 1 << (W - 1)))
        if op in ("load.w", "store.w"):
            a, a_is_reg = 2 * rnd.randrange(8), False
        body.append((op, rnd.randrange(7), rnd.randrange(R), a, a_is_reg))
    return body + [("add", 7, 7, 1, False), ("cmpe", 7, 0, iterations, False), ("cnjmp", 0, 0, 0, False), ("answer", 0, 0, 0, False)]


@functools.lru_cache(maxsize=None)
def long_trace():
    steps, _ = em.run(W, R, long_program(), [5, 6, 7, 8])
    assert len(steps) == 22 * 45 + 1 and {s.op for s in steps} == set(em.NAMES) - {em.OPCODES["jmp"], em.OPCODES["cjmp"]}
    return steps


def both_entries(field, steps, n):
    pc, inst, a, regs, flags, value = arrays(steps, R)
    b = witness.AdviceBuilder(field, EXE_COLS + CHIP_COLS, n)
    b.exe_table(0, W, R, pc, inst, a, regs, flags, value)
    b.exe_chips(EXE_COLS, W, R, pc, inst, a, regs, flags, value)
    return b.tensor()


def ones_column(field, n, rows):
    return witness.columns_from_ints(field, np.ones(rows, dtype=np.uint8), n)


def test_the_gates_vanish_on_the_columns_of_both_entries():
    field, k, n, table_len = "fp", 10, 1024, 1000
    f = o.FIELDS[field]
    steps = long_trace()
    advice = both_entries(field, steps, n)
    gates = [as_expr(g) for _, g in system().gates]
    prog = expr.compile_gates(field, gates, 0x5EED5EED5EED5EED1234 % f.m)
    ev = expr.GateEvaluator(prog)
    columns = {("advice", i): advice[i] for i in range(advice.shape[0])}
    columns[("fixed", 0)] = ones_column(field, n, table_len)
    assert not host(ev.eval({key: columns[key] for key in prog.columns}, k, 1)).any()
    for cell, bit in (("a_flag", cm.FLAG2), ("r_odd", cm.FLAG3), ("sg_c_sigma", cm.SSUM)):
        at = next(i for i, s in enumerate(steps) if i > 600 and cm.DEFAULT[em.NAMES[s.op]] & bit)
        bad = advice.clone()
        bad[INDEX[cell], at, 0] += 1
        columns.update({("advice", i): bad[i] for i in range(advice.shape[0])})
        rows = host(ev.eval({key: columns[key] for key in prog.columns}, k, 1)).any(axis=1)
        assert np.nonzero(rows)[0].tolist() == [at], cell


# ---- the circuit ---------------------------------------------------------------------------------------------------------------------------------------
CURVE_OF = {"fp": "vesta", "fq": "pallas"}
K, TABLE_LEN, BLINDING = 9, 256, 5


class Setup:
    """the gates and lookups as a circuit at k = 9.  Fixed: 0 s_table (TABLE_LEN rows), 1 the even-bits table (2^(W/2) = 256 rows, 0 behind
    them), 2 / 3 the pow table's values and powers ((i, 2^i) for i <= W, with (W, 2^W); (0, 1) behind them)"""

    def __init__(self, field):
        self.field, self.curve, self.k, self.n = field, CURVE_OF[field], K, 1 << K
        self.names = [name for name, _ in system().gates]
        self.gates = [as_expr(g) for _, g in system().gates]
        t_even, t_value, t_power, out_shift = expr.Fixed(1), expr.Fixed(2), expr.Fixed(3), column_expr("out_shift")
        self.lookups = [(f"even.{cell}", [expr.Fixed(0) * column_expr(s) * column_expr(cell)], [t_even]) for s, cell in cm.System.EVEN_LOOKUPS]
        a, a_shift = column_expr("tv_a"), column_expr("a_shift")
        self.lookups.append(("pow", [out_shift * (a + a_shift * (expr.Constant(W) - a)), out_shift * column_expr("a_power") + expr.Constant(1) - out_shift], [t_value, t_power]))
        self.circuit = Circuit("ExeChips", field, 4, EXE_COLS + CHIP_COLS, 0, self.gates, [(i, t) for _, i, t in self.lookups], [], None)
        self.cs = self.circuit.system()
        self.usable = self.n - (BLINDING + 1)
        fixed = np.zeros((4, self.n), dtype=np.uint64)
        fixed[0, :TABLE_LEN] = 1
        for i in range(1 << (W // 2)):
            fixed[1, i] = sum(((i >> j) & 1) << (2 * j) for j in range(W // 2))
        fixed[3, :] = 1
        for i in range(W + 1):
            fixed[2, i], fixed[3, i] = i, 1 << i
        self.fixed = torch.zeros((4, self.n, 4), dtype=torch.int64, device="cuda")
        for j in range(4):
            witness.columns_from_ints(field, fixed[j], self.n, out=self.fixed[j])
        by_name = {}
        for name, g in zip(self.names, self.gates):
            by_name.setdefault(name, []).append(g)
        self.mock = mock.MockProver(field, self.k, self.usable, list(by_name.items()), self.lookups)

    def failures(self, advice):
        columns = {("advice", i): advice[i] for i in range(advice.shape[0])}
        columns.update({("fixed", j): self.fixed[j] for j in range(4)})
        return self.mock.verify(columns)


@functools.lru_cache(maxsize=None)
def setup(field):
    return Setup(field)


def circuit_trace():
    steps, _ = em.run(W, R, long_program(5), [5, 6, 7, 8])
    assert len(steps) == 5 * 45 + 1 < TABLE_LEN
    return steps


def test_mock_prover_accepts_the_trace_and_names_a_wrong_a_power():
    s = setup("fq")
    assert s.cs.blinding_factors() == BLINDING and TABLE_LEN < s.usable and len(s.lookups) == 21
    steps = circuit_trace()
    advice = both_entries("fq", steps, s.n)
    assert s.failures(advice) == []
    at = next(i for i, st in enumerate(steps) if em.NAMES[st.op] == "shl" and em.operand(st) == W and st.regs[st.rj])
    advice[INDEX["a_power"], at] = 0  # the reference's a_power at A == W
    found = s.failures(advice)
    assert {type(x) for x in found} == {mock.ConstraintNotSatisfied, mock.Lookup} and all(x.row == at for x in found), found
    assert {x.name for x in found} == {"shift", "pow"}


def test_a_whole_proof_is_accepted_by_both_verifiers_and_a_wrong_a_power_is_not_proved():
    s = setup("fp")
    steps = circuit_trace()
    advice = both_entries("fp", steps, s.n)
    params = poly.Params.new(s.curve, s.k)
    vk, pk = plonk.keygen(params, s.cs, s.fixed, [])
    proof = plonk.create_proof_bytes(params, pk, [], advice, api.Rng(bytes([9]) * 32))
    guard = plonk.verify_proof_bytes(params, vk, [], proof)
    assert plonk.single_verify(params, guard)
    pts = lambda rows: np.asarray(rows, dtype=np.uint64).reshape(-1, 8)  # noqa: E731
    g, gl = params._g.download(), params._g_lagrange.download()

    def model_accepts(proof_bytes):
        ok, _, refused = tm.verify(s.curve, s.k, pts(g[:s.n]), pts(gl[:s.n]), pts(g[s.n:s.n + 1])[0], pts(np.asarray(params.u, dtype=np.uint64).reshape(1, 8))[0],
                                   s.circuit.model(), pts(vk.fixed_commitments), pts(vk.sigma_commitments), vk.transcript_repr, [], proof_bytes, group="cpp")
        return ok and refused is None

    assert model_accepts(proof)
    # a wrong a_power: 2^(a + 1) on a shift by a < W - 1 stays in the pow table's powers, but not next to a's value.  The prover's lookup
    # argument finds no table row for the pair (pow is the last of the 21 lookups) and refuses to prove; told to prove anyway, it makes a
    # proof that both verifiers refuse
    at = next(i for i, st in enumerate(steps) if em.NAMES[st.op] in ("shl", "shr") and em.operand(st) < W - 1 and st.regs[st.rj])
    advice[INDEX["a_power"], at] = torch.from_numpy(np.array(o.FIELDS["fp"].limbs(2 << em.operand(steps[at])), dtype=np.uint64).view(np.int64))
    with pytest.raises(api.TrhError, match="an input value of lookup 20 does not occur in its table"):
        plonk.create_proof_bytes(params, pk, [], advice, api.Rng(bytes([9]) * 32))
    bad = plonk.create_proof_bytes(params, pk, [], advice, api.Rng(bytes([9]) * 32), strict_lookups=False)
    assert len(bad) == len(proof) and bad != proof
    with pytest.raises(plonk.VerifyError):
        plonk.verify_proof_bytes(params, vk, [], bad)
    assert not model_accepts(bad)


# ---- another table ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_custom_chips_table():
    """sub's Out bit moved from sum to ssum: the signed words of a and c appear on sub's rows, and b's halves stay (ssum decomposes b too)"""
    moved = dict(cm.DEFAULT, sub=(cm.DEFAULT["sub"] & ~cm.SUM) | cm.SSUM)
    package = dict(exetable.DEFAULT_CHIPS, sub=(exetable.DEFAULT_CHIPS["sub"] & ~exetable.SUM) | exetable.SSUM)
    steps = drawn(16, 8, 2 * T + 1)
    cols, got = compare("fq", 16, 8, steps, 1024, chips=package, model_chips=moved)
    sub = [r for r, s in enumerate(steps) if s.op == em.OPCODES["sub"]]
    assert sub and all(cols["out_ssum"][r] == 1 and cols["out_sum"][r] == 0 for r in sub) and any(cols["sg_a_sigma"][r] for r in sub)
    assert not (host(got) == host(device_chips("fq", 16, 8, steps, 1024))).all()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def filled(R_, n):
    return torch.full((52 + R_, n, 4), FILL, dtype=torch.int64, device="cuda")


def test_refusals_name_the_cause_and_write_nothing():
    steps = drawn(16, 8, 2 * T + 9)
    out = filled(8, 1024)
    with pytest.raises(api.TrhError, match="word_bits 15 is odd"):
        device_chips("fp", 15, 8, steps, out=out)
    with pytest.raises(api.TrhError, match=r"chips\[9\] = 0x[0-9a-f]+ sets flag3 and shift"):
        device_chips("fp", 16, 8, steps, out=out, chips=dict(exetable.DEFAULT_CHIPS, udiv=exetable.DEFAULT_CHIPS["udiv"] | exetable.SHIFT))
    with pytest.raises(api.TrhError, match=r"chips\[23\] = 0x0 and selection's entry are not both known"):
        device_chips("fp", 16, 8, steps, out=out, chips={**exetable.DEFAULT_CHIPS, 23: 0})
    with pytest.raises(api.TrhError, match=r"chips\[10\] = 0xffffffff and selection's entry are not both known"):
        device_chips("fp", 16, 8, steps, out=out, chips={op: v for op, v in exetable.DEFAULT_CHIPS.items() if op != "umod"})
    assert (host(out) == FILL).all()
    # a bad step: the first one is named, in the other entry's words
    bad = list(steps)
    bad[T + 3], bad[90] = bad[T + 3]._replace(pc=1 << 16), bad[90]._replace(rj=8)
    assert em.first_violation(16, 8, bad) == 90
    with pytest.raises(api.TrhError, match="exe_chips_dev: step 90 breaks the table's rules"):
        device_chips("fq", 16, 8, bad, out=out)
    # an opcode both tables leave out refuses the first step that uses it
    at = next(i for i, s in enumerate(steps) if s.op == em.OPCODES["umod"])
    with pytest.raises(api.TrhError, match=f"step {at} "):
        device_chips("fq", 16, 8, steps, out=out, chips={op: v for op, v in exetable.DEFAULT_CHIPS.items() if op != "umod"},
                     selection={op: v for op, v in exetable.DEFAULT_SELECTION.items() if op != "umod"})
    assert (host(out) == FILL).all(), "a refused call writes nothing"


# ---- the remaining entry points ----------------------------------------------------------------------------------------------------------------------------
def test_on_a_non_blocking_stream_behind_a_delay():
    """the inputs become valid on S only behind a delay: an entry that worked on another stream would read the zeros they are prefilled with"""
    from test_gpu_streams import _window
    w = _window()
    steps = drawn(16, 8, T * B + 1)
    n = 2 * T * B
    pc, inst, a, regs, flags, value = arrays(steps, 8)
    real = [torch.from_numpy(x.reshape(-1).view(np.int32)).cuda() for x in (pc, inst, a, regs, witness.pack_bits(flags), value)]
    torch.cuda.synchronize()
    bufs = [torch.zeros_like(r) for r in real]
    out = filled(8, n)
    torch.cuda.synchronize()
    S = w.A
    with torch.cuda.stream(S):
        torch.cuda._sleep(w.ticks)
        for b, r in zip(bufs, real):
            b.copy_(r, non_blocking=True)
    got = exetable.build_chips("fp", 16, 8, bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], bufs[5], out=out, stream=S.cuda_stream, m=len(steps))
    S.synchronize()
    compare("fp", 16, 8, steps, n, got=got)
    assert api.stat("exechips_flag2_rows") == cm.flag2_rows(steps)
    again = exetable.build_chips("fp", 16, 8, real[0], real[1], real[2], real[3], real[4], real[5], n=n, m=len(steps))
    assert (host(again) == host(got)).all()


def test_advice_builder_places_the_columns():
    steps = drawn(16, 8, 100)
    pc, inst, a, regs, flags, value = arrays(steps, 8)
    b = witness.AdviceBuilder("fq", 64, 128)
    got = b.exe_chips(3, 16, 8, pc, inst, a, regs, flags, value)
    alone = device_chips("fq", 16, 8, steps, 128)
    t = host(b.tensor())
    assert (t[3:63] == host(alone)).all() and not t[:3].any() and not t[63:].any() and got.data_ptr() == b.tensor()[3].data_ptr()
    assert api.stat("exechips_rows") == 100


def test_native_driver():
    exe = os.path.join(ROOT, "tests", "native", "exechips_test")
    assert os.path.exists(exe), "tests/native/exechips_test is missing: run `make`"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["test"] == "exechips" and rec["checks_failed"] == 0 and rec["checks"] > 100000
