"""trh_exe_table_dev (tiny_ram_halo2_amd.exetable, csrc/exetable.hip): the steps of a trace into the 28 + 9 reg_count columns of the Exe
table.  Every column is compared word for word with tests/exetable_model.py (Python integers -> oracle/pasta.py's Montgomery limbs).
T = 256 is the rows per workgroup of the row kernel.

  word for word  steps drawn independently, W = 16, R = 8, m in {1, 2, 31, 32, 33, T - 1, T, T + 1, 2 T + 1} with n the next power of two above m
                 (the flag bitmap's word boundary, the successor read across a workgroup's edge, the zero rows) and m = n - 1; Fp and Fq
  extremes       W = 32, R in {1, 16}, m = T + 1: pc + 1 = 2^32, 0xFFFFFFFF squared, shifts by 0 and 32 (the negative value), equal comparands,
                 division by zero
  the gates      the 90 gates of tests/golden/exe_tempvar_gates.json through expr.compile_gates / GateEvaluator on the device-built columns
                 (n = 1024, m = 700, s_table on 800 rows): zero on every row; one corrupted cell gives exactly its row
  the circuit    the interpreter's traces through mock.MockProver on a circuit of those gates; one proof at k = 7 accepted by the package's
                 verifier and by tests/plonk_model.py
  another table  one opcode's b moved to another legal source: the model's columns for that table
  refusals       an unknown opcode, ri / rj / a register operand at reg_count, a pc / a / register / value at 2^W, a last step that does not
                 answer: the first bad step is named and a sentinel-filled destination stays as it was
  the rest       the caller's stream behind a delay, AdviceBuilder.exe_table, trh_stat, tests/native/exetable_test.cpp over include/trh.hpp"""
import functools
import json
import os
import random
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import exetable_model as em
import pasta as o
import transcript_model as tm
from plonk_circuits import Circuit
from tiny_ram_halo2_amd import api, exetable, expr, mock, plonk, poly, witness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "exe_tempvar_gates.json")
T = exetable.ROWS_PER_WORKGROUP
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


def device_build(field, W, R, steps, n=None, **kw):
    pc, inst, a, regs, flags, value = arrays(steps, R)
    return exetable.build(field, W, R, pc, inst, a, regs, flags, value, n=n, **kw)


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


def compare(field, W, R, steps, n, got=None, selection=None, model_selection=em.DEFAULT):
    """the device's table against the model's, every cell"""
    cols = em.build(W, R, steps, n, model_selection)
    got = device_build(field, W, R, steps, n, selection=selection) if got is None else got
    assert api.stat("exetable_rows") == len(steps)
    cells, want = host(got).view(np.uint64), expected_limbs(field, cols, n)
    assert cells.shape == want.shape == (28 + 9 * R, n, 4)
    if not (cells == want).all():
        c, r = [int(x[0]) for x in np.nonzero((cells != want).any(axis=2))]
        raise AssertionError(f"column {em.columns(R)[c]}, row {r} of {len(steps)} (n = {n}), step {steps[r] if r < len(steps) else None}: {cells[c, r]} for {want[c, r]} = {cols[c][r]}")
    return cols, got


@functools.lru_cache(maxsize=None)
def drawn(W, R, m, seed=0):
    return em.random_steps(random.Random(1000 * W + 10 * R + m + seed), W, R, m)


SIZES = [(m, 1 << m.bit_length()) for m in (1, 2, 31, 32, 33, T - 1, T, T + 1, 2 * T + 1)] + [(127, 128)]


# ---- word for word -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("m,n", SIZES)
def test_word_for_word_against_the_model(field, m, n):
    assert m < n and (n == m + 1 or n & (n - 1) == 0)
    compare(field, 16, 8, drawn(16, 8, m), n)


@pytest.mark.parametrize("field,R", [("fp", 1), ("fq", 16), ("fq", 1), ("fp", 16)])
def test_the_extreme_words_at_32_bits(field, R):
    steps = em.extreme_steps(R, T + 1)
    assert len(steps) == T + 1
    cols, _ = compare(field, 32, R, steps, 2 * T)
    names = em.columns(R)
    td, tb, tc = (cols[names.index(x)] for x in ("tv_d", "tv_b", "tv_c"))
    top = 0xFFFFFFFF
    assert 1 << 32 in td and 1 << 32 in tb and -top * top in td and top << 32 in td and top - 1 in tc   # pc + 1; shr by 0 and by 32; the square's high word


# ---- the gates on the device ------------------------------------------------------------------------------------------------------------------------
def fixture():
    with open(FIXTURE) as fh:
        doc = json.load(fh)
    assert doc["reg_count"] == 8 and doc["word_bits"] == 16 and len(doc["gates"]) == 90
    return doc


def as_fixed(j):
    """the fixture's expression over Advice columns and its two selectors as Fixed(0) = first_line, Fixed(1) = s_table"""
    tag = j[0]
    if tag == "const":
        return expr.Constant(int(j[1], 16))
    if tag == "advice":
        return expr.Advice(j[1], j[2])
    if tag == "selector":
        return expr.Fixed(j[1])
    if tag == "neg":
        return expr.Negated(as_fixed(j[1]))
    if tag == "scaled":
        return expr.Scaled(as_fixed(j[1]), int(j[2], 16))
    return {"sum": expr.Sum, "prod": expr.Product}[tag](as_fixed(j[1]), as_fixed(j[2]))


def fixed_columns(field, n, table_len):
    fixed = torch.zeros((2, n, 4), dtype=torch.int64, device="cuda")
    witness.columns_from_ints(field, np.ones(1, dtype=np.uint8), n, out=fixed[0])
    witness.columns_from_ints(field, np.ones(table_len, dtype=np.uint8), n, out=fixed[1])
    return fixed


def test_the_gates_vanish_on_the_device_built_columns():
    field, k, m, table_len = "fp", 10, 700, 800
    f, n = o.FIELDS[field], 1 << 10
    doc = fixture()
    gates = [as_fixed(g["expr"]) for g in doc["gates"]]
    steps = drawn(16, 8, m)
    cols = device_build(field, 16, 8, steps, n)
    fixed = fixed_columns(field, n, table_len)
    prog = expr.compile_gates(field, gates, 0x5EED5EED5EED5EED1234 % f.m)
    ev = expr.GateEvaluator(prog)
    columns = {("advice", i): cols[i] for i in range(len(doc["advice"]))}
    columns.update({("fixed", j): fixed[j] for j in range(2)})
    assert set(prog.columns) == set(columns)
    assert not host(ev.eval({key: columns[key] for key in prog.columns}, k, 1)).any()
    # one cell: tv_b of a row whose b is a register of the row itself
    at = next(i for i, s in enumerate(steps) if i > 300 and em.DEFAULT[em.NAMES[s.op]][1] == em.REG_RJ)
    bad = cols.clone()
    bad[em.columns(8).index("tv_b"), at, 0] += 1
    columns.update({("advice", i): bad[i] for i in range(len(doc["advice"]))})
    rows = host(ev.eval({key: columns[key] for key in prog.columns}, k, 1)).any(axis=1)
    assert np.nonzero(rows)[0].tolist() == [at]


# ---- the circuit ---------------------------------------------------------------------------------------------------------------------------------------
CURVE_OF = {"fp": "vesta", "fq": "pallas"}
K, TABLE_LEN, BLINDING = 7, 110, 5
PROGRAMS = {"load_store": (em.reference_load_store, [1]), "load_answer": (em.reference_load_answer, [1]), "loop": (em.loop_program, []),
            "every_opcode": (em.every_opcode_program, [3, 5])}


class Setup:
    """the 90 gates as a circuit at k = 7: two fixed columns (first_line, s_table on TABLE_LEN rows), the 100 advice columns the entry writes"""

    def __init__(self, field):
        doc = fixture()
        self.field, self.curve, self.k, self.n = field, CURVE_OF[field], K, 1 << K
        self.gates = [as_fixed(g["expr"]) for g in doc["gates"]]
        self.names = [g["name"] for g in doc["gates"]]
        self.circuit = Circuit("ExeTempVars", field, 2, 28 + 9 * 8, 0, self.gates, [], [], None)
        self.cs = self.circuit.system()
        self.usable = self.n - (BLINDING + 1)
        self.fixed = fixed_columns(field, self.n, TABLE_LEN)
        by_name = {}
        for name, g in zip(self.names, self.gates):
            by_name.setdefault(name, []).append(g)
        self.mock = mock.MockProver(field, self.k, self.usable, list(by_name.items()), [])

    def advice(self, steps):
        b = witness.AdviceBuilder(self.field, 28 + 9 * 8, self.n)
        pc, inst, a, regs, flags, value = arrays(steps, 8)
        b.exe_table(0, 16, 8, pc, inst, a, regs, flags, value)
        return b.tensor()

    def failures(self, advice):
        columns = {("advice", i): advice[i] for i in range(advice.shape[0])}
        columns.update({("fixed", j): self.fixed[j] for j in range(2)})
        return self.mock.verify(columns)


@functools.lru_cache(maxsize=None)
def setup(field):
    return Setup(field)


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_mock_prover_on_the_interpreters_traces(name):
    s = setup("fq")
    assert s.cs.blinding_factors() == BLINDING and TABLE_LEN < s.usable
    make, tape = PROGRAMS[name]
    steps, _ = em.run(16, 8, make(), tape)
    advice = s.advice(steps)
    assert s.failures(advice) == []
    if name == "every_opcode":   # and a cell that no longer equals its source is named with its gate and row
        at = next(i for i, st in enumerate(steps) if st.op == em.OPCODES["mull"])
        advice[em.columns(8).index("tv_d"), at, 0] += 1
        found = s.failures(advice)
        assert found and all(isinstance(f, mock.ConstraintNotSatisfied) and f.row == at and f.name.startswith("tv.d.reg_next") for f in found), found


def test_a_whole_proof_is_accepted_by_both_verifiers():
    s = setup("fp")
    steps, _ = em.run(16, 8, em.every_opcode_program(), [3, 5])
    advice = s.advice(steps)
    assert s.failures(advice) == []
    params = poly.Params.new(s.curve, s.k)
    vk, pk = plonk.keygen(params, s.cs, s.fixed, [])
    proof = plonk.create_proof_bytes(params, pk, [], advice, api.Rng(bytes([9]) * 32))
    guard = plonk.verify_proof_bytes(params, vk, [], proof)
    assert plonk.single_verify(params, guard)
    pts = lambda rows: np.asarray(rows, dtype=np.uint64).reshape(-1, 8)  # noqa: E731
    g, gl = params._g.download(), params._g_lagrange.download()
    ok, _, refused = tm.verify(s.curve, s.k, pts(g[:s.n]), pts(gl[:s.n]), pts(g[s.n:s.n + 1])[0], pts(np.asarray(params.u, dtype=np.uint64).reshape(1, 8))[0],
                               s.circuit.model(), pts(vk.fixed_commitments), pts(vk.sigma_commitments), vk.transcript_repr, [], proof, group="cpp")
    assert ok and refused is None


# ---- another table ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_custom_selection_table():
    """add's b from reg[rj] to reg[ri], sub's b to pc + 1: the model's columns for that table, and not the default's"""
    moved = dict(em.DEFAULT, add=(em.A, em.REG_RI, em.REG_NEXT_RI, em.ZERO), sub=(em.A, em.PC_PLUS_ONE, em.REG_RJ, em.ZERO))
    package = dict(exetable.DEFAULT_SELECTION, add=(exetable.A, exetable.REG_RI, exetable.REG_NEXT_RI, exetable.ZERO),
                   sub=(exetable.A, exetable.PC_PLUS_ONE, exetable.REG_RJ, exetable.ZERO))
    steps = drawn(16, 8, 2 * T + 1)
    _, got = compare("fq", 16, 8, steps, 1024, selection=package, model_selection=moved)
    assert not (host(got) == host(device_build("fq", 16, 8, steps, 1024))).all()
    # a table that leaves an opcode out refuses the first step that uses it
    partial = {op: v for op, v in exetable.DEFAULT_SELECTION.items() if op != "umod"}
    at = next(i for i, s in enumerate(steps) if s.op == em.OPCODES["umod"])
    out = filled(8, 1024)
    with pytest.raises(api.TrhError, match=f"step {at} "):
        device_build("fq", 16, 8, steps, out=out, selection=partial)
    assert (host(out) == FILL).all()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def filled(R, n):
    return torch.full((28 + 9 * R, n, 4), FILL, dtype=torch.int64, device="cuda")


def refused(W, R, steps, index, field="fq"):
    n = 1 << len(steps).bit_length()
    out = filled(R, n)
    with pytest.raises(api.TrhError, match=f"step {index} "):
        device_build(field, W, R, steps, out=out)
    assert (host(out) == FILL).all(), "a refused call writes nothing"
    assert em.first_violation(W, R, steps) == index


def test_refusals_name_the_first_step_and_write_nothing():
    R = 4
    good = drawn(16, R, 2 * T + 9)
    assert em.first_violation(16, R, good) is None
    with_reg = next(i for i, s in enumerate(good) if i > T and s.a_is_reg)
    changes = [(T + 3, dict(op=23)), (5, dict(op=30)), (T - 1, dict(ri=R)), (T, dict(rj=R)), (with_reg, dict(a=R)), (40, dict(pc=1 << 16)),
               (2 * T + 1, dict(a=1 << 16, a_is_reg=False)), (77, dict(value=1 << 16)), (0, dict(regs=(0, 0, 0, 1 << 16))), (2 * T + 7, dict(regs=(1 << 16, 0, 0, 0))),
               (len(good) - 1, dict(op=em.OPCODES["jmp"]))]
    for at, change in changes:
        steps = list(good)
        steps[at] = steps[at]._replace(**change)
        refused(16, R, steps, at)
    steps = list(good)   # two bad steps: the first one is named
    steps[300], steps[90] = steps[300]._replace(pc=1 << 16), steps[90]._replace(op=24)
    refused(16, R, steps, 90)
    # at 32 bits no word can be too large: only the structure is left to refuse
    wide = list(em.extreme_steps(R, T + 1))
    wide[T - 2] = wide[T - 2]._replace(rj=R, ri=0)
    refused(32, R, wide, T - 2, field="fp")
    # the shape: m == 0 and m >= n
    out = filled(R, 64)
    pc, inst, a, regs, flags, value = arrays(good[:64], R)
    for m in (0, 64):
        with pytest.raises(api.TrhError, match="steps do not fit"):
            exetable.build("fp", 16, R, pc[:m], inst[:m], a[:m], regs[:m], flags[:m], value[:m], out=out)
    assert (host(out) == FILL).all()


# ---- the remaining entry points ----------------------------------------------------------------------------------------------------------------------------
def test_on_a_non_blocking_stream_behind_a_delay():
    """the inputs become valid on S only behind a delay: an entry that worked on another stream would read the zeros they are prefilled with"""
    from test_gpu_streams import _window
    w = _window()
    steps = drawn(16, 8, T + 1)
    pc, inst, a, regs, flags, value = arrays(steps, 8)
    real = [torch.from_numpy(x.reshape(-1).view(np.int32)).cuda() for x in (pc, inst, a, regs, witness.pack_bits(flags), value)]
    torch.cuda.synchronize()
    bufs = [torch.zeros_like(r) for r in real]
    out = filled(8, 2 * T)
    torch.cuda.synchronize()
    S = w.A
    with torch.cuda.stream(S):
        torch.cuda._sleep(w.ticks)
        for b, r in zip(bufs, real):
            b.copy_(r, non_blocking=True)
    got = exetable.build("fp", 16, 8, bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], bufs[5], out=out, stream=S.cuda_stream, m=len(steps))
    S.synchronize()
    compare("fp", 16, 8, steps, 2 * T, got=got)
    # device tensors on the current stream give what numpy arrays give
    again = exetable.build("fp", 16, 8, real[0], real[1], real[2], real[3], real[4], real[5], n=2 * T, m=len(steps))
    assert (host(again) == host(got)).all()


def test_advice_builder_places_the_table():
    steps = drawn(16, 8, 100)
    pc, inst, a, regs, flags, value = arrays(steps, 8)
    b = witness.AdviceBuilder("fq", 104, 128)
    got = b.exe_table(3, 16, 8, pc, inst, a, regs, flags, value)
    alone = device_build("fq", 16, 8, steps, 128)
    t = host(b.tensor())
    assert (t[3:103] == host(alone)).all() and not t[:3].any() and not t[103:].any() and got.data_ptr() == b.tensor()[3].data_ptr()
    assert api.stat("exetable_rows") == 100


def test_native_driver():
    exe = os.path.join(ROOT, "tests", "native", "exetable_test")
    assert os.path.exists(exe), "tests/native/exetable_test is missing: run `make`"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["test"] == "exetable" and rec["checks_failed"] == 0 and rec["checks"] > 200000
