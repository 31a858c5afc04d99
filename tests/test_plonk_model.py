"""No device: the pieces of tests/plonk_model.py (the independent verifier of tests/test_gpu_plonk.py) against hand computation and direct
evaluation, its view of the two test circuits against tiny_ram_halo2_amd.plonk.ConstraintSystem's, the chain of the product columns as
integers, and -- after `make` -- the registers of the chain kernels (csrc/scan.hip), read from the built code objects through
tools/isa_regs.py in the manner of tests/test_quotient_registers.py."""
import functools
import glob
import importlib.util
import os
import random

import pytest

import pasta as o
import plonk_circuits as pc
import plonk_model as pm
from tiny_ram_halo2_amd import multiopen, plonk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL = lambda kind, c, r=0: ("col", (kind, c), r)  # noqa: E731


def test_degree_and_blinding_factors_by_hand():
    a0, a1, f0 = COL("advice", 0), COL("advice", 1), COL("fixed", 0)
    # nothing but a linear gate: the permutation argument's 3; one query per column: max(3, 1) + 2
    s = pm.System([("sum", a0, ("neg", a1))], [], [], 2)
    assert (s.degree(), s.blinding_factors(), s.chunk_len()) == (3, 5, 1)
    # f0 a0 a0 a1(+1) a1(-1) 7 a1: degree 6; a1 is queried at 0, +1, -1 and, being equality-enabled, stays at three queries; a0 at 0 only
    g = ("prod", ("prod", ("prod", f0, a0), ("prod", a0, COL("advice", 1, 1))), ("prod", COL("advice", 1, -1), ("scaled", a1, 7)))
    s = pm.System([g], [], [("advice", 1), ("advice", 0), ("instance", 0)], 2)
    assert (s.degree(), s.blinding_factors(), s.chunk_len(), s.n_sets()) == (6, 5, 4, 1)
    assert s.queries == {"instance": [(0, 0)], "advice": [(0, 0), (1, 1), (1, -1), (1, 0)], "fixed": [(0, 0)]}
    # four queries of one column: 4 + 2; a lookup with a degree-2 input and a degree-1 table: 2 + 2 + 1; a plain one: 4
    four = ("sum", ("sum", a0, COL("advice", 0, 1)), ("sum", COL("advice", 0, 2), COL("advice", 0, -1)))
    s = pm.System([four], [([("prod", f0, a1)], [f0])], [("advice", 0)], 2)
    assert (s.degree(), s.blinding_factors(), s.chunk_len(), s.n_sets()) == (5, 6, 3, 1)
    assert pm.System([], [([a1], [f0])], [], 2).degree() == 4
    assert pm.System([], [([a1], [f0])], [("advice", 0)] * 9, 2, minimum_degree=6).n_sets() == 3


@pytest.mark.parametrize("name", ["A", "B"])
def test_the_model_and_the_package_read_the_circuits_alike(name):
    c = pc.circuit_a() if name == "A" else pc.circuit_b()
    cs, model = c.system(), c.model()
    assert (cs.degree(), cs.blinding_factors(), cs.chunk_len(), cs.n_sets()) == (model.degree(), model.blinding_factors(), model.chunk_len(), model.n_sets())
    assert cs.degree() == 6 and cs.blinding_factors() == pc.BLINDING and cs.n_sets() == (3 if name == "A" else 0)
    assert cs.queries == model.queries
    plan, queries = cs.eval_plan(), cs.query_plan()
    assert len(set(plan)) == len(plan) and set(queries) == set(plan) and len(queries) == len(plan)


def test_the_package_refuses_what_it_does_not_model():
    from tiny_ram_halo2_amd import expr
    with pytest.raises(ValueError):
        plonk.ConstraintSystem("fp", 1, 1, 0, [expr.Selector(0) * expr.Advice(0)], [], [])
    with pytest.raises(ValueError):
        plonk.ConstraintSystem("fp", 1, 1, 0, [expr.Advice(1)], [], [])
    with pytest.raises(ValueError):
        plonk.ConstraintSystem("fp", 1, 1, 0, [], [([expr.Advice(0)], [])], [])


@pytest.mark.parametrize("field", ["fp", "fq"])
def test_interpolation_against_direct_evaluation(field):
    m = o.FIELDS[field].m
    rng = random.Random(5)
    for count in (1, 2, 3, 4):
        xs = [rng.randrange(m) for _ in range(count)]
        ys = [rng.randrange(m) for _ in range(count)]
        coeffs = pm.interpolate(m, xs, ys)
        assert len(coeffs) == count and [pm.horner(m, coeffs, x) for x in xs] == ys
        assert multiopen.lagrange_interpolate(m, xs, ys) == coeffs
    assert pm.interpolate(m, [3, 5], [7, 11]) == [1, 2]  # 2 X + 1


@pytest.mark.parametrize("field", ["fp", "fq"])
def test_l_i_against_the_definition(field):
    f = o.FIELDS[field]
    m, k = f.m, 3
    n, omega = 1 << k, f.omega(k)
    x = random.Random(6).randrange(m)
    roots = [pow(omega, j, m) for j in range(n)]
    for i in list(range(n)) + [-1, -3]:
        direct = 1
        for j in range(n):
            if j != i % n:
                direct = direct * (x - roots[j]) % m * pow(roots[i % n] - roots[j], -1, m) % m
        assert pm.l_i(m, n, omega, i, x) == direct
    assert sum(pm.l_i(m, n, omega, i, x) for i in range(n)) % m == 1
    assert plonk.lagrange_evals(m, n, omega, x, range(-3, 1)) == [pm.l_i(m, n, omega, i, x) for i in range(-3, 1)]


def test_intermediate_sets_against_the_package():
    x, xw, xi, xl = 100, 101, 99, 77
    queries = [(x, "a"), (x, "b"), (xw, "b"), (xi, "b"), (x, "c"), (x, "z"), (xw, "z"), (xl, "y"), (x, "y"), (xw, "y"), (x, "h"), (xw, "b")]
    with_evals = [(p, key, 1000 * i + 1) for i, (p, key) in enumerate(queries)]
    members, point_sets, claimed = pm.intermediate_sets(with_evals)
    want_members, want_sets = multiopen.construct_intermediate_sets(queries)
    assert members == want_members and point_sets == want_sets
    assert point_sets == [[x], [x, xw, xi], [x, xw], [x, xw, xl]]       # a set's points in order of the points' first appearance, not the key's
    assert members == [("a", 0), ("b", 1), ("c", 0), ("z", 2), ("y", 3), ("h", 0)]
    assert claimed[("b", xw)] == 2001 and claimed[("y", xl)] == 7001    # the first claim of a repeated query
    got, got_sets = multiopen.construct_intermediate_sets_with_evals(with_evals)
    assert got_sets == point_sets and got == [(key, s, [claimed[(key, p)] for p in point_sets[s]]) for key, s in members]


@pytest.mark.parametrize("field", ["fp", "fq"])
def test_the_chain_is_the_set_by_set_definition(field):
    """z_s[0] = z_(s-1)[u], set after set, as the prover's host loop did it: scale set s by the CHAINED value of the set before it"""
    m = o.FIELDS[field].m
    rng = random.Random(7)
    n, link = 8, 5
    for rows in (1, 2, 3, 6):
        z = [[1] + [rng.randrange(1, m) for _ in range(n - 1)] for _ in range(rows)]
        if rows == 6:
            z[3][link] = 0
        want = [list(z[0])]
        for s in range(1, rows):
            start = want[-1][link]
            want.append([v * start % m for v in z[s]])
        got = pm.chain(m, z, link)
        assert got == want
        assert all(got[s][0] == got[s - 1][link] for s in range(1, rows))
        if rows == 6:
            assert all(not any(r) for r in got[4:]) and any(got[3])


# ---- the model's two group backends --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_the_two_groups_give_the_same_sums(curve):
    """sum of scalar * point over 1, 2 and 40 terms, the identity and a repeated point among them; scalars 0, 1 and m - 1 too"""
    import cpu_ref
    cv = o.CURVES[curve]
    m = cv.scalar.m
    py, cpp = pm.GROUPS["python"](curve), pm.GROUPS["cpp"](curve)
    rng = random.Random(41)
    rows = cpu_ref.gen_bases_hashed(curve, 0x51, 40)
    points = [cv.affine_from_limbs(r) for r in rows]
    assert all(cpp.affine(cpp.lift(pt)) == pt for pt in points[:3] + [None])
    for count in (1, 2, 40):
        pts = points[:count]
        if count == 40:
            pts[7], pts[20], pts[21] = None, pts[3], pts[3]
        scalars = [rng.randrange(m) for _ in range(count)]
        if count == 40:
            scalars[0], scalars[1], scalars[2] = 0, 1, m - 1
        want = py.combine(list(zip(scalars, pts)))
        assert want == cv.msm_naive(scalars, pts)
        assert cpp.affine(cpp.combine([(s, cpp.lift(pt)) for s, pt in zip(scalars, pts)])) == want, count
    # a sum that is the identity: s P + (m - s) P
    assert py.combine([(5, points[0]), (m - 5, points[0])]) is None
    assert cpp.affine(cpp.combine([(5, rows[0]), (m - 5, rows[0])])) is None


class _Recorder:
    """the transcript of cpu_ref.ipa_create_proof (limbs in, limb challenges out) that keeps what it saw as the model wants it"""

    def __init__(self, cv):
        from common import LimbTranscript
        self.cv, self.inner, self.points, self.scalars, self.challenges = cv, LimbTranscript(cv.scalar), [], [], []

    def write_point(self, jac):
        self.inner.write_point(jac)
        self.points.append(self.cv.jacobian_limbs_to_affine([int(v) for v in jac]))

    def write_scalar(self, limbs):
        self.inner.write_scalar(limbs)
        self.scalars.append(self.cv.scalar.from_limbs([int(v) for v in limbs]))

    def squeeze_challenge_scalar(self):
        c = self.inner.squeeze_challenge_scalar()
        self.challenges.append(self.cv.scalar.from_limbs([int(v) for v in c]))
        return c


@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_the_two_groups_agree_on_an_opening(curve):
    """an opening of a random polynomial at k = 5 by the C++ prover: both accept it, both refuse it with f + 1 and with c + 1"""
    import cpu_ref
    import numpy as np
    cv = o.CURVES[curve]
    fs, k = cv.scalar, 5
    m, n = fs.m, 32
    rng = random.Random(43)
    lim = lambda v: np.array(fs.limbs(v % m), dtype=np.uint64)  # noqa: E731
    g_l, w_l, u_l = cpu_ref.gen_bases_hashed(curve, 0x61, n), cpu_ref.gen_bases_hashed(curve, 0x62, 1)[0], cpu_ref.gen_bases_hashed(curve, 0x63, 1)[0]
    p, blind, x3 = [rng.randrange(m) for _ in range(n)], rng.randrange(m), rng.randrange(m)
    s_poly, s_blind = [rng.randrange(m) for _ in range(n)], rng.randrange(m)
    arr = lambda poly: np.array([fs.limbs(c) for c in poly], dtype=np.uint64)  # noqa: E731
    tr = _Recorder(cv)
    c, f = cpu_ref.ipa_create_proof(curve, k, g_l, w_l, u_l, lambda: lim(rng.randrange(m)), tr, arr(p), lim(blind), lim(x3), arr(s_poly), lim(s_blind))
    c, f = fs.from_limbs(c), fs.from_limbs(f)
    assert len(tr.points) == 1 + 2 * k and len(tr.challenges) == 2 + k
    v = pm.horner(m, p, x3)
    rounds = [(tr.points[1 + 2 * j], tr.points[2 + 2 * j]) for j in range(k)]
    xi, z, challenges = tr.challenges[0], tr.challenges[1], tr.challenges[2:]
    py, cpp = pm.GROUPS["python"](curve), pm.GROUPS["cpp"](curve)
    pts = lambda rows: [cv.affine_from_limbs(r) for r in rows]  # noqa: E731
    g, w, u = pts(g_l), pts([w_l])[0], pts([u_l])[0]
    commitment = py.combine(list(zip(p + [blind], g + [w])))
    assert cpp.affine(cpp.combine(list(zip(p + [blind], list(g_l) + [w_l])))) == commitment
    for c_, f_, want in ((c, f, True), (c, (f + 1) % m, False), ((c + 1) % m, f, False)):
        assert py.opening_holds(k, g, w, u, commitment, x3, v, tr.points[0], xi, z, rounds, challenges, c_, f_) is want
        got = cpp.opening_holds(k, g_l, w_l, u_l, cpp.lift(commitment), x3, v, cpp.lift(tr.points[0]), xi, z,
                                [(cpp.lift(l), cpp.lift(r)) for l, r in rounds], challenges, c_, f_)
        assert got is want


# ---- the witnesses of tests/test_gpu_plonk_sizes.py ----------------------------------------------------------------------------------------
def _column_values(m, node, columns, n):
    """an expression on every row at once: the oracle's evaluate_expression, column by column"""
    tag = node[0]
    if tag == "const":
        return [node[1] % m] * n
    if tag == "col":
        col, r = columns[node[1]], node[2] % n
        return col[r:] + col[:r]
    a = _column_values(m, node[1], columns, n)
    if tag == "neg":
        return [-x % m for x in a]
    if tag == "scaled":
        return [x * node[2] % m for x in a]
    b = _column_values(m, node[2], columns, n)
    return [(x + y) % m for x, y in zip(a, b)] if tag == "sum" else [x * y % m for x, y in zip(a, b)]


def unsatisfied(circuit, k, advice, fixed, instances, copies):
    """-> what the witness breaks, as (kind, index, row): every gate on every usable row, every copy, every lookup input in its table"""
    m, n, u = o.FIELDS[circuit.field].m, 1 << k, pc.usable(k)
    model = circuit.model()
    columns = {("advice", i): list(c) for i, c in enumerate(advice)}
    columns.update({("fixed", i): list(c) for i, c in enumerate(fixed)})
    columns.update({("instance", i): list(c) + [0] * (n - len(c)) for i, c in enumerate(instances)})
    assert all(len(c) == n for c in columns.values())
    bad = []
    for i, g in enumerate(model.gates):
        bad += [("gate", i, row) for row, v in enumerate(_column_values(m, g, columns, n)[:u]) if v]
    for i, (inputs, tables) in enumerate(model.lookups):
        table = set(zip(*[_column_values(m, e, columns, n)[:u] for e in tables]))
        bad += [("lookup", i, row) for row, v in enumerate(zip(*[_column_values(m, e, columns, n)[:u] for e in inputs])) if v not in table]
    for i, (c0, r0, c1, r1) in enumerate(copies):
        if columns[model.permutation_columns[c0]][r0] != columns[model.permutation_columns[c1]][r1] or max(r0, r1) >= u:
            bad.append(("copy", i, r0))
    return bad


def test_the_column_evaluator_is_the_oracles():
    m = o.FIELDS["fq"].m
    w = pc.WitnessA("fq")
    columns = {("advice", i): c for i, c in enumerate(w.advice)}
    columns.update({("fixed", i): c for i, c in enumerate(w.fixed)})
    for g in pc.circuit_a("fq").model().gates:
        assert _column_values(m, g, columns, 32) == [o.evaluate_expression(o.FIELDS["fq"], g, columns, row, 32, 1) for row in range(32)]


@functools.lru_cache(maxsize=None)
def witness_a(k):
    return pc.WitnessA("fq", k)


@functools.lru_cache(maxsize=None)
def witness_b(k):
    return pc.witness_b("fp", k)


@pytest.mark.parametrize("k", [5, 10, 14])
def test_witness_a_satisfies_its_circuit(k):
    w, circuit = witness_a(k), pc.circuit_a("fq")
    assert unsatisfied(circuit, k, w.advice, w.fixed, [w.instance], w.copies) == []
    if k == 5:
        return
    # and the check sees one cell of each kind change: the Rotation(+1) gate's cell on the last usable row, one end of a copy, a lookup input
    u = pc.usable(k)
    adv = [list(c) for c in w.advice]
    adv[2][u - 1] += 1
    assert unsatisfied(circuit, k, adv, w.fixed, [w.instance], w.copies) == [("gate", 1, u - 1)]
    column, row = w.copied_cell(tail=256)
    adv = [list(c) for c in w.advice]
    adv[column][row] += 1
    assert {b[0] for b in unsatisfied(circuit, k, adv, w.fixed, [w.instance], w.copies)} == {"copy"}
    row = w.free_cell(5, tail=256)
    adv = [list(c) for c in w.advice]
    adv[5][row] += 1
    assert unsatisfied(circuit, k, adv, w.fixed, [w.instance], w.copies) == [("lookup", 1, row)]


@pytest.mark.parametrize("k", [5, 10, 14])
def test_witness_b_satisfies_its_circuit(k):
    advice, fixed = witness_b(k)
    circuit, u = pc.circuit_b("fp"), pc.usable(k)
    assert unsatisfied(circuit, k, advice, fixed, [], []) == []
    cols = dict(zip(pc.ADV_B, advice))
    enabled = {op: [r for r in range(u) if fixed[0][r] and cols["s_" + op][r]] for op in ("and", "xor", "or")}
    assert fixed[0] == [1] * (u - 3) + [0] * ((1 << k) - u + 3)
    if k > 5:  # the chip is at work up to the last 256 usable rows, where the broken-witness cases of the size tests sit
        assert all(rows[-1] >= u - 256 and len(rows) > u // 8 for rows in enabled.values())
    broken = [list(c) for c in advice]
    broken[pc.ADV_B.index("res")][enabled["xor"][-1]] += 1
    assert unsatisfied(circuit, k, broken, fixed, [], []) == [("gate", 7, enabled["xor"][-1])]
    broken = [list(c) for c in advice]
    assert not broken[pc.ADV_B.index("a_e")][enabled["and"][-1]] & 2
    broken[pc.ADV_B.index("a_e")][enabled["and"][-1]] |= 2
    assert ("lookup", 0, enabled["and"][-1]) in unsatisfied(circuit, k, broken, fixed, [], [])


@pytest.mark.parametrize("k,block", [(10, 256), (14, 4096)])
def test_witness_a_holds_what_its_docstring_names(k, block):
    w = witness_a(k)
    n, u = 1 << k, pc.usable(k)
    assert pc.cycle_block(k) == block and len(w.copies) >= n // 8 + 3
    # the four-cell cycle: these cells and no others, in all three permutation sets (columns 0..3 | 4..7 | 8), rows in different blocks
    assert w.cycle == [(3, 0), (6, block - 1), (pc.INSTANCE_COLUMN, block), (7, u - 1)]
    assert [c // 4 for c, _ in w.cycle] == [0, 1, 2, 1]
    assert [r // block for _, r in w.cycle] == [0, 0, 1, (u - 1) // block] and (u - 1) // block == n // block - 1 >= 3
    import permkeygen_model
    asm = permkeygen_model.Assembly(9, k)
    assert all(asm.copy(*c) for c in w.copies)
    cell = lambda column, row: column * n + row  # noqa: E731
    assert frozenset(cell(*c) for c in w.cycle) in permkeygen_model.cycles(asm.mapping)
    value = w.advice[3][0]
    assert w.advice[6][block - 1] == w.advice[7][u - 1] == w.instance[block] == value
    assert sum(col.count(value) for col in w.advice[:8] + [w.instance]) == 4
    # copies that cross the sets and the blocks beside it
    real = [c for c in w.copies if c[:2] != c[2:]]
    assert {(0, 1), (0, 2), (1, 2)} <= {tuple(sorted((c[0] // 4, c[2] // 4))) for c in real} and any(c[1] // block != c[3] // block for c in real)
    # the gates: Rotation(+1) enabled on the last usable row, where it reads row u of F2; Rotation(-1) from row 1
    assert w.fixed[1][u - 1] == 1 and w.fixed[1][u] == 0 and w.fixed[2][u] != 0 and w.fixed[3][:3] == [0, 1, 1] and w.fixed[3][u - 1] == 1
    # the lookups: every usable row of the tables filled, in another order than the inputs; one input value twice; one table value unused
    a4, t1 = w.advice[4][:u], w.fixed[4][:u]
    assert a4 != t1 and len(t1) == u and len(set(a4)) < u and len(set(t1) - set(a4)) == 1 and set(a4) <= set(t1)
    pairs, table = list(zip(w.advice[5][:u], w.advice[9][:u])), list(zip(w.fixed[5][:u], w.fixed[6][:u]))
    assert pairs != table and sorted(pairs) == sorted(table)
    # the cells the broken-witness cases change lie in the last 256 usable rows; the gate's cell on the last row is tied to nothing
    assert w.free_cell(5, tail=256) >= u - 256 and w.copied_cell(tail=256)[1] >= u - 256 and w.copied_cell(tail=256)[0] in (6, 7)
    assert (2, u - 1) not in w._tied() and (5, w.free_cell(5, tail=256)) not in w._tied()


# ---- the chain kernels' registers ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def registers():
    assert glob.glob(os.path.join(ROOT, "tiny-ram-halo2_amd", "csrc", "*.o")), "no objects in csrc/: run `make`"
    spec = importlib.util.spec_from_file_location("isa_regs", os.path.join(ROOT, "tools", "isa_regs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect(count_instructions=False)


@pytest.mark.parametrize("field", ["Fp", "Fq"])
def test_the_chain_kernels_use_no_scratch(registers, field):
    """the pass is a load, one multiplication and a store per element and lives on memory latency: at most 64 VGPRs keep eight waves per SIMD
    resident (the register file holds 512 per lane); the one-workgroup carry launch keeps its scan in LDS (256 elements of 36 bytes)"""
    for kernel, lds, vgpr_limit in (("chain_apply_kernel", 0, 64), ("chain_carries_kernel", 256 * 36, 128)):
        name = f"{kernel}<{field}>"
        assert name in registers, f"{name} not found among {len(registers)} kernels"
        r = registers[name]
        print(name, r)
        assert r["scratch"] == 0, f"{name} uses scratch memory: {r}"
        assert r["lds"] == lds and 0 < r["vgpr"] <= vgpr_limit, r
