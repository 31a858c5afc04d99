"""No device: the pieces of tests/plonk_model.py (the independent verifier of tests/test_gpu_plonk.py) against hand computation and direct
evaluation, its view of the two test circuits against tiny_ram_halo2_amd.plonk.ConstraintSystem's, the chain of the product columns as
integers, and -- after `make` -- the registers of the chain kernels (csrc/scan.hip), read from the built code objects through
tools/isa_regs.py in the manner of tests/test_quotient_registers.py."""
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
