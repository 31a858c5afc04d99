"""CPU only: tests/ipa_exponent_model.py against the big-int restatement of the Rust prover, oracle/pasta.py::ipa_create_proof, over the
same multiples of the generator -- transcript item for item, for k = 3, 4, 5 on both curves, with generators that are all equal, that
are +-P, 2 P and the identity, and that are distinct.  The GPU tests of tests/test_gpu_ipa_collisions.py rest on this model."""
import random

import numpy as np
import pytest

import ipa_exponent_model as X
import pasta as o
from common import OracleTranscript

SETS = ["all-equal", "pm-one-two-zero", "distinct"]


def generator_logs(which, n, q, rnd):
    if which == "all-equal":
        return [7] * n
    if which == "pm-one-two-zero":
        logs = [1, q - 1, 2, 0] + [rnd.choice([1, q - 1, 2, 0]) for _ in range(n - 4)]
        return logs
    logs = [rnd.randrange(1, q) for _ in range(n)]
    assert len(set(logs)) == n
    return logs


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("k", [3, 4, 5])
@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_exponent_model_writes_the_oracles_transcript(curve, k, which):
    cv = o.CURVES[curve]
    fs, q, n = cv.scalar, cv.scalar.m, 1 << k
    rnd = random.Random(0xE4B0 + 16 * k + SETS.index(which))
    a = generator_logs(which, n, q, rnd)
    # w = g_0 and u = -g_0 once, unrelated multiples otherwise
    omega, upsilon = (a[0], q - a[0]) if which == "all-equal" and k == 4 else (rnd.randrange(1, q), rnd.randrange(1, q))
    p_poly, s_poly = [rnd.randrange(q) for _ in range(n)], [rnd.randrange(q) for _ in range(n)]
    if k == 5:  # zero and repeated coefficients next to the random ones
        p_poly[3] = p_poly[n - 1] = 0
        s_poly[5] = s_poly[6]
    p_blind, s_blind, x3 = rnd.randrange(q), rnd.randrange(q), rnd.randrange(q)
    draws = [rnd.randrange(q) for _ in range(2 * k)]
    point = lambda log: cv.mul(log, cv.generator) if log % q else None  # noqa: E731

    it = iter(draws)
    t_ref = OracleTranscript(cv)
    c_ref, f_ref = o.ipa_create_proof(cv, k, [point(v) for v in a], point(omega), point(upsilon), lambda: next(it), t_ref,
                                      p_poly, p_blind, x3, s_poly, s_blind)
    it = iter(draws)
    t_mod = X.LogTranscript(fs, lambda log: np.array(cv.affine_limbs(point(log)), dtype=np.uint64))
    got = X.create_proof(q, k, a, omega, upsilon, lambda: next(it), t_mod, p_poly, p_blind, x3, s_poly, s_blind)
    assert len(t_mod.log) == len(t_ref.log) == 1 + 2 * k + 2
    for i, (x, y) in enumerate(zip(t_mod.log, t_ref.log)):
        assert x == y, f"transcript item {i} ({got.items()[i][0]})"
    assert (got.c, got.f) == (c_ref, f_ref)
    assert [name for name, _ in got.items()] == ["S"] + [f"{side}_{j}" for j in range(k) for side in "LR"] + ["c", "f"]
    # the scalar rows the cases of tests/ipa_collision_cases.py are built from are the MSMs of S, L_0 and R_0
    full = [v % q for v in a] + [omega, upsilon]
    assert X.dot(got.row_s, full, q) == got.S and X.dot(got.row_l0, full, q) == got.L[0] and X.dot(got.row_r0, full, q) == got.R[0]
    if which == "all-equal":  # the collapsed generators all coincide: a' = a_0 prod (1 + u_j) at every index
        assert got.S == (7 * sum(got.row_s[:n]) + s_blind * omega) % q
