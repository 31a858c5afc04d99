"""GPU tests (-m gpu): the MSM route of the IPA opening (csrc/ipa.hip sets MsmFlags::dense_hint for the commitment to s' and for every
round's L / R pair) on generators that collide.

With that flag csrc/msm.hip takes the lean sort (no chunked fallback launches; `lean_gate` is non-null in msm_accumulate_seg_kernel, in the
combine and in the window-sum kernels), combines the pieces of a bucket with one DPP quad (msm_combine_q4_kernel, with its own choice between
`first`, `direct` and `last` and its own hand-over to msm_combine_heavy_kernel), and runs the MSM again with force_fallback when a bin
overflows.  The other tests of trh_ipa_create_proof use unstructured generators and random polynomials, so this route never saw an identity
piece, two equal or opposite pieces, a bucket of identical points or an all-zero scalar row.  Here every generator is a KNOWN multiple of the
curve generator (w and u too), so the whole opening is integers mod the group order (tests/ipa_exponent_model.py, pinned to
oracle/pasta.py::ipa_create_proof by tests/test_ipa_exponent_model.py): every test compares the device's WHOLE transcript -- S, every L_j and
R_j, c, f -- with that model, limb for limb (Z included: the Montgomery one, or all zero for the identity), then lets the oracle's verifier
equation judge what the GPU produced, and compares with the literal C++ prover (cpu_ref.ipa_create_proof) as well.

  * the designed cases of tests/ipa_collision_cases.py at k = 14 with tables: the commitment to s' and round 0 are MSMs designed entry by
    entry; tests/test_msm_events_model.py proves on the CPU which events each meets in which stage.  trh_stat proves the route: three lean
    sorts and three quad combines (S, rounds 0 and 1), no retry, one generator collapse, twelve one-launch rounds behind it;
  * duplicate generators (all equal; P, -P alternating; a_i in {1, -1, 2, 0} at random; w = g_0 and u = -g_0) under random full-size p and s:
    k = 5 and 13 with tables (msm_small_kernel over level 0 of the table), k = 14 with tables (after the collapse the generators all
    coincide: msm_small_kernel over 4096 copies of one point; a random s(X) always overflows bin 0 of this table's sort, see _route, so
    these openings also run the retry) and k = 14 without (the per-window pipeline: 32 bucket sets, lean sort, msm_combine_kernel<4> under
    the gate);
  * the polynomial of test_ipa_skewed_polynomial_takes_the_chunked_sort_again over duplicates: the overflow and the retry;
  * degenerate rows: p = 0 and s = 0; p with one non-zero coefficient at 0, half - 1, half, n - 1.

The transcript assertions are unconditional; the route assertions depend on the options reduce_q4, bin_sort and ipa_fold.  test_gpu_q4.py runs
this file again with TRH_REDUCE_Q4=0: the combine is then msm_combine_kernel<4> under the gate and msm_quad_combines stays 0."""
import random

import numpy as np
import pytest
import torch

import cpu_ref
import ipa_collision_cases as I
import ipa_exponent_model as X
import msm_events_model as M
import pasta as o
from common import DeviceTranscript, LimbTranscript, ipa_verify_fast
from tiny_ram_halo2_amd import api, ipa, poly

pytestmark = pytest.mark.gpu
CURVES = ["pallas", "vesta"]
_POINTS = {c: {} for c in CURVES}  # curve -> {discrete log: (8,) affine POD}: every multiple is computed once
_PARAMS = {}                       # (curve, generator set, k, tables) -> (poly.Params, g_l, w_l, u_l): one per module
COUNTERS = ("msm_quad_combines", "msm_lean_sorts", "msm_lean_retries", "ipa_generator_collapses", "msm_small_launches")


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield
    _PARAMS.clear()


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def _mont(fs, vals):
    return np.array([fs.limbs(v) for v in vals], dtype=np.uint64).reshape(-1, 4)


def _points(curve, logs):
    cv, known = o.CURVES[curve], _POINTS[curve]
    new = sorted(set(logs) - set(known))
    if new:
        g = np.array(cv.affine_limbs(cv.generator), dtype=np.uint64)
        xy = cpu_ref.scale_points(curve, g, _mont(cv.scalar, new))
        for v, row in zip(new, xy):
            assert row.any() == (v != 0)
            known[v] = row
    return np.stack([known[v] for v in logs])


def _point(curve, log):
    """log G as the (12,) normalised Jacobian the library writes: the oracle's affine point and the Montgomery one, or all zero"""
    cv = o.CURVES[curve]
    want = np.zeros(12, dtype=np.uint64)
    if log:
        g = np.array(cv.affine_limbs(cv.generator), dtype=np.uint64)
        want[:8] = cpu_ref.to_affine(curve, cpu_ref.scalar_mul(curve, g, np.array(o.int_to_limbs(log), np.uint64)))
        want[8:] = np.array(cv.base.limbs(1), np.uint64)
    return want


class Recording(DeviceTranscript):
    """keeps what the prover wrote, whole (points as the 12 limbs it handed over), and the challenges it drew"""

    def __init__(self, modulus):
        super().__init__(modulus)
        self.items, self.challenges = [], []

    def write_point(self, jac):
        self.items.append(np.ascontiguousarray(jac, dtype=np.uint64).copy())
        super().write_point(jac)

    def write_scalar(self, limbs):
        self.items.append(np.ascontiguousarray(limbs, dtype=np.uint64).copy())
        super().write_scalar(limbs)

    def squeeze_challenge_scalar(self):
        c = super().squeeze_challenge_scalar()
        self.challenges.append(c)
        return c


def _params(curve, key, k, tables, logs, omega, upsilon):
    """one poly.Params per curve and generator set for the whole module"""
    full = (curve, key, k, tables)
    if full not in _PARAMS:
        q = o.CURVES[curve].scalar.m
        g_l = _points(curve, [v % q for v in logs])
        w_l, u_l = _points(curve, [omega % q]), _points(curve, [upsilon % q])
        params = poly.Params(curve, k, g_l, g_l, w_l, u=u_l, precompute=tables)
        if tables:
            bits = int(api.lib().trh_bases_precomputed_window_bits(params.ipa_bases().handle))
            assert len(params.ipa_bases()) == (1 << k) + 2 and bits == {5: 6, 13: 11, 14: 12}[k], bits
        else:
            assert len(params.ipa_bases()) == (1 << k) + 1
        _PARAMS[full] = (params, g_l, w_l, u_l)
    return _PARAMS[full]


def _model_events(curve, k, tables, logs_full, row):
    """what tests/msm_events_model.py meets for one MSM over the original generators, as _events() of test_gpu_msm_collisions.py lists it"""
    q = o.CURVES[curve].scalar.m
    if tables and k == I.K:
        sh = I.SHAPE
        zero = [0] * M.num_windows(sh["c"])
        lists = M.window_lists(q, logs_full, [M.recode_pipeline(s, sh["c"]) if s else zero for s in row], flat_c=sh["c"])
        ev, _ = M.run_lists(q, lists, sh["c"], sh["seg_len"], sh["m"], "q4" if api.get_option("reduce_q4") else 4, bool(api.get_option("reduce_q4")), True)
    elif tables:
        ev, _ = M.run_small(q, logs_full, row)
    else:
        ev, _ = M.run_pipeline(q, logs_full, row, 8, 16, 1, 4)
    return sorted(f"{stage}:{event} x{n}" for (stage, event), n in ev.n.items() if event not in ("add-identity", "first") and not event.startswith(("publish", "head")))


def _open(curve, key, k, tables, inp, case, route):
    """one opening on the device against the exponent model, the verifier equation and the literal prover; `route`: what the counters must
    have moved by, or None"""
    cv = o.CURVES[curve]
    fs, q, n = cv.scalar, cv.scalar.m, 1 << k
    params, g_l, w_l, u_l = _params(curve, key, k, tables, inp["a"], inp["omega"], inp["upsilon"])
    p_l, s_l = _mont(fs, inp["p_poly"]), _mont(fs, inp["s_poly"])
    before = {c: api.stat(c) for c in COUNTERS}
    it = iter(inp["draws"])
    t_dev = Recording(q)
    c_dev, f_dev = ipa.create_proof_native(params, lambda: next(it), t_dev, to_dev(p_l), inp["p_blind"], inp["x3"], s_l, inp["s_blind"])
    moved = {c: api.stat(c) - before[c] for c in COUNTERS}

    # the model: integers, and one scalar multiplication of the oracle per point
    it = iter(inp["draws"])
    t_mod = X.LogTranscript(fs, lambda log: _point(curve, log)[:8])
    op = X.create_proof(q, k, inp["a"], inp["omega"], inp["upsilon"], lambda: next(it), t_mod, inp["p_poly"], inp["p_blind"], inp["x3"], inp["s_poly"], inp["s_blind"])
    names = op.items()
    assert len(t_dev.items) == len(names) == 1 + 2 * k + 2, f"{curve} {case}: {len(t_dev.items)} transcript items"
    for got, (name, value) in zip(t_dev.items, names):
        want = np.array(fs.limbs(value), np.uint64) if name in ("c", "f") else _point(curve, value)
        if got.shape != want.shape or (got != want).any():
            rows = {"S": op.row_s, "L_0": op.row_l0, "R_0": op.row_r0}
            events = _model_events(curve, k, tables, I.logs_of(inp), rows[name]) if name in rows else "(a later round: its scalar rows are folds of these)"
            raise AssertionError(f"{curve} {case} (k = {k}, tables {'on' if tables else 'off'}): the transcript differs first at {name}: got {[hex(int(v)) for v in got]}, "
                                 f"the model has {'the identity' if name not in ('c', 'f') and not value else hex(value)}; counters moved by {moved}; the model meets {events}")
    assert (c_dev, f_dev) == (op.c, op.f) and t_dev.challenges == t_mod.challenges

    # the verifier equation on what the GPU produced; P = commit(p, p_blind) and v = p(x3) come from the integers
    commitment = _point(curve, (X.dot(inp["p_poly"], inp["a"], q) + inp["p_blind"] * inp["omega"]) % q)[:8]
    v = X.eval_poly(inp["p_poly"], inp["x3"], q)
    xi, z, ch = t_dev.challenges[0], t_dev.challenges[1], t_dev.challenges[2:]
    pts = [p[:8] for p in t_dev.items[:1 + 2 * k]]
    rounds = [(pts[1 + 2 * j], pts[2 + 2 * j]) for j in range(k)]
    assert ipa_verify_fast(curve, k, g_l, w_l[0], u_l[0], commitment, inp["x3"], v, pts[0], xi, z, rounds, ch, c_dev, f_dev), f"{curve} {case}: the verifier rejects"

    # the literal prover of the C++ oracle writes the same transcript
    lim = lambda val: np.array(fs.limbs(val), np.uint64)  # noqa: E731
    it = iter(inp["draws"])
    t_ref = LimbTranscript(fs)
    c_ref, f_ref = cpu_ref.ipa_create_proof(curve, k, g_l, w_l[0], u_l[0], lambda: lim(next(it)), t_ref, p_l, lim(inp["p_blind"]), lim(inp["x3"]), s_l, lim(inp["s_blind"]))
    assert (c_dev, f_dev) == (fs.from_limbs(c_ref), fs.from_limbs(f_ref))
    for i, (x, y) in enumerate(zip(t_dev.log, t_ref.log)):
        assert x == y, f"{curve} {case}: transcript item {i} ({names[i][0]}) differs from cpu_ref.ipa_create_proof"

    if route is not None:
        assert moved == route, f"{curve} {case}: the counters moved by {moved}, the route it is meant to take moves them by {route}"
    return moved


def _route(k, tables, full_size=False):
    """what one opening moves the counters by, from the options of this process (hostplan.h: up to k = 13 a tabled opening is k + 1
    one-launch MSMs; k = 14 runs S and rounds 0, 1 over the table, collapses to 2^12 and runs 12 one-launch rounds; without tables every
    round is a per-window pipeline MSM over 32 bucket sets, and the commitment to s' does not vouch for its scalars).
    full_size: s(X) is random.  The 12-bit table has 21 full windows and a top window of 3 bits, whose digits 1 .. 3 all lie in bin 0 of the
    16: that bin gets 21 / 16 + 3 / 4 of the 16386 scalars' digits, 33800 entries against the 24576 the LDS sort holds -- the lean sort of
    the commitment to s' gives up for EVERY random s, the MSM is run again, and rounds 0 and 1 (the same shape) keep the fallback launches"""
    q4, lean, fold = api.get_option("reduce_q4"), api.get_option("bin_sort"), api.get_option("ipa_fold")
    if fold != 1:
        return None
    if tables and k < I.K:
        return dict(msm_quad_combines=0, msm_lean_sorts=0, msm_lean_retries=0, ipa_generator_collapses=0, msm_small_launches=k + 1)
    if tables:
        again = 1 if full_size and lean else 0
        return dict(msm_quad_combines=3 + again if q4 else 0, msm_lean_sorts=(1 if again else 3) if lean else 0, msm_lean_retries=again, ipa_generator_collapses=1,
                    msm_small_launches=12)
    return dict(msm_quad_combines=0, msm_lean_sorts=k if lean else 0, msm_lean_retries=0, ipa_generator_collapses=0, msm_small_launches=0)


# ---------------------------------------------------------------------------------------
# 1. the designed cases
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("name", [c.name for c in I.CASES])
def test_opening_msm_designed_case(curve, name):
    """k = 14, tables on: the quad combine ran for S and for rounds 0 and 1, no lean retry, one collapse, 12 small launches"""
    case = I.BY_NAME[name]
    inp, designs, rows = case.build(curve, point_of=lambda log: _point(curve, log)[:8])
    _open(curve, name, I.K, True, inp, f"{name} ({', '.join(d.name for d in designs.values())})", _route(I.K, True))


# ---------------------------------------------------------------------------------------
# 2. duplicate generators, random full-size polynomials
# ---------------------------------------------------------------------------------------
GENERATOR_SETS = ["all-equal", "alternating", "pm-one-two-zero", "w-and-u-of-g0"]
SHAPES = [(5, True), (13, True), (14, True), (14, False)]


def _generators(which, n, q, rnd):
    """(logs of g, omega, upsilon)"""
    P = 0x1D0F5A7E9B3C2468ACE13579BDF02468ACE13579BDF0246 % q
    if which == "all-equal":
        return [P] * n, rnd.randrange(1, q), rnd.randrange(1, q)
    if which == "alternating":
        return [P, q - P] * (n // 2), rnd.randrange(1, q), rnd.randrange(1, q)
    if which == "pm-one-two-zero":
        return [1, q - 1, 2, 0] + [rnd.choice([1, q - 1, 2, 0]) for _ in range(n - 4)], rnd.randrange(1, q), rnd.randrange(1, q)
    logs = [rnd.randrange(1, q) for _ in range(n)]  # distinct generators, w = g_0 and u = -g_0
    return logs, logs[0], q - logs[0]


def _random_inputs(curve, which, k, seed):
    q, n = o.CURVES[curve].scalar.m, 1 << k
    a, omega, upsilon = _generators(which, n, q, random.Random(f"generators/{which}/{k}"))
    rnd = random.Random(f"{seed}/{curve}/{which}/{k}")
    full = lambda: rnd.randrange(1, q)  # noqa: E731
    return dict(a=a, omega=omega, upsilon=upsilon, p_poly=[full() for _ in range(n)], s_poly=[full() for _ in range(n)], p_blind=full(), s_blind=full(),
                x3=full(), draws=[full() for _ in range(2 * k)])


@pytest.mark.parametrize("k,tables", SHAPES)
@pytest.mark.parametrize("which", GENERATOR_SETS)
def test_opening_msm_over_duplicate_generators(which, k, tables):
    """every generator set at every shape once, the curves alternating so that each shape and each set runs on both"""
    curve = CURVES[(GENERATOR_SETS.index(which) + SHAPES.index((k, tables))) % 2]
    inp = _random_inputs(curve, which, k, "random")
    _open(curve, which, k, tables, inp, f"{which} generators, random p and s", _route(k, tables, full_size=True))


# ---------------------------------------------------------------------------------------
# 3. overflow and retry over duplicates
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,which", [("pallas", "all-equal"), ("vesta", "alternating")])
def test_opening_msm_retry_over_duplicate_generators(curve, which):
    """the polynomial of test_ipa_skewed_polynomial_takes_the_chunked_sort_again (tests/test_gpu_realsize.py) -- every coefficient the same
    value with the digit 1 in every window of the table, s(X) = 0 -- puts every entry of round 0 into bucket 1, far above a bin's LDS
    capacity: the lean sort gives up, msm_finish runs the MSM again with force_fallback and dense_hint (the chunked passes, then the quad
    combine hands bucket 1 to the heavy kernel), over generators that are all equal or +-P"""
    if api.get_option("bin_sort") == 0:
        pytest.skip("option bin_sort = 0: every MSM takes the chunked passes, there is no lean sort to fall back from")
    k = I.K
    q, n = o.CURVES[curve].scalar.m, 1 << k
    inp = _random_inputs(curve, which, k, "retry")
    c0 = sum(1 << (12 * j) for j in range(255 // 12 + 1)) % q   # digit 1 in every window of the 12-bit table, no carries
    inp["p_poly"], inp["s_poly"] = [c0] * n, [0] * n
    moved = _open(curve, which, k, True, inp, f"{which} generators, skewed p", None)
    assert moved["msm_lean_retries"] >= 1, "the skewed round did not overflow a bin: the test no longer reaches the retry"
    if api.get_option("ipa_fold") == 1:
        # S and round 0 are enqueued lean; round 0 overflows and is run again; round 1 has the same shape and keeps the fallback launches
        assert moved == dict(msm_quad_combines=4 if api.get_option("reduce_q4") else 0, msm_lean_sorts=2, msm_lean_retries=1, ipa_generator_collapses=1, msm_small_launches=12), moved


# ---------------------------------------------------------------------------------------
# 4. degenerate rows
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["zero", "0", "half-1", "half", "n-1"])
def test_opening_msm_degenerate_rows(where):
    """s = 0 and p = 0, or p with ONE non-zero coefficient: the scalar rows of every MSM are all zero but for coefficient 0, w and u
    (p'[0] = -p_i x3^i; for i = 0 that is zero too), over the +-1, 2, identity generators"""
    k = I.K
    n = 1 << k
    index = {"zero": None, "0": 0, "half-1": n // 2 - 1, "half": n // 2, "n-1": n - 1}[where]
    curve = CURVES[(index or 0) % 2]
    q = o.CURVES[curve].scalar.m
    inp = _random_inputs(curve, "pm-one-two-zero", k, "degenerate/" + where)
    coefficient = inp["p_poly"][7]
    inp["p_poly"], inp["s_poly"] = [0] * n, [0] * n
    if index is not None:
        inp["p_poly"][index] = coefficient
    _open(curve, "pm-one-two-zero", k, True, inp, f"p = {'0' if index is None else f'one coefficient at {index}'}, s = 0", _route(k, True))
