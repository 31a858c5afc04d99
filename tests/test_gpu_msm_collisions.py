"""GPU tests (-m gpu): every MSM stage that adds points, on inputs where the operands of its additions coincide BY CONSTRUCTION.

The formulas of the group law are tested elsewhere (test_gpu_lazy29*.py, test_gpu_q4.py); this file is about the control flow AROUND their
exceptional cases -- an identity operand, P + P, P + (-P) -- in each stage: the `fresh` flag, the re-read for the doubling and the three
publish targets of msm_accumulate_seg_kernel; msm_combine_kernel<1>, <4> and msm_combine_heavy_kernel; both branches of msm_reduce_kernel,
msm_reduce_q4_kernel and the window-sum kernels; msm_small_kernel in both forms; the host Horner of msm_finish.

Every base is a known small multiple a_i of the generator (tests/msm_collision_cases.py: 0 is the identity, negatives are q - a), so the
expected point of ANY of these MSMs is (sum s_i a_i mod q) G: Python integers and one scalar multiplication of the C++ oracle, independent of
how the device orders or splits the work.  Every result is compared limb for limb, Z included (the Montgomery one, or all zero for the
identity); up to 4096 pairs also with cpu_ref.best_multiexp.  trh_stat "msm_small_launches" proves the route; the pipeline is forced at
small n with api.set_window_bits.  tests/test_msm_events_model.py proves on the CPU which events each case meets at which stage;
test_gpu_q4.py runs this file again with TRH_REDUCE_Q4=0 (thread-per-slice reduction, the small kernel's shuffle sums).
msm_combine_q4_kernel runs only for the IPA's dense_hint: that route (the lean sort, the quad combine and its heavy hand-over, the retry) has
its own designed cases, run through trh_ipa_create_proof, in tests/test_gpu_ipa_collisions.py (tests/ipa_collision_cases.py)."""
import numpy as np
import pytest

import cpu_ref
import msm_collision_cases as C
import pasta as o
from tiny_ram_halo2_amd import api

pytestmark = pytest.mark.gpu
CURVES = ["pallas", "vesta"]
_POINTS = {c: {} for c in CURVES}  # curve -> {discrete log: (8,) affine POD}: every multiple is computed once


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


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


def _expected(curve, total):
    cv = o.CURVES[curve]
    want = np.zeros(12, dtype=np.uint64)
    if total:
        g = np.array(cv.affine_limbs(cv.generator), dtype=np.uint64)
        want[:8] = cpu_ref.to_affine(curve, cpu_ref.scalar_mul(curve, g, np.array(o.int_to_limbs(total), np.uint64)))
        want[8:] = np.array(cv.base.limbs(1), np.uint64)
    return want


def _events(cs, q):
    ev, _ = cs.run_model(q)
    return sorted(f"{stage}:{event} x{k}" for (stage, event), k in ev.n.items() if event != "add-identity" and not event.startswith("publish") and event != "first")


def _check(curve, cs, got, xy, sc):
    q = o.CURVES[curve].scalar.m
    want = _expected(curve, cs.total(q))
    assert (np.asarray(got) == want).all(), f"{curve} {cs.name} ({cs.shape}, n = {cs.n}): wrong point; the model meets {_events(cs, q)}"
    if cs.n <= 4096:
        ref = cpu_ref.best_multiexp(curve, sc, xy, threads=4)
        assert (cpu_ref.to_affine(curve, ref) == want[:8]).all(), f"{cs.name}: the oracle's best_multiexp disagrees with the closed form"


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("name", [cs.name for cs in C.ALL])
def test_msm_collision_case(curve, name):
    cs = C.BY_NAME[name]
    cv, sh = o.CURVES[curve], C.SHAPES[C.BY_NAME[name].shape]
    xy, sc = _points(curve, cs.logs(cv.scalar.m)), _mont(cv.scalar, cs.s)
    small = api.stat("msm_small_launches")
    if sh["mode"] == "override":
        try:
            api.set_window_bits(sh["c"])
            got = api.best_multiexp(curve, sc, xy)
        finally:
            api.set_window_bits(0)
    elif sh["mode"] == "table":
        bases = api.Bases.from_host(curve, xy)
        try:
            assert bases.precompute(sh["c"]) == sh["c"]
            got = bases.msm(sc)
        finally:
            bases.destroy()
    else:
        got = api.best_multiexp(curve, sc, xy)
    assert api.stat("msm_small_launches") - small == (1 if sh["mode"] == "small" else 0)
    _check(curve, cs, got, xy, sc)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("name", sorted(C.BATCHES))
def test_msm_collision_batches(curve, name):
    """msm_batch_dev: item k is case k over the concatenation of the cases' bases, zero scalars elsewhere -- a different case per item, so a
    wrong blockIdx.z offset shows.  Two items (small kernel; pipeline under the override) and eight (the plan's own c = 8 with segments sized
    to the entry counts)"""
    shape, names = C.BATCHES[name]
    cases = [C.BY_NAME[k] for k in names]
    cv = o.CURVES[curve]
    q, n, batch = cv.scalar.m, sum(cs.n for cs in cases), len(cases)
    xy = np.concatenate([_points(curve, cs.logs(q)) for cs in cases])
    sc = np.zeros((batch, n, 4), dtype=np.uint64)
    at = 0
    for k, cs in enumerate(cases):
        sc[k, at:at + cs.n] = _mont(cv.scalar, cs.s)
        at += cs.n
    small = api.stat("msm_small_launches")
    bases = d = None
    try:
        bases = api.Bases.from_host(curve, xy)
        d = api.DeviceBuffer.from_host(sc)
        api.set_window_bits(8 if shape == "c8" else 0)
        got = bases.msm_batch_dev(d, n, batch)
    finally:
        api.set_window_bits(0)
        if d is not None:
            d.free()
        if bases is not None:
            bases.destroy()
    assert api.stat("msm_small_launches") - small == (1 if shape == "small" else 0)
    at = 0
    for k, cs in enumerate(cases):
        want = _expected(curve, cs.total(q))
        assert (got[k] == want).all(), f"{curve} {name}: item {k} ({cs.name}) is wrong; the model meets {_events(cs, q)}"
        if k < 2:
            ref = cpu_ref.best_multiexp(curve, sc[k, at:at + cs.n], xy[at:at + cs.n], threads=4)
            assert (cpu_ref.to_affine(curve, ref) == want[:8]).all()
        at += cs.n
