"""GPU test (-m gpu): one segment of the MSM's accumulation outside the library.  One wave, 64 lanes, each running 128 consecutive
mixed additions (csrc/curve.h xyzzz_madd_main; 128 is msm_accumulate_seg_kernel's segment length) onto one accumulator that stays in
registers across the loop -- what the records of tests/test_gpu_lazy29.py, one call each, cannot show: limbs of the accumulator
carried from one addition's column blocks into the next.  The points are multiples (s0 + i d) G as trh_bases_generate makes them;
lane 5 meets p = acc half way (the doubling) and lane 9 meets p = -acc at its last addition (the identity).
tests/native/lazy29_segment_test (built by `make` with the library's flags) records the accumulator after EVERY addition on the
device and through the plain C++ host branch of the same headers: equal limb for limb; and the end of every lane is the oracle's
affine sum.  One subprocess per field, under a time limit, never retried."""
import os
import subprocess

import numpy as np
import pytest

import lazy29_gen as gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "lazy29_segment_test")
FIELDS = ["fp", "fq"]
LANES, SEG = 64, 128
S0, D = 100003, 7           # point i of the table is (S0 + i D) G
LANE_DOUBLE, STEP_DOUBLE = 5, 64     # addition 64 of lane 5 adds the lane's own partial sum
LANE_CANCEL, STEP_CANCEL = 9, SEG    # the last addition of lane 9 adds the negated partial sum


def lane_points(field):
    """per lane the SEG + 1 (scalar, affine point) pairs, and the scalar of every lane's sum"""
    cv = gen.o.CURVES[gen.CURVE_OF[field]]
    G, r = cv.generator, cv.scalar.m
    step = cv.mul(D, G)
    table, p = [], cv.mul(S0, G)
    for i in range(LANES * (SEG + 1)):
        table.append((S0 + i * D, p))
        p = cv.add(p, step)
    lanes, totals = [], []
    for l in range(LANES):
        pts = list(table[l * (SEG + 1):(l + 1) * (SEG + 1)])
        if l == LANE_DOUBLE:
            k = sum(s for s, _ in pts[:STEP_DOUBLE])
            pts[STEP_DOUBLE] = (k, cv.mul(k, G))
        if l == LANE_CANCEL:
            k = sum(s for s, _ in pts[:STEP_CANCEL])
            pts[STEP_CANCEL] = (-k, cv.neg(cv.mul(k, G)))
        lanes.append(pts)
        totals.append(sum(s for s, _ in pts) % r)
    return lanes, totals


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    done = {}

    def run(field):
        if field not in done:
            done[field] = None  # a failed run is not started again by the next test of the field
            assert os.path.exists(EXE), "tests/native/lazy29_segment_test is missing: run `make`"
            f = gen.o.FIELDS[field]
            lanes, totals = lane_points(field)
            words = np.array([[gen.norm_limbs(p[0] * gen.K % f.m) + gen.norm_limbs(p[1] * gen.K % f.m) for _, p in pts] for pts in lanes], dtype=np.int64)
            assert words.shape == (LANES, SEG + 1, 18)
            d = tmp_path_factory.mktemp("lazy29_segment_" + field)
            src, dst = str(d / "points.bin"), str(d / "trace.bin")
            words.astype("<i4").tofile(src)
            r = subprocess.run(["timeout", "-k", "10", "60", EXE, field, src, dst], capture_output=True, text=True)
            assert r.returncode == 0 and "additions ok" in r.stdout, f"exit {r.returncode}\n{r.stdout}{r.stderr}"
            t = np.fromfile(dst, dtype="<i4")
            assert t.size == 2 * LANES * SEG * 37
            t = t.reshape(2, LANES, SEG, 37)
            done[field] = (totals, t[0], t[1])
        assert done[field] is not None, "the device run of this field failed (see the first test of the field)"
        return done[field]
    return run


@pytest.mark.parametrize("field", FIELDS)
def test_every_addition_of_a_segment_matches_host_branch(traces, field):
    _, dev, host = traces(field)
    differ = np.argwhere((dev != host).any(axis=2))
    msg = [f"lane {l}, addition {s + 1}: device {dev[l, s].tolist()} != host {host[l, s].tolist()}" for l, s in differ[:4]]
    assert differ.size == 0, f"{len(differ)} of {LANES * SEG} accumulator states differ between device and host\n" + "\n".join(msg)
    # the two exceptional lanes took the exceptional paths, exactly once, and nobody else did
    codes = dev[:, :, 36]
    want = np.zeros((LANES, SEG), dtype=codes.dtype)
    want[LANE_DOUBLE, STEP_DOUBLE - 1] = 1
    want[LANE_CANCEL, STEP_CANCEL - 1] = 2
    assert (codes == want).all(), f"codes differ at (lane, addition - 1) {np.argwhere(codes != want)[:8].tolist()}"


@pytest.mark.parametrize("field", FIELDS)
def test_end_of_every_lane_is_the_oracle_sum(traces, field):
    totals, dev, _ = traces(field)
    f = gen.o.FIELDS[field]
    cv = gen.o.CURVES[gen.CURVE_OF[field]]
    bad = []
    for l in range(LANES):
        want = cv.mul(totals[l], cv.generator) if totals[l] else None
        got = gen.decode_point(f, dev[l, SEG - 1, :36].reshape(4, 9).tolist())
        if got != want:
            bad.append(f"lane {l}: {got} != oracle {want}")
    assert totals[LANE_CANCEL] == 0 and sum(1 for t in totals if t == 0) == 1
    assert not bad, "\n".join(bad[:4])
