"""CPU tests of csrc/fieldsqrt.h and of the host-side point encoding (trh_point_to_bytes / trh_point_from_bytes), no GPU.
fe_sqrt runs in a stand-alone program (tests/native/fieldsqrt_vec_test.cpp) under -fsanitize=undefined over records written here; the
flag, r^2 = a and the even-root convention are checked against oracle/pasta.py (tests/encoding_cases.py).  The two C-ABI entries run
through ctypes on a machine without a device, as trh_point_sum does; tests/test_gpu_encoding.py sends the same records through the kernels.
The id dispatch those entries go through (csrc/dispatch.h) has its own stand-alone program, tests/native/dispatch_test.cpp."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import encoding_cases as ec
import pasta as o
from tiny_ram_halo2_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["fp", "fq"]
CURVES = ["pallas", "vesta"]


@pytest.fixture(scope="module")
def sqrt_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fieldsqrt") / "fieldsqrt_vec_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "fieldsqrt_vec_test.cpp"), "-o", exe])
    return exe


def test_records_cover_every_order_of_the_two_part():
    for field in FIELDS:
        f = o.FIELDS[field]
        recs = dict(ec.sqrt_records(field))
        exp = dict(zip((t for t, _ in ec.sqrt_records(field)), ec.sqrt_expected(field)))
        for j in range(33):
            w = recs[f"omega_{j}"]
            assert pow(w, 1 << j, f.m) == 1 and (j == 0 or pow(w, 1 << (j - 1), f.m) != 1)
            assert exp[f"omega_{j}"][1] == (1 if j <= 31 else 0)  # order 2^32 is a non-square
            if j <= 31:
                assert exp[f"r^2*omega_{j}"][1] == 1
        assert exp["generator"] == (0, 0) and exp["5*r^2"] == (0, 0) and exp["0"] == (0, 1) and exp["4"] == (2, 1)
        assert exp["1"] == (f.m - 1, 1)  # m - 1 is even, 1 is odd: the convention picks -1
        assert sum(1 for t in recs if t.startswith("random-square-")) == 256 and sum(1 for t in recs if t.startswith("random-") and "square" not in t) == 256


@pytest.mark.parametrize("field", FIELDS)
def test_fe_sqrt_host_branch_matches_the_oracle(sqrt_exe, tmp_path, field):
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "roots.bin")
    a = ec.sqrt_input_limbs(field)
    a.tofile(src)
    r = subprocess.run([sqrt_exe, field, src, dst], capture_output=True, text=True, timeout=120, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and f"{len(a)} records ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
    raw = np.fromfile(dst, np.uint8).reshape(-1, 33)
    assert raw.shape[0] == len(a)
    bad = ec.check_sqrt(field, raw[:, :32].copy().view(np.uint64), raw[:, 32])
    assert not bad, "\n".join(bad[:20])


def test_dispatch_tags_pair_the_fields_with_the_curves(tmp_path):
    """csrc/dispatch.h (with_field / with_curve) through tests/native/dispatch_test.cpp, built like fieldsqrt_vec_test"""
    exe = str(tmp_path / "dispatch_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "dispatch_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "dispatch: ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


def _points(curve, count=64):
    cv = o.CURVES[curve]
    return [o.synth_base(cv, 0x1234567 + 97 * len(curve), 0x10001, i) for i in range(count)]


@pytest.mark.parametrize("curve", CURVES)
def test_point_to_bytes_any_z(curve):
    cv = o.CURVES[curve]
    f = cv.base
    rng = random.Random(5)
    for p in _points(curve):
        want = ec.encode(curve, p)
        assert api.point_to_bytes(curve, np.array(f.limbs(p[0]) + f.limbs(p[1]) + f.limbs(1), np.uint64)) == want
        z = rng.randrange(2, f.m)
        assert api.point_to_bytes(curve, np.array(f.limbs(p[0] * z * z) + f.limbs(p[1] * z ** 3) + f.limbs(z), np.uint64)) == want
    assert {e[31] >> 7 for e in (ec.encode(curve, p) for p in _points(curve))} == {0, 1}  # both signs occur among the 64
    assert api.point_to_bytes(curve, np.zeros(12, np.uint64)) == bytes(32)
    assert api.point_to_bytes(curve, np.array(f.limbs(3) + f.limbs(4) + [0] * 4, np.uint64)) == bytes(32)  # Z = 0: the identity


@pytest.mark.parametrize("curve", CURVES)
def test_point_from_bytes_round_trip(curve):
    cv = o.CURVES[curve]
    for p in _points(curve):
        got = api.point_from_bytes(curve, ec.encode(curve, p))
        assert cv.affine_from_limbs(got) == p and [int(v) for v in got] == cv.affine_limbs(p)
        q = cv.neg(p)
        assert cv.affine_from_limbs(api.point_from_bytes(curve, ec.encode(curve, q))) == q
    assert (api.point_from_bytes(curve, bytes(32)) == 0).all()


@pytest.mark.parametrize("curve", CURVES)
def test_point_from_bytes_rejections(curve):
    cv = o.CURVES[curve]
    m = cv.base.m
    # what the cases rest on: 5 is a non-square, x = m - 1 and x = 1 are on the curve, x = 2 is not
    assert cv.base.sqrt(5) is None and cv.lift_x(m - 1) is not None and cv.lift_x(1) is not None and cv.lift_x(2) is None
    lib = api.lib()
    seen = set()
    for tag, enc in ec.special_encodings(curve):
        want = ec.decode(curve, enc)
        seen.add(tag)
        if want == ec.INVALID:
            with pytest.raises(api.TrhError):
                api.point_from_bytes(curve, enc)
            out = np.full(8, 7, np.uint64)
            assert lib.trh_point_from_bytes(api.CURVE_ID[curve], ctypes.c_char_p(enc), api._p(out)) == -1 and (out == 0).all(), tag
        else:
            assert want is None and (api.point_from_bytes(curve, enc) == 0).all(), tag
    assert {"sign-bit-only", "x=m", "x=m,sign", "x=m+1", "x=2^255-1", "x=2"} <= seen
    assert all(ec.decode(curve, e) == ec.INVALID for t, e in ec.special_encodings(curve) if t != "identity")
    # x = m + 1 aliases x = 1, a point: a decoder that reduces instead of rejecting would return it
    assert cv.affine_from_limbs(api.point_from_bytes(curve, ec.enc_int(1))) == ec.decode(curve, ec.enc_int(1))
