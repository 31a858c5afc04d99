"""CPU tests of hash_to_curve (csrc/blake2b.h, csrc/hashtocurve.h, trh_hash_to_curve), no GPU.
1. tests/hash_to_curve_model.py itself, with integers: both iso-curves have the order of Pallas / Vesta, -13 is a non-square, the isogeny the
   model DERIVES from A and 1265 lands on y^2 = x^3 + 5 and is additive, its rational form leads with 9^-1 and 27^-1, simplified SWU lands on the
   iso-curve with sgn0(y) = sgn0(u); the constants of the committed header are the derived ones.
2. The headers' plain C++ branch in a stand-alone program (tests/native/hashtocurve_vec_test.cpp) under address + undefined sanitizers: BLAKE2b
   against hashlib at the lengths around a block boundary, hash_to_field (byte-wise and through the per-index plan the device kernel uses) and
   the whole map against the model.
3. trh_hash_to_curve through ctypes on a machine without a device: both curves, messages and prefixes whose hash inputs straddle block
   boundaries, the refusals, w and u of Halo2-Parameters and the recorded values of tests/golden/hash_to_curve_kat.json.
tests/test_gpu_hashtocurve.py sends the same function through the kernels."""
import ctypes
import hashlib
import importlib.util
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import common
import hash_to_curve_model as h2c
from tiny_ram_halo2_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["pallas", "vesta"]
BASE_FIELD = {"pallas": "fp", "vesta": "fq"}
EINVAL = -1
HALO2 = h2c.HALO2_PREFIX
# b1's input is 64 + 1 + len(DST') bytes, DST' = prefix + 1 + len(curve) + 21 + 1: exactly one block at 34 (pallas) / 35 (vesta), two beyond;
# b0's tail with a 5-byte message is 5 + 3 + len(DST'): exactly one block past the zero block at 91 / 92
PREFIX_LENGTHS = [0, 16, 34, 35, 91, 92, 128]
MESSAGES = [b"", b"\x01", b"\x00\x07\x00\x01\x00", bytes((7 * i + 3) & 0xff for i in range(200))]


def _prefix(n: int) -> bytes:
    return (HALO2 * 9)[:n]  # printable, no NUL: it crosses the C ABI as a string


def _spec(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- 1. the model ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_model_group_order_and_nonsquare_z(curve):
    c = h2c.CURVES[curve]
    rng = random.Random(0x150 + len(curve))
    assert pow(c.z, (c.m - 1) // 2, c.m) == c.m - 1, "Z = -13 must be a non-square"
    for _ in range(3):
        p = c.swu(rng.randrange(c.m))
        assert c.on_iso(p) and c.mul(c.order, p) is None and c.mul(c.order - 1, p) == (p[0], c.m - p[1])
    # Hasse: the order is within 2 sqrt(m) of m + 1, and a prime that kills random points IS the order
    assert abs(c.order - (c.m + 1)) ** 2 <= 4 * c.m


@pytest.mark.parametrize("curve", CURVES)
def test_model_isogeny_is_derived_lands_on_the_curve_and_is_additive(curve):
    c = h2c.CURVES[curve]
    rng = random.Random(0x3150 + len(curve))
    assert c.x0 * c.x0 % c.m == -3 * c.a * pow(10, -1, c.m) % c.m and c.div3(c.x0) == 0 and c.div3(c.m - c.x0) != 0
    assert c.iso["x_num"][0] == pow(9, -1, c.m) and c.iso["y_num"][0] == pow(27, -1, c.m)
    assert c.iso["x_num"][1] == -2 * c.x0 * pow(9, -1, c.m) % c.m
    pts = [c.swu(rng.randrange(c.m)) for _ in range(20)]
    for p, q in zip(pts, pts[1:] + pts[:1]):
        ip, iq = c.iso_map(p), c.iso_map(q)
        assert ip is not None and c.on_curve(ip) and ip == c.iso_map_polynomial(p)
        assert c.iso_map(c.add(p, q)) == c.add(ip, iq, 0)
        assert c.iso_map(c.add(p, p)) == c.add(ip, ip, 0)
    assert c.iso_map(None) is None and c.iso_map(c.add(pts[0], (pts[0][0], c.m - pts[0][1]))) is None


@pytest.mark.parametrize("curve", CURVES)
def test_model_swu_is_on_the_iso_curve_with_the_sign_of_u(curve):
    c = h2c.CURVES[curve]
    rng = random.Random(0x5300 + len(curve))
    us = [0, 1, c.m - 1] + [rng.randrange(c.m) for _ in range(40)]
    r = h2c.sqrt_mod(pow(13, -1, c.m), c.m)  # u^2 = -1 / Z: the second exceptional input, where it exists
    if r is not None:
        us += [r, c.m - r]
    seen = set()
    for u in us:
        x, y = c.swu(u)
        assert c.on_iso((x, y)) and c.sgn0(y) == c.sgn0(u), hex(u)
        seen.add(c.gx1_is_square(u))
    assert seen == {True, False}
    x1 = c.b * pow(c.z * c.a, -1, c.m) % c.m  # tv1 = 0: x1 = B / (Z A), and x2 = Z u^2 x1 = 0 at u = 0
    assert c.swu(0)[0] == (x1 if c.gx1_is_square(0) else 0)


def test_committed_header_holds_the_derived_constants():
    gen = _spec("make_hashtocurve_consts", "tests", "golden", "make_hashtocurve_consts.py")
    path = os.path.join(ROOT, "tiny-ram-halo2_amd", "csrc", "hashtocurve_consts.h")
    text = open(path).read()
    assert text == gen.header_text(), "csrc/hashtocurve_consts.h is not what tests/golden/make_hashtocurve_consts.py writes"
    # and read back word by word, so that the comparison does not rest on the generator's own formatting
    want = gen.header_constants()
    for field, block in re.findall(r"struct H2cConsts<(\w+)> \{(.*?)\n\};", text, re.S):
        got = {name: [int(w, 16) for w in re.findall(r"0x([0-9a-f]{8})u", words)] for name, words in re.findall(r"u32 (\w+)\[8\] = \{([^}]*)\}", block)}
        assert got == want[field] and len(got) == 7, field
    for name, c in h2c.CURVES.items():
        f = gen.FIELD_OF[name]
        val = lambda k: sum(w << (32 * i) for i, w in enumerate(want[f][k])) * pow(1 << 256, -1, c.m) % c.m
        assert (val("A"), val("B"), val("Z")) == (c.a, 1265, c.m - 13)
        assert val("THETA") ** 2 % c.m == c.z ** 3 * pow(c.g, -1, c.m) % c.m and pow(c.g, 1 << 31, c.m) == c.m - 1


def test_recorded_known_answers_are_the_models():
    gen = _spec("make_hashtocurve_consts", "tests", "golden", "make_hashtocurve_consts.py")
    assert common.load_json("hash_to_curve_kat.json") == json.loads(json.dumps(gen.kat()))


# ---- 2. the headers' host branch ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vec_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hashtocurve") / "hashtocurve_vec_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "hashtocurve_vec_test.cpp"), "-o", exe])
    return exe


def _run(exe, mode, curve, strings, records, tmp_path, tag):
    src, dst = str(tmp_path / f"{tag}.in"), str(tmp_path / f"{tag}.out")
    with open(src, "wb") as fh:
        for s in strings:
            fh.write(len(s).to_bytes(4, "little") + s)
    r = subprocess.run([exe, mode, curve, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"{records} records ok" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr
    return open(dst, "rb").read()


def _fe(curve, raw):
    """32 stored bytes -> the canonical integer"""
    m = h2c.CURVES[curve].m
    return int.from_bytes(raw, "little") * pow(1 << 256, -1, m) % m


def _point(curve, raw):
    return None if not any(raw) else (_fe(curve, raw[:32]), _fe(curve, raw[32:64]))


def _stored(curve, v):
    m = h2c.CURVES[curve].m
    return (v % m * (1 << 256) % m).to_bytes(32, "little")


def test_blake2b_host_branch_against_hashlib(vec_exe, tmp_path):
    assert hashlib.blake2b(b"abc").hexdigest().startswith("ba80a53f981c4d0d") and hashlib.blake2b(b"abc", person=bytes(16)).digest() == hashlib.blake2b(b"abc").digest()
    inputs = [b"", b"\x00", b"abc"] + [bytes((i * 131 + n) & 0xff for i in range(n)) for n in (127, 128, 129, 255, 256, 257, 384, 1000)]
    out = _run(vec_exe, "blake2b", "pallas", inputs, len(inputs), tmp_path, "blake2b")
    assert len(out) == 64 * len(inputs)
    for i, s in enumerate(inputs):
        assert out[64 * i:64 * i + 64] == hashlib.blake2b(s).digest(), f"input of {len(s)} bytes"
    assert out[128:136].hex() == "ba80a53f981c4d0d"


@pytest.mark.parametrize("curve", CURVES)
def test_hash_to_field_host_branch(vec_exe, tmp_path, curve):
    c = h2c.CURVES[curve]
    cases = [(_prefix(n), msg) for n in PREFIX_LENGTHS for msg in MESSAGES]
    out = _run(vec_exe, "field", curve, [s for case in cases for s in case], len(cases), tmp_path, "field")
    for i, (prefix, msg) in enumerate(cases):
        got = [_fe(curve, out[64 * i:64 * i + 32]), _fe(curve, out[64 * i + 32:64 * i + 64])]
        assert got == c.hash_to_field(prefix, msg), f"prefix of {len(prefix)} bytes, message of {len(msg)}"


@pytest.mark.parametrize("curve", CURVES)
def test_hash_to_field_indexed_plan_host_branch(vec_exe, tmp_path, curve):
    """the per-index plan of the device kernel (precomputed zero block, shared tail words), on the host"""
    c = h2c.CURVES[curve]
    indices = [0, 1, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, (1 << 32) - 1]
    cases = [(_prefix(n), tag, i) for n in PREFIX_LENGTHS for tag in (0, 1, 0xFE) for i in indices]
    strings = [s for prefix, tag, i in cases for s in (prefix, bytes([tag]), i.to_bytes(4, "little"))]
    out = _run(vec_exe, "indexed", curve, strings, len(cases), tmp_path, "indexed")
    for k, (prefix, tag, i) in enumerate(cases):
        got = [_fe(curve, out[64 * k:64 * k + 32]), _fe(curve, out[64 * k + 32:64 * k + 64])]
        assert got == c.hash_to_field(prefix, bytes([tag]) + i.to_bytes(4, "little")), f"prefix of {len(prefix)} bytes, tag {tag}, index {i}"


@pytest.mark.parametrize("curve", CURVES)
def test_map_host_branch(vec_exe, tmp_path, curve):
    c = h2c.CURVES[curve]
    rng = random.Random(0x3A9 + len(curve))
    singles = [0, 1, c.m - 1] + [rng.randrange(c.m) for _ in range(24)]
    r = h2c.sqrt_mod(pow(13, -1, c.m), c.m)
    if r is not None:
        singles += [r, c.m - r]
    u = rng.randrange(1, c.m)
    pairs = [(u, c.m - u), (u, u), (0, u), (u, 0), (0, 0)] + [(rng.randrange(c.m), rng.randrange(c.m)) for _ in range(12)]
    records = [(v,) for v in singles] + pairs
    out = _run(vec_exe, "map", curve, [b"".join(_stored(curve, v) for v in rec) for rec in records], len(records), tmp_path, "map")
    for k, rec in enumerate(records):
        assert _point(curve, out[64 * k:64 * k + 64]) == c.map_sum(rec), [hex(v) for v in rec]
    assert not any(out[64 * len(singles):64 * len(singles) + 64]), "(u, -u) is the all-zero POD"
    assert {c.gx1_is_square(v) for v in singles} == {True, False}


# ---- 3. trh_hash_to_curve through ctypes ---------------------------------------------------------------------------------------------------
def _limbs(curve, p):
    return h2c.point_limbs(h2c.CURVES[curve].m, p)


@pytest.mark.parametrize("curve", CURVES)
def test_hash_to_curve_entry_against_the_model(curve):
    c = h2c.CURVES[curve]
    for n in PREFIX_LENGTHS:
        for msg in MESSAGES:
            got = api.hash_to_curve(curve, _prefix(n), msg)
            assert got.tolist() == _limbs(curve, c.hash_to_curve(_prefix(n), msg)), f"prefix of {n} bytes, message of {len(msg)}"


@pytest.mark.parametrize("curve", CURVES)
def test_params_w_and_u_and_recorded_answers(curve):
    kat = common.load_json("hash_to_curve_kat.json")
    unhex = lambda p: (int(p[0], 16), int(p[1], 16))
    assert kat["prefix"] == HALO2.decode()
    assert api.hash_to_curve(curve, HALO2, b"\x01").tolist() == _limbs(curve, h2c.params_w(curve)) == _limbs(curve, unhex(kat[curve]["w"]))
    assert api.hash_to_curve(curve, HALO2, b"\x02").tolist() == _limbs(curve, h2c.params_u(curve)) == _limbs(curve, unhex(kat[curve]["u"]))
    for i, p in kat[curve]["g"].items():
        msg = b"\x00" + int(i).to_bytes(4, "little")
        assert api.hash_to_curve(curve, HALO2, msg).tolist() == _limbs(curve, unhex(p)) == _limbs(curve, h2c.params_g(curve, int(i)))


def test_hash_to_curve_entry_refusals():
    lib = api.lib()
    out = np.zeros(8, dtype=np.uint64)
    p = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    msg = ctypes.c_char_p(b"\x01")
    assert lib.trh_hash_to_curve(0, _prefix(128), msg, 1, p) == 0
    assert lib.trh_hash_to_curve(0, _prefix(129), msg, 1, p) == EINVAL and b"prefix" in lib.trh_last_error()
    for bad in (2, -1, 7):
        assert lib.trh_hash_to_curve(bad, HALO2, msg, 1, p) == EINVAL and b"unknown curve id" in lib.trh_last_error()
    assert lib.trh_hash_to_curve(0, None, msg, 1, p) == EINVAL and b"null" in lib.trh_last_error()
    assert lib.trh_hash_to_curve(0, HALO2, None, 1, p) == EINVAL and b"null" in lib.trh_last_error()
    assert lib.trh_hash_to_curve(0, HALO2, msg, 1, None) == EINVAL and b"null" in lib.trh_last_error()
    assert lib.trh_hash_to_curve(1, HALO2, None, 0, p) == 0, "an empty message needs no pointer"
    assert out.tolist() == _limbs("vesta", h2c.VESTA.hash_to_curve(HALO2, b""))
