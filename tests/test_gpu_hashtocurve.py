"""GPU tests (-m gpu) of csrc/hashtocurve.hip: Params::new's hash_to_curve on the device, bit for bit against tests/hash_to_curve_model.py -- the
model tests/test_hashtocurve_host.py pins with integers and hashlib.
1. trh_hash_to_field_indexed_dev: prefixes whose hash inputs end exactly on a block and one byte past it, index ranges across every byte of
   le32(index) and up to 2^32 - 1, one element, none, and the refusal past 2^32.
2. trh_map_to_curve_dev, one element per point: 0, 1, m - 1, the roots of u^2 = -1 / Z where they exist, random elements of both branches
   (gx1 square / not), the stored forms at the edges of the nine-limb register form.
3. two elements per point: (u, -u) -> the all-zero POD, (u, u) -> the doubling, (0, u), random pairs; 1, 63, 64, 65 and 257 records with the
   exceptional ones scattered among ordinary ones of the same wavefront.
4. the fused entry over the ranges of 1., against the model and against the host entry trh_hash_to_curve.
5. Params.new(curve, k), k = 1, 4, 7: g, w, u against the model, g_lagrange through commit_lagrange(column) = commit(lagrange_to_coeff(column)),
   write -> read byte for byte, and trh::Params::create (tests/native/params_new_test) writing the same file.
Every sentinel row around an output must survive: the launches write their n records and no more.
The refusal of an unknown curve id by the three device entries is checked HERE (test_hash_to_field_empty_and_refused; the host entry's in
tests/test_hashtocurve_host.py): include/trh.h names their first parameter curve_id, so the table of tests/test_gpu_id_refusals.py, which
lists the entries whose first parameter is spelled `curve` or `field`, does not claim them."""
import ctypes
import functools
import io
import json
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import common
import hash_to_curve_model as h2c
import pasta as o
from tiny_ram_halo2_amd import api, poly, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["pallas", "vesta"]
BASE_FIELD = {"pallas": "fp", "vesta": "fq"}
EINVAL = -1
HALO2 = h2c.HALO2_PREFIX
SENTINEL = 0x5E5E5E5E5E5E5E5E
PREFIX_LENGTHS = [16, 34, 35, 91, 92]  # see tests/test_hashtocurve_host.py: b1 / b0 end exactly on a block at 34 / 91 (pallas), 35 / 92 (vesta)
# (first, n): 0 .. 299 crosses 255 / 256; then 65 535 / 65 536, 2^24, the last 70 indices, one element
RANGES = [(0, 300), (65530, 12), ((1 << 24) - 6, 12), ((1 << 32) - 70, 70), (12345, 1)]


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


def _prefix(n: int) -> bytes:
    return (HALO2 * 9)[:n]


def sentinel(rows, width):
    return torch.full((rows, width), SENTINEL, dtype=torch.int64, device="cuda")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda")


def mont_rows(curve, values):
    """canonical integers -> (n, 4) stored limbs"""
    m = h2c.CURVES[curve].m
    return np.array([[(v % m * (1 << 256) % m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in values], dtype=np.uint64).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def model_fields(curve, prefix, tag, first, n):
    """(n, 8) limbs: u0, u1 of tag || le32(first + i) -- computed once, shared, never written to"""
    c = h2c.CURVES[curve]
    us = [u for i in range(n) for u in c.hash_to_field(prefix, bytes([tag]) + (first + i).to_bytes(4, "little"))]
    a = mont_rows(curve, us).reshape(n, 8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def model_points(curve, prefix, tag, first, n):
    c = h2c.CURVES[curve]
    a = np.array([h2c.point_limbs(c.m, c.hash_to_curve(prefix, bytes([tag]) + (first + i).to_bytes(4, "little"))) for i in range(n)], dtype=np.uint64).reshape(n, 8)
    a.setflags(write=False)
    return a


def differing(got, want):
    return np.nonzero((got != want).any(axis=1))[0][:10]


# ---- 1. hash_to_field -----------------------------------------------------------------------------------------------------------------------
def _hash_to_field(curve, prefix, tag, first, n):
    d = sentinel(n + 2, 8)  # one record of margin on either side
    api.hash_to_field_indexed_dev(curve, prefix, tag, first, n, d[1:])
    got = host(d)
    assert (got[0] == SENTINEL).all() and (got[n + 1] == SENTINEL).all(), "the launch wrote outside its n records"
    return got[1:n + 1]


@pytest.mark.parametrize("first,n", RANGES)
@pytest.mark.parametrize("curve", CURVES)
def test_hash_to_field_index_ranges(curve, first, n):
    got = _hash_to_field(curve, HALO2, 0, first, n)
    want = model_fields(curve, HALO2, 0, first, n)
    assert (got == want).all(), differing(got, want)


@pytest.mark.parametrize("length", PREFIX_LENGTHS)
@pytest.mark.parametrize("curve", CURVES)
def test_hash_to_field_prefixes_at_the_block_boundaries(curve, length):
    for tag in (0, 0xA7):
        got = _hash_to_field(curve, _prefix(length), tag, 250, 70)  # one wavefront and a few lanes, across index 255 / 256
        want = model_fields(curve, _prefix(length), tag, 250, 70)
        assert (got == want).all(), (tag, differing(got, want))


@pytest.mark.parametrize("curve", CURVES)
def test_hash_to_field_empty_and_refused(curve):
    lib, cid = api.lib(), api.CURVE_ID[curve]
    d = sentinel(4, 8)
    api.hash_to_field_indexed_dev(curve, HALO2, 0, 7, 0, d)
    api.hash_to_field_indexed_dev(curve, HALO2, 0, (1 << 32) - 1, 0, d)
    assert lib.trh_hash_to_field_indexed_dev(cid, HALO2, 0, 0, 0, None, None) == 0, "n = 0 needs no buffer"
    assert (host(d) == SENTINEL).all(), "n = 0 writes nothing"
    p = api._devptr(d)
    assert lib.trh_hash_to_field_indexed_dev(cid, HALO2, 0, (1 << 32) - 3, 4, p, None) == EINVAL and b"2^32" in lib.trh_last_error()  # first + n = 2^32 + 1
    assert lib.trh_hash_to_field_indexed_dev(cid, HALO2, 0, 1, 1 << 32, p, None) == EINVAL
    assert lib.trh_hash_to_field_indexed_dev(cid, _prefix(129), 0, 0, 1, p, None) == EINVAL and b"prefix" in lib.trh_last_error()
    assert lib.trh_hash_to_field_indexed_dev(cid, None, 0, 0, 1, p, None) == EINVAL
    assert lib.trh_hash_to_field_indexed_dev(cid, HALO2, 0, 0, 1, None, None) == EINVAL
    assert lib.trh_hash_to_field_indexed_dev(2, HALO2, 0, 0, 1, p, None) == EINVAL and b"unknown curve id" in lib.trh_last_error()
    assert lib.trh_hash_to_curve_indexed_dev(cid, HALO2, 0, (1 << 32) - 3, 4, p, None) == EINVAL and b"2^32" in lib.trh_last_error()
    assert lib.trh_hash_to_curve_indexed_dev(2, HALO2, 0, 0, 1, p, None) == EINVAL
    assert lib.trh_map_to_curve_dev(2, p, 1, 1, p, None) == EINVAL
    for per_point in (0, 3, -1):
        assert lib.trh_map_to_curve_dev(cid, p, 1, per_point, p, None) == EINVAL and b"per_point" in lib.trh_last_error()
    torch.cuda.synchronize()
    assert (host(d) == SENTINEL).all(), "a refused call writes nothing"


# ---- 2. / 3. the map ------------------------------------------------------------------------------------------------------------------------
def _map(curve, rows, per_point):
    """rows: (n * per_point, 4) stored limbs -> (n, 8) points"""
    n = rows.shape[0] // per_point
    d = sentinel(n + 2, 8)
    api.map_to_curve_dev(curve, dev(rows), n, per_point, d[1:])
    got = host(d)
    assert (got[0] == SENTINEL).all() and (got[n + 1] == SENTINEL).all(), "the launch wrote outside its n records"
    return got[1:n + 1]


def _model_map(curve, records):
    c = h2c.CURVES[curve]
    return np.array([h2c.point_limbs(c.m, c.map_sum(r)) for r in records], dtype=np.uint64).reshape(len(records), 8)


def _single_inputs(curve):
    c = h2c.CURVES[curve]
    rng = random.Random(0x51A6 + len(curve))
    us = [0, 1, c.m - 1]
    r = h2c.sqrt_mod(pow(13, -1, c.m), c.m)  # u^2 = -1 / Z = 1 / 13: tv2 = 0 there as at u = 0; no such u where 13 is a non-square
    if r is not None:
        us += [r, c.m - r]
    inv_r = pow(1 << 256, -1, c.m)
    us += [v * inv_r % c.m for v in common.edge_residue_ints(BASE_FIELD[curve])]  # the STORED forms sit at the edges of the nine-limb form
    us += [rng.randrange(c.m) for _ in range(200)]
    return us


@pytest.mark.parametrize("curve", CURVES)
def test_map_one_element_per_point(curve):
    c = h2c.CURVES[curve]
    us = _single_inputs(curve)
    branches = [c.gx1_is_square(u) for u in us[-200:]]
    assert 40 < sum(branches) < 160, "both branches of the map must occur among the random elements"
    got = _map(curve, mont_rows(curve, us), 1)
    want = _model_map(curve, [(u,) for u in us])
    assert (got == want).all(), differing(got, want)
    assert got.any(axis=1).all(), "map_to_curve never gives the identity"


def _pair_records(curve, n, seed):
    """n records; where they fit, the first slots of every run of 16 hold (u, -u), (u, u), (0, u), (u, 0), (0, 0), then the order is shuffled"""
    c = h2c.CURVES[curve]
    rng = random.Random(seed)
    recs = []
    for i in range(n):
        u = rng.randrange(1, c.m)
        recs.append([(u, c.m - u), (u, u), (0, u), (u, 0), (0, 0)][i % 16] if i % 16 < 5 else (u, rng.randrange(c.m)))
    rng.shuffle(recs)
    return recs


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("curve", CURVES)
def test_map_two_elements_per_point(curve, n):
    c = h2c.CURVES[curve]
    recs = _pair_records(curve, n, 0x2E1 + n)
    got = _map(curve, mont_rows(curve, [u for r in recs for u in r]), 2)
    want = _model_map(curve, recs)
    assert (got == want).all(), differing(got, want)
    for i, (u0, u1) in enumerate(recs):
        assert got[i].any() == ((u0 + u1) % c.m != 0 or u0 == 0), "(u, -u) and only it gives the all-zero POD"  # swu(0) + swu(0) is a doubling
    if n >= 63:
        doubled = [i for i, (u0, u1) in enumerate(recs) if u0 == u1 and u0]
        single = _map(curve, mont_rows(curve, [recs[i][0] for i in doubled]), 1)
        cv = o.CURVES[curve]
        for i, s in zip(doubled, single):
            assert cv.affine_limbs(cv.double(cv.affine_from_limbs([int(x) for x in s]))) == [int(x) for x in got[i]], "(u, u) is twice map(u)"


# ---- 4. the fused entry ---------------------------------------------------------------------------------------------------------------------
def _hash_to_curve(curve, prefix, tag, first, n):
    d = sentinel(n + 2, 8)
    api.hash_to_curve_indexed_dev(curve, prefix, tag, first, n, d[1:])
    got = host(d)
    assert (got[0] == SENTINEL).all() and (got[n + 1] == SENTINEL).all(), "the launches wrote outside their n records"
    return got[1:n + 1]


@pytest.mark.parametrize("first,n", RANGES)
@pytest.mark.parametrize("curve", CURVES)
def test_fused_entry_index_ranges(curve, first, n):
    got = _hash_to_curve(curve, HALO2, 0, first, n)
    want = model_points(curve, HALO2, 0, first, n)
    assert (got == want).all(), differing(got, want)
    for i in sorted({0, n // 2, n - 1}):
        msg = b"\x00" + (first + i).to_bytes(4, "little")
        assert (api.hash_to_curve(curve, HALO2, msg) == got[i]).all(), f"host entry and device disagree at index {first + i}"
    # the two kernels on their own give what the fused entry gives
    u = sentinel(n, 8)
    api.hash_to_field_indexed_dev(curve, HALO2, 0, first, n, u)
    assert (_map(curve, host(u).reshape(2 * n, 4), 2) == got).all()


@pytest.mark.parametrize("length", PREFIX_LENGTHS)
@pytest.mark.parametrize("curve", CURVES)
def test_fused_entry_prefixes_and_tags(curve, length):
    got = _hash_to_curve(curve, _prefix(length), 0xA7, 250, 12)
    want = model_points(curve, _prefix(length), 0xA7, 250, 12)
    assert (got == want).all(), differing(got, want)


@pytest.mark.parametrize("curve", CURVES)
def test_fused_entry_empty(curve):
    d = sentinel(3, 8)
    api.hash_to_curve_indexed_dev(curve, HALO2, 0, 5, 0, d)
    assert (host(d) == SENTINEL).all()


# ---- 5. Params.new --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def params_file(curve, k):
    """(Params.new(curve, k), the bytes it writes): made once per shape"""
    p = poly.Params.new(curve, k)
    buf = io.BytesIO()
    p.write(buf)
    return p, buf.getvalue()


@pytest.mark.parametrize("k", [1, 4, 7])
@pytest.mark.parametrize("curve", CURVES)
def test_params_new_against_the_model(curve, k):
    c, n = h2c.CURVES[curve], 1 << k
    p, _ = params_file(curve, k)
    g = p._g.download()
    assert g.shape == (n + 1, 8) and (g[:n] == model_points(curve, HALO2, 0, 0, n)).all()
    w, u = h2c.point_limbs(c.m, h2c.params_w(curve)), h2c.point_limbs(c.m, h2c.params_u(curve))
    assert g[n].tolist() == w and np.asarray(p.w).reshape(8).tolist() == w and np.asarray(p.u).reshape(8).tolist() == u
    assert p._g_lagrange.download()[n].tolist() == w
    # g_lagrange is the Lagrange basis of g: commit_lagrange(column) = commit(lagrange_to_coeff(column)), same blind
    sf = o.FIELDS[api.SCALAR_FIELD[curve]]
    rng = random.Random(0xC01 + k + len(curve))
    column = [rng.randrange(sf.m) for _ in range(n)]
    coeffs = o.EvaluationDomain(sf, 2, k).lagrange_to_coeff(list(column))
    limbs = lambda vals: np.array([sf.limbs(sf.to_mont(v)) for v in vals], dtype=np.uint64).reshape(-1, 4)
    blind = limbs([rng.randrange(sf.m)])[0]
    assert (p.commit_lagrange(limbs(column), blind) == p.commit(limbs(coeffs), blind)).all()


@pytest.mark.parametrize("k", [1, 4, 7])
@pytest.mark.parametrize("curve", CURVES)
def test_params_new_write_read_round_trip(curve, k):
    p, file = params_file(curve, k)
    n = 1 << k
    assert len(file) == 4 + 32 * (2 * n + 2) and file[:4] == k.to_bytes(4, "little")
    q = poly.Params.read(curve, io.BytesIO(file))
    assert (q._g.download() == p._g.download()).all() and (q._g_lagrange.download() == p._g_lagrange.download()).all()
    assert (np.asarray(q.u).reshape(8) == np.asarray(p.u).reshape(8)).all()
    buf = io.BytesIO()
    q.write(buf)
    assert buf.getvalue() == file
    # the first encoding is g[0] of the model: x canonical, little endian, the parity of y in the top bit
    x, y = h2c.params_g(curve, 0)
    assert file[4:36] == (x | (y & 1) << 255).to_bytes(32, "little")


@pytest.mark.parametrize("curve", CURVES)
def test_native_params_create_writes_the_same_file(curve, tmp_path):
    """tests/native/params_new_test.cpp: trh::Params::create over include/trh.hpp from a compiled host"""
    exe = os.path.join(ROOT, "tests", "native", "params_new_test")
    if not os.path.exists(exe):  # normally built by `make` / __graft_entry__.build(); g++ only, libtrh.so must already be there
        subprocess.check_call(["make", "-s", "-C", ROOT, "tests/native/params_new_test"])
    prefix = str(tmp_path / f"{curve}_k")
    r = subprocess.run([exe, curve, prefix, "1", "4", "7"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["checks_failed"] == 0 and res["files"] == 3
    for k in (1, 4, 7):
        assert open(f"{prefix}{k}.params", "rb").read() == params_file(curve, k)[1], f"k = {k}"
