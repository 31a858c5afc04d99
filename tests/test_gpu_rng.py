"""GPU tests (-m gpu) of csrc/random.hip: the random-scalar stream expanded on the device (trh_rng_fill_dev / trh_rng_fill_rows_dev), bit for bit
against tests/chacha_model.py -- the model tests/test_rng_host.py pins by RFC 8439's vector and Python integers.  Sizes cross one wavefront,
one workgroup and many workgroups; positions cross the counter's 32-bit carry inside one launch and end on the stream's last block.  The
refusals are argument checks that return before any launch."""
import ctypes
import functools
import json
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import chacha_model as cm
import cpu_ref
import pasta as o
from common import DeviceTranscript
from tiny_ram_halo2_amd import api, ipa, poly

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["fp", "fq"]
EINVAL = -1
SEED = bytes((0x5b + 29 * i) & 0xff for i in range(32))
STREAM = 0x8badf00d12345678
START = 0x1_0000_0123  # a position whose high counter word is not zero
SENTINEL = 0x5E5E5E5E5E5E5E5E
N_MAX = (1 << 16) + 3


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


@functools.lru_cache(maxsize=None)
def model(field, first=START, n=N_MAX):
    """elements first .. first + n - 1 as Montgomery limbs: computed once per field, shared by the tests, never written to"""
    a = cm.elements_limbs(field, SEED, first, n, STREAM)
    a.setflags(write=False)
    return a


def sentinel(n_elems):
    return torch.full((n_elems, 4), SENTINEL, dtype=torch.int64, device="cuda")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64).reshape(-1, 4)


def rng_at(pos):
    r = api.Rng(SEED, STREAM)
    r.seek(pos)
    return r


# ---- fill -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, N_MAX])
@pytest.mark.parametrize("field", FIELDS)
def test_fill_matches_the_model(field, n):
    rng = rng_at(START)
    d = sentinel(n + 2)  # one element of margin on either side: the launch writes n elements and no more
    rng.fill(field, d[1:], n)
    got = host(d)
    assert rng.position() == START + n
    assert (got[0] == SENTINEL).all() and (got[n + 1] == SENTINEL).all()
    want = model(field)[:n]
    assert (got[1:n + 1] == want).all(), np.nonzero((got[1:n + 1] != want).any(axis=1))[0][:10]


@pytest.mark.parametrize("field", FIELDS)
def test_fill_across_the_counter_carry(field):
    first = (1 << 32) - 3
    rng = rng_at(first)
    d = sentinel(8)
    rng.fill(field, d, 8)
    assert (host(d) == cm.elements_limbs(field, SEED, first, 8, STREAM)).all()
    assert rng.position() == (1 << 32) + 5


@pytest.mark.parametrize("field", FIELDS)
def test_fill_to_the_last_block_and_not_past_it(field):
    lib = api.lib()
    first = (1 << 64) - 4
    rng = rng_at(first)
    d = sentinel(5)
    assert lib.trh_rng_fill_dev(rng.handle, api.FIELD_ID[field], api._devptr(d), 5, None) == EINVAL  # 2^64 - 4 + 5 > 2^64
    assert "end of the stream" in lib.trh_last_error().decode()
    assert (host(d) == SENTINEL).all() and rng.position() == first
    rng.fill(field, d, 4)
    got = host(d)
    assert (got[:4] == cm.elements_limbs(field, SEED, first, 4, STREAM)).all() and (got[4] == SENTINEL).all()
    # the position is 2^64 now: nothing more, on the device or on the host, until a seek
    assert lib.trh_rng_fill_dev(rng.handle, api.FIELD_ID[field], api._devptr(d), 1, None) == EINVAL
    out = np.zeros(4, np.uint64)
    assert lib.trh_rng_next_scalar(rng.handle, api.FIELD_ID[field], api._p(out)) == EINVAL
    assert (host(d)[:4] == got[:4]).all()
    rng.seek(first)
    assert rng.position() == first


@pytest.mark.parametrize("field", FIELDS)
def test_fills_and_host_draws_share_one_position(field):
    want = model(field)
    a, b = rng_at(START), rng_at(START)
    d1, d2 = sentinel(12), sentinel(12)
    a.fill(field, d1, 5)
    a.fill(field, d1[5:], 7)
    b.fill(field, d2, 12)
    assert (host(d1) == host(d2)).all() and (host(d1) == want[:12]).all()
    c = rng_at(START)
    d3 = sentinel(12)
    c.fill(field, d3, 5)
    mid = c.next_scalar(field)  # takes exactly position START + 5
    c.fill(field, d3[5:], 7)
    got = host(d3)
    assert (got[:5] == want[:5]).all() and (mid == want[5]).all() and (got[5:] == want[6:13]).all()
    assert c.position() == START + 13
    api.lib().trh_rng_fill_dev(c.handle, api.FIELD_ID[field], None, 0, None)
    assert c.position() == START + 13  # n = 0 does nothing


# ---- fill_rows --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_fill_rows_writes_the_blinding_cells_only(field):
    rows, row_len, first, count = 3, 64, 58, 6
    want = model(field)
    rng = rng_at(START)
    d = sentinel(rows * row_len + 2)
    d[:, 1] = torch.arange(rows * row_len + 2, device="cuda")  # every cell its own pattern
    before = host(d).copy()
    rng.fill_rows(field, d[1:], rows, row_len, first, count)
    got = host(d)
    assert rng.position() == START + rows * count
    written = np.zeros(rows * row_len + 2, bool)
    for r in range(rows):
        for c in range(count):
            cell = 1 + r * row_len + first + c
            written[cell] = True
            assert (got[cell] == want[r * count + c]).all(), (r, c)
    assert written.sum() == 18 and (got[~written] == before[~written]).all()
    # one row, every cell: the same as a fill
    rng.seek(START)
    d1 = sentinel(row_len + 1)
    rng.fill_rows(field, d1, 1, row_len, 0, row_len)
    g1 = host(d1)
    assert (g1[:row_len] == want[:row_len]).all() and (g1[row_len] == SENTINEL).all() and rng.position() == START + row_len
    # count = 0 and rows = 0 do nothing
    rng.fill_rows(field, d1, 1, row_len, 64, 0)
    rng.fill_rows(field, d1, 0, row_len, 0, row_len)
    assert (host(d1) == g1).all() and rng.position() == START + row_len
    lib = api.lib()
    assert lib.trh_rng_fill_rows_dev(rng.handle, api.FIELD_ID[field], api._devptr(d1), 1, row_len, 60, 5, None) == EINVAL  # first + count > row_len
    assert (host(d1) == g1).all() and rng.position() == START + row_len


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_unknown_field_id_on_the_device_entries():
    lib = api.lib()
    want = model("fp")
    rng = rng_at(START)
    d = sentinel(64)
    assert lib.trh_rng_fill_dev(rng.handle, 7, api._devptr(d), 4, None) == EINVAL
    assert lib.trh_last_error().decode() == "unknown field id 7"
    assert lib.trh_rng_fill_rows_dev(rng.handle, 7, api._devptr(d), 2, 32, 30, 2, None) == EINVAL
    assert lib.trh_last_error().decode() == "unknown field id 7"
    assert (host(d) == SENTINEL).all() and rng.position() == START
    assert lib.trh_rng_fill_dev(rng.handle, 0, api._devptr(d), 4, None) == 0
    assert lib.trh_rng_fill_rows_dev(rng.handle, 0, api._devptr(d[32:]), 1, 32, 30, 2, None) == 0
    got = host(d)
    assert (got[:4] == want[:4]).all() and (got[62:64] == want[4:6]).all() and (got[4:62] == SENTINEL).all()
    assert rng.position() == START + 6


# ---- the opening with the library's own randomness --------------------------------------------------------------------------------------
def test_opening_with_device_drawn_s_poly_verifies():
    """k = 8: s(X) filled by Rng.fill, the round blinds drawn through the adapter (ipa.RngScalarFn -> trh_rng_next_scalar inside the locked
    context), s_blind by a host draw; the device verifier accepts the opening and rejects it with f + 1.  The s coefficients downloaded before
    the call and the position after it are the model's."""
    curve, k = "vesta", 8
    cv = o.CURVES[curve]
    fs, sf = cv.scalar, api.SCALAR_FIELD[curve]
    n = 1 << k
    rnd = random.Random(0x5EED)
    g_l = cpu_ref.gen_bases(curve, 29, 13, n, threads=4)
    w_l = cpu_ref.gen_bases(curve, 515153, 1, 1, threads=1)
    u_l = cpu_ref.gen_bases(curve, 626264, 1, 1, threads=1)
    params = poly.Params(curve, k, g_l, g_l, w_l, u=u_l)
    p_l = np.array([fs.limbs(rnd.randrange(fs.m)) for _ in range(n)], np.uint64)
    p_blind, x3 = rnd.randrange(fs.m), rnd.randrange(fs.m)
    p_dev = torch.from_numpy(p_l.view(np.int64).copy()).cuda()
    commitment = cpu_ref.to_affine(curve, params.commit(p_l, np.array(fs.limbs(p_blind), np.uint64)))

    rng = rng_at(START)
    s_dev = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    rng.fill(sf, s_dev, n, stream=torch.cuda.current_stream().cuda_stream)
    s_host = host(s_dev).copy()
    assert (s_host == model(sf)[:n]).all()
    s_blind = fs.from_limbs(rng.next_scalar(sf))
    assert s_blind == cm.element(sf, SEED, START + n, STREAM)

    class Rec(DeviceTranscript):
        def __init__(self, m):
            super().__init__(m)
            self.points, self.challenges = [], []

        def write_point(self, jac):
            self.points.append(np.ascontiguousarray(jac, dtype=np.uint64)[:8].copy())
            super().write_point(jac)

        def squeeze_challenge_scalar(self):
            c = super().squeeze_challenge_scalar()
            self.challenges.append(c)
            return c

    tr = Rec(fs.m)
    adapter = ipa.RngScalarFn(rng, curve)
    c, f = ipa.create_proof_native(params, adapter, tr, p_dev, p_blind, x3, s_dev, s_blind)
    assert adapter.error is None
    assert rng.position() == START + n + 1 + 2 * k  # two round blinds per round, nothing else
    assert len(tr.points) == 1 + 2 * k and len(tr.challenges) == 2 + k
    v = fs.from_limbs(cpu_ref.eval_polynomial(sf, p_l, np.array(fs.limbs(x3), np.uint64)))
    rounds = [(tr.points[1 + 2 * j], tr.points[2 + 2 * j], tr.challenges[2 + j]) for j in range(k)]
    args = (params, [(1, commitment)], v, x3, tr.points[0], tr.challenges[0], tr.challenges[1], rounds, c)
    assert ipa.batch_verify(params, [ipa.verify_proof(*args, f)], [1])
    assert not ipa.batch_verify(params, [ipa.verify_proof(*args, (f + 1) % fs.m)], [1])


# ---- trh::Rng from C++ ------------------------------------------------------------------------------------------------------------------
def _fnv(limbs):
    h = 0xcbf29ce484222325
    for w in np.asarray(limbs, dtype=np.uint64).reshape(-1):
        h = ((h ^ int(w)) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def test_rng_from_cpp():
    """tests/native/rng_fill_test.cpp: trh::Rng over include/trh.hpp from a compiled host -- fill, next_scalar, fill_rows, position"""
    exe = os.path.join(ROOT, "tests", "native", "rng_fill_test")
    if not os.path.exists(exe):  # normally built by `make` / __graft_entry__.build(); g++ only, libtrh.so must already be there
        subprocess.check_call(["make", "-s", "-C", ROOT, "tests/native/rng_fill_test"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["checks_failed"] == 0
    seed = bytes((0xa5 ^ (7 * i)) & 0xff for i in range(32))
    stream, pos, n, rows, row_len, first, count = 0x0123456789abcdef, 77, 1000, 3, 40, 34, 6
    for field in FIELDS:
        want = cm.elements_limbs(field, seed, pos, n + 1 + rows * count, stream)
        assert got[f"{field}_fill"] == _fnv(want[:n]), field
        assert got[f"{field}_next"] == _fnv(want[n]), field
        cols = np.zeros((rows * row_len, 4), np.uint64)
        for r_ in range(rows):
            cols[r_ * row_len + first:r_ * row_len + first + count] = want[n + 1 + r_ * count:n + 1 + (r_ + 1) * count]
        assert got[f"{field}_rows"] == _fnv(cols), field
