"""GPU tests (-m gpu) of csrc/encoding.hip: the device square root, the 32-byte point encoding in both directions, resident base sets
made from compressed points (single device and range-sharded) and Params.read / Params.write.  Every expected value comes from
oracle/pasta.py through tests/encoding_cases.py (the records of tests/test_encoding_host.py, the Python encoder / decoder); the round
trip at the prover's own size compares the device with itself and needs no oracle square root."""
import ctypes
import functools
import io
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import cpu_ref
import encoding_cases as ec
import pasta as o
from tiny_ram_halo2_amd import api, poly, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["fp", "fq"]
CURVES = ["pallas", "vesta"]


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


def dev_u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def dev_bytes(b):
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()


def host_u64(t, cols):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64).reshape(-1, cols)


def generated(curve, n, seed=0):
    """a resident set of n device-generated points (the caller destroys it)"""
    return api.Bases.generate(curve, synth.BASE_S0 + seed, synth.BASE_D, n)


# ---- trh_field_sqrt_dev ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("field", FIELDS)
def test_field_sqrt_dev_matches_the_oracle(field, n):
    a = ec.sqrt_input_limbs(field)
    want_r, want_f = ec.sqrt_expected_limbs(field)
    idx = np.arange(n) % len(a) if n >= len(a) else (np.arange(n) * 37 + n) % len(a)  # the small sizes start inside the records of the 2-part
    d_a, d_out, d_fl = dev_u64(a[idx]), torch.zeros((n, 4), dtype=torch.int64, device="cuda"), torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    api.field_sqrt_dev(field, d_a, d_out, d_fl, n)
    got_r, got_f = host_u64(d_out, 4), d_fl.cpu().numpy()
    assert (got_f == want_f[idx]).all(), np.nonzero(got_f != want_f[idx])[0][:10]
    assert (got_r == want_r[idx]).all(), np.nonzero((got_r != want_r[idx]).any(axis=1))[0][:10]
    if n == 4097:  # every record went through: the same checker as the host branch (flag, r^2 = a, even root)
        assert not ec.check_sqrt(field, got_r[:len(a)], got_f[:len(a)])


@pytest.mark.parametrize("field", FIELDS)
def test_field_sqrt_dev_n0(field):
    assert api.lib().trh_field_sqrt_dev(api.FIELD_ID[field], None, None, None, 0, None) == 0


# ---- trh_points_decompress_dev --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def decompress_cases(curve):
    """x = 0 .. 2047 with both signs, the special encodings and an identity in the middle; the oracle's answer for each (one square root per x)"""
    cv = o.CURVES[curve]
    encs, want = [], []
    for x in range(2048):
        pt = cv.lift_x(x)
        for s in (0, 1):
            encs.append(ec.enc_int(x, s))
            if x == 0 and s == 0:
                want.append(None)  # the all-zero encoding is the identity, whatever x = 0 is
            elif pt is None:
                want.append(ec.INVALID)
            else:
                want.append((x, pt[1] if pt[1] & 1 == s else cv.base.m - pt[1]))
        if x == 1000:
            encs.append(bytes(32))
            want.append(None)
    for _, e in ec.special_encodings(curve):
        encs.append(e)
        want.append(ec.decode(curve, e))
    return tuple(encs), tuple(want)


def test_decompress_cases_are_about_half_valid():
    for curve, first256 in (("pallas", 135), ("vesta", 125)):
        cv = o.CURVES[curve]
        assert sum(1 for x in range(256) if cv.lift_x(x) is not None) == first256
        encs, want = decompress_cases(curve)
        assert all(ec.decode(curve, e) == w for e, w in zip(encs[:64] + encs[-9:], want[:64] + want[-9:]))  # the table above against the definition


@pytest.mark.parametrize("curve", CURVES)
def test_points_decompress_dev(curve):
    encs, want = decompress_cases(curve)
    n = len(encs)
    valid = np.array([w != ec.INVALID for w in want], np.uint8)
    pods = np.array([ec.pod(curve, w) for w in want], np.uint64)
    first_invalid = int(np.nonzero(valid == 0)[0][0])
    d_enc = dev_bytes(b"".join(encs))
    d_xy, d_ok = torch.full((n, 8), -1, dtype=torch.int64, device="cuda"), torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    assert api.points_decompress_dev(curve, d_enc, d_xy, n, ok_dev=d_ok) == first_invalid
    got_ok, got = d_ok.cpu().numpy(), host_u64(d_xy, 8)
    assert (got_ok == valid).all(), np.nonzero(got_ok != valid)[0][:10]
    assert (got == pods).all(), np.nonzero((got != pods).any(axis=1))[0][:10]
    assert (got[valid == 0] == 0).all()
    # the same without the validity array and without the read-back
    d_xy2 = torch.full((n, 8), -1, dtype=torch.int64, device="cuda")
    assert api.points_decompress_dev(curve, d_enc, d_xy2, n, first_bad=False) is None
    assert (host_u64(d_xy2, 8) == pods).all()
    # the invalid ones removed: first_bad == n
    good = [e for e, v in zip(encs, valid) if v]
    d_xy3 = torch.zeros((len(good), 8), dtype=torch.int64, device="cuda")
    assert api.points_decompress_dev(curve, dev_bytes(b"".join(good)), d_xy3, len(good)) == len(good)
    assert (host_u64(d_xy3, 8) == pods[valid == 1]).all()
    assert api.points_decompress_dev(curve, d_enc, d_xy, 0) == 0


# ---- trh_points_compress_dev ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 4097])
@pytest.mark.parametrize("curve", CURVES)
def test_points_compress_dev(curve, n):
    b = generated(curve, n, seed=n)
    xy = b.download()
    d_enc = torch.full((n * 32,), 0x5a, dtype=torch.uint8, device="cuda")
    api.points_compress_dev(curve, api.lib().trh_bases_device_ptr(b.handle), d_enc, n)
    torch.cuda.synchronize()
    assert d_enc.cpu().numpy().tobytes() == ec.encode_pods(curve, xy)
    b.destroy()


@pytest.mark.parametrize("curve", CURVES)
def test_points_compress_dev_with_identities(curve):
    n = 200
    b = generated(curve, n)
    xy = b.download()
    for i in (0, 63, 64, 130, n - 1):
        xy[i] = 0
    d_enc = torch.full((n * 32,), 0x5a, dtype=torch.uint8, device="cuda")
    api.points_compress_dev(curve, dev_u64(xy), d_enc, n)
    torch.cuda.synchronize()
    got = d_enc.cpu().numpy().tobytes()
    assert got == ec.encode_pods(curve, xy) and got[:32] == bytes(32) and got[63 * 32:65 * 32] == bytes(64)
    b.destroy()


@pytest.mark.parametrize("curve", CURVES)
def test_round_trip_at_the_provers_size(curve):
    """2^18 + 1 points (Params.g ‖ w at the reference's k): compress, decompress, the bytes of the originals come back"""
    n = (1 << 18) + 1
    b = generated(curve, n, seed=18)
    src = api.lib().trh_bases_device_ptr(b.handle)
    d_enc = torch.zeros((n * 32,), dtype=torch.uint8, device="cuda")
    d_xy, d_ok = torch.zeros((n, 8), dtype=torch.int64, device="cuda"), torch.zeros((n,), dtype=torch.uint8, device="cuda")
    api.points_compress_dev(curve, src, d_enc, n)
    assert api.points_decompress_dev(curve, d_enc, d_xy, n, ok_dev=d_ok) == n
    assert bool((d_ok == 1).all())
    assert (host_u64(d_xy, 8) == b.download()).all()
    b.destroy()


# ---- trh_bases_create_compressed / trh_bases_download_compressed ----------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_bases_create_compressed(curve):
    n = 4097
    src = generated(curve, n, seed=3)
    xy = src.download()
    data = ec.encode_pods(curve, xy)
    b = api.Bases.from_compressed(curve, data)
    assert len(b) == n and b.shards() == 1
    assert (b.download() == xy).all()
    assert b.download_compressed() == data and b.download_compressed(100, 33) == data[3200:3200 + 33 * 32]
    plain = api.Bases.from_host(curve, xy)
    sc = synth.field_elements(0xE1C0 + len(curve), n)
    want = cpu_ref.to_affine(curve, cpu_ref.best_multiexp(curve, sc, xy, threads=4))
    got = b.msm(sc)
    assert (got == plain.msm(sc)).all() and (np.asarray(got)[:8] == want).all()
    assert b.precompute(0) > 0 and plain.precompute(0) > 0
    got = b.msm(sc)
    assert (got == plain.msm(sc)).all() and (np.asarray(got)[:8] == want).all()
    # one corrupted encoding: the error names it, the handle is untouched, and the next create works
    bad = bytearray(data)
    bad[2049 * 32:2050 * 32] = ec.enc_int(2, 1)  # x = 2 is on neither curve
    buf = np.frombuffer(bytes(bad), dtype=np.uint8)
    h = ctypes.c_void_p(0x1234)
    assert api.lib().trh_bases_create_compressed(api.CURVE_ID[curve], buf.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(h)) == -1
    assert b"2049" in api.lib().trh_last_error() and h.value == 0x1234
    with pytest.raises(api.TrhError, match="2049"):
        api.Bases.from_compressed(curve, bytes(bad))
    again = api.Bases.from_compressed(curve, data)
    assert (again.download(2040, 20) == xy[2040:2060]).all()
    empty = api.Bases.from_compressed(curve, b"")
    assert len(empty) == 0
    for s in (src, b, plain, again, empty):
        s.destroy()


SHARDED_SCRIPT = r"""
import numpy as np, torch
import cpu_ref, encoding_cases as ec
from tiny_ram_halo2_amd import api, synth
api.init_multi([0, 0])
api.set_shard_min(1024)
for curve in ("pallas", "vesta"):
    n = 2049
    src = api.Bases.generate(curve, synth.BASE_S0 + 5, synth.BASE_D, n)
    xy = src.download()
    data = ec.encode_pods(curve, xy)
    b = api.Bases.from_compressed(curve, data)
    assert b.shards() == 2 and len(b) == n
    assert (b.download() == xy).all() and b.download_compressed() == data and b.download_compressed(1000, 100) == data[32000:35200]
    sc = synth.field_elements(0xE1C1, n)
    want = cpu_ref.to_affine(curve, cpu_ref.best_multiexp(curve, sc, xy, threads=4))
    assert (np.asarray(b.msm(sc))[:8] == want).all()
    bad = bytearray(data)
    bad[1500 * 32:1501 * 32] = ec.enc_int(2)
    try:
        api.Bases.from_compressed(curve, bytes(bad))
        raise SystemExit("a corrupted encoding in the second shard was accepted")
    except api.TrhError as e:
        assert "1500" in str(e), str(e)
    print("sharded ok", curve)
"""


def test_bases_create_compressed_sharded():
    """a device group {0, 0} in a fresh process (the suite's own group is another list): 2049 encodings become two shards, the MSM over them
    is the oracle's, and an invalid encoding in the second shard is named by its index in the caller's array"""
    from common import run_with_options
    out = run_with_options(SHARDED_SCRIPT, {})
    assert "sharded ok pallas" in out and "sharded ok vesta" in out


# ---- Params.read / Params.write -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def params_k10():
    made = {}

    def get(curve):
        if curve not in made:
            k, n = 10, 1 << 10
            g = cpu_ref.gen_bases(curve, 11, 3, n, threads=4)
            gl = host_u64(poly.Params.g_lagrange_from_g(curve, k, dev_u64(g)), 8)
            w = cpu_ref.gen_bases(curve, 999, 1, 1, threads=1)
            u = cpu_ref.gen_bases(curve, 4242, 1, 1, threads=1)
            p = poly.Params(curve, k, g, gl, w, u.reshape(8))
            want = int(k).to_bytes(4, "little") + ec.encode_pods(curve, g) + ec.encode_pods(curve, gl) + ec.encode_pods(curve, w) + ec.encode_pods(curve, u)
            made[curve] = (p, want)
        return made[curve]
    return get


@pytest.mark.parametrize("curve", CURVES)
def test_params_write_read(params_k10, curve):
    p, want = params_k10(curve)
    n = p.n
    f = io.BytesIO()
    p.write(f)
    data = f.getvalue()
    assert len(data) == 4 + 32 * 2050 and data == want
    q = poly.Params.read(curve, io.BytesIO(data))
    assert q.k == 10 and q.n == n and (q.w.reshape(8) == p.w.reshape(8)).all() and (np.asarray(q.u).reshape(8) == np.asarray(p.u).reshape(8)).all()
    col = synth.field_elements(0xFA11, n)
    r = synth.field_elements(0xFA12, 1)[0]
    assert (q.commit(col, r) == p.commit(col, r)).all() and (q.commit_lagrange(col, r) == p.commit_lagrange(col, r)).all()
    d_col = dev_u64(col)
    assert (q.commit(d_col, r) == p.commit(col, r)).all()
    ipa = q.ipa_bases()
    assert len(ipa) == n + 2 and int(api.lib().trh_bases_precomputed_window_bits(ipa.handle)) != 0
    assert (ipa.download() == p.ipa_bases().download()).all()
    g = io.BytesIO()
    q.write(g)
    assert g.getvalue() == data
    plain = poly.Params.read(curve, io.BytesIO(data), precompute=False)
    assert int(api.lib().trh_bases_precomputed_window_bits(plain._g.handle)) == 0 and (plain.commit(col, r) == p.commit(col, r)).all()


@pytest.mark.parametrize("curve", CURVES)
def test_params_read_rejects_bad_files(params_k10, curve):
    _, data = params_k10(curve)
    n = 1 << 10
    with pytest.raises(ValueError, match="truncated"):
        poly.Params.read(curve, io.BytesIO(data[:-1]))
    with pytest.raises(ValueError, match="truncated"):
        poly.Params.read(curve, io.BytesIO(data[:3]))
    for section, index, at in (("g", 5, 4 + 32 * 5), ("g_lagrange", 17, 4 + 32 * (n + 17)), ("w", 0, 4 + 64 * n), ("u", 0, 4 + 64 * n + 32)):
        bad = bytearray(data)
        bad[at:at + 32] = ec.enc_int(o.CURVES[curve].base.m + 1)  # aliases x = 1, a point: it must be rejected, not reduced
        with pytest.raises(ValueError, match=rf"{section}\[{index}\]"):
            poly.Params.read(curve, io.BytesIO(bytes(bad)), precompute=False)


def test_native_params_round_trip():
    """tests/native/params_io_test.cpp: trh::Params::write / read over include/trh.hpp from a compiled host"""
    exe = os.path.join(ROOT, "tests", "native", "params_io_test")
    if not os.path.exists(exe):  # normally built by `make` / __graft_entry__.build(); g++ only, libtrh.so must already be there
        subprocess.check_call(["make", "-s", "-C", ROOT, "tests/native/params_io_test"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert json.loads(r.stdout.strip().splitlines()[-1])["checks_failed"] == 0
