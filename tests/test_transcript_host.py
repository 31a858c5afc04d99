"""CPU tests of the proof transcript (csrc/blake2b.h with a personalisation, csrc/transcript.h, the trh_tr_* entries, include/trh.hpp's
Blake2bWrite / Blake2bRead, tiny_ram_halo2_amd.transcript), no GPU and no trh_init.  The independent side is tests/transcript_model.py:
hashlib's BLAKE2b, Python integers, oracle/pasta.py.
1. The hash with the personalisation in a stand-alone program (tests/native/transcript_test.cpp) under address + undefined sanitizers, against
   hashlib at the lengths where "a full buffer is compressed only when more input follows" and the final flag can go wrong.
2. The sponge through ctypes against the model on both curves: a script of commons, writes and squeezes whose squeezes fall on absorbed totals
   of 127, 128, 129 and 255, 256, 257 bytes; every challenge and the final bytes.
3. The round trip through a reader; finished() exactly at the end.
4. The refusals, each with its latched status and with everything after it a no-op that leaves its outputs zero.
5. The filled trh_transcript_t called from ctypes as C function pointers.
6. The same script through trh.hpp inside the stand-alone program (which also round-trips it and tries the refusals in C++)."""
import ctypes
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

import pasta as o
import transcript_model as tm
from tiny_ram_halo2_amd import api, transcript

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["pallas", "vesta"]
EINVAL = -1
HASH_LENGTHS = [0, 1, 127, 128, 129, 255, 256, 257]


@pytest.fixture(scope="module")
def exe():
    path = os.path.join(ROOT, "tests", "native", "transcript_test")
    if not os.path.exists(path):  # normally built by `make` / __graft_entry__.build(); g++ only
        subprocess.check_call(["make", "-s", "-C", ROOT, "tests/native/transcript_test"])
    return path


def _run(exe, args):
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


# ---- 1. the hash ----------------------------------------------------------------------------------------------------------------------
def test_personalised_blake2b_against_hashlib(exe, tmp_path):
    msgs = [bytes((5 * i + n) & 0xff for i in range(n)) for n in HASH_LENGTHS]
    src, dst = tmp_path / "hash.in", tmp_path / "hash.out"
    src.write_bytes(b"".join(struct.pack("<I", len(m)) + m for m in msgs))
    assert f"{len(msgs)} digests ok" in _run(exe, ["hash", str(src), str(dst)])
    got = dst.read_bytes()
    assert len(got) == 64 * len(msgs)
    for i, m in enumerate(msgs):
        assert got[64 * i:64 * i + 64] == hashlib.blake2b(m, digest_size=64, person=tm.PERSON).digest(), f"{len(m)} bytes"
    assert got[:64] != hashlib.blake2b(b"", digest_size=64).digest(), "the personalisation takes part"


# ---- the script -----------------------------------------------------------------------------------------------------------------------
def _jacobian(cv, pt):
    return np.array(cv.affine_limbs(pt) + cv.base.limbs(1), dtype=np.uint64)


def _scalar(cv, v):
    return np.array(cv.scalar.limbs(v), dtype=np.uint64)


def script(curve):
    """(kind, limbs or None) operations: 'p' / 'P' common / write point, 's' / 'S' common / write scalar, 'C' squeeze.  Absorbed totals: a point
    is 65 bytes, a scalar 33, a squeeze 1.  P S -> 98, then 31 squeezes at 99 .. 129 (127, 128 -- the digest of a full block -- and 129, whose
    absorb has to compress that block without the final flag); p s -> 227, then 30 squeezes at 228 .. 257 (255, 256, 257); then one of each
    again, so that the state after the second full block is used too."""
    cv = o.CURVES[curve]
    g = cv.generator
    pts = [_jacobian(cv, cv.mul(k, g)) for k in (1, 2, 3, 7)]
    m = cv.scalar.m
    ops = [("P", pts[0]), ("S", _scalar(cv, m - 1))] + [("C", None)] * 31
    ops += [("p", pts[1]), ("s", _scalar(cv, 0x1234567 ** 9 % m))] + [("C", None)] * 30
    ops += [("P", pts[2]), ("C", None), ("S", _scalar(cv, 0)), ("S", _scalar(cv, 1)), ("p", pts[3]), ("C", None), ("P", pts[3]), ("C", None)]
    return ops


def absorbed_at_squeezes(ops):
    total, at = 0, []
    for kind, _ in ops:
        total += {"p": 65, "P": 65, "s": 33, "S": 33, "C": 1}[kind]
        if kind == "C":
            at.append(total)
    return at


def play(writer, ops):
    """-> the challenges"""
    out = []
    for kind, v in ops:
        if kind == "C":
            out.append(writer.squeeze_challenge_scalar())
        else:
            {"p": writer.common_point, "P": writer.write_point, "s": writer.common_scalar, "S": writer.write_scalar}[kind](v)
    return out


def test_the_script_squeezes_where_the_blocks_end():
    at = absorbed_at_squeezes(script("pallas"))
    assert {127, 128, 129, 255, 256, 257} <= set(at)


# ---- 2. the sponge against the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_sponge_against_the_model(curve):
    ops = script(curve)
    w, model = transcript.Blake2bWrite(curve), tm.Writer(curve)
    got, want = play(w, ops), play(model, ops)
    assert got == want and len(set(got)) == len(got) == 64
    assert all(0 <= c < o.CURVES[curve].scalar.m for c in got)
    proof = w.finalize()
    assert proof == model.finalize() and len(proof) == 32 * sum(kind in "PS" for kind, _ in ops)
    w.raise_if_failed()
    # affine points in: the same bytes
    w2 = transcript.Blake2bWrite(curve)
    assert play(w2, [(kind, v[:8] if kind in "pP" else v) for kind, v in ops]) == want and w2.finalize() == proof


# ---- 3. the round trip ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_round_trip_through_a_reader(curve):
    cv = o.CURVES[curve]
    ops = script(curve)
    w = transcript.Blake2bWrite(curve)
    challenges = play(w, ops)
    proof = w.finalize()
    for r in (transcript.Blake2bRead(curve, proof), tm.Reader(curve, proof)):
        left = sum(kind in "PS" for kind, _ in ops)
        got = []
        for kind, v in ops:
            assert r.finished() == (left == 0)
            if kind == "C":
                got.append(r.squeeze_challenge_scalar())
            elif kind == "p":
                r.common_point(v)
            elif kind == "s":
                r.common_scalar(v)
            elif kind == "P":
                assert r.read_point().tolist() == v[:8].tolist()
                left -= 1
            else:
                assert r.read_scalar() == cv.scalar.from_limbs([int(x) for x in v])
                left -= 1
        assert got == challenges and r.finished()
    r = transcript.Blake2bRead(curve, proof)
    assert r.remaining() == len(proof)
    with pytest.raises(transcript.TranscriptError):
        transcript.Blake2bRead(curve, proof[:0]).read_point()


# ---- 4. the refusals -----------------------------------------------------------------------------------------------------------------
def _reader(curve, data: bytes):
    h = api._vp()
    assert api.lib().trh_tr_create_reader(api.CURVE_ID[curve], data, len(data), ctypes.byref(h)) == 0
    return h


def _writer(curve):
    h = api._vp()
    assert api.lib().trh_tr_create_writer(api.CURVE_ID[curve], ctypes.byref(h)) == 0
    return h


def _message(h) -> str:
    buf = ctypes.create_string_buffer(200)
    assert api.lib().trh_tr_message(h, buf, len(buf)) == 0
    return buf.value.decode()


def _latched(h, word, reader=True):
    """the handle holds an error whose text has `word`; every further operation returns it, leaves its output zero and changes nothing"""
    lib = api.lib()
    assert lib.trh_tr_status(h) == EINVAL and word in _message(h) and word.encode() in lib.trh_last_error()
    n0 = ctypes.c_size_t(0)
    assert lib.trh_tr_bytes_len(h, ctypes.byref(n0)) == 0
    left0 = ctypes.c_size_t(0)
    if reader:
        assert lib.trh_tr_remaining(h, ctypes.byref(left0)) == 0
    cv = o.PALLAS
    ones = lambda k: np.full(k, 0xffffffffffffffff, dtype=np.uint64)  # noqa: E731
    for fn, out in ((lib.trh_tr_squeeze_challenge_scalar, ones(4)), (lib.trh_tr_read_scalar, ones(4)), (lib.trh_tr_read_point, ones(8))):
        assert fn(h, api._p(out)) == EINVAL and not out.any(), fn.__name__
    assert lib.trh_tr_write_scalar(h, api._p(_scalar(cv, 5))) == EINVAL and lib.trh_tr_common_scalar(h, api._p(_scalar(cv, 5))) == EINVAL
    assert lib.trh_tr_write_point(h, api._p(_jacobian(cv, cv.generator))) == EINVAL and lib.trh_tr_common_point(h, api._p(_jacobian(cv, cv.generator))) == EINVAL
    n1, left1 = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.trh_tr_bytes_len(h, ctypes.byref(n1)) == 0 and n1.value == n0.value
    if reader:
        assert lib.trh_tr_remaining(h, ctypes.byref(left1)) == 0 and left1.value == left0.value
    assert lib.trh_tr_status(h) == EINVAL and word in _message(h), "the FIRST error is kept"
    lib.trh_tr_destroy(h)


def _off_curve_x(cv):
    return next(x for x in range(1, 50) if cv.lift_x(x) is None)


@pytest.mark.parametrize("curve", CURVES)
def test_refusals_latch(curve):
    lib = api.lib()
    cv = o.CURVES[curve]
    good_point = tm.compress(cv, cv.mul(5, cv.generator))
    out8, out4 = np.zeros(8, np.uint64), np.zeros(4, np.uint64)
    # the proof ends: 31 bytes and 0 bytes where a point is due (after one good item, and at once), and where a scalar is due
    for data, first_ok in ((good_point + good_point[:31], True), (good_point, True), (good_point[:31], False), (b"", False)):
        h = _reader(curve, data)
        if first_ok:
            assert lib.trh_tr_read_point(h, api._p(out8)) == 0 and lib.trh_tr_status(h) == 0 and _message(h) == ""
        assert lib.trh_tr_read_point(h, api._p(out8)) == EINVAL and not out8.any()
        _latched(h, "fewer than 32 bytes")
    h = _reader(curve, bytes(31))
    assert lib.trh_tr_read_scalar(h, api._p(out4)) == EINVAL
    _latched(h, "fewer than 32 bytes")
    # scalars that are no scalars; the largest one that is
    m = cv.scalar.m
    for v in (m, 2 ** 256 - 1, m + 1):
        h = _reader(curve, v.to_bytes(32, "little") + bytes(32))
        out4[:] = 7
        assert lib.trh_tr_read_scalar(h, api._p(out4)) == EINVAL and not out4.any()
        _latched(h, "not below the modulus")
    r = transcript.Blake2bRead(curve, (m - 1).to_bytes(32, "little"))
    assert r.read_scalar() == m - 1 and r.finished()
    # points that are no points: x off the curve, x >= p (p + a good x: nothing reduces it), the identity
    x_bad, p = _off_curve_x(cv), cv.base.m
    x_good = cv.mul(5, cv.generator)[0]
    assert x_good + p < 2 ** 255
    for enc, word in ((x_bad.to_bytes(32, "little"), "not the encoding"), ((x_bad | 1 << 255).to_bytes(32, "little"), "not the encoding"),
                      (p.to_bytes(32, "little"), "not the encoding"), ((p + x_good).to_bytes(32, "little"), "not the encoding"),
                      (bytes(32), "infinity")):
        h = _reader(curve, enc + good_point)
        out8[:] = 7
        assert lib.trh_tr_read_point(h, api._p(out8)) == EINVAL and not out8.any()
        with pytest.raises(tm.TranscriptError):
            tm.Reader(curve, enc).read_point()
        _latched(h, word)
    # the identity on write, as Jacobian Z = 0 with any X, Y and as the all-zero affine POD
    for limbs in (np.zeros(12, np.uint64), np.concatenate([_jacobian(cv, cv.generator)[:8], np.zeros(4, np.uint64)])):
        for fn in (lib.trh_tr_write_point, lib.trh_tr_common_point):
            h = _writer(curve)
            assert lib.trh_tr_write_scalar(h, api._p(_scalar(cv, 9))) == 0
            assert fn(h, api._p(limbs)) == EINVAL
            _latched(h, "infinity", reader=False)
    w = transcript.Blake2bWrite(curve)
    with pytest.raises(transcript.TranscriptError, match="infinity"):
        w.write_point(np.zeros(8, np.uint64))
    with pytest.raises(transcript.TranscriptError, match="infinity"):
        w.write_scalar(_scalar(cv, 1))  # latched
    assert w.finalize() == b""
    # a reader does not write, a writer does not read
    h = _reader(curve, good_point)
    assert lib.trh_tr_write_scalar(h, api._p(_scalar(cv, 9))) == EINVAL
    _latched(h, "on a reader")
    h = _writer(curve)
    assert lib.trh_tr_read_point(h, api._p(out8)) == EINVAL
    _latched(h, "on a writer", reader=False)


def test_unknown_curve_ids_and_null_pointers():
    lib = api.lib()
    h = api._vp()
    for bad in (2, -1, 7):
        assert lib.trh_tr_create_writer(bad, ctypes.byref(h)) == EINVAL and b"unknown curve id" in lib.trh_last_error() and not h
        assert lib.trh_tr_create_reader(bad, b"", 0, ctypes.byref(h)) == EINVAL and b"unknown curve id" in lib.trh_last_error() and not h
    assert lib.trh_tr_create_writer(0, None) == EINVAL and b"null" in lib.trh_last_error()
    assert lib.trh_tr_create_reader(0, None, 32, ctypes.byref(h)) == EINVAL and b"null" in lib.trh_last_error()
    assert lib.trh_tr_create_reader(1, None, 0, ctypes.byref(h)) == 0, "an empty proof needs no pointer"
    n = ctypes.c_size_t(9)
    assert lib.trh_tr_remaining(h, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.trh_tr_read_point(h, None) == EINVAL and lib.trh_tr_status(h) == 0, "a null pointer is the caller's mistake, not the proof's"
    assert lib.trh_tr_squeeze_challenge_scalar(None, api._p(np.zeros(4, np.uint64))) == EINVAL
    assert lib.trh_tr_callbacks(h, ctypes.byref(api.Transcript())) == EINVAL and b"reader" in lib.trh_last_error()
    lib.trh_tr_destroy(h)
    lib.trh_tr_destroy(None)
    w = _writer("pallas")
    assert lib.trh_tr_remaining(w, ctypes.byref(n)) == EINVAL
    assert lib.trh_tr_write_scalar(w, api._p(_scalar(o.PALLAS, 3))) == 0
    small = ctypes.create_string_buffer(31)
    assert lib.trh_tr_bytes(w, small, 31) == EINVAL and lib.trh_tr_status(w) == 0
    lib.trh_tr_destroy(w)


# ---- 5. the callbacks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_callbacks_give_the_bytes_of_the_direct_entries(curve):
    m = o.CURVES[curve].scalar.m
    ops = script(curve)
    direct = transcript.Blake2bWrite(curve)
    want = play(direct, ops)
    w = transcript.Blake2bWrite(curve)
    tr = w.callbacks()
    assert tr.ctx == w.handle.value
    got = []
    for kind, v in ops:
        if kind == "C":
            out = np.zeros(4, dtype=np.uint64)
            tr.squeeze_challenge_scalar(tr.ctx, api._p(out))
            got.append(transcript._canon(out, m))
        elif kind == "P":
            tr.write_point(tr.ctx, api._p(v))
        elif kind == "S":
            tr.write_scalar(tr.ctx, api._p(v))
        else:
            {"p": w.common_point, "s": w.common_scalar}[kind](v)
    assert got == want and w.finalize() == direct.finalize()
    w.raise_if_failed()
    # a callback cannot fail where it stands: the identity latches, the squeeze after it writes zero, raise_if_failed reports it
    tr.write_point(tr.ctx, api._p(np.zeros(12, np.uint64)))
    out = np.full(4, 3, dtype=np.uint64)
    tr.squeeze_challenge_scalar(tr.ctx, api._p(out))
    assert not out.any() and w.finalize() == direct.finalize()
    with pytest.raises(transcript.TranscriptError, match="infinity"):
        w.raise_if_failed()


# ---- 6. trh.hpp ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_trh_hpp_in_the_stand_alone_program(exe, tmp_path, curve):
    ops = script(curve)
    src, dst = tmp_path / "script.in", tmp_path / "script.out"
    src.write_bytes(b"".join(kind.encode() + (b"" if v is None else v.tobytes()) for kind, v in ops))
    assert f"{len(ops)} operations, 64 challenges" in _run(exe, ["script", curve, str(src), str(dst)])
    model = tm.Writer(curve)
    want = play(model, ops)
    got = dst.read_bytes()
    f = o.CURVES[curve].scalar
    assert [f.from_limbs(list(struct.unpack("<4Q", got[32 * i:32 * i + 32]))) for i in range(len(want))] == want
    assert got[32 * len(want):] == model.finalize()
