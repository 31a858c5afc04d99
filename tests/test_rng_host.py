"""CPU tests of the random-scalar stream (csrc/chacha.h, trh_rng_*), no GPU.
1. tests/chacha_model.py itself: RFC 8439's block vector reached through the 64 + 64 layout, the all-zero key's first block, that block as an
   element of both fields; the numpy form against the integer form where the counter's words carry.
2. chacha20_block and fe_from_u512 through the header's plain C++ branch in a stand-alone program (tests/native/chacha_vec_test.cpp) under
   -fsanitize=undefined; expected values from Python integers.  The wide-reduction records sit on the bounds the header's comment argues about:
   halves at m - 1, m, m + 1, 2 m, 3 m, 4 m - 1 and 2^256 - 1.
3. The handle through ctypes on a machine without a device, as trh_point_sum is tested: host draws, seek / position, the carry at 2^32, the
   refusal at 2^64, unknown field ids, null pointers.  tests/test_gpu_rng.py sends the same stream through the kernels."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import chacha_model as cm
import pasta as o
from tiny_ram_halo2_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["fp", "fq"]
EINVAL = -1

ZERO_KEY = bytes(32)
RFC_KEY = bytes(range(32))
RFC_COUNTER, RFC_STREAM = 0x0900000000000001, 0x000000004A000000
RFC_BLOCK = bytes.fromhex("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4ed2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")
ZERO_BLOCK_ELEMENT = {"fp": 0x2b45caa7e07be72fb67eb69f215da19792122d771b3d76ef21ead535b0f3aa24,
                      "fq": 0x277972c30ca37a9357e354c2137f8b62400275bfc2bc60d568e095af17d98b83}
SEED = bytes((0x3c + 11 * i) & 0xff for i in range(32))
STREAM = 0xfedcba9876543210


# ---- 1. the model ---------------------------------------------------------------------------------------------------------------------
def test_model_block_vectors():
    z = cm.block(ZERO_KEY, 0, 0)
    assert z[:16].hex() == "76b8e0ada0f13d90405d6ae55386bd28" and z[-8:].hex() == "c387b669b2ee6586"
    assert cm.block(RFC_KEY, RFC_COUNTER, RFC_STREAM) == RFC_BLOCK


@pytest.mark.parametrize("field", FIELDS)
def test_model_first_element_of_the_zero_key(field):
    assert cm.element(field, ZERO_KEY, 0) == ZERO_BLOCK_ELEMENT[field]
    assert cm.from_u512(field, cm.block(ZERO_KEY, 0, 0)) == ZERO_BLOCK_ELEMENT[field]


def test_model_vectorised_form_equals_the_scalar_form():
    counters = list(range(0, 5)) + list(range((1 << 32) - 3, (1 << 32) + 3)) + [(1 << 64) - 2, (1 << 64) - 1, RFC_COUNTER]
    for seed, stream in ((SEED, STREAM), (RFC_KEY, RFC_STREAM), (ZERO_KEY, 0)):
        got = cm.blocks(seed, counters, stream)
        assert got.dtype == np.uint32 and got.shape == (len(counters), 16)
        for row, c in zip(got, counters):
            assert row.astype("<u4").tobytes() == cm.block(seed, c, stream), hex(c)
    assert cm.blocks(RFC_KEY, [RFC_COUNTER], RFC_STREAM)[0].astype("<u4").tobytes() == RFC_BLOCK
    f = o.FIELDS["fp"]
    limbs = cm.elements_limbs("fp", SEED, (1 << 32) - 2, 4, STREAM)
    assert [f.from_limbs(r) for r in limbs] == [cm.element("fp", SEED, (1 << 32) - 2 + i, STREAM) for i in range(4)]


# ---- 2. csrc/chacha.h, host branch, under the sanitizer ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vec_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chacha") / "chacha_vec_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "chacha_vec_test.cpp"), "-o", exe])
    return exe


def _run(exe, mode, src, dst, records):
    r = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=120, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and f"{records} records ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_chacha20_block_host_branch(vec_exe, tmp_path):
    cases = [(ZERO_KEY, 0, 0), (RFC_KEY, RFC_COUNTER, RFC_STREAM)]
    for c in ((1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 64) - 2, (1 << 64) - 1):
        cases.append((SEED, c, STREAM))
        cases.append((SEED, c, 0))
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "blocks.bin")
    with open(src, "wb") as fh:
        for key, counter, stream in cases:
            fh.write(key + counter.to_bytes(8, "little") + stream.to_bytes(8, "little"))
    _run(vec_exe, "block", src, dst, len(cases))
    got = open(dst, "rb").read()
    assert len(got) == 64 * len(cases)
    assert got[:16].hex() == "76b8e0ada0f13d90405d6ae55386bd28" and got[56:64].hex() == "c387b669b2ee6586" and got[64:128] == RFC_BLOCK
    for i, (key, counter, stream) in enumerate(cases):
        assert got[64 * i:64 * i + 64] == cm.block(key, counter, stream), (i, hex(counter))


def wide_records(field):
    """(tag, 512-bit value): the halves on the bounds of fe_from_u512's conditional-subtract chain, then random values.  4 m - 1 = 2^256 + 4 t - 1
    does not fit a 256-bit half (m = 2^254 + t): as a `lo` record it is that integer (its top bit lands in the high half); as a `hi` record it
    would pass 2^512, so that record takes the largest half there is, 2^256 - 1, which lies in [3 m, 4 m)"""
    m = o.FIELDS[field].m
    top = (1 << 256) - 1
    assert 3 * m < top < 4 * m - 1  # why the chain has three rounds, and why 4 m - 1 is no half
    edge = [("m-1", m - 1), ("m", m), ("m+1", m + 1), ("2m", 2 * m), ("3m", 3 * m), ("4m-1", 4 * m - 1), ("2^256-1", top)]
    recs = [("0", 0), ("both-max", top | top << 256)]
    recs += [("lo=" + t, v) for t, v in edge] + [("hi=" + t, min(v, top) << 256) for t, v in edge]
    rng = random.Random(0xC4AC4A + len(field) + (field == "fq"))
    recs += [(f"random-{i}", rng.getrandbits(512)) for i in range(256)]
    assert all(0 <= v < 1 << 512 for _, v in recs)
    return recs


def test_wide_records_are_the_ones_asked_for():
    for field in FIELDS:
        m = o.FIELDS[field].m
        recs = dict(wide_records(field))
        assert recs["lo=4m-1"] == 4 * m - 1 and recs["lo=4m-1"] >> 256 == 1 and recs["hi=4m-1"] == recs["hi=2^256-1"] == ((1 << 256) - 1) << 256
        assert recs["lo=2^256-1"] == (1 << 256) - 1 and recs["hi=3m"] == (3 * m) << 256 and recs["both-max"] == (1 << 512) - 1
        assert sum(1 for t in recs if t.startswith("random-")) == 256 and len(recs) == 2 + 14 + 256


@pytest.mark.parametrize("field", FIELDS)
def test_fe_from_u512_host_branch(vec_exe, tmp_path, field):
    f = o.FIELDS[field]
    recs = wide_records(field)
    src, dst = str(tmp_path / "wide.bin"), str(tmp_path / "reduced.bin")
    with open(src, "wb") as fh:
        for _, v in recs:
            fh.write(v.to_bytes(64, "little"))
    _run(vec_exe, field, src, dst, len(recs))
    got = np.fromfile(dst, np.uint64).reshape(-1, 4)
    assert got.shape[0] == len(recs)
    bad = [t for (t, v), row in zip(recs, got) if [int(w) for w in row] != f.limbs(v % f.m)]
    assert not bad, bad[:20]


# ---- 3. the handle, no device ---------------------------------------------------------------------------------------------------------
def _err():
    return api.lib().trh_last_error().decode()


@pytest.mark.parametrize("field", FIELDS)
def test_next_scalar_matches_the_model(field):
    f = o.FIELDS[field]
    rng = api.Rng(SEED, STREAM)
    assert rng.position() == 0
    got = [rng.next_scalar(field) for _ in range(64)]
    assert rng.position() == 64
    want = cm.elements_limbs(field, SEED, 0, 64, STREAM)
    assert (np.stack(got) == want).all()
    assert [f.from_limbs(r) for r in got[:3]] == [cm.element(field, SEED, i, STREAM) for i in range(3)]
    zero = api.Rng(ZERO_KEY)
    assert f.from_limbs(zero.next_scalar(field)) == ZERO_BLOCK_ELEMENT[field]
    assert f.from_limbs(zero.next_scalar(field)) == cm.element(field, ZERO_KEY, 1)
    rng.destroy(); zero.destroy()


def test_the_stream_id_and_the_seed_select_the_stream():
    a, b, c = api.Rng(SEED, 0), api.Rng(SEED, 1), api.Rng(RFC_KEY, RFC_STREAM)
    assert o.FIELDS["fp"].from_limbs(a.next_scalar("fp")) == cm.element("fp", SEED, 0, 0)
    assert o.FIELDS["fp"].from_limbs(b.next_scalar("fp")) == cm.element("fp", SEED, 0, 1)
    c.seek(RFC_COUNTER)
    assert o.FIELDS["fq"].from_limbs(c.next_scalar("fq")) == int.from_bytes(RFC_BLOCK, "little") % o.FIELDS["fq"].m


@pytest.mark.parametrize("field", FIELDS)
def test_seek_position_and_the_carry_at_2_32(field):
    f = o.FIELDS[field]
    rng = api.Rng(SEED, STREAM)
    start = (1 << 32) - 2
    rng.seek(start)
    assert rng.position() == start
    got = [f.from_limbs(rng.next_scalar(field)) for _ in range(4)]
    assert got == [cm.element(field, SEED, start + i, STREAM) for i in range(4)]
    assert rng.position() == (1 << 32) + 2
    rng.seek(5)
    assert f.from_limbs(rng.next_scalar(field)) == cm.element(field, SEED, 5, STREAM) and rng.position() == 6
    # the two fields share the position: one block per draw, whichever field reads it
    other = "fq" if field == "fp" else "fp"
    assert o.FIELDS[other].from_limbs(rng.next_scalar(other)) == cm.element(other, SEED, 6, STREAM) and rng.position() == 7


def test_refusal_at_2_64():
    lib = api.lib()
    f = o.FIELDS["fp"]
    rng = api.Rng(SEED, STREAM)
    last = (1 << 64) - 1
    rng.seek(last)
    assert rng.position() == last
    assert f.from_limbs(rng.next_scalar("fp")) == cm.element("fp", SEED, last, STREAM)  # the last block exists
    out = np.full(4, 7, np.uint64)
    assert lib.trh_rng_next_scalar(rng.handle, api.FP, api._p(out)) == EINVAL and (out == 7).all()  # position 2^64: nothing left
    assert "end of the stream" in _err()
    pos = ctypes.c_uint64(123)
    assert lib.trh_rng_position(rng.handle, ctypes.byref(pos)) == EINVAL and pos.value == 123  # 2^64 is no u64
    assert lib.trh_rng_next_scalar(rng.handle, api.FP, api._p(out)) == EINVAL  # ... and stays there
    rng.seek(last)
    assert rng.position() == last and f.from_limbs(rng.next_scalar("fp")) == cm.element("fp", SEED, last, STREAM)


def test_unknown_field_id_is_refused_and_takes_no_position():
    lib = api.lib()
    rng = api.Rng(SEED, STREAM)
    rng.seek(41)
    out = np.full(4, 7, np.uint64)
    assert lib.trh_rng_next_scalar(rng.handle, 7, api._p(out)) == EINVAL
    assert _err() == "unknown field id 7"
    assert (out == 7).all() and rng.position() == 41
    assert lib.trh_rng_next_scalar(rng.handle, -1, api._p(out)) == EINVAL and rng.position() == 41
    assert lib.trh_rng_next_scalar(rng.handle, 0, api._p(out)) == 0 and rng.position() == 42
    # the device entries check the id before they look for a device
    assert lib.trh_rng_fill_dev(rng.handle, 7, None, 0, None) == EINVAL and _err() == "unknown field id 7"
    assert lib.trh_rng_fill_rows_dev(rng.handle, 7, None, 0, 0, 0, 0, None) == EINVAL and _err() == "unknown field id 7"
    assert rng.position() == 42


def test_null_pointers_and_bad_rows():
    lib = api.lib()
    rng = api.Rng(SEED)
    out = np.zeros(4, np.uint64)
    pos = ctypes.c_uint64(0)
    h = api._vp()
    assert lib.trh_rng_create(None, 0, ctypes.byref(h)) == EINVAL and h.value is None
    assert lib.trh_rng_create(ctypes.c_char_p(SEED), 0, None) == EINVAL
    assert lib.trh_rng_next_scalar(None, 0, api._p(out)) == EINVAL
    assert lib.trh_rng_next_scalar(rng.handle, 0, None) == EINVAL and rng.position() == 0
    assert lib.trh_rng_seek(None, 0) == EINVAL
    assert lib.trh_rng_position(None, ctypes.byref(pos)) == EINVAL and lib.trh_rng_position(rng.handle, None) == EINVAL
    assert lib.trh_rng_fill_dev(None, 0, None, 0, None) == EINVAL
    assert lib.trh_rng_fill_rows_dev(None, 0, None, 0, 0, 0, 0, None) == EINVAL
    assert lib.trh_rng_fill_dev(rng.handle, 0, None, 4, None) == EINVAL                     # n elements into a null buffer
    assert lib.trh_rng_fill_rows_dev(rng.handle, 0, None, 3, 64, 60, 5, None) == EINVAL     # first + count > row_len
    assert "do not fit a row" in _err()
    assert lib.trh_rng_fill_rows_dev(rng.handle, 0, None, 3, 64, 65, 0, None) == EINVAL
    assert rng.position() == 0
    lib.trh_rng_destroy(None)  # a no-op


def test_the_seed_is_not_in_the_error_text():
    """every refusal above formats positions and sizes only: no message holds a key word in hex or decimal"""
    lib = api.lib()
    rng = api.Rng(SEED, STREAM)
    words = cm.key_words(SEED)
    out = np.zeros(4, np.uint64)
    rng.seek((1 << 64) - 1)
    rng.next_scalar("fp")
    msgs = []
    assert lib.trh_rng_next_scalar(rng.handle, 0, api._p(out)) == EINVAL
    msgs.append(_err())
    assert lib.trh_rng_next_scalar(rng.handle, 7, api._p(out)) == EINVAL
    msgs.append(_err())
    assert lib.trh_rng_fill_rows_dev(rng.handle, 0, None, 3, 64, 60, 5, None) == EINVAL
    msgs.append(_err())
    for msg in msgs:
        for w in words:
            assert f"{w:x}" not in msg.lower() and str(w) not in msg
        assert SEED.hex() not in msg.lower()
