"""No device: csrc/witness.h on the host and the host side of the packed witness intake.

  witness_vec_test   the header's functions in a stand-alone program under address + undefined sanitizers (tests/native/witness_vec_test.cpp,
                     built by program() below as `make` builds it; it never loads libtrh), its lines against Python integers and oracle/pasta.py's limbs
  pack_bits          against an explicit bit loop
  the ABI            the four entries are exported, answer TRH_ENODEV without a device, and keep the stream out of their parameter lists"""
import atexit
import ctypes
import os
import random
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import pasta as o
from tiny_ram_halo2_amd import api, witness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = [""]  # program()
ENTRIES = ["trh_columns_from_ints_dev", "trh_columns_from_ints_host", "trh_even_odd_split_dev", "trh_even_bits_table_dev"]
M64 = (1 << 64) - 1
EVEN = int("01" * 32, 2)


def program():
    """the stand-alone program, compiled here once per run with the Makefile's command line into a directory of its own (as test_foldplan.py
    and test_hashtocurve_host.py do): the tests without a device then need no build product under tests/"""
    if not os.path.exists(PROGRAM[0]):
        tmp = tempfile.mkdtemp(prefix="witness_vec_test_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        PROGRAM[0] = os.path.join(tmp, "witness_vec_test")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(ROOT, "tests", "native", "witness_vec_test.cpp"), "-o", PROGRAM[0]])
    return PROGRAM[0]


def run(lines):
    p = subprocess.run([program()], input="".join(line + "\n" for line in lines), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]   # a sanitizer report ends the program with a non-zero status
    out = p.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return [[int(w, 16) for w in line.split()] for line in out]


@pytest.mark.parametrize("field", ["fp", "fq"])
def test_fe_from_u64(field):
    f, rng = o.FIELDS[field], random.Random(0x64 + api.FIELD_ID[field])
    values = [0, 1, (1 << 32) - 1, 1 << 63, M64] + [rng.getrandbits(64) for _ in range(200)]
    got = run([f"u {api.FIELD_ID[field]} {v}" for v in values])
    assert got == [list(f.limbs(v)) for v in values]


@pytest.mark.parametrize("field", ["fp", "fq"])
def test_fe_from_i64(field):
    f, rng = o.FIELDS[field], random.Random(0x164 + api.FIELD_ID[field])
    values = [0, -1, 1 << 31, -(1 << 31), (1 << 63) - 1, -(1 << 63)] + [rng.getrandbits(64) - (1 << 63) for _ in range(200)]
    got = run([f"i {api.FIELD_ID[field]} {v}" for v in values])
    assert got == [list(f.limbs(v % f.m)) for v in values]
    assert got[1] == list(f.limbs(f.m - 1)) and got[5] == list(f.limbs(f.m - (1 << 63)))


def test_even_and_odd_parts():
    rng = random.Random(0xE0)
    words = [0, M64, int("10" * 32, 2), EVEN] + [rng.getrandbits(64) for _ in range(200)]
    for w, (even, odd) in zip(words, run([f"e {w}" for w in words])):
        assert even == sum(((w >> b) & 1) << b for b in range(0, 64, 2))
        assert odd == sum(((w >> (b + 1)) & 1) << b for b in range(0, 64, 2))
        assert even & ~EVEN == 0 and odd & ~EVEN == 0 and even + 2 * odd == w


def test_spread_bits():
    values = list(range(256)) + [(1 << 32) - 1]
    got = run([f"s {v}" for v in values])
    assert got == [[sum(((v >> j) & 1) << (2 * j) for j in range(32))] for v in values]
    assert got[-1] == [EVEN]


@pytest.mark.parametrize("live", [1, 31, 32, 33, 1000])
def test_pack_bits(live):
    flags = np.random.default_rng(live).integers(0, 2, size=(3, live)).astype(bool)
    flags[1, -1] = True
    packed = witness.pack_bits(flags)
    assert packed.dtype == np.uint32 and packed.shape == (3, (live + 31) // 32)
    for c in range(3):
        want = [0] * ((live + 31) // 32)
        for r in range(live):
            if flags[c, r]:
                want[r >> 5] |= 1 << (r & 31)
        assert [int(w) for w in packed[c]] == want
    one = witness.pack_bits(flags[2])
    assert one.shape == ((live + 31) // 32,) and (one == packed[2]).all()


def test_the_entries_are_exported_and_bound():
    lib = api.lib()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in api.EXPORTED_SYMBOLS


def _has_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_no_device_is_enodev():
    lib = api.lib()
    src = np.arange(8, dtype=np.uint32)
    a = api.IntsArgs(kind=witness.U32, src=src.ctypes.data, src_stride=8, n_cols=1, live_rows=8, dst=0x1000, dst_odd=0x2000, n=8, stream=None)
    for name in ENTRIES[:3]:
        assert getattr(lib, name)(api.FP, ctypes.byref(a)) == -2 and b"trh_init" in lib.trh_last_error(), name
    t = api.EvenBitsTableArgs(word_bits=8, dst=0x1000, n=16, stream=None)
    assert lib.trh_even_bits_table_dev(api.FQ, ctypes.byref(t)) == -2 and b"trh_init" in lib.trh_last_error()
    # a bad argument is still a bad argument without a device
    a.kind = 99
    assert lib.trh_columns_from_ints_dev(api.FP, ctypes.byref(a)) == -1 and b"kind" in lib.trh_last_error()


def test_no_new_declaration_takes_a_stream_parameter():
    """tests/test_gpu_streams.py's table lists every declaration with a `void* stream` parameter; these keep theirs in the args struct"""
    header = open(os.path.join(ROOT, "include", "trh.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    decl = dict(re.findall(r"\b(trh_\w+)\s*\(([^;{}]*?)\)\s*;", header))
    for name in ENTRIES:
        assert name in decl and "stream" not in decl[name], (name, decl.get(name))
