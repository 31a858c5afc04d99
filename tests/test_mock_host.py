"""CPU tests of the MockProver layer (tiny_ram_halo2_amd/mock.py, trh_expr_check_dev, trh_lookup_check_dev): what needs no device.

  * decode_failures / bitmap_rows: bitmaps -> failure records, their order and the max_failures cap (a pure function of host arrays);
  * csrc/tuplehash.h, the set behind the lookup check, built sequentially by tests/native/tuplehash_test.cpp (compiled here, address + undefined sanitizers)
    over the inputs of tests/mock_cases.py -- the inputs tests/test_gpu_mock.py gives the device -- against a Python set of tuples, and the
    slots it visits against the probe cap;
  * without a device both entries fail loudly."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import mock_cases as mc
from tiny_ram_halo2_amd import api, expr, mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 2, 5, 16)


@pytest.fixture(scope="module")
def tuplehash_test(tmp_path_factory):
    """tests/native/tuplehash_test.cpp compiled once, with the Makefile's flags, outside the tree: the test then needs nothing that a build
    left under tests/"""
    exe = str(tmp_path_factory.mktemp("tuplehash") / "tuplehash_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "tuplehash_test.cpp"), "-o", exe])
    return exe


def _words(n_words, rows):
    w = np.zeros(n_words, dtype=np.uint64)
    for r in rows:
        w[r // 64] |= np.uint64(1) << np.uint64(r % 64)
    return w


def test_bitmap_rows_reads_bit_r_of_word_r_div_64():
    rows = [0, 1, 63, 64, 65, 127, 128, 500]
    assert mock.bitmap_rows(_words(8, rows)) == rows
    assert mock.bitmap_rows(_words(8, rows), limit=3) == rows[:3]
    assert mock.bitmap_rows(_words(8, rows), limit=0) == []
    assert mock.bitmap_rows(np.zeros(4, np.uint64)) == []
    # device bitmaps arrive as int64 tensors: the sign bit is row 63
    assert mock.bitmap_rows(_words(2, [63, 64]).view(np.int64)) == [63, 64]
    assert mock.bitmap_rows(np.array([[1, 0], [0, 2]], np.uint64)[1]) == [65]


def test_decode_failures_orders_by_gate_poly_row_then_lookup_row():
    polys = [(0, 0, "decompose"), (1, 0, "l_add"), (1, 1, "l_add"), (2, 0, "xor")]
    gate_bitmaps = [None, _words(8, [400, 7]), _words(8, [3]), _words(8, [7, 64])]
    lookups = ["even", "odd"]
    lookup_bitmaps = [_words(8, [9, 2]), None]
    got = mock.decode_failures(polys, gate_bitmaps, lookups, lookup_bitmaps)
    C, L = mock.ConstraintNotSatisfied, mock.Lookup
    assert got == [C(1, 0, "l_add", 7), C(1, 0, "l_add", 400), C(1, 1, "l_add", 3), C(2, 0, "xor", 7), C(2, 0, "xor", 64), L(0, "even", 2), L(0, "even", 9)]
    # outputs given out of order are still reported by (gate, poly)
    shuffled = mock.decode_failures(polys[::-1], gate_bitmaps[::-1], lookups, lookup_bitmaps)
    assert shuffled == got
    assert mock.decode_failures(polys, [None] * 4, lookups, [None, None]) == []


def test_decode_failures_stops_at_max_failures():
    polys = [(0, 0, "g0"), (0, 1, "g0")]
    every = _words(8, range(512))
    got = mock.decode_failures(polys, [every, every], ["l"], [every], max_failures=600)
    assert len(got) == 600
    assert got[:512] == [mock.ConstraintNotSatisfied(0, 0, "g0", r) for r in range(512)]
    assert got[512:] == [mock.ConstraintNotSatisfied(0, 1, "g0", r) for r in range(88)]
    got = mock.decode_failures(polys, [None, _words(8, [5])], ["l"], [every], max_failures=3)
    assert got == [mock.ConstraintNotSatisfied(0, 1, "g0", 5), mock.Lookup(0, "l", 0), mock.Lookup(0, "l", 1)]
    assert len(mock.decode_failures(polys, [every, every], ["l"], [every])) == 64      # the default
    assert mock.decode_failures(polys, [every, every], ["l"], [every], max_failures=0) == []


def _write_case(path, inputs, tables, usable):
    width, rows = inputs.shape[0], inputs.shape[1]
    with open(path, "wb") as fh:
        fh.write(np.array([width, usable, rows], dtype="<u8").tobytes())
        fh.write(np.ascontiguousarray(inputs, dtype="<u8").tobytes())
        fh.write(np.ascontiguousarray(tables, dtype="<u8").tobytes())


@pytest.mark.parametrize("width", WIDTHS)
def test_tuple_set_on_the_host_matches_a_python_set_and_the_probe_cap(width, tmp_path, tuplehash_test):
    """every case of mock_cases through the header's own insert / probe code: the verdict equals the Python model's, the program's own
    std::set agrees row by row, the probe total is within the cap, and the sanitizers stay quiet"""
    cases, files = [], []
    for kind in mc.TABLES:
        for usable in mc.sizes(kind):
            for bad in (False, True):
                inputs, tables = mc.lookup_case(kind, width, usable, bad)
                path = str(tmp_path / f"{kind}_{usable}_{int(bad)}.bin")
                _write_case(path, inputs, tables, usable)
                cases.append((kind, usable, bad, inputs, tables))
                files.append(path)
    r = subprocess.run([tuplehash_test] + files, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(lines) == len(cases)
    for (kind, usable, bad, inputs, tables), got in zip(cases, lines):
        n_bad, first, words = mc.lookup_model(inputs, tables, usable)
        what = (kind, width, usable, bad)
        assert (n_bad > 0) == bad, what                      # the planted misses are misses, and nothing else is
        assert (got["width"], got["usable_rows"]) == (width, usable), what
        assert (got["n_bad"], got["first_bad_row"], got["bitmap"]) == (n_bad, first, mc.bitmap_hex(words)), what
        assert got["set_mismatches"] == 0 and got["within_cap"] is True, what
        assert 2 * usable <= got["probes"] <= mc.PROBE_CAP * (usable + usable), (what, got["probes"])
        if kind == "same" and not bad:                       # the duplicates are dropped at the first slot: no chain
            assert got["probes"] == 2 * usable, what


def test_planted_misses_are_where_the_cases_say():
    inputs, tables = mc.lookup_case("range", 2, (1 << 10) - 6, True)
    n_bad, first, words = mc.lookup_model(inputs, tables, (1 << 10) - 6)
    assert mock.bitmap_rows(words) == [0, 20, 30, 40, (1 << 10) - 7] and (n_bad, first) == (5, 0)
    inputs, tables = mc.lookup_case("topword", 5, 65, True)
    assert mock.bitmap_rows(mc.lookup_model(inputs, tables, 65)[2]) == [0, 20, 64]
    inputs, tables = mc.lookup_case("same", 1, 1, True)
    assert mc.lookup_model(inputs, tables, 1)[:2] == (1, 0)


def _has_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_no_device_mock_entries_fail_loudly():
    """trh_expr_check_dev and trh_lookup_check_dev return TRH_ENODEV without a device, never a host-side answer"""
    lib = api.lib()
    col = np.zeros((64, 4), np.uint64)
    ptrs = (ctypes.c_void_p * 1)(col.ctypes.data)
    n_bad, first = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
    assert lib.trh_lookup_check_dev(api.FP, ptrs, ptrs, 1, 64, api._p(n_bad), api._p(first), None) == -2 and b"trh_init" in lib.trh_last_error()
    assert lib.trh_expr_check_dev(None, ptrs, 6, 58, api._p(n_bad), api._p(first), None) == -2 and b"trh_init" in lib.trh_last_error()
    with pytest.raises(api.TrhError):
        mock.MockProver("fp", 6, 58, gates=[("g", [expr.Advice(0)])])
