"""CPU tests of the permutation keygen assembly (csrc/permkeygen.h, trh_perm_create / copy / copy_batch / mapping), no GPU.
1. The header alone in a stand-alone program (tests/native/permkeygen_test.cpp) under address + undefined sanitizers: every script of
   tests/permkeygen_model.py at k = 1, 3, 6 with 1, 3, 5 columns.  The mapping must equal the Python model's (the recalled upstream algorithm,
   line by line), be a permutation, and -- whatever the recall got wrong -- have exactly the connected components of the copy graph as its
   cycles, computed here by a plain union-find.  Cells outside the columns are refused and leave the state as it was.
2. The same handle through ctypes on a machine without a device, as trh_rng_* is tested: create, copy, copy_batch, mapping, destroy, the
   refusals; trh_perm_sigma_dev / trh_perm_check_dev fail loudly there.  tests/test_gpu_permkeygen.py runs the kernels."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import permkeygen_model as pm
from tiny_ram_halo2_amd import api, permutation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
SHAPES = [(k, c) for k in (1, 3, 6) for c in (1, 3, 5)]
U32 = (1 << 32) - 1


def _bad_copies(n_columns, k):
    """every way a cell can lie outside the columns, on either side of the copy"""
    n = 1 << k
    bad = [(n_columns, 0), (0, n), (n_columns - 1, n), (n_columns, n - 1), (U32, 0), (0, U32), (U32, U32)]
    return [b + (0, n - 1) for b in bad] + [(n_columns - 1, 0) + b for b in bad]


def _cases():
    """(name, n_columns, k, copies): every script on every shape, and every script again with the refused copies spread through it"""
    out = []
    for k, n_columns in SHAPES:
        for name, copies in pm.scripts(n_columns, k).items():
            out.append((name, n_columns, k, copies))
            bad = _bad_copies(n_columns, k)
            mixed = []
            for i, c in enumerate(copies):
                mixed.append(c)
                mixed.append(bad[i % len(bad)])
            out.append((name + "+refused", n_columns, k, mixed + bad))
    return out


@pytest.fixture(scope="module")
def native_results(tmp_path_factory):
    """the native program's (return codes, mapping) for every case, from ONE run"""
    tmp = tmp_path_factory.mktemp("permkeygen")
    exe, fin, fout = (str(tmp / n) for n in ("permkeygen_test", "in.txt", "out.txt"))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "native", "permkeygen_test.cpp"), "-o", exe])
    cases = _cases()
    refused_shapes = [(0, 3), (1, 28), (33, 27), (1 << 31, 2), (U32, 27), (1 << 32, 0), (1, 1 << 32)]
    with open(fin, "w") as fh:
        fh.write(f"{len(cases) + len(refused_shapes)}\n")
        for _, n_columns, k, copies in cases:
            fh.write(f"{n_columns} {k} {len(copies)}\n" + "".join("%d %d %d %d\n" % c for c in copies))
        for n_columns, k in refused_shapes:
            fh.write(f"{n_columns} {k} 1\n0 0 0 0\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and f"permkeygen: ok ({len(cases) + len(refused_shapes)} cases)" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    lines = open(fout).read().split("\n")
    got = {}
    for i, (name, n_columns, k, _) in enumerate(cases):
        got[(name, n_columns, k)] = ([int(v) for v in lines[2 * i].split()], [int(v) for v in lines[2 * i + 1].split()])
    for j, shape in enumerate(refused_shapes):
        i = len(cases) + j
        assert lines[2 * i].split() == [str(EINVAL)] and lines[2 * i + 1] == "", shape  # the shape is refused before anything is allocated
    return got


@pytest.mark.parametrize("k,n_columns", SHAPES)
def test_native_mapping_equals_the_model_and_the_copy_graph(native_results, k, n_columns):
    n, cells = 1 << k, n_columns << k
    seen = set()
    for name, nc, kk, copies in _cases():
        if (nc, kk) != (n_columns, k):
            continue
        seen.add(name)
        codes, mapping = native_results[(name, n_columns, k)]
        model = pm.Assembly(n_columns, k)
        want_codes = [0] + [0 if model.copy(*c) else EINVAL for c in copies]
        assert codes == want_codes, name
        assert mapping == model.mapping, name
        assert sorted(mapping) == list(range(cells)), name                       # a permutation
        assert pm.cycles(mapping) == pm.components(n_columns, k, copies), name   # ... whose cycles are the components of the copy graph
        if name.endswith("+refused"):  # the refused copies changed nothing: the same mapping as the script's valid copies alone
            alone = pm.Assembly(n_columns, k)
            for c in copies:
                if c[0] < n_columns and c[2] < n_columns and c[1] < n and c[3] < n:
                    assert alone.copy(*c)
            assert mapping == alone.mapping and EINVAL in codes, name
        # each script reaches the branch it is named for
        base = name.split("+")[0]
        if base in ("none", "self"):
            assert mapping == list(range(cells)) and model.merges == 0, name
        if base in ("twice", "both_orders"):
            assert model.merges == 1 and len([c for c in pm.cycles(mapping) if len(c) > 1]) == 1, name
        if base == "equal_merge":
            assert model.ties >= 1 and model.swaps == 0, name
        if base == "small_left_into_large_right" and cells >= 3:
            assert model.swaps == 1, name
        if base == "full_cycle":
            assert len(pm.cycles(mapping)) == 1, name
        if base == "chain":
            assert max(len(c) for c in pm.cycles(mapping)) == min(cells, 12), name
    assert len(seen) == 18


def test_the_model_on_a_case_worked_by_hand():
    """two columns of two rows: cells 0 1 | 2 3.  copy(0,0 -> 1,0) swaps mapping[0] and mapping[2]; copy(0,1 -> 1,1) likewise for 1 and 3;
    copy(1,0 -> 1,1) joins the two pairs (a tie: the left representative 0 stays) and swaps mapping[2] and mapping[3]"""
    a = pm.Assembly(2, 1)
    assert a.copy(0, 0, 1, 0) and a.mapping == [2, 1, 0, 3] and a.aux == [0, 1, 0, 3] and a.sizes[0] == 2
    assert a.copy(0, 1, 1, 1) and a.mapping == [2, 3, 0, 1]
    assert a.copy(1, 0, 1, 1) and a.mapping == [2, 3, 1, 0] and a.aux == [0, 0, 0, 0] and a.sizes[0] == 4 and a.ties == 3
    assert a.copy(1, 1, 0, 0) and a.mapping == [2, 3, 1, 0]  # one cycle already
    assert not a.copy(2, 0, 0, 0) and not a.copy(0, 2, 0, 0) and a.mapping == [2, 3, 1, 0]
    assert pm.cycles(a.mapping) == {frozenset(range(4))}


# ---- 2. the handle, no device ---------------------------------------------------------------------------------------------------------
def _err():
    return api.lib().trh_last_error().decode()


@pytest.mark.parametrize("k,n_columns", SHAPES)
def test_handle_mapping_equals_the_model(k, n_columns):
    for name, copies in pm.scripts(n_columns, k).items():
        model = pm.Assembly(n_columns, k)
        for c in copies:
            assert model.copy(*c)
        one_by_one, batched = permutation.Assembly("fp", k, n_columns), permutation.Assembly("fq", k, n_columns)
        for c in copies:
            one_by_one.copy(*c)
        batched.copy_many(np.array(copies, dtype=np.int64).reshape(-1, 4))
        want = np.array(model.mapping, dtype=np.uint32).reshape(n_columns, 1 << k)
        assert (one_by_one.mapping() == want).all() and (batched.mapping() == want).all(), name
        if n_columns >= 3:
            assert (batched.mapping(1, 2) == want[1:3]).all() and batched.mapping(n_columns, 0).shape == (0, 1 << k)
        one_by_one.destroy(); batched.destroy()


def test_refused_copies_leave_the_state_unchanged():
    lib = api.lib()
    k, n_columns = 3, 3
    a = permutation.Assembly("fp", k, n_columns)
    copies = pm.scripts(n_columns, k)["random"][:50]
    a.copy_many(copies)
    before = a.mapping().copy()
    for bad in _bad_copies(n_columns, k):
        assert lib.trh_perm_copy(a.handle, *bad) == EINVAL and "outside 3 columns of 8 rows" in _err(), bad
        with pytest.raises(api.TrhError):
            a.copy(*bad)
    assert (a.mapping() == before).all()
    # a batch stops at the first refused copy, names it, and keeps the copies before it
    batch = np.array([(0, 0, 2, 7), (1, 1, 1, 2), (0, 0, 3, 0), (2, 2, 2, 3)], dtype=np.uint32)
    assert lib.trh_perm_copy_batch(a.handle, batch.ctypes.data_as(api._vp), 4) == EINVAL and "copy 2:" in _err()
    model = pm.Assembly(n_columns, k)
    for c in copies + [(0, 0, 2, 7), (1, 1, 1, 2)]:
        assert model.copy(*c)
    assert (a.mapping().reshape(-1) == np.array(model.mapping, dtype=np.uint32)).all()
    with pytest.raises(api.TrhError):
        a.copy_many([(0, 0, 0, -1)])
    with pytest.raises(api.TrhError):
        a.copy(0, 0, 0, 1 << 32)


def test_shapes_and_null_pointers_are_refused():
    lib = api.lib()
    h = api._vp()
    for n_columns, k in ((0, 3), (1, 28), (33, 27), (1 << 31, 2), (U32, 27)):
        assert lib.trh_perm_create(n_columns, k, ctypes.byref(h)) == EINVAL and h.value is None, (n_columns, k)
        assert "2^32" in _err()
    assert lib.trh_perm_create(1, 1, None) == EINVAL
    a = permutation.Assembly("fp", 2, 2)
    out = np.zeros(8, np.uint32)
    assert lib.trh_perm_copy(None, 0, 0, 0, 0) == EINVAL
    assert lib.trh_perm_copy_batch(None, out.ctypes.data_as(api._vp), 1) == EINVAL and lib.trh_perm_copy_batch(a.handle, None, 1) == EINVAL
    assert lib.trh_perm_copy_batch(a.handle, None, 0) == 0
    assert lib.trh_perm_mapping(None, 0, 1, out.ctypes.data_as(api._vp)) == EINVAL and lib.trh_perm_mapping(a.handle, 0, 2, None) == EINVAL
    assert lib.trh_perm_mapping(a.handle, 1, 2, out.ctypes.data_as(api._vp)) == EINVAL and lib.trh_perm_mapping(a.handle, 3, 0, out.ctypes.data_as(api._vp)) == EINVAL
    assert lib.trh_perm_mapping(a.handle, U32, 2, out.ctypes.data_as(api._vp)) == EINVAL and (out == 0).all()  # first + count wraps a u32
    assert lib.trh_perm_sigma_dev(None, 0, 0, 1, None, None) == EINVAL
    n_bad = ctypes.c_uint64(7)
    assert lib.trh_perm_check_dev(None, 0, None, ctypes.byref(n_bad), ctypes.byref(n_bad), None) == EINVAL and n_bad.value == 7
    lib.trh_perm_destroy(None)  # a no-op
    a.destroy()
    a.destroy()


def _has_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_device_entries_fail_loudly_without_a_device():
    lib = api.lib()
    a = permutation.Assembly("fp", 3, 2)
    a.copy(0, 1, 1, 2)
    fake = ctypes.c_void_p(4096)
    assert lib.trh_perm_sigma_dev(a.handle, api.FP, 0, 2, fake, None) == -2 and "trh_init" in _err()
    ptrs = (api._vp * 2)(4096, 8192)
    n_bad, first = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert lib.trh_perm_check_dev(a.handle, api.FP, ptrs, ctypes.byref(n_bad), ctypes.byref(first), None) == -2 and "trh_init" in _err()
    assert n_bad.value == 7 and first.value == 7
    assert a.mapping()[0, 1] == 8 + 2  # the host side is as usable as before
