"""GPU tests (-m gpu) of the permutation keygen (csrc/permutation.hip, permutation.Assembly): the sigma columns against big integers, the
device copy of the mapping across a copy(), the sigma columns through the grand product that consumes them, the copy-constraint check's
reductions against numpy, build_vk / build_pk against the oracle, the refusals, and trh::PermutationAssembly from a compiled host.
Every comparison is limb for limb.  The assembly itself (the order of the merges) is tested without a device in tests/test_permkeygen_host.py."""
import ctypes
import functools
import json
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import cpu_ref
import pasta as o
import permkeygen_model as pm
from tiny_ram_halo2_amd import api, permutation, poly, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["fp", "fq"]
EINVAL = -1
# (k, columns): one block of two cells; 96 cells, a partial block; several blocks; twenty columns with thousands of copies
SHAPES = [(1, 1), (5, 3), (9, 5), (12, 20)]
N_COPIES = {(1, 1): 1, (5, 3): 40, (9, 5): 500, (12, 20): 5000}


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def to_host(t):
    torch.cuda.synchronize()
    return t.contiguous().cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def identity_limbs(field, k, n_columns):
    """(cells, 4): f.limbs(delta^c omega^r) for cell c * n + r, in big integers; computed once per shape and never written to"""
    f = o.FIELDS[field]
    m, n = f.m, 1 << k
    delta, omega = pow(5, 1 << 32, m), f.omega(k)
    assert delta == f.DELTA == permutation.delta(field) and omega == permutation.omega(field, k) and pow(omega, n, m) == 1 and (n == 1 or pow(omega, n // 2, m) != 1)
    dc, wr = [pow(delta, c, m) for c in range(n_columns)], [pow(omega, r, m) for r in range(n)]
    out = np.array([f.limbs(d * w % m) for d in dc for w in wr], dtype=np.uint64)
    out.setflags(write=False)
    return out


def random_copies(k, n_columns, count, seed, max_row=None):
    rng = random.Random(seed)
    rows = (1 << k) if max_row is None else max_row
    return [(rng.randrange(n_columns), rng.randrange(rows), rng.randrange(n_columns), rng.randrange(rows)) for _ in range(count)]


def sort_rows(a):
    a = np.ascontiguousarray(a).reshape(-1, 4)
    return a[np.lexsort((a[:, 0], a[:, 1], a[:, 2], a[:, 3]))]


# ---- sigma values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k,n_columns", SHAPES)
@pytest.mark.parametrize("copies", ["identity", "copies"])
def test_sigma_columns_against_big_integers(field, k, n_columns, copies):
    n = 1 << k
    ident = identity_limbs(field, k, n_columns)
    a = permutation.Assembly(field, k, n_columns)
    if copies == "copies":
        script = [(0, 0, 0, 1)] if (k, n_columns) == (1, 1) else random_copies(k, n_columns, N_COPIES[(k, n_columns)], 0xC0B1E5 + k)
        a.copy_many(script)
    mapping = a.mapping().reshape(-1).astype(np.int64)
    if copies == "identity":
        assert (mapping == np.arange(n_columns * n)).all()
    else:
        assert (mapping != np.arange(n_columns * n)).any()
    got = to_host(a.sigma_columns())
    assert got.shape == (n_columns, n, 4)
    assert (got.reshape(-1, 4) == ident[mapping]).all()
    # a permutation of the cells: the multiset of sigma values is the multiset of delta^c omega^r
    assert (sort_rows(got) == sort_rows(ident)).all()
    a.destroy()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k,n_columns", SHAPES)
def test_sigma_window_whose_cells_map_outside_it(field, k, n_columns):
    """columns [2, 4) of a mapping whose cells there point into columns 0 and 4: a delta table sized to the window, or indexed from its
    first column, gives other values.  Shapes with fewer than five columns have no such window; they take their last column alone, with
    cells that point into column 0 where there is another column."""
    n = 1 << k
    ident = identity_limbs(field, k, n_columns)
    a = permutation.Assembly(field, k, n_columns)
    if n_columns >= 5:
        first, count = 2, 2
        for r in range(0, n, max(n // 16, 1)):
            a.copy(2, r, 0, (r + 1) % n)
            a.copy(3, r, 4, (r + 3) % n)
    else:
        first, count = n_columns - 1, 1
        a.copy(first, 0, 0, n - 1)
    mapping = a.mapping().astype(np.int64)
    window = mapping[first:first + count]
    if n_columns >= 5:
        assert (window[0] // n == 0).any() and (window[1] // n == 4).any()  # cells of the window do map to columns 0 and 4
    got = to_host(a.sigma_columns(first, count))
    assert got.shape == (count, n, 4) and (got.reshape(-1, 4) == ident[window.reshape(-1)]).all()
    assert (to_host(a.sigma_columns(n_columns, 0)).shape == (0, n, 4))
    a.destroy()


@pytest.mark.parametrize("field", FIELDS)
def test_a_copy_invalidates_the_device_mapping(field):
    k, n_columns = 5, 3
    n = 1 << k
    ident = identity_limbs(field, k, n_columns)
    a = permutation.Assembly(field, k, n_columns)
    a.copy_many(random_copies(k, n_columns, 20, 77))
    m0 = a.mapping().reshape(-1).astype(np.int64)
    s0 = to_host(a.sigma_columns()).reshape(-1, 4)
    assert (to_host(a.sigma_columns()).reshape(-1, 4) == s0).all()  # the resident copy, used again
    left, right = (0, 3), (2, 7)
    cl, cr = left[0] * n + left[1], right[0] * n + right[1]
    cyc = [c for c in pm.cycles(list(m0)) if cl in c]
    assert cr not in cyc[0]  # the two cells are in different cycles: the copy swaps their images
    a.copy(*left, *right)
    m1 = a.mapping().reshape(-1).astype(np.int64)
    s1 = to_host(a.sigma_columns()).reshape(-1, 4)
    changed = np.nonzero((s0 != s1).any(axis=1))[0]
    assert list(changed) == sorted((cl, cr)) and (s1 == ident[m1]).all()
    assert (s1[cl] == s0[cr]).all() and (s1[cr] == s0[cl]).all()
    a.destroy()


# ---- the sigma columns in the argument that consumes them -------------------------------------------------------------------------------
def cycle_values(mapping, seed):
    """(cells, 4): one random element per cycle of the mapping"""
    cyc = sorted(pm.cycles(list(mapping)), key=min)
    vals = synth.field_elements(seed, len(cyc))
    out = np.zeros((len(mapping), 4), dtype=np.uint64)
    for i, c in enumerate(cyc):
        out[sorted(c)] = vals[i]
    return out, cyc


@pytest.mark.parametrize("field", FIELDS)
def test_grand_product_closes_and_check_agrees(field):
    k, n_columns = 9, 4
    n = 1 << k
    f = o.FIELDS[field]
    rng = random.Random(0x9A0D + len(field))
    beta, gamma = rng.randrange(1, f.m), rng.randrange(1, f.m)
    a = permutation.Assembly(field, k, n_columns)
    a.copy_many(random_copies(k, n_columns, 300, 0x10099, max_row=n - 1))  # no cell of row n - 1: that row's ratio is one
    mapping = a.mapping().reshape(-1).astype(np.int64)
    assert all(mapping[c * n + n - 1] == c * n + n - 1 for c in range(n_columns))
    values, cyc = cycle_values(mapping, 0xCE11)
    sig = a.sigma_columns()
    pc = permutation.ProductColumn(field, k, n_columns)

    def z_last(vals):
        cols = to_dev(vals.reshape(n_columns, n, 4))
        z = pc.compute([cols[j] for j in range(n_columns)], [sig[j] for j in range(n_columns)], beta, gamma)
        return [int(v) for v in to_host(z)[n - 1]], a.check(cols)

    one = f.limbs(1)
    z, chk = z_last(values)
    assert z == one and chk == (0, None)
    cell = min(min(c) for c in cyc if len(c) >= 2)
    pred = int(np.nonzero(mapping == cell)[0][0])
    broken = values.copy()
    broken[cell] = synth.field_elements(0xBAD, 1)[0]
    z, chk = z_last(broken)
    first = min(cell, pred)
    assert z != one and chk == (2, (first // n, first % n))
    a.destroy()


# ---- the check kernel's reductions ------------------------------------------------------------------------------------------------------
WAVE_EDGES = [3 * 256 + 63, 3 * 256 + 64, 3 * 256 + 191, 3 * 256 + 192, 9 * 256, 9 * 256 + 255]   # cells of column 0; then the last cell


def big_assembly(extra_pairs):
    k, n_columns = 12, 20
    n = 1 << k
    a = permutation.Assembly("fp", k, n_columns)
    a.copy_many(random_copies(k, n_columns, 5000, 0xB16))
    pairs = [(c, r, (c + 7) % n_columns, r + 1) for c in range(n_columns) for r in range(0, n, 128)] + [(n_columns - 1, n - 1, 3, 5)]
    a.copy_many(pairs + extra_pairs)
    mapping = a.mapping().reshape(-1).astype(np.int64)
    values, _ = cycle_values(mapping, 0xB17)
    values.setflags(write=False)
    return a, mapping, values, [c * n + r for c, r, _, _ in pairs]


@pytest.fixture(scope="module")
def big():
    """(12, 20) with 5 000 random copies, and pairs that put a cycle of two or more cells into every block of 256 cells, cell 0 and the last"""
    made = big_assembly([])
    yield made
    made[0].destroy()


@pytest.fixture(scope="module")
def big_edges():
    """the same, and every cell of WAVE_EDGES copied to its row in column 10: in `big` four of the six are alone in their cycle, and a cell
    that maps to itself cannot be bad whatever its value"""
    made = big_assembly([(0, cell, 10, cell) for cell in WAVE_EDGES])
    yield made
    made[0].destroy()


@pytest.mark.parametrize("case", ["none", "cell_0", "last_cell", "every_block", "wave_edges"])
def test_check_against_numpy(request, case):
    """wave_edges: the last lane of a wave and the first of the next, twice in one block (all four of its waves report), the first and the
    last lane of another block, and the last cell -- every wave adds its own count and lowers the minimum itself, so the total and the
    first cell are right only if no wave's report is lost or merged with a neighbour's"""
    a, mapping, values, marked = request.getfixturevalue("big_edges" if case == "wave_edges" else "big")
    n, cells = a.n, a.n * a.n_columns
    vals = values.copy()
    changed = {"none": [], "cell_0": [0], "last_cell": [cells - 1], "every_block": marked, "wave_edges": WAVE_EDGES + [cells - 1]}[case]
    vals[changed] = synth.field_elements(0xC4A, len(changed))
    bad = (vals != vals[mapping]).any(axis=1)
    n_bad = int(bad.sum())
    if case == "none":
        assert n_bad == 0
    elif case == "every_block":
        assert bad.reshape(-1, 256).any(axis=1).all() and n_bad > cells // 256
    elif case == "wave_edges":
        # every changed cell is bad, and no cell that maps to one lies in blocks 0 .. 2: the first bad cell is in block 3, not in block 0
        assert bad[changed].all() and not bad[:3 * 256].any() and int(np.argmax(bad)) == 3 * 256 + 63
    else:
        assert n_bad == 2 and bad[changed[0]]
    first = int(np.argmax(bad)) if n_bad else None
    want = (n_bad, (first // n, first % n) if n_bad else None)
    cols = to_dev(vals.reshape(a.n_columns, n, 4))
    assert a.check(cols) == want
    assert a.check([cols[j] for j in range(a.n_columns)]) == want


# ---- build_vk / build_pk ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["vesta", "pallas"])
def test_build_vk_and_build_pk_against_the_oracle(curve):
    k, n_columns, j = 6, 3, 4
    n = 1 << k
    field = api.SCALAR_FIELD[curve]
    f = o.FIELDS[field]
    gl = cpu_ref.gen_bases(curve, 1234567, 5, n, threads=4)
    w = cpu_ref.gen_bases(curve, 999, 1, 1, threads=1)
    params = poly.Params(curve, k, cpu_ref.gen_bases(curve, 11, 3, n, threads=4), gl, w)
    a = permutation.Assembly(field, k, n_columns)
    a.copy_many(random_copies(k, n_columns, 60, 0xF1C))
    sigma = identity_limbs(field, k, n_columns)[a.mapping().reshape(-1).astype(np.int64)].reshape(n_columns, n, 4)
    one = np.array(f.limbs(1), dtype=np.uint64)
    got = a.build_vk(params)
    assert got.shape == (n_columns, 12)
    for c in range(n_columns):  # commit_lagrange(sigma_c, Blind::default()): the MSM over g_lagrange plus [1] W
        want = cpu_ref.to_affine(curve, cpu_ref.best_multiexp(curve, np.concatenate([sigma[c], one[None]]), np.concatenate([gl, w]), threads=4))
        assert (got[c, :8] == want).all() and [int(v) for v in got[c, 8:]] == o.CURVES[curve].base.limbs(1)
    dom, ref = poly.EvaluationDomain(field, j, k), cpu_ref.EvaluationDomain(field, j, k, threads=4)
    permutations, polys, cosets = a.build_pk(dom)
    assert (to_host(permutations) == sigma).all()
    want_polys = np.stack([ref.lagrange_to_coeff(sigma[c]) for c in range(n_columns)])
    assert (to_host(polys) == want_polys).all()
    assert cosets.shape == (n_columns, dom.extended_len(), 4)
    assert (to_host(cosets) == np.stack([ref.coeff_to_extended(want_polys[c]) for c in range(n_columns)])).all()
    assert (to_host(dom.coeff_to_extended(to_dev(want_polys))) == to_host(cosets)).all()  # the existing mirror, from the oracle's coefficients
    a.destroy()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _err():
    return api.lib().trh_last_error().decode()


def test_refusals_leave_the_context_usable():
    lib = api.lib()
    k, n_columns = 5, 3
    n = 1 << k
    a = permutation.Assembly("fp", k, n_columns)
    a.copy(0, 1, 2, 2)
    ident = identity_limbs("fp", k, n_columns)
    want = ident[a.mapping().reshape(-1).astype(np.int64)]
    out = torch.zeros((n_columns, n, 4), dtype=torch.int64, device="cuda")
    cols = to_dev(np.tile(ident[:1], (n_columns * n, 1)).reshape(n_columns, n, 4))
    ptrs = (api._vp * n_columns)(*[cols[j].data_ptr() for j in range(n_columns)])
    n_bad, first = ctypes.c_uint64(7), ctypes.c_uint64(7)
    st = torch.cuda.current_stream().cuda_stream
    # an unknown field id
    assert lib.trh_perm_sigma_dev(a.handle, 7, 0, n_columns, api._devptr(out), st) == EINVAL and _err() == "unknown field id 7"
    assert lib.trh_perm_check_dev(a.handle, 7, ptrs, ctypes.byref(n_bad), ctypes.byref(first), st) == EINVAL and _err() == "unknown field id 7"
    # null pointers
    assert lib.trh_perm_sigma_dev(a.handle, 0, 0, n_columns, None, st) == EINVAL
    assert lib.trh_perm_sigma_dev(None, 0, 0, n_columns, api._devptr(out), st) == EINVAL
    assert lib.trh_perm_check_dev(a.handle, 0, None, ctypes.byref(n_bad), ctypes.byref(first), st) == EINVAL
    assert lib.trh_perm_check_dev(a.handle, 0, ptrs, None, ctypes.byref(first), st) == EINVAL
    assert lib.trh_perm_check_dev(a.handle, 0, ptrs, ctypes.byref(n_bad), None, st) == EINVAL
    holed = (api._vp * n_columns)(cols[0].data_ptr(), None, cols[2].data_ptr())
    assert lib.trh_perm_check_dev(a.handle, 0, holed, ctypes.byref(n_bad), ctypes.byref(first), st) == EINVAL and "column 1" in _err()
    # a window past the last column
    for first_column, count in ((2, 2), (4, 0), (0, 4), ((1 << 32) - 1, 2)):
        assert lib.trh_perm_sigma_dev(a.handle, 0, first_column, count, api._devptr(out), st) == EINVAL and "of 3" in _err(), (first_column, count)
    with pytest.raises(api.TrhError):
        a.sigma_columns(2, 2)
    torch.cuda.synchronize()
    assert n_bad.value == 7 and first.value == 7 and not out.any()  # nothing was written by any of the refused calls
    # the same handle and context, used straight afterwards
    assert lib.trh_perm_sigma_dev(a.handle, 0, 0, n_columns, api._devptr(out), st) == 0
    assert (to_host(out).reshape(-1, 4) == want).all()
    assert a.check(cols) == (0, None)  # equal values everywhere satisfy any copy constraint
    a.destroy()


# ---- the C++ mirror ---------------------------------------------------------------------------------------------------------------------
def _fnv(words):
    h = 0xcbf29ce484222325
    for w in words:
        h = ((h ^ int(w)) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def test_permutation_assembly_from_cpp(tmp_path):
    """tests/native/perm_assembly_test.cpp: trh::PermutationAssembly over include/trh.hpp from a compiled host, against this side's mapping"""
    exe = os.path.join(ROOT, "tests", "native", "perm_assembly_test")
    if not os.path.exists(exe):  # normally built by `make` / __graft_entry__.build(); g++ only, libtrh.so must already be there
        subprocess.check_call(["make", "-s", "-C", ROOT, "tests/native/perm_assembly_test"])
    field, k, n_columns = "fq", 6, 3
    n = 1 << k
    copies = random_copies(k, n_columns, 41, 0xC99)
    a = permutation.Assembly(field, k, n_columns)
    a.copy_many(copies)
    mapping = a.mapping().reshape(-1)
    sigma = to_host(a.sigma_columns()).reshape(-1)
    src = tmp_path / "copies.txt"
    src.write_text(f"{field} {k} {n_columns} {len(copies)}\n" + "".join("%d %d %d %d\n" % c for c in copies))
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    got = json.loads(r.stdout.strip().splitlines()[-1])
    moved = np.nonzero(mapping != np.arange(n_columns * n))[0]
    assert got["checks_failed"] == 0 and got["mapping"] == _fnv(mapping) and got["sigma"] == _fnv(sigma)
    assert got["n_bad"] == len(moved) > 0 and got["first_bad_cell"] == int(moved[0])
    # build_vk over the same synthetic resident generators (trh::Params(curve, k, 11, 3): g_lagrange = generate(11 + 77, 3 + 2) of n + 1 points), build_pk at j = 4
    gl = api.Bases.generate("pallas", 11 + 77, 3 + 2, n + 1)
    one = np.array(o.FIELDS[field].limbs(1), dtype=np.uint64)
    vk = gl.commit_batch_dev(a.sigma_columns(), n, n_columns, np.tile(one, (n_columns, 1)), stream=torch.cuda.current_stream().cuda_stream)
    _, polys, cosets = a.build_pk(poly.EvaluationDomain(field, 4, k))
    assert got["vk"] == _fnv(vk.reshape(-1)) and got["polys"] == _fnv(to_host(polys).reshape(-1)) and got["cosets"] == _fnv(to_host(cosets).reshape(-1))
    gl.destroy()
    a.destroy()
