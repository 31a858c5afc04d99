"""csrc/quotient.hip (trh_quotient_terms_dev) against tests/quotient_model.py, bit for bit:
  pointwise      random columns at k = 4, extended_k = 7: no term at all, one set, an exact multiple, a ragged last set, lookups alone; two
                 blinding factors; the flat layout and 1, 5, 8 coset blocks; a zero and a non-zero starting acc
  sizes          k = 11, extended_k = 14: more than one workgroup and two levels of the X tables, every row compared; one block at
                 extended_k = 19 for the third level
  second shape   extended_k = k + 1
  bounds         edge residues, every stored word p - 1, every word zero; chunk_len 8
  gates          the fold continues GateEvaluator's accumulator
  end to end     a satisfying witness through the library's own keygen / product / lookup / transform pipeline: the numerator is divisible
                 by X^n - 1 in both layouts, and is not with a copy constraint broken
  stream         inputs written on a non-blocking stream, no synchronisation before the call; a second call on another stream
  refusals       every TRH_EINVAL of the header
  native         tests/native/quotient_test over include/trh.hpp
  replay         --h-args reports its time beside the others"""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import quotient_model as qm
from common import with_edges
from tiny_ram_halo2_amd import api, expr, permutation, quotient, synth
from tiny_ram_halo2_amd.poly import _MODULUS, EvaluationDomain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(0, 4, 0), (1, 4, 0), (4, 4, 0), (8, 4, 1), (9, 4, 3), (5, 2, 2), (0, 4, 2)]  # (n_columns, chunk_len, n_lookups)
BETA, GAMMA, Y = 0x1234567 ** 5, 0x7654321 ** 7, 0xABCDEF ** 9


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


@functools.lru_cache(maxsize=None)
def domain(field, j, k):
    return EvaluationDomain(field, j, k)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1, 4)


def n_sets(n_columns, chunk_len):
    return -(-n_columns // chunk_len)


class Case:
    """stored columns of one call, in the entry's order: values, sigmas, product columns, lookups x 5, l0, l_blind, l_last, acc"""

    def __init__(self, field, dom, shape, blinding, n_blocks, columns, beta=BETA, gamma=GAMMA, y=Y):
        self.field, self.dom, self.shape, self.blinding, self.n_blocks = field, dom, shape, blinding, n_blocks
        self.m = _MODULUS[field]
        self.beta, self.gamma, self.y = beta % self.m, gamma % self.m, y % self.m
        self.lay = qm.Layout(dom, n_blocks)
        n_columns, chunk_len, n_lookups = shape
        self.counts = (n_columns, n_columns, n_sets(n_columns, chunk_len), 5 * n_lookups, 3, 1)
        assert len(columns) == sum(self.counts) and all(c.shape == (self.lay.rows, 4) for c in columns)
        self.columns = columns

    @classmethod
    def random(cls, field, dom, shape, blinding, n_blocks, seed, zero_acc=False, **kw):
        n_columns, chunk_len, n_lookups = shape
        rows = qm.Layout(dom, n_blocks).rows
        cols = qm.random_stored(seed, 2 * n_columns + n_sets(n_columns, chunk_len) + 5 * n_lookups + 4, rows)
        if zero_acc:
            cols[-1] = np.zeros((rows, 4), dtype=np.uint64)
        return cls(field, dom, shape, blinding, n_blocks, cols, **kw)

    def split(self, cols):
        out, at = [], 0
        for c in self.counts:
            out.append(cols[at:at + c])
            at += c
        values, sigmas, zs, lk, ls, acc = out
        return values, sigmas, zs, [lk[5 * i:5 * i + 5] for i in range(len(lk) // 5)], ls, acc[0]

    def model(self, gates=()):
        """stored words of acc after the fold (gates: term columns folded in front of the arguments' own)"""
        values, sigmas, zs, lookups, ls, acc = self.split([qm.to_values(self.field, c) for c in self.columns])
        terms = qm.term_columns(self.lay, values, sigmas, zs, lookups, ls[0], ls[1], ls[2], self.beta, self.gamma, self.shape[1], self.blinding)
        return qm.to_stored(self.field, qm.fold(self.m, acc, list(gates) + terms, self.y))

    def device(self, q=None, stream=None, tensors=None):
        tensors = tensors or [dev(c) for c in self.columns]
        values, sigmas, zs, lookups, ls, acc = self.split(tensors)
        q = q or quotient.QuotientTerms(self.dom, self.shape[0], self.shape[1], self.shape[2], self.blinding)
        q.eval(acc, values, sigmas, zs, lookups, ls[0], ls[1], ls[2], self.beta, self.gamma, self.y, n_blocks=self.n_blocks, stream=stream)
        return host(acc)

    def check(self, **kw):
        got, want = self.device(**kw), self.model()
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, f"{self.field} {self.shape} blinding {self.blinding} blocks {self.n_blocks}: {bad.size} rows differ, first {bad[:8]}"
        return got


# ---- pointwise parity on random columns ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d" % s)
@pytest.mark.parametrize("field", ["fp", "fq"])
def test_random_columns(field, shape):
    dom = domain(field, 9, 4)
    assert dom.extended_k == 7
    for blinding in (2, 5):
        q = quotient.QuotientTerms(dom, shape[0], shape[1], shape[2], blinding)
        for n_blocks in (0, 1, 5, 8):
            for zero_acc in (True, False):
                c = Case.random(field, dom, shape, blinding, n_blocks, seed=1000 * blinding + 10 * n_blocks + zero_acc, zero_acc=zero_acc)
                got = c.check(q=q)
                if shape == (0, 4, 0):
                    assert (got == c.columns[-1]).all(), "no term: acc has to stay as it is"


# ---- past one workgroup and one level of X ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_blocks", [0, 5])
@pytest.mark.parametrize("field", ["fp", "fq"])
def test_many_workgroups(field, n_blocks):
    k = 11
    dom = domain(field, 9, k)
    assert dom.extended_k == 14
    c = Case.random(field, dom, (9, 4, 2), 5, n_blocks, seed=77 + n_blocks)
    got, want = c.device(), c.model()
    n = 1 << k
    pins = [b * n + o for b in range(n_blocks or 8) for o in (0, n - 1)]  # the rotation's wrap, and X across the blocks (stretches of the flat layout)
    for r in pins:
        assert (got[r] == want[r]).all(), f"row {r}"
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:8]


def test_the_third_level_of_the_x_tables():
    """extended_k = 19: a row of block 0 has the exponent q * 8, up to 2^19 - 8, so the third table is read beyond its first entry"""
    k = 16
    dom = domain("fp", 9, k)
    assert dom.extended_k == 19
    c = Case.random("fp", dom, (1, 4, 0), 5, 1, seed=19)
    got, want = c.device(), c.model()
    assert (got[[0, (1 << k) - 1]] == want[[0, (1 << k) - 1]]).all()
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:8]


# ---- a second domain shape -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_blocks", [0, 1, 2])
@pytest.mark.parametrize("field", ["fp", "fq"])
def test_extended_k_one_above_k(field, n_blocks):
    dom = domain(field, 3, 4)
    assert dom.extended_k == 5
    Case.random(field, dom, (5, 2, 2), 2, n_blocks, seed=31 + n_blocks).check()


# ---- the bounds of the lazy domain -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_blocks", [0, 5])
@pytest.mark.parametrize("field", ["fp", "fq"])
def test_edge_residues(field, n_blocks):
    """n_columns = 9 in sets of 8: the longest product chain (eight factors on each side, degree 6 + margin for the reference's 4)"""
    dom = domain(field, 9, 6)
    c = Case.random(field, dom, (9, 8, 2), 5, n_blocks, seed=5)
    c.columns = [with_edges(col, seed=i, field=field, zeros=True) for i, col in enumerate(c.columns)]
    c.check()


@pytest.mark.parametrize("word", ["p-1", "zero"])
@pytest.mark.parametrize("field", ["fp", "fq"])
def test_extreme_words(field, word):
    """every stored word of every column and of beta, gamma, y the largest canonical one, p - 1 (every loaded value just below 32 p, every
    constant just below p: the bounds of csrc/quotient.hip's header at their ends), or zero"""
    m = _MODULUS[field]
    dom = domain(field, 9, 4)
    stored = m - 1 if word == "p-1" else 0
    challenge = stored * pow(1 << 256, -1, m) % m  # the value whose Montgomery word is `stored`
    for n_blocks in (0, 5):
        rows = qm.Layout(dom, n_blocks).rows
        c = Case.random(field, dom, (9, 8, 2), 5, n_blocks, seed=1, beta=challenge, gamma=challenge, y=challenge)
        c.columns = [synth.ints_to_limbs([stored] * rows) for _ in c.columns]
        c.check()


# ---- the fold continues the gates' -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["fp", "fq"])
def test_the_fold_continues_the_gates(field):
    k, m = 4, _MODULUS[field]
    dom = domain(field, 9, k)
    c = Case.random(field, dom, (5, 2, 2), 2, 0, seed=404, zero_acc=True)
    A = [expr.Advice(i, 0) for i in range(3)]
    gates = [A[0] * A[1] - A[2], expr.Advice(0, 1) - A[1] + 3]
    ev = expr.GateEvaluator(expr.compile_gates(field, gates, y=c.y))
    adv = qm.random_stored(9001, 3, c.lay.rows)
    tensors = [dev(col) for col in c.columns]
    out = ev.eval({("advice", i): dev(adv[i]) for i in range(3)}, dom.extended_k, 1 << (dom.extended_k - k), out=tensors[-1])
    assert out.data_ptr() == tensors[-1].data_ptr()
    got = c.device(tensors=tensors)
    a = [qm.to_values(field, col) for col in adv]
    R = range(c.lay.rows)
    g0 = [(a[0][i] * a[1][i] - a[2][i]) % m for i in R]
    g1 = [(a[0][c.lay.rot(i, 1)] - a[1][i] + 3) % m for i in R]
    assert (got == c.model(gates=[g0, g1])).all()


# ---- end to end: the library's own pipeline on a satisfying witness ---------------------------------------------------------------------
def _pipeline(w, dom, beta, gamma, break_a_copy=False):
    """the witness's advice values and lookup inputs / tables -> sigma columns (Assembly), product columns (grand_products_terms), permuted
    columns (lookup_permute), all as Lagrange columns on the device: values, sigmas, zs, lookups"""
    field, n, u, m = w.field, w.n, w.usable, w.m
    lag = lambda col: dev(qm.to_stored(field, col))  # noqa: E731
    cols = [list(c) for c in w.values]
    if break_a_copy:
        c = next(c for c in w.copies if c[:2] != c[2:])
        cols[c[0]][c[1]] = (cols[c[0]][c[1]] + 1) % m
    values = [lag(c) for c in cols]
    asm = permutation.Assembly(field, w.k, w.n_columns)
    asm.copy_many(w.copies)
    sig = asm.sigma_columns()
    sigmas = [sig[j] for j in range(w.n_columns)]
    st = torch.cuda.current_stream().cuda_stream
    omega_powers = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    api.powers_dev(field, omega_powers, n, expr._limbs(field, permutation.omega(field, w.k)), stream=st)
    num, den = [], []
    for s in range(0, w.n_columns, w.chunk_len):
        a, b = permutation.permutation_terms(field, values[s:s + w.chunk_len], sigmas[s:s + w.chunk_len], omega_powers, beta, gamma, first_column=s)
        num.append(a); den.append(b)
    lookups = []
    for a, s_, ap, sp, _ in w.lookups:
        da, ds = lag(a), lag(s_)
        pa, ps = permutation.lookup_permute(field, da, ds, usable_rows=u)
        pa = torch.cat([pa, lag(ap[u:])]).contiguous()  # the blinding rows
        ps = torch.cat([ps, lag(sp[u:])]).contiguous()
        a_, b_ = permutation.lookup_terms(field, da, ds, pa, ps, beta, gamma)
        num.append(a_); den.append(b_)
        lookups.append([da, ds, pa, ps])
    z = permutation.grand_products_terms(field, w.k, num, den)
    sets = n_sets(w.n_columns, w.chunk_len)
    zs = [z[0].contiguous()]
    for s in range(1, sets):  # z_s[0] = z_(s-1)[u]: the next set's column starts where the last one ended
        start = synth.limbs_to_ints(host(zs[-1])[u:u + 1])[0]
        col = z[s].contiguous()
        api.field_scale_dev(field, col, n, synth.ints_to_limbs([start])[0], stream=st)
        zs.append(col)
    for i, l in enumerate(lookups):
        l.append(z[sets + i].contiguous())
    return values, sigmas, zs, lookups


def test_end_to_end_divisibility():
    field, k, j = "fp", 5, 6
    m, n = _MODULUS[field], 1 << k
    dom = domain(field, j, k)
    assert dom.extended_k == k + 3 and dom.quotient_poly_degree == 5
    beta, gamma, y = BETA % m, GAMMA % m, Y % m
    blinding, shape = 5, (9, 4, 2)
    w = qm.Witness(field, k, shape[0], shape[1], shape[2], blinding, beta, gamma, seed=23)
    q = quotient.QuotientTerms(dom, shape[0], shape[1], shape[2], blinding)

    def numerator(cols, n_blocks):
        values, sigmas, zs, lookups = cols
        flat = list(values) + list(sigmas) + list(zs) + [c for l in lookups for c in l]
        coeff = dom.lagrange_to_coeff(torch.stack(flat))
        ext = dom.coeff_to_extended_blocks(coeff, n_blocks) if n_blocks else dom.coeff_to_extended(coeff)
        ext = [ext[i] for i in range(len(flat))]
        nv, ns = len(values), len(zs)
        ls = quotient.lagrange_basis_columns(dom, blinding, n_blocks)
        acc = torch.zeros_like(ext[0])
        q.eval(acc, ext[:nv], ext[nv:2 * nv], ext[2 * nv:2 * nv + ns], [ext[2 * nv + ns + 5 * i:2 * nv + ns + 5 * i + 5] for i in range(len(lookups))],
               ls[0], ls[1], ls[2], beta, gamma, y, n_blocks=n_blocks)
        return acc

    good = _pipeline(w, dom, beta, gamma)
    acc = numerator(good, 0)
    dom.extended_to_coeff(acc)  # in place; every one of the 2^extended_k coefficients is read below
    coeffs = qm.to_values(field, host(acc))
    assert qm.residues_mod_vanishing(m, coeffs, n) == [0] * n
    assert 0 <= qm.degree(coeffs) <= 6 * (n - 1)
    blocks = numerator(good, dom.quotient_poly_degree)
    h = qm.to_values(field, host(dom.blocks_to_quotient(blocks, divide_by_vanishing=True)))
    assert len(h) == 5 * n
    product = [((h[i - n] if i >= n else 0) - (h[i] if i < 5 * n else 0)) % m for i in range(6 * n)]
    assert product == coeffs[:6 * n] and not any(coeffs[6 * n:])
    # control: one copy constraint broken
    acc = numerator(_pipeline(w, dom, beta, gamma, break_a_copy=True), 0)
    dom.extended_to_coeff(acc)
    assert any(qm.residues_mod_vanishing(m, qm.to_values(field, host(acc)), n))


# ---- stream ----------------------------------------------------------------------------------------------------------------------------
def test_inputs_written_on_the_callers_stream():
    field = "fq"
    dom = domain(field, 9, 4)
    c = Case.random(field, dom, (9, 4, 2), 5, 5, seed=808)
    want = c.model()
    q = quotient.QuotientTerms(dom, 9, 4, 2, 5)
    real = [dev(col) for col in c.columns]
    bufs = [torch.full_like(t, 0x0101010101010101) for t in real]  # what a call that does not wait for the stream would read
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()  # torch's streams are non-blocking: nothing orders them behind the null stream
    with torch.cuda.stream(s1):
        torch.cuda._sleep(2_000_000)  # the copies are still queued when the entry is called
        for b, r in zip(bufs, real):
            b.copy_(r, non_blocking=True)
    assert (c.device(q=q, stream=s1.cuda_stream, tensors=bufs) == want).all()
    with torch.cuda.stream(s2):
        s2.wait_stream(s1)
        torch.cuda._sleep(2_000_000)
        bufs[-1].copy_(real[-1], non_blocking=True)  # acc again: the first call wrote its result there
    assert (c.device(q=q, stream=s2.cuda_stream, tensors=bufs) == want).all()
    torch.cuda.synchronize()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = api.lib()
    dom = domain("fp", 9, 4)

    def refused(rc):
        assert rc == -1 and lib.trh_last_error(), rc

    h = ctypes.c_void_p()
    refused(lib.trh_quotient_create(dom.handle(), 4, 0, 1, 2, ctypes.byref(h)))         # chunk_len = 0
    refused(lib.trh_quotient_create(dom.handle(), 4, 4, 1, 15, ctypes.byref(h)))        # blinding_factors + 2 > 2^k
    assert lib.trh_quotient_create(dom.handle(), 4, 4, 1, 14, ctypes.byref(h)) == 0      # ... and the largest that fits
    lib.trh_quotient_destroy(h)
    c = Case.random("fp", dom, (4, 4, 1), 2, 5, seed=3)
    q = quotient.QuotientTerms(dom, 4, 4, 1, 2)
    tensors = [dev(col) for col in c.columns]
    before = host(tensors[-1]).copy()
    values, sigmas, zs, lookups, ls, acc = c.split(tensors)

    def args(**change):
        a = api.QuotientArgs()
        keep = [(ctypes.c_void_p * len(g))(*[t.data_ptr() for t in g]) for g in (values, sigmas, zs, lookups[0])]
        a.perm_values, a.perm_sigmas, a.perm_z, a.lookups = keep
        a.l0, a.l_blind, a.l_last, a.acc = ls[0].data_ptr(), ls[1].data_ptr(), ls[2].data_ptr(), acc.data_ptr()
        a.beta[:], a.gamma[:], a.y[:] = [[int(v) for v in expr._limbs("fp", ch)] for ch in (c.beta, c.gamma, c.y)]
        a.n_blocks = 5
        a.stream = torch.cuda.current_stream().cuda_stream
        for name, v in change.items():
            setattr(a, name, v)
        return a, keep

    null_array = ctypes.POINTER(ctypes.c_void_p)()
    changes = [dict(n_blocks=9)] + [{name: null_array} for name in ("perm_values", "perm_sigmas", "perm_z", "lookups")]
    changes += [{name: None} for name in ("acc", "l0", "l_blind", "l_last")]
    changes += [dict(acc=values[1].data_ptr()), dict(acc=zs[0].data_ptr()), dict(acc=lookups[0][2].data_ptr()), dict(acc=ls[2].data_ptr())]
    with_null = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in values])
    with_null[2] = None
    changes.append(dict(perm_values=with_null))
    for change in changes:
        a, keep = args(**change)
        refused(lib.trh_quotient_terms_dev(q.handle, ctypes.byref(a)))
    torch.cuda.synchronize()
    assert (host(tensors[-1]) == before).all() and (host(values[1]) == c.columns[1]).all(), "a refused call wrote"
    a, keep = args()
    assert lib.trh_quotient_terms_dev(q.handle, ctypes.byref(a)) == 0
    assert (host(tensors[-1]) == c.model()).all()


# ---- trh::QuotientTerms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,n_blocks", [("fp", 0), ("fq", 5)])
def test_native_quotient_terms(field, n_blocks, tmp_path):
    exe = os.path.join(ROOT, "tests", "native", "quotient_test")
    assert os.path.exists(exe), "tests/native/quotient_test is missing: run `make`"
    j, k, shape, blinding = 9, 4, (9, 4, 2), 5
    c = Case.random(field, domain(field, j, k), shape, blinding, n_blocks, seed=606)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as fh:
        fh.write(np.array([api.FIELD_ID[field], j, k, shape[0], shape[1], shape[2], blinding, n_blocks], dtype="<u4").tobytes())
        for v in (c.beta, c.gamma, c.y):
            fh.write(expr._limbs(field, v).astype("<u8").tobytes())
        for col in c.columns:
            fh.write(np.ascontiguousarray(col, dtype="<u8").tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["checks_failed"] == 0
    got = np.fromfile(dst, dtype="<u8").reshape(-1, 4)
    assert (got == c.model()).all()


# ---- the replay's opt-in step ----------------------------------------------------------------------------------------------------------
def test_replay_reports_h_args_outside_the_total():
    from tiny_ram_halo2_amd import replay
    res = replay.run(16, batch=32, verbose=False, columns="witness", keygen=False, h_args=True)
    assert res["h_args_ms"] > 0 and res["h_args"]["perm_columns"] == 188 and res["h_args"]["lookups"] == 31
    assert "h_args" not in res["gpu_ms"] and abs(sum(res["gpu_ms"].values()) - res["gpu_ms_total"]) < 0.01
