"""GPU tests (-m gpu) of the scan, reduction and powers kernels (csrc/scan.hip, the element-wise part of csrc/ipa.hip) past their
first level: sizes at which the totals scan gives a thread more than one block total, the rows form with several blocks per row and
more rows than one launch takes, reductions sized against the block caps of their launch code, and inputs that hold the stored words
random data never produces (common.with_edges: 0, m - 1, [2^254, m), ...).

Scans and powers are checked in full by induction with the C++ oracle's field operations (oracle/cpu_ref.cpp, itself checked on the
edge residues by tests/test_oracle.py): the first element is the identity and every element follows from the one before it, which
determines the whole output.  One big-int value per case shares nothing with that oracle.  All comparisons are limb-for-limb."""
import numpy as np
import pytest
import torch

import cpu_ref
import pasta as o
from common import stored_ints, with_edges
from tiny_ram_halo2_amd import api, synth

pytestmark = pytest.mark.gpu

FIELDS = ["fp", "fq"]
SCAN_BLOCK = 4096     # scan.hip: elements per workgroup of the first level (256 threads x 16)
TOTALS_THREADS = 256  # scan.hip scan_totals_kernel: one workgroup, thread t takes the totals [t * per, (t + 1) * per), per = ceil(blocks / 256)


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def to_host(t):
    torch.cuda.synchronize()
    return t.contiguous().cpu().numpy().view(np.uint64)


def lim(f, v):
    return np.array(f.limbs(v), np.uint64)


def first_bad(ok):
    """index of the first row of the (n, 4) comparison `ok` that does not match, or None"""
    bad = np.flatnonzero(~ok.all(axis=-1).reshape(-1))
    return int(bad[0]) if bad.size else None


def scan_where(i, n):
    """where element i of a scan of n elements is computed: (block, thread of the totals scan that owns the block's total, per)"""
    blocks = (n + SCAN_BLOCK - 1) // SCAN_BLOCK
    per = (blocks + TOTALS_THREADS - 1) // TOTALS_THREADS
    return {"index": i, "block": i // SCAN_BLOCK, "totals_thread": i // SCAN_BLOCK // per, "per": per, "n": n}


def check_exclusive_scan(field, op, a, out):
    """out[0] is the identity of `op` and out[i + 1] == out[i] op a[i] for every i: `out` is the exclusive scan of `a`"""
    f = o.FIELDS[field]
    n = a.shape[0]
    assert out.shape == a.shape
    ident = lim(f, 1) if op == "mul" else np.zeros(4, np.uint64)
    assert (out[0] == ident).all()
    if n > 1:
        bad = first_bad(cpu_ref.field_op(field, op, out[:-1], a[:-1]) == out[1:])
        assert bad is None, scan_where(bad + 1, n)


def stored_product(f, vals):
    """stored form of the product of the elements whose stored forms are `vals` (big ints): prod(vals) R^-(len - 1)"""
    run = 1
    for v in vals:
        run = run * v % f.m
    return run * pow(f.R, 1 - len(vals), f.m) % f.m


def prefix_sum_dev(field, d, out, n):
    api._check(api.lib().trh_field_prefix_sum_dev(api.FIELD_ID[field], api._devptr(d), api._devptr(out), n, None))


def prefix_product_rows_dev(field, d, out, n, rows):
    api._check(api.lib().trh_field_prefix_product_rows_dev(api.FIELD_ID[field], api._devptr(d), api._devptr(out), n, rows, None))


# 4096 / 4097: one block / two.  2^20: 256 totals, every thread of the totals scan has exactly one.  2^20 + 1: 257 totals, per = 2, threads
# 129 and above have nothing.  3 2^20 + 5: 769 totals, per = 4, the last busy thread (192) has one.
SCAN_SIZES = [4096, 4097, 1 << 20, (1 << 20) + 1, 3 * (1 << 20) + 5]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_prefix_product_sizes(field, n):
    """z[i] = prod_{j < i} a[j] in full; the input holds edge residues and exactly one zero, at n - 3 (an earlier one would blind the rest)"""
    f = o.FIELDS[field]
    a = with_edges(synth.field_elements(0x5C10 + n, n), n, field, zero_at=(n - 3,))
    out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    api.prefix_product_dev(field, to_dev(a), out, n)
    z = to_host(out)
    check_exclusive_scan(field, "mul", a, z)
    # big ints: the last prefix before the zero, and the last index (zero: the prefix includes a[n - 3])
    assert stored_ints(z[n - 3:n - 2]) == [stored_product(f, stored_ints(a[:n - 3]))]
    assert not z[n - 1].any() and not z[n - 2].any()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_prefix_sum_sizes(field, n):
    """s[i] = sum_{j < i} a[j] in full (the scan kate_division runs); edge residues and zeros anywhere"""
    f = o.FIELDS[field]
    a = with_edges(synth.field_elements(0x5C20 + n, n), n + 1, field, zeros=True)
    out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    prefix_sum_dev(field, to_dev(a), out, n)
    s = to_host(out)
    check_exclusive_scan(field, "add", a, s)
    assert stored_ints(s[n - 1:]) == [sum(stored_ints(a[:n - 1])) % f.m]  # the stored form is linear: the sum of the stored forms mod m


# (rows, n): several blocks per row with a ragged last block; a row length that is no multiple of anything; per = 2 in every row's totals
# scan; and more rows than one launch takes (grid.y limit 32768: the only case that runs the second trip of the row loop)
ROWS_CASES = [(3, 4097), (4, 3 * 4096 - 5), (5, (1 << 20) + 1), (32769, 2)]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("rows,n", ROWS_CASES)
def test_prefix_product_rows(field, rows, n):
    """trh_field_prefix_product_rows_dev: every row is the exclusive prefix product of that row alone (distinct data per row, one zero
    at n - 3 of every row), and rows 0, 1 and the last equal what the single-row entry gives for them"""
    f = o.FIELDS[field]
    one = lim(f, 1)
    zero_at = [r * n + n - 3 for r in range(rows)] if n >= 3 else []
    a = with_edges(synth.field_elements(0x5C30 + rows, rows * n), rows + n, field, zero_at=zero_at).reshape(rows, n, 4)
    d = to_dev(a)
    out = torch.empty((rows, n, 4), dtype=torch.int64, device="cuda")
    prefix_product_rows_dev(field, d, out, n, rows)
    z = to_host(out).reshape(rows, n, 4)
    bad = first_bad(z[:, 0] == one)
    assert bad is None, {"row": bad, "index": 0}
    step = cpu_ref.field_op(field, "mul", z, a).reshape(rows, n, 4)  # z[r][i] a[r][i] == z[r][i + 1] within a row
    bad = first_bad(step[:, :-1] == z[:, 1:])
    assert bad is None, dict(scan_where(bad % (n - 1) + 1, n), row=bad // (n - 1))
    if n == 2:
        assert (z[:, 1] == a[:, 0]).all()
    single = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    for r in sorted({0, 1, rows - 1}):
        api.prefix_product_dev(field, d[r], single, n)
        bad = first_bad(to_host(single) == z[r])
        assert bad is None, dict(scan_where(bad, n), row=r)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n", [4097, 1 << 20, (1 << 20) + 1])
def test_kate_division_sizes(field, n):
    """multiopen.KateDivider (a z^i, prefix sum, total - P[i], z^-i) against the Rust loop q[n-2] = a[n-1], q[i-1] = a[i] + z q[i],
    vectorised and in full.  z = 0 has no inverse powers: KateDivider divides by X with a shift, which satisfies the same recurrence."""
    from tiny_ram_halo2_amd import multiopen
    f = o.FIELDS[field]
    a = with_edges(synth.field_elements(0x5C40 + n, n), n + 2, field, zeros=True)
    d = to_dev(a)
    z_rand = f.from_limbs(synth.field_elements(0x5C41 + n, 1)[0])
    for z in (z_rand, 1, f.m - 1, 0):
        q = to_host(multiopen.KateDivider(field, n, z, d.device).divide(d))
        assert q.shape == (n - 1, 4)
        assert (q[n - 2] == a[n - 1]).all(), z
        want = cpu_ref.field_op(field, "add", a[1:n - 1], cpu_ref.field_op(field, "mul", np.tile(lim(f, z), (n - 2, 1)), q[1:]))
        bad = first_bad(q[:-1] == want)
        # q[bad] is made from the prefix sum P[bad + 1] and the total, P[n - 1] + t[n - 1]: either may be the wrong one
        assert bad is None, {"quotient_index": bad, "z": z, "prefix_sum": scan_where(bad + 1, n), "total": scan_where(n - 1, n)}
        assert f.from_limbs(q[n - 3]) == (f.from_limbs(a[n - 2]) + z * f.from_limbs(a[n - 1])) % f.m  # big ints, no oracle


@pytest.mark.parametrize("field", FIELDS)
def test_powers_past_bit_12(field):
    """trh_field_powers_dev at n = 2^20 + 1: out[0] = 1 and out[i + 1] = out[i] x in full (bits 0 .. 20 of the index are walked), and
    x^(2^20) as a big int.  The bit loop of powers_kernel stops at bit 32: n >= 2^32 is outside what it can do and is not tested."""
    f = o.FIELDS[field]
    n = (1 << 20) + 1
    one = lim(f, 1)
    bases = [("random", synth.field_elements(0x5C50, 1)[0]), ("1", one), ("m-1", lim(f, f.m - 1)), ("0", np.zeros(4, np.uint64)),
             ("stored m-1", synth.ints_to_limbs([f.m - 1])[0])]
    out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    for name, x in bases:
        api.powers_dev(field, out, n, x)
        p = to_host(out)
        assert (p[0] == one).all(), name
        bad = first_bad(cpu_ref.field_op(field, "mul", p[:-1], np.tile(x, (n - 1, 1))) == p[1:])
        assert bad is None, (name, bad + 1)
        assert f.from_limbs(p[1 << 20]) == pow(f.from_limbs(x), 1 << 20, f.m), name


# ipa.hip inner_product_t: blocks = min(ceil(n / 256), IP_BLOCK_CAP) workgroups of 256 threads in a grid-stride loop, one partial per
# workgroup, summed by one workgroup of 256 threads.  Every thread makes one trip up to n = 1024 * 256 = 2^18; the partials exceed 256
# from n = 256 * 256 + 1 on (257: the second trip of sum_partials_kernel has one), and are 1024 (four full trips) from 2^18 on.
# IP_BLOCK_CAP copies the literal of `if (blocks > 1024) blocks = 1024;` in inner_product_t (csrc/ipa.hip): if that line changes, so must this.
IP_BLOCK_CAP = 1024
IP_SIZES = [256 * 256 + 1, IP_BLOCK_CAP * 256, IP_BLOCK_CAP * 256 + 1, 2 * IP_BLOCK_CAP * 256 + 12345]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n", IP_SIZES)
def test_inner_product_sized_to_block_cap(field, n):
    """compute_inner_product: one trip per thread at the cap, one element more, and three trips with a ragged last one; reference: the
    oracle's element-wise products, summed as Python ints"""
    f = o.FIELDS[field]
    a = with_edges(synth.field_elements(0x5C60 + n, n), n, field, zeros=True)
    b = with_edges(synth.field_elements(0x5C61 + n, n), n + 3, field, zeros=True)
    got = api.inner_product_dev(field, to_dev(a), to_dev(b), n)
    assert stored_ints(got[None]) == [sum(stored_ints(cpu_ref.field_op(field, "mul", a, b))) % f.m]


# ipa.hip eval_batch_t: blocks = min(ceil(n / 2048), EVAL_BLOCK_CAP) workgroups of 256 threads per polynomial, grid-stride.  Every
# thread makes one trip only up to n = 256 (one workgroup); up to the cap, n = 64 * 2048, a thread makes at most eight; past it the
# trips grow with n.  The partials per polynomial are at most 64, so sum_partials_batch_kernel never takes a second trip.
# EVAL_BLOCK_CAP and the 2048 copy the literals of `blocks = (n + 2047) / 2048; if (blocks > 64) blocks = 64;` in eval_batch_t
# (csrc/ipa.hip): if those lines change, so must these.
EVAL_BLOCK_CAP = 64
EVAL_SIZES = [256, 257, EVAL_BLOCK_CAP * 2048, EVAL_BLOCK_CAP * 2048 + 1, (1 << 20) + 4099]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n", EVAL_SIZES)
def test_poly_eval_batch_sized_to_block_cap(field, n):
    """eval_polynomial of a batch of three: one trip per thread, one element more, eight trips at the block cap, nine just past it,
    and 64 trips with a ragged 65th; reference: the oracle's Horner loop, and big-int Horner at the smallest size"""
    f = o.FIELDS[field]
    batch = 3
    polys = with_edges(synth.field_elements(0x5C70 + n, batch * n), n, field, zeros=True).reshape(batch, n, 4)
    d = to_dev(polys)
    for x in (synth.field_elements(0x5C71 + n, 1)[0], synth.ints_to_limbs([f.m - 1])[0]):
        got = api.poly_eval_batch_dev(field, d, n, batch, x)
        for b in range(batch):
            assert (got[b] == cpu_ref.eval_polynomial(field, polys[b], x)).all(), b
        if n == EVAL_SIZES[0]:
            xv, acc = f.from_limbs(x), 0
            for cf in reversed([f.from_limbs(r) for r in polys[batch - 1]]):
                acc = (acc * xv + cf) % f.m
            assert f.from_limbs(got[batch - 1]) == acc


@pytest.mark.parametrize("field", FIELDS)
def test_batch_invert_edge_residues(field):
    """ff::BatchInvert on edge residues, plain and with the fused numerator: zeros (from the residues and at every 97th index) stay
    zero, inv a == 1 elsewhere, and both forms equal the oracle's inversion"""
    f = o.FIELDS[field]
    n = 256 * 64 + 1  # one full workgroup of 64-element chunks and one element
    a = with_edges(synth.field_elements(0x5C80, n), 0x80, field, zeros=True, zero_at=range(0, n, 97))
    num = with_edges(synth.field_elements(0x5C81, n), 0x81, field, zeros=True)
    nz = a.any(axis=1)
    assert 170 < int((~nz).sum()) < 220
    want = np.zeros_like(a)
    want[nz] = cpu_ref.field_op(field, "inv", a[nz])
    d = to_dev(a)
    api.batch_invert_dev(field, d, n)
    got = to_host(d)
    assert not got[~nz].any()
    assert (cpu_ref.field_op(field, "mul", got[nz], a[nz]) == lim(f, 1)).all()
    assert (got == want).all()
    d = to_dev(a)
    api.batch_invert_mul_dev(field, d, to_dev(num), n)
    assert (to_host(d) == cpu_ref.field_op(field, "mul", want, num)).all()
