"""GPU tests (-m gpu) of the domain transforms (csrc/domain.hip) on batches that the lazy NTT passes (csrc/ntt.hip ntt_device_t) run as
several launch sets: hostplan::ntt_lazy_chunk transforms at a time -- 2 GiB of raw scratch at 72 B per element, whole polynomials
(a multiple of the block count) for the coset-block form.  With an NttFusion the loop moves the fused input pointer by `row0` rows per
set, rounds the set to the block count (the kernel takes the block as index % blocks inside a launch), raises it to one polynomial
when fewer transforms would fit, and runs a last set of fewer than 8 transforms on the plain grid instead of the batch-major one.

Every case calls the entry ONCE on the whole batch (distinct random polynomials made on the device) and then compares, bit for bit,
  (a) every polynomial with the same entry called on slices of at most half a launch set (those run as one set with offset 0, the form the
      tests of tests/test_gpu_poly.py pin to the oracle), on the device;
  (b) the polynomials on both sides of every set boundary, the first and the last with cpu_ref.EvaluationDomain.

Sizes: hostplan::ntt_plan_passes gives one pass of log_n stages up to log_n = NTT_TILE_LOG = 11 (ntt_can_fuse is false there, nothing is
fused and nothing is chunked) and ceil(log_n / 9) >= 2 lazy passes from 12, so 2^12 is the smallest transform with the loop under test.

trh_domain_blocks_to_quotient runs j - 1 <= 8 transforms in one call: below k = 23 that is never more than one set, so it is not here.

Last, the single-pass path (log_n <= 11) on 65537 transforms, one more than 2^16 in the grid's second dimension."""
import time

import numpy as np
import pytest
import torch

import cpu_ref
import pasta as o
from tiny_ram_halo2_amd import api, poly

pytestmark = pytest.mark.gpu

SCRATCH, RAW_BYTES = 2 << 30, 72   # csrc/hostplan.h: NTT_MAX_SCRATCH, two raw planes of NTT_RAW_BYTES per element
ORACLE_THREADS = min(cpu_ref.hardware_threads(), 16)


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield
    _release()


def _release():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    api._check(api.lib().trh_pool_trim())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def random_elements(seed, *shape):
    """(*shape, 4) int64 on the device: uniform 64-bit words, the top word cut to 62 bits -- values below 2^254, under both moduli, so
    every row is a canonical stored word; one generator call, every row distinct (a repeat has probability ~ rows^2 / 2^254)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randint(-(1 << 63), (1 << 63) - 1, shape + (4,), dtype=torch.int64, device="cuda", generator=g)
    a[..., 3] &= (1 << 62) - 1
    return a


def to_host(t):
    torch.cuda.synchronize()
    return t.contiguous().cpu().numpy().view(np.uint64)


def lazy_chunk(log_n, blocks):
    """the documented rule, restated (tests/native/hostplan_test.cpp checks hostplan::ntt_lazy_chunk without a device)"""
    chunk = max(SCRATCH // (RAW_BYTES << log_n), 1)
    if blocks:
        chunk = blocks if chunk < blocks else chunk - chunk % blocks
    return chunk


def expect_split(log_n, blocks, polys, chunk, splits):
    """the launch sets the case is built for follow from the rule: a change of the rule fails here, not by un-chunking the case"""
    per = blocks or 1
    assert lazy_chunk(log_n, blocks) == chunk and chunk % per == 0
    total, sets = polys * per, []
    for b0 in range(0, total, chunk):
        sets.append(min(chunk, total - b0))
    assert sets == splits and len(sets) >= 2, sets
    return chunk // per   # polynomials per set


def boundaries(c, batch):
    """first, last and both sides of every set boundary, in polynomials"""
    idx = {0, batch - 1}
    for b in range(c, batch, c):
        idx |= {b - 1, b}
    return sorted(idx)


def report(name, t0, **extra):
    torch.cuda.synchronize()
    print(f"\n[domain_chunks] {name}: {time.perf_counter() - t0:.2f} s" + "".join(f", {k} = {v}" for k, v in extra.items()))


@pytest.mark.parametrize("field,k,j,chunk,batch,splits", [
    ("fp", 12, 3, 7281, 7286, [7281, 5]),        # a last set below 8: the plain grid
    ("fq", 18, 6, 113, 235, [113, 113, 9]),      # three sets, the last one batch-major
])
def test_lagrange_to_coeff_in_several_sets(field, k, j, chunk, batch, splits):
    t0 = time.perf_counter()
    c = expect_split(k, 0, batch, chunk, splits)
    dom, cd = poly.EvaluationDomain(field, j, k), cpu_ref.EvaluationDomain(field, j, k, threads=ORACLE_THREADS)
    a = random_elements(0x1A60 + k, batch, 1 << k)
    got = dom.lagrange_to_coeff(a.clone())
    assert api.stat("ntt_tableless_passes") == 0
    step = c // 2
    for b0 in range(0, batch, step):
        assert torch.equal(got[b0:b0 + step], dom.lagrange_to_coeff(a[b0:b0 + step].clone())), b0
    idx = boundaries(c, batch)
    g, src = to_host(got[idx]), to_host(a[idx])
    for i, b in enumerate(idx):
        assert (g[i] == cd.lagrange_to_coeff(src[i])).all(), b
    del a, got
    _release()
    report(f"lagrange_to_coeff {field} k={k} batch={batch}", t0)


@pytest.mark.parametrize("field,k,j,chunk,batch,splits", [
    ("fq", 11, 3, 7281, 7290, [7281, 9]),
    ("fp", 18, 6, 14, 31, [14, 14, 3]),          # the reference's shape
])
def test_coeff_to_extended_in_several_sets(field, k, j, chunk, batch, splits):
    t0 = time.perf_counter()
    dom, cd = poly.EvaluationDomain(field, j, k), cpu_ref.EvaluationDomain(field, j, k, threads=ORACLE_THREADS)
    c = expect_split(dom.extended_k, 0, batch, chunk, splits)
    a = random_elements(0xC0E0 + k, batch, 1 << k)
    got = dom.coeff_to_extended(a)
    assert api.stat("ntt_tableless_passes") == 0
    step = c // 2
    for b0 in range(0, batch, step):
        assert torch.equal(got[b0:b0 + step], dom.coeff_to_extended(a[b0:b0 + step])), b0
    idx = boundaries(c, batch)
    g, src = to_host(got[idx]), to_host(a[idx])
    for i, b in enumerate(idx):
        assert (g[i] == cd.coeff_to_extended(src[i])).all(), b
    del a, got
    _release()
    report(f"coeff_to_extended {field} k={k} batch={batch}", t0)


def test_extended_to_coeff_in_several_sets():
    """random extended values in (every value is a valid input): the whole 2^extended_k output against the sliced calls, the truncated
    (j - 1) 2^k coefficients against the oracle"""
    field, k, j, chunk, batch, splits = "fp", 18, 6, 14, 17, [14, 3]
    t0 = time.perf_counter()
    dom, cd = poly.EvaluationDomain(field, j, k), cpu_ref.EvaluationDomain(field, j, k, threads=ORACLE_THREADS)
    c = expect_split(dom.extended_k, 0, batch, chunk, splits)
    a = random_elements(0xE7C0 + k, batch, dom.extended_len())
    got = a.clone()
    trunc = dom.extended_to_coeff(got)
    assert api.stat("ntt_tableless_passes") == 0
    assert trunc.shape == (batch, (j - 1) << k, 4)
    step = c // 2
    for b0 in range(0, batch, step):
        part = a[b0:b0 + step].clone()
        dom.extended_to_coeff(part)
        assert torch.equal(got[b0:b0 + step], part), b0
    idx = boundaries(c, batch)
    g, src = to_host(trunc[idx]), to_host(a[idx])
    for i, b in enumerate(idx):
        assert (g[i] == np.asarray(cd.extended_to_coeff(src[i])).reshape(-1, 4)).all(), b
    del a, got, trunc
    _release()
    report(f"extended_to_coeff {field} k={k} batch={batch}", t0)


@pytest.mark.parametrize("field,k,j,blocks,chunk,batch,splits", [
    ("fp", 18, 6, 5, 110, 32, [110, 50]),        # the replay's batch
    ("fp", 18, 6, 8, 112, 31, [112, 112, 24]),
    ("fq", 18, 6, 3, 111, 40, [111, 9]),
    ("fq", 12, 6, 5, 7280, 1460, [7280, 20]),
])
def test_coeff_to_extended_blocks_in_several_sets(field, k, j, blocks, chunk, batch, splits):
    t0 = time.perf_counter()
    dom, cd = poly.EvaluationDomain(field, j, k), cpu_ref.EvaluationDomain(field, j, k, threads=ORACLE_THREADS)
    c = expect_split(k, blocks, batch, chunk, splits)
    stride = 1 << (dom.extended_k - k)
    a = random_elements(0xB10C + 16 * k + blocks, batch, 1 << k)
    got = dom.coeff_to_extended_blocks(a, blocks)
    assert api.stat("ntt_tableless_passes") == 0
    assert got.shape == (batch, blocks, 1 << k, 4)
    step = c // 2   # polynomials: step * blocks <= chunk / 2 transforms
    assert 1 <= step and step * blocks <= chunk // 2
    for b0 in range(0, batch, step):
        assert torch.equal(got[b0:b0 + step], dom.coeff_to_extended_blocks(a[b0:b0 + step], blocks)), b0
    idx = boundaries(c, batch)
    g, src = to_host(got[idx]), to_host(a[idx])
    for i, b in enumerate(idx):
        want = np.asarray(cd.coeff_to_extended(src[i])).reshape(-1, 4)
        for r in range(blocks):
            assert (g[i, r] == want[r::stride]).all(), (b, r)
    del a, got
    _release()
    report(f"coeff_to_extended_blocks {field} k={k} blocks={blocks} batch={batch}", t0)


def test_coeff_to_extended_blocks_set_raised_to_one_polynomial():
    """2^22 with 8 blocks: 7 transforms fit the scratch, the set is raised to the 8 of one polynomial -- 3 polynomials run as 8 + 8 + 8.
    The oracle's 2^25 transform is out of a unit test's reach: (a) against three calls of one polynomial each (exactly one set, the form
    the k = 18 case pins); (b) four entries (q, r) of every polynomial, blocks 0 and 7 among them, against an independent kernel: entry q of
    block r is the polynomial's value at zeta * extended_omega^(8 q + r) (api.poly_eval_batch_dev, which tests/test_gpu_poly.py pins to
    big integers), the point computed with Python integers"""
    field, k, j, blocks, chunk, batch, splits = "fp", 22, 6, 8, 8, 3, [8, 8, 8]
    t0 = time.perf_counter()
    f = o.FIELDS[field]
    assert SCRATCH // (RAW_BYTES << k) == 7   # fewer than the 8 blocks of one polynomial
    dom = poly.EvaluationDomain(field, j, k)
    assert expect_split(k, blocks, batch, chunk, splits) == 1 and dom.extended_k == 25
    n = 1 << k
    a = random_elements(0xB10C22, batch, n)
    got = dom.coeff_to_extended_blocks(a, blocks)
    assert api.stat("ntt_tableless_passes") == 0
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()   # everything the call needed is still held: input, output, tables, scratch
    for b in range(batch):
        one = dom.coeff_to_extended_blocks(a[b:b + 1], blocks)
        assert torch.equal(got[b:b + 1], one), b
        del one
    cdom = o.EvaluationDomain(f, j, k)
    assert cdom.extended_k == 25
    for q, r in ((0, 0), (n - 1, 7), (0x2B5A17, 3), (n // 2 + 1, 0)):
        x = cdom.g_coset * pow(cdom.extended_omega, 8 * q + r, f.m) % f.m
        want = api.poly_eval_batch_dev(field, a, n, batch, np.array(f.limbs(x), np.uint64), stream=_stream())
        assert (to_host(got[:, r, q]) == want).all(), (q, r)
    del a, got
    _release()
    report(f"coeff_to_extended_blocks {field} k={k} blocks={blocks} batch={batch}", t0, device_memory_in_use_GiB=round((total - free) / 2**30, 2))


@pytest.mark.parametrize("field", ["fp", "fq"])
@pytest.mark.parametrize("log_n", [3, 10])
def test_ntt_single_pass_batch_beyond_one_grid_dimension(field, log_n):
    """log_n <= 11 is one pass that hands the batch to the grid's second dimension as it is; 65537 transforms are past the 65535 the lazy
    path's batch-major condition treats as that dimension's limit.  The runtime takes the launch (no error return) and every transform is
    there: each against calls of 4096, transforms 0, 65535 and 65536 (either side of 2^16) against the oracle.  Should a runtime refuse such
    a launch, ntt_device_t has to loop over launches of at most 65535 transforms, and this test pins that too"""
    t0 = time.perf_counter()
    f = o.FIELDS[field]
    n, batch, step = 1 << log_n, 65537, 4096
    w = np.array(f.limbs(f.omega(log_n)), np.uint64)
    a = random_elements(0x65537 + log_n, batch, n)
    got = a.clone()
    api.ntt_dev(field, got, log_n, w, batch=batch, stream=_stream())
    for b0 in range(0, batch, step):
        part = a[b0:b0 + step].clone()
        api.ntt_dev(field, part, log_n, w, batch=part.shape[0], stream=_stream())
        assert torch.equal(got[b0:b0 + step], part), b0
    idx = [0, 65535, 65536]
    g, src = to_host(got[idx]), to_host(a[idx])
    for i, b in enumerate(idx):
        assert (g[i] == cpu_ref.best_fft(field, src[i], w, log_n, threads=4)).all(), b
    del a, got
    _release()
    report(f"ntt {field} log_n={log_n} batch={batch}", t0)
