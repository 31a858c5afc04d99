"""GPU tests (-m gpu) of trh_product_chain_dev (csrc/scan.hip; permutation.chain_products): the link between the product columns of consecutive
permutation sets, z_s[0] = z_(s-1)[u], against Python integers, word for word.

With z_in the rows on entry, row r >= 1 becomes z_in[r][i] * c_r, c_r = prod_{t < r} z_in[t][link]; row 0 stays.  In stored (Montgomery) words
a product is a * b * R^-1 mod m, which is all the reference below uses.

  shapes     rows 1, 2, 3 (a carry of a carry), 47 (the reference's sets), 65 and 257 (past one wave and one workgroup of rows in the carry
             launch, whose threads then own two rows each); n = 2^5 (several rows per workgroup of the pass) and 2^12 (several workgroups per
             row); link 0, the usable rows, n - 1
  words      inputs hold the stored words random data never produces (common.with_edges: m - 1, [2^254, m), R, ...)
  zero       a zero at `link` of a middle row: every later row is zero, the rows up to it are not
  bounds     rows behind `rows` and the bytes behind the buffer stay as they were; rows = 0 and 1 do nothing
  refusals   unknown id, link >= n, n no power of two, null z
  stream     the rows written on a non-blocking stream, no synchronisation before the call"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import pasta as o
from common import stored_ints, with_edges
from tiny_ram_halo2_amd import api, permutation, synth

FIELDS = ["fp", "fq"]
BLINDING = 5  # usable rows = n - (blinding_factors + 1)


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def to_host(t):
    torch.cuda.synchronize()
    return t.contiguous().cpu().numpy().view(np.uint64)


def chained(field, rows_in, link):
    """the definition on stored words: rows_in = list of lists of ints -> the chained rows"""
    f = o.FIELDS[field]
    rinv = pow(f.R, -1, f.m)
    carry, out = f.R % f.m, []  # the stored form of one
    for r, row in enumerate(rows_in):
        out.append(list(row) if r == 0 else [v * carry % f.m * rinv % f.m for v in row])
        carry = carry * row[link] % f.m * rinv % f.m
    return out


def make_rows(field, rows, n, seed, zero_at=()):
    return with_edges(synth.field_elements(seed, max(rows, 1) * n), seed, field, zero_at=zero_at)[: rows * n].reshape(rows, n, 4)


def call(field, z, n, rows, link, stream=None):
    a = api.ProductChainArgs(z=None if z is None else api._devptr(z), n=n, rows=rows, link=link, stream=stream)
    return api.lib().trh_product_chain_dev(api.FIELD_ID[field], ctypes.byref(a))


@pytest.mark.parametrize("n", [1 << 5, 1 << 12])
@pytest.mark.parametrize("rows", [1, 2, 3, 47, 65, 257])
@pytest.mark.parametrize("field", FIELDS)
def test_against_integers(field, rows, n):
    a = make_rows(field, rows, n, 0xC4A1 + rows + n)
    ints = [stored_ints(a[r]) for r in range(rows)]
    for link in (0, n - (BLINDING + 1), n - 1):
        d = to_dev(a)
        assert permutation.chain_products(field, d, link) is d
        got = to_host(d).reshape(rows, n, 4)
        want = chained(field, ints, link)
        for r in range(rows):
            assert stored_ints(got[r]) == want[r], {"row": r, "link": link}
        assert (got[0] == a[0]).all()


@pytest.mark.parametrize("field", FIELDS)
def test_a_zero_at_the_link_of_a_middle_row(field):
    rows, n, link, at = 9, 1 << 5, 26, 4
    a = make_rows(field, rows, n, 0xC4A2, zero_at=(at * n + link,))
    d = to_dev(a)
    permutation.chain_products(field, d, link)
    got = to_host(d).reshape(rows, n, 4)
    want = chained(field, [stored_ints(a[r]) for r in range(rows)], link)
    for r in range(rows):
        assert stored_ints(got[r]) == want[r], r
    assert all(got[r].any(axis=1).sum() == n - (r == at) for r in range(at + 1)), "the rows up to the zero keep their values"
    assert not got[at + 1:].any(), "every row behind the zero link is zero"


@pytest.mark.parametrize("field", FIELDS)
def test_rows_behind_the_chain_and_the_bytes_behind_the_buffer_stay(field):
    """the chain covers the leading `rows` rows of a larger buffer (the lookup products follow the permutation sets in one allocation)"""
    total, rows, n, link = 8, 5, 1 << 5, 26
    a = make_rows(field, total, n, 0xC4A3)
    d = to_dev(a)
    permutation.chain_products(field, d, link, rows=rows)
    got = to_host(d).reshape(total, n, 4)
    want = chained(field, [stored_ints(a[r]) for r in range(rows)], link)
    for r in range(rows):
        assert stored_ints(got[r]) == want[r], r
    assert (got[rows:] == a[rows:]).all()
    # a window inside the buffer: the rows in front of it stay too
    d = to_dev(a)
    assert call(field, d[2:], n, 3, link) == 0
    got = to_host(d).reshape(total, n, 4)
    want = chained(field, [stored_ints(a[r]) for r in range(2, 5)], link)
    assert (got[:3] == a[:3]).all() and (got[5:] == a[5:]).all()
    for r in range(3):
        assert stored_ints(got[2 + r]) == want[r], r
    for rows in (0, 1):
        d = to_dev(a)
        assert call(field, d, n, rows, link) == 0
        assert (to_host(d).reshape(total, n, 4) == a).all()
    assert call(field, None, n, 0, link) == 0  # nothing is read


def test_refusals():
    lib = api.lib()
    n = 1 << 5
    a = make_rows("fp", 3, n, 0xC4A4)
    d = to_dev(a)

    def refused(rc, text):
        assert rc == -1 and text in lib.trh_last_error().decode(), (rc, lib.trh_last_error())

    refused(call_id(7, d, n, 3, 0), "unknown field id 7")
    assert lib.trh_last_error().decode() == "unknown field id 7"
    refused(call_id(-1, d, n, 0, 0), "unknown field id -1")
    refused(call("fp", d, n, 3, n), "link")
    refused(call("fp", d, 24, 3, 0), "power of two")
    refused(call("fp", None, n, 3, 0), "null")
    assert lib.trh_product_chain_dev(0, None) == -1
    assert (to_host(d).reshape(3, n, 4) == a).all()
    assert call("fp", d, n, 3, 0) == 0  # the context stays usable
    torch.cuda.synchronize()


def call_id(field_id, z, n, rows, link):
    a = api.ProductChainArgs(z=None if z is None else api._devptr(z), n=n, rows=rows, link=link, stream=None)
    return api.lib().trh_product_chain_dev(field_id, ctypes.byref(a))


@pytest.mark.parametrize("field", FIELDS)
def test_on_a_non_blocking_stream(field):
    """the rows arrive on a torch stream (non-blocking: nothing orders it behind the null stream) behind a delay; the call follows without a
    synchronisation, and a second call on another stream continues from the first one's result"""
    rows, n, link = 47, 1 << 12, (1 << 12) - 6
    a = make_rows(field, rows, n, 0xC4A5)
    ints = [stored_ints(a[r]) for r in range(rows)]
    once = chained(field, ints, link)
    twice = chained(field, once, link)
    real = to_dev(a)
    bufs = [torch.full_like(real, 0x0101010101010101) for _ in range(2)]  # what a call that does not wait for the stream would read
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        torch.cuda._sleep(2_000_000)
        bufs[0].copy_(real, non_blocking=True)
        permutation.chain_products(field, bufs[0], link)
    got = to_host(bufs[0]).reshape(rows, n, 4)
    for r in range(rows):
        assert stored_ints(got[r]) == once[r], r
    with torch.cuda.stream(s1):
        torch.cuda._sleep(2_000_000)
        bufs[1].copy_(real, non_blocking=True)
        permutation.chain_products(field, bufs[1], link)
    with torch.cuda.stream(s2):
        permutation.chain_products(field, bufs[1], link)  # ordered behind the context's previous call, whatever stream that used
    got = to_host(bufs[1]).reshape(rows, n, 4)
    for r in range(rows):
        assert stored_ints(got[r]) == twice[r], r
