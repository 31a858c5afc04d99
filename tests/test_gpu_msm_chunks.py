"""Batched MSMs past one launch set (csrc/msm.hip enqueue_pipeline's chunk loop: `chunk` items at a time through one set of launches,
blockIdx.z = item; hostplan::msm_plan caps the chunk at 64 items and at option msm_chunk_gb), plain and over a fixed-base table.

What a second chunk relies on: every offset by b0 (scalars, blinds, window sums, the dense runs and the unit path's final sums of
sparse_chunk), the reuse of ONE scratch set by a full chunk and a shorter one behind it (heavy lists, bucket counters, oversize flags,
the sparse counters and lists), size_segments deciding per chunk (at c = 8 a chunk of 64 keeps the plan's segments, a last chunk of 32
fills the 4 KiB read-back area to its last byte, 33 is one item over), the fused zeroing meeting a second chunk (batch < 8 under a
small budget) and msm_finish_t on both sides of its 256-item Horner split.

Bases are P_i = (s0 + i d) G, so every expected point is one scalar multiplication of G by the exact weighted sum of the item's
scalars; the first, last and two middle items of every chunk also go through the oracle's best_multiexp over the downloaded bases.
Comparisons are limb for limb.  Every item of a batch is different, so a wrong b0 shows as another item's point; every batch holds an
all-zero item and an item whose scalars are all equal.  trh_stat "msm_chunks" / "msm_unit_chunks" prove that the path under test ran;
the expected counts are pinned without a device by the "chunk shapes" rows of tests/native/hostplan_test.cpp."""
import numpy as np
import pytest

import cpu_ref
import msm_chunk_cases as C
import pasta as o
from common import point_hex, run_with_options
from tiny_ram_halo2_amd import api, replay, synth

pytestmark = pytest.mark.gpu

CURVES = ["pallas", "vesta"]
S0, D = synth.BASE_S0, synth.BASE_D
CHUNK = C.CHUNK


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


def _mont(curve, can):
    return cpu_ref.field_op(api.SCALAR_FIELD[curve], "to_mont", np.ascontiguousarray(can).reshape(-1, 4)).reshape(can.shape)


def _expected(curve, can):
    """the closed form: (sum_i scalar_i (s0 + i d) mod q) G as the entry returns a point (affine, z = 1; all zero: the identity)"""
    cv = o.CURVES[curve]
    total = synth.weighted_scalar_sum(can, S0, D) % cv.scalar.m
    want = np.zeros(12, dtype=np.uint64)
    if total:
        g = np.array(cv.affine_limbs(cv.generator), dtype=np.uint64)
        want[:8] = cpu_ref.to_affine(curve, cpu_ref.scalar_mul(curve, g, np.array(o.int_to_limbs(total), np.uint64)))
        want[8:] = np.array(cv.base.limbs(1), np.uint64)
    return want


def _where(i, chunk):
    return f"item {i} (chunk {i // chunk}, position {i % chunk})"


def _oracle_picks(batch, chunk):
    """first, last and two middle items of every chunk"""
    picks = set()
    for b0 in range(0, batch, chunk):
        nb = min(chunk, batch - b0)
        picks |= {b0, b0 + nb // 3, b0 + (2 * nb) // 3, b0 + nb - 1}
    return sorted(picks)


def _check(curve, got, want, chunk, what, order=None):
    """got[j] against want[order[j]]; a failure names the item, its chunk and its position in the chunk, and -- when the point is
    another item's -- whose"""
    order = range(len(got)) if order is None else order
    for j, i in enumerate(order):
        if (np.asarray(got[j]) == want[i]).all():
            continue
        others = [k for k in range(len(want)) if (np.asarray(got[j]) == want[k]).all()]
        raise AssertionError(f"{curve} {what}: {_where(j, chunk)} is wrong" + (f"; it is the point of item(s) {others} of the batch as built" if others else ""))


def _check_oracle(curve, want, mont, xy, picks, chunk, what):
    th = cpu_ref.hardware_threads()
    for i in picks:
        ref = cpu_ref.to_affine(curve, cpu_ref.best_multiexp(curve, mont[i], xy, threads=th))
        assert (ref == want[i][:8]).all(), f"{curve} {what}: the oracle's best_multiexp disagrees with the closed form on {_where(i, chunk)}"


# ---- a. more than 64 items, no table ----------------------------------------------------------------------------------------------------
_PLAIN_BASES = {}


@pytest.fixture(scope="module")
def plain_bases():
    def get(curve, n):
        if (curve, n) not in _PLAIN_BASES:
            b = api.Bases.generate(curve, S0, D, n)
            _PLAIN_BASES[(curve, n)] = (b, b.download())
        return _PLAIN_BASES[(curve, n)]
    yield get
    for b, _ in _PLAIN_BASES.values():
        b.destroy()
    _PLAIN_BASES.clear()


def _run_batch(bases, mont, chunks):
    """the batch through trh_msm_batch_dev; asserts the launch sets it ran as"""
    batch, n = mont.shape[0], mont.shape[1]
    d = api.DeviceBuffer.from_host(mont)
    try:
        before = api.stat("msm_chunks")
        got = bases.msm_batch_dev(d, n, batch)
        assert api.stat("msm_chunks") - before == chunks, (batch, chunks)
    finally:
        d.free()
    return got


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n,c,batch", [(1500, 8, 65), (1500, 8, 96), (1500, 8, 97), (1500, 8, 129), (300, 4, 256), (300, 4, 257)])
def test_plain_batches_past_one_chunk(plain_bases, curve, n, c, batch):
    """skewed items (heavy lists) in the first chunk, sparse ones in the last, then the reverse; then the last chunk's items as a batch
    of their own and one by one on the same bases and context: the same points.  Last chunks of 1, 32, 33 and 64 items: with and without
    the read-back of the entry totals behind a chunk that kept the plan's segments; 256 / 257 items: both forms of msm_finish_t"""
    bases, xy = plain_bases(curve, n)
    can = C.plain_items(0xA11 + (curve == "vesta"), n, c, batch)
    chunks = (batch + CHUNK - 1) // CHUNK
    assert not can[batch - 2].any() and (can[0] == can[0, 0]).all()
    mont = _mont(curve, can)
    want = [_expected(curve, can[i]) for i in range(batch)]
    assert not want[batch - 2].any() and len({point_hex(w) for w in want}) == batch
    _check_oracle(curve, want, mont, xy, _oracle_picks(batch, CHUNK), CHUNK, f"n = {n}, batch {batch}")
    fwd = _run_batch(bases, mont, chunks)
    _check(curve, fwd, want, CHUNK, f"n = {n}, batch {batch}")
    rev = list(range(batch))[::-1]
    _check(curve, _run_batch(bases, mont[rev], chunks), want, CHUNK, f"n = {n}, batch {batch} reversed", rev)
    # the last chunk's items alone: one launch set of their own (up to four items: one launch, no launch set)
    last = list(range((chunks - 1) * CHUNK, batch))
    alone = _run_batch(bases, mont[last], 1 if len(last) > 4 else 0)
    _check(curve, alone, want, CHUNK, f"n = {n}, the last chunk of batch {batch} alone", last)
    d = api.DeviceBuffer.from_host(mont[last])
    try:
        for j, i in enumerate(last):
            lone = bases.msm_dev(d.ptr.value + j * n * 32, n)
            assert (lone == fwd[i]).all(), f"{curve} n = {n}, batch {batch}: {_where(i, CHUNK)} differs from the same scalars as a lone MSM"
    finally:
        d.free()


# ---- b. blinds past the first chunk, no table -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_commit_blinds_past_one_chunk(curve):
    """trh_commit_batch_dev over 1501 bases without a table: 70 columns (64 + 6) with 70 different blinds, then the blinds reversed under
    the same columns: every point moves by (blind difference) P_n.  Column 65 is all zero: its point is its blind times P_n and nothing else"""
    n, batch = 1500, 70
    cv = o.CURVES[curve]
    q, sf = cv.scalar.m, api.SCALAR_FIELD[curve]
    cols = np.zeros((batch, n, 4), dtype=np.uint64)
    for i in range(batch):
        rng = np.random.default_rng([0xB11D, int(curve == "vesta"), i])
        cols[i] = C.all_equal(rng, n) if i == 3 else C.uniform(rng, n)
    cols[65] = 0
    blinds = synth.field_elements(0xB1B + (curve == "vesta"), batch)   # Montgomery form as stored
    blinds_can = cpu_ref.field_op(sf, "from_mont", blinds)
    assert len({point_hex(b) for b in blinds}) == batch
    bases = api.Bases.generate(curve, S0, D, n + 1)
    d = api.DeviceBuffer.from_host(_mont(curve, cols))
    try:
        xy = bases.download()
        runs = []
        for bl, bl_can, what in ((blinds, blinds_can, "blinds in order"), (blinds[::-1].copy(), blinds_can[::-1].copy(), "blinds reversed")):
            before = api.stat("msm_chunks")
            got = bases.commit_batch_dev(d, n, batch, bl)
            assert api.stat("msm_chunks") - before == 2
            want = [_expected(curve, np.concatenate([cols[i], bl_can[i][None]])) for i in range(batch)]
            _check(curve, got, want, CHUNK, f"commit, {what}")
            runs.append((got, want))
        mont = np.concatenate([_mont(curve, cols), blinds[:, None]], axis=1)
        _check_oracle(curve, runs[0][1], mont, xy, _oracle_picks(batch, CHUNK), CHUNK, "commit")
        # the second run from the first: + (b'_i - b_i) P_n on the oracle's group law
        ints = synth.limbs_to_ints(blinds_can)
        for i in range(batch):
            delta = (ints[batch - 1 - i] - ints[i]) % q
            step = cpu_ref.scalar_mul(curve, xy[n], np.array(o.int_to_limbs(delta), np.uint64))
            moved = cpu_ref.to_affine(curve, cpu_ref.point_op(curve, "add", runs[0][0][i], step))
            assert (moved == runs[1][0][i][:8]).all(), f"{curve} commit: {_where(i, CHUNK)} did not move by its blind difference times P_n"
    finally:
        d.free()
        bases.destroy()


# ---- c. the budget cuts the chunk ---------------------------------------------------------------------------------------------------------
BUDGET_SCRIPT = r"""
import numpy as np, torch
import cpu_ref
import msm_chunk_cases as C
from common import point_hex
from tiny_ram_halo2_amd import api, synth
api.init(0)
assert api.get_option("msm_chunk_gb") == 1
for name in ("k18", "k20"):
    log_n, can = C.budget_items(name)
    n, batch = 1 << log_n, can.shape[0]
    bases = api.Bases.generate("pallas", synth.BASE_S0, synth.BASE_D, n)
    d = api.DeviceBuffer.from_host(cpu_ref.field_op("fq", "to_mont", can.reshape(-1, 4)))
    before = api.stat("msm_chunks")
    got = bases.msm_batch_dev(d, n, batch)
    print("chunks", name, api.stat("msm_chunks") - before)
    print("sorted", name, api.stat("msm_bin_sorted_windows"))
    for i in range(batch):
        print("point", name, i, point_hex(got[i]))
    d.free()
    bases.destroy()
"""


@pytest.fixture(scope="module")
def budget_child():
    """one child process under msm_chunk_gb = 1 (options are fixed while a context exists) for both shapes"""
    out = run_with_options(BUDGET_SCRIPT, {"TRH_MSM_CHUNK_GB": "1"})
    res = {}
    for line in out.splitlines():
        f = line.split()
        if f and f[0] in ("chunks", "sorted"):
            res[(f[0], f[1])] = int(f[2])
        elif f and f[0] == "point":
            res[("point", f[1], int(f[2]))] = f[3]
    return res


@pytest.mark.parametrize("name", ["k18", "k20"])
def test_budget_cuts_the_chunk(budget_child, name):
    """2^18 x 20 runs as 18 + 2 under one GiB (adaptive: the entry totals of both chunks are read back); 2^20 x 6 as 5 + 1: a batch below 8,
    so the fused zeroing meets a second chunk, on the shape that takes the LDS bin sort -- item 4 has window 0's bin 0 one entry over the
    LDS capacity and item 5, alone in the second chunk, exactly at it: all but the short top window of item 5 must be sorted in the LDS
    (a stale oversize flag or bin counter of chunk 0 would send window 0 to the chunked passes).  The child's points, this process's
    one-chunk run of the same scalars and the closed form agree"""
    curve = "pallas"
    log_n, can = C.budget_items(name)
    n, batch = 1 << log_n, can.shape[0]
    per, chunks = C.BUDGET_CHUNKS[name]
    assert (batch + per - 1) // per == chunks and batch > per
    assert sum(1 for i in range(batch) if not can[i].any()) == 1 and sum(1 for i in range(batch) if can[i].any() and (can[i] == can[i, 0]).all()) == 1
    want = [_expected(curve, can[i]) for i in range(batch)]
    assert len({point_hex(w) for w in want}) == batch
    bases = api.Bases.generate(curve, S0, D, n)
    d = api.DeviceBuffer.from_host(_mont(curve, can))
    try:
        before = api.stat("msm_chunks")
        got = bases.msm_batch_dev(d, n, batch)
        assert api.stat("msm_chunks") - before == 1
        th = cpu_ref.hardware_threads()
        xy = bases.download()
        for i in sorted({0, per - 1, per, batch - 1}):   # both sides of the cut
            ref = cpu_ref.to_affine(curve, cpu_ref.best_multiexp(curve, _mont(curve, can[i]), xy, threads=th))
            assert (ref == want[i][:8]).all(), f"{name}: the oracle's best_multiexp disagrees with the closed form on {_where(i, per)}"
    finally:
        d.free()
        bases.destroy()
    _check(curve, got, want, batch, f"{name}, one chunk")
    assert budget_child[("chunks", name)] == chunks
    child = [np.array([int(budget_child[("point", name, i)][16 * k:16 * k + 16], 16) for k in range(12)], dtype=np.uint64) for i in range(batch)]
    _check(curve, child, want, per, f"{name}, msm_chunk_gb = 1")
    if name == "k20":   # the last chunk is item 5 alone: every window but the top one in the LDS
        assert budget_child[("sorted", name)] == C.S.lds_windows(C.S.BIN_CAP) == 15
    else:
        assert budget_child[("sorted", name)] == 0   # 2^18: no LDS bin sort


# ---- d. the fixed-base sparse path past one chunk ---------------------------------------------------------------------------------------------
K, N = 14, 1 << 14
FB_C = 12   # the table trh_bases_precompute(0) attaches to 2^14 + 1 bases
_TABLED = {}


@pytest.fixture(scope="module")
def tabled_bases():
    def get(curve):
        if curve not in _TABLED:
            b = api.Bases.generate(curve, S0, D, N + 1)
            assert b.precompute(0) == FB_C
            _TABLED[curve] = (b, b.download())
        return _TABLED[curve]
    yield get
    for b, _ in _TABLED.values():
        b.destroy()
    _TABLED.clear()


def _full_size(seed, count):
    return cpu_ref.field_op("fp", "from_mont", synth.field_elements(seed, count))  # uniformly random canonical values (either field: < 2^254)


def _with_hidden(col, count, seed):
    """`count` full-size scalars (about 21 digits each that are not +-1) on rows the sampler does not read (it reads every 16th row): the
    column still votes for the unit path; its class follows its real digit count -- tiny up to 256 entries, general above"""
    col = col.copy()
    rows = 16 * np.random.default_rng(seed).choice(N // 16, size=count, replace=False) + 5
    col[rows] = _full_size(seed, count)
    return col


def _sparse_orders():
    """name -> (70 columns, (chunk 0 votes, chunk 1 votes)).  The vote is msm_sparse_sample_kernel's: a column votes for the unit path when
    its sampled rows show nothing but 0 / +-1 digits OR when it is dense (a full-size column is: ~21 digits on each of 1024 sampled rows
    times the step of 16 is far above twice the list capacity); a word column shows three 12-bit digits per live row, is not dense and does
    NOT vote.  sparse_chunk sends a chunk whose vote is not unanimous through the plain pipeline, so `msm_unit_chunks` counts exactly the
    unanimous chunks (the vote is read again after the emit, which does not change it)."""
    flags = replay.witness_columns("flag", True, 0xF1A6, 72, N, 32)
    full = replay.witness_columns("full", True, 0xF011, 5, N, 32)
    word = replay.witness_columns("word", True, 0x30FD, 1, N, 32)[0]
    zero = np.zeros((N, 4), dtype=np.uint64)
    ones = zero.copy(); ones[:, 0] = 1
    general = _with_hidden(flags[64], 17, 0x6E2)   # 17 x ~21 digits: above the tiny limit of 256
    tiny = _with_hidden(flags[65], 3, 0x717)
    flag_chunk = [flags[i] for i in range(64)]
    flag_chunk[9], flag_chunk[20] = zero, ones     # the all-zero item and the item whose scalars are all equal
    tail = [flags[66], full[0], full[1], word, general, full[2]]         # flag, full, full, word, general, full
    tail_unit = [flags[66], full[0], full[1], tiny, general, full[2]]    # the same with a tiny column for the word: the vote holds
    quiet = [flags[67], tiny, flags[68], zero, flags[69], _with_hidden(flags[70], 2, 0x718)]  # nothing for the pipeline
    one_full = list(flag_chunk); one_full[31] = full[3]
    one_word = list(flag_chunk); one_word[31] = word
    ones_chunk = [ones] * 64; ones_chunk[9] = zero
    return {
        # dense runs of 2 and 1 behind b0 = 64 -- but the word column breaks chunk 1's vote: its six columns run the plain pipeline at b0 = 64
        "1": (flag_chunk + tail, (True, False)),
        # a full-size column is dense and votes: chunk 0 stays on the unit path with a dense run of one; chunk 1 launches no pipeline
        "2": (one_full + quiet, (True, True)),
        # every unit list of chunk 0 long, chunk 1's short
        "3": (ones_chunk + tail, (True, False)),
        # what orders 1 and 2 aim at, reached: the unit path in chunk 1 with a general column and dense runs at z = 1 (two) and z = 5 (one) ...
        "1-unit": (flag_chunk + tail_unit, (True, True)),
        "3-unit": (ones_chunk + tail_unit, (True, True)),
        # ... and a chunk 0 whose vote fails (a word column among flags: the plain pipeline) in front of a chunk 1 with nothing for the pipeline
        "2-word": (one_word + quiet, (False, True)),
    }


@pytest.fixture(scope="module")
def sparse_orders():
    return _sparse_orders()


@pytest.mark.parametrize("curve,order", [("vesta", k) for k in ("1", "2", "3", "1-unit", "3-unit", "2-word")] + [("pallas", "1"), ("pallas", "1-unit")])
def test_sparse_path_past_one_chunk(tabled_bases, sparse_orders, curve, order):
    """trh_commit_batch_dev of 70 witness-like columns over 2^14 + 1 bases with their table: 64 + 6.  All 70 points against the closed
    form; chunk 1's columns as a batch of 6 on their own give the same points; `msm_unit_chunks` counts the chunks whose vote held"""
    bases, xy = tabled_bases(curve)
    cols_l, votes = sparse_orders[order]
    cols = np.stack(cols_l)
    batch = cols.shape[0]
    assert batch == 70
    # the expected counter from the sampler's rule, column by column
    col_votes = [C.sampler_votes(c, N + 1, FB_C) for c in cols]
    assert (all(col_votes[:CHUNK]), all(col_votes[CHUNK:])) == votes, [i for i, v in enumerate(col_votes) if not v]
    sf = api.SCALAR_FIELD[curve]
    blinds = synth.field_elements(0xD0 + len(order) + (curve == "pallas"), batch)
    blinds_can = cpu_ref.field_op(sf, "from_mont", blinds)
    want = [_expected(curve, np.concatenate([cols[i], blinds_can[i][None]])) for i in range(batch)]
    assert len({point_hex(w) for w in want}) == batch
    mont = _mont(curve, cols)
    d = api.DeviceBuffer.from_host(mont)
    try:
        chunks, units = api.stat("msm_chunks"), api.stat("msm_unit_chunks")
        got = bases.commit_batch_dev(d, N, batch, blinds)
        assert api.stat("msm_chunks") - chunks == 2
        assert api.stat("msm_unit_chunks") - units == sum(votes), (order, votes)
        _check(curve, got, want, CHUNK, f"order {order}")
        units = api.stat("msm_unit_chunks")
        tail = bases.commit_batch_dev(d.ptr.value + CHUNK * N * 32, N, batch - CHUNK, blinds[CHUNK:].copy())
        assert api.stat("msm_unit_chunks") - units == int(votes[1])
        _check(curve, tail, want, CHUNK, f"order {order}, chunk 1 alone", list(range(CHUNK, batch)))
    finally:
        d.free()
    full = np.concatenate([mont, blinds[:, None]], axis=1)
    _check_oracle(curve, want, full, xy, _oracle_picks(batch, CHUNK), CHUNK, f"order {order}")
