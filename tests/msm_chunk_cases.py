"""Inputs of tests/test_gpu_msm_chunks.py: batches that run as more than one launch set (`chunk` items, hostplan::msm_plan), every item
different and seeded so that the child process of the budget cases rebuilds the parent's scalars bit for bit.  Pure numpy: canonical
(.., 4) uint64 limbs below 2^254; the tests convert to the Montgomery form the entries take.

The window widths, chunk sizes and chunk counts used here are pinned without a device by the "chunk shapes" rows of
tests/native/hostplan_test.cpp."""
import numpy as np

import msm_sort_cases as S

CHUNK = 64  # hostplan::msm_plan: items per launch set at most


def uniform(rng, n):
    can = rng.integers(0, 1 << 63, (n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 4), dtype=np.uint64)
    can[:, 3] &= np.uint64((1 << 62) - 1)
    return can


def all_equal(rng, n):
    """one full-size value on every row: every window has ONE bucket, of n entries"""
    return np.repeat(uniform(rng, 1), n, axis=0)


def one_digit(rng, n, c):
    """uniform scalars in which one window (not the short top one) holds the same digit on every row, and the window below it a value
    under a quarter of the range so that no carry reaches it: one bucket of that window holds all n entries, the others stay uniform"""
    assert 64 % c == 0 and c >= 4
    can = uniform(rng, n)
    w = int(rng.integers(1, 256 // c - 1))
    dv = int(rng.integers(2, 1 << (c - 1)))  # a positive digit that is not 1
    for win, keep, val in ((w - 1, (1 << (c - 2)) - 1, 0), (w, 0, dv)):
        limb, sh = (win * c) // 64, (win * c) % 64
        field = np.uint64(((1 << c) - 1) << sh)
        can[:, limb] = (can[:, limb] & ~field) | (can[:, limb] & np.uint64(keep << sh)) | np.uint64(val << sh)
    return can


def sparse(rng, n, count):
    """`count` full-size scalars on distinct rows, zero elsewhere"""
    can = np.zeros((n, 4), dtype=np.uint64)
    can[rng.choice(n, size=count, replace=False)] = uniform(rng, count)
    return can


def plain_items(seed, n, c, batch):
    """(batch, n, 4): the first chunk's items are skewed (all scalars equal, or one digit value in one window: at 1500 pairs and segments
    of 16 entries such a bucket spans 94 segments and goes through the heavy list), the last chunk's are sparse (24 .. 40 non-zero
    scalars), the chunks between are uniform; item batch - 2 is all zero (the identity) and item 0 has all scalars equal"""
    chunks = (batch + CHUNK - 1) // CHUNK
    out = np.zeros((batch, n, 4), dtype=np.uint64)
    for i in range(batch):
        rng = np.random.default_rng([seed, n, batch, i])
        ch = i // CHUNK
        if i == batch - 2:
            continue
        if ch == chunks - 1:
            out[i] = sparse(rng, n, 24 + i % 17)
        elif ch == 0:
            out[i] = all_equal(rng, n) if i % 2 == 0 else one_digit(rng, n, c)
        else:
            out[i] = uniform(rng, n)
    return out


# ---- the budget cases: option msm_chunk_gb = 1 cuts the chunk below the batch (hostplan_test: 18 + 2 and 5 + 1) ------------------------
BUDGET_SEED = 0xC4A9


def budget_items(name):
    """(log_n, (batch, n, 4)).  "k18": 20 uniform items at 2^18, item 19 (the second of the two in the last chunk) all zero, item 1 all
    equal.  "k20": 6 items at 2^20 from the bin-sort generator -- item 4 has window 0's bin 0 one entry over the LDS capacity, item 5 (alone
    in the second chunk) exactly at it; item 1 is all zero, item 2 all equal"""
    if name == "k18":
        n, batch = 1 << 18, 20
        out = np.zeros((batch, n, 4), dtype=np.uint64)
        for i in range(batch - 1):
            rng = np.random.default_rng([BUDGET_SEED, 18, i])
            out[i] = all_equal(rng, n) if i == 1 else uniform(rng, n)
        return 18, out
    assert name == "k20" and S.LOG_N == 20
    n = 1 << 20
    out = np.zeros((6, n, 4), dtype=np.uint64)
    out[0] = S.canonical(BUDGET_SEED + 0, S.BIN_CAP - 1)
    out[2] = all_equal(np.random.default_rng([BUDGET_SEED, 20, 2]), n)
    out[3] = S.canonical(BUDGET_SEED + 3, 0)
    out[4] = S.canonical(BUDGET_SEED + 4, S.BIN_CAP + 1)
    out[5] = S.canonical(BUDGET_SEED + 5, S.BIN_CAP)
    return 20, out


BUDGET_CHUNKS = {"k18": (18, 2), "k20": (5, 2)}  # items per launch set and launch sets under msm_chunk_gb = 1; one launch set by default


# ---- the sampler's vote (msm_sparse_sample_kernel), restated: what the counter "msm_unit_chunks" is expected from -------------------------
def sampler_votes(col, n_pairs, c):
    """True when a column votes for the unit path: the sampler reads rows q * step (q < 1024, step = n_pairs // 1024) and counts their
    non-zero signed c-bit digits and those among them that are not +-1; the column is dense when count * step exceeds twice the list
    capacity W n / 8 (rounded down to a multiple of the 16 lists), and it votes when it is dense or showed no digit other than 0 / +-1.
    col: (n_pairs - 1, 4) canonical limbs (the blind, row n_pairs - 1, is beyond the last sampled row for the shapes used here)"""
    W = 255 // c + 1
    samples = min(n_pairs, 1024)
    step = n_pairs // samples
    assert (samples - 1) * step < col.shape[0]
    rows = col[:: step][:samples].astype(np.uint64)
    cap = (W * n_pairs // 8 // 16) * 16
    carry = np.zeros(samples, dtype=np.int64)
    nonzero = other = 0
    for j in range(W):
        limb, sh = (c * j) // 64, (c * j) % 64
        v = rows[:, limb] >> np.uint64(sh)
        if sh + c > 64 and limb + 1 < 4:
            v = v | (rows[:, limb + 1] << np.uint64(64 - sh))
        raw = (v & np.uint64((1 << c) - 1)).astype(np.int64) + carry
        carry = (raw > (1 << (c - 1))).astype(np.int64)
        nz = (raw != 0) & (raw != (1 << c))
        nonzero += int(nz.sum())
        other += int((nz & (raw != 1) & (raw != (1 << c) - 1)).sum())
    return nonzero * step > 2 * cap or other == 0
