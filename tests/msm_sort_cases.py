"""Scalars that aim at the capacity of the whole-bin LDS bucket sort (msm_bin_sort_kernel) at 2^20 pairs, shared by
tests/test_gpu_msm_sort.py and tests/test_gpu_msm_chunks.py.

At 2^20 pairs (c = 16, 256 level-1 bins of 2^7 buckets each) a bin holds 4096 entries on average and the LDS takes up to
BIN_CAP = 5120 of them; a window with a bigger bin takes the chunked passes instead.  canonical() moves every window-0 digit of bins 0
and 255 to a uniform draw over the 254 bins between, then puts exactly k digits into bin 0."""
import numpy as np

LOG_N = 20
BIN_CAP = 5120  # msm.hip: (avg + avg / 16 + 512) rounded up to 1024 with avg = 2^20 / 256
WINDOWS = 16    # 255 // 16 + 1; the last (bits 240 ..) is the short top window


def lds_windows(k):
    """windows of one item that the LDS sort takes: all but the top one, and window 0 only when its bin 0 fits"""
    return WINDOWS - 1 - (k > BIN_CAP)


def window0_bins(can):
    """level-1 bin of every window-0 digit (signed base-2^16 recoding; -1: digit 0)"""
    raw = (can[:, 0] & np.uint64(0xFFFF)).astype(np.int64)
    bucket = np.where(raw > 1 << 15, (1 << 16) - raw, raw)
    return np.where(bucket > 0, (bucket - 1) >> 7, -1)


def canonical(seed, k, one_bucket=False):
    """uniform canonical scalars < 2^254 whose window-0 digits miss bins 0 and 255, except the first k: bucket 1 + (i mod 128), or
    all bucket 5 (one bucket holding k entries)"""
    n = 1 << LOG_N
    rng = np.random.default_rng(seed)
    can = rng.integers(0, 1 << 63, (n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 4), dtype=np.uint64)
    can[:, 3] &= np.uint64((1 << 62) - 1)
    edge = np.isin(window0_bins(can), (0, 255))
    moved = rng.integers(129, 32641, int(edge.sum())).astype(np.uint64)  # buckets of bins 1 .. 254, positive digits
    can[edge, 0] = (can[edge, 0] & ~np.uint64(0xFFFF)) | moved
    sub = np.full(k, 5, np.uint64) if one_bucket else (np.arange(k, dtype=np.uint64) % np.uint64(128)) + np.uint64(1)
    can[:k, 0] = (can[:k, 0] & ~np.uint64(0xFFFF)) | sub
    hist = np.bincount(window0_bins(can) + 1, minlength=257)[1:]
    assert hist[0] == k and hist[255] == 0 and hist[1:255].max() < BIN_CAP - 512
    return can
