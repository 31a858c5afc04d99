"""Scalars at the edges of msm_recode_kernel's signed base-2^c recoding, for tests/test_msm_windows_host.py (big integers, no device) and
tests/test_gpu_msm_windows.py.

The kernel cuts digit j from bits [c j, c j + c) of the scalar, adds the carry of the window below and folds raw > half = 2^(c-1) to
raw - 2^c with a carry; raw = half stays positive (tests/msm_events_model.py has the rule).  The cases: the tie, carries that run through
every window or die in a chosen one, the values around 2^254 where the top window of canonical scalars begins to fill, and -- for scalars
handed over in canonical form (mont = 0), which may be anything below 2^256 -- values that reach the last window."""
import os
import re

import numpy as np

import msm_events_model as M
import pasta as o

HOSTPLAN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tiny-ram-halo2_amd", "csrc", "hostplan.h")


def small_max_n():
    """the largest MSM hostplan::msm_route hands to msm_small_kernel: one pair more takes the pipeline"""
    with open(HOSTPLAN) as f:
        return int(re.search(r"constexpr uint32_t SMALL_MAX_N = (\d+);", f.read()).group(1))


def _windows_below(c, digit, bound):
    """digit in every window from 0 up, as many windows as stay below bound"""
    s = 0
    for j in range(M.num_windows(c)):
        t = s + (digit << (c * j))
        if t >= bound:
            break
        s = t
    return s


def carry_dies_in(c, k):
    """window 0 folds (half + 1), windows 1 .. k - 1 are all ones (with the carry: digit 0, the carry goes on), window k holds 1 (with the
    carry: 2, the carry ends)"""
    mask, half = (1 << c) - 1, 1 << (c - 1)
    return (half + 1) + sum(mask << (c * j) for j in range(1, k)) + (1 << (c * k))


def edge_scalars(c, m, mont):
    """the edge values below `bound` (the modulus for Montgomery scalars, 2^256 for canonical ones), without repeats, in a fixed order"""
    bound = m if mont else 1 << 256
    half = 1 << (c - 1)
    vals = [0, 1, m - 1, m - 2, (1 << 254) - 1, 1 << 254, (1 << 254) + 1,
            _windows_below(c, half, bound),       # the tie in every window: all digits + half, no carry
            _windows_below(c, half + 1, bound)]   # every window folds: the carry runs to the top
    vals += [carry_dies_in(c, k) for k in range(1, M.num_windows(c))]
    if not mont:
        vals += [(1 << 255) - 1, (1 << 256) - 1]
    out = []
    for v in vals:
        if v < bound and v not in out:
            out.append(v)
    return out


def limbs(vals):
    return np.array([o.int_to_limbs(v) for v in vals], dtype=np.uint64).reshape(-1, 4)


def scalars_with_edges(c, m, mont, n, seed):
    """n scalars as Python integers: random ones below m with the edge values spread among them (the first and the last slot included)"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 1 << 63, (n, 5), dtype=np.uint64)
    vals = [sum(int(x) << (62 * i) for i, x in enumerate(row)) % m for row in raw]
    edges = edge_scalars(c, m, mont)
    assert len(edges) <= n
    where = np.linspace(0, n - 1, len(edges)).astype(int)
    for i, v in zip(where, edges):
        vals[int(i)] = v
    return vals
