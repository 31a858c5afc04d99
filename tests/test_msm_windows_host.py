"""Which windows of the signed recoding can hold an entry, with big integers (no device).

At c = 17 the recoding has 255 // 17 + 1 = 16 windows, and fifteen of them hold every value up to 2^16 (2^255 - 1) / (2^17 - 1) >
2^254 + 2^237, which is above both Pasta moduli: the sixteenth window of a canonical scalar is empty (hostplan::choose_window_bits'
"almost always empty carry window" is always empty).  Nothing may DEPEND on that: a scalar handed over in canonical form can be anything
below 2^256 and does reach the last window.  Both halves are pinned here, with what the edge scalars of tests/msm_window_cases.py do to the
digits; tests/test_gpu_msm_windows.py runs them on the device."""
import random

import pytest

import msm_events_model as M
import msm_window_cases as C
import pasta as o

MODULI = [o.FIELDS["fp"].m, o.FIELDS["fq"].m]


def value_of(digits, c):
    return sum(d << (c * j) for j, d in enumerate(digits))


def test_top_window_of_canonical_scalars_is_empty_at_c17():
    c = 17
    assert M.num_windows(c) == 16
    fits = (1 << (c - 1)) * ((1 << (c * 15)) - 1) // ((1 << c) - 1)  # fifteen digits of + half
    assert all(m - 1 <= fits for m in MODULI)
    rng = random.Random(0x17C0)
    vals = [m - 1 for m in MODULI] + [(1 << 254) - 1, (1 << 254) + 1]
    vals += [rng.randrange(MODULI[k & 1]) for k in range(10000)]
    for s in vals:
        d = M.recode_pipeline(s, c)
        assert d[15] == 0 and value_of(d, c) == s, hex(s)


def test_top_window_of_a_full_width_scalar_is_not():
    d = M.recode_pipeline((1 << 256) - 1, 17)
    assert d[15] != 0
    # (the value is 2^256 - 1 minus the carry out of the last window, which the MSM drops like the kernel does: the digits are what is pinned)
    assert d[15] == 2 and d[0] == -1 and all(x == 0 for x in d[1:15])


@pytest.mark.parametrize("c", [8, 12, 15, 16, 17])
def test_edge_scalars_do_what_their_names_say(c):
    W, half = M.num_windows(c), 1 << (c - 1)
    for k in range(1, W):
        d = M.recode_pipeline(C.carry_dies_in(c, k), c)
        assert d[0] == half + 1 - (1 << c) and all(x == 0 for x in d[1:k]) and d[k] == 2 and all(x == 0 for x in d[k + 1:]), (c, k)
    for m in MODULI:
        for mont in (0, 1):
            bound = m if mont else 1 << 256
            edges = C.edge_scalars(c, m, mont)
            assert all(0 <= v < bound for v in edges) and len(set(edges)) == len(edges)
            tie, fold = C._windows_below(c, half, bound), C._windows_below(c, half + 1, bound)
            assert tie in edges and fold in edges
            dt, df = M.recode_pipeline(tie, c), M.recode_pipeline(fold, c)
            live = sum(1 for x in dt if x)
            assert live >= W - 2 and all(x == half for x in dt[:live])       # the tie stays positive, nothing carries
            folds = (fold.bit_length() + c - 1) // c
            assert folds >= W - 2 and df[0] == half + 1 - (1 << c) and all(x == half + 2 - (1 << c) for x in df[1:folds])  # every window folds, with the carry
            assert {0, 1, m - 1, m - 2, (1 << 254) - 1, 1 << 254, (1 << 254) + 1} <= set(edges)
            assert (((1 << 256) - 1) in edges) == (not mont) and (((1 << 255) - 1) in edges) == (not mont)
