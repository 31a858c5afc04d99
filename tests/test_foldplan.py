"""CPU test: the bucket lists of the IPA generator collapse (csrc/foldplan.h fold_plan: the signed sub-digit recoding of the shared scalars,
the carry between sub-windows, the bit extraction across 64-bit words, the counting sort) checked with big integers.  The native program
(tests/native/foldplan_test.cpp, built with address + undefined sanitizers) only runs fold_plan over the scalars this file writes and
writes the plans back; every property is asserted here.  No GPU, no HIP."""
import os
import random
import subprocess
import tempfile

import pasta as o
from ipa_collapse_model import recode as _recode, shape as _shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGN = 1 << 31
WINDOWS = range(10, 19)  # the table windows ipa_fold_supported accepts


def _scalars(c, rng):
    """named scalars first (the docstring of test_fold_plan... lists them), then random elements of both scalar fields"""
    _, W, w0, w1 = _shape(c)
    out = []
    for f in (o.FP, o.FQ):
        out += [0, 1, f.m - 1, f.m - 2]
    out.append((1 << 255) - 1)  # not a field element: refused as "does not fit" or reconstructed exactly

    def every_sub_digit(pick):  # the same pattern in every sub-window below bit 254
        v = 0
        for j in range(W):
            for s, w in ((0, w0), (1, w1)):
                sh = c * j + (w0 if s else 0)
                if sh + w <= 254:
                    v |= pick(w) << sh
        return v
    out.append(every_sub_digit(lambda w: 1 << (w - 1)))        # the boundary that does not carry
    out.append(every_sub_digit(lambda w: (1 << (w - 1)) + 1))  # every sub-window carries into the next
    out.append(every_sub_digit(lambda w: (1 << w) - 1))        # all ones: one carry rides to the top
    for j in range(1, W):  # a carry that ripples through j windows; and one that starts above a gap
        if c * j <= 254:
            out.append((1 << (c * j)) - 1)
            out.append(((1 << (c * j)) - 1) ^ ((1 << (c * (j // 2))) - 1))
    for edge in (64, 128, 192):  # set bits on both sides of a word boundary, in every alignment a sub-window can have there
        for lo in range(1, 10):
            for hi in range(1, 10):
                out.append(((1 << (lo + hi)) - 1) << (edge - lo))
        out += [1 << edge, 1 << (edge - 1), 3 << (edge - 1), (1 << edge) - 1, ((1 << 254) - 1) ^ ((1 << edge) - 1)]
    for i in range(64):
        out.append(rng.randrange((o.FP, o.FQ)[i & 1].m))
    if c in (10, 18):  # t = 1023, the largest index the collapse puts beside the level in an entry word (r = 10)
        while len(out) < 1024:
            out.append(rng.randrange(o.FQ.m))
    assert all(0 <= v < 1 << 255 for v in out) and len(out) <= 1024
    return out


def _run_native(cases):
    src = os.path.join(ROOT, "tests", "native", "foldplan_test.cpp")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    with tempfile.TemporaryDirectory() as tmp:
        exe, fin, fout = (os.path.join(tmp, n) for n in ("foldplan_test", "in.txt", "out.txt"))
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src, "-o", exe])
        with open(fin, "w") as fh:
            fh.write(f"{len(cases)}\n")
            for (c, W, w0, w1), sc in cases:
                fh.write(f"{c} {W} {w0} {w1} {len(sc)}\n")
                for v in sc:
                    fh.write(" ".join(f"{(v >> (64 * i)) & o.MASK64:x}" for i in range(4)) + "\n")
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and f"foldplan: ok ({len(cases)} cases)" in r.stdout, r.stdout + r.stderr
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
        lines = open(fout).read().split("\n")
    plans = []
    for q in range(len(cases)):
        rc, nbk, words = (int(v) for v in lines[2 * q].split())
        plan = [int(v) for v in lines[2 * q + 1].split()]
        assert len(plan) == words
        plans.append((rc, nbk, plan))
    return plans


def _check_plan(shape, sc, rc, nbk, plan):
    c, W, w0, w1 = shape
    nb0, nb1 = 1 << (w0 - 1), 1 << (w1 - 1)
    tag = f"c = {c}"
    want = [_recode(v, c, W, w0, w1) for v in sc]
    if any(left for _, left in want):
        assert rc != 0, f"{tag}: a scalar that does not fit {W} windows was accepted"
        return False
    assert rc == 0, f"{tag}: refused although every scalar fits"
    assert nbk == nb0 + nb1
    # size bound: what hostplan::ipa_collapse_geometry (fold_list_words) sizes the buffers by, (2 << r) * W entries for 2^r scalars
    assert len(plan) <= nbk + 1 + 2 * len(sc) * W, tag
    off, ent = plan[:nbk + 1], plan[nbk + 1:]
    assert off[0] == 0 and off[nbk] == len(ent) and all(a <= b for a, b in zip(off, off[1:])), f"{tag}: offsets"
    total = [0] * len(sc)
    seen = set()
    for b in range(nbk):
        s = 1 if b >= nb0 else 0
        mag = b - (nb0 if s else 0) + 1
        prev = None
        for e in ent[off[b]:off[b + 1]]:
            t, j, neg = e & 0xFFFF, (e >> 16) & 0x7FFF, bool(e & SIGN)
            assert t < len(sc) and j < W, f"{tag}: bucket {b}: entry {e:#x} names scalar {t}, level {j}"
            assert prev is None or (t, j) > prev, f"{tag}: bucket {b}: entries out of (t, j) order at {e:#x}"
            prev = (t, j)
            d = -mag if neg else mag
            # no entry in a bucket whose digit it does not have
            assert want[t][0].get((j, s)) == d, f"{tag}: bucket {b} (sub-window {s}, digit {mag}): scalar {t} level {j} has digit {want[t][0].get((j, s), 0)}, entry says {d}"
            assert (t, j, s) not in seen
            seen.add((t, j, s))
            total[t] += d << (c * j + (w0 if s else 0))
    for t, v in enumerate(sc):
        assert total[t] == v, f"{tag}: scalar {t} = {v:#x} reconstructs as {total[t]:#x}"  # exact, not mod m
    assert len(seen) == sum(len(d) for d, _ in want), f"{tag}: entry count"
    return True


def test_fold_plan_reconstructs_every_scalar_exactly():
    """csrc/foldplan.h for every table window c = 10 .. 18 (W = 255 / c + 1, sub-windows (c + 1) / 2 and c / 2: equal for even c, unequal for
    odd c).  Scalars: 0, 1, m - 1, m - 2 of both scalar fields; 2^255 - 1; every sub-digit 2^(w-1) (no carry) and 2^(w-1) + 1 (every
    sub-window carries); all ones; 2^(c j) - 1 carry chains; set bits straddling bits 64, 128 and 192 in every alignment; random elements;
    1024 scalars for c = 10 and 18 (t up to 1023 in the entry word).  Asserted: each scalar equals, as an integer, the sum over its entries
    of sign * digit * 2^(c j + sub-window shift); offsets start at 0, never decrease and end at the entry count; every entry sits in the
    bucket of the digit an independent recoding gives it; entries of a bucket ascend in (t, j), which tests/test_gpu_ipa_collapse.py relies
    on; the plan is no longer than the bound of hostplan::ipa_collapse_geometry (fold_list_words).  Every c * W >= 256 here, so 2^255 - 1 fits and is reconstructed."""
    rng = random.Random(0xF01D)
    cases = [(_shape(c), _scalars(c, rng)) for c in WINDOWS]
    # a table too short for its scalar: c = 16 with 15 windows cannot hold bit 240 and up
    short = ((16, 15, 8, 8), [1, (1 << 240) - 1, 1 << 239])      # 2^240 - 1 carries out of window 14
    plans = _run_native(cases + [short])
    for (shape, sc), (rc, nbk, plan) in zip(cases, plans):
        assert _check_plan(shape, sc, rc, nbk, plan), f"c = {shape[0]}: refused"
    assert plans[-1][0] != 0 and plans[-1][2] == [], "a carry out of the last window must be refused"
