"""GPU test (-m gpu): the product forms of the signed 29-bit lazy domain (csrc/field.h) with the result written over each operand in
turn and with one value in several operand slots: a = mul(a, b), b = mul(a, b), a = sqr(a), mul2(a, b, a, b), mul_sub(a, a, a), ...
On the device a product is one block of v_mad_i64_i32 inline assembly per column; tests/test_gpu_lazy29.py keeps every operand and
the result in slots of their own, where a wrong constraint of such a block (early clobber, tied operand) cannot show.
tests/native/lazy29_alias_test (built by `make` with the library's flags) runs each record through the device branch and through the
plain C++ host branch of the same headers.  Per shape and field: all four slots after the call are equal on both, limb for limb, the
untouched ones are unchanged, and the written one is the big-integer value.  256 random records per shape plus the operand bounds of
tests/lazy29_gen.py.  One subprocess per field, under a time limit, never retried."""
import os
import subprocess

import numpy as np
import pytest

import lazy29_gen as gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "lazy29_alias_test")
FIELDS = ["fp", "fq"]
RANDOM_PER_SHAPE = 256

# shape -> (operation, slots the call reads as its operands, slot it writes); order = enum Shape of the driver
SHAPES = [("mul_a", "mul", (0, 1), 0), ("mul_b", "mul", (0, 1), 1), ("mul_aa", "mul", (0, 0), 0),
          ("nonneg_a", "mul_nonneg", (0, 1), 0), ("nonneg_b", "mul_nonneg", (0, 1), 1), ("nonneg_aa", "mul_nonneg", (0, 0), 0),
          ("sqr_a", "sqr", (0,), 0),
          ("mul2_a", "mul2", (0, 1, 2, 3), 0), ("mul2_b", "mul2", (0, 1, 2, 3), 1), ("mul2_c", "mul2", (0, 1, 2, 3), 2), ("mul2_d", "mul2", (0, 1, 2, 3), 3),
          ("mul2_abab", "mul2", (0, 1, 0, 1), 0),
          ("mul_sub_a", "mul_sub", (0, 1, 2), 0), ("mul_sub_b", "mul_sub", (0, 1, 2), 1), ("mul_sub_s", "mul_sub", (0, 1, 2), 2), ("mul_sub_aaa", "mul_sub", (0, 0, 0), 0),
          ("sqr_sub_a", "sqr_sub_sub2", (0, 1, 2), 0), ("sqr_sub_s1", "sqr_sub_sub2", (0, 1, 2), 1), ("sqr_sub_s2", "sqr_sub_sub2", (0, 1, 2), 2),
          ("sqr_sub_aaa", "sqr_sub_sub2", (0, 0, 0), 0)]
SHAPE_NAMES = [s[0] for s in SHAPES]
ZERO = [0] * 9


def expected(f, op, x):
    """big-integer value of the call on operand limbs x, and the (a, b) pairs whose columns it sums"""
    v = [gen.val(l) for l in x]
    if op in ("mul", "mul_nonneg"):
        return gen.reduce_(f, v[0] * v[1], op == "mul_nonneg"), [(x[0], x[1])]
    if op == "sqr":
        return gen.reduce_(f, v[0] ** 2), [(x[0], x[0])]
    if op == "mul2":
        return gen.reduce_(f, v[0] * v[1] + v[2] * v[3]), [(x[0], x[1]), (x[2], x[3])]
    if op == "mul_sub":
        return gen.reduce_(f, v[0] * v[1]) - v[2], [(x[0], x[1])]
    return gen.reduce_(f, v[0] ** 2) - v[1] - 2 * v[2], [(x[0], x[0])]


def shape_records(field, si):
    """(tag, [a, b, c, d]) of one shape: the operand bounds of lazy29_gen.py in the kinds the shape permits, then random ones"""
    f = gen.o.FIELDS[field]
    name, op, reads, _ = SHAPES[si]
    edges, core, subs = gen.norm_edges(f), gen.core_edges(f), gen.sub_edges(f)
    nmax, nmin = [gen.YM] * 8 + [gen.TOP], [gen.YM] * 8 + [-gen.TOP]
    rnd = gen.Rand(0xA11A5 + 64 * gen.FIELD_ID[field] + si)
    R = RANDOM_PER_SHAPE
    rn, rb, rl, rc, rd = rnd.N(R), rnd.N(R), rnd.L(R), rnd.S(R), rnd.S(R)
    out = []
    shared = len(set(reads)) < len(reads)
    if shared:  # one value in several slots: every slot has to be normalised for the columns to fit
        for ta, a in edges:
            if name == "mul2_abab":
                out += [(f"{ta} x {tb}", [a, b, ZERO, ZERO]) for tb, b in core[:6]]
            else:
                out.append((ta, [a, ZERO, ZERO, ZERO]))
        out += [("random", [rn[i], rb[i], ZERO, ZERO]) for i in range(R)]
    elif op in ("mul", "mul_nonneg"):
        for ta, a in edges:
            for tb, b in core:
                out += [(f"{ta} x {tb}", [a, b, ZERO, ZERO]), (f"{tb} x {ta}", [b, a, ZERO, ZERO])]
        if op == "mul":
            for tl, l in gen.LAZY_EDGES:
                for tb, b in core:
                    out += [(f"{tl} x {tb}", [l, b, ZERO, ZERO]), (f"{tb} x {tl}", [b, l, ZERO, ZERO])]
            out += [("random lazy x normalised", [rl[i], rb[i], ZERO, ZERO]) if i % 2 else ("random normalised x lazy", [rb[i], rl[i], ZERO, ZERO]) for i in range(R)]
        else:
            out += [("random", [rn[i], rb[i], ZERO, ZERO]) for i in range(R)]
    elif op == "sqr":
        out += [(ta, [a, ZERO, ZERO, ZERO]) for ta, a in edges]
        out += [("random", [rn[i], ZERO, ZERO, ZERO]) for i in range(R)]
    elif op == "mul2":
        for tl, l in gen.LAZY_EDGES:
            for tb, b in (("normalised-max", nmax), ("normalised-max,top=-max", nmin)):
                out += [(f"worst-column {tl} x {tb} + max x max", [l, b, nmax, nmax]), (f"worst-column {tb} x {tl} + max x negated-max", [b, l, nmax, gen.neg_limbs(nmax)]),
                        (f"worst-column {tl} x {tb} + negated-max x negated-max", [l, b, gen.neg_limbs(nmax), gen.neg_limbs(nmin)])]
        for ta, a in core:
            out += [(f"{ta} x {tb} + {tb} x {ta}", [a, b, b, a]) for tb, b in core[:6]]
        out += [("random", [rl[i], rb[i], rc[i], rd[i]] if i % 2 else [rb[i], rl[i], rc[i], rd[i]]) for i in range(R)]
    elif op == "mul_sub":
        for ts, s in subs:
            for ta, a in core:
                out += [(f"{ta} x {tb} - {ts}", [a, b, s, ZERO]) for tb, b in core[:6]]
        out += [("random", [rn[i], rc[i], rd[i], ZERO]) for i in range(R)]
    else:
        for ts, s in subs:
            for ta, a in core:
                out += [(f"{ta}^2 - {ts} - 2 {ts2}", [a, s, s2, ZERO]) for ts2, s2 in subs]
        out += [("random", [rn[i], rc[i], rd[i], ZERO]) for i in range(R)]
    for tag, s in out:
        x = [s[k] for k in reads]
        v, pairs = expected(f, op, x)
        assert gen.columns_fit(*pairs) and abs(v) < 1 << 260, (name, tag)
    return out


@pytest.fixture(scope="module")
def device_results(tmp_path_factory):
    done = {}

    def run(field):
        if field not in done:
            done[field] = None  # a failed run is not started again by the next test of the field
            assert os.path.exists(EXE), "tests/native/lazy29_alias_test is missing: run `make`"
            recs = [shape_records(field, si) for si in range(len(SHAPES))]
            n = sum(len(r) for r in recs)
            words = np.zeros((n, 2 + 8 * 9), dtype=np.int32)
            first, i = [], 0
            for si, rs in enumerate(recs):
                first.append(i)
                for _, s in rs:
                    words[i, 0], words[i, 1] = si, gen.FIELD_ID[field]
                    words[i, 2:2 + 36] = np.array(s, dtype=np.int64).reshape(36)
                    i += 1
            d = tmp_path_factory.mktemp("lazy29_alias_" + field)
            src, dst = str(d / "cases.bin"), str(d / "results.bin")
            words.astype("<i4").tofile(src)
            r = subprocess.run(["timeout", "-k", "10", "120", EXE, src, dst], capture_output=True, text=True)
            assert r.returncode == 0 and "records ok" in r.stdout, f"exit {r.returncode}\n{r.stdout}{r.stderr}"
            res = gen.read_results(dst, n, sets=2)
            done[field] = (recs, first, res[0], res[1])
        assert done[field] is not None, "the device run of this field failed (see the first test of the field)"
        return done[field]
    return run


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("field", FIELDS)
def test_in_place_and_shared_operands_match_host_branch(device_results, field, shape):
    recs, first, dev, host = device_results(field)
    si = SHAPE_NAMES.index(shape)
    _, op, reads, written = SHAPES[si]
    f = gen.o.FIELDS[field]
    rs = recs[si]
    assert len(rs) >= RANDOM_PER_SHAPE
    bad = []
    for k, (tag, s) in enumerate(rs):
        i = first[si] + k
        d, h = np.asarray(dev[i]), np.asarray(host[i])
        if (d != h).any():
            bad.append(f"{shape}[{field}] {tag} (record {i}): device {d.tolist()} != host {h.tolist()}; operands {s}")
            continue
        got = d.reshape(-1)[:36].reshape(4, 9).tolist()
        v, _ = expected(f, op, [s[j] for j in reads])
        want = [gen.norm_limbs(v) if j == written else s[j] for j in range(4)]
        if got != want:
            bad.append(f"{shape}[{field}] {tag} (record {i}): slots {got} != big-integer reference {want}")
    assert not bad, f"{len(bad)} of {len(rs)} records\n" + "\n".join(bad[:8])
