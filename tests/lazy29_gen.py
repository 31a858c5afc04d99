"""Cases and big-integer references for the signed 29-bit lazy domain (csrc/field.h "Fy", csrc/curve.h "XYZZz").

One generator for tests/test_lazy29_vectors.py (host branch under UBSan) and tests/test_gpu_lazy29.py (device branch): for every
operation of tests/native/lazy29_cases.h and both fields it places operands ON the bounds that the operation's comment states --
not near them by chance -- adds a random fill over the whole permitted limb range, asserts that every operand is inside the stated
precondition (the self-check), and computes what the operation must return from oracle/pasta.py integers:

  * where the result is determined (everything below the group law) the expected limbs themselves: a reduction returns exactly
    (T - rho m) / 2^261 with rho = T / m mod 2^261 (NONNEG: (T + Q m) / 2^261, Q = -T / m mod 2^261), and a normalised or balanced
    limb vector is the unique one of its value; the defining congruence and the documented result range are asserted on top,
  * for the group law the affine point the oracle computes, the coordinate box that lets the MSM chain these operations without
    renormalising (in_bounds of tests/native/lazy29_test.cpp), and zz^3 = zzz^2.

Value of a limb vector: sum l[k] 2^(29 k), limbs signed.  K = 2^261 is the Montgomery radix of the domain.
"""
import functools

import numpy as np

import pasta as o

Y = 29
YM = (1 << Y) - 1
K = 1 << 261
NL = 9
IN_SLOTS, OUT_SLOTS = 8, 5
IN_WORDS, OUT_WORDS = 2 + IN_SLOTS * NL, OUT_SLOTS * NL + 1
TOP = (1 << 26) - 1  # top limb of a normalised value at the 16 m bound (16 m = 2^258 + ...)
RANDOM_PER_OP = 4096

OPS = ["from_fe", "to_fe", "load_store", "store_load", "mul", "mul_nonneg", "sqr", "mul2", "mul_sub", "sqr_sub_sub2",
       "add", "sub", "sub_sub2", "norm", "balance", "mul_add_lazy", "mul_sub_lazy", "mul_neg_lazy", "mul_bal_wide",
       "maybe_zero_mod", "is_zero_mod",
       "xyzzz_from_canonical", "xyzzz_to_canonical", "xyzzz_dbl_affine", "xyzzz_dbl", "xyzzz_madd", "xyzzz_madd_main", "xyzzz_add"]
OP_ID = {n: i for i, n in enumerate(OPS)}
FIELD_ID = {"fp": 0, "fq": 1}
CURVE_OF = {"fp": "pallas", "fq": "vesta"}  # the curve whose coordinates live in the field


# ---- limb vectors <-> integers ----
def val(l):
    return sum(int(x) << (Y * k) for k, x in enumerate(l))


def norm_limbs(v):
    """the normalised limbs of v: eight digits in [0, 2^29) and a signed top limb"""
    return [(v >> (Y * k)) & YM for k in range(8)] + [v >> (Y * 8)]


def bal_limbs(v):
    """the balanced limbs of v: eight digits in [-2^28, 2^28) and a signed top limb"""
    out = []
    for _ in range(8):
        d = ((v + (1 << 28)) & YM) - (1 << 28)
        out.append(d)
        v = (v - d) >> Y
    return out + [v]


def words_of(v):
    assert 0 <= v < 1 << 256
    return [(v >> (32 * i)) & 0xffffffff for i in range(8)] + [0]


def words_val(s):
    return sum((int(x) & 0xffffffff) << (32 * i) for i, x in enumerate(s[:8]))


def neg_limbs(l):
    return [-x for x in l]


# ---- the stated preconditions ----
def is_norm(f, l, bound=16):
    return all(0 <= x <= YM for x in l[:8]) and abs(val(l)) < bound * f.m


def is_small(f, l, bound=16):  # a limb-wise negated value next to normalised ones (the MSM's negated base y): |l[k]| < 2^29
    return all(-YM <= x <= YM for x in l[:8]) and abs(val(l)) < bound * f.m


def is_lazy(l):  # L1: the limb-wise sum or difference of two normalised values
    return all(abs(x) < 1 << 30 for x in l)


def is_wide(l):  # the NTT's level-3 multiplicand: |limb| <= 1.5 * 2^30
    return all(abs(x) <= 3 << 29 for x in l)


def is_bal(l):  # a balanced table constant
    return all(-(1 << 28) <= x < 1 << 28 for x in l[:8]) and abs(l[8]) <= (1 << 22) + 1


def is_any32(l):  # fy_norm's input
    return all(abs(x) < (1 << 31) - 8 for x in l)


def columns_fit(*pairs):
    """the 64-bit columns of sum a_i b_j over the given operand pairs, with the reduction's own terms (four r * m_k < 2^58, r * 2^22
    and a carry) on top, stay inside a signed 64-bit word"""
    if sum(9 * max(map(abs, a)) * max(map(abs, b)) for a, b in pairs) + (1 << 60) + (1 << 52) < 1 << 63:
        return True  # already by the limb bounds of the operand kinds
    for k in range(17):
        s = sum(abs(a[i] * b[k - i]) for a, b in pairs for i in range(max(0, k - 8), min(8, k) + 1))
        if s + (1 << 60) + (1 << 52) >= 1 << 63:
            return False
    return True


# ---- what a reduction returns ----
def reduce_(f, t, nonneg=False):
    minv = pow(f.m, -1, K)
    if nonneg:
        v = t + ((-t * minv) % K) * f.m
    else:
        v = t - ((t * minv) % K) * f.m
    assert v % K == 0
    return v >> 261


def rho_digits(f, t):
    r = (t * pow(f.m, -1, K)) % K
    return [(r >> (Y * i)) & YM for i in range(9)]


class Case:
    __slots__ = ("op", "field", "tag", "slots", "expect", "flag", "prop")

    def __init__(self, op, field, tag, slots, expect=None, flag=0, prop=None):
        self.op, self.field, self.tag, self.slots, self.expect, self.flag, self.prop = op, field, tag, slots, expect, flag, prop


def _fits(l):
    return all(-(1 << 31) <= x < 1 << 31 for x in l)


# =========================================================================================
# operand sets
# =========================================================================================
def norm_edges(f):
    """(tag, limbs) of normalised values at the edges of the domain"""
    m = f.m
    e = []
    for top in (TOP, -TOP, 0, -1):
        e.append((f"low-limbs-0,top={top}", [0] * 8 + [top]))
        e.append((f"low-limbs-max,top={top}", [YM] * 8 + [top]))
    for k in range(8):
        e.append((f"only-limb{k}-set", [YM if i == k else 0 for i in range(8)] + [0]))
        e.append((f"only-limb{k}-clear", [0 if i == k else YM for i in range(8)] + [0]))
    for j in range(-16, 17):
        for d in (-1, 0, 1):
            v = j * m + d
            if abs(v) < 16 * m:
                e.append((f"{j}m{d:+d}" if d else f"{j}m", norm_limbs(v)))
    for x in (0, 1, -1, 2, -2, m - 1):
        r = (x * K) % m
        e.append((f"R''({x if x < m - 1 else 'm-1'})", norm_limbs(r)))
        e.append((f"R''({x if x < m - 1 else 'm-1'})-m", norm_limbs(r - m)))
    for _, l in e:
        assert is_norm(f, l), l
    return e


def core_edges(f):
    m = f.m
    c = [("low-limbs-max,top=+max", [YM] * 8 + [TOP]), ("low-limbs-max,top=-max", [YM] * 8 + [-TOP]), ("low-limbs-0,top=-max", [0] * 8 + [-TOP]),
         ("low-limbs-max,top=-1", [YM] * 8 + [-1]), ("16m-1", norm_limbs(16 * m - 1)), ("-16m+1", norm_limbs(-16 * m + 1)),
         ("zero", [0] * 9), ("one", [1] + [0] * 8), ("R''(1)", norm_limbs(K % m)), ("R''(m-1)", norm_limbs((-K) % m)),
         ("alternating-limbs", [YM if i % 2 else 0 for i in range(8)] + [TOP]), ("m", norm_limbs(m))]
    for _, l in c:
        assert is_norm(f, l)
    return c


LAZY_EDGES = [("lazy-all+max", [(1 << 30) - 1] * 9), ("lazy-all-max", [-((1 << 30) - 1)] * 9),
              ("lazy-alternating+-", [((1 << 30) - 1) * (1 if i % 2 == 0 else -1) for i in range(9)]),
              ("lazy-alternating-+", [((1 << 30) - 1) * (-1 if i % 2 == 0 else 1) for i in range(9)])]


def sub_edges(f):
    """subtrahends of the merged forms: maximal and negative top limbs, and the limb-wise negated form a bucket's y takes"""
    return [("sub-top=+max", [YM] * 8 + [TOP]), ("sub-top=-max", [YM] * 8 + [-TOP]), ("sub-top=-1", [0] * 8 + [-1]),
            ("sub-low0-top=+max", [0] * 8 + [TOP]), ("sub-negated-limbs", [-YM] * 8 + [-(TOP - 1)]), ("sub-zero", [0] * 9),
            ("sub-one-limb-negative", [0, -YM, 0, 0, 0, 0, 0, 0, 1])]


class Rand:
    """random operands over the whole permitted limb range of each kind"""

    def __init__(self, seed):
        self.g = np.random.default_rng(seed)

    def _mk(self, n, lo, hi, tlo, thi):
        a = self.g.integers(lo, hi, size=(n, 8), endpoint=True)
        t = self.g.integers(tlo, thi, size=(n, 1), endpoint=True)
        return np.concatenate([a, t], axis=1).tolist()

    def N(self, n): return self._mk(n, 0, YM, -TOP, TOP)
    def S(self, n): return self._mk(n, -YM, YM, -(TOP - 1), TOP - 1)
    def L(self, n): return self._mk(n, -((1 << 30) - 1), (1 << 30) - 1, -((1 << 30) - 1), (1 << 30) - 1)
    def W(self, n): return self._mk(n, -(3 << 29), 3 << 29, -(3 << 29), 3 << 29)
    def B(self, n): return self._mk(n, -(1 << 28), (1 << 28) - 1, -((1 << 22) + 1), (1 << 22) + 1)
    def A(self, n): return self._mk(n, -((1 << 31) - 9), (1 << 31) - 9, -((1 << 31) - 9), (1 << 31) - 9)

    def below(self, n, bound):
        return [int.from_bytes(self.g.bytes(40), "little") % bound for _ in range(n)]


# =========================================================================================
# field layer
# =========================================================================================
def _mul_like(f, op, field, tag, ops, t, pairs, subs=(), nonneg=False, check_range=None):
    """a record of a product form: T = t, result reduce(T) - sum subs"""
    assert columns_fit(*pairs), (op, tag)
    r = reduce_(f, t, nonneg)
    v = r - sum(subs)
    # the defining congruence and the documented interval of the reduction itself
    assert (r * K - t) % f.m == 0
    if nonneg:
        assert t <= r * K < t + f.m * K, (op, tag)
    else:
        assert -abs(t) - f.m * K < r * K <= abs(t), (op, tag)
        assert t - f.m * K < r * K <= t
    out = norm_limbs(v)
    assert _fits(out) and abs(v) < 1 << 260, (op, tag)
    return Case(op, field, tag, ops, [out])


def field_cases(field):
    f = o.FIELDS[field]
    m = f.m
    rnd = Rand(0x1A2929 + FIELD_ID[field])
    edges, core, subs = norm_edges(f), core_edges(f), sub_edges(f)
    cases = []
    R = RANDOM_PER_OP

    def mul(op, tag, a, b, nonneg=False):
        return _mul_like(f, op, field, tag, [a, b], val(a) * val(b), [(a, b)], nonneg=nonneg)

    # ---- fy_mul / fy_mul_nonneg: every edge against the core set, both operand orders ----
    for op, nn in (("mul", False), ("mul_nonneg", True)):
        for ta, a in edges:
            for tb, b in core:
                cases.append(mul(op, f"{ta} x {tb}", a, b, nn))
                cases.append(mul(op, f"{tb} x {ta}", b, a, nn))
        # exact multiples of 2^261: the result sits on the closed end of its interval
        for top in (TOP, -TOP, 1, -1):
            for tb, b in core:
                b0 = [0] + b[1:]
                c = mul(op, f"product-multiple-of-2^261,top={top} x {tb}", [0] * 8 + [top], b0, nn)
                assert val(c.expect[0]) * K == top * (1 << 232) * val(b0)
                cases.append(c)
        # a chosen reduction round sees r = 0, r = 2^29 - 1 (and r = 1): digit i of rho = T / m mod 2^261 is that round's r
        # (NONNEG works on -T: its q = -r mod 2^29)
        rb = rnd.N(27)
        for i in range(9):
            for ti, target in enumerate((0, YM, 1)):
                b = list(rb[i * 3 + ti])
                b[0] |= 1
                sign = -1 if nn else 1
                if i < 8:
                    want = rnd.below(1, 1 << 232)[0]
                    want = (want & ~(YM << (Y * i))) | (target << (Y * i))
                    blow = val(b[:8] + [0])
                    alow = (sign * want * m * pow(blow, -1, 1 << 232)) % (1 << 232)
                    a = norm_limbs(alow)[:8] + [rb[i * 3 + ti][8]]
                else:  # round 8: the top limbs steer it, a8 * b0 + a0 * b8 with b0 = 8 and a0 = 1
                    b[0] = 8
                    a = [1] + rnd.N(1)[0][1:8] + [0]
                    b[8] = 0
                    d = (target - rho_digits(f, sign * val(a) * val(b))[8]) % (1 << Y)
                    d = d if sign > 0 else (-d) % (1 << Y)
                    a[8], b[8] = d >> 3, d & 7
                assert rho_digits(f, sign * val(a) * val(b))[i] == target, (op, i, target)
                assert is_norm(f, a) and is_norm(f, b)
                cases.append(mul(op, f"round{i}-r={'0' if target == 0 else '2^29-1' if target == YM else '1'}", a, b, nn))
    # lazy operands at their limb bound against normalised edges
    for tl, l in LAZY_EDGES:
        assert is_lazy(l)
        for tb, b in core:
            cases.append(mul("mul", f"{tl} x {tb}", l, b))
            cases.append(mul("mul", f"{tb} x {tl}", b, l))
    ra, rb = rnd.L(R), rnd.N(R)
    for i in range(R):
        a, b = (ra[i], rb[i]) if i % 2 else (rb[i], ra[i])
        cases.append(mul("mul", "random lazy x normalised" if i % 2 else "random normalised x lazy", a, b))
    ra, rb = rnd.N(R), rnd.N(R)
    cases += [mul("mul_nonneg", "random", ra[i], rb[i], True) for i in range(R)]
    for c in cases:
        if c.op == "mul_nonneg" and val(c.slots[0]) * val(c.slots[1]) >= 0:
            assert val(c.expect[0]) >= 0

    # ---- fy_sqr ----
    for ta, a in edges:
        cases.append(_mul_like(f, "sqr", field, ta, [a], val(a) ** 2, [(a, a)]))
    for a in rnd.N(R):
        cases.append(_mul_like(f, "sqr", field, "random", [a], val(a) ** 2, [(a, a)]))

    # ---- fy_mul2: the stated worst column, a lazy-maximal product plus a normalised-maximal one ----
    nmax, nmin = [YM] * 8 + [TOP], [YM] * 8 + [-TOP]
    def mul2(tag, a, b, c, d):
        assert (is_lazy(a) and is_small(f, b)) or (is_small(f, a) and is_lazy(b)), tag
        assert is_small(f, c) and is_small(f, d), tag
        return _mul_like(f, "mul2", field, tag, [a, b, c, d], val(a) * val(b) + val(c) * val(d), [(a, b), (c, d)])
    for tl, l in LAZY_EDGES:
        for tb, b in (("normalised-max", nmax), ("normalised-max,top=-max", nmin)):
            cases.append(mul2(f"worst-column {tl} x {tb} + max x max (same sign)" if l[0] > 0 else f"worst-column {tl} x {tb} + max x max (signs opposed)", l, b, nmax, nmax))
            cases.append(mul2(f"worst-column {tb} x {tl} + max x negated-max", b, l, nmax, neg_limbs(nmax)))
            cases.append(mul2(f"worst-column {tl} x {tb} + negated-max x negated-max", l, b, neg_limbs(nmax), neg_limbs(nmin)))
    for ta, a in core:
        for tb, b in core[:6]:
            cases.append(mul2(f"{ta} x {tb} + {tb} x {ta}", a, b, b, a))
    ra, rb, rc, rd = rnd.L(R), rnd.N(R), rnd.S(R), rnd.S(R)
    for i in range(R):
        a, b = (ra[i], rb[i]) if i % 2 else (rb[i], ra[i])
        cases.append(mul2("random", a, b, rc[i], rd[i]))

    # ---- fy_mul_sub / fy_sqr_sub_sub2: subtrahends with maximal and negative top limbs (the -1 / -2 rows) ----
    for ts, s in subs:
        assert is_small(f, s)
        for ta, a in core:
            for tb, b in core[:6]:
                cases.append(_mul_like(f, "mul_sub", field, f"{ta} x {tb} - {ts}", [a, b, s], val(a) * val(b), [(a, b)], subs=[val(s)]))
            for ts2, s2 in subs:
                cases.append(_mul_like(f, "sqr_sub_sub2", field, f"{ta}^2 - {ts} - 2 {ts2}", [a, s, s2], val(a) ** 2, [(a, a)], subs=[val(s), 2 * val(s2)]))
    ra, rb, rs, rs2 = rnd.N(R), rnd.S(R), rnd.S(R), rnd.S(R)
    for i in range(R):
        cases.append(_mul_like(f, "mul_sub", field, "random", [ra[i], rb[i], rs[i]], val(ra[i]) * val(rb[i]), [(ra[i], rb[i])], subs=[val(rs[i])]))
        cases.append(_mul_like(f, "sqr_sub_sub2", field, "random", [ra[i], rs[i], rs2[i]], val(ra[i]) ** 2, [(ra[i], ra[i])], subs=[val(rs[i]), 2 * val(rs2[i])]))

    # ---- lazy operands built by fy_add_lazy / fy_sub_lazy / fy_neg_lazy, then multiplied ----
    for ta, a in core:
        for tb, b in core:
            for tc, c in core[:4]:
                cases.append(_mul_like(f, "mul_add_lazy", field, f"({ta} + {tb}) x {tc}", [a, b, c], (val(a) + val(b)) * val(c), [([x + y for x, y in zip(a, b)], c)]))
                cases.append(_mul_like(f, "mul_sub_lazy", field, f"({ta} - {tb}) x {tc}", [a, b, c], (val(a) - val(b)) * val(c), [([x - y for x, y in zip(a, b)], c)]))
            cases.append(_mul_like(f, "mul_neg_lazy", field, f"(-{ta}) x {tb}", [a, b], -val(a) * val(b), [(neg_limbs(a), b)]))
    ra, rb, rc = rnd.N(R), rnd.N(R), rnd.N(R)
    for i in range(R):
        a, b, c = ra[i], rb[i], rc[i]
        cases.append(_mul_like(f, "mul_add_lazy", field, "random", [a, b, c], (val(a) + val(b)) * val(c), [([x + y for x, y in zip(a, b)], c)]))
        cases.append(_mul_like(f, "mul_sub_lazy", field, "random", [a, b, c], (val(a) - val(b)) * val(c), [([x - y for x, y in zip(a, b)], c)]))
        cases.append(_mul_like(f, "mul_neg_lazy", field, "random", [a, b], -val(a) * val(b), [(neg_limbs(a), b)]))

    # ---- balanced constant x wide multiplicand (the NTT's butterflies) ----
    wide = [("wide-all+1.5*2^30", [3 << 29] * 9), ("wide-all-1.5*2^30", [-(3 << 29)] * 9), ("wide-alternating", [(3 << 29) * (1 if i % 2 else -1) for i in range(9)])]
    bals = [("twiddle-all--2^28", [-(1 << 28)] * 8 + [(1 << 22) + 1]), ("twiddle-all-2^28-1", [(1 << 28) - 1] * 8 + [(1 << 22) + 1]),
            ("twiddle-all--2^28,top-", [-(1 << 28)] * 8 + [-1]), ("twiddle-alternating", [-(1 << 28) if i % 2 else (1 << 28) - 1 for i in range(8)] + [1 << 22])]
    for tw, w in wide:
        for tb, b in bals:
            assert is_wide(w) and is_bal(b)
            cases.append(_mul_like(f, "mul_bal_wide", field, f"{tw} x {tb}", [w, b], val(w) * val(b), [(w, b)]))
    ra, rb = rnd.W(R), rnd.B(R)
    for i in range(R):
        cases.append(_mul_like(f, "mul_bal_wide", field, "random", [ra[i], rb[i]], val(ra[i]) * val(rb[i]), [(ra[i], rb[i])]))

    # ---- carry chains: add, sub, sub_sub2, norm, balance ----
    def exact(op, tag, ops, v, limbs=norm_limbs):
        out = limbs(v)
        assert _fits(out), (op, tag)
        return Case(op, field, tag, ops, [out])
    smalls = core + [("negated-limbs-max", neg_limbs(nmax)), ("negated-limbs,top=+", [-YM] * 8 + [TOP - 1])]
    for ta, a in edges + smalls[-2:]:
        for tb, b in smalls:
            assert is_small(f, a) and is_small(f, b)
            cases.append(exact("add", f"{ta} + {tb}", [a, b], val(a) + val(b)))
            cases.append(exact("sub", f"{ta} - {tb}", [a, b], val(a) - val(b)))
    for ta, a in core:
        for tb, b in core:
            for tc, c in core:
                cases.append(exact("sub_sub2", f"{ta} - {tb} - 2 {tc}", [a, b, c], val(a) - val(b) - 2 * val(c)))
    ra, rb, rc = rnd.S(R), rnd.S(R), rnd.N(R)
    rn = rnd.N(R)
    for i in range(R):
        cases.append(exact("add", "random", [ra[i], rb[i]], val(ra[i]) + val(rb[i])))
        cases.append(exact("sub", "random", [ra[i], rb[i]], val(ra[i]) - val(rb[i])))
        cases.append(exact("sub_sub2", "random", [rn[i], rc[i], rc[(i + 1) % R]], val(rn[i]) - val(rc[i]) - 2 * val(rc[(i + 1) % R])))
    big = (1 << 31) - 8 - 1
    for tag, a in [("all+(2^31-2^3-1)", [big] * 9), ("all-(2^31-2^3-1)", [-big] * 9), ("alternating+-(2^31-2^3-1)", [big if i % 2 else -big for i in range(9)]),
                   ("alternating-+(2^31-2^3-1)", [-big if i % 2 else big for i in range(9)]), ("carry-ripple", [YM + 1] + [YM] * 7 + [0]), ("borrow-ripple", [-1] + [0] * 8)] + edges:
        assert is_any32(a)
        cases.append(exact("norm", tag, [a], val(a)))
    for a in rnd.A(R):
        cases.append(exact("norm", "random", [a], val(a)))
    for tag, a in [("all-2^28-1", [(1 << 28) - 1] * 8 + [0]), ("all-2^28", [1 << 28] * 8 + [0]), ("carry-ripples-through-all-limbs", [1 << 28] + [(1 << 28) - 1] * 7 + [5]),
                   ("carry-ripples,low-max", [YM] * 8 + [-3]), ("2^28-then-2^28-1", [(1 << 28) if i % 2 == 0 else (1 << 28) - 1 for i in range(8)] + [1 << 22])] + edges:
        assert is_norm(f, a)
        c = exact("balance", tag, [a], val(a), bal_limbs)
        assert all(-(1 << 28) <= x < 1 << 28 for x in c.expect[0][:8]) and val(c.expect[0]) == val(a)
        cases.append(c)
    for a in rnd.N(R):
        cases.append(exact("balance", "random", [a], val(a), bal_limbs))

    # ---- zero tests ----
    def zero_cases(tag, a):
        assert all(0 <= x <= YM for x in a[:8]) and abs(val(a)) <= 16 * m, tag
        v = val(a)
        cases.append(Case("is_zero_mod", field, tag, [a], [], flag=int(v % m == 0)))
        cases.append(Case("maybe_zero_mod", field, tag, [a], [], flag=int((v + 16) % (1 << Y) <= 32)))
        assert v % m != 0 or (v + 16) % (1 << Y) <= 32  # the cheap test never hides a multiple of m
    for j in range(-16, 17):
        jm = norm_limbs(j * m)
        zero_cases(f"{j}m", jm)
        for k in range(9):
            for bit in ((0, 14, 28) if k < 8 else (0, 10, 21)):
                a = list(jm)
                a[k] ^= 1 << bit
                if abs(val(a)) <= 16 * m:
                    zero_cases(f"{j}m,limb{k}-bit{bit}-flipped", a)
        for d in (-1, 1):
            if abs(j * m + d) <= 16 * m:
                zero_cases(f"{j}m{d:+d}", norm_limbs(j * m + d))
    ra = rnd.N(256)
    for i, a in enumerate(ra):  # low limb inside the 33-value window, not a multiple of m
        a[0] = (i % 33 - 16) % (1 << Y)
        zero_cases(f"low-limb-in-window({i % 33 - 16}),not-multiple", a)
        assert val(a) % m != 0
    for te, a in edges:
        zero_cases(te, a)
    for a in rnd.N(R):
        zero_cases("random", a)

    # ---- conversions ----
    def to_fe_expect(a):
        return words_of((val(a) * pow(32, -1, m)) % m)  # x 2^256 / 2^261
    def from_fe_expect(w, tag="from_fe"):
        assert w < m
        c = (1 << 266) % m
        r = reduce_(f, w * c, True)
        assert 0 <= r < m + (m >> 7) and (r - 32 * w) % m == 0, tag
        return norm_limbs(r)
    tofe = list(edges) + [(f"{j}m-1", norm_limbs(j * m - 1)) for j in range(-15, 17)] + [(f"{j}m", norm_limbs(j * m)) for j in range(-15, 16)]
    for k in range(1, 9):  # every 29-bit and 30-bit limb boundary +- 1
        for base, name in ((Y * k, "2^(29*%d)" % k), (30 * k, "2^(30*%d)" % k)):
            for d in (-1, 0, 1):
                for sgn in (1, -1):
                    tofe.append((f"{'-' if sgn < 0 else ''}({name}{d:+d})", norm_limbs(sgn * ((1 << base) + d))))
    for tag, a in tofe:
        assert is_norm(f, a), tag
        c = Case("to_fe", field, tag, [a], [to_fe_expect(a)])
        if val(a) % m == 0:
            assert words_val(c.expect[0]) == 0
        if (val(a) + 1) % m == 0:
            assert words_val(c.expect[0]) == ((m - 1) * pow(32, -1, m)) % m
        cases.append(c)
    for a in rnd.N(R):
        cases.append(Case("to_fe", field, "random", [a], [to_fe_expect(a)]))
    fes = [("0", 0), ("1", 1), ("m-1", m - 1), ("2^254", 1 << 254), ("2^254-1", (1 << 254) - 1), ("R", f.R), ("m-2", m - 2)]
    for k in range(1, 9):
        for base, name in ((Y * k, "2^(29*%d)" % k), (30 * k, "2^(30*%d)" % k)):
            fes += [(f"{name}{d:+d}", (1 << base) + d) for d in (-1, 0, 1)]
    for tag, w in fes:
        cases.append(Case("from_fe", field, tag, [words_of(w)], [from_fe_expect(w)]))
    for w in rnd.below(R, m):
        cases.append(Case("from_fe", field, "random", [words_of(w)], [from_fe_expect(w)]))
    allw = [("0", 0), ("2^256-1", (1 << 256) - 1), ("m", m), ("alternating-words", int("ffffffff00000000" * 4, 16))] + [(t, w) for t, w in fes]
    for tag, w in allw + [("random", w) for w in rnd.below(R, 1 << 256)]:
        l = [(w >> (Y * k)) & YM for k in range(8)] + [w >> 232]
        cases.append(Case("load_store", field, tag, [words_of(w)], [l, words_of(w)]))
        cases.append(Case("store_load", field, tag, [l], [words_of(w), l]))
    return cases


# =========================================================================================
# group law
# =========================================================================================
def in_box(l, top_bits, signed_limbs=False):
    lo = -YM if signed_limbs else 0
    return all(lo <= x <= YM for x in l[:8]) and abs(l[8]) < 1 << top_bits


def decode_point(f, slots):
    """result slots x, y, zz, zzz -> affine point (None: identity), with zz^3 = zzz^2 asserted"""
    x, y, zz, zzz = (val(s) for s in slots[:4])
    if all(v == 0 for v in slots[2]):
        return None
    c = pow(K, -1, f.m)
    assert zz % f.m != 0 and zzz % f.m != 0, "zz = 0 (mod m) with non-zero limbs"
    assert (pow(zz * c, 3, f.m) - pow(zzz * c, 2, f.m)) % f.m == 0, "zz^3 != zzz^2"
    return (x * pow(zz, -1, f.m) % f.m, y * pow(zzz, -1, f.m) % f.m)


def point_prop(f, want, box=True):
    def prop(out, flag):
        got = decode_point(f, out)
        assert got == want, f"point {got} != oracle {want}"
        if box and got is not None:
            assert in_box(out[0], 25), "x leaves |x| < 8 m / normalised"
            assert in_box(out[1], 24, True), "y leaves |y| < 4 m / |limb| < 2^29"
            assert in_box(out[2], 23) and in_box(out[3], 23), "zz / zzz leave the box"
    return prop


def group_cases(field):
    f = o.FIELDS[field]
    m = f.m
    cv = o.CURVES[CURVE_OF[field]]
    rnd = Rand(0x6209 + FIELD_ID[field])
    G = cv.generator
    ks = [1, 2, 3, 5, 7, 0xdeadbeef, cv.scalar.m - 1, cv.scalar.m - 2, 0x123456789abcdef0123456789abcdef]
    pts = [cv.mul(k, G) for k in ks]
    assert all(cv.is_on_curve(p) and p is not None for p in pts)
    lams = [1] + [x or 1 for x in rnd.below(6, m)]
    cases = []

    def fy(res, j, negated=False):
        """the residue res (x 2^261) shifted by j m, as normalised limbs or as the limb-wise negation of the normalised limbs of
        the opposite value (how the MSM hands over the y of a negated base)"""
        v = (res * K) % m + j * m
        return neg_limbs(norm_limbs(-v)) if negated else norm_limbs(v)

    def xyzzz(p, lam, js, negated=False):
        """p as a lazy XYZZ point with zz = lam^2, zzz = lam^3, coordinate k shifted by js[k] m"""
        if p is None:
            return [[0] * 9] * 4
        l2, l3 = lam * lam % m, pow(lam, 3, m)
        s = [fy(p[0] * l2, js[0]), fy(p[1] * l3, js[1], negated), fy(l2, js[2]), fy(l3, js[3])]
        assert is_norm(f, s[0], 8) and is_small(f, s[1], 4) and is_norm(f, s[2], 2) and is_norm(f, s[3], 2)
        assert -5 * m < 4 * val(s[2]) < 5 * m and -5 * m < 4 * val(s[3]) < 5 * m
        assert in_box(s[0], 25) and in_box(s[1], 24, True) and in_box(s[2], 23) and in_box(s[3], 23)
        return s

    def affz(p, negated=False):
        """an affine base: coordinates in [0, 1.01 m); y optionally as negated limbs (the value is then y - m <= 0)"""
        if p is None:
            return [[0] * 9] * 2
        s = [fy(p[0], 0), neg_limbs(fy(m - p[1], 0)) if negated else fy(p[1], 0)]
        assert is_norm(f, s[0], 2) and is_small(f, s[1], 2)
        return s

    # coordinate shifts: positive and negative mixed across x, y, zz, zzz, the largest that keep every residue inside the box among
    # them (a residue in [0, m) plus 6 m stays below 7 m, whose top limb is below 2^25; one plus 7 m may reach 2^257)
    shifts = [(0, 0, 0, 0), (6, -3, -1, 0), (-7, 2, 0, -1), (6, 2, 0, 0), (-7, -3, -1, -1), (3, -2, -1, 0), (-5, 1, 0, -1), (1, -1, 0, 0)]
    tagj = lambda js: "shift(x%+dm,y%+dm,zz%+dm,zzz%+dm)" % js

    # conversions of whole points
    c32 = pow(32, -1, m)
    for i, p in enumerate(pts + [None]):
        for lam in lams[:3]:
            if p is None:
                can = [0, 0, 0, 0]
            else:
                can = [f.to_mont(v) for v in (p[0] * lam * lam % m, p[1] * pow(lam, 3, m) % m, lam * lam % m, pow(lam, 3, m))]
            exp = [norm_limbs(reduce_(f, w * ((1 << 266) % m), True)) for w in can] if p is not None else [[0] * 9] * 4
            cases.append(Case("xyzzz_from_canonical", field, "identity" if p is None else f"{ks[i]:#x}G", [words_of(w) for w in can], exp, flag=int(p is None)))
            for js in shifts:
                z = xyzzz(p, lam, js, negated=(js[1] < 0 and p is not None))
                exp = [words_of(val(s) * c32 % m) for s in z]
                if p is not None:
                    assert exp == [words_of(w) for w in can]
                cases.append(Case("xyzzz_to_canonical", field, ("identity" if p is None else f"{ks[i]:#x}G") + "," + tagj(js), z, exp, flag=int(p is None)))

    # y = +-2, +-16 (mod m) in the x 2^261 form: G = (-1, 2) scaled by lam = t / 2^87 has Y = 2 t^3 / 2^261
    near0 = []
    for t in (1, -1, 2, -2):
        lam = t * pow(1 << 87, -1, m) % m
        assert (2 * pow(lam, 3, m) * K - 2 * t ** 3) % m == 0
        near0.append((f"y={2 * t ** 3:+d}(mod m)", lam))

    # doublings
    for i, p in enumerate(pts):
        for neg in (False, True):
            cases.append(Case("xyzzz_dbl_affine", field, f"{ks[i]:#x}G" + (",y-negated-limbs" if neg else ""), affz(p, neg), prop=point_prop(f, cv.double(p))))
        for n, js in enumerate(shifts):
            lam = lams[(i + n) % len(lams)]
            cases.append(Case("xyzzz_dbl", field, f"{ks[i]:#x}G," + tagj(js), xyzzz(p, lam, js, negated=(n % 3 == 1)), prop=point_prop(f, cv.double(p))))
    for tag, lam in near0:
        for js in shifts:
            cases.append(Case("xyzzz_dbl", field, f"G,{tag}," + tagj(js), xyzzz(G, lam, js), prop=point_prop(f, cv.double(G))))
    cases.append(Case("xyzzz_dbl", field, "identity", xyzzz(None, 1, shifts[0]), prop=point_prop(f, None)))

    # mixed additions: generic pairs, then every exceptional pair with the two sides congruent but not equal as integers
    def madd_cases(tag, acc, base, a_pt, b_pt):
        want = cv.add(a_pt, b_pt)
        cases.append(Case("xyzzz_madd", field, tag, acc + base, prop=point_prop(f, want)))
        if a_pt is None or b_pt is None:
            return  # the straight line is only entered with two points
        same_x = a_pt[0] == b_pt[0]
        rv = (val(base[1]) * val(acc[3]) * pow(K, -1, m) - val(acc[1])) % m

        def prop(out, flag, want=want, same_x=same_x, rv=rv):
            assert flag == int(same_x), f"same-x flag {flag}"
            assert in_box(out[4], 26) and (val(out[4]) - rv) % m == 0, "R"
            assert (val(out[4]) % m == 0) == (same_x and a_pt == b_pt) or not same_x, "R = 0 (mod m) tells P + P from P - P"
            if not same_x:
                point_prop(f, want)(out, flag)
        cases.append(Case("xyzzz_madd_main", field, tag, acc + base, prop=prop))

    n = 0
    for i, p in enumerate(pts):
        for k, q in enumerate(pts):
            js = shifts[n % len(shifts)]
            lam = lams[n % len(lams)]
            n += 1
            if i != k and cv.add(p, q) is not None:
                madd_cases(f"{ks[i]:#x}G + {ks[k]:#x}G," + tagj(js), xyzzz(p, lam, js, negated=(n % 4 == 0)), affz(q, n % 2 == 0), p, q)
        for n2, js in enumerate(shifts):
            lam = lams[(i + n2 + 1) % len(lams)]
            for negb in (False, True):
                nb = ",base-y-negated-limbs" if negb else ""
                madd_cases(f"P + P,P={ks[i]:#x}G,acc " + tagj(js) + nb, xyzzz(p, lam, js), affz(p, negb), p, p)
                madd_cases(f"P + (-P),P={ks[i]:#x}G,acc " + tagj(js) + nb, xyzzz(p, lam, js, negated=(n2 % 2 == 1)), affz(cv.neg(p), negb), p, cv.neg(p))
            madd_cases(f"P + identity,P={ks[i]:#x}G," + tagj(js), xyzzz(p, lam, js), affz(None), p, None)
        for neg in (False, True):
            madd_cases(f"identity + P,P={ks[i]:#x}G" + (",base-y-negated-limbs" if neg else ""), xyzzz(None, 1, shifts[0]), affz(p, neg), None, p)
    for tag, lam in near0:
        for js in shifts[:4]:
            madd_cases(f"P + P,P=G,acc {tag}," + tagj(js), xyzzz(G, lam, js), affz(G), G, G)
            madd_cases(f"P + (-P),P=G,acc {tag}," + tagj(js), xyzzz(G, lam, js), affz(cv.neg(G), True), G, cv.neg(G))

    # full additions
    def add_case(tag, a, b, a_pt, b_pt):
        cases.append(Case("xyzzz_add", field, tag, a + b, prop=point_prop(f, cv.add(a_pt, b_pt))))
    n = 0
    for i, p in enumerate(pts):
        for k, q in enumerate(pts):
            ja, jb = shifts[n % len(shifts)], shifts[(n // 2 + 3) % len(shifts)]
            la, lb = lams[n % len(lams)], lams[(n + 3) % len(lams)]
            n += 1
            if i != k and cv.add(p, q) is not None:
                add_case(f"{ks[i]:#x}G + {ks[k]:#x}G,a " + tagj(ja) + ",b " + tagj(jb), xyzzz(p, la, ja, negated=(n % 4 == 1)), xyzzz(q, lb, jb, negated=(n % 3 == 0)), p, q)
        for n2, ja in enumerate(shifts):
            jb = shifts[(n2 + 3) % len(shifts)]
            la, lb = lams[(i + n2) % len(lams)], lams[(i + n2 + 2) % len(lams)]
            add_case(f"P + P,P={ks[i]:#x}G,a " + tagj(ja) + ",b " + tagj(jb), xyzzz(p, la, ja), xyzzz(p, lb, jb), p, p)
            add_case(f"P + (-P),P={ks[i]:#x}G,b-y-negated-limbs,a " + tagj(ja) + ",b " + tagj(jb), xyzzz(p, la, ja), xyzzz(cv.neg(p), lb, jb, negated=True), p, cv.neg(p))
            add_case(f"P + (-P),P={ks[i]:#x}G,a " + tagj(ja) + ",b " + tagj(jb), xyzzz(p, la, ja, negated=True), xyzzz(cv.neg(p), lb, jb), p, cv.neg(p))
            add_case(f"identity + P,P={ks[i]:#x}G," + tagj(ja), xyzzz(None, 1, ja), xyzzz(p, la, ja), None, p)
            add_case(f"P + identity,P={ks[i]:#x}G," + tagj(ja), xyzzz(p, la, ja, negated=(n2 % 2 == 0)), xyzzz(None, 1, ja), p, None)
    for tag, lam in near0:
        for n2, ja in enumerate(shifts[:4]):
            add_case(f"P + P,P=G,{tag},a " + tagj(ja), xyzzz(G, lam, ja), xyzzz(G, lams[n2 + 1], shifts[n2 + 2]), G, G)
    add_case("identity + identity", xyzzz(None, 1, shifts[0]), xyzzz(None, 1, shifts[0]), None, None)
    return cases


# =========================================================================================
# files and checking
# =========================================================================================
@functools.lru_cache(maxsize=None)
def cases(field):
    """every record of a field, grouped by operation (a driver needs the records of one (op, field) to be contiguous); computed once
    per process and shared by the tests"""
    cs = field_cases(field) + group_cases(field)
    cs.sort(key=lambda c: OP_ID[c.op])  # stable
    for c in cs:
        assert len(c.slots) <= IN_SLOTS and all(len(s) == NL and _fits([x if x < 1 << 31 else x - (1 << 32) for x in s]) for s in c.slots), (c.op, c.tag)
    assert {c.op for c in cs} == set(OPS)
    return cs


def write_cases(path, cs):
    a = np.zeros((len(cs), IN_WORDS), dtype="<u4")
    for i, c in enumerate(cs):
        a[i, 0], a[i, 1] = OP_ID[c.op], FIELD_ID[c.field]
        flat = [x & 0xffffffff for s in c.slots for x in s]
        a[i, 2:2 + len(flat)] = flat
    a.tofile(path)


def read_results(path, n, sets=1):
    """result sets of a driver: (sets, n, OUT_WORDS) signed words"""
    a = np.fromfile(path, dtype="<i4")
    assert a.size == sets * n * OUT_WORDS, f"{path}: {a.size} words for {n} records"
    return a.reshape(sets, n, OUT_WORDS)


def _signed_or_word(exp, got):
    return all((int(e) - int(g)) % (1 << 32) == 0 for e, g in zip(exp, got))


def check_case(c, row):
    """one record's result words against its reference: None, or what is wrong"""
    out = [row[k * NL:(k + 1) * NL].tolist() for k in range(OUT_SLOTS)]
    flag = int(row[OUT_SLOTS * NL]) & 0xffffffff
    try:
        if c.prop is not None:
            c.prop(out, flag)
            return None
        for k, e in enumerate(c.expect):
            if not _signed_or_word(e, out[k]):
                return f"result {k}: got {out[k]}, want {e}"
        for k in range(len(c.expect), OUT_SLOTS):
            if any(out[k]):
                return f"result slot {k} not empty: {out[k]}"
        if flag != c.flag:
            return f"flag {flag}, want {c.flag}"
    except AssertionError as e:
        return str(e) or "property"
    return None


def rows_of(cs, op):
    """the (contiguous) records of an operation"""
    first = next(i for i, c in enumerate(cs) if c.op == op)
    last = first
    while last < len(cs) and cs[last].op == op:
        last += 1
    return range(first, last)


def failures(cs, res, op, limit=8):
    """messages for the records of `op` whose result is not the reference's"""
    bad = []
    for i in rows_of(cs, op):
        c = cs[i]
        why = check_case(c, res[i])
        if why:
            bad.append(f"{c.op}[{c.field}] {c.tag} (record {i}): {why}; operands {c.slots}")
            if len(bad) >= limit:
                break
    return bad


def edge_classes(cs):
    return sorted({(c.op, c.tag) for c in cs if not c.tag.startswith("random")})
