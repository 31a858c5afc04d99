"""Designed MSMs of the IPA opening's dense route (csrc/ipa.hip: MsmFlags::dense_hint -- the lean sort, msm_combine_q4_kernel), for
tests/test_gpu_ipa_collisions.py, and what tests/test_msm_events_model.py proves about them on the CPU.

The smallest opening that runs the table pipeline is k = 14 over a resident set g || w || u of N = 2^14 + 2 points with the default table of
12 bits (shape "ipa14" of msm_collision_cases.SHAPES; tests/native/hostplan_test.cpp asserts the plan numbers): W = 22 windows in ONE set of
2048 buckets, segments of 16, the LDS bin sort, eleven expected pieces per bucket.  Two kinds of opening make an MSM of that route designable
from outside:

  kind S   s(X) is designed, p(X) is random.  s' = s - s(x3) differs from s in coefficient 0 only, so the commitment to s' (one item) is
           the designed MSM: pair j of the Case sits at generator 1 + j.
  kind P   s(X) = 0, p(X) is designed.  p' = p except at coefficient 0; row L of round 0 holds p'[half ..] on the generators below half and
           row R holds p'[.. half] on those from half on: L_0 and R_0 are two DIFFERENT designed MSMs in one launch (items 0 and 1).  Pair j
           of the L design sits at generator j with p[half + j], pair j of the R design at generator half + 1 + j with p[1 + j].
           S is then s_blind W over an otherwise all-zero row.

The scalars that are not designed -- s'[0] or p'[0], the blind or rand_l / rand_r on w, z value_l / z value_r on u -- are full-size and
known once x3, the draws and the transcript are fixed (tests/ipa_exponent_model.py): their 22 digits each fall into arbitrary buckets of the
same set.  The rows used everywhere are the real ones, these scalars included.  PINS holds, per case and curve, the seed of the free inputs
and the number of entries below the first designed bucket (mod 16) the designs were laid out for, found by `python tests/ipa_collision_cases.py`:
with them no undesigned entry falls into the designed range of buckets and the aligned buckets start on a segment boundary.  The CPU test
asserts both, so a change of the plan or of the transcript fails there and the search is run again.

Designs (all digits in window 0, every bucket's points multiples of its own small P):
  pieces   whole segments of one point, so that the quad combine meets: piece + equal piece; an identity piece in first, middle and last
           position; piece + opposite piece with the chain going on; a bucket inside one segment (`direct`); a bucket that starts
           mid-segment and runs on (`last`), once with a doubling; a bucket of 1100 entries of one point between ordinary buckets (the
           heavy hand-over).  Buckets of one point meet their event in EVERY order of their entries; the mixed ones are palindromes, and
           ascending and descending order are what the CPU test proves.
  multisets  E1 - E6 of msm_collision_cases._msets at rotating segment offsets: the accumulate events under the lean gate."""
import random

import ipa_exponent_model as X
import msm_collision_cases as C
import msm_events_model as M
import pasta as o

K = 14
N = 1 << K
HALF = N // 2
SET = N + 2
SHAPE = C.SHAPES["ipa14"]
B0 = 16  # the first bucket of a design: above the few buckets the short top window of the undesigned scalars fills


def gen_fill(i):
    """the generator of an index no design uses: distinct multiples far from every designed value and from C.FILL"""
    return (1 << 61) + 7919 * i + 1


class Design(C.Case):
    """a Case of shape ipa14 laid out bucket by bucket from B0; `pos` is the position (mod 16) of the next entry in the sorted list"""

    def __init__(self, name, shift):
        super().__init__(name, "ipa14")
        self.shift = self.pos = shift % 16
        self.bucket = B0

    def lead(self, want):
        """an ordinary bucket of 1 .. 16 distinct fillers after which the next bucket starts at offset `want` of a segment"""
        count = (want - self.pos - 1) % 16 + 1
        self.fill(0, self.bucket, count)
        self.pos, self.bucket = (self.pos + count) % 16, self.bucket + 1

    def run(self, values, needs="", label=""):
        """the next bucket: entries with these multiples (ints, or (value, negative digit?)) in index order"""
        b = self.bucket
        for v in values:
            v, neg = v if isinstance(v, tuple) else (v, False)
            self.put(0, b, v, neg)
        self.designed.append((0, b, needs, f"{label} at offset {self.pos}"))
        self.pos, self.bucket = (self.pos + len(values)) % 16, b + 1
        return (0, b)

    @property
    def last_bucket(self):
        return self.bucket - 1


def add_pieces(d):
    """the combine's cases; d.expect names what the quad combine must meet where"""
    q4 = "combine-q4"
    P = lambda: 3 + 2 * len(d.designed)  # noqa: E731  (a fresh small multiple per bucket; the multisets take theirs from 301 on)
    d.lead(0)
    w = d.run([P()] * 32, label="double: 16 P + 16 P")
    d.expect += [(q4, M.HEAD_FIRST, w), (q4, M.DOUBLE, w)]
    p = P()
    w = d.run([0] * 16 + [p] * 16 + [0] * 16, label="identity piece first and last")
    d.expect += [(q4, "identity-first", w), (q4, "identity-last", w), (q4, M.ADD_ID, w), ("accumulate", M.SKIP, w)]
    p = P()
    w = d.run([p] * 16 + [0] * 16 + [p] * 16, label="identity piece in the middle, then 16 P + 16 P")
    d.expect += [(q4, "identity-middle", w), (q4, M.ADD_ID, w), (q4, M.DOUBLE, w)]
    p = P()
    w = d.run([p] * 16 + [-p] * 16 + [1001 + p] * 16 + [-p] * 16 + [p] * 16, label="16 P - 16 P, then the chain goes on")
    d.expect += [(q4, M.CANCEL, w), (q4, M.ADD_ID, w)]
    d.lead(3)
    w = d.run([P()] * 2, label="inside one segment")
    d.expect += [(q4, M.HEAD_DIRECT, w), ("accumulate", "publish-direct", w), ("accumulate", M.DOUBLE, w)]
    d.lead(8)
    w = d.run([P()] * 16, label="8 P (last) + 8 P (first)")
    d.expect += [(q4, M.HEAD_LAST, w), ("accumulate", "publish-last", w), (q4, M.DOUBLE, w)]
    d.lead(5)
    w = d.run([P()] * 34, label="starts mid-segment and runs on: 11 + 16 + 7")
    d.expect += [(q4, M.HEAD_LAST, w), ("accumulate", "publish-last", w)]
    d.lead((d.pos + 5) % 16)
    w = d.run([P()] * 1100, label="1100 entries of one point")
    d.heavy = w
    d.expect += [(q4, M.HANDOVER, w), ("combine-heavy-tree", M.DOUBLE, w)]
    d.lead((d.pos + 5) % 16)


def add_multisets(d, rot):
    """E1 - E6 (the order-dependent E7 are left to tests/test_gpu_msm_collisions.py), multiset k at offset rot + 5 k"""
    sets = [ms for ms in C._msets() if not ms[0].startswith("E7")]
    base = len(d.designed)
    for k, (label, ents, needs) in enumerate(sets):
        p = 301 + 2 * (base + k)
        d.lead((rot + 5 * k) % 16)
        d.run([(mult * p, neg) for mult, neg in ents], needs, label)
    d.lead((d.pos + 3) % 16)


class OpeningCase:
    def __init__(self, name, kind):
        self.name, self.kind = name, kind
        self._cache = {}

    def designs(self, shift):
        """{row: Design}; `shift`: entries below bucket B0 (mod 16) of the row whose design is aligned"""
        if self.kind == "S":
            d = Design(self.name + "/S", shift)
            add_pieces(d)
            add_multisets(d, 1)
            return {"S": d}
        dl, dr = Design(self.name + "/L_0", shift), Design(self.name + "/R_0", 0)
        add_multisets(dl, 6)
        add_pieces(dl)
        add_multisets(dr, 11)   # the R row is not aligned: multisets and the heavy bucket, which need no alignment
        w = dr.run([77] * 1100, label="1100 entries of one point")
        dr.heavy = w
        dr.expect += [("combine-q4", M.HANDOVER, w), ("combine-heavy-tree", M.DOUBLE, w)]
        dr.lead((dr.pos + 5) % 16)
        return {"L_0": dl, "R_0": dr}

    def first_index(self, row):
        return {"S": 1, "L_0": 0, "R_0": HALF + 1}[row]

    def inputs(self, curve, seed, shift):
        """everything create_proof takes: generators' logs, omega, upsilon, the polynomials, blinds, x3 and the draws"""
        q = o.CURVES[curve].scalar.m
        rnd = random.Random(f"{self.name}/{curve}/{seed}")
        full = lambda: rnd.randrange(1, q)  # noqa: E731
        designs = self.designs(shift)
        a = [gen_fill(i) for i in range(N)]
        poly = [0] * N
        for row, d in designs.items():
            at = self.first_index(row)
            assert d.n <= (HALF - 1 if self.kind == "P" else N - 1)
            for j, (aj, sj) in enumerate(zip(d.a, d.s)):
                a[at + j] = aj % q
                poly[(at + j + HALF) % N if self.kind == "P" else at + j] = sj
        inp = dict(a=a, omega=full(), upsilon=full(), p_blind=full(), s_blind=full(), x3=full(), draws=[full() for _ in range(2 * K)])
        if self.kind == "S":
            inp["s_poly"], inp["p_poly"] = poly, [full() for _ in range(N)]
        else:
            inp["s_poly"], inp["p_poly"] = [0] * N, poly
        return inp, designs

    def build(self, curve, seed=None, shift=None, point_of=None):
        """-> (inputs, designs, rows): rows[name] = the N + 2 scalars of that MSM as the opening forms it, undesigned ones included"""
        pinned = seed is None
        if pinned:
            if curve in self._cache:
                return self._cache[curve]
            seed, shift = PINS[(self.name, curve)]
        cv = o.CURVES[curve]
        q = cv.scalar.m
        inp, designs = self.inputs(curve, seed, shift)
        if point_of is None:
            import numpy as np
            point_of = lambda log: np.array(cv.affine_limbs(cv.mul(log, cv.generator) if log else None), dtype=np.uint64)  # noqa: E731
        it = iter(inp["draws"])
        tr = X.LogTranscript(cv.scalar, point_of)
        op = X.create_proof(q, K, inp["a"], inp["omega"], inp["upsilon"], lambda: next(it), tr, inp["p_poly"], inp["p_blind"], inp["x3"],
                            inp["s_poly"], inp["s_blind"], rounds=1)
        rows = {"S": op.row_s, "L_0": op.row_l0, "R_0": op.row_r0}
        out = (inp, designs, rows)
        if pinned:
            self._cache[curve] = out
        return out


def logs_of(inp):
    return inp["a"] + [inp["omega"], inp["upsilon"]]


def sorted_lists(q, inp, row, order="asc"):
    """the sorted list of one MSM over the table: window_lists' {0: [(bucket, value, flat index)]}"""
    zero = [0] * M.num_windows(SHAPE["c"])
    digits = [M.recode_pipeline(s, SHAPE["c"]) if s else zero for s in row]
    return M.window_lists(q, logs_of(inp), digits, flat_c=SHAPE["c"], order=order)


def run(q, lists, lose=None):
    """the dense route behind the sort: accumulate, quad combine (heavy hand-over), quad reduction -> (Events, result)"""
    return M.run_lists(q, lists, SHAPE["c"], SHAPE["seg_len"], SHAPE["m"], "q4", True, True, lose)


def closed_form(q, inp, row):
    return X.dot(row, logs_of(inp), q)


def undesigned_inside(lists, d, first_index):
    """entries of the designed range of buckets that are not the design's own: [(bucket, window, index)]"""
    own = range(first_index, first_index + d.n)
    return [(b, flat // SET, flat % SET) for b, _, flat in lists[0] if B0 <= b <= d.last_bucket and not (flat // SET == 0 and flat % SET in own)]


def layout_problems(q, inp, designs, rows, case):
    """why this seed and shift do not fit, or []"""
    out = []
    for row, d in designs.items():
        lists = sorted_lists(q, inp, rows[row])
        inside = undesigned_inside(lists, d, case.first_index(row))
        if inside:
            out.append(f"{row}: undesigned entries inside the design {inside[:3]}")
        start = M.bucket_ranges(lists[0])[B0][0]
        if row != "R_0" and start % 16 != d.shift:
            out.append(f"{row}: {start} entries below bucket {B0}, laid out for {d.shift} (mod 16)")
    return out


CASES = [OpeningCase("S-dense", "S"), OpeningCase("P-dense", "P")]
BY_NAME = {c.name: c for c in CASES}
# (case, curve) -> (seed, shift): see the module docstring
PINS = {
    ("S-dense", "pallas"): (0, 4),
    ("S-dense", "vesta"): (0, 4),
    ("P-dense", "pallas"): (0, 4),
    ("P-dense", "vesta"): (15, 4),
}


def search(case, curve, seeds=range(400)):
    q = o.CURVES[curve].scalar.m
    for seed in seeds:
        for shift in range(16):
            inp, designs, rows = case.build(curve, seed, shift)
            if not layout_problems(q, inp, designs, rows, case):
                return seed, shift
    raise RuntimeError(f"{case.name} {curve}: no seed fits")


if __name__ == "__main__":
    for case in CASES:
        for curve in ("pallas", "vesta"):
            print(f'    ("{case.name}", "{curve}"): {search(case, curve)},', flush=True)
