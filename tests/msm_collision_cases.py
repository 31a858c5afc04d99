"""The cases of tests/test_gpu_msm_collisions.py, and what tests/test_msm_events_model.py proves about them on the CPU.

Every base is a small known multiple a_i of the generator (0: the identity, negative: q - |a|), every scalar is chosen digit by digit, so
operands of the MSM's point additions coincide BY CONSTRUCTION at the stage a case aims at; the expected point is (sum s_i a_i mod q) G.

A case is curve-independent: `a` holds signed integers, reduced mod the curve's group order when the case is used.  The plan numbers in
SHAPES are those of csrc/hostplan.h for the sizes used here; tests/native/hostplan_test.cpp asserts them ("collision shapes")."""
import random

import msm_events_model as M

# name -> how the MSM is run and the geometry the model needs.  mode "override": api.set_window_bits(c); "table": Bases.precompute(c), no
# override; "small": neither (n <= 8448: msm_small_kernel).  m: buckets per reduce slice; G: lanes per bucket of the combine; n: (lo, hi)
# pairs for which hostplan_test.cpp asserts these numbers
SHAPES = {
    "c8": dict(mode="override", c=8, seg_len=16, nbk=128, tpw=128, m=1, G=1, n=(64, 2400)),
    "c3": dict(mode="override", c=3, seg_len=16, nbk=4, tpw=4, m=1, G=4, n=(1024, 2048)),
    "c15": dict(mode="override", c=15, seg_len=16, nbk=16384, tpw=2048, m=8, G=1, n=(512, 512)),
    "c17": dict(mode="override", c=17, seg_len=16, nbk=65536, tpw=4096, m=16, G=1, n=(512, 512)),
    "c18": dict(mode="override", c=18, seg_len=16, nbk=131072, tpw=4096, m=32, G=1, n=(512, 512)),
    "table16": dict(mode="table", c=16, seg_len=16, nbk=32768, tpw=16384, m=2, G=1, n=(512, 512)),
    "small": dict(mode="small", c=5),
    # the table pipeline of the IPA opening at k = 14 (tests/ipa_collision_cases.py): the set g || w || u, the default table of 12 bits, the
    # quad combine of the dense route; tpw and m for one item (the commitment to s') and for two (a round)
    "ipa14": dict(mode="table", c=12, seg_len=16, nbk=2048, tpw=2048, m=1, G="q4", n=(16386, 16386)),
}
_rng = random.Random(0x5EED)
FILL = [(1 << 60) + _rng.getrandbits(60) for _ in range(2048)]  # fillers: distinct multiples far from every designed value
assert len(set(FILL)) == len(FILL)


class Case:
    def __init__(self, name, shape):
        self.name, self.shape = name, shape
        self.c = SHAPES[shape]["c"]
        self.a, self.s = [], []
        self.designed = []   # (window, bucket, needs, label): what the bucket's accumulate + combine must meet in EVERY order of its entries
        self.expect = []     # (stage, event[, where]): what the whole run must meet, in ascending and in descending order
        self._fill = 0

    def put(self, window, bucket, value, negative_digit=False):
        """one pair whose digit in `window` is +bucket (negative_digit: -bucket, which also carries +1 into the window above)"""
        assert 1 <= bucket < (1 << (self.c - 1)) or (self.shape == "small" and bucket == 16 and not negative_digit)
        self.a.append(value)
        self.s.append((((1 << self.c) - bucket) if negative_digit else bucket) << (self.c * window))

    def fill(self, window, bucket, count=1):
        for _ in range(count):
            self.put(window, bucket, FILL[self._fill])
            self._fill += 1

    def pad(self, n):
        """up to n pairs with zero scalars over filler bases: no entry anywhere, the plan numbers are those of n"""
        while len(self.a) < n:
            self.a.append(FILL[-1 - len(self.a)])
            self.s.append(0)
        return self

    @property
    def n(self):
        return len(self.a)

    def logs(self, q):
        return [v % q for v in self.a]

    def total(self, q):
        return sum(x * y for x, y in zip(self.s, self.a)) % q

    def run_model(self, q, order="asc", quad=None):
        sh = SHAPES[self.shape]
        if sh["mode"] == "small":
            return M.run_small(q, self.logs(q), self.s, order)
        quad = sh["mode"] == "table" if quad is None else quad
        return M.run_pipeline(q, self.logs(q), self.s, sh["c"], sh["seg_len"], sh["m"], sh["G"], quad, sh["mode"] == "table", order)


# ---------------------------------------------------------------------------------------
# A. the accumulate loop: designed multisets in the even buckets of window 0, at every offset of a 16-entry segment
# ---------------------------------------------------------------------------------------
# Only window 0 has entries, with one exception: a NEGATIVE digit -d is the scalar 2^c - d, which also carries +1 into window 1, so each E6
# bucket leaves one entry per negative digit in bucket 1 of window 1 (a handful per MSM, distinct multiples: no collision there).  The closed
# form accounts for them like for every other entry.
# entries: (multiple of the bucket's own P -- 0: identity, "q": +Q, "-q": -Q --, negative digit?), in index order
def _msets():
    P, N, O = (1, False), (-1, False), (0, False)
    alt = lambda k: [P, N] * k
    blk = lambda k: [P] * k + [N] * k
    sets = [
        ("E1 {P,P}", [P, P], "double"),
        ("E2 {P,-P}", [P, N], "cancel"),
        ("E3 {Px3}", [P] * 3, "double"), ("E3 {Px16}", [P] * 16, "double"), ("E3 {Px17}", [P] * 17, "double"), ("E3 {Px33}", [P] * 33, "double"),
        # E4: the partial sums of the bucket in the order it is walked start and end at the identity and move by +-P: wherever the segment
        # cuts fall, either a thread's accumulator comes back to the identity (cancel / late-cancel), or two pieces are negatives of each
        # other or identities (cancel / add-identity in the combine).  Ascending index order: blocks at even k, alternating at odd k
        ("E4 {P,-P}x1", alt(1), "cancel"), ("E4 {P,-P}x2", blk(2), "cancel"), ("E4 {P,-P}x8", alt(8), "cancel"), ("E4 {P,-P}x20", blk(20), "cancel"),
        ("E5 {O}", [O], "skip"), ("E5 {O,O,O}", [O] * 3, "skip"), ("E5 {O,P}", [O, P], "skip"), ("E5 {O,P,P}", [O, P, P], "skip double"),
        ("E5 {O,P,-P}", [O, P, N], "skip cancel"), ("E5 {P,Ox5}", [P] + [O] * 5, "skip"),
        ("E6 P: +d, -d", [(1, False), (1, True)], "cancel"), ("E6 -P: -d, P: +d", [(-1, True), (1, False)], "double"),
        # order-dependent: P, Q, -Q, P meets P + P with an accumulator that is a sum of three entries when walked up OR down (other orders
        # double early, or not at all: P, Q, P, -Q); sixteen buckets of each, and the late forms count as covered through mutation runs only
        ("E7 late-double [P,Q,-Q,P]", [P, ("q", False), ("-q", False), P], ""),
        ("E7 late-cancel [P,Q,-Q,-P]", [P, ("q", False), ("-q", False), N], ""),
        # (a segment end cuts three of the sixteen placements of a four-entry bucket: a second, longer pair keeps sixteen whole ones)
        ("E7 late-double [P,Q,Q,-Q,-Q,P]", [P, ("q", False), ("q", False), ("-q", False), ("-q", False), P], ""),
        ("E7 late-cancel [P,Q,Q,-Q,-Q,-P]", [P, ("q", False), ("q", False), ("-q", False), ("-q", False), N], ""),
    ]
    return sets


A_PER_MSM = 54


def family_a():
    items = [(off, ms) for off in range(16) for ms in _msets()]
    cases = []
    for k0 in range(0, len(items), A_PER_MSM):
        cs = Case(f"A{k0 // A_PER_MSM}", "c8")
        pos = 0
        for k, (off, (label, ents, needs)) in enumerate(items[k0:k0 + A_PER_MSM]):
            p, qv = 3 + 2 * k, 1001 + 2 * k
            lead = (off - pos - 1) % 16 + 1  # 1..16 fillers: every designed bucket follows a non-empty bucket
            cs.fill(0, 2 * k + 1, lead)
            for mult, neg in ents:
                cs.put(0, 2 * k + 2, qv if mult == "q" else -qv if mult == "-q" else mult * p, neg)
            cs.designed.append((0, 2 * k + 2, needs, f"{label} at offset {off}"))
            pos += lead + len(ents)
        cs.fill(0, 2 * A_PER_MSM + 1, 3)
        cases.append(cs)
    return cases


# ---------------------------------------------------------------------------------------
# B. pieces: buckets cut evenly by the segments, so the COMBINE adds equal or opposite sums
# ---------------------------------------------------------------------------------------
def _mixed(cs, window, bucket, p, pattern):
    for sign in pattern:
        cs.put(window, bucket, sign * p)


def family_b():
    out = []
    cs = Case("B-c8", "c8")  # one lane per bucket
    for _ in range(32):
        cs.put(0, 2, 3)                                   # 0..31: 16 P + 16 P, first with first
    cs.fill(0, 3, 8)
    for _ in range(16):
        cs.put(0, 4, 5)                                   # 40..55: 8 P + 8 P, last with first
    cs.fill(0, 5, 8)
    _mixed(cs, 0, 6, 7, [1] * 10 + [-1] * 16 + [1] * 6)   # 64..95: two pieces, negatives of each other in every order
    cs.fill(0, 7, 16)
    _mixed(cs, 0, 8, 11, [1] * 16 + [-1] * 16)            # 112..143
    cs.fill(0, 9, 5)
    cs.expect = [("combine", M.DOUBLE, (0, 2)), ("combine", M.DOUBLE, (0, 4)), ("accumulate", "publish-last", (0, 4)),
                 ("combine", M.CANCEL, (0, 6)), ("combine", M.CANCEL, (0, 8))]
    out.append(cs)

    # Four lanes per bucket: lane `sub` adds the pieces 1 + sub, 5 + sub, ... and lane 0 the head as well, then lanes 0 + 2 and 1 + 3, then 0 + 1.
    # With equal entries the pieces are equal and lanes 1 and 3 hold the same count when the bucket has 4 k + 1 or 4 k + 2 pieces: the tree's
    # first level doubles there.  Its last level cannot double on equal entries (lanes 0 and 2 always hold one piece more than 1 and 3),
    # and unequal entries would make the pieces depend on the order inside the bucket
    cs = Case("B-c3-offset", "c3")  # n = 1024
    cs.fill(0, 1, 8)
    for _ in range(464):
        cs.put(0, 2, 3)                                   # 8..471: last (8 P), twenty-eight firsts of 16 P, a first of 8 P
    _mixed(cs, 0, 3, 5, [1, 1, -1, 1, -1, -1, -1, 1] * 69)  # 472..1023: sums to the identity
    cs.expect = [("combine", M.DOUBLE, (0, 2)), ("combine-tree", M.DOUBLE, (0, 2)), ("accumulate", "publish-last", (0, 2))]
    out.append(cs)

    cs = Case("B-c3-aligned", "c3")
    for _ in range(464):
        cs.put(0, 1, 3)                                   # 29 pieces of 16 P
    _mixed(cs, 0, 2, 5, ([1] * 8 + [-1] * 8) * 35)        # 560 entries that sum to the identity
    cs.expect = [("combine", M.DOUBLE, (0, 1)), ("combine-tree", M.DOUBLE, (0, 1))]
    out.append(cs)

    # P + (-P) between pieces at four lanes.  Bucket 1, {P x 16, -P x 16} over exactly two segments: lane 0 adds the head and the one other
    # piece, which are negatives of each other in EVERY order (k P and -k P; identities only if each segment happens to hold eight of each).
    # Bucket 2, {P x 40, -P x 40} over exactly five segments: whatever the pieces are, the tree's last level adds lanes (0 + 2) and (1 + 3),
    # two sums that are negatives of each other because the bucket sums to the identity -- a cancellation unless both are the identity; in
    # ascending and descending order they are +-16 P.  Zero scalars pad the case to the 1024 pairs of the shape
    cs = Case("B-c3-opposite", "c3")
    _mixed(cs, 0, 1, 3, [1] * 16 + [-1] * 16)             # 0..31
    _mixed(cs, 0, 2, 5, [1] * 40 + [-1] * 40)             # 32..111
    cs.fill(0, 3, 9)
    cs.pad(1024)
    cs.expect = [("combine", M.CANCEL, (0, 1)), ("combine-tree", M.CANCEL, (0, 2))]
    out.append(cs)

    cs = Case("B-heavy-equal", "c3")  # n = 2048 in ONE bucket: 128 segments > HEAVY_PIECES
    for _ in range(2048):
        cs.put(0, 1, 3)
    cs.expect = [("combine-heavy-tree", M.DOUBLE, (0, 1))]
    out.append(cs)

    cs = Case("B-heavy-cancel", "c3")  # half P, half -P: the identity from non-zero inputs
    _mixed(cs, 0, 2, 7, ([1] * 8 + [-1] * 8) * 32 + ([1] * 24 + [-1] * 24) * 32)
    cs.expect = [("combine-heavy-tree", M.CANCEL, (0, 2))]
    out.append(cs)
    assert [c.n for c in out] == [149, 1024, 1024, 1024, 2048, 2048]
    return out


# ---------------------------------------------------------------------------------------
# C. reduce: ONE entry per bucket (deterministic), scalar = bucket id < 2^(c-1): only window 0 has entries
# ---------------------------------------------------------------------------------------
def _scatter(cs, nbk, count, taken, seed):
    r = random.Random(seed)
    ids = set()
    while len(ids) < count:
        b = r.randrange(1, nbk)
        if b not in taken:
            ids.add(b)
    for b in sorted(ids):
        cs.fill(0, b)


def _running_sum_slices(cs, m, t_list):
    """the four running-sum collisions, in the slices t_list (buckets t m + 1 .. t m + m; t_list[1] must be 1)"""
    t0, t1, t2, t3 = t_list
    assert t1 == 1
    cs.put(0, t0 * m + m, 3)                # only the top bucket: run = V, acc = V, then acc + run = V + V
    cs.put(0, t1 * m + m, 5)                # k + 1 = m = off: acc = m V meets off * run = m V
    cs.put(0, t2 * m + m, 7)
    cs.put(0, t2 * m + m - 1, -7)           # V, -V adjacent: run + v cancels
    cs.put(0, t3 * m + m, 11)
    cs.put(0, t3 * m + m - 1, -22)          # V, -2 V: run = -V, acc + run cancels
    cs.expect += [("reduce-acc", M.DOUBLE), ("reduce-final", M.DOUBLE), ("reduce-run", M.CANCEL), ("reduce-acc", M.CANCEL)]


def _pair(cs, id1, id2, v, sign):
    """two lone buckets whose slice totals are equal (sign = 1) or opposite: id1 * (id2 v) = +-id2 * (id1 v)"""
    cs.put(0, id1, id2 * v)
    cs.put(0, id2, sign * id1 * v)


def family_c():
    out = []
    cs = Case("C-c15-running", "c15")  # slices of 8, 2048 threads in 8 workgroups
    _running_sum_slices(cs, 8, (0, 1, 5, 7))
    _pair(cs, 805, 805 + 128 * 8, 13, 1)      # threads 100 and 228: the LDS tree's first level
    _pair(cs, 813, 813 + 128 * 8, 17, -1)
    _scatter(cs, 16384, 120, set(range(1, 65)) | set(range(801, 817)) | set(range(1825, 1841)), 15)
    cs.expect += [("reduce-tree", M.DOUBLE), ("reduce-tree", M.CANCEL)]
    out.append(cs)

    for sign in (1, -1):  # two WORKGROUPS with equal / opposite partial sums: the window-sum kernel's tree; -1: the identity from non-zero inputs
        cs = Case(f"C-c15-window-sum{'+' if sign > 0 else '-'}", "c15")
        _pair(cs, 7, 7 + 4 * 256 * 8, 19, sign)          # workgroups 0 and 4
        cs.expect = [("window-sum-tree", M.DOUBLE if sign > 0 else M.CANCEL)]
        out.append(cs)

    for shape, m in (("c17", 16), ("c18", 32)):  # the "at most four live buckets" branch
        cs = Case(f"C-{shape}-live", shape)
        b = lambda t, k: t * m + 1 + k
        cs.put(0, b(100, 2), 3); cs.put(0, b(100, 9), 3)            # two live buckets, equal sums: 0 + V, then V + V at the top bit
        cs.put(0, b(102, 2), 5); cs.put(0, b(102, 9), -5)           # opposite sums
        for k, v in ((m - 1, 7), (m - 2, -7), (5, 23), (3, 29), (0, 31)):
            cs.put(0, b(104, k), v)                                  # five live buckets: back to the running sums, whose run cancels
        for k, v in ((1, 37), (4, 41), (8, 43), (m - 1, 47)):
            cs.put(0, b(106, k), v)                                  # four: the last count that takes the shared double-and-add
        _pair(cs, b(10, 4), b(138, 4), 13, 1)                        # threads 10 and 138
        _pair(cs, b(11, 4), b(139, 4), 17, -1)
        taken = set()
        for t in (100, 102, 104, 106, 10, 11, 138, 139):
            taken |= set(range(t * m + 1, t * m + m + 1))
        _scatter(cs, 1 << (cs.c - 1), 100, taken, 17)
        cs.expect = [("reduce-live", M.DOUBLE), ("reduce-live", M.CANCEL), ("reduce-run", M.CANCEL), ("reduce-tree", M.DOUBLE), ("reduce-tree", M.CANCEL)]
        out.append(cs)

    cs = Case("C-table-running", "table16")  # fixed-base table: one bucket set, slices of 2; 64 quads or 256 threads per workgroup
    _running_sum_slices(cs, 2, (0, 1, 5, 7))
    _pair(cs, 41, 41 + 32 * 2, 13, 1)         # quads 20 and 52
    _pair(cs, 43, 43 + 32 * 2, 17, -1)
    _pair(cs, 141, 141 + 128 * 2, 19, 1)      # threads 70 and 198 of the thread-per-slice form
    _pair(cs, 143, 143 + 128 * 2, 23, -1)
    taken = set(range(1, 17)) | set(range(41, 45)) | set(range(105, 109)) | set(range(141, 145)) | set(range(397, 401))
    _scatter(cs, 32768, 120, taken, 19)
    cs.expect += [("reduce-tree", M.DOUBLE), ("reduce-tree", M.CANCEL)]
    out.append(cs)

    for sign in (1, -1):  # partial sums 0 and 64 meet in quad 0's strided loop; workgroups 0 and 16 in the thread form's tree
        cs = Case(f"C-table-window-sum{'+' if sign > 0 else '-'}", "table16")
        _pair(cs, 1, 1 + 64 * 64 * 2, 29, sign)
        cs.expect = [("window-sum", M.DOUBLE if sign > 0 else M.CANCEL)]
        out.append(cs)
    return [cs.pad(512) for cs in out]


# ---------------------------------------------------------------------------------------
# D. msm_small_kernel: digits in [-15, 16], 16 lanes per bucket, scalar = digit * 32^window
# ---------------------------------------------------------------------------------------
def family_d():
    out = []
    cs = Case("D-lanes", "small")
    for b in range(1, 17):  # window 0: two entries per bucket land on lanes 7 and 15: the tree's first level
        cs.put(0, b, 2 * b + 1)
        cs.put(0, b, (2 * b + 1) * (1 if b % 2 else -1))
    for b, k in ((2, 4), (5, 8), (9, 16)):  # window 1: 4, 8, 16 equal entries: the quad pair and the two shuffles above it
        for _ in range(k):
            cs.put(1, b, 100 + b)
    for _ in range(32):  # window 2: two entries per lane
        cs.put(2, 3, 201)
    _mixed(cs, 2, 5, 203, [1, -1, -1, 1, 1, 1, -1, -1] * 4)
    for _ in range(32):
        cs.put(2, 16, 205)  # a digit of +16
    cs.fill(3, 7, 3)
    cs.expect = [("small-tree-8", M.DOUBLE, (0, 1)), ("small-tree-8", M.CANCEL, (0, 2)), ("small-tree", M.DOUBLE, (1, 2)), ("small-tree", M.DOUBLE, (1, 5)),
                 ("small-lane", M.DOUBLE, (2, 3)), ("small-tree", M.DOUBLE, (2, 16))]
    out.append(cs)

    for name, signs in (("D-scan-equal", [1] * 16), ("D-scan-alternating", [1, -1] * 8)):
        cs = Case(name, "small")
        for window, v in ((0, 3), (9, 5)):  # all 16 bucket sums equal (or +-V): the suffix scan doubles (cancels) on every lane at every step
            for b in range(1, 17):
                cs.put(window, b, signs[b - 1] * v)
        cs.put(20, 16, 7)  # a lone digit of +16
        cs.expect = [("small-scan", M.DOUBLE if signs[1] > 0 else M.CANCEL, (0,)), ("small-scan", M.DOUBLE if signs[1] > 0 else M.CANCEL, (9,))]
        out.append(cs)
    return out


# ---------------------------------------------------------------------------------------
# E. the host Horner over the window sums
# ---------------------------------------------------------------------------------------
def family_e():
    out = []
    for shape, top in (("c8", 31), ("small", 50)):
        c = SHAPES[shape]["c"]
        cs = Case(f"E-{shape}-top-window", shape)  # only the top window that a scalar below q can fill
        for d, v in ((1, 3), (5, 7), (13, -11)):
            cs.put(top, d, v)
        out.append(cs)
        cs = Case(f"E-{shape}-window-0", shape)
        for d, v in ((1, 3), (5, 7), (13, -11)):
            cs.put(0, d, v)
        out.append(cs)
        cs = Case(f"E-{shape}-cancel-and-double", shape)
        cs.put(5, 1, 3); cs.put(4, 1, -3 << c)     # W_4 = -2^c W_5: the accumulator cancels, the doublings below are skipped
        cs.put(2, 1, 5); cs.put(1, 1, 5 << c)      # W_1 = 2^c W_2: acc + W_1 doubles
        cs.expect = [("horner", M.CANCEL, (4,)), ("horner", M.DOUBLE, (1,))]
        out.append(cs)
        cs = Case(f"E-{shape}-identity", shape)    # non-zero inputs, identity result
        cs.put(5, 1, 3); cs.put(4, 1, -3 << c)
        cs.expect = [("horner", M.CANCEL, (4,))]
        out.append(cs)
    return [cs.pad(64) if cs.shape == "c8" else cs for cs in out]


FAMILIES = {"A": family_a(), "B": family_b(), "C": family_c(), "D": family_d(), "E": family_e()}
ALL = [cs for fam in FAMILIES.values() for cs in fam]
BY_NAME = {cs.name: cs for cs in ALL}
assert len(BY_NAME) == len(ALL)
# F. batches: item k of a batch is case k, over the concatenation of the cases' bases (zero scalars elsewhere)
BATCHES = {
    "F-2-items-c8": ("c8", ["A0", "B-c8"]),
    "F-2-items-small": ("small", ["D-lanes", "D-scan-alternating"]),
    "F-8-items": ("adaptive", ["A1", "B-c8", "A2", "E-c8-cancel-and-double", "A3", "E-c8-identity", "A4", "E-c8-top-window"]),
}
