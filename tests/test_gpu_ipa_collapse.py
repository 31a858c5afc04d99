"""GPU tests (-m gpu) of the IPA generator collapse on its own (csrc/ipafold.hip through trh_ipa_collapse_generators_dev), generator by
generator, at the smallest shapes at which each piece of it can go wrong.

Reference: G''[i] = sum over t < 2^r of s_t G[i + t m], m = 2^(k-r), s_t = the product of u_j over the set bits (r - 1 - j) of t -- what r
literal rounds of halo2's parallel_generator_collapse leave.  The generators are KNOWN multiples a_x of the curve generator (a_x = 0: the
identity, an all-zero record), so the expected G''[i] is (sum of s_t a_(i + t m) mod the group order) times the generator: Python
integers and one scalar multiplication of the C++ oracle per output.  Nothing of the code under test enters the reference.

Every comparison is bit-exact, for both curves: the 64-byte affine output against the oracle's point (64 zero bytes for the identity), and
the 128-byte record WORD FOR WORD against the record store_zrec makes of that point -- fy_from_fe's output is the unique normalised limb
vector of the reduction that tests/lazy29_gen.py models (ipa_collapse_model.zrec_words), so no comparison by decoded value is needed.

A failure names the first lane i, what the input of that lane was built to reach, every step of that lane that leaves the plain mixed
addition (from a big-integer walk of the lane through its bucket lists), and the bucket whose loss would explain the point, if one does."""
import random
import time

import numpy as np
import pytest

import cpu_ref
import ipa_collapse_model as model
import pasta as o
from common import run_with_options
from tiny_ram_halo2_amd import api, synth

pytestmark = pytest.mark.gpu
CURVES = ["pallas", "vesta"]


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


def _mont(fs, vals):
    return np.array([fs.limbs(v) for v in vals], dtype=np.uint64).reshape(-1, 4)


def _multiples(curve, logs):
    """logs[x] * generator as (n, 8) affine PODs, by the C++ oracle; 0 -> the all-zero record"""
    cv = o.CURVES[curve]
    g = np.array(cv.affine_limbs(cv.generator), dtype=np.uint64)
    xy = cpu_ref.scale_points(curve, g, _mont(cv.scalar, logs))
    zero = np.array([v % cv.scalar.m == 0 for v in logs])
    assert not xy[zero].any() and xy[~zero].any(axis=1).all()
    return xy


def _tabled(curve, xy, c):
    b = api.Bases.from_host(curve, xy)
    assert b.precompute(c) == c
    return b


def _check(curve, bases, logs, k, c, u, notes=None):
    """one launch against the integer reference.  logs: indexable, logs[x] = the discrete log of generator x; notes: {lane: what it is there for}"""
    cv = o.CURVES[curve]
    fs, fb = cv.scalar, cv.base
    order, r = fs.m, len(u)
    m = 1 << (k - r)
    s = model.fold_scalars(u, order)
    want_log = [sum(s[t] * logs[i + t * m] for t in range(1 << r)) % order for i in range(m)]
    t0 = time.perf_counter()
    got_xy, got_rec = bases.collapse_generators(k, _mont(fs, u))
    seconds = time.perf_counter() - t0
    assert got_xy.shape == (m, 8) and got_rec.shape == (m, 32)
    want_xy = _multiples(curve, want_log)
    lists = model.bucket_lists(s, c)
    # the model of the walk explains the reference before it is used to explain a failure: lane 0's buckets, weighted, sum to G''[0]
    sums0, _ = model.walk_lane(lists, logs, 0, m, c, order)
    assert sum(model.bucket_weight(b, c) * v for b, v in sums0.items()) % order == want_log[0]

    def explain(i, what):
        sums, events = model.walk_lane(lists, logs, i, m, c, order)
        live = [b for b in sorted(sums) if sums[b]]
        lost = _multiples(curve, [(want_log[i] - model.bucket_weight(b, c) * sums[b]) % order for b in live]) if live else np.zeros((0, 8), np.uint64)
        hit = [model.bucket_name(b, c) for b, p in zip(live, lost) if (p == got_xy[i]).all()]
        return (f"{curve} k = {k}, r = {r}, c = {c}: {what} differs first at lane i = {i} (workgroup {i // 256}, wave {i % 256 // 64})"
                + (f" [{notes[i]}]" if notes and i in notes else "")
                + f"; expected {'the identity' if want_log[i] == 0 else 'log ' + hex(want_log[i])}, got xy {' '.join(f'{int(v):016x}' for v in got_xy[i])}"
                + ("; as if " + " / ".join(hit) + " were lost" if hit else "; no single lost bucket explains the point")
                + "; special steps of this lane: " + ("; ".join(events[:12]) + (" ..." if len(events) > 12 else "") if events else "none"))

    bad = np.nonzero((got_xy != want_xy).any(axis=1))[0]
    assert bad.size == 0, explain(int(bad[0]), "G'' (affine)") + f" ({bad.size} of {m} lanes differ)"
    words = lambda row: (o.limbs_to_int(row[0:4]), o.limbs_to_int(row[4:8]))  # noqa: E731
    want_rec = np.array([model.zrec_words(fb, *words(row)) for row in want_xy], dtype=np.uint32)
    assert not want_rec[~want_xy.any(axis=1)].any()
    bad = np.nonzero((got_rec != want_rec).any(axis=1))[0]
    if bad.size:
        i = int(bad[0])
        w = int(np.nonzero(got_rec[i] != want_rec[i])[0][0])
        raise AssertionError(explain(i, "the 128-byte record") + f": word {w} is {int(got_rec[i][w]):#010x}, store_zrec of the expected point has {int(want_rec[i][w]):#010x}")
    return seconds


# (k, r, c, rows beyond 2^k): the smallest shapes at which each piece can go wrong
SHAPES = [(10, 2, 10, 2),   # m = 256: one workgroup per bucket; one bucket per slice of the reduction, the offset multiple does all the work
          (10, 2, 11, 2),   # w0 = 6, w1 = 5: unequal sub-windows, the high one doubled w0 times
          (10, 2, 13, 2),
          (10, 2, 16, 2),
          (10, 2, 17, 2),   # w0 = 9, w1 = 8: the largest unequal split
          (10, 2, 18, 2),   # 16 buckets per slice
          (10, 2, 12, 0),   # a set of exactly 2^k rows: the table's stride equals 2^k
          (11, 2, 15, 2),   # m = 512: two workgroups in x
          (13, 5, 14, 2)]   # a middle shape


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("k,r,c,extra", SHAPES)
def test_collapse_matches_integer_reference(curve, k, r, c, extra):
    """random known generators, random challenges, every shape of SHAPES; sets of 2^k + 2 rows (the opening's g || w || u stride) except
    where the row says otherwise"""
    order = o.CURVES[curve].scalar.m
    rnd = random.Random(0xC011A95E ^ (k << 16) ^ (c << 8) ^ r)
    logs = [rnd.randrange(1, order) for _ in range((1 << k) + extra)]
    bases = _tabled(curve, _multiples(curve, logs), c)
    try:
        _check(curve, bases, logs, k, c, [rnd.randrange(1, order) for _ in range(r)])
    finally:
        bases.destroy()


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("c,which", [(13, "minus-one"), (12, "one")])
def test_collapse_with_unit_challenges(curve, c, which):
    """(10, 2) with u = (m - 1, m - 1): s = 1, -1, -1, 1, scalars with every high window full; and with u = (1, 1): all four scalars are 1,
    the whole collapse is bucket 0 with four entries per lane"""
    order = o.CURVES[curve].scalar.m
    rnd = random.Random(0x0171 + c)
    logs = [rnd.randrange(1, order) for _ in range((1 << 10) + 2)]
    bases = _tabled(curve, _multiples(curve, logs), c)
    try:
        _check(curve, bases, logs, 10, c, [order - 1, order - 1] if which == "minus-one" else [1, 1])
    finally:
        bases.destroy()


class _Progression:
    """the discrete logs of api.Bases.generate: s0 + x d"""

    def __init__(self, s0, d):
        self.s0, self.d = s0, d

    def __getitem__(self, x):
        return self.s0 + x * self.d


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("k,r,c", [(17, 9, 12), (18, 10, 10)])
def test_collapse_with_many_scalars(curve, k, r, c):
    """512 and 1024 shared scalars (t up to 1023 beside the level in an entry word; c = 10: 26 table levels) over device-generated bases
    with logs s0 + x d, which are never downloaded.  The (18, 10) device call is timed (NOTEBOOK.md has the figure): the reference here
    is 2^r + m integer products and m scalar multiplications"""
    order = o.CURVES[curve].scalar.m
    rnd = random.Random(0xB16 + k)
    bases = api.Bases.generate(curve, synth.BASE_S0, synth.BASE_D, (1 << k) + 2)
    try:
        assert bases.precompute(c) == c
        seconds = _check(curve, bases, _Progression(synth.BASE_S0, synth.BASE_D), k, c, [rnd.randrange(1, order) for _ in range(r)])
        print(f"collapse ({k}, {r}, c = {c}) {curve}: {seconds * 1e3:.1f} ms for the call and the two downloads")
    finally:
        bases.destroy()


def _exceptional_logs(curve, second):
    """(10, 2, c = 12), m = 256: ordinary lanes with the exceptional ones among them, several per wave.  First launch (u_1 = 1: t and t + 1
    carry the same scalar and share every bucket, t first):
      double    G[i + m] = G[i]: bucket 0 (digit 1) meets the same point at its second entry -- the doubling that reads the record again
      cancel    G[i + m] = -G[i]: the second entry cancels the first and the bucket goes on fresh with t = 2, 3 (u_0 = 1 mod 64 puts them there)
      skip      G[i] = identity: the record is skipped and the bucket starts on its second entry
      skip2     G[i + m] = identity: a skipped record in the middle of a list
      empty     G[i + t m] = identity for every t: every bucket ends fresh, the reduction sums identities, the affine kernel's identity branch
      pairs     G[i + m] = -G[i] and G[i + 3m] = -G[i + 2m]: in every bucket of u_0's digits the last entry cancels an accumulator with
                zz != 1 and the bucket ends fresh; G''[i] is the identity by arithmetic
    Second launch (u = (1, 1): bucket 0 holds t = 0, 1, 2, 3 of every lane):
      late-double  G[i + 2m] = G[i] + G[i + m]: a doubling met by an accumulator with zz != 1
      late-cancel  the same and G[i + 3m] = -2 (G[i] + G[i + m]): the last entry cancels; G''[i] is the identity"""
    order = o.CURVES[curve].scalar.m
    m = 256
    rnd = random.Random(0xE8CE + second)
    logs = [rnd.randrange(1, order) for _ in range(4 * m + 2)]
    notes = {}
    if not second:
        kinds = {"double": [3, 64, 200], "cancel": [5, 65, 201], "skip": [7, 66, 255], "skip2": [8, 130], "empty": [9, 67], "pairs": [0, 11, 68, 254]}
        for kind, lanes in kinds.items():
            for i in lanes:
                notes[i] = kind
                if kind == "double":
                    logs[i + m] = logs[i]
                elif kind == "cancel":
                    logs[i + m] = order - logs[i]
                elif kind == "skip":
                    logs[i] = 0
                elif kind == "skip2":
                    logs[i + m] = 0
                elif kind == "empty":
                    for t in range(4):
                        logs[i + t * m] = 0
                else:
                    logs[i + m], logs[i + 3 * m] = order - logs[i], order - logs[i + 2 * m]
    else:
        kinds = {"late-double": [2, 63, 64, 129], "late-cancel": [4, 70, 191, 255]}
        for kind, lanes in kinds.items():
            for i in lanes:
                notes[i] = kind
                logs[i + 2 * m] = (logs[i] + logs[i + m]) % order
                if kind == "late-cancel":
                    logs[i + 3 * m] = (-2 * (logs[i] + logs[i + m])) % order
    return logs, notes


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("second", [0, 1])
def test_collapse_exceptional_branches(curve, second):
    """every branch of the accumulation's case analysis beside ordinary lanes of the same waves (see _exceptional_logs), against the same
    integer reference: the expected scalar simply comes out as what it is, or as zero"""
    order = o.CURVES[curve].scalar.m
    logs, notes = _exceptional_logs(curve, second)
    rnd = random.Random(0xE8CF)
    # u_0 = 1 (mod 64): its lowest sub-digit is 1, so bucket 0 holds (t, level 0) for t = 0, 1, 2, 3 and goes on after t = 1
    u = [1, 1] if second else [(rnd.randrange(64, order) & ~63) | 1, 1]
    # the inputs reach what they are there for: the walk of each marked lane shows the step (and ordinary lanes show none)
    s = model.fold_scalars(u, order)
    lists = model.bucket_lists(s, 12)
    expect = {"double": "entry 1 (t = 1, level 0): doubling", "cancel": "entry 1 (t = 1, level 0): cancellation", "skip": "entry 0 (t = 0, level 0): identity record skipped",
              "skip2": "entry 1 (t = 1, level 0): identity record skipped", "empty": "ends fresh", "pairs": "ends fresh",
              "late-double": "entry 2 (t = 2, level 0): doubling", "late-cancel": "entry 3 (t = 3, level 0): cancellation"}
    for i in range(256):
        _, events = model.walk_lane(lists, logs, i, 256, 12, order)
        if i in notes:
            assert any(expect[notes[i]] in e for e in events), (i, notes[i], events[:4])
            if notes[i] in ("empty", "pairs"):
                assert sum("ends fresh" in e for e in events) == len(lists)
            if notes[i] in ("cancel", "pairs"):  # the cancellation is not the end of its bucket: the next entry has to find it fresh
                assert any("entry 2 (t = 2, level 0): starts the bucket again after a cancellation" in e for e in events), (i, events[:4])
        else:
            assert not events, (i, events[:4])
    bases = _tabled(curve, _multiples(curve, logs), 12)
    try:
        _check(curve, bases, logs, 10, 12, u, notes)
    finally:
        bases.destroy()


def test_collapse_refusals():
    """what the entry refuses, each with TRH_EINVAL and a message: no table, fewer than 2^k points, and the shapes ipa_fold_supported rejects"""
    curve = "pallas"
    logs = list(range(1, (1 << 10) + 3))
    xy = _multiples(curve, logs)
    u = _mont(o.CURVES[curve].scalar, [3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23][:11])
    plain = api.Bases.from_host(curve, xy)
    try:
        with pytest.raises(api.TrhError, match="no fixed-base table"):
            plain.collapse_generators(10, u[:2])
        assert plain.precompute(12) == 12
        with pytest.raises(api.TrhError, match="at least 2\\^k"):
            plain.collapse_generators(11, u[:2])
        for k, r in ((10, 1), (10, 3), (9, 2), (10, 11)):   # r < 2, k < r + 8 (twice), r > 10
            with pytest.raises(api.TrhError, match="unsupported shape"):
                plain.collapse_generators(k, u[:r])
        assert plain.precompute(9) == 9                      # a table window below 10 bits
        with pytest.raises(api.TrhError, match="unsupported shape"):
            plain.collapse_generators(10, u[:2])
    finally:
        plain.destroy()


OPENING_SCRIPT = r"""
import random
import numpy as np, torch
import cpu_ref
import pasta as o
from common import LimbTranscript
from tiny_ram_halo2_amd import api, ipa, poly, synth
api.init(0)
curve, k, r = "pallas", 14, 6
assert api.get_option("ipa_fold") == r
cv = o.CURVES[curve]
fs = cv.scalar
order, n, m = fs.m, 1 << k, 1 << (k - r)
lim = lambda v: np.array(fs.limbs(v), np.uint64)
rnd = random.Random(0x0BE7)
logs = [rnd.randrange(1, order) for _ in range(n)]
# u_5 = 1: t and t + 1 (t even) carry the same scalar.  Lanes of the collapse with repeated, negated and identity generators, a column of
# identities and a column whose pairs all cancel: G''[9], G''[67], G''[11] and G''[68] are the identity
for i in (3, 64, 200):
    logs[i + m] = logs[i]
for i in (5, 65, 201):
    logs[i + 3 * m] = order - logs[i + 2 * m]
for i in (7, 66, 255):
    logs[i] = 0
for i in (9, 67):
    for t in range(1 << r):
        logs[i + t * m] = 0
for i in (11, 68):
    for t in range(0, 1 << r, 2):
        logs[i + (t + 1) * m] = order - logs[i + t * m]
gen = np.array(cv.affine_limbs(cv.generator), np.uint64)
g_l = cpu_ref.scale_points(curve, gen, np.array([fs.limbs(v) for v in logs], np.uint64))
w_l = cpu_ref.gen_bases_hashed(curve, 0x5151, 1)
u_l = cpu_ref.gen_bases_hashed(curve, 0x6262, 1)

class OneBeforeTheCollapse(LimbTranscript):
    # challenges: xi, z, u_0 .. u_(k-1); u_(r-1) is 1, the others are the hash's
    def __init__(self, field, as_int):
        super().__init__(field)
        self.count, self.as_int, self.challenges = 0, as_int, []
    def squeeze_challenge_scalar(self):
        v = self.field.from_limbs(super().squeeze_challenge_scalar())
        if self.count == 2 + r - 1:
            v = 1
        self.count += 1
        self.challenges.append(v)
        return v if self.as_int else lim(v)

params = poly.Params(curve, k, g_l, g_l, w_l, u=u_l, precompute=True)
cbits = int(api.lib().trh_bases_precomputed_window_bits(params.ipa_bases().handle))
assert len(params.ipa_bases()) == n + 2 and cbits == 13, cbits
p_l, s_l = synth.field_elements(0xC0A1, n), synth.field_elements(0xC0A2, n)
p_blind, s_blind, x3 = rnd.randrange(order), rnd.randrange(order), rnd.randrange(order)
draws = [rnd.randrange(order) for _ in range(2 * k)]
p_dev = torch.from_numpy(np.ascontiguousarray(p_l, dtype=np.uint64).view(np.int64).copy()).cuda()
before = api.stat("ipa_generator_collapses")
it = iter(draws)
t_dev = OneBeforeTheCollapse(fs, True)
c_dev, f_dev = ipa.create_proof_native(params, lambda: next(it), t_dev, p_dev, p_blind, x3, s_l, s_blind)
print("collapses", api.stat("ipa_generator_collapses") - before)
it = iter(draws)
t_ref = OneBeforeTheCollapse(fs, False)
c_ref, f_ref = cpu_ref.ipa_create_proof(curve, k, g_l, w_l[0], u_l[0], lambda: lim(next(it)), t_ref, p_l, lim(p_blind), lim(x3), s_l, lim(s_blind))
assert t_dev.challenges[2 + r - 1] == 1 and t_ref.challenges[2 + r - 1] == 1
# the collapsed generators of THIS opening, from the challenges it drew: some are the identity
u = t_dev.challenges[2:2 + r]
s = [1] * (1 << r)
for t in range(1 << r):
    for j in range(r):
        if (t >> (r - 1 - j)) & 1:
            s[t] = s[t] * u[j] % order
ident = [i for i in range(m) if sum(s[t] * logs[i + t * m] for t in range(1 << r)) % order == 0]
print("identity lanes", ident)
print("items", len(t_dev.log), len(t_ref.log))
for i, (a, b) in enumerate(zip(t_dev.log, t_ref.log)):
    if a != b:
        print("transcript item", i, "differs")
        break
else:
    print("transcript equal", (c_dev, f_dev) == (fs.from_limbs(c_ref), fs.from_limbs(f_ref)))
"""


def test_opening_over_collapsed_generators_with_identities():
    """one whole opening (pallas, k = 14, collapse after 6 rounds: m = 256, a 13-bit table) over generators with the repeated, negated and
    identity structure of test_collapse_exceptional_branches and a transcript whose last challenge before the collapse is 1: the rounds
    after the collapse run over a G'' that holds identities, and every transcript item is still the C++ oracle's literal prover's"""
    out = run_with_options(OPENING_SCRIPT, {"TRH_IPA_FOLD": "6", "TRH_IPA_TABLE_BITS": "13"}, timeout=300)
    assert "collapses 1\n" in out, out
    assert "identity lanes [9, 11, 67, 68]" in out, out
    assert f"items {1 + 2 * 14 + 2} {1 + 2 * 14 + 2}" in out, out
    assert "transcript equal True" in out, out
