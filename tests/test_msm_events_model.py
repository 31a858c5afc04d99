"""CPU only: what tests/msm_events_model.py says about every case of tests/test_gpu_msm_collisions.py (tests/msm_collision_cases.py).

  * both signed recodings sum back to the scalar and stay inside their digit sets;
  * the model's walk of every case ends at sum s_i a_i mod q -- the closed form the GPU test compares with -- in ascending and in
    descending order of the entries inside the buckets (the order is not deterministic on the device);
  * the events a case is built for occur: those of a whole run in both orders; those of a designed bucket of family A in EVERY distinct order
    of its entries when it has at most 8 of them, else in both orders and a sample of random ones (all-equal multisets have one order; the
    +-P multisets come back to the identity wherever the segments cut them -- the walk argument in msm_collision_cases._msets);
  * the designed buckets of family A start at every offset of a 16-entry segment and publish to first, direct and last; the order-dependent
    events (late-double, late-cancel) sit in at least 16 buckets under ascending AND under descending order."""
import itertools
import random

import pytest

import msm_collision_cases as C
import msm_events_model as M
import pasta as o

ORDERS = {name: cv.scalar.m for name, cv in o.CURVES.items() if name in ("pallas", "vesta")}


def test_recodings_sum_back_to_the_scalar():
    r = random.Random(7)
    q = max(ORDERS.values())
    scalars = [0, 1, q - 1, (1 << 254) - 1, 16, 17, 127, 128, 129] + [r.randrange(q) for _ in range(200)] + sorted({x for cs in C.ALL for x in cs.s})
    for s in scalars:
        d = M.recode_small(s)
        assert sum(v << (5 * j) for j, v in enumerate(d)) == s and all(-15 <= v <= 16 for v in d)
        for c in (2, 3, 5, 8, 15, 16, 17, 18):
            d = M.recode_pipeline(s, c)
            assert sum(v << (c * j) for j, v in enumerate(d)) == s and all(-(1 << (c - 1)) < v <= 1 << (c - 1) for v in d), (s, c)
    # a digit of magnitude exactly 2^(c-1) stays positive in the pipeline's recoding, +16 in the small kernel's
    assert M.recode_pipeline(128, 8)[:2] == [128, 0] and M.recode_pipeline(129, 8)[:2] == [-127, 1]
    assert M.recode_small(16)[:2] == [16, 0] and M.recode_small(17)[:2] == [-15, 1]


def test_cases_use_only_the_digits_they_name():
    """a designed digit is below 2^(c-1) in magnitude (the small kernel's +16 apart), so no case depends on the sign of the half digit"""
    for cs in C.ALL:
        small = cs.shape == "small"
        for s in cs.s:
            d = M.recode_small(s) if small else M.recode_pipeline(s, cs.c)
            assert all(abs(v) < (1 << (cs.c - 1)) or (small and v == 16) for v in d), cs.name
        lo, hi = C.SHAPES[cs.shape].get("n", (1, 8448))
        assert lo <= cs.n <= hi, (cs.name, cs.n)
    for shape, names in C.BATCHES.values():
        n = sum(C.BY_NAME[k].n for k in names)
        if shape == "small":
            assert n <= 8448 and len(names) <= 4
        elif shape == "c8":
            assert n <= C.SHAPES["c8"]["n"][1]
        else:
            assert 512 <= n < 6144 and len(names) >= 8  # c = 8 is the plan's own choice, one lane per bucket, adaptive segments of 16


@pytest.mark.parametrize("curve", sorted(ORDERS))
@pytest.mark.parametrize("name", [cs.name for cs in C.ALL])
def test_model_reaches_the_closed_form_and_the_events(curve, name):
    q, cs = ORDERS[curve], C.BY_NAME[name]
    for order in ("asc", "desc"):
        forms = (None,) if C.SHAPES[cs.shape]["mode"] != "table" else (True, False)  # the table shape runs in the quad and in the thread form
        for quad in forms:
            ev, result = cs.run_model(q, order, quad)
            assert result == cs.total(q), (order, quad)
            for e in cs.expect:
                if quad is False and e[0].startswith(("reduce-tree", "window-sum")):
                    e = ("reduce-tree" if e[0] == "reduce-tree" else "window-sum-tree",) + tuple(e[1:])
                assert ev.has(*e), (order, quad, e, sorted(k for k in ev.n if k[1] != M.ADD_ID))


def _orders(k, values, rng):
    if k <= 8:
        seen = set()
        for perm in itertools.permutations(range(k)):
            key = tuple(values[i] for i in perm)
            if key not in seen:
                seen.add(key)
                yield perm
        return
    yield tuple(range(k))
    yield tuple(reversed(range(k)))
    if len(set(values)) > 1:
        for _ in range(6):
            p = list(range(k))
            rng.shuffle(p)
            yield tuple(p)


def _any(ev, w, *pairs):
    return any(ev.has(stage, event, w) for stage, event in pairs)


DOUBLES = (("accumulate", M.DOUBLE), ("accumulate", M.LATE_DOUBLE), ("combine", M.DOUBLE))
CANCELS = (("accumulate", M.CANCEL), ("accumulate", M.LATE_CANCEL), ("combine", M.CANCEL))


@pytest.mark.parametrize("name", [cs.name for cs in C.FAMILIES["A"]])
def test_designed_buckets_meet_their_events_in_every_order(name):
    q, cs = ORDERS["pallas"], C.BY_NAME[name]
    sh = C.SHAPES[cs.shape]
    rng = random.Random(11)
    lst = M.window_lists(q, cs.logs(q), [M.recode_pipeline(x, cs.c) for x in cs.s])[0]
    ranges = M.bucket_ranges(lst)
    for window, bucket, needs, label in cs.designed:
        S, E = ranges[bucket]
        assert label.endswith(f"at offset {S % 16}"), (label, S)
        assert S > 0 and lst[S - 1][1] != 0  # it follows a non-empty bucket (in the same segment unless it starts one)
        values = [v for _, v, _ in lst[S:E]]
        for perm in _orders(E - S, values, rng):
            ev, total = M.bucket_events(q, lst, bucket, perm, sh["seg_len"], sh["G"])
            w = (window, bucket)
            assert total == sum(values) % q, (label, perm)
            if "skip" in needs:
                assert ev.has("accumulate", M.SKIP, w), (label, perm)
            if "double" in needs:
                assert _any(ev, w, *DOUBLES), (label, perm)
            if "cancel" in needs:
                assert _any(ev, w, *CANCELS), (label, perm)


def test_family_a_covers_offsets_publish_targets_and_the_order_dependent_events():
    q = ORDERS["vesta"]
    offsets, targets, sizes = {}, {}, {}
    late = {(order, e): 0 for order in ("asc", "desc") for e in (M.LATE_DOUBLE, M.LATE_CANCEL, M.RESTART, M.STALE)}
    for cs in C.FAMILIES["A"]:
        for order in ("asc", "desc"):
            ev, result = cs.run_model(q, order)
            assert result == cs.total(q)
            for window, bucket, needs, label in cs.designed:
                kind, off = label.split(" at offset ")
                w = (window, bucket)
                if order == "asc":
                    offsets.setdefault(kind, set()).add(int(off))
                    sizes[kind] = sum(1 for x in cs.s if x & 255 in (bucket, 256 - bucket))
                    targets.setdefault(kind, set()).update(t for t in ("first", "direct", "last") if ev.has("accumulate", "publish-" + t, w))
                for e in (M.LATE_DOUBLE, M.LATE_CANCEL, M.RESTART, M.STALE):
                    late[(order, e)] += ev.has("accumulate", e, w)
    assert len(offsets) == 22 and all(v == set(range(16)) for v in offsets.values()), offsets
    for kind, t in targets.items():  # a one-entry bucket cannot run past its segment, one of 16 or more cannot lie inside one
        assert t == {"first"} | ({"direct"} if sizes[kind] < 16 else set()) | ({"last"} if sizes[kind] > 1 else set()), (kind, t, sizes[kind])
    assert all(v >= 16 for v in late.values()), late


def test_four_lane_cancellations_hold_in_every_order():
    """B-c3-opposite: lane 0's head + piece (bucket 1) and the last level of the shuffle tree (bucket 2) add two opposite sums whatever the
    order of the entries is; they cancel unless both sums are the identity.  A sample of random orders next to the two of `expect`"""
    q, cs = ORDERS["pallas"], C.BY_NAME["B-c3-opposite"]
    rng = random.Random(13)
    sizes = {1: 32, 2: 80}
    cancels = 0
    for _ in range(40):
        order = {(0, b): rng.sample(range(k), k) for b, k in sizes.items()}
        ev, result = cs.run_model(q, order)
        assert result == cs.total(q)
        for stage, b in (("combine", 1), ("combine-tree", 2)):
            assert ev.has(stage, M.CANCEL, (0, b)) or ev.has(stage, M.ADD_ID, (0, b)), (stage, order)
            cancels += ev.has(stage, M.CANCEL, (0, b))
        assert not ev.has("combine", M.DOUBLE, (0, 1))
    assert cancels >= 60  # identities on both sides are the rare outcome
