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


# ---------------------------------------------------------------------------------------
# The designed MSMs of the IPA opening's dense route (tests/ipa_collision_cases.py, tests/test_gpu_ipa_collisions.py): the rows are the ones
# the opening really forms -- the undesigned full-size scalars on coefficient 0, w and u included -- walked with the quad combine
# ---------------------------------------------------------------------------------------
import ipa_collision_cases as I  # noqa: E402

Q4 = "combine-q4"
NOTES_ONLY = ("identity-first", "identity-middle", "identity-last")  # positions of an identity piece: the event that can be lost there is the add-identity
DOUBLES_Q4 = (("accumulate", M.DOUBLE), ("accumulate", M.LATE_DOUBLE), (Q4, M.DOUBLE))
CANCELS_Q4 = (("accumulate", M.CANCEL), ("accumulate", M.LATE_CANCEL), (Q4, M.CANCEL))


def _sensitive(q, lists, want, event, context):
    ev, result = I.run(q, lists, lose=event)
    assert ev.lost > 0, (context, event, "the walk never reaches the event that was to be lost")
    assert result != want, (context, event, "the total does not change when this event's result is lost")


@pytest.mark.parametrize("curve", sorted(ORDERS))
@pytest.mark.parametrize("name", [c.name for c in I.CASES])
def test_opening_cases_meet_their_events_and_are_sensitive(curve, name):
    """for every designed MSM of an opening, as the opening forms it, in ascending and descending order: the layout the designs were made for
    holds; the model's total is the closed form (and the exponent model's S, L_0, R_0); every named event occurs at its bucket in its stage;
    with that one event's result lost the total changes"""
    q, case = ORDERS[curve], I.BY_NAME[name]
    inp, designs, rows = case.build(curve)
    assert not I.layout_problems(q, inp, designs, rows, case)
    assert all(len(r) == I.SET for r in rows.values())
    walked = dict(designs, S=designs.get("S"))  # kind P: S = s_blind W over an otherwise all-zero row, a case of its own
    for row, d in walked.items():
        want = I.closed_form(q, inp, rows[row])
        if d is None:
            assert case.kind == "P" and not any(rows[row][:I.N]) and rows[row][I.N] == inp["s_blind"] and want == inp["s_blind"] * inp["omega"] % q
        for order in ("asc", "desc"):
            lists = I.sorted_lists(q, inp, rows[row], order)
            ev, result = I.run(q, lists)
            ctx = (name, curve, row, order)
            assert result == want, ctx
            if d is None:
                continue
            for e in d.expect:
                assert ev.has(*e), (ctx, e, sorted(k for k in ev.at if k[2:] == e[2]))
                if e[1] not in NOTES_ONLY:
                    _sensitive(q, lists, want, e, ctx)
            for window, bucket, needs, label in d.designed:
                w = (window, bucket)
                for need, options in (("skip", (("accumulate", M.SKIP),)), ("double", DOUBLES_Q4), ("cancel", CANCELS_Q4)):
                    if need in needs:
                        met = [(s, e) for s, e in options if ev.has(s, e, w)]
                        assert met, (ctx, label, need)
                        for s, e in met:
                            _sensitive(q, lists, want, (s, e, w), (ctx, label))
            # the accumulate's control flow under the gate: a restart after a cancellation, and stale limbs that must not be published
            for event in (M.RESTART, M.STALE):
                at = sorted(k[2:] for k in ev.at if k[:2] == ("accumulate", event))
                assert at, (ctx, event)
                changed = 0
                for w in at:
                    changed += I.run(q, lists, lose=("accumulate", event, w))[1] != want
                assert changed >= 1, (ctx, event, at)
            # the heavy bucket lies between ordinary buckets that the quad stores itself
            hw, hb = d.heavy
            assert ev.at[(Q4, M.HANDOVER, hw, hb)] == 1 and ev.n[(Q4, M.HANDOVER)] == 1, ctx
            assert all(any(ev.has(Q4, h, (hw, b)) for h in (M.HEAD_FIRST, M.HEAD_DIRECT, M.HEAD_LAST)) for b in (hb - 1, hb + 1)), ctx


@pytest.mark.parametrize("name", [c.name for c in I.CASES])
def test_opening_multisets_meet_their_events_in_every_order(name):
    """the multisets E1 - E6 inside an opening's rows, under the quad combine: every distinct order of a bucket of at most 8 entries, both
    orders and a sample of random ones otherwise; no undesigned entry shares a bucket with them (asserted above)"""
    q, case = ORDERS["pallas"], I.BY_NAME[name]
    inp, designs, rows = case.build("pallas")
    rng = random.Random(17)
    offsets, targets = set(), set()
    for row, d in designs.items():
        lst = I.sorted_lists(q, inp, rows[row])[0]
        ranges = M.bucket_ranges(lst)
        for window, bucket, needs, label in d.designed:
            if not needs:
                continue
            S, E = ranges[bucket]
            offsets.add(S % 16)
            assert S > 0 and lst[S - 1][1] != 0 and lst[S - 1][0] == bucket - 1  # it follows an ordinary bucket
            if row != "R_0":
                assert label.endswith(f"at offset {S % 16}"), (label, S)
            values = [v for _, v, _ in lst[S:E]]
            w = (window, bucket)
            for perm in _orders(E - S, values, rng):
                ev, total = M.bucket_events(q, lst, bucket, perm, I.SHAPE["seg_len"], "q4")
                assert total == sum(values) % q, (label, perm)
                targets.update(t for t in ("first", "direct", "last") if ev.has("accumulate", "publish-" + t, w))
                if "skip" in needs:
                    assert ev.has("accumulate", M.SKIP, w), (label, perm)
                if "double" in needs:
                    assert _any(ev, w, *DOUBLES_Q4), (label, perm)
                if "cancel" in needs:
                    assert _any(ev, w, *CANCELS_Q4), (label, perm)
    assert len(offsets) >= 12 and targets == {"first", "direct", "last"}, (offsets, targets)


def test_quad_combine_model_order_and_hand_over():
    """the quad combine as msm_combine_q4_kernel does it: the first piece from first / direct / last, then t_lo + 1 .. t_hi one after the other
    (one lane group, no tree), and more than 64 pieces go to the heavy list; 64 further pieces still stay with the quad.  The bucket starts
    at offset 3: 13 + 64 * 16 = 1037 entries end segment 64, one more opens segment 65"""
    q = ORDERS["pallas"]
    for count, heavy in ((1037, False), (1038, True), (1026, False)):
        lst = [(1, 5, i) for i in range(3)] + [(2, 3, 3 + i) for i in range(count)] + [(3, 7, 3 + count)]
        ev = M.Events(q)
        pieces = M.accumulate(ev, lst, 16)
        total = M.combine_bucket(ev, 2, 3, 3 + count, pieces, 16, "q4")
        assert total == 3 * count % q
        assert ev.has(Q4, M.HANDOVER, (0, 2)) == heavy and ev.has(Q4, M.HEAD_LAST, (0, 2)) == (not heavy)
        assert ev.has("combine-heavy-tree", M.DOUBLE, (0, 2)) == heavy
        assert not ev.has("combine", M.DOUBLE) and not ev.has("combine-tree", M.DOUBLE)  # neither the one-lane nor the four-lane form
    # serial order: 13 P (last), then 16 P five times: the running sum meets no equal piece but the second (13 + 16 != 16); with an aligned
    # start every piece is 16 P and only the FIRST addition doubles -- the four-lane tree would double again at its last level
    lst = [(2, 3, i) for i in range(16 * 6)]
    ev = M.Events(q)
    assert M.combine_bucket(ev, 2, 0, 96, M.accumulate(ev, lst, 16), 16, "q4") == 3 * 96
    assert ev.at[(Q4, M.DOUBLE, 0, 2)] == 1 and ev.has(Q4, M.HEAD_FIRST, (0, 2))
