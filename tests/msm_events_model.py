"""A discrete-log model of the MSM's stages (csrc/msm.hip, csrc/hostcombine.h), for tests/test_msm_events_model.py and the cases of
tests/msm_collision_cases.py.

Every base is a KNOWN multiple a_i of the generator, so a point is an integer mod the group order q (0: the identity), an addition is an
integer addition, and the exceptional cases of the group law are visible as integer relations: "same x" is k = +-a (k, a != 0), the doubling
k = a, the cancellation k = -a.  The model walks the stages in the order and with the geometry the kernels use -- the plan numbers
(c, seg_len, nbk, slice, the combine's lanes per bucket G, thread or quad form of the reduction) are parameters, asserted against
csrc/hostplan.h by tests/native/hostplan_test.cpp -- and returns which of these cases each stage meets:

    skip-identity          an identity base is passed over (accumulate, the small kernel's lanes)
    first                  a bucket's first point is taken as it is
    double / cancel        acc + p with acc = p / acc = -p, acc being ONE base (the second entry of a run)
    late-double / -cancel  the same with acc a sum of several entries
    restart-after-cancel   the first point taken after a cancellation in the same bucket (the `fresh` flag set again)
    stale-clear            an identity base arrives while acc still holds the previous bucket's limbs (the stale-limbs guard)
    add-identity           a full addition one of whose operands is the identity
    publish-first / -direct / -last    where msm_accumulate_seg_kernel stores a run
    head-first / -direct / -last       which of these msm_combine_q4_kernel takes as a bucket's first piece
    heavy-handover                     a bucket of more than 64 pieces is put on the heavy list instead of being stored
    identity-first / -middle / -last   a bucket of several pieces whose first / an inner / last piece is the identity (the quad combine)

The quad combine (G = "q4": msm_combine_q4_kernel, the dense route of the IPA opening) takes the first piece from `first`, `direct` or
`last`, adds the pieces t_lo + 1 .. t_hi one after the other (stage "combine-q4"), and hands a bucket of more than 64 pieces to
msm_combine_heavy_kernel.

Sensitivity.  Events(q, lose=(stage, event, where)) replaces the special-case branch of ONE event by "result lost": where the event is
met (at `where`, or anywhere with where = None) the value the branch should have produced becomes the junk point LOST -- a doubling that
was not taken, a cancellation that did not clear the accumulator, an identity that was added as if it were a point, a piece read from
the wrong place; a lost stale-clear keeps the previous bucket's value in the register.  A case is sensitive to an event when the
total changes under that replacement (tests/test_msm_events_model.py).

The order of the entries INSIDE a bucket is decided by atomic ranks on the device (the sort; `cursor` in msm_small_kernel) and is not
deterministic, so it is a parameter here: "asc" (by pair index), "desc", or a dict {(window, bucket): permutation}.

Signed recodings.  msm_recode_kernel takes raw = low c bits + carry and makes it negative when raw > 2^(c-1): a digit of magnitude EXACTLY
2^(c-1) stays positive (bucket nbk).  msm_small_kernel reads the digits of v + H, H = sum 15 * 32^j: digits in [-15, 16], +16 positive."""
from collections import Counter

SKIP, FIRST, DOUBLE, CANCEL = "skip-identity", "first", "double", "cancel"
LATE_DOUBLE, LATE_CANCEL, RESTART, STALE, ADD_ID = "late-double", "late-cancel", "restart-after-cancel", "stale-clear", "add-identity"
HEAD_FIRST, HEAD_DIRECT, HEAD_LAST, HANDOVER = "head-first", "head-direct", "head-last", "heavy-handover"
HEAVY_PIECES = 64
LOST = 0x1057_0000_0BAD_C0DE_0000_1057_0BAD_C0DE_1057  # the junk point of a lost result: far from every designed value and every filler
SMALL_C, SMALL_NBK = 5, 16


def num_windows(c):
    return 255 // c + 1


def recode_pipeline(s, c):
    """msm_recode_kernel: the signed digits of s, lowest window first"""
    mask, half, out, carry = (1 << c) - 1, 1 << (c - 1), [], 0
    for _ in range(num_windows(c)):
        raw = (s & mask) + carry
        s >>= c
        if raw > half:
            out.append(raw - (1 << c))
            carry = 1
        else:
            out.append(raw)
            carry = 0
    return out


def recode_small(s):
    """msm_small_kernel: digit j = bits [5 j, 5 j + 5) of s + H, minus 15"""
    W = num_windows(SMALL_C)
    v = s + sum((SMALL_NBK - 1) << (SMALL_C * j) for j in range(W))
    return [((v >> (SMALL_C * j)) & 31) - (SMALL_NBK - 1) for j in range(W)]


class Events:
    """what the stages met: a Counter over (stage, event), and the same per (stage, event, window, bucket) where a bucket is known"""

    def __init__(self, q, lose=None):
        self.q = q
        self.n = Counter()
        self.at = Counter()
        self.lose, self.lost = lose, 0  # the one event whose result is lost, and how often that happened

    def loses(self, stage, event, where=None):
        if self.lose is None or (stage, event) != tuple(self.lose[:2]):
            return False
        if self.lose[2] is not None and (where is None or tuple(self.lose[2]) != tuple(where)):
            return False
        self.lost += 1
        return True

    def note(self, stage, event, where=None):
        self.n[(stage, event)] += 1
        if where is not None:
            self.at[(stage, event) + tuple(where)] += 1

    def add(self, stage, x, y, where=None):
        """a full addition (xyzzz_add, q4_add, the host's padd)"""
        event = ADD_ID if x == 0 or y == 0 else DOUBLE if x == y else CANCEL if (x + y) % self.q == 0 else None
        if event:
            self.note(stage, event, where)
            if self.loses(stage, event, where):
                return LOST
        return (x + y) % self.q

    def has(self, stage, event, where=None):
        if where is None:
            return self.n[(stage, event)] > 0
        return self.at[(stage, event) + tuple(where)] > 0


def window_lists(q, a, digit_rows, flat_c=0, order="asc"):
    """{window: [(bucket, value, pair index)] in sorted order}.  digit_rows[i] = the digits of scalar i.  flat_c != 0: the fixed-base form -- ONE
    list (window 0) over the table entries 2^(c j) P_i, flat index j n + i"""
    n = len(a)
    per = {}
    for i, digs in enumerate(digit_rows):
        for j, d in enumerate(digs):
            if d == 0:
                continue
            v = a[i] % q if d > 0 else (-a[i]) % q
            if flat_c:
                per.setdefault(0, {}).setdefault(abs(d), []).append((j * n + i, v * pow(2, flat_c * j, q) % q))
            else:
                per.setdefault(j, {}).setdefault(abs(d), []).append((i, v))
    out = {}
    for j, buckets in per.items():
        lst = []
        for b in sorted(buckets):
            ent = sorted(buckets[b])
            if order == "desc":
                ent.reverse()
            elif isinstance(order, dict) and (j, b) in order:
                ent = [ent[k] for k in order[(j, b)]]
            lst += [(b, v, i) for i, v in ent]
        out[j] = lst
    return out


def bucket_ranges(lst):
    """{bucket: (start, end)} of a sorted list"""
    r = {}
    for p, (b, _, _) in enumerate(lst):
        s, _e = r.get(b, (p, p))
        r[b] = (s, p + 1)
    return r


def accumulate(ev, lst, seg_len, window=0, segments=None):
    """msm_accumulate_seg_kernel over one window's sorted list: one thread per segment of seg_len entries.  Returns (first, last, direct):
    {segment: value}, {segment: value}, {bucket: value}.  `reg` is the accumulator REGISTER: a publish does not clear it, `fresh` says that it
    holds nothing of the current bucket"""
    q, total = ev.q, len(lst)
    first, last, direct = {}, {}, {}
    for t in (range((total + seg_len - 1) // seg_len) if segments is None else segments):
        pos, stop = t * seg_len, min(t * seg_len + seg_len, total)
        if pos >= total:
            continue
        reg, is_first, fresh, terms, cancelled = 0, True, True, 0, False
        B = lst[pos][0]
        for p in range(pos, stop):
            b, v, _ = lst[p]
            if b != B:  # bucket finished: publish its run and start the next bucket
                if is_first:
                    first[t] = reg
                    ev.note("accumulate", "publish-first", (window, B))
                else:
                    direct[B] = LOST if ev.loses("accumulate", "publish-direct", (window, B)) else reg
                    ev.note("accumulate", "publish-direct", (window, B))
                is_first, fresh, terms, cancelled, B = False, True, 0, False, b
            w = (window, B)
            if v == 0:
                ev.note("accumulate", SKIP, w)
                if ev.loses("accumulate", SKIP, w):  # the identity record taken for a point
                    reg, fresh, terms = LOST, False, terms + 1
                elif fresh:
                    if reg:
                        ev.note("accumulate", STALE, w)
                        if ev.loses("accumulate", STALE, w):
                            continue  # the previous bucket's limbs stay in the register
                    reg = 0
            elif fresh:
                e = RESTART if cancelled else FIRST
                ev.note("accumulate", e, w)
                reg, fresh, terms = (LOST if ev.loses("accumulate", e, w) else v), False, 1
            elif reg == v:
                e = DOUBLE if terms == 1 else LATE_DOUBLE
                ev.note("accumulate", e, w)
                reg, terms = (LOST if ev.loses("accumulate", e, w) else 2 * v % q), terms + 1
            elif (reg + v) % q == 0:
                e = CANCEL if terms == 1 else LATE_CANCEL
                ev.note("accumulate", e, w)
                if ev.loses("accumulate", e, w):
                    reg, terms = LOST, terms + 1
                else:
                    reg, fresh, terms, cancelled = 0, True, 0, True
            else:
                reg, terms = (reg + v) % q, terms + 1
        w = (window, B)
        if is_first:
            first[t] = reg
            ev.note("accumulate", "publish-first", w)
        elif stop == total or lst[stop][0] != B:  # cur_end == stop
            direct[B] = LOST if ev.loses("accumulate", "publish-direct", w) else reg
            ev.note("accumulate", "publish-direct", w)
        else:
            last[t] = LOST if ev.loses("accumulate", "publish-last", w) else reg
            ev.note("accumulate", "publish-last", w)
    return first, last, direct


def combine_bucket(ev, b, S, E, pieces, seg_len, G, window=0):
    """msm_combine_kernel<G> (G = "q4": msm_combine_q4_kernel) / msm_combine_heavy_kernel for bucket b = entries [S, E) of the list"""
    first, last, direct = pieces
    t_lo, t_hi = S // seg_len, (E - 1) // seg_len
    w = (window, b)
    if S == t_lo * seg_len:
        head, choice = first[t_lo], HEAD_FIRST
    elif E <= (t_lo + 1) * seg_len:
        head, choice = direct[b], HEAD_DIRECT
    else:
        head, choice = last[t_lo], HEAD_LAST
    if G == "q4":
        if t_hi - t_lo > HEAVY_PIECES:
            ev.note("combine-q4", HANDOVER, w)
            if ev.loses("combine-q4", HANDOVER, w):
                return LOST  # neither kernel stores the bucket: whatever the buffer held
        else:
            ev.note("combine-q4", choice, w)
            acc = LOST if ev.loses("combine-q4", choice, w) else head
            if t_hi > t_lo and head == 0:
                ev.note("combine-q4", "identity-first", w)
            for t in range(t_lo + 1, t_hi + 1):  # one quad, the pieces one after the other
                if first[t] == 0:
                    ev.note("combine-q4", "identity-last" if t == t_hi else "identity-middle", w)
                acc = ev.add("combine-q4", acc, first[t], w)
            return acc
    if t_hi - t_lo > HEAVY_PIECES:  # one workgroup: thread 0 takes the head, the threads stride over the other pieces, LDS tree
        lanes = [0] * 256
        lanes[0] = head
        for i in range(256):
            for t in range(t_lo + 1 + i, t_hi + 1, 256):
                lanes[i] = ev.add("combine-heavy", lanes[i], first[t], w)
        st = 128
        while st:
            for i in range(st):
                lanes[i] = ev.add("combine-heavy-tree", lanes[i], lanes[i + st], w)
            st >>= 1
        return lanes[0]
    lanes = [0] * G
    lanes[0] = head
    for sub in range(G):
        for t in range(t_lo + 1 + sub, t_hi + 1, G):
            lanes[sub] = ev.add("combine", lanes[sub], first[t], w)
    off = G // 2
    while off:  # shuffle tree; only the lanes below `off` reach the result
        lanes = [ev.add("combine-tree", lanes[s], lanes[s + off], w) if s < off else lanes[s] for s in range(G)]
        off >>= 1
    return lanes[0]


def _tree(ev, stage, vals, top):
    s = top
    while s:
        for i in range(s):
            vals[i] = ev.add(stage, vals[i], vals[i + s])
        s >>= 1
    return vals[0]


def reduce_window(ev, buckets, nbk, m, quad):
    """msm_reduce_kernel (quad: msm_reduce_q4_kernel) and the window-sum kernel behind it.  buckets: {bucket id: value}; slices of m buckets;
    blocks of 256 threads (64 quads).  Slices and blocks that hold nothing are skipped: they add identities to identities"""
    q = ev.q
    tpw = nbk // m
    per_block = 64 if quad else 256
    nblocks = (tpw + per_block - 1) // per_block
    totals = {}
    for t in sorted({(b - 1) // m for b, v in buckets.items() if v}):
        B = [buckets.get(t * m + k + 1, 0) for k in range(m)]
        live = [k for k in range(m) if B[k]]
        if not quad and m >= 16 and len(live) <= 4:  # one shared double-and-add over the ids of the live buckets
            sc, base_id = 0, t * m + 1
            for i in range((base_id + live[-1]).bit_length() - 1, -1, -1):
                sc = 2 * sc % q
                for k in live:
                    if ((base_id + k) >> i) & 1:
                        sc = ev.add("reduce-live", sc, B[k])
            totals[t] = sc
            continue
        run = acc = 0
        for k in range(m - 1, -1, -1):
            run = ev.add("reduce-run", run, B[k])
            acc = ev.add("reduce-acc", acc, run)
        off = t * m
        if off:
            sc = 0
            for i in range(off.bit_length() - 1, -1, -1):
                sc = 2 * sc % q
                if (off >> i) & 1:
                    sc = ev.add("reduce-off", sc, run)
            acc = ev.add("reduce-final", acc, sc)
        totals[t] = acc
    partials = [0] * nblocks
    for blk in sorted({t // per_block for t in totals}):
        vals = [totals.get(blk * per_block + i, 0) for i in range(per_block)]
        partials[blk] = _tree(ev, "reduce-tree", vals, per_block // 2)
    vals = [0] * per_block
    for k, p in enumerate(partials):
        if p:
            vals[k % per_block] = ev.add("window-sum", vals[k % per_block], p)
    top = per_block // 2
    while top > 1 and top >= nblocks:
        top >>= 1
    return _tree(ev, "window-sum-tree", vals + [0] * per_block, top)


def horner(ev, sums, W, c):
    """hostcombine::horner: the window sums, top window first"""
    acc = 0
    for j in range(W - 1, -1, -1):
        if acc:
            acc = acc * (1 << c) % ev.q
        acc = ev.add("horner", acc, sums.get(j, 0), (j,))
    return acc


def run_pipeline(q, a, s, c, seg_len, m, G=1, quad=False, table=False, order="asc"):
    """the per-window pipeline (table: the fixed-base form, one bucket set) -> (Events, result)"""
    lists = window_lists(q, a, [recode_pipeline(x, c) for x in s], flat_c=c if table else 0, order=order)
    return run_lists(q, lists, c, seg_len, m, G, quad, table)


def run_lists(q, lists, c, seg_len, m, G=1, quad=False, table=False, lose=None):
    """run_pipeline behind the sort: `lists` as window_lists makes them; lose: see Events"""
    ev = Events(q, lose)
    nbk = 1 << (c - 1)
    sums = {}
    for j, lst in lists.items():
        pieces = accumulate(ev, lst, seg_len, j)
        buckets = {b: combine_bucket(ev, b, S, E, pieces, seg_len, G, j) for b, (S, E) in bucket_ranges(lst).items()}
        sums[j] = reduce_window(ev, buckets, nbk, m, quad)
    return ev, horner(ev, sums, 1 if table else num_windows(c), c)


def bucket_events(q, lst, bucket, perm, seg_len, G, window=0):
    """the accumulate and combine events of ONE bucket of a sorted list with the bucket's entries permuted: only the segments the bucket
    touches are walked.  Returns (Events, the bucket's sum)"""
    ev = Events(q)
    S, E = bucket_ranges(lst)[bucket]
    lst = lst[:S] + [lst[S + k] for k in perm] + lst[E:]
    pieces = accumulate(ev, lst, seg_len, window, segments=range(S // seg_len, (E - 1) // seg_len + 1))
    return ev, combine_bucket(ev, bucket, S, E, pieces, seg_len, G, window)


def small_window(ev, lst, window=0):
    """one workgroup of msm_small_kernel: 16 lanes per bucket split its list evenly (mixed additions), a tree over the 16 lanes, the suffix
    scan over the 16 bucket sums and the tree over the suffix sums.  The quad form adds the same operands at the same levels"""
    q = ev.q
    rng = bucket_ranges(lst)
    sums = [0] * SMALL_NBK
    for b, (S, E) in rng.items():
        cnt, w = E - S, (window, b)
        lanes = []
        for sl in range(16):
            acc, terms = 0, 0
            for e in range(S + cnt * sl // 16, S + cnt * (sl + 1) // 16):
                v = lst[e][1]
                if v == 0:
                    ev.note("small-lane", SKIP, w)
                elif acc == 0:
                    ev.note("small-lane", RESTART if terms else FIRST, w)
                    acc, terms = v, terms + 1
                elif acc == v:
                    ev.note("small-lane", DOUBLE if terms == 1 else LATE_DOUBLE, w)
                    acc, terms = 2 * v % q, terms + 1
                elif (acc + v) % q == 0:
                    ev.note("small-lane", CANCEL if terms == 1 else LATE_CANCEL, w)
                    acc, terms = 0, terms + 1
                else:
                    acc, terms = (acc + v) % q, terms + 1
            lanes.append(acc)
        o = 8
        while o:  # level 8 is a plain addition in both forms; 4, 2, 1 are the quad form's pair, and its two shuffles
            for sl in range(o):
                lanes[sl] = ev.add("small-tree-8" if o == 8 else "small-tree", lanes[sl], lanes[sl + o], w)
            o >>= 1
        sums[b - 1] = lanes[0]
    o = 1
    while o < SMALL_NBK:  # suffix scan: S_b = sum of the buckets >= b
        sums = [ev.add("small-scan", sums[t], sums[t + o], (window,)) if t + o < SMALL_NBK else sums[t] for t in range(SMALL_NBK)]
        o <<= 1
    return _tree(ev, "small-sum", sums, SMALL_NBK // 2)


def run_small(q, a, s, order="asc"):
    """msm_small_kernel and the host Horner -> (Events, result)"""
    ev = Events(q)
    lists = window_lists(q, a, [recode_small(x) for x in s], order=order)
    sums = {j: small_window(ev, lst, j) for j, lst in lists.items()}
    return ev, horner(ev, sums, num_windows(SMALL_C), SMALL_C)
