"""Big-integer model of the IPA generator collapse (csrc/ipafold.hip) for tests/test_foldplan.py and tests/test_gpu_ipa_collapse.py:
the shared scalars s_t, the signed sub-digit recoding and the bucket lists (csrc/foldplan.h) restated with Python integers, the walk of
one lane through its buckets over generators with KNOWN discrete logs, and the 128-byte record of a point (ctx.h ZREC).  Nothing here
calls the library."""
import lazy29_gen as lz

SIGN = 1 << 31


def shape(c):
    """table window c -> (c, W, w0, w1): windows of the table, bits of the low and of the high sub-window"""
    return c, 255 // c + 1, (c + 1) // 2, c // 2


def fold_scalars(u, order):
    """s_t = the product of u_j over the set bits (r - 1 - j) of t: the weight of G[i + t m] in G''[i] after the rounds 0 .. r - 1"""
    r = len(u)
    out = []
    for t in range(1 << r):
        s = 1
        for j in range(r):
            if (t >> (r - 1 - j)) & 1:
                s = s * u[j] % order
        out.append(s)
    return out


def recode(v, c, W, w0, w1):
    """the signed sub-digits of v by plain integer arithmetic: take w bits; a digit above 2^(w-1) becomes d - 2^w and adds one to what is
    left.  Returns ({(j, s): d != 0}, what is left after W windows -- non-zero: v does not fit the table)"""
    digits = {}
    for j in range(W):
        for s, w in ((0, w0), (1, w1)):
            d = v & ((1 << w) - 1)
            v >>= w
            if d > 1 << (w - 1):
                d -= 1 << w
                v += 1
            if d:
                digits[(j, s)] = d
    return digits, v


def bucket_of(s, d, w0):
    return ((1 << (w0 - 1)) if s else 0) + abs(d) - 1


def bucket_lists(scalars, c):
    """bucket row -> [(t, j, sign)] in the order the accumulation walks them: (t, j) ascending (asserted of fold_plan by test_foldplan.py)"""
    _, W, w0, w1 = shape(c)
    lists = {}
    for t, v in enumerate(scalars):
        digits, left = recode(v, c, W, w0, w1)
        assert left == 0
        for (j, s), d in sorted(digits.items()):
            lists.setdefault(bucket_of(s, d, w0), []).append((t, j, 1 if d > 0 else -1))
    return lists


def bucket_weight(b, c):
    """what a bucket's sum is multiplied by in G'': its digit times the shift of its sub-window"""
    _, _, w0, _ = shape(c)
    nb0 = 1 << (w0 - 1)
    return (b - nb0 + 1) << w0 if b >= nb0 else b + 1


def bucket_name(b, c):
    _, _, w0, _ = shape(c)
    nb0 = 1 << (w0 - 1)
    return f"bucket {b} (sub-window {1 if b >= nb0 else 0}, digit {b - nb0 + 1 if b >= nb0 else b + 1})"


def walk_lane(lists, logs, i, m, c, order):
    """lane i through every bucket, over the discrete logs of its generators (logs[x]: G[x] = logs[x] * generator; 0: the identity).
    Returns ({bucket: its sum as a scalar}, [description of every step that leaves the plain mixed addition])"""
    sums, events = {}, []
    for b in sorted(lists):
        acc, fresh, cancelled = 0, True, False
        for pos, (t, j, sign) in enumerate(lists[b]):
            p = sign * (logs[i + t * m] << (c * j)) % order
            where = f"{bucket_name(b, c)} entry {pos} (t = {t}, level {j})"
            if p == 0:
                events.append(f"{where}: identity record skipped")
            elif fresh:
                if cancelled:
                    events.append(f"{where}: starts the bucket again after a cancellation")
                acc, fresh, cancelled = p, False, False
            elif acc == p:
                events.append(f"{where}: doubling")
                acc = 2 * p % order
            elif (acc + p) % order == 0:
                events.append(f"{where}: cancellation")
                acc, fresh, cancelled = 0, True, True
            else:
                acc = (acc + p) % order
        if fresh:
            events.append(f"{bucket_name(b, c)}: ends fresh")
        sums[b] = acc
    return sums, events


def zrec_words(f, x_word, y_word):
    """the 32 words of the 128-byte record store_zrec (msm.hip) makes of an affine point given as its two stored 256-bit Montgomery words:
    fy_from_fe of each coordinate -- the reduction of word * (2^266 mod m), whose normalised limbs are unique (lazy29_gen from_fe) -- then
    x, y, the limb-wise negated y (limbs 0 .. 7 each), the three top limbs and five spare words; the identity (0, 0) is all zero"""
    def from_fe(w):
        assert 0 <= w < f.m
        r = lz.reduce_(f, w * ((1 << 266) % f.m), True)
        assert 0 <= r < f.m + (f.m >> 7)
        return lz.norm_limbs(r)
    x, y = from_fe(x_word), from_fe(y_word)
    ny = lz.neg_limbs(y)
    words = x[:8] + y[:8] + ny[:8] + [x[8], y[8], ny[8]] + [0] * 5
    return [v & 0xFFFFFFFF for v in words]
