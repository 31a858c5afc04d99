"""Cases for the host-pointer staging rings (csrc/hostio.hip, csrc/copypool.h) at slot sizes where the rings wrap, and a model of what
each case reaches.

One table for tests/test_hostio_cases.py (no GPU: the model against the real chunk_plan, and the conditions every case has to meet on
its inputs) and tests/test_gpu_hostio_rings.py (the device against references that are not the code under test, bit for bit, and the
byte counters of trh_io_stats against the values computed HERE).  Plain Python over row ranges: a vector is described by the ranges of
its rows (32-byte field elements) that are not zero; `build` makes the array and checks that the description is true of it.

The model restates, from the comments of the two files and from what they are seen to do:

  chunk_plan    how ONE transfer is cut for a ring of `slot`-byte slots: full slots in the middle; a short head (2 MiB, then 6 MiB) and a
                short tail (6 MiB, then 2 MiB) where asked for and where the slot is larger than that piece; in front of everything else
                that is cut off the end, a `tiny_tail` piece (256 KiB) for transfers whose zero chunks are elided.  Checked against the
                real function through tests/native/chunkplan_dump.cpp.
  stage_h2d     chunk after chunk into slot `used % NS`, where `used` counts the chunks that took a slot: a chunk that is zero throughout
                (zero_elide) becomes a memset on the device, takes no slot and does not advance the ring.  With `speculate`, a chunk of
                1 MiB or more whose probed lines (probe_lines) are all zero is cleared on the device unread; the caller reads it through
                afterwards and starts over without guessing if it was not zero.
  stage_d2h     chunk i lands in slot i % NS; NS chunks are issued ahead of the one being copied out.
  msm_host_tiled / best_fft_host / the batch forms: which of the flags above each passes.

Nothing here reads the library: the expected h2d_zero_bytes of every case is this model's.

Where the restatement comes from.  The thresholds of chunk_plan (`left > 2 * small`, `left > mid + small`, `bytes > 4 * tiny_tail`), the
order in which it cuts (tiny tail, head, tail) and the order of the two tests in stage_h2d (the guess before the scan) are in no comment:
they were read from the code, and chunk_plan and h2d_schedule follow its control flow.  For chunk_plan the comparison with the real
function makes that harmless.  The slot schedule has no such check: a misreading of stage_h2d shared by the model and its author would
show only in the counters the GPU tests compare (h2d_zero_bytes, exact) and in the results.  The probe set, the rule that a zero chunk
takes no slot, NS chunks ahead on the way down, the parts of the pool and the flags per MSM range are from the comments."""
import bisect
import functools
from typing import NamedTuple

import numpy as np

KiB, MiB = 1 << 10, 1 << 20
ROW = 32                      # bytes of a field element / scalar
NS = 4                        # Stage::NS: pinned slots per direction
SMALL, MID = 2 * MiB, 6 * MiB  # the graded head / tail pieces of chunk_plan
TINY_TAIL = 256 * KiB         # what stage_h2d passes as tiny_tail for a lone transfer with zero_elide
LINE, PROBE_STRIDE = 64, 64 * KiB
GUESS_MIN_CHUNK = MiB         # chunks below this are never probed
GUESS_MIN_BYTES = 8 * MiB     # best_fft_host speculates from this size on
POOL_MIN = MiB                # CopyPool::copy splits transfers of at least this size over its threads
RING_TURNS = 2 * NS + 1       # chunks that reuse every slot of a ring at least twice

# (stage_slot_mb, copy_threads; None = the library's default, -1).  1 MiB: ungraded plans; 3 MiB: slot > SMALL but not > MID; 7 MiB: both.
# copy_threads 0, 1, 62 and the default give CopyPool::copy 1, 2, 63 and (on a host with 16 hardware threads or more) 5 parts.
OPTION_SETS = ((1, 0), (1, None), (3, 1), (7, 62))


def option_env(slot_mb, threads):
    env = {"TRH_STAGE_SLOT_MB": str(slot_mb)}
    if threads is not None:
        env["TRH_COPY_THREADS"] = str(threads)
    return env


def option_id(slot_mb, threads):
    return f"slot{slot_mb}-threads{'default' if threads is None else threads}"


# ---- the rules of csrc/copypool.h and csrc/hostio.hip, restated -------------------------------------------------------------------
def chunk_plan(nbytes, slot, head, tail, tiny_tail=0):
    if not slot or not nbytes:
        return []
    left, front, end = nbytes, [], []          # `end`: the pieces cut off the end, outermost first
    if tiny_tail and tiny_tail < slot and left > 4 * tiny_tail:
        end.append(tiny_tail)
        left -= tiny_tail
    if slot > SMALL:                            # slots no larger than the short piece are not graded
        for wanted, pieces in ((head, front), (tail, end)):
            if wanted and left > 2 * SMALL:
                pieces.append(SMALL)
                left -= SMALL
                if slot > MID and left > MID + SMALL:
                    pieces.append(MID)
                    left -= MID
    middle = [slot] * (left // slot) + ([left % slot] if left % slot else [])
    return front + middle + end[::-1]


def probe_lines(size):
    """probe_zero: the chunk-relative offsets of the 64-byte lines it reads -- the first, the last, one at every multiple of 64 KiB"""
    return sorted({0, size - LINE} | set(range(PROBE_STRIDE, size - LINE + 1, PROBE_STRIDE)))


def pool_parts(size, threads):
    """CopyPool::copy: the (offset, length) parts a transfer is scanned and copied in; one part below POOL_MIN or without threads"""
    if size < POOL_MIN or not threads:
        return [(0, size)]
    parts = min(threads, 62) + 1
    per = (-(-size // parts) + 4095) & ~4095
    return [(lo, min(per, size - lo)) for lo in range(0, size, per)]


class Rows:
    """the rows of a vector that are not zero, as sorted disjoint half-open ranges"""

    def __init__(self, ranges):
        self.ranges = sorted((int(a), int(b)) for a, b in ranges if b > a)
        self.starts = [a for a, _ in self.ranges]
        assert all(b <= c for (_, b), (c, _) in zip(self.ranges, self.ranges[1:]))

    def any(self, lo_byte, hi_byte):
        """is any byte range [lo_byte, hi_byte) row of the vector not zero?  (whole rows: every cut of the model is a multiple of 32)"""
        assert lo_byte % ROW == 0 and hi_byte % ROW == 0
        lo, hi = lo_byte // ROW, hi_byte // ROW
        i = bisect.bisect_right(self.starts, lo) - 1
        if i >= 0 and self.ranges[i][1] > lo:
            return True
        return i + 1 < len(self.ranges) and self.ranges[i + 1][0] < hi


class Chunk(NamedTuple):
    off: int      # byte offset in the transfer
    size: int
    kind: str     # "copy": through a slot; "zero": seen to be zero, memset; "guess": probed as zero, memset, verified later
    slot: object  # ring slot of a "copy" chunk, else None


def h2d_schedule(rows, nbytes, slot, *, head, tail, tiny_tail=0, zero_elide=False, speculate=False, base=0, used=0):
    """stage_h2d on pageable memory.  base: byte offset of the transfer in the vector `rows` describes; used: chunks that took a slot
    before this transfer.  Returns (chunks, used afterwards)."""
    out, off = [], 0
    for cur in chunk_plan(nbytes, slot, head, tail, tiny_tail):
        lo = base + off
        if speculate and cur >= GUESS_MIN_CHUNK and not any(rows.any(lo + l, lo + l + LINE) for l in probe_lines(cur)):
            out.append(Chunk(off, cur, "guess", None))
        elif zero_elide and not rows.any(lo, lo + cur):
            out.append(Chunk(off, cur, "zero", None))
        else:
            out.append(Chunk(off, cur, "copy", used % NS))
            used += 1
        off += cur
    assert off == nbytes
    return out, used


def d2h_schedule(nbytes, slot):
    """stage_d2h into pageable memory as a list of steps: ("issue", chunk, slot) queues the DMA of a chunk into a slot, ("drain", chunk,
    slot) waits for it and copies the slot out"""
    plan = chunk_plan(nbytes, slot, False, True)
    steps, issued = [], 0
    for k in range(len(plan)):
        while issued < len(plan) and issued < k + NS:
            steps.append(("issue", issued, issued % NS))
            issued += 1
        steps.append(("drain", k, k % NS))
    return plan, steps


def msm_host_cuts(host_bases, n):
    """csrc/hostplan.h: host bases -- one range up to 2^21 pairs, above that equal ranges of about 2^20; resident bases -- one range up
    to 3 * 2^21, above that 2^21, 2^22 and the rest"""
    if host_bases and n > 1 << 21:
        ranges = -(-n // (1 << 20))
        length = -(-n // ranges)
        return list(range(0, n, length)) + [n]
    if not host_bases and n > 3 << 21:
        return [0, 1 << 21, 3 << 21, n]
    return [0, n]


def summary(chunks):
    kinds = [c.kind for c in chunks]
    used = [i for i, k in enumerate(kinds) if k == "copy"]
    return {
        "chunks": len(chunks), "used": len(used), "elided": len(chunks) - len(used),
        "zero_bytes": sum(c.size for c in chunks if c.kind != "copy"),
        # an elided chunk between two that took a slot: the ring index stands still while the transfer moves on
        "between": any(kinds[i] != "copy" for i in range(used[0], used[-1])) if used else False,
    }


def best_fft_model(rows, log_n, slot):
    """best_fft_host on pageable memory: the upload with zero elision (and, from 8 MiB on, the guess), the restart when a guess was wrong
    (the dropped pass leaves the counters), the download"""
    nbytes = ROW << log_n
    flags = dict(head=True, tail=True, tiny_tail=TINY_TAIL, zero_elide=True)
    first, _ = h2d_schedule(rows, nbytes, slot, speculate=nbytes >= GUESS_MIN_BYTES, **flags)
    wrong = [c for c in first if c.kind == "guess" and rows.any(c.off, c.off + c.size)]
    final = h2d_schedule(rows, nbytes, slot, **flags)[0] if wrong else first
    down, steps = d2h_schedule(nbytes, slot)
    s = summary(final)
    return {"first": first, "final": final, "restart": bool(wrong), "guessed": sum(c.kind == "guess" for c in first), "down": down, "down_steps": steps,
            "h2d_bytes": nbytes, "d2h_bytes": nbytes, "h2d_zero_bytes": s["zero_bytes"], **{k: s[k] for k in ("used", "elided", "between")}}


def mixed_chunks(rows, chunks, threads):
    """chunks of a schedule that go through a slot and hold data, then zeros to their end; with the parts of CopyPool::copy that are zero
    throughout (skipped by the thread that scanned them, cleared afterwards) next to parts that are not"""
    out = []
    for c in chunks:
        if c.kind != "copy":
            continue
        filled = [rows.any(c.off + lo, c.off + lo + ROW) for lo in (0, c.size - ROW)]
        if filled != [True, False]:
            continue
        parts = [rows.any(c.off + lo, c.off + lo + ln) for lo, ln in pool_parts(c.size, threads)]
        out.append((c, parts.count(False) if any(parts) else 0))
    return out


def msm_model(rows, n, slot, host_bases):
    """msm_host_tiled: per range the scalars with zero elision (the first range as a lone transfer -- head graded, tail graded only where
    the call is one range over resident bases -- every later range as part of a batch: full slots, no tiny tail), then the range's bases
    (64 B per pair, part of a batch, never elided) on the same upload ring"""
    cuts = msm_host_cuts(host_bases, n)
    lone = len(cuts) == 2
    used, transfers, zero = 0, [], 0
    for t, (a, b) in enumerate(zip(cuts, cuts[1:])):
        first = t == 0
        sc, used = h2d_schedule(rows, (b - a) * ROW, slot, head=first, tail=first and lone and not host_bases, tiny_tail=TINY_TAIL if first else 0,
                                zero_elide=True, base=a * ROW, used=used)
        transfers.append(("scalars", sc))
        zero += summary(sc)["zero_bytes"]
        if host_bases:
            bs, used = h2d_schedule(FULL, (b - a) * 2 * ROW, slot, head=False, tail=False, used=used)
            transfers.append(("bases", bs))
    return {"ranges": len(cuts) - 1, "transfers": transfers, "h2d_bytes": n * ROW * (3 if host_bases else 1), "h2d_zero_bytes": zero, "used": used}


FULL = Rows([(0, 1 << 40)])


# ---- vectors ---------------------------------------------------------------------------------------------------------------------
class Vec(NamedTuple):
    name: str
    n: int          # rows
    seed: int
    ranges: tuple   # rows that hold data (synth.field_elements(seed, n) at the same index); every other row is zero

    @property
    def rows(self):
        return Rows(self.ranges)


def build(vec):
    """the (n, 4) uint64 array `vec` describes"""
    from tiny_ram_halo2_amd import synth
    a = np.zeros((vec.n, 4), dtype=np.uint64)
    for lo, hi in vec.ranges:
        a[lo:hi] = synth.field_elements(vec.seed, hi - lo, start=lo)
        assert a[lo:hi].any(axis=1).all()   # every described row is not zero
    return a


def with_row(vec, name, row):
    return Vec(name, vec.n, vec.seed, tuple(sorted(vec.ranges + ((row, row + 1),))))


# ---- (a) single transfers past several ring turns ----------------------------------------------------------------------------------
def ring_log_ns(slot_mb):
    """log_n = 18 everywhere.  A ring is reused twice from RING_TURNS chunks on: the upload of 8 MiB in 1 MiB slots makes exactly that
    many (seven full slots, 768 KiB and the tiny tail), its download only eight, so 1 MiB slots get log_n = 19 too; 3 MiB slots need
    log_n = 20 (13 up, 11 down); at 7 MiB log_n = 20 makes 8 up and 6 down, so log_n = 21 (12 and 10) joins it."""
    return {1: (18, 19), 3: (18, 20), 7: (18, 20, 21)}[slot_mb]


# which ring a case turns at least twice (RING_TURNS chunks), per (slot MiB, log_n).  The sizes with () are the issue's own: they put the
# graded plans (2 MiB pieces at 3 MiB slots, 6 MiB pieces at 7 MiB) through the ring without a second turn.
RING_STRESS = {(1, 18): ("up",), (1, 19): ("up", "down"), (3, 18): (), (3, 20): ("up", "down"), (7, 18): (), (7, 20): (), (7, 21): ("up", "down")}


def ring_cases(slot_mb):
    return [(f"ring-{field}-{log_n}", field, Vec(f"full{log_n}", 1 << log_n, 0xA100 + log_n + (field == "fq"), ((0, 1 << log_n),)))
            for log_n in ring_log_ns(slot_mb) for field in ("fp", "fq")]


# ---- (a'), (d') the same uploads while the stream is held back --------------------------------------------------------------------
# The host fills a 1 MiB slot in about 30 us and the DMA engine empties it in 18: on an idle device the DMA that last read a slot is long
# over when the slot comes round again, and the wait on the slot's event never has to wait.  The held cases queue device work on the
# context first (HELD_REPEATS transforms of 2^HELD_LOG_N elements through trh_ntt_dev, not waited for): the staging streams join the
# context's order, so every DMA of the upload queues behind that work while the host goes on filling slots -- the event wait on a reused
# slot is then the only thing that keeps chunk k + NS out of the slot chunk k still sits in.
HELD_LOG_N, HELD_REPEATS = 24, 8
HELD_MSM_LOG_N = 20


def held_cases(slot_mb):
    """(name, kind, field or None, vector): the largest ring case of each field, and one MSM over resident bases"""
    top = max(ring_log_ns(slot_mb))
    out = [("held-" + name, "fft", field, vec) for name, field, vec in ring_cases(slot_mb) if vec.n == 1 << top]
    out.append((f"held-msm-{HELD_MSM_LOG_N}-random", "msm", None, Vec("random", 1 << HELD_MSM_LOG_N, 0xD400 + HELD_MSM_LOG_N, ((0, 1 << HELD_MSM_LOG_N),))))
    return out


# ---- (b) zero elision and speculation ------------------------------------------------------------------------------------------
ELIDE_LOG_N = 18              # the smallest size at which best_fft_host speculates
BLIND_ROWS = 5
HIDDEN_KINDS = ("after-line", "before-line", "block-end", "tiny-tail", "unprobed")


@functools.lru_cache(None)
def elide_vectors():
    n = 1 << ELIDE_LOG_N
    eighth = n // 8
    return {
        "padded": Vec("padded", n, 0xB200, ((0, eighth),)),                                  # what coeff_to_extended hands over
        "zero": Vec("zero", n, 0xB201, ()),
        "blinded": Vec("blinded", n, 0xB202, ((0, eighth), (n - BLIND_ROWS, n))),           # a witness column: what tiny_tail exists for
        # the data ends inside a chunk of every plan, and not on a part boundary of the copy pool
        "ragged": Vec("ragged", n, 0xB203, ((0, eighth + n // 32 + 5), (n - BLIND_ROWS, n))),
    }


def hidden_rows(slot_mb):
    """kind -> row of the one element hidden in the padding of the `padded` vector, chosen from the upload plan at this slot size.
    `guessed`: the chunks of the plan that probe as zero on `padded`."""
    slot, n = slot_mb * MiB, 1 << ELIDE_LOG_N
    first = best_fft_model(elide_vectors()["padded"].rows, ELIDE_LOG_N, slot)["first"]
    guessed = [c for c in first if c.kind == "guess"]
    c = guessed[len(guessed) // 2]
    inner = c.off + 3 * PROBE_STRIDE                     # a probed line that is neither the chunk's first nor next to its last
    out = {
        "after-line": (inner + LINE) // ROW,            # the 32 bytes right after a probed line
        "before-line": inner // ROW - 1,                # the 32 bytes right before one
        "block-end": (c.off + c.size - PROBE_STRIDE) // ROW - 1,   # last element of the chunk's second-to-last 64 KiB block
        "tiny-tail": (n * ROW - TINY_TAIL // 2) // ROW + 1,
    }
    small = [c for c in first if c.size < GUESS_MIN_CHUNK and c.size != TINY_TAIL]
    if small:                                           # at 7 MiB slots the plan of 8 MiB has no such chunk
        out["unprobed"] = (small[0].off + small[0].size // 2) // ROW + 3
    return out


def hidden_vectors(slot_mb):
    padded = elide_vectors()["padded"]
    return {kind: with_row(padded, "hidden-" + kind, row) for kind, row in hidden_rows(slot_mb).items()}


def elide_cases(slot_mb):
    """(name, field, vector, repeat): `repeat` vectors run twice in a row and are followed by the plain padded vector"""
    out = [(f"elide-{v.name}", ("fp", "fq")[i % 2], v, False) for i, v in enumerate(elide_vectors().values())]
    out += [(f"elide-{v.name}", ("fq", "fp")[i % 2], v, True) for i, v in enumerate(hidden_vectors(slot_mb).values())]
    return out


# ---- (c) pipelines ---------------------------------------------------------------------------------------------------------------
def group_for(bytes_per_column):
    """columns per pipeline item: the smallest power of two, at most 64, that makes 32 MiB"""
    g = 1
    while g < 64 and g * bytes_per_column < 32 * MiB:
        g <<= 1
    return g


class Batch(NamedTuple):
    name: str
    field: str
    log_n: int
    count: int
    pinned: dict    # column -> "alloc" (trh_host_alloc) or "register" (trh_host_register)
    zero: tuple     # columns that are zero throughout


BATCHES = (
    Batch("batch-17", "fp", 17, 29, {8: "alloc", 12: "register", 15: "alloc"}, (3,)),
    Batch("batch-12", "fq", 12, 131, {}, ()),
)
DOMAIN = {"field": "fp", "j": 6, "k": 11, "count": 70}


def batch_model(b, slot):
    nbytes = ROW << b.log_n
    group = group_for(nbytes)
    items = [list(range(g0, min(g0 + group, b.count))) for g0 in range(0, b.count, group)]
    # the helper thread of host_pipeline: one chunk per pinned segment, ceil(bytes / slot) ring chunks per pageable one, one counter
    # (issue_ctr) over both kinds
    down = [[1 if col in b.pinned else -(-nbytes // slot) for col in item] for item in items]
    return {"group": group, "items": items, "down_chunks": down, "edges": sorted({i for item in items for i in (item[0], item[-1])}),
            "h2d_bytes": b.count * nbytes, "d2h_bytes": b.count * nbytes, "h2d_zero_bytes": 0}   # part of a batch: nothing is elided


# ---- (d) MSM uploads -------------------------------------------------------------------------------------------------------------
def msm_vectors(log_n):
    n = 1 << log_n
    chunk = MiB // ROW            # rows of a 1 MiB chunk: a boundary of every plan below lies on a multiple of 256 KiB
    return [
        Vec("random", n, 0xD400 + log_n, ((0, n),)),
        Vec("run-aligned", n, 0xD410 + log_n, ((0, chunk), (n - chunk // 4, n)) if n == 2 * chunk else ((0, 2 * chunk), (5 * chunk, n))),
        Vec("run-mid-chunk", n, 0xD420 + log_n, ((0, chunk // 2 + 7), (n - chunk // 4 - 9, n))),
        Vec("run-to-last-8", n, 0xD430 + log_n, ((n - 8, n),)),
    ]


MSM_LOG_NS = (16, 18)
SPLIT_N = (1 << 21) + 1       # host bases: three ranges
SPLIT_OPTIONS = (1, None)


@functools.lru_cache(None)
def split_vector():
    """2^12 scalars that are not zero, 256 in each of 16 blocks of 2^15 rows spread over the three ranges"""
    from tiny_ram_halo2_amd import synth
    block, rows = 1 << 15, []
    for i, b in enumerate(range(1, SPLIT_N // block, 4)):
        pick = synth.splitmix64_stream(0xD500 + i, 0, 4096) % np.uint64(block)
        rows += [b * block + int(r) for r in sorted(set(pick.tolist()))[:256]]
    rows[-1] = SPLIT_N - 1        # the ragged last range's last pair takes part
    assert len(set(rows)) == 1 << 12
    return Vec("split", SPLIT_N, 0xD5FF, tuple((r, r + 1) for r in sorted(set(rows))))


def msm_cases(slot_mb, threads):
    """(name, vector, host_bases)"""
    out = [(f"msm-{log_n}-{v.name}", v, False) for log_n in MSM_LOG_NS for v in msm_vectors(log_n)]
    out += [(f"multiexp-16-{v.name}", v, True) for v in msm_vectors(16)[:2]]
    if (slot_mb, threads) == SPLIT_OPTIONS:
        out.append(("multiexp-split", split_vector(), True))
    return out


COMMIT = {"curve": "vesta", "n": 1 << 12, "batches": (17, 40)}

# ---- (e) the down ring shared with the hand-over -----------------------------------------------------------------------------------
HANDOVER = {"options": (1, None), "group": [0, 0], "n": 1 << 20, "fft_log_n": 18}


def case_names(slot_mb, threads):
    """every line the child of this option set has to print"""
    names = [c[0] for c in ring_cases(slot_mb)] + [c[0] for c in held_cases(slot_mb)]
    for name, _, _, repeat in elide_cases(slot_mb):
        names += [name, name + "-again", name + "-then-padded"] if repeat else [name]
    names += [b.name for b in BATCHES] + ["domain-extended", "domain-blocks"]
    names += [c[0] for c in msm_cases(slot_mb, threads)]
    names += [f"commit-{b}" for b in COMMIT["batches"]]
    return names
