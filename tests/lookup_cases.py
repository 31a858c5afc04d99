"""Cases for the lookup permutation (csrc/lookup.hip, halo2's `permute_expression_pair`) past one scan block and one 32-lookup chunk.

One generator for tests/test_lookup_cases.py (no GPU: the oracle on every case, and a check that each case reaches the part of the
file it is meant for) and tests/test_gpu_lookup_sizes.py (the device against the oracle, bit for bit).  Plain Python, canonical
integers, fixed seeds.  A case is

    Case(name, field, inputs, tables, usable_rows, rows, call, error, reach)

inputs / tables: one list of `rows` integers per lookup; only the first `usable_rows` take part, the rows behind them hold random
padding.  call: "single" (trh_lookup_permute_dev, one lookup, the columns cut to usable_rows or not as given) or "batch"
(trh_lookup_permute_batch_dev).  error: None, or the index of the lookup the call has to name when it fails.  reach: what the
case is meant to exercise, as data that test_lookup_cases.py checks with the rules restated below.

The constants and the three rules (varies, fast_key, tied) restate csrc/lookup.hip: if the file changes them, so must this.

Why there is no valid lookup with a tie in the input column alone.  A tie is two different values x, y of a column that agree in the
bits the fast path sorts by: limb k, the most significant limb that is not constant over the column, under the column's varying-bit
mask with its low digits cleared while 48 varying bits remain above them.  In a lookup that succeeds every input value occurs in the
table.  So every bit that varies in the input column varies in the table column: the table's key limb is the same or higher, and in
the same limb its mask has no fewer bits above any digit, so at least as many low digits are cleared.  x and y agree in every limb
above the input's key limb and differ only in the digits cleared there, hence they tie in the table as well.  The input-only tie
therefore exists only where y is missing from the table; that is the `input-only-tie` case, and it has to fail.
"""
import functools
import random
from typing import NamedTuple

import pasta as o

TILE, THREADS = 2048, 256
RADIX_BITS, RADIX, PASSES = 4, 16, 16
FAST_KEY_BITS = 48
CHUNK = 32                            # lookups per set of launches (lookup_permute_all_t)
RADIX_SCAN_BLOCK = THREADS * 8        # histogram words per trip of radix_scan_kernel; a column has RADIX words per tile
SUMS_SCAN_BLOCK = THREADS             # tile sums per trip of scan_sums_kernel
M64 = (1 << 64) - 1


class Case(NamedTuple):
    name: str
    field: str
    inputs: list
    tables: list
    usable_rows: int
    rows: int
    call: str
    error: object
    reach: dict


# ---- the rules of csrc/lookup.hip, restated ----
def tiles(n):
    return (n + TILE - 1) // TILE


def varies(col):
    """plane_varies_kernel: per limb, the bits in which the column is not constant"""
    acc, x0 = 0, col[0]
    for v in set(col):
        acc |= v ^ x0
    return [(acc >> (64 * k)) & M64 for k in range(4)]


def fast_key(var):
    """select_limb_kernel, step < 0: (limb the fast path sorts by, -1 for a constant column; the bits of it that are sorted by)"""
    k = max((j for j in range(4) if var[j]), default=-1)
    mask = var[k] if k >= 0 else 0
    d = 0
    while d < PASSES and bin(mask >> (RADIX_BITS * (d + 1))).count("1") >= FAST_KEY_BITS:
        mask &= ~((RADIX - 1) << (RADIX_BITS * d))
        d += 1
    return k, mask


def tied(col):
    """tie_check_kernel: two different values of the column agree in the bits the fast path sorted by"""
    k, mask = fast_key(varies(col))
    if k < 0:
        return False
    distinct = set(col)
    return len({(v >> (64 * k)) & mask for v in distinct}) < len(distinct)


def digits_seen(col):
    """per pass of the fast sort that is not an identity: the set of digit values the column holds"""
    k, mask = fast_key(varies(col))
    keys = {(v >> (64 * k)) & M64 for v in set(col)} if k >= 0 else set()
    return {p: {(key >> (RADIX_BITS * p)) & (RADIX - 1) for key in keys} for p in range(PASSES) if (mask >> (RADIX_BITS * p)) & (RADIX - 1)}


def limb_value(l0=0, l1=0, l2=0, l3=0):
    return l0 | (l1 << 64) | (l2 << 128) | (l3 << 192)


# ---- columns ----
KINDS = ["range", "wide", "ties", "low-ties", "one-run", "constant"]


def distinct_values(kind, rng, f, count):
    """the value set of one lookup, by character (the kinds of test_lookup_permuted_columns_batch)"""
    if kind == "range":       # a 16-bit range table: only the low limb varies, four passes of sixteen
        return rng.sample(range(1 << 16), min(count, 40000))
    if kind == "wide":        # spread over the whole field and its two ends: the top 48 varying bits separate them.  (The limb boundaries
        return [rng.randrange(f.m) for _ in range(count)] + [0, f.m - 1]  # 2^64, 2^128 ... share the top limb 0 with 0: those are "ties")
    if kind == "ties":        # one top limb, low limbs that differ: limb 2 is sorted by, and 40 values have limb 2 = 0
        top = rng.randrange(1, 1 << 60) << 192
        return ([top + rng.randrange(1 << 190) for _ in range(count)] + [top + (v << 64) + 7 for v in range(20)] + [top + 8 + v for v in range(20)]
                + [top + (1 << 64), top + (1 << 64) - 1, top + (1 << 128) - 1])
    if kind == "low-ties":    # spread-out values, some of which differ only in low bits of the top limb, below the 48 sorted by
        d = [rng.randrange(f.m >> 1) for _ in range(max(count, 64))]
        return d + [v ^ (1 << 192) for v in d[:20]] + [v ^ (0x5A5 << 192) for v in d[20:40]] + [(v ^ (3 << 192)) + 1 for v in d[40:50]]
    if kind == "one-run":
        return [5]
    assert kind == "constant"  # the input constant, the table with one more value
    return [12345, 99]


def column_pair(rng, f, distinct, n, rows, inputs_from=None, constant=False):
    """(input column, table column): the table is `distinct` cycled and shuffled, the inputs are drawn from it (or from `inputs_from`);
    the rows behind n hold random padding that no result may depend on"""
    assert len(distinct) <= n
    table = [distinct[i % len(distinct)] for i in range(n)]
    rng.shuffle(table)
    src = distinct if inputs_from is None else inputs_from
    inp = [src[0]] * n if constant else rng.choices(src, k=n)
    pad = [rng.randrange(f.m) for _ in range(rows - n)]
    return inp + pad, table + pad[::-1]


def kind_pair(kind, rng, f, n, rows, count=None):
    count = n // 3 if count is None else count
    return column_pair(rng, f, distinct_values(kind, rng, f, count), n, rows, constant=kind == "constant")


def batch_case(name, field, pairs, n, rows, error=None, **reach):
    return Case(name, field, [p[0] for p in pairs], [p[1] for p in pairs], n, rows, "batch", error, reach)


def single_case(name, field, pair, n, error=None, **reach):
    return Case(name, field, [pair[0]], [pair[1]], n, len(pair[0]), "single", error, reach)


# ---- the cases ----
BIG_N = SUMS_SCAN_BLOCK * TILE + TILE + 1   # 526 337: 258 tiles, the last of one element; 4128 histogram words, a third, partial trip


def big():
    """three lookups of 526 337 rows: scan_sums_kernel takes a second trip (258 tile sums) and radix_scan_kernel a third (4128 words),
    both with a carry; (a) wide, (b) 16-bit range, (c) one top limb: tied, redone in the general form at this size"""
    f, rng = o.FIELDS["fp"], random.Random(0xB16)
    n, rows = BIG_N, BIG_N + 7
    pairs = [kind_pair(kind, rng, f, n, rows) for kind in ("wide", "range", "ties")]
    return batch_case("big", "fp", pairs, n, rows, tiles=258, radix_scan_trips=3, sums_scan_trips=2, high_tile=[0, 1, 2], all_digits=[0, 1],
                      tied={2: "some"}, untied=[0, 1])


CHUNKS_TIED = {31: "ties", 32: "ties", 40: "low-ties", 66: "ties"}  # last of a chunk, first of the next, the middle, last of the call


def chunks():
    """67 lookups in one call: chunks of 32 + 32 + 3; n = 2349 (two tiles, the second ragged), padding behind usable_rows"""
    f, rng = o.FIELDS["fq"], random.Random(0xC4A2C5)
    n, rows, batch = TILE + 1 + 300, TILE + 1 + 300 + 51, 67
    kinds = [CHUNKS_TIED.get(i, KINDS[i % len(KINDS)]) for i in range(batch)]
    pairs = [kind_pair(kd, rng, f, n, rows, count=300) for kd in kinds]
    tied_at = {i: "some" for i, kd in enumerate(kinds) if kd in ("ties", "low-ties")}
    untied = [i for i in range(batch) if i not in tied_at]
    return batch_case("chunks", "fq", pairs, n, rows, batch_gt=64, tied=tied_at, untied=untied, kinds=kinds)


def sizes(field, n, kind):
    f, rng = o.FIELDS[field], random.Random(0x512E5 + n * 4 + (kind == "wide") * 2 + (field == "fq"))
    return single_case(f"sizes-{field}-{n}-{kind}", field, kind_pair(kind, rng, f, n, n), n, tiles=tiles(n), untied=[0])


def no_repeats(field, kind):
    """the inputs are a shuffle of a table of n distinct values: no repeated row, no left-over table value, S' = A'"""
    f, rng = o.FIELDS[field], random.Random(0x40BE9 + (field == "fq"))
    n = 2 * TILE + 904
    table = rng.sample(range(1 << 16), n) if kind == "range" else [rng.randrange(f.m) for _ in range(n)]
    assert len(set(table)) == n
    inp = list(table)
    rng.shuffle(inp)
    return single_case(f"no-repeats-{field}-{kind}", field, (inp, table), n, n_rep=0, untied=[0])


SPARSE_L1, SPARSE_L3 = 0x0123456789ABCDEF, 0x0FEDCBA987654321  # the constant limbs: not zero, limb 3 below that of the moduli


def sparse_limbs(variant):
    """values that vary in some limbs only, the others constant and not zero.  "0+2": limbs 0 and 2 vary and limb 2 is drawn from 64
    values, so the fast path (by limb 2) ties and the general form runs with two identity steps (limbs 1 and 3).  "1": limb 1 alone
    varies and separates: the fast path sorts by a middle limb.  "1-tied": limb 1 alone, some values differ only below its 48 sorted bits:
    the general form with three identity steps"""
    f, rng = o.FIELDS["fp"], random.Random(0x59A25E + len(variant))
    n = TILE + 500
    if variant == "0+2":
        l2 = [rng.getrandbits(64) for _ in range(64)]
        distinct = list({limb_value(rng.getrandbits(64), SPARSE_L1, rng.choice(l2), SPARSE_L3) for _ in range(700)})
        reach = dict(varying_limbs={0: (0, 2)}, tied={0: "both"})
    elif variant == "1":
        distinct = list({limb_value(7, rng.getrandbits(64), 9, SPARSE_L3) for _ in range(700)})
        reach = dict(varying_limbs={0: (1,)}, untied=[0])
    else:
        base = [rng.getrandbits(64) & ~0xFFFF for _ in range(300)]
        distinct = list({limb_value(7, b | rng.getrandbits(12), 9, SPARSE_L3) for b in base for _ in range(3)})
        reach = dict(varying_limbs={0: (1,)}, tied={0: "both"})
    return single_case(f"sparse-limbs-{variant}", "fp", column_pair(rng, f, distinct, n, n), n, **reach)


ALTERNATE_BITS = 0x5555555555555555


def sparse_mask(variant):
    """limb 3 constant, limb 2 the top varying limb.  "alternate": it varies in every other bit, 32 bits, nothing trimmed: every pass runs
    and meets four of the sixteen digit values.  "48+16": it varies in all 64 bits, so exactly the 48 bits above bit 16 are sorted by, and
    groups of values differ only in bits 0..15: a tie and a redo"""
    f, rng = o.FIELDS["fq"], random.Random(0x3A5C + len(variant))
    n = TILE + 700
    if variant == "alternate":
        distinct = list({limb_value(rng.getrandbits(64), rng.getrandbits(64), rng.getrandbits(64) & ALTERNATE_BITS, SPARSE_L3) for _ in range(800)})
        reach = dict(key={0: (2, ALTERNATE_BITS)}, digit_values={0: 4}, untied=[0])
    else:
        high = [rng.getrandbits(48) << 16 for _ in range(300)]
        distinct = list({limb_value(rng.getrandbits(64), rng.getrandbits(64), h | rng.getrandbits(16), SPARSE_L3) for h in high for _ in range(3)})
        reach = dict(key={0: (2, M64 & ~0xFFFF)}, tied={0: "both"})
    return single_case(f"sparse-mask-{variant}", "fq", column_pair(rng, f, distinct, n, n), n, **reach)


def table_only_tie(field):
    """20 table values have a partner that differs from them in bit 0 of the top limb, below the bits sorted by; the inputs are drawn from the
    values without the partners, which the fast key separates: only the table column reports the tie"""
    f, rng = o.FIELDS[field], random.Random(0x7AB1E + (field == "fq"))
    n = TILE + 333
    base = [rng.randrange(f.m >> 1) for _ in range(600)]
    partners = [v ^ (1 << 192) for v in base[:20]]
    return single_case(f"table-only-tie-{field}", field, column_pair(rng, f, base + partners, n, n, inputs_from=base), n, tied={0: "table-only"})


def input_only_tie(field):
    """the mirror image, which exists only as a failure (module docstring): the partners are among the inputs and not in the table"""
    f, rng = o.FIELDS[field], random.Random(0x1A9E7 + (field == "fq"))
    n = TILE + 333
    base = [rng.randrange(f.m >> 1) for _ in range(600)]
    partners = [v ^ (1 << 192) for v in base[:20]]
    inp, table = column_pair(rng, f, base, n, n)
    for i, v in enumerate(partners):
        inp[37 * i + 5] = v
    return single_case(f"input-only-tie-{field}", field, (inp, table), n, error=0, tied={0: "input-only"})


def missing(field, where):
    """one input value that is not in the table: "below" every table value, strictly "between" two of them, "above" all of them -- the miss
    branches of remove_from_table_kernel (lower bound inside the table with an unequal value: below, between; lower bound == n: above);
    "table-tail": the value is in the table only behind usable_rows, which has to fail; "input-tail": the value that is not in the table
    is among the inputs only behind usable_rows, which must not fail"""
    f, rng = o.FIELDS[field], random.Random(0x3155 + (field == "fq") + 8 * len(where))
    n, rows = TILE + 150, TILE + 150 + 40
    distinct = [v for v in (rng.randrange(1 << 200, f.m - (1 << 200)) for _ in range(500))]
    inp, table = column_pair(rng, f, distinct, n, rows)
    srt = sorted(distinct)
    absent = {"below": srt[0] // 2, "above": (srt[-1] + f.m) // 2}.get(where, (srt[250] + srt[251]) // 2)  # midpoints: far from every value in the bits sorted by
    assert absent not in distinct and 0 <= absent < f.m
    if where == "input-tail":
        inp[n + 3] = absent
        return single_case(f"missing-{field}-{where}", field, (inp, table), n, untied=[0])
    inp[n // 2] = absent
    if where == "table-tail":
        table[n + 5] = absent
    return single_case(f"missing-{field}-{where}", field, (inp, table), n, error=0, untied=[0], miss_branch={0: "above" if where == "above" else "inside"})


def missing_order(variant):
    """which lookup a failing call names: the FIRST in order, as halo2 fails at the first.  A lookup that is tied and misses a value is
    found by its redo, a plain one by the first pass.  "3+5": tied-and-missing at 3, plain missing at 5.  "35+37": the same pair in the
    second chunk.  "40": a tied-and-missing lookup alone at 40.  "37": a plain missing lookup alone in the second chunk"""
    f, rng = o.FIELDS["fp"], random.Random(0x0D3E + len(variant) * 16 + int(variant[0]))
    n, rows = 300, 310
    tied_at, plain_at, batch = {"3+5": (3, 5, 8), "35+37": (35, 37, 40), "40": (40, None, 41), "37": (None, 37, 39)}[variant]
    pairs = [list(kind_pair(("range", "wide")[i % 2], rng, f, n, rows, count=80)) for i in range(batch)]
    reach = dict(untied=[i for i in range(batch) if i != tied_at])
    if tied_at is not None:  # a table-only tie, and an input value far from every table value
        base = [rng.randrange(1 << 200, f.m >> 1) for _ in range(80)]
        inp, table = column_pair(rng, f, base + [v ^ (1 << 192) for v in base[:10]], n, rows, inputs_from=base)
        inp[n - 1] = 12345
        pairs[tied_at] = [inp, table]
        reach["tied"] = {tied_at: "table-only"}
    if plain_at is not None:
        pairs[plain_at][0][n // 3] = (f.m >> 1) + 12345  # not a table value, and far from all of them in the bits sorted by
    return batch_case(f"missing-order-{variant}", "fp", pairs, n, rows, error=tied_at if tied_at is not None else plain_at, **reach)


SIZES_N = [TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1]

BUILDERS = {"big": big, "chunks": chunks}
for _field in ("fp", "fq"):
    for _n in SIZES_N:
        for _kind in ("wide", "range"):
            BUILDERS[f"sizes-{_field}-{_n}-{_kind}"] = functools.partial(sizes, _field, _n, _kind)
    for _where in ("below", "between", "above", "table-tail", "input-tail"):
        BUILDERS[f"missing-{_field}-{_where}"] = functools.partial(missing, _field, _where)
    BUILDERS[f"table-only-tie-{_field}"] = functools.partial(table_only_tie, _field)
    BUILDERS[f"input-only-tie-{_field}"] = functools.partial(input_only_tie, _field)
BUILDERS["no-repeats-fp-wide"] = functools.partial(no_repeats, "fp", "wide")
BUILDERS["no-repeats-fq-range"] = functools.partial(no_repeats, "fq", "range")
for _v in ("0+2", "1", "1-tied"):
    BUILDERS[f"sparse-limbs-{_v}"] = functools.partial(sparse_limbs, _v)
for _v in ("alternate", "48+16"):
    BUILDERS[f"sparse-mask-{_v}"] = functools.partial(sparse_mask, _v)
for _v in ("3+5", "35+37", "40", "37"):
    BUILDERS[f"missing-order-{_v}"] = functools.partial(missing_order, _v)

NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    """the case of that name; built once per process, never modified by its users"""
    c = BUILDERS[name]()
    assert c.name == name and len(c.inputs) == len(c.tables) and all(len(col) == c.rows for col in c.inputs + c.tables)
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle on every lookup of the case, in order: ([(A', S') per lookup], None), or (None, index of the first lookup that fails)"""
    c = case(name)
    out = []
    for l, (inp, table) in enumerate(zip(c.inputs, c.tables)):
        try:
            out.append(o.permute_expression_pair(inp, table, c.usable_rows))
        except ValueError:
            return None, l
    return out, None
