"""The memory-consistency table as Python integers: what trh_mem_table_dev (csrc/memtable.hip) and csrc/memtable.h must compute, written
from the table's description and from nothing else.  No device, no numpy.

Inputs: word_bits (even, 2 .. 32), a tape of t words, a log of m records (address, time, value, is_store) in execution order.
  - address, time and value are below 2^word_bits; time >= 1 and times strictly increase along the log;
  - tape word i lives at address i * word_bits / 8 (tapes need word_bits % 8 == 0);
  - every tape address has a run, accessed or not; every other address has a run from its first access on; runs ascend by address;
  - a run is one Init row (time 0; value = the tape word, or 0) and then the address's accesses in time order;  rows = #runs + m.
Columns (COLUMNS, in this order): s_trace = 1; address; time (0 for Init); the one-hot init / store / load; value = the value of the latest
Init or Store row at or above the row in its run (a load's claimed value is not used); addr_inc = max(address - address of the previous run
- 1, 0) on every row of a run, the first run measuring from 0; time_inc = time - time of the row above, 0 on the Init row; and the even-bits
halves  w & 0x5555..,  (w & 0xAAAA..) >> 1  of the two increments."""
import random

COLUMNS = ["s_trace", "address", "time", "init", "store", "load", "value", "addr_inc", "time_inc", "addr_inc_even", "addr_inc_odd", "time_inc_even",
           "time_inc_odd"]
NO_SOURCE = 0xFFFFFFFF
EVEN = 0x5555555555555555


class Table:
    """rows: one list of 13 integers per row; src_index: the log index of each row (NO_SOURCE for Init rows); inconsistent: the log indices
    of loads whose claimed value differs from the value on their row, ascending"""

    def __init__(self, rows, src_index, inconsistent, m):
        self.rows, self.src_index, self.inconsistent, self.m = rows, src_index, inconsistent, m

    @property
    def n_inconsistent(self):
        return len(self.inconsistent)

    @property
    def first_inconsistent(self):
        """the smallest such log index; the log's length when there is none (as the entry reports it)"""
        return self.inconsistent[0] if self.inconsistent else self.m

    def column(self, name):
        c = COLUMNS.index(name)
        return [r[c] for r in self.rows]

    def columns(self, n):
        """13 lists of n integers: the rows, zero behind them"""
        assert len(self.rows) <= n
        return [[r[c] for r in self.rows] + [0] * (n - len(self.rows)) for c in range(len(COLUMNS))]


def first_violation(word_bits, log):
    """the index of the first record that breaks a range or ordering rule, or None"""
    limit, prev = 1 << word_bits, 0
    for i, (address, time, value, _) in enumerate(log):
        if not (0 <= address < limit and 0 <= time < limit and 0 <= value < limit) or time <= prev:
            return i
        prev = time
    return None


def check_inputs(word_bits, tape):
    assert word_bits % 2 == 0 and 2 <= word_bits <= 32
    if len(tape):
        assert word_bits % 8 == 0, "a tape needs byte-sized words"
        assert (len(tape) - 1) * word_bits // 8 < 1 << word_bits and all(0 <= w < 1 << word_bits for w in tape)


def build(word_bits, log, tape=()):
    """-> Table; raises ValueError naming the first offending log index"""
    check_inputs(word_bits, tape)
    bad = first_violation(word_bits, log)
    if bad is not None:
        raise ValueError(f"log record {bad}")
    tape_at = {i * word_bits // 8: w for i, w in enumerate(tape)}
    runs = {address: [] for address in tape_at}
    for i, (address, _, _, _) in enumerate(log):
        runs.setdefault(address, []).append(i)
    rows, src, inconsistent = [], [], []
    prev_run_address = 0
    for address in sorted(runs):
        addr_inc = max(address - prev_run_address - 1, 0)
        value = tape_at.get(address, 0)
        prev_time = 0

        def row(time, init, store, time_inc):
            return [1, address, time, int(init), int(store), int(not init and not store), value, addr_inc, time_inc, addr_inc & EVEN, (addr_inc & ~EVEN) >> 1,
                    time_inc & EVEN, (time_inc & ~EVEN) >> 1]

        rows.append(row(0, True, False, 0))
        src.append(NO_SOURCE)
        for i in runs[address]:  # execution order is time order
            _, time, claimed, is_store = log[i]
            if is_store:
                value = claimed
            elif claimed != value:
                inconsistent.append(i)
            rows.append(row(time, False, bool(is_store), time - prev_time))
            src.append(i)
            prev_time = time
        prev_run_address = address
    assert len(rows) == len(runs) + len(log)
    return Table(rows, src, sorted(inconsistent), len(log))


# ---- the reference's own cases, all at word_bits = 8 -----------------------------------------------------------------------------------------
def answer_only():
    """a program that only answers: no tape, no access -> no rows"""
    return 8, [], []


def load_and_answer(b):
    """tape [1], one load at address b at time 1 (the value it claims is what the table holds there)"""
    return 8, [(b, 1, 1 if b == 0 else 0, False)], [1]


REFERENCE_CASES = [("answer_only", answer_only())] + [(f"load_and_answer_{b}", load_and_answer(b)) for b in (0, 1, 2, 255)]


# ---- generators ---------------------------------------------------------------------------------------------------------------------------------
def random_log(rng, word_bits, m, addresses, tape=(), wrong_loads=0.0):
    """an unrestricted valid log over the given addresses: stores of random values, loads that claim the value held (or, with probability
    wrong_loads, another one)"""
    limit = 1 << word_bits
    assert m < limit
    times = sorted(rng.sample(range(1, limit), m)) if limit <= 1 << 20 else _increasing_times(rng, m, limit)
    held = {i * word_bits // 8: w for i, w in enumerate(tape)}
    log = []
    for time in times:
        address = rng.choice(addresses)
        if rng.random() < 0.5:
            v = rng.randrange(limit)
            held[address] = v
            log.append((address, time, v, True))
        else:
            v = held.get(address, 0)
            if rng.random() < wrong_loads:
                v = (v + 1 + rng.randrange(limit - 1)) % limit
            log.append((address, time, v, False))
    return log


def _increasing_times(rng, m, limit):
    step = max((limit - 1) // max(m, 1), 1)
    t, out = 0, []
    for _ in range(m):
        t += rng.randrange(1, step + 1)
        out.append(t)
    assert t < limit
    return out


def family_f(rng, word_bits, n_addresses, max_rows, tape=()):
    """A log whose table satisfies ALL FOUR Mem polynomials of the fixture.  The fourth, load . (value(next) - value), is not gated by the end
    of a run and reads the current row's load, so: every run ends in a store or holds no load, and every load is followed inside its run
    by a load or by a store of the value it read.  Per address, blocks  store v, load v x j, store v  (the first block may leave out its
    leading store when v is the initial value); the blocks of the addresses are interleaved in time.  The table has at most max_rows rows."""
    limit = 1 << word_bits
    step = word_bits // 8 if word_bits % 8 == 0 else 1
    pool = list(range(0, limit, step))
    addresses = sorted(rng.sample(pool, min(n_addresses, len(pool))))
    tape_addresses = {i * word_bits // 8 for i in range(len(tape))}
    budget = max_rows - len(tape_addresses | set(addresses))
    per_address = {a: [] for a in addresses}
    initial = {i * word_bits // 8: w for i, w in enumerate(tape)}
    while budget >= 2:
        a = rng.choice(addresses)
        ops = per_address[a]
        j = rng.randrange(0, 4)
        v = rng.randrange(limit)
        block = [(v, True)] + [(v, False)] * j + [(v, True)]
        if not ops and rng.random() < 0.5:
            v = initial.get(a, 0)
            block = [(v, False)] * j + [(v, True)]
        if len(block) > budget:
            break
        ops += block
        budget -= len(block)
    order = [a for a in addresses for _ in per_address[a]]
    rng.shuffle(order)
    assert len(order) < limit - 1
    times = sorted(rng.sample(range(1, limit), len(order)))
    cursor = {a: 0 for a in addresses}
    log = []
    for a, time in zip(order, times):
        v, is_store = per_address[a][cursor[a]]
        cursor[a] += 1
        log.append((a, time, v, is_store))
    return log


def rng_of(seed):
    return random.Random(seed)
