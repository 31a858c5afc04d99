"""trh_mem_table_dev (tiny_ram_halo2_amd.memtable, csrc/memtable.hip): an access log into the 13 columns of the memory-consistency table.
Every column is compared word for word with tests/memtable_model.py (Python integers -> oracle/pasta.py's Montgomery limbs), and rows,
n_inconsistent, first_inconsistent and src_index with it.  T = max(SORT_TILE, SCAN_TILE).

  smallest      m in {0, 1, 2} x t in {0, 1, 3}; a tape address never accessed, an access to a tape address; the reference's five cases
  past a tile   m + t in {T - 1, T, T + 1, 3 T + 5} at word_bits = 32: one address (the max-scan's carry and the sort's stability cross
                every tile), all addresses distinct (the insertion offsets cross tiles), run heads and synthesized Init rows on a tile's
                first and last row, addresses that differ in one byte only (every radix pass matters), neighbours 0 and 0xFFFFFFFF;
                trh_stat says four passes ran and every stage crossed a tile
  passes        word_bits 2, 8, 16, 24, 32 -> 1, 1, 2, 3, 4
  capacity      rows == max_rows == n accepted; one more refused with rows reported and dst untouched
  refusals      a value, an address, a time at 2^word_bits; time 0; equal neighbouring times; a decreasing time in the last tile: the first
                index is named and nothing is written
  wrong loads   counted, the smallest index named, the columns those of the corrected log
  streams       the same result on a non-blocking stream behind a delay; host and device sources agree
  the circuit   tests/mem_circuit.py (the fixture's four Mem polynomials): MockProver, proofs as bytes through both verifiers and the
                BatchVerifier at word_bits 8 (k = 6) and 16 (k = 10); a swapped row pair and a changed addr_inc_even cell are named and
                refused; an unrestricted log at k = 17 leaves the first three polynomials clean
  builder       witness.AdviceBuilder.mem_table == build placed by hand;   native: tests/native/memtable_test.cpp over include/trh.hpp"""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import mem_circuit as mc
import memtable_model as mm
import pasta as o
import transcript_model as tm
from tiny_ram_halo2_amd import api, expr, memtable, mock, plonk, poly, witness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = max(memtable.SORT_TILE, memtable.SCAN_TILE)
SIZES = [T - 1, T, T + 1, 3 * T + 5]
TOP = 0xFFFFFFFF
FIELDS = ["fp", "fq"]
FILL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def expected_limbs(field, table, n):
    """(13, n, 4) uint64: the model's columns as Montgomery limbs; each distinct value is converted once"""
    f = o.FIELDS[field]
    cells = np.array(table.columns(n), dtype=np.uint64)
    values, inverse = np.unique(cells, return_inverse=True)
    limbs = np.array([f.limbs(int(v)) for v in values], dtype=np.uint64).reshape(len(values), 4)
    return limbs[inverse.reshape(-1)].reshape(len(mm.COLUMNS), n, 4)


def arrays(log):
    a = np.array([r[:3] for r in log], dtype=np.uint32).reshape(len(log), 3)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), np.array([bool(r[3]) for r in log], dtype=np.bool_)


def device_build(field, word_bits, log, tape=(), n=None, **kw):
    address, time, value, is_store = arrays(log)
    return memtable.build(field, word_bits, address, time, value, is_store, tape=np.array(tape, dtype=np.uint32), n=n, **kw)


def compare(field, word_bits, log, tape=(), n=None, got=None, table=None):
    """the device's table against the model's, everything the entry returns; -> (model table, MemTable)"""
    table = mm.build(word_bits, log, tape) if table is None else table
    n = len(table.rows) + 7 if n is None else n
    got = device_build(field, word_bits, log, tape, n) if got is None else got
    assert got.rows == len(table.rows) == api.stat("memtable_rows")
    assert (got.n_inconsistent, got.first_inconsistent) == (table.n_inconsistent, table.first_inconsistent)
    src = host(got.src_index).view(np.uint32)
    assert src.tolist() == table.src_index + [mm.NO_SOURCE] * (n - len(table.rows))
    cells, want = host(got.columns).view(np.uint64), expected_limbs(field, table, n)
    if not (cells == want).all():
        c, r = [int(x[0]) for x in np.nonzero((cells != want).any(axis=2))]
        raise AssertionError(f"column {mm.COLUMNS[c]}, row {r} of {len(table.rows)} (n = {n}): {cells[c, r]} for {want[c, r]} = {table.columns(n)[c][r]}")
    return table, got


def log_over(rng, word_bits, addresses, tape=(), last_time=None):
    """a valid log that visits `addresses` in this order: stores of random values, loads that claim the value held; random increasing times"""
    limit = 1 << word_bits
    times = mm._increasing_times(rng, len(addresses), limit) if limit > 1 << 20 else sorted(rng.sample(range(1, limit), len(addresses)))
    if last_time is not None and times:
        times[-1] = last_time
    held = {i * word_bits // 8: w for i, w in enumerate(tape)}
    log = []
    for a, time in zip(addresses, times):
        if rng.random() < 0.5:
            held[a] = rng.randrange(limit)
            log.append((a, time, held[a], True))
        else:
            log.append((a, time, held.get(a, 0), False))
    return log


# ---- smallest logs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_smallest_logs(field):
    rng = mm.rng_of(0x51)
    for t in (0, 1, 3):
        tape = [rng.randrange(1, 1 << 16) for _ in range(t)]
        for m in (0, 1, 2):
            for addresses in ([5, 5], [7, 2], [2, 2], [0, 4], [4, 0x10000 - 1]):  # off the tape, on it (t = 3: words at 0, 2, 4), both
                table, _ = compare(field, 16, log_over(rng, 16, addresses[:m], tape), tape)
                assert len(table.rows) >= t + m
    # a tape address never accessed keeps its run; an access to a tape address joins it
    table, _ = compare(field, 16, [(2, 9, 77, False)], [11, 77, 13])
    assert table.column("address") == [0, 2, 2, 4] and table.column("value") == [11, 77, 77, 13] and table.inconsistent == []
    assert api.stat("memtable_sort_passes") == 2 and api.stat("memtable_tiles") == 1


@pytest.mark.parametrize("field", FIELDS)
def test_an_empty_call_zeroes_the_columns(field):
    out = torch.full((13, 40, 4), -1, dtype=torch.int64, device="cuda")
    got = device_build(field, 8, [], [], out=out)
    assert got.rows == 0 and got.n_inconsistent == 0 and not host(out).any() and (host(got.src_index).view(np.uint32) == mm.NO_SOURCE).all()
    assert api.stat("memtable_rows") == 0 and api.stat("memtable_sort_passes") == 0


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name,case", mm.REFERENCE_CASES)
def test_the_reference_cases(field, name, case):
    table, _ = compare(field, *case, n=16)
    assert len(table.rows) == {"answer_only": 0, "load_and_answer_0": 2}.get(name, 3)


# ---- past one tile -----------------------------------------------------------------------------------------------------------------------------
def tile_edge_addresses(size):
    """(addresses per record in run order, tape): rows 0 .. 1022 the run of tape address 0; a synthesized Init on row 1023, the LAST row of a
    scan tile (its access is the last record of the records' first scan tile, the next run's first access the first record of the second);
    the unaccessed tape address 4 on row 2047, the last row of a tile; tape address 8 opens its run on row 2048, the FIRST row of a tile;
    from 3 T + 5 records on, address 9's synthesized Init lies on row 3072, the first row of a tile"""
    S = memtable.SCAN_TILE
    assert S == 1024 and size >= 3 + 2 * S - 4
    rest = size - 3 - (2 * S - 4)
    on8 = min(rest, S - 1)
    return [0] * (S - 2) + [1] + [2] * (S - 3) + [8] * on8 + [9] * (rest - on8), [21, 22, 23]


def distribution(name, size, rng):
    """-> (log, tape) of size = m + t records at word_bits = 32"""
    tape = []
    if name == "one_address":
        addresses = [0x01020304] * size
    elif name == "distinct":
        addresses = rng.sample(range(1 << 32), size)
    elif name == "tile_edges":
        addresses, tape = tile_edge_addresses(size)
        rng.shuffle(addresses)  # the order of execution is not the order of the table
    elif name == "one_byte":
        pool = [b << 24 | 0x345678 for b in range(256)] + [0x12345600 | b for b in range(256)] + [0x12005678 | b << 16 for b in range(256)] + [0x12340078 | b << 8 for b in range(256)]
        addresses = [rng.choice(pool) for _ in range(size)]
    else:
        assert name == "neighbours"
        tape = [7]
        addresses = [rng.choice([0, TOP]) for _ in range(size - 1)]
    return log_over(rng, 32, addresses, tape, last_time=TOP if name in ("neighbours", "one_address") else None), tape


DISTRIBUTIONS = ["one_address", "distinct", "tile_edges", "one_byte", "neighbours"]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", DISTRIBUTIONS)
def test_past_one_tile(name, size):
    field = FIELDS[(DISTRIBUTIONS.index(name) + SIZES.index(size)) % 2]
    log, tape = distribution(name, size, mm.rng_of(size * 31 + len(name)))
    assert len(log) + len(tape) == size
    table, _ = compare(field, 32, log, tape)
    assert api.stat("memtable_sort_passes") == 4
    tiles = api.stat("memtable_tiles")
    assert tiles == min(-(-size // memtable.SORT_TILE), -(-size // memtable.SCAN_TILE), -(-len(table.rows) // memtable.SCAN_TILE))
    if size > T:
        assert tiles > 1
    if name == "distinct":
        assert len(table.rows) == 2 * size and table.column("init") == [1, 0] * size
    if name == "one_address":
        assert len(table.rows) == size + 1 and table.src_index[1:] == list(range(size)), "time order is the log's order: the sort is stable"
    if name == "tile_edges":
        S, init, src = memtable.SCAN_TILE, table.column("init"), table.src_index
        assert init[S - 1] and table.column("address")[S - 1] == 1 and init[2 * S - 1] and init[2 * S] and table.column("address")[2 * S - 1: 2 * S + 1] == [4, 8]
        if size > 3 * T:
            assert init[3 * S] and table.column("address")[3 * S] == 9
    if name == "neighbours":
        assert sorted(set(table.column("address"))) == [0, TOP] and TOP - 1 in table.column("addr_inc") and max(table.column("time")) == TOP


@pytest.mark.parametrize("field", FIELDS)
def test_both_fields_past_one_tile(field):
    log, tape = distribution("one_byte", 3 * T + 5, mm.rng_of(99))
    compare(field, 32, log, tape)


@pytest.mark.parametrize("word_bits,passes", [(2, 1), (8, 1), (16, 2), (24, 3), (32, 4)])
def test_pass_counts(word_bits, passes):
    rng = mm.rng_of(word_bits)
    limit = 1 << word_bits
    m = min(limit - 1, 300)
    tape = [limit - 1, 0] if word_bits % 8 == 0 else []
    log = log_over(rng, word_bits, [rng.randrange(limit) for _ in range(m)], tape)
    compare("fp" if word_bits % 16 else "fq", word_bits, log, tape)
    assert api.stat("memtable_sort_passes") == passes == memtable.plan(m, len(tape), word_bits)["passes"]


# ---- capacity and refusals ----------------------------------------------------------------------------------------------------------------------
def filled(n):
    return torch.full((13, n, 4), FILL, dtype=torch.int64, device="cuda")


def test_capacity():
    rng = mm.rng_of(0xCA)
    log = log_over(rng, 16, [rng.randrange(40) for _ in range(90)], [1, 2, 3])
    table = mm.build(16, log, [1, 2, 3])
    rows = len(table.rows)
    out = filled(rows)
    got = device_build("fp", 16, log, [1, 2, 3], out=out, max_rows=rows)
    compare("fp", 16, log, [1, 2, 3], n=rows, got=got, table=table)
    out = filled(rows)
    with pytest.raises(memtable.MemTableTooLong, match=f"{rows} rows") as e:
        device_build("fp", 16, log, [1, 2, 3], out=out, max_rows=rows - 1)
    assert e.value.rows == rows and (host(out) == FILL).all(), "a refused call writes nothing"


def refused(word_bits, log, tape, index):
    n = len(log) * 2 + len(tape) + 1
    out = filled(n)
    with pytest.raises(api.TrhError, match=f"log record {index} ") as e:
        device_build("fq", word_bits, log, tape, out=out)
    assert not isinstance(e.value, memtable.MemTableTooLong) and (host(out) == FILL).all(), "a refused call writes nothing"
    with pytest.raises(ValueError, match=f"record {index}$"):
        mm.build(word_bits, log, tape)


def test_refusals_name_the_first_index():
    rng = mm.rng_of(0xBAD)
    good = log_over(rng, 16, [rng.randrange(100) for _ in range(50)], [4, 5])
    for at, change in ((7, lambda r: (r[0], r[1], 1 << 16, r[3])), (9, lambda r: (1 << 16, r[1], r[2], r[3])), (11, lambda r: (r[0], 1 << 16, r[2], r[3]))):
        log = list(good)
        log[at] = change(log[at])
        refused(16, log, [4, 5], at)
    log = [(3, 0, 1, True)] + [(r[0], r[1] + 1, r[2], r[3]) for r in good[:-1]]
    refused(16, log, [4, 5], 0)                                    # time 0
    log = list(good)
    log[20] = (log[20][0], log[19][1], log[20][2], log[20][3])     # equal neighbouring times
    log[30] = (1 << 16, log[30][1], log[30][2], log[30][3])        # and a later violation: the first index is the one named
    refused(16, log, [4, 5], 20)
    big, tape = distribution("one_byte", 3 * T + 5, mm.rng_of(5))   # a decreasing time in the last tile
    at = len(big) - 3
    big[at] = (big[at][0], big[at - 1][1] - 1, big[at][2], big[at][3])
    refused(32, big, tape, at)


def test_inconsistent_loads():
    log, tape = distribution("one_byte", 3 * T + 5, mm.rng_of(6))
    loads = [i for i, r in enumerate(log) if not r[3]]
    last, earlier = loads[-1], loads[len(loads) // 2]
    assert last >= len(log) - memtable.SCAN_TILE
    right = mm.build(32, log, tape)
    one = list(log)
    one[last] = (log[last][0], log[last][1], log[last][2] ^ 1, False)
    table, got = compare("fp", 32, one, tape)
    assert (got.n_inconsistent, got.first_inconsistent) == (1, last) and table.rows == right.rows
    two = list(one)
    two[earlier] = (log[earlier][0], log[earlier][1], (log[earlier][2] + 5) & TOP, False)
    table, got = compare("fq", 32, two, tape)
    assert (got.n_inconsistent, got.first_inconsistent) == (2, earlier) and table.rows == right.rows
    assert (host(got.columns) == host(device_build("fq", 32, log, tape, len(right.rows) + 7).columns)).all()


# ---- the caller's stream; host and device sources ----------------------------------------------------------------------------------------------
def test_on_a_non_blocking_stream_behind_a_delay():
    """the inputs become valid on S only behind a delay: an entry that worked on another stream would read the zeros they are prefilled with"""
    from test_gpu_streams import _window
    w = _window()
    log, tape = distribution("tile_edges", T + 1, mm.rng_of(8))
    address, time, value, is_store = arrays(log)
    real = [torch.from_numpy(a.view(np.int32)).cuda() for a in (address, time, value, witness.pack_bits(is_store), np.array(tape, dtype=np.uint32))]
    torch.cuda.synchronize()
    bufs = [torch.zeros_like(r) for r in real]
    table = mm.build(32, log, tape)
    n = len(table.rows) + 7
    out = filled(n)
    torch.cuda.synchronize()
    S = w.A
    with torch.cuda.stream(S):
        torch.cuda._sleep(w.ticks)
        for b, r in zip(bufs, real):
            b.copy_(r, non_blocking=True)
    got = memtable.build("fp", 32, bufs[0], bufs[1], bufs[2], bufs[3], tape=bufs[4], out=out, stream=S.cuda_stream, m=len(log))
    compare("fp", 32, log, tape, n=n, got=got, table=table)
    # device tensors on the current stream give what numpy arrays give
    again = memtable.build("fp", 32, real[0], real[1], real[2], real[3], tape=real[4], n=n, m=len(log))
    assert (host(again.columns) == host(got.columns)).all() and (host(again.src_index) == host(got.src_index)).all()


# ---- the circuit ---------------------------------------------------------------------------------------------------------------------------------
CURVE_OF = {"fp": "vesta", "fq": "pallas"}


class Setup:
    """the Mem circuit of tests/mem_circuit.py at one word size: keys, and the parameters as tests/plonk_model.py wants them (limb rows, its
    C++ group)"""

    def __init__(self, field, word_bits):
        self.field, self.word_bits, self.curve, self.k, self.group = field, word_bits, CURVE_OF[field], mc.k_of(word_bits), "cpp"
        self.n, self.cv = 1 << self.k, o.CURVES[CURVE_OF[field]]
        self.params = poly.Params.new(self.curve, self.k)
        self.circuit = mc.circuit(field)
        self.cs = self.circuit.system()
        self.fixed = torch.zeros((2, self.n, 4), dtype=torch.int64, device="cuda")
        witness.columns_from_ints(field, np.ones(mc.max_rows_of(word_bits), dtype=np.uint8), self.n, out=self.fixed[0])
        witness.even_bits_table(field, word_bits, self.n, out=self.fixed[1])
        self.vk, self.pk = plonk.keygen(self.params, self.cs, self.fixed, [])
        g, gl = self.params._g.download(), self.params._g_lagrange.download()
        self.pts = lambda rows: np.asarray(rows, dtype=np.uint64).reshape(-1, 8)
        self.g, self.g_lagrange, self.w = self.pts(g[:self.n]), self.pts(gl[:self.n]), self.pts(g[self.n:self.n + 1])[0]
        self.u = self.pts(np.asarray(self.params.u, dtype=np.uint64).reshape(1, 8))[0]
        self.model = self.circuit.model()
        self.instances = []
        gates, lookups = mc.mock_gates()
        self.mock = mock.MockProver(field, self.k, mc.usable(word_bits), gates, lookups)

    def advice(self, log, tape=()):
        b = witness.AdviceBuilder(self.field, 13, self.n)
        address, time, value, is_store = arrays(log)
        got = b.mem_table(0, self.word_bits, address, time, value, is_store, tape=np.array(tape, dtype=np.uint32), max_rows=mc.max_rows_of(self.word_bits))
        return b.tensor(), got

    def failures(self, advice):
        columns = {("advice", i): advice[i] for i in range(13)}
        columns.update({("fixed", j): self.fixed[j] for j in range(2)})
        return self.mock.verify(columns)

    def prove(self, advice, seed=7, strict_lookups=True):
        return plonk.create_proof_bytes(self.params, self.pk, [], advice, api.Rng(bytes([seed]) * 32), strict_lookups=strict_lookups)

    def accepts(self, proof):
        try:
            guard = plonk.verify_proof_bytes(self.params, self.vk, [], proof)
        except plonk.VerifyError:
            return False
        return plonk.single_verify(self.params, guard)

    def model_accepts(self, proof):
        ok, _, refused = tm.verify(self.curve, self.k, self.g, self.g_lagrange, self.w, self.u, self.model, self.pts(self.vk.fixed_commitments),
                                   self.pts(self.vk.sigma_commitments), self.vk.transcript_repr, [], proof, group=self.group)
        return ok and refused is None


@functools.lru_cache(maxsize=None)
def setup(field, word_bits):
    return Setup(field, word_bits)


def whole_circuit(s, logs):
    """every log: MockProver satisfied, a proof accepted by both verifiers; the first two proofs through one BatchVerifier (two_programs)"""
    proofs = []
    for seed, (log, tape) in enumerate(logs):
        advice, got = s.advice(log, tape)
        assert got.n_inconsistent == 0 and s.failures(advice) == []
        proof = s.prove(advice, seed=7 + seed)
        assert s.accepts(proof) and s.model_accepts(proof)
        proofs.append(proof)
    if len(proofs) >= 2:
        batch = plonk.BatchVerifier()
        for p in proofs[:2]:
            batch.add_proof([], p)
        assert batch.finalize(s.params, s.vk)
    return proofs


@pytest.mark.parametrize("field", FIELDS)
def test_the_circuit_on_the_reference_cases(field):
    s = setup(field, 8)
    assert s.cs.degree() == 6 and s.cs.blinding_factors() == mc.BLINDING and s.k == 6
    whole_circuit(s, [(case[1], case[2]) for _, case in mm.REFERENCE_CASES])


@pytest.mark.parametrize("field,word_bits", [("fp", 8), ("fq", 8), ("fq", 16)])
def test_the_circuit_on_family_f(field, word_bits):
    s = setup(field, word_bits)
    logs = []
    for seed in (1, 2):
        rng = mm.rng_of(seed + word_bits)
        tape = [rng.randrange(1 << word_bits) for _ in range(2)]
        logs.append((mm.family_f(rng, word_bits, 3 if word_bits == 8 else 24, mc.max_rows_of(word_bits), tape), tape))
    if word_bits == 16:
        assert s.k == 10 and all(200 <= len(mm.build(16, log, tape).rows) <= 256 for log, tape in logs)
    whole_circuit(s, logs)


def test_swapped_rows_and_a_changed_cell_are_named_and_refused():
    s = setup("fq", 8)
    rng = mm.rng_of(3 + 8)
    tape = [rng.randrange(256) for _ in range(2)]
    log = mm.family_f(rng, 8, 3, 16, tape)
    table = mm.build(8, log, tape)
    advice, _ = s.advice(log, tape)
    assert s.failures(advice) == []
    # two neighbouring accesses of one run, swapped in every column
    r = next(r for r in range(1, len(table.rows) - 1) if not table.column("init")[r] and not table.column("init")[r + 1])
    swapped = advice.clone()
    swapped[:, r], swapped[:, r + 1] = advice[:, r + 1], advice[:, r]
    found = s.failures(swapped)
    assert any(isinstance(f, mock.ConstraintNotSatisfied) and f.name == "Mem" and f.row in (r - 1, r, r + 1) for f in found), found
    assert not any(isinstance(f, mock.Lookup) for f in found)
    proof = s.prove(swapped)
    with pytest.raises(plonk.VerifyError):
        plonk.verify_proof_bytes(s.params, s.vk, [], proof)
    assert not s.model_accepts(proof)
    # one half of one increment: 2 has no bit at an even position, so it is not in the table
    changed = advice.clone()
    row = len(table.rows) // 2
    changed[mm.COLUMNS.index("addr_inc_even"), row] = torch.from_numpy(np.array(o.FIELDS["fq"].limbs(2), dtype=np.uint64).view(np.int64)).cuda()
    found = s.failures(changed)
    assert mock.Lookup(0, "addr_inc_even in even_bits_table", row) in found, found
    assert [f for f in found if isinstance(f, mock.Lookup)] == [mock.Lookup(0, "addr_inc_even in even_bits_table", row)]


def test_an_unrestricted_log_keeps_the_first_three_polynomials():
    """word_bits = 30: k = 17, up to 2^15 rows, four sort passes, dozens of tiles; only the fourth polynomial, which no unrestricted log
    satisfies, may be reported"""
    word_bits, field = 30, "fp"
    k, n = mc.k_of(word_bits), 1 << mc.k_of(word_bits)
    rng = mm.rng_of(0x17)
    pool = [rng.randrange(1 << word_bits) for _ in range(3000)]
    log = mm.random_log(rng, word_bits, 24000, pool)
    address, time, value, is_store = arrays(log)
    got = memtable.build(field, word_bits, address, time, value, is_store, n=n, max_rows=mc.max_rows_of(word_bits))
    assert k == 17 and 24000 < got.rows <= mc.max_rows_of(word_bits) and got.n_inconsistent == 0
    assert api.stat("memtable_sort_passes") == 4 and api.stat("memtable_tiles") > 1
    fixed = torch.zeros((2, n, 4), dtype=torch.int64, device="cuda")
    witness.columns_from_ints(field, np.ones(mc.max_rows_of(word_bits), dtype=np.uint8), n, out=fixed[0])
    witness.even_bits_table(field, word_bits, n, out=fixed[1])
    columns = {("advice", i): got.columns[i] for i in range(13)}
    columns.update({("fixed", j): fixed[j] for j in range(2)})
    first_three = [mc.mem_polynomials()[i] for i in mc.FIRST_THREE]
    ev = expr.GateEvaluator(expr.compile_outputs(field, first_three), n_outputs=3)
    n_bad, _ = ev.check({key: columns[key] for key in ev.program.columns}, k, mc.usable(word_bits))
    assert n_bad.tolist() == [0, 0, 0]
    gates, lookups = mc.mock_gates()
    found = mock.MockProver(field, k, mc.usable(word_bits), gates, lookups).verify(columns)
    assert found and all(isinstance(f, mock.ConstraintNotSatisfied) and (f.name, f.poly_index) == ("Mem", 3) for f in found), found[:4]
    # and the columns are the model's: the live rows and a few behind them word for word, the rest zero
    assert not got.columns[:, got.rows:].any().item()
    head = got.rows + 7
    compare(field, word_bits, log, n=head, got=memtable.MemTable(got.columns[:, :head], got.rows, got.n_inconsistent, got.first_inconsistent, got.src_index[:head]))


# ---- the builder and the native driver -----------------------------------------------------------------------------------------------------------
def test_advice_builder_places_the_table():
    rng = mm.rng_of(0xAB)
    log = log_over(rng, 16, [rng.randrange(60) for _ in range(120)], [8, 9])
    address, time, value, is_store = arrays(log)
    n = 256
    b = witness.AdviceBuilder("fq", 17, n)
    got = b.mem_table(2, 16, address, time, value, is_store, tape=np.array([8, 9], dtype=np.uint32))
    alone = device_build("fq", 16, log, [8, 9], n)
    t = host(b.tensor())
    assert (t[2:15] == host(alone.columns)).all() and not t[:2].any() and not t[15:].any()
    assert (got.rows, got.n_inconsistent) == (alone.rows, alone.n_inconsistent) and got.columns.data_ptr() == b.tensor()[2].data_ptr()


def test_native_driver():
    exe = os.path.join(ROOT, "tests", "native", "memtable_test")
    assert os.path.exists(exe), "tests/native/memtable_test is missing: run `make`"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["test"] == "memtable" and rec["checks_failed"] == 0 and rec["checks"] > 100000
