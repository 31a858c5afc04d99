"""No device: the Mem table's integer model, csrc/memtable.h on the host, and the host side of trh_mem_table_dev.

  model              tests/memtable_model.py on the reference's cases (word_bits = 8: a program that only answers has no rows;
                     load_and_answer with one load at address b in {0, 1, 2, 255} has 2 rows for b = 0 and 3 otherwise), its inconsistent-load
                     report and its refusals
  the fixture        the model's rows satisfy the four Mem polynomials of tests/golden/chip_gates.json, the two decomposition gates and the
                     four lookups (tests/mem_circuit.py, plonk.evaluate over integers) on those cases and on family F; on unrestricted logs
                     the first three polynomials hold and the fourth is the only one that fails
  memtable_vec_test  the header's plan, record rule and row derivation in a stand-alone program under address + undefined sanitizers
                     (tests/native/memtable_vec_test.cpp, built by program() below as `make` builds it; it never loads libtrh), against the
                     model -- with word_bits = 32, addresses 0 and 0xFFFFFFFF and times up to 2^32 - 1, where a signed subtraction would show
  the plan           passes = ceil(word_bits / 8); tile counts at m + t in {0, 1, TILE - 1, TILE, TILE + 1} for both tiles; the Python mirrors
                     of the constants
  the ABI            exported, TRH_ENODEV without a device, TRH_EINVAL for null, misaligned and bad-word_bits arguments, no stream parameter"""
import atexit
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import mem_circuit as mc
import memtable_model as mm
import pasta as o
from tiny_ram_halo2_amd import api, memtable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = [""]  # program()
M = o.FIELDS["fp"].m


def program():
    """the stand-alone program, compiled here once per run with the Makefile's command line into a directory of its own (as
    test_witness_host.py does): the tests without a device then need no build product under tests/"""
    if not os.path.exists(PROGRAM[0]):
        tmp = tempfile.mkdtemp(prefix="memtable_vec_test_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        PROGRAM[0] = os.path.join(tmp, "memtable_vec_test")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(ROOT, "tests", "native", "memtable_vec_test.cpp"), "-o", PROGRAM[0]])
    return PROGRAM[0]


def run(lines):
    p = subprocess.run([program()], input="".join(line + "\n" for line in lines), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]   # a sanitizer report ends the program with a non-zero status
    out = p.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return [line.split() for line in out]


# ---- the model --------------------------------------------------------------------------------------------------------------------------------
def test_the_model_on_the_reference_cases():
    word_bits, log, tape = mm.answer_only()
    assert mm.build(word_bits, log, tape).rows == []
    for b, n_rows in ((0, 2), (1, 3), (2, 3), (255, 3)):
        word_bits, log, tape = mm.load_and_answer(b)
        t = mm.build(word_bits, log, tape)
        assert len(t.rows) == n_rows and t.inconsistent == [] and t.first_inconsistent == 1
        assert t.column("address") == ([0, 0] if b == 0 else [0, b, b]) and t.column("init") == ([1, 0] if b == 0 else [1, 1, 0])
        assert t.column("value") == ([1, 1] if b == 0 else [1, 0, 0]) and t.column("time")[-1] == 1 and t.column("load")[-1] == 1
        assert t.column("addr_inc") == ([0, 0] if b == 0 else [0, b - 1, b - 1]) and t.column("time_inc")[-1] == 1
        assert t.src_index == [mm.NO_SOURCE] * (n_rows - 1) + [0]


def test_the_model_by_hand():
    # two addresses, the higher one accessed first; a load that claims a wrong value; word_bits = 16, tape of two words at addresses 0 and 2
    log = [(9, 3, 0, False), (2, 5, 70, True), (9, 6, 41, True), (2, 8, 71, False), (9, 0x8000, 41, False)]
    t = mm.build(16, log, [11, 12])
    want = {"address": [0, 2, 2, 2, 9, 9, 9, 9], "time": [0, 0, 5, 8, 0, 3, 6, 0x8000], "init": [1, 1, 0, 0, 1, 0, 0, 0], "store": [0, 0, 1, 0, 0, 0, 1, 0],
            "load": [0, 0, 0, 1, 0, 1, 0, 1], "value": [11, 12, 70, 70, 0, 0, 41, 41], "addr_inc": [0, 1, 1, 1, 6, 6, 6, 6],
            "time_inc": [0, 0, 5, 3, 0, 3, 3, 0x8000 - 6], "s_trace": [1] * 8, "addr_inc_even": [0, 1, 1, 1, 4, 4, 4, 4], "addr_inc_odd": [0, 0, 0, 0, 1, 1, 1, 1]}
    for name, column in want.items():
        assert t.column(name) == column, name
    assert t.src_index == [mm.NO_SOURCE, mm.NO_SOURCE, 1, 3, mm.NO_SOURCE, 0, 2, 4]
    assert t.inconsistent == [3] and t.n_inconsistent == 1 and t.first_inconsistent == 3
    assert all(e + 2 * d == w for e, d, w in zip(t.column("time_inc_even"), t.column("time_inc_odd"), t.column("time_inc")))
    assert t.columns(10)[1] == want["address"] + [0, 0]


def test_the_model_names_the_first_offending_record():
    ok = [(1, 1, 1, True), (2, 2, 2, False), (3, 3, 3, True)]
    assert mm.first_violation(8, ok) is None
    for at, record in ((1, (256, 2, 2, False)), (2, (3, 256, 3, True)), (0, (1, 1, 256, True)), (0, (1, 0, 1, True)), (1, (2, 1, 2, False)), (2, (3, 1, 3, True))):
        log = list(ok)
        log[at] = record
        assert mm.first_violation(8, log) == at
        with pytest.raises(ValueError, match=f"record {at}$"):
            mm.build(8, log)
    assert mm.first_violation(32, [(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, True)]) is None


# ---- the fixture's polynomials over the model's rows -----------------------------------------------------------------------------------------------
def judged(word_bits, log, tape=(), polys=None):
    table = mm.build(word_bits, log, tape)
    assert len(table.rows) <= mc.max_rows_of(word_bits)
    columns = table.columns(1 << mc.k_of(word_bits))
    return mc.violations(word_bits, columns, M, polys), mc.lookup_misses(word_bits, columns), table


def test_the_fixture_has_the_four_polynomials():
    polys = mc.mem_polynomials()
    assert [p.degree() for p in polys] == [4, 4, 4, 4]
    c = mc.circuit("fp")
    cs = c.system()
    assert cs.degree() == 6 and cs.blinding_factors() == mc.BLINDING and c.shape == (2, 13, 0)
    assert mc.COLUMNS == list(memtable.COLUMNS) == mm.COLUMNS


@pytest.mark.parametrize("name,case", mm.REFERENCE_CASES)
def test_the_reference_cases_satisfy_the_circuit(name, case):
    bad, misses, _ = judged(*case)
    assert bad == {} and misses == []


@pytest.mark.parametrize("word_bits,seed", [(8, 1), (8, 2), (8, 3), (16, 4), (16, 5)])
def test_family_f_satisfies_the_circuit(word_bits, seed):
    rng = mm.rng_of(seed)
    tape = [rng.randrange(1 << word_bits) for _ in range(seed % 3)]
    log = mm.family_f(rng, word_bits, 3 if word_bits == 8 else 20, mc.max_rows_of(word_bits), tape)
    bad, misses, table = judged(word_bits, log, tape)
    assert bad == {} and misses == [] and table.inconsistent == []
    assert len(table.rows) > mc.max_rows_of(word_bits) // 2 and sum(table.column("load")) > 0


def test_unrestricted_logs_break_the_fourth_polynomial_only():
    rng = mm.rng_of(77)
    broken = 0
    for _ in range(8):
        log = mm.random_log(rng, 16, 200, [rng.randrange(1 << 16) for _ in range(12)], tape=[5, 6])
        bad, misses, _ = judged(16, log, [5, 6])
        assert set(bad) <= {3} and misses == []
        broken += len(bad.get(3, []))
    assert broken > 0, "the generator no longer leaves family F"


# ---- csrc/memtable.h under the sanitizers ---------------------------------------------------------------------------------------------------------
def derive_lines(table):
    """one `r` line per row of a model table: the row's own fields, and what the scans carry to it, read off the model's rows"""
    lines, run_start, prev_run_address = [], 0, 0
    C = {name: i for i, name in enumerate(mm.COLUMNS)}
    for r, row in enumerate(table.rows):
        if row[C["init"]]:
            prev_run_address = table.rows[r - 1][C["address"]] if r else 0
            run_start = r
        prev_time = 0 if r == run_start else table.rows[r - 1][C["time"]]
        lines.append(f"r {row[C['address']]} {row[C['time']]} {row[C['init']]} {row[C['store']]} {prev_time} {prev_run_address} {row[C['value']]}")
    return lines


def test_derive_row_against_the_model():
    rng = mm.rng_of(0x3E3)
    tables = [mm.build(*case) for _, case in mm.REFERENCE_CASES]
    tables.append(mm.build(16, mm.random_log(rng, 16, 300, [rng.randrange(1 << 16) for _ in range(9)], tape=[1, 2, 3]), [1, 2, 3]))
    # 32-bit words at their ends: neighbouring addresses 0 and 0xFFFFFFFF, times up to 2^32 - 1
    top = 0xFFFFFFFF
    ends = [(top, 1, 5, True), (0, 2, 6, True), (top, 0x7FFFFFFF, 5, False), (0, 0x80000000, 6, False), (0, top - 1, 6, False), (top, top, 5, False)]
    tables.append(mm.build(32, ends))
    tables.append(mm.build(32, ends[:4] + [(top - 1, 0x80000001, top, True)] + ends[4:]))
    tables.append(mm.build(32, [(top, top, top, True)]))
    tables.append(mm.build(32, mm.random_log(rng, 32, 300, [0, 4, top, top - 1, 1 << 31, (1 << 31) - 1] + [rng.getrandbits(32) for _ in range(5)], tape=[top, 0])[:300], [top, 0]))
    for table in tables:
        got = run(derive_lines(table))
        assert [[int(w) for w in line] for line in got] == table.rows
    assert mm.build(32, ends).column("addr_inc")[-1] == top - 1 and mm.build(32, ends).column("time_inc")[-1] == top - 0x7FFFFFFF


def test_record_ok_against_the_model():
    rng = mm.rng_of(0x0C)
    cases = []
    for word_bits in (2, 8, 16, 24, 32):
        limit = 1 << word_bits
        edge = [0, 1, limit - 1, min(limit, 0xFFFFFFFF), limit // 2]
        for _ in range(60):
            cases.append((word_bits, rng.choice(edge), rng.choice(edge), rng.choice(edge), rng.choice(edge[:3] + [limit // 2])))
    cases += [(32, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFE), (32, 0, 0x80000000, 0, 0x7FFFFFFF), (32, 0, 0x7FFFFFFF, 0, 0x80000000), (32, 0, 5, 0, 5)]
    got = run([f"k {w} {a} {t} {v} {p}" for w, a, t, v, p in cases])
    for (w, a, t, v, p), line in zip(cases, got):
        want = mm.first_violation(w, [(0, p, 0, True), (a, t, v, True)]) is None if p else mm.first_violation(w, [(a, t, v, True)]) is None
        assert int(line[0]) == int(want), (w, a, t, v, p)
    got = run([f"w {w} {t}" for w, t in ((0, 0), (2, 0), (2, 1), (7, 0), (8, 256), (8, 257), (12, 0), (12, 1), (16, 1 << 15), (16, (1 << 15) + 1), (32, 1 << 20), (34, 0), (33, 0))])
    assert [[int(x) for x in line] for line in got] == [[0, 0], [1, 1], [1, 0], [0, 0], [1, 1], [1, 0], [1, 1], [1, 0], [1, 1], [1, 0], [1, 1], [0, 0], [0, 0]]


def test_the_constants_are_mirrored():
    (sort_tile, scan_tile, columns), = run(["c"])
    assert (int(sort_tile), int(scan_tile), int(columns)) == (memtable.SORT_TILE, memtable.SCAN_TILE, len(memtable.COLUMNS))


@pytest.mark.parametrize("word_bits,passes", [(2, 1), (8, 1), (10, 2), (16, 2), (18, 3), (24, 3), (26, 4), (32, 4)])
def test_the_plan_passes(word_bits, passes):
    (line,) = run([f"p 10 0 64 {word_bits}"])
    assert int(line[0]) == passes == -(-word_bits // 8) == memtable.plan(10, 0, word_bits)["passes"] and line[-1] == "ok"


def test_the_plan_tiles():
    shapes = []
    for tile in (memtable.SORT_TILE, memtable.SCAN_TILE):
        for records in (0, 1, tile - 1, tile, tile + 1):
            for t in sorted({0, min(records, 3)}):
                shapes.append((records - t, t))
    n = 1 << 14
    got = run([f"p {m} {t} {n} 32" for m, t in shapes] + [f"p 5000 7 6000 32", f"p {(1 << 22)} 0 {1 << 23} 32"])
    ceil = lambda a, b: -(-a // b)  # noqa: E731
    for (m, t), line in zip(shapes + [(5000, 7), (1 << 22, 0)], got):
        passes, records, row_cap, sort_tiles, hist_tiles, record_tiles, row_tiles, nbytes = (int(x) for x in line[:8])
        cols = 6000 if (m, t) == (5000, 7) else (1 << 23) if m == 1 << 22 else n
        assert line[8] == "ok" and records == m + t and row_cap == min(t + 2 * m, cols)
        assert sort_tiles == ceil(records, memtable.SORT_TILE) == memtable.plan(m, t, 32)["sort_tiles"]
        assert record_tiles == ceil(records, memtable.SCAN_TILE) == memtable.plan(m, t, 32)["scan_tiles"]
        assert hist_tiles == ceil(256 * sort_tiles, memtable.SCAN_TILE) and row_tiles == ceil(row_cap, memtable.SCAN_TILE)
        assert nbytes >= 20 * records + 4 * 256 * sort_tiles + 24 * row_cap and nbytes <= 20 * records + 1024 * sort_tiles + 24 * row_cap + 8 * (record_tiles + hist_tiles + row_tiles) + 14 * 256


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------------
def _has_gpu():
    import torch
    return torch.cuda.is_available()


def _args(**over):
    fields = dict(word_bits=8, address=0x1000, time=0x2000, value=0x3000, store_bits=0x4000, m=4, tape=None, t=0, dst=0x10000, n=64, max_rows=16, src_index=None,
                  stream=None)
    fields.update(over)
    return api.MemTableArgs(**fields)


def test_bad_arguments_are_einval():
    """refused before the device is looked for: the pointers are never followed"""
    lib = api.lib()
    assert lib.trh_mem_table_dev(api.FP, None) == -1
    for over, word in ((dict(word_bits=7), "word_bits"), (dict(word_bits=0), "word_bits"), (dict(word_bits=34), "word_bits"), (dict(dst=0x10008), "16-byte"),
                       (dict(dst=None), "16-byte"), (dict(address=None), "null log"), (dict(store_bits=None), "null log"), (dict(time=0x2002), "4-byte"),
                       (dict(t=2, tape=None), "null tape"), (dict(t=2, tape=0x5000, word_bits=12), "tape"), (dict(t=300, tape=0x5000), "tape"),
                       (dict(max_rows=65), "max_rows"), (dict(src_index=0x6001), "4-byte"), (dict(m=1 << 31), "2^31")):
        a = _args(**over)
        assert lib.trh_mem_table_dev(api.FP, ctypes.byref(a)) == -1, over
        assert word in lib.trh_last_error().decode(), (over, lib.trh_last_error())
    assert lib.trh_mem_table_dev(7, ctypes.byref(_args())) == -1


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_no_device_is_enodev():
    a = _args()
    assert api.lib().trh_mem_table_dev(api.FQ, ctypes.byref(a)) == -2


def test_the_stream_travels_in_the_struct():
    header = open(os.path.join(ROOT, "include", "trh.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    (params,) = re.findall(r"\btrh_mem_table_dev\s*\(([^;{}]*?)\)\s*;", header)
    assert "stream" not in params
    assert "trh_mem_table_dev" in api.EXPORTED_SYMBOLS and hasattr(api.lib(), "trh_mem_table_dev")
    assert [name for name, _ in api.MemTableArgs._fields_][-4:] == ["stream", "rows", "n_inconsistent", "first_inconsistent"]
