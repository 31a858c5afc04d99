"""The Mem table as a circuit, built from the committed fixture: the four "Mem" polynomials of tests/golden/chip_gates.json are the
reference's own, transcribed; what the device writes (tiny_ram_halo2_amd.memtable) is judged by them.  Nothing here needs a device.

  fixed 0    the table's selector (the fixture's m_s_table): 1 on rows < max_rows = 2^(word_bits / 2)
  fixed 1    the even-bits table (witness.even_bits_table)
  advice     the 13 columns of memtable.COLUMNS, in that order
  gates      the four Mem polynomials (each reads s_trace of the NEXT row, so the last live row constrains nothing behind it) and the two
             decompositions  F0 s_trace (even + 2 odd - word)  of addr_inc and time_inc
  lookups    [F0 s_trace half] in [F1] for the four halves
k = 2 + word_bits / 2, degree 6, 5 blinding factors -- as circuit B of tests/plonk_circuits.py.

The fourth polynomial, load . (value(next) - value), is not gated by the end of a run and reads the CURRENT row's load: a load followed by a
store of another value violates it, and so does a load that closes a run when the next run opens on another value.  Whole-circuit tests
therefore draw from memtable_model.family_f; on unrestricted logs only polynomials 0 .. 2 are expected to hold (FIRST_THREE)."""
import json
import os

from plonk_circuits import Circuit
from tiny_ram_halo2_amd import expr, gateset

COLUMNS = ["s_trace", "address", "time", "init", "store", "load", "value", "addr_inc", "time_inc", "addr_inc_even", "addr_inc_odd", "time_inc_even",
           "time_inc_odd"]
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chip_gates.json")
BLINDING = 5
FIRST_THREE = (0, 1, 2)
HALVES = ["addr_inc_even", "addr_inc_odd", "time_inc_even", "time_inc_odd"]


class _Columns:
    """gateset._from_json's column numbering, pinned: the selector is Fixed(0), the advice columns are COLUMNS"""

    def adv(self, name, rot=0):
        return expr.Advice(COLUMNS.index(name), rot)

    def sel(self, name):
        assert name == "m_s_table", name
        return expr.Fixed(0)


def mem_polynomials():
    """the fixture's four Mem entries as Expressions over Fixed(0) and the 13 advice columns"""
    with open(FIXTURE) as fh:
        doc = json.load(fh)
    entries = [g for g in doc["gates"] if g["name"] == "Mem"]
    assert len(entries) == 4
    rename = lambda name: "s_trace" if name == "m_s_trace" else name  # noqa: E731
    return [gateset._from_json(g["expr"], doc["advice"], doc["selectors"], _Columns(), rename) for g in entries]


def k_of(word_bits):
    return 2 + word_bits // 2


def max_rows_of(word_bits):
    return 1 << (word_bits // 2)


def usable(word_bits):
    return (1 << k_of(word_bits)) - (BLINDING + 1)


def gates_and_lookups():
    A = {name: expr.Advice(i) for i, name in enumerate(COLUMNS)}
    s = expr.Fixed(0) * A["s_trace"]
    two = expr.Constant(2)
    gates = mem_polynomials()
    gates.append(s * (A["addr_inc_even"] + two * A["addr_inc_odd"] - A["addr_inc"]))
    gates.append(s * (A["time_inc_even"] + two * A["time_inc_odd"] - A["time_inc"]))
    lookups = [([s * A[h]], [expr.Fixed(1)]) for h in HALVES]
    return gates, lookups


def circuit(field):
    gates, lookups = gates_and_lookups()
    return Circuit("Mem", field, 2, len(COLUMNS), 0, gates, lookups, [], None)


def mock_gates():
    """for mock.MockProver: the four reference polynomials as one gate "Mem", the decompositions as "even_bits"; and the lookups by name"""
    gates, lookups = gates_and_lookups()
    return [("Mem", gates[:4]), ("even_bits", gates[4:])], [(f"{h} in even_bits_table", i, t) for h, (i, t) in zip(HALVES, lookups)]


def fixed_columns(word_bits):
    """-> [selector, table] as lists of 2^k integers"""
    n, rows = 1 << k_of(word_bits), max_rows_of(word_bits)
    spread = lambda i: sum(((i >> j) & 1) << (2 * j) for j in range(word_bits // 2))  # noqa: E731
    return [[1] * rows + [0] * (n - rows), [spread(i) for i in range(rows)] + [0] * (n - rows)]


def violations(word_bits, columns, m, polys=None):
    """{gate index: [rows]} of the gates (all six, or `polys`) that do not vanish on a usable row, by plonk.evaluate over integers;
    columns: 13 lists of 2^k integers"""
    from tiny_ram_halo2_amd import plonk
    n = 1 << k_of(word_bits)
    fixed = fixed_columns(word_bits)
    gates, _ = gates_and_lookups()
    bad = {}
    for gi in range(len(gates)) if polys is None else polys:
        for row in range(usable(word_bits)):
            query = lambda kind, column, rot: (fixed if kind == "fixed" else columns)[column][(row + rot) % n]  # noqa: E731
            if plonk.evaluate(gates[gi], m, query):
                bad.setdefault(gi, []).append(row)
    return bad


def lookup_misses(word_bits, columns):
    """rows (of any half) whose selected value is not in the even-bits table"""
    fixed = fixed_columns(word_bits)
    table = set(fixed[1][:usable(word_bits)])
    out = []
    for h in HALVES:
        col = columns[COLUMNS.index(h)]
        strace = columns[0]
        out += [(h, r) for r in range(usable(word_bits)) if fixed[0][r] * strace[r] * col[r] not in table]
    return out
