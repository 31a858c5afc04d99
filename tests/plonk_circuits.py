"""The two circuits of tests/test_gpu_plonk.py as data: the Expression form for tiny_ram_halo2_amd.plonk, the tuple form for
tests/plonk_model.py, and satisfying witnesses as lists of integers.  Nothing here needs a device.

Circuit A (k = 5): 10 advice columns, 1 instance column, 7 fixed columns.
  equality   advice 0 .. 7 and the instance column: nine columns, in sets of four with minimum_degree = 6 -- three product sets; the copies
             are quotient_model.Witness's random ones among the usable rows, advice <-> instance cells included
  gates      F0 (a0 a1 - a8)                      degree 3
             F1 (a9 - F2(+1) a2)                  enabled on EVERY usable row: at the last one Rotation(+1) reads row u of the fixed column F2,
                                                  the first row behind the usable ones
             F3 (a8(-1) - a0(-1) a1(-1))          Rotation(-1); enabled from row 1 (row 0 would read the last blinding row)
  lookups    a4 in F4;   (a5, a9) in (F5, F6)     the tables hold the inputs' values in another order; a4 has one value twice and F4 one
                                                  value that no input takes, so the permuted table has a left-over row to fill
Every advice column has at most two queries, so blinding_factors = max(3, 2) + 2 = 5 and 26 of the 32 rows are usable.

Circuit B (k = 5): the logic chip of tests/test_gpu_logic_chip.py (even-bits decomposition, and / xor / or) with its selector and its table
as the fixed columns 0 and 1: 9 gates of degree 3, 8 lookups whose input has degree 3 (so the system's degree is 2 + 3 + 1 = 6), no copies."""
import random

from common import expr_to_tuple
from tiny_ram_halo2_amd import expr

K = 5
BLINDING = 5
USABLE = (1 << K) - (BLINDING + 1)


class Circuit:
    def __init__(self, name, field, num_fixed, num_advice, num_instance, gates, lookups, permutation_columns, minimum_degree):
        self.name, self.field = name, field
        self.shape = (num_fixed, num_advice, num_instance)
        self.gates, self.lookups, self.permutation_columns, self.minimum_degree = gates, lookups, permutation_columns, minimum_degree

    def system(self):
        """plonk.ConstraintSystem"""
        from tiny_ram_halo2_amd import plonk
        return plonk.ConstraintSystem(self.field, *self.shape, self.gates, self.lookups, self.permutation_columns, minimum_degree=self.minimum_degree)

    def model(self):
        """plonk_model.System"""
        import plonk_model
        return plonk_model.System([expr_to_tuple(g) for g in self.gates], [([expr_to_tuple(e) for e in i], [expr_to_tuple(e) for e in t]) for i, t in self.lookups],
                                  self.permutation_columns, self.shape[1], self.minimum_degree)


def circuit_a(field="fq"):
    a = [expr.Advice(i) for i in range(10)]
    f = [expr.Fixed(i) for i in range(7)]
    gates = [f[0] * (a[0] * a[1] - a[8]),
             f[1] * (a[9] - expr.Fixed(2, 1) * a[2]),
             f[3] * (expr.Advice(8, -1) - expr.Advice(0, -1) * expr.Advice(1, -1))]
    lookups = [([a[4]], [f[4]]), ([a[5], a[9]], [f[5], f[6]])]
    columns = [("advice", i) for i in range(8)] + [("instance", 0)]
    return Circuit("A", field, 7, 10, 1, gates, lookups, columns, 6)


class WitnessA:
    """advice: 10 lists of n integers, instance: the usable rows of the ninth equality column, fixed: 7 lists, copies: quads over the nine
    equality-enabled columns"""

    def __init__(self, field="fq", seed=23, n_copies=40):
        import quotient_model as qm
        w = qm.Witness(field, K, 9, 4, 0, BLINDING, 3, 5, seed=seed, n_copies=n_copies)
        assert w.usable == USABLE
        m, n, u = w.m, w.n, w.usable
        rng = random.Random(seed ^ 0xA)
        self.m, self.copies = m, [tuple(c) for c in w.copies]
        v = [list(c) for c in w.values]
        f2 = [rng.randrange(1, m) for _ in range(n)]
        a8 = [v[0][i] * v[1][i] % m for i in range(n)]
        a9 = [f2[(i + 1) % n] * v[2][i] % m for i in range(n)]
        self.advice = v[:8] + [a8, a9]
        self.instance = v[8][:u]
        tied = {(c[0], c[1]) for c in self.copies} | {(c[2], c[3]) for c in self.copies}
        r1, r2 = [r for r in range(u) if (4, r) not in tied][:2]
        self.advice[4][r2] = self.advice[4][r1]  # an input value twice ...
        order = list(range(u))
        rng.shuffle(order)
        t1 = [self.advice[4][j] for j in order]
        t1[order.index(r2)] = rng.randrange(m)   # ... and a table value that no input takes
        t2a, t2b = [v[5][j] for j in reversed(range(u))], [a9[j] for j in reversed(range(u))]
        zeros = [0] * (n - u)
        ones = [1] * u + zeros
        self.fixed = [ones, ones, f2, [0] + [1] * (u - 1) + zeros, t1 + zeros, t2a + zeros, t2b + zeros]

    def free_cell(self, column):
        """a usable row of an equality-enabled column that no copy touches"""
        tied = {(c[0], c[1]) for c in self.copies} | {(c[2], c[3]) for c in self.copies}
        return next(r for r in range(2, USABLE) if (column, r) not in tied)

    def copied_cell(self, columns=(6, 7)):
        """(column, row) of a cell, in a column no gate or lookup reads, that a copy ties to another cell"""
        return next((c[0], c[1]) for c in self.copies if c[0] in columns and c[:2] != c[2:])


# ---- circuit B: the logic chip -------------------------------------------------------------------------------------------------------------
ADV_B = ["s_and", "s_xor", "s_or", "a", "a_e", "a_o", "b", "b_e", "b_o", "es", "es_e", "es_o", "os", "os_e", "os_o", "res"]
DECOMPOSED_B = [("a", "a_e", "a_o"), ("b", "b_e", "b_o"), ("es", "es_e", "es_o"), ("os", "os_e", "os_o")]


def circuit_b(field="fp"):
    A = {name: expr.Advice(i) for i, name in enumerate(ADV_B)}
    s_table, t_even = expr.Fixed(0), expr.Fixed(1)
    s = s_table * (A["s_and"] + A["s_xor"] + A["s_or"])
    two = expr.Constant(2)
    gates, lookups = [], []
    for word, even, odd in DECOMPOSED_B:
        gates.append(s * (A[even] + two * A[odd] - A[word]))
        lookups.append(([s * A[even]], [t_even]))
        lookups.append(([s * A[odd]], [t_even]))
    gates.append(s * (A["a_e"] + A["b_e"] - A["es"]))
    gates.append(s * (A["a_o"] + A["b_o"] - A["os"]))
    and_ = A["es_o"] + two * A["os_o"]
    xor = A["es_e"] + two * A["os_e"]
    gates.append(s_table * A["s_and"] * (and_ - A["res"]))
    gates.append(s_table * A["s_xor"] * (xor - A["res"]))
    gates.append(s_table * A["s_or"] * (xor + and_ - A["res"]))
    return Circuit("B", field, 2, 16, 0, gates, lookups, [], None)


# ---- the two smallest shapes: gates alone (degree 3, two coset blocks, no product column) and copies alone (no gate, no fixed column) --------
def circuit_gates_only(field="fq"):
    a = [expr.Advice(i) for i in range(3)]
    return Circuit("G", field, 1, 3, 0, [expr.Fixed(0) * (a[0] * a[1] - a[2])], [], [], None)


def witness_gates_only(field="fq", seed=31):
    """-> (advice, fixed)"""
    from tiny_ram_halo2_amd.poly import _MODULUS
    m, n, rng = _MODULUS[field], 1 << K, random.Random(seed)
    a0, a1 = [rng.randrange(m) for _ in range(n)], [rng.randrange(m) for _ in range(n)]
    return [a0, a1, [x * y % m for x, y in zip(a0, a1)]], [[1] * USABLE + [0] * (n - USABLE)]


def circuit_copies_only(field="fp"):
    """degree 3: sets of ONE column, so two advice columns make two product columns and the chain links them"""
    return Circuit("P", field, 0, 2, 0, [], [], [("advice", 0), ("advice", 1)], None)


def witness_copies_only(field="fp", seed=37):
    """-> (advice, copies): column 1 is column 0 read backwards over the usable rows, every cell tied to its twin"""
    from tiny_ram_halo2_amd.poly import _MODULUS
    m, n, rng = _MODULUS[field], 1 << K, random.Random(seed)
    a0 = [rng.randrange(m) for _ in range(n)]
    a1 = [a0[USABLE - 1 - r] if r < USABLE else rng.randrange(m) for r in range(n)]
    return [a0, a1], [(0, r, 1, USABLE - 1 - r) for r in range(USABLE)]
