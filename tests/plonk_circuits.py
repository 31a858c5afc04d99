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
as the fixed columns 0 and 1: 9 gates of degree 3, 8 lookups whose input has degree 3 (so the system's degree is 2 + 3 + 1 = 6), no copies.

Every witness takes k (default K = 5, the size of tests/test_gpu_plonk.py); u = usable(k) = 2^k - 6 for all four circuits.  WitnessA for k > 5
(tests/test_gpu_plonk_sizes.py) holds by construction:
  copies     2^k / 8 random ones among the nine equality columns, and ONE cycle of exactly four cells (WitnessA.cycle)
                 (3, 0)  (6, B - 1)  (instance, B)  (7, u - 1)          B = cycle_block(k): 256 up to k = 13, 4096 (SCAN_BLOCK) from k = 14
             column 3 lies in the first permutation set, 6 and 7 in the second, the instance column (equality column 8) in the third; rows
             B - 1 and B lie in neighbouring blocks of B rows, u - 1 in the last one.  No random copy touches these cells or (2, u - 1).
  gates      F1 enabled on row u - 1 (Rotation(+1) reads row u), F3 from row 1, as at k = 5
  lookups    tables over all u usable rows in another order than the inputs, one input value twice, one table value no input takes
Columns 3, 6, 7 and the instance column are read by no gate and no lookup, so their cells are free to change."""
import random

from common import expr_to_tuple
from tiny_ram_halo2_amd import expr

K = 5
BLINDING = 5
INSTANCE_COLUMN = 8  # the instance column among circuit A's nine equality columns


def usable(k=K):
    return (1 << k) - (BLINDING + 1)


def cycle_block(k):
    return 4096 if k >= 14 else 256


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

    def __init__(self, field="fq", k=K, seed=23, n_copies=None):
        from tiny_ram_halo2_amd.poly import _MODULUS
        m, n, u = _MODULUS[field], 1 << k, usable(k)
        self.m, self.k, self.usable, self.cycle = m, k, u, []
        if k == K:
            import quotient_model as qm
            w = qm.Witness(field, K, 9, 4, 0, BLINDING, 3, 5, seed=seed, n_copies=40 if n_copies is None else n_copies)
            assert (w.m, w.usable) == (m, u)
            self.copies = [tuple(c) for c in w.copies]
            v = [list(c) for c in w.values]
        else:
            self.copies, v = self._tied_columns(random.Random(seed ^ (k << 8)), n // 8 if n_copies is None else n_copies)
        rng = random.Random(seed ^ 0xA)
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

    def _tied_columns(self, rng, n_copies):
        """-> (copies, nine columns of n values): random copies beside the four-cell cycle, one value per tied class"""
        m, n, u, block = self.m, 1 << self.k, self.usable, cycle_block(self.k)
        assert block < u - 1
        self.cycle = [(3, 0), (6, block - 1), (INSTANCE_COLUMN, block), (7, u - 1)]
        reserved = set(self.cycle) | {(2, u - 1)}
        copies = []
        while len(copies) < n_copies:
            c = (rng.randrange(9), rng.randrange(u), rng.randrange(9), rng.randrange(u))
            if c[:2] not in reserved and c[2:] not in reserved:
                copies.append(c)
        at = rng.randrange(len(copies))  # the cycle's three copies go into the middle of the list, not to its end
        copies[at:at] = [a + b for a, b in zip(self.cycle, self.cycle[1:])]
        parent = {}

        def find(cell):
            root = cell
            while parent.setdefault(root, root) != root:
                root = parent[root]
            while parent[cell] != root:
                parent[cell], cell = root, parent[cell]
            return root

        for c in copies:
            parent[find(c[:2])] = find(c[2:])
        v = [[rng.randrange(m) for _ in range(n)] for _ in range(9)]
        for column, row in list(parent):
            root = find((column, row))
            v[column][row] = v[root[0]][root[1]]
        return copies, v

    def _tied(self):
        return {(c[0], c[1]) for c in self.copies} | {(c[2], c[3]) for c in self.copies}

    def free_cell(self, column, tail=None):
        """a usable row of an equality-enabled column that no copy touches; with `tail`, among the last `tail` usable rows"""
        tied = self._tied()
        return next(r for r in range(2 if tail is None else self.usable - tail, self.usable) if (column, r) not in tied)

    def copied_cell(self, columns=(6, 7), tail=None):
        """(column, row) of a cell, in a column no gate or lookup reads, that a copy ties to another cell; with `tail`, among the last `tail`
        usable rows"""
        real = [c for c in self.copies if c[:2] != c[2:]]
        if tail is None:
            return next(c[:2] for c in real if c[0] in columns)
        return next(end for c in real for end in (c[:2], c[2:]) if end[0] in columns and end[1] >= self.usable - tail)


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


def witness_b(field="fp", k=K, used=None, seed=0x10B):
    """-> (advice, fixed): test_gpu_logic_chip.witness with the chip's table enabled on the first `used` rows (default: all usable rows but
    three); the values are small integers, whatever the field"""
    from test_gpu_logic_chip import ADV, witness
    assert ADV == ADV_B
    cols, s_table, table = witness(1 << k, usable(k) - 3 if used is None else used, seed)
    return [cols[name] for name in ADV], [s_table, table]


# ---- the two smallest shapes: gates alone (degree 3, two coset blocks, no product column) and copies alone (no gate, no fixed column) --------
def circuit_gates_only(field="fq"):
    a = [expr.Advice(i) for i in range(3)]
    return Circuit("G", field, 1, 3, 0, [expr.Fixed(0) * (a[0] * a[1] - a[2])], [], [], None)


def witness_gates_only(field="fq", k=K, seed=31):
    """-> (advice, fixed)"""
    from tiny_ram_halo2_amd.poly import _MODULUS
    m, n, u, rng = _MODULUS[field], 1 << k, usable(k), random.Random(seed)
    a0, a1 = [rng.randrange(m) for _ in range(n)], [rng.randrange(m) for _ in range(n)]
    return [a0, a1, [x * y % m for x, y in zip(a0, a1)]], [[1] * u + [0] * (n - u)]


def circuit_copies_only(field="fp"):
    """degree 3: sets of ONE column, so two advice columns make two product columns and the chain links them"""
    return Circuit("P", field, 0, 2, 0, [], [], [("advice", 0), ("advice", 1)], None)


def witness_copies_only(field="fp", k=K, seed=37):
    """-> (advice, copies): column 1 is column 0 read backwards over the usable rows, every cell tied to its twin"""
    from tiny_ram_halo2_amd.poly import _MODULUS
    m, n, u, rng = _MODULUS[field], 1 << k, usable(k), random.Random(seed)
    a0 = [rng.randrange(m) for _ in range(n)]
    a1 = [a0[u - 1 - r] if r < u else rng.randrange(m) for r in range(n)]
    return [a0, a1], [(0, r, 1, u - 1 - r) for r in range(u)]
