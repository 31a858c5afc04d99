"""The permutation and lookup terms of the quotient's numerator in Python integers: a restatement of halo2_proofs 0.2.0
plonk/permutation/prover.rs `Committed::construct` and plonk/lookup/prover.rs `Committed::construct` (as recalled), which
csrc/quotient.hip is compared with bit for bit, and a small satisfying witness on which the folded numerator has to be divisible by
X^n - 1.  Columns are lists of canonical integers (values, not stored Montgomery words); to_values / to_stored convert."""
import random

import numpy as np

from permkeygen_model import Assembly as CopyModel
from tiny_ram_halo2_amd import permutation, synth
from tiny_ram_halo2_amd.poly import _MODULUS, EvaluationDomain


def to_values(field, stored):
    """(n, 4) stored Montgomery words -> the n field values"""
    m = _MODULUS[field]
    r_inv = pow(1 << 256, -1, m)
    return [w * r_inv % m for w in synth.limbs_to_ints(stored)]


def to_stored(field, values):
    m = _MODULUS[field]
    return synth.ints_to_limbs([v % m * (1 << 256) % m for v in values])


class Layout:
    """the rows of an extended column: flat (2^extended_k rows, Rotation(r) = r * 2^(extended_k - k) rows, cyclic) or n_blocks coset blocks
    of 2^k rows (Rotation(r) = row (q + r) mod 2^k of the same block); x(i) is the domain point of row i"""

    def __init__(self, domain: EvaluationDomain, n_blocks: int | None = None):
        self.d, self.m, self.n, self.k = domain, _MODULUS[domain.field], domain.n, domain.k
        self.shift = domain.extended_k - domain.k
        self.n_blocks = n_blocks or 0
        assert 0 <= self.n_blocks <= 1 << self.shift
        self.rows = self.n_blocks << self.k if self.n_blocks else 1 << domain.extended_k
        self._pow = None

    def exponent(self, i):
        return (i >> self.k) + ((i & (self.n - 1)) << self.shift) if self.n_blocks else i

    def x(self, i):
        if self._pow is None:  # zeta * extended_omega^e for every e, once
            self._pow = [self.d.g_coset]
            for _ in range((1 << self.d.extended_k) - 1):
                self._pow.append(self._pow[-1] * self.d.extended_omega % self.m)
        return self._pow[self.exponent(i)]

    def rot(self, i, r):
        if self.n_blocks:
            return (i & ~(self.n - 1)) | ((i + r) & (self.n - 1))
        return (i + (r << self.shift)) % self.rows


def term_columns(lay: Layout, values, sigmas, zs, lookups, l0, l_blind, l_last, beta, gamma, chunk_len, blinding_factors):
    """every term of the two arguments as a list over the rows, in the order create_proof folds them"""
    m, R = lay.m, range(lay.rows)
    delta = permutation.delta(lay.d.field)
    last = -(blinding_factors + 1)
    active = [(1 - (l_last[i] + l_blind[i])) % m for i in R]
    out = []
    n_cols = len(values)
    sets = [range(s, min(s + chunk_len, n_cols)) for s in range(0, n_cols, chunk_len)]
    assert len(zs) == len(sets) and len(sigmas) == n_cols
    if sets:
        out.append([l0[i] * (1 - zs[0][i]) % m for i in R])
        zl = zs[-1]
        out.append([l_last[i] * (zl[i] * zl[i] - zl[i]) % m for i in R])
        for s in range(1, len(sets)):
            out.append([l0[i] * (zs[s][i] - zs[s - 1][lay.rot(i, last)]) % m for i in R])
        xs = [lay.x(i) for i in R]
        bd = [beta * pow(delta, j, m) % m for j in range(n_cols)]
        for s, cols in enumerate(sets):
            t = []
            for i in R:
                left, right = zs[s][lay.rot(i, 1)], zs[s][i]
                for j in cols:
                    left = left * (values[j][i] + beta * sigmas[j][i] + gamma) % m
                    right = right * (values[j][i] + bd[j] * xs[i] + gamma) % m
                t.append(active[i] * (left - right) % m)
            out.append(t)
    for a, s_, ap, sp, z in lookups:
        out.append([l0[i] * (1 - z[i]) % m for i in R])
        out.append([l_last[i] * (z[i] * z[i] - z[i]) % m for i in R])
        out.append([active[i] * (z[lay.rot(i, 1)] * (ap[i] + beta) * (sp[i] + gamma) - z[i] * (a[i] + beta) * (s_[i] + gamma)) % m for i in R])
        out.append([l0[i] * (ap[i] - sp[i]) % m for i in R])
        out.append([active[i] * (ap[i] - sp[i]) * (ap[i] - ap[lay.rot(i, -1)]) % m for i in R])
    return out


def fold(m, acc, terms, y):
    """acc = acc * y + t for every term, row by row"""
    acc = list(acc)
    for t in terms:
        acc = [(a * y + v) % m for a, v in zip(acc, t)]
    return acc


# ---- polynomials over the domain, for the witness ----------------------------------------------------------------------------------
def lagrange_to_coeff(dom: EvaluationDomain, col):
    m, n = _MODULUS[dom.field], dom.n
    wi = [pow(dom.omega_inv, i, m) for i in range(n)]
    return [sum(col[r] * wi[(r * c) % n] for r in range(n)) * dom.ifft_divisor % m for c in range(n)]


def evaluate(m, coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % m
    return acc


def extend(lay: Layout, col):
    """a Lagrange column of the domain -> its values on the rows of the layout"""
    coeffs = lagrange_to_coeff(lay.d, col)
    return [evaluate(lay.m, coeffs, lay.x(i)) for i in range(lay.rows)]


def extended_to_coeff(dom: EvaluationDomain, ext):
    """values on the flat extended domain -> the 2^extended_k coefficients"""
    m, N = _MODULUS[dom.field], 1 << dom.extended_k
    assert len(ext) == N
    wi = [pow(dom.extended_omega_inv, i, m) for i in range(N)]
    zi = pow(dom.g_coset, -1, m)
    return [sum(ext[r] * wi[(r * c) % N] for r in range(N)) * dom.extended_ifft_divisor % m * pow(zi, c, m) % m for c in range(N)]


def residues_mod_vanishing(m, coeffs, n):
    """the coefficients of (polynomial mod X^n - 1): all zero exactly when X^n - 1 divides it"""
    return [sum(coeffs[r::n]) % m for r in range(n)]


def degree(coeffs):
    return max((i for i, c in enumerate(coeffs) if c), default=-1)


def permute_expression_pair(m, a, s_):
    """plonk/lookup/prover.rs permute_expression_pair over the usable rows: A' sorted, S'[i] = A'[i] wherever A' starts a run, the rest of
    the table in the remaining rows"""
    ap = sorted(a)
    left = {}
    for v in s_:
        left[v] = left.get(v, 0) + 1
    sp, repeated = [None] * len(a), []
    for i, v in enumerate(ap):
        if i == 0 or v != ap[i - 1]:
            assert left.get(v, 0) > 0, "an input value is missing from the table"
            sp[i] = v
            left[v] -= 1
        else:
            repeated.append(i)
    rest = [v for v in sorted(left) for _ in range(left[v])]
    assert len(rest) == len(repeated)
    for i, v in zip(repeated, rest):
        sp[i] = v
    return ap, sp


class Witness:
    """Lagrange columns (lists of n integers) that satisfy both arguments: n_columns equality-enabled columns tied by random copies among
    the usable rows, their sigma columns, one product column per set chained through z_s[0] = z_(s-1)[u], n_lookups lookups, random values
    on the blinding rows (u = n - (blinding_factors + 1) usable rows)"""

    def __init__(self, field, k, n_columns, chunk_len, n_lookups, blinding_factors, beta, gamma, seed=1, n_copies=None):
        m = self.m = _MODULUS[field]
        n = self.n = 1 << k
        u = self.usable = n - (blinding_factors + 1)
        assert u >= 2
        rng = random.Random(seed)
        rnd = lambda: rng.randrange(m)  # noqa: E731
        self.field, self.k, self.n_columns, self.chunk_len, self.blinding_factors = field, k, n_columns, chunk_len, blinding_factors
        self.l0 = [1] + [0] * (n - 1)
        self.l_last = [int(i == u) for i in range(n)]
        self.l_blind = [int(i > u) for i in range(n)]
        # copies and the permutation they induce
        self.copies = []
        self.values, self.sigmas, self.zs = [], [], []
        if n_columns:
            cm = CopyModel(n_columns, k)
            for _ in range(n_columns * u // 2 if n_copies is None else n_copies):
                c = (rng.randrange(n_columns), rng.randrange(u), rng.randrange(n_columns), rng.randrange(u))
                self.copies.append(c)
                assert cm.copy(*c)
            cells = [rnd() for _ in range(n_columns * n)]
            for cell in range(n_columns * n):  # one value per cycle: that of its smallest cell
                i, low = cm.mapping[cell], cell
                while i != cell:
                    low = min(low, i)
                    i = cm.mapping[i]
                cells[cell] = cells[low]
            self.values = [cells[j * n:(j + 1) * n] for j in range(n_columns)]
            delta, omega = permutation.delta(field), permutation.omega(field, k)
            self.sigmas = [[pow(delta, cm.mapping[j * n + i] // n, m) * pow(omega, cm.mapping[j * n + i] % n, m) % m for i in range(n)] for j in range(n_columns)]
            start = 1
            for s in range(0, n_columns, chunk_len):
                z = [start]
                for i in range(u):
                    num = den = 1
                    for j in range(s, min(s + chunk_len, n_columns)):
                        num = num * (self.values[j][i] + beta * pow(delta, j, m) * pow(omega, i, m) + gamma) % m
                        den = den * (self.values[j][i] + beta * self.sigmas[j][i] + gamma) % m
                    z.append(z[-1] * num % m * pow(den, -1, m) % m)
                start = z[u]
                self.zs.append(z + [rnd() for _ in range(n - u - 1)])
            assert start == 1, "the copies do not hold"
        self.lookups = []
        for _ in range(n_lookups):
            table = [rnd() for _ in range(max(2, u // 2))]
            s_ = [table[rng.randrange(len(table))] if i >= len(table) else table[i] for i in range(u)]
            a = [table[rng.randrange(len(table))] for _ in range(u)]
            ap, sp = permute_expression_pair(m, a, s_)
            z = [1]
            for i in range(u):
                z.append(z[-1] * (a[i] + beta) * (s_[i] + gamma) % m * pow((ap[i] + beta) * (sp[i] + gamma) % m, -1, m) % m)
            assert z[u] == 1
            blind = lambda: [rnd() for _ in range(n - u)]  # noqa: E731
            self.lookups.append([a + blind(), s_ + blind(), ap + blind(), sp + blind(), z + blind()[1:]])

    def numerator(self, lay: Layout, beta, gamma, y, acc=None, spoil=None):
        """the folded terms on the rows of the layout; spoil(values, sigmas, zs, lookups) may change the Lagrange columns first"""
        cols = [list(c) for c in self.values], [list(c) for c in self.sigmas], [list(c) for c in self.zs], [[list(c) for c in l] for l in self.lookups]
        if spoil:
            spoil(*cols)
        ext = lambda c: extend(lay, c)  # noqa: E731
        values, sigmas, zs = ([ext(c) for c in group] for group in cols[:3])
        lookups = [[ext(c) for c in l] for l in cols[3]]
        terms = term_columns(lay, values, sigmas, zs, lookups, ext(self.l0), ext(self.l_blind), ext(self.l_last), beta, gamma, self.chunk_len, self.blinding_factors)
        return fold(self.m, acc if acc is not None else [0] * lay.rows, terms, y)


def random_stored(seed, count, rows):
    """count columns of rows stored elements (synth.field_elements: every 256-bit pattern below 2^254)"""
    return [np.ascontiguousarray(synth.field_elements(seed + 7919 * c, rows)) for c in range(count)]
