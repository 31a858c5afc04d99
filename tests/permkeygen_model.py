"""The permutation keygen assembly in Python lists: a line-by-line model of csrc/permkeygen.h (halo2_proofs 0.2.0
plonk/permutation/keygen.rs `Assembly::copy`, as recalled), an independent union-find over the same copies, and the copy scripts that
tests/test_permkeygen_host.py and tests/test_gpu_permkeygen.py run.  A cell is column * n + row, n = 2^k."""
import random


class Assembly:
    def __init__(self, n_columns: int, k: int):
        assert n_columns >= 1 and k <= 27 and n_columns << k <= 1 << 32
        self.n_columns, self.k, self.n = n_columns, k, 1 << k
        cells = n_columns << k
        self.mapping = list(range(cells))
        self.aux = list(range(cells))
        self.sizes = [1] * cells
        self.merges = self.swaps = self.ties = 0  # which branches the copies took (the scripts below name the one they are for)

    def copy(self, left_column: int, left_row: int, right_column: int, right_row: int) -> bool:
        """False: refused (a cell outside the columns), nothing changed"""
        if not (0 <= left_column < self.n_columns and 0 <= right_column < self.n_columns and 0 <= left_row < self.n and 0 <= right_row < self.n):
            return False
        left, right = left_column * self.n + left_row, right_column * self.n + right_row
        lc, rc = self.aux[left], self.aux[right]
        if lc == rc:
            return True
        self.merges += 1
        if self.sizes[lc] == self.sizes[rc]:
            self.ties += 1
        if self.sizes[lc] < self.sizes[rc]:
            lc, rc = rc, lc
            self.swaps += 1
        self.sizes[lc] += self.sizes[rc]
        i = rc
        while True:
            self.aux[i] = lc
            i = self.mapping[i]
            if i == rc:
                break
        self.mapping[left], self.mapping[right] = self.mapping[right], self.mapping[left]
        return True


def cycles(mapping):
    """the cycles of a permutation given as a list, each as a frozenset of cells"""
    seen, out = [False] * len(mapping), set()
    for start in range(len(mapping)):
        if seen[start]:
            continue
        cyc, i = [], start
        while not seen[i]:
            seen[i] = True
            cyc.append(i)
            i = mapping[i]
        assert i == start, "not a permutation"
        out.add(frozenset(cyc))
    return out


def components(n_columns: int, k: int, copies):
    """connected components of the copy graph by a plain union-find (no sizes, no cycle walk): what the cycles of ANY correct assembly are,
    whatever the order of its merges.  Refused copies (a cell outside the columns) join nothing."""
    n, cells = 1 << k, n_columns << k
    parent = list(range(cells))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for lc, lr, rc, rr in copies:
        if 0 <= lc < n_columns and 0 <= rc < n_columns and 0 <= lr < n and 0 <= rr < n:
            a, b = find(lc * n + lr), find(rc * n + rr)
            if a != b:
                parent[a] = b
    groups = {}
    for c in range(cells):
        groups.setdefault(find(c), []).append(c)
    return {frozenset(g) for g in groups.values()}


def scripts(n_columns: int, k: int, seed: int = 0x5167A):
    """name -> list of (left_column, left_row, right_column, right_row).  Cells are taken row by row across the columns (cell i of the walk
    = column i % n_columns, row i // n_columns), so that cycles cross columns wherever there is more than one."""
    n, cells = 1 << k, n_columns << k
    at = lambda i: (i % n_columns, i // n_columns)  # noqa: E731
    q = lambda i, j: at(i) + at(j)                  # noqa: E731
    last = cells - 1
    half = min(2, cells // 2)          # two cycles of `half` cells each, then merged: a tie, the left representative stays
    big = min(3, cells - 1)            # a cycle of `big` cells on the right of a single cell: the swap branch (from three cells up)
    rng = random.Random(seed + 1000 * k + n_columns)
    rnd = lambda: (rng.randrange(n_columns), rng.randrange(n))  # noqa: E731
    return {
        "none": [],
        "self": [q(last, last)],
        "twice": [q(0, last), q(0, last)],
        "both_orders": [q(0, last), q(last, 0)],
        "chain": [q(i - 1, i) for i in range(1, min(cells, 12))],
        "equal_merge": [q(i - 1, i) for i in range(1, half)] + [q(half + i - 1, half + i) for i in range(1, half)] + [q(half - 1, 2 * half - 1)],
        "small_left_into_large_right": [q(i, i + 1) for i in range(1, big)] + [q(0, big)],
        "full_cycle": [q(i, i + 1) for i in range(cells - 1)],
        "random": [rnd() + rnd() for _ in range(2000)],
    }
