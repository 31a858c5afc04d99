"""An independent verifier for the proofs of tiny_ram_halo2_amd.plonk, in Python integers over oracle/pasta.py alone (its field and curve
arithmetic, evaluate_expression, ipa_verify_proof): it reads the recorded proof items and evaluates the verification equations of halo2_proofs
0.2.0 (plonk/verifier.rs, poly/multiopen/verifier.rs, poly/commitment/verifier.rs, as recalled) itself.  It imports neither the package's plonk
nor its multiopen module; what it shares with them is the protocol.

The group work -- sums of scalar * point, and the opening's final equation -- has a second implementation over the C++ oracle (verify's
group="cpp": cpu_ref.best_multiexp, common.ipa_verify_fast) for 2^10 rows and more, where the Python one would take minutes; everything else
is the same integers for both.  tests/test_plonk_model.py holds the two against each other.

A proof is the list of items a Writer recorded: ("P", affine point or None) and ("S", canonical integer), in the order they were written.
Writer / Reader speak limbs (the device side's interface), ModelReader speaks integers; all three absorb the same bytes and so squeeze the same
challenges, which they keep in `squeezes`.

Expressions are the oracle's tuples: ("const", v) | ("col", (kind, column), rotation) | ("neg", e) | ("sum", a, b) | ("prod", a, b) |
("scaled", e, v)."""
import hashlib

import numpy as np

import pasta as o


# ---- transcripts -------------------------------------------------------------------------------------------------------------------------
class _Sponge:
    def __init__(self, curve: str):
        self.cv = o.CURVES[curve]
        self.h = hashlib.blake2b(b"trh-plonk-test-transcript")
        self.squeezes = []

    def absorb_point(self, pt):
        self.h.update(b"P" + (bytes(64) if pt is None else pt[0].to_bytes(32, "little") + pt[1].to_bytes(32, "little")))

    def absorb_scalar(self, v):
        self.h.update(b"S" + (v % self.cv.scalar.m).to_bytes(32, "little"))

    def squeeze_challenge_scalar(self):
        self.h.update(b"C")
        c = int.from_bytes(self.h.digest(), "little") % self.cv.scalar.m
        self.squeezes.append(c)
        return c

    def _point_of(self, limbs):
        limbs = [int(v) for v in np.asarray(limbs).reshape(-1)]
        return self.cv.jacobian_limbs_to_affine(limbs) if len(limbs) == 12 else self.cv.affine_from_limbs(limbs)


class Writer(_Sponge):
    """the prover's transcript: points arrive as 12-limb normalised Jacobian (or 8-limb affine) words, scalars as Montgomery limbs"""

    def __init__(self, curve: str):
        super().__init__(curve)
        self.items = []

    def common_point(self, limbs):
        self.absorb_point(self._point_of(limbs))

    def common_scalar(self, limbs):
        self.absorb_scalar(self.cv.scalar.from_limbs([int(v) for v in limbs]))

    def write_point(self, limbs):
        pt = self._point_of(limbs)
        self.absorb_point(pt)
        self.items.append(("P", pt))

    def write_scalar(self, limbs):
        v = self.cv.scalar.from_limbs([int(x) for x in limbs])
        self.absorb_scalar(v)
        self.items.append(("S", v))


class _ItemReader(_Sponge):
    def __init__(self, curve: str, items):
        super().__init__(curve)
        self.items, self.at = list(items), 0

    def _next(self, kind):
        if self.at >= len(self.items) or self.items[self.at][0] != kind:
            raise ValueError(f"item {self.at} of the proof is no {kind}")
        self.at += 1
        return self.items[self.at - 1][1]

    def finished(self):
        return self.at == len(self.items)


class Reader(_ItemReader):
    """the device verifier's transcript: read_point() -> the 8-limb affine POD, read_scalar() -> int"""

    def common_point(self, limbs):
        self.absorb_point(self._point_of(limbs))

    def common_scalar(self, limbs):
        self.absorb_scalar(self.cv.scalar.from_limbs([int(v) for v in limbs]))

    def read_point(self):
        pt = self._next("P")
        self.absorb_point(pt)
        return np.array(self.cv.affine_limbs(pt), dtype=np.uint64)

    def read_scalar(self):
        v = self._next("S")
        self.absorb_scalar(v)
        return v


class ModelReader(_ItemReader):
    """the model's transcript: affine tuples and integers throughout"""

    def common_point(self, pt):
        self.absorb_point(pt)

    def common_scalar(self, v):
        self.absorb_scalar(v)

    def read_point(self):
        pt = self._next("P")
        self.absorb_point(pt)
        return pt

    def read_scalar(self):
        v = self._next("S")
        self.absorb_scalar(v)
        return v


# ---- the constraint system as data ---------------------------------------------------------------------------------------------------------
def expr_degree(node) -> int:
    tag = node[0]
    if tag == "const":
        return 0
    if tag == "col":
        return 1
    if tag in ("neg", "scaled"):
        return expr_degree(node[1])
    a, b = expr_degree(node[1]), expr_degree(node[2])
    return max(a, b) if tag == "sum" else a + b


def expr_queries(node, out):
    """appends the (key, rotation) queries of an expression that `out` does not hold yet, depth first, left to right"""
    tag = node[0]
    if tag == "col":
        if (node[1], node[2]) not in out:
            out.append((node[1], node[2]))
    elif tag in ("neg", "scaled"):
        expr_queries(node[1], out)
    elif tag in ("sum", "prod"):
        expr_queries(node[1], out)
        expr_queries(node[2], out)


class System:
    """gates: expressions; lookups: (input expressions, table expressions); permutation_columns: (kind, column) keys"""

    def __init__(self, gates, lookups, permutation_columns, num_advice, minimum_degree=None):
        self.gates, self.lookups, self.permutation_columns = list(gates), [(list(i), list(t)) for i, t in lookups], list(permutation_columns)
        self.num_advice, self.minimum_degree = num_advice, minimum_degree
        found = []
        for g in self.gates:
            expr_queries(g, found)
        for inputs, tables in self.lookups:
            for e in inputs + tables:
                expr_queries(e, found)
        for key in self.permutation_columns:
            expr_queries(("col", key, 0), found)
        self.queries = {kind: [(key[1], r) for key, r in found if key[0] == kind] for kind in ("instance", "advice", "fixed")}

    def degree(self):
        need = [3, self.minimum_degree or 0] + [expr_degree(g) for g in self.gates]
        for inputs, tables in self.lookups:
            need.append(max(4, 2 + max([1] + [expr_degree(e) for e in inputs]) + max([1] + [expr_degree(e) for e in tables])))
        return max(need)

    def blinding_factors(self):
        per_column = [0] * self.num_advice
        for c, _ in self.queries["advice"]:
            per_column[c] += 1
        return max([3] + per_column) + 2

    def chunk_len(self):
        return self.degree() - 2

    def n_sets(self):
        return (len(self.permutation_columns) + self.chunk_len() - 1) // self.chunk_len()


# ---- pieces of the verifier ----------------------------------------------------------------------------------------------------------------
def interpolate(m, xs, ys):
    """Lagrange interpolation by Newton's divided differences -> coefficients, lowest first"""
    k = len(xs)
    dd = [y % m for y in ys]
    for level in range(1, k):
        for i in range(k - 1, level - 1, -1):
            dd[i] = (dd[i] - dd[i - 1]) * pow((xs[i] - xs[i - level]) % m, -1, m) % m
    coeffs = [0] * k
    for i in range(k - 1, -1, -1):  # Horner over the Newton form: coeffs = coeffs * (X - xs[i]) + dd[i]
        shifted = [0] + coeffs[:-1]
        coeffs = [(s - xs[i] * c) % m for s, c in zip(shifted, coeffs)]
        coeffs[0] = (coeffs[0] + dd[i]) % m
    return coeffs


def horner(m, coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % m
    return acc


def l_i(m, n, omega, i, x):
    """the Lagrange basis polynomial of row i (mod n) of the 2^k-row domain at x, in closed form"""
    w = pow(omega, i % n, m)
    return w * (pow(x, n, m) - 1) % m * pow(n * (x - w) % m, -1, m) % m


def intermediate_sets(queries):
    """(point, key, eval) queries -> (members, point_sets): members = [(key, set index)] in order of the keys' first appearance, sets numbered
    in order of first appearance, each set's points in order of the points' first appearance; and evals[(key, point)]"""
    seen_points, per_key, evals = [], {}, {}
    for p, key, e in queries:
        if p not in seen_points:
            seen_points.append(p)
        per_key.setdefault(key, set()).add(seen_points.index(p))
        evals.setdefault((key, p), e)
    sets, members = [], []
    for key, idx in per_key.items():  # dicts keep insertion order
        s = sorted(idx)
        if s not in sets:
            sets.append(s)
        members.append((key, sets.index(s)))
    return members, [[seen_points[i] for i in s] for s in sets], evals


def chain(m, rows, link):
    """the product columns of consecutive sets linked: row r times the product of the earlier rows' ORIGINAL values at `link`"""
    out, carry = [], 1
    for row in rows:
        out.append([v * carry % m for v in row])
        carry = carry * row[link] % m
    return out


class _AtX:
    """a column as evaluate_expression indexes it (row 0, rotation r -> index r mod n), backed by the proof's evaluations"""

    def __init__(self, evals, key, n):
        self.evals, self.key, self.n = evals, key, n

    def __getitem__(self, i):
        return self.evals[(self.key, i if i <= self.n // 2 else i - self.n)]


def combine(cv, terms):
    """sum of scalar * point over (scalar, point) terms, one scalar multiplication per distinct point"""
    by_point = {}
    for s, pt in terms:
        by_point[pt] = (by_point.get(pt, 0) + s) % cv.scalar.m
    acc = None
    for pt, s in by_point.items():
        acc = cv.add(acc, cv.mul(s, pt))
    return acc


# ---- the group work of the verifier: two operations, two implementations -------------------------------------------------------------------
class PythonGroup:
    """points are the oracle's affine tuples (None: the identity), the arithmetic is oracle/pasta.py's Python integers: 7 ms for a scalar
    multiplication, so for 2^5 rows"""

    def __init__(self, curve: str):
        self.curve, self.cv = curve, o.CURVES[curve]

    def lift(self, pt):
        """a proof item's point (affine tuple) in this group's form"""
        return pt

    def affine(self, pt):
        """-> the affine tuple the transcript absorbs"""
        return pt

    def combine(self, terms):
        """sum of scalar * point over (scalar, point) terms"""
        return combine(self.cv, terms)

    def opening_holds(self, k, g, w, u, commitment, x3, v, s_commitment, xi, z, rounds, challenges, c, f):
        """the final equation of the opening (poly/commitment/verifier.rs)"""
        return o.ipa_verify_proof(self.cv, k, g, w, u, commitment, x3, v, s_commitment, xi, z, rounds, challenges, c, f)


class CppGroup:
    """points are 8-limb affine rows (all zero: the identity) as the device hands them out, so g and g_lagrange stay the (n, 8) arrays they
    were downloaded as; the arithmetic is the C++ oracle's (cpu_ref.best_multiexp, common.ipa_verify_fast): 2^14 pairs in a tenth of a second"""

    def __init__(self, curve: str):
        self.curve, self.cv = curve, o.CURVES[curve]

    def lift(self, pt):
        return np.array(self.cv.affine_limbs(pt), dtype=np.uint64)

    def affine(self, pt):
        return self.cv.affine_from_limbs([int(v) for v in np.asarray(pt).reshape(8)])

    def combine(self, terms):
        import cpu_ref
        f = self.cv.scalar
        scalars = np.array([f.limbs(s % f.m) for s, _ in terms], dtype=np.uint64)
        points = np.stack([np.asarray(pt, dtype=np.uint64).reshape(8) for _, pt in terms])
        return cpu_ref.to_affine(self.curve, cpu_ref.best_multiexp(self.curve, scalars, points, threads=4))

    def opening_holds(self, k, g, w, u, commitment, x3, v, s_commitment, xi, z, rounds, challenges, c, f):
        from common import ipa_verify_fast
        return ipa_verify_fast(self.curve, k, np.asarray(g, dtype=np.uint64).reshape(1 << k, 8), w, u, commitment, x3, v, s_commitment, xi, z, rounds, challenges, c, f)


GROUPS = {"python": PythonGroup, "cpp": CppGroup}
REFUSALS = ("instance values", "vanishing identity", "transcript", "opening")


def verify(curve, k, g, g_lagrange, w, u, system, fixed_commitments, sigma_commitments, transcript_repr, instances, items, group="python"):
    """-> (accepted, squeezes, refused): refused is None or the one of REFUSALS that names the check which said no -- too many instance values,
    the vanishing identity at x, a transcript that the proof does not exhaust, the opening.  g, g_lagrange: n points; w, u: points; the
    commitments of the key: all in the form of `group` (affine tuples for "python", 8-limb rows for "cpp"); instances: one list of integers
    per instance column; items: the recorded proof.  Only the sums of scalar * point and the opening's final equation go through the group;
    the transcript, the vanishing identity, the intermediate sets and the interpolation are integers here for both."""
    grp = GROUPS[group](curve)
    cv = o.CURVES[curve]
    f = cv.scalar
    m, n = f.m, 1 << k
    omega = f.omega(k)
    tr = ModelReader(curve, items)
    read_point = lambda: grp.lift(tr.read_point())  # noqa: E731
    bf, sets, chunk = system.blinding_factors(), system.n_sets(), system.chunk_len()
    usable, last = n - (bf + 1), -(bf + 1)
    n_lookups, n_perm, pieces_count = len(system.lookups), len(system.permutation_columns), system.degree() - 1
    com = {}
    tr.common_scalar(transcript_repr)
    for i, values in enumerate(instances):
        if len(values) > usable:
            return False, tr.squeezes, REFUSALS[0]
        pt = grp.combine([(1, w)] + [(v, g_lagrange[row]) for row, v in enumerate(values)])  # commit_lagrange with Blind::default() = 1
        tr.common_point(grp.affine(pt))
        com[(("instance", i))] = [(1, pt)]
    for i in range(system.num_advice):
        com[("advice", i)] = [(1, read_point())]
    theta = tr.squeeze_challenge_scalar()
    for l in range(n_lookups):
        com[("A'", l)] = [(1, read_point())]
        com[("S'", l)] = [(1, read_point())]
    beta, gamma = tr.squeeze_challenge_scalar(), tr.squeeze_challenge_scalar()
    for s in range(sets):
        com[("Zp", s)] = [(1, read_point())]
    for l in range(n_lookups):
        com[("Zl", l)] = [(1, read_point())]
    com["random"] = [(1, read_point())]
    y = tr.squeeze_challenge_scalar()
    h_pieces = [read_point() for _ in range(pieces_count)]
    x = tr.squeeze_challenge_scalar()
    xn = pow(x, n, m)
    com["h"] = [(pow(xn, i, m), pt) for i, pt in enumerate(h_pieces)]
    for i, pt in enumerate(fixed_commitments):
        com[("fixed", i)] = [(1, pt)]
    for j, pt in enumerate(sigma_commitments):
        com[("sigma", j)] = [(1, pt)]
    # the evaluations, in the prover's order
    ev = {}
    for kind in ("instance", "advice", "fixed"):
        for c, r in system.queries[kind]:
            ev[((kind, c), r)] = tr.read_scalar()
    h_eval = tr.read_scalar()
    random_eval = tr.read_scalar()
    sigma_evals = [tr.read_scalar() for _ in range(n_perm)]
    zp = []
    for s in range(sets):
        zp.append({0: tr.read_scalar(), 1: tr.read_scalar()})
        if s != sets - 1:
            zp[s][last] = tr.read_scalar()
    lk = []
    for l in range(n_lookups):
        lk.append(dict(z=tr.read_scalar(), z_next=tr.read_scalar(), a=tr.read_scalar(), a_prev=tr.read_scalar(), s=tr.read_scalar()))

    # the vanishing identity
    columns = {key: _AtX(ev, key, n) for key in {q[0] for q in ev}}
    at_x = lambda e: o.evaluate_expression(f, e, columns, 0, n, 1)  # noqa: E731
    l_0, l_last = l_i(m, n, omega, 0, x), l_i(m, n, omega, usable, x)
    l_blind = sum(l_i(m, n, omega, row, x) for row in range(usable + 1, n)) % m
    l_active = (1 - l_last - l_blind) % m
    exprs = [at_x(g_) for g_ in system.gates]
    if n_perm:
        delta = f.DELTA
        exprs.append(l_0 * (1 - zp[0][0]))
        exprs.append(l_last * (zp[-1][0] ** 2 - zp[-1][0]))
        for s in range(1, sets):
            exprs.append(l_0 * (zp[s][0] - zp[s - 1][last]))
        for s in range(sets):
            lhs, rhs = zp[s][1], zp[s][0]
            for j in range(s * chunk, min(n_perm, (s + 1) * chunk)):
                value = ev[(system.permutation_columns[j], 0)]
                lhs = lhs * (value + beta * sigma_evals[j] + gamma) % m
                rhs = rhs * (value + beta * pow(delta, j, m) * x + gamma) % m
            exprs.append(l_active * (lhs - rhs))
    for l, (inputs, tables) in enumerate(system.lookups):
        a_c = s_c = 0
        for e in inputs:
            a_c = (a_c * theta + at_x(e)) % m
        for e in tables:
            s_c = (s_c * theta + at_x(e)) % m
        q = lk[l]
        exprs.append(l_0 * (1 - q["z"]))
        exprs.append(l_last * (q["z"] ** 2 - q["z"]))
        exprs.append(l_active * (q["z_next"] * (q["a"] + beta) * (q["s"] + gamma) - q["z"] * (a_c + beta) * (s_c + gamma)))
        exprs.append(l_0 * (q["a"] - q["s"]))
        exprs.append(l_active * (q["a"] - q["s"]) * (q["a"] - q["a_prev"]))
    folded = 0
    for e in exprs:
        folded = (folded * y + e) % m
    if (folded - h_eval * (xn - 1)) % m:
        return False, tr.squeezes, REFUSALS[1]

    # the queries, in the prover's order
    rot = lambda r: x * pow(omega, r % n, m) % m  # noqa: E731
    queries = []
    for kind in ("instance", "advice"):
        queries += [(rot(r), (kind, c), ev[((kind, c), r)]) for c, r in system.queries[kind]]
    for s in range(sets):
        queries += [(rot(0), ("Zp", s), zp[s][0]), (rot(1), ("Zp", s), zp[s][1])]
    for s in range(sets - 2, -1, -1):
        queries.append((rot(last), ("Zp", s), zp[s][last]))
    for l in range(n_lookups):
        q = lk[l]
        queries += [(rot(0), ("Zl", l), q["z"]), (rot(0), ("A'", l), q["a"]), (rot(0), ("S'", l), q["s"]), (rot(-1), ("A'", l), q["a_prev"]), (rot(1), ("Zl", l), q["z_next"])]
    queries += [(rot(r), ("fixed", c), ev[(("fixed", c), r)]) for c, r in system.queries["fixed"]]
    queries += [(rot(0), ("sigma", j), sigma_evals[j]) for j in range(n_perm)]
    queries += [(rot(0), "h", h_eval), (rot(0), "random", random_eval)]

    # multiopen
    x1, x2 = tr.squeeze_challenge_scalar(), tr.squeeze_challenge_scalar()
    members, point_sets, claimed = intermediate_sets(queries)
    q_com = [[] for _ in point_sets]
    q_evals_claimed = [[0] * len(pts) for pts in point_sets]
    for key, s in members:
        q_com[s] = [(c * x1 % m, pt) for c, pt in q_com[s]] + com[key]
        q_evals_claimed[s] = [(acc * x1 + claimed[(key, p)]) % m for acc, p in zip(q_evals_claimed[s], point_sets[s])]
    q_prime = read_point()
    x3 = tr.squeeze_challenge_scalar()
    q_evals = [tr.read_scalar() for _ in point_sets]
    expected = 0
    for pts, claimed_evals, q_eval in zip(point_sets, q_evals_claimed, q_evals):
        value = (q_eval - horner(m, interpolate(m, pts, claimed_evals), x3)) % m
        for p in pts:
            value = value * pow((x3 - p) % m, -1, m) % m
        expected = (expected * x2 + value) % m
    x4 = tr.squeeze_challenge_scalar()
    final, v = [(1, q_prime)], expected
    for terms, q_eval in zip(q_com, q_evals):
        final = [(c * x4 % m, pt) for c, pt in final] + terms
        v = (v * x4 + q_eval) % m
    s_commitment = read_point()
    xi, z = tr.squeeze_challenge_scalar(), tr.squeeze_challenge_scalar()
    rounds, challenges = [], []
    for _ in range(k):
        rounds.append((read_point(), read_point()))
        challenges.append(tr.squeeze_challenge_scalar())
    c, f_ = tr.read_scalar(), tr.read_scalar()
    if not tr.finished():
        return False, tr.squeezes, REFUSALS[2]
    ok = grp.opening_holds(k, g, w, u, grp.combine(final), x3, v, s_commitment, xi, z, rounds, challenges, c, f_)
    return ok, tr.squeezes, None if ok else REFUSALS[3]
