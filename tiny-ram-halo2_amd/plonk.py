"""keygen, create_proof and verify_proof of halo2_proofs 0.2.0 (plonk/{circuit, keygen, prover, verifier}.rs, as recalled; the reference reaches
them from gen_proofs_and_verify, src/test_utils.rs:21-68 of the reference) put together from the device entries of this package: one circuit
per proof, selectors as plain fixed columns, the proof a byte string or -- for tests that record items -- whatever a transcript object keeps.

    cs = ConstraintSystem(field, num_fixed, num_advice, num_instance, gates, lookups, permutation_columns, minimum_degree=None)
    vk, pk = keygen(params, cs, fixed_columns, copies)
    create_proof(params, pk, instances, advice, rng, transcript)              transcript: a writer
    guard = verify_proof(params, vk, instances, transcript)                    transcript: a reader; raises VerifyError
    single_verify(params, guard)                                               the guard's MSM is the identity
    proof = create_proof_bytes(params, pk, instances, advice, rng)             Blake2bWrite::init(vec![]) .. transcript.finalize()
    guard = verify_proof_bytes(params, vk, instances, proof)                   Blake2bRead::init(&proof[..]); raises VerifyError
    BatchVerifier().add_proof(instances, proof) .. .finalize(params, vk)       plonk::BatchVerifier
    gen_proofs_and_verify(params, vk, pk, inputs, rng)                         the reference's harness, restated

Every operation on a column-sized vector is a libtrh entry on the current stream (commitments, transforms, expr.GateEvaluator,
permutation.grand_products_terms / chain_products / lookup_permute_batch, quotient.QuotientTerms, api.poly_eval_batch_dev, multiopen); the host does
O(#columns) integer work and nothing per row.

A writer has common_point(jacobian12), common_scalar(limbs4), write_point(jacobian12), write_scalar(limbs4) and squeeze_challenge_scalar() -> int;
a reader has read_point() -> the 8-limb affine POD and read_scalar() -> int in place of the writes.  Limbs are Montgomery words, as everywhere
at the ABI.  transcript.Blake2bWrite / Blake2bRead are the writer and the reader of upstream's byte format (BLAKE2b, Challenge255), kept
inside libtrh.so; the *_bytes functions use them.  The bytes are upstream's ENCODING of this module's item order (next paragraph), so a proof
made by upstream does not verify here, nor the other way round.

Deviations from upstream, all on purpose: the evaluation h(x) of the folded quotient pieces is written in front of the random polynomial's, so
that the verifier can test the vanishing identity on scalars and refuse (VerifyError) before any group work; the blinding scalars are drawn
from one trh_rng stream column-block by column-block instead of cell by cell; with strict_lookups=False a lookup whose input is missing from
its table does not stop the prover (upstream: Error::ConstraintSystemFailure) -- its permuted columns are the unpermuted ones, which no
verifier accepts."""
from __future__ import annotations

import hashlib
import secrets

import numpy as np

from . import api, expr, ipa, multiopen, permutation, quotient, witness
from .transcript import Blake2bRead, Blake2bWrite, TranscriptError
from .poly import _MODULUS, EvaluationDomain, _mont


class VerifyError(Exception):
    """the proof does not satisfy the vanishing identity at x (or is malformed): refused before any group work"""


# ---- the constraint system ---------------------------------------------------------------------------------------------------------------
def _walk(e, visit):
    """the queries of an expression, depth first, left to right"""
    if isinstance(e, expr._Query):
        visit(e)
    elif isinstance(e, (expr.Negated, expr.Scaled)):
        _walk(e.e, visit)
    elif isinstance(e, (expr.Sum, expr.Product)):
        _walk(e.a, visit)
        _walk(e.b, visit)
    elif not isinstance(e, expr.Constant):
        raise TypeError(f"not an Expression: {e!r}")


def _describe(e) -> str:
    if isinstance(e, expr.Constant):
        return f"c{e.value}"
    if isinstance(e, expr._Query):
        return f"{e.kind[0]}{e.column}@{e.rotation}"
    if isinstance(e, expr.Negated):
        return f"-({_describe(e.e)})"
    if isinstance(e, expr.Scaled):
        return f"({_describe(e.e)})*{e.value}"
    op = "+" if isinstance(e, expr.Sum) else "*"
    return f"({_describe(e.a)}{op}{_describe(e.b)})"


def evaluate(e, m: int, query) -> int:
    """Expression::evaluate over integers; query(kind, column, rotation) -> int"""
    if isinstance(e, expr.Constant):
        return e.value % m
    if isinstance(e, expr._Query):
        return query(e.kind, e.column, e.rotation)
    if isinstance(e, expr.Negated):
        return -evaluate(e.e, m, query) % m
    if isinstance(e, expr.Scaled):
        return evaluate(e.e, m, query) * e.value % m
    a, b = evaluate(e.a, m, query), evaluate(e.b, m, query)
    return (a + b) % m if isinstance(e, expr.Sum) else a * b % m


class ConstraintSystem:
    """plonk::ConstraintSystem for one circuit: gates (Expressions that vanish on the usable rows), lookups (pairs of equally long lists of
    input and table Expressions) and the equality-enabled columns, as (kind, index) with kind "advice", "fixed" or "instance", in the order
    the permutation argument takes them.  The query lists are in order of first appearance over the gates, then the lookups' inputs and
    tables, then -- enable_equality -- the permutation columns at the current row."""

    def __init__(self, field: str, num_fixed: int, num_advice: int, num_instance: int, gates, lookups, permutation_columns, minimum_degree: int | None = None):
        self.field, self.num_fixed, self.num_advice, self.num_instance = field, num_fixed, num_advice, num_instance
        self.gates = list(gates)
        self.lookups = [(list(i), list(t)) for i, t in lookups]
        self.permutation_columns = [tuple(c) for c in permutation_columns]
        self.minimum_degree = minimum_degree
        self.queries = {"advice": [], "fixed": [], "instance": []}
        count = {"advice": num_advice, "fixed": num_fixed, "instance": num_instance}

        def visit(q):
            if q.kind not in self.queries:
                raise ValueError(f"a {q.kind} query: selectors are plain fixed columns here (expr.Fixed)")
            if not 0 <= q.column < count[q.kind]:
                raise ValueError(f"{q.kind} column {q.column} of {count[q.kind]}")
            if (q.column, q.rotation) not in self.queries[q.kind]:
                self.queries[q.kind].append((q.column, q.rotation))

        for g in self.gates:
            _walk(g, visit)
        for inputs, tables in self.lookups:
            if not inputs or len(inputs) != len(tables):
                raise ValueError("a lookup takes as many table expressions as input expressions, at least one")
            for e in inputs + tables:
                _walk(e, visit)
        for kind, column in self.permutation_columns:
            visit({"advice": expr.Advice, "fixed": expr.Fixed, "instance": expr.Instance}[kind](column, 0))
        if len(set(self.permutation_columns)) != len(self.permutation_columns):
            raise ValueError("a column is equality-enabled twice")

    advice_queries = property(lambda self: self.queries["advice"])
    fixed_queries = property(lambda self: self.queries["fixed"])
    instance_queries = property(lambda self: self.queries["instance"])

    def degree(self) -> int:
        """ConstraintSystem::degree: the permutation argument needs 3, a lookup max(4, 2 + input degree + table degree), a gate its own"""
        d = 3
        for inputs, tables in self.lookups:
            d = max(d, 4, 2 + max(1, max(e.degree() for e in inputs)) + max(1, max(e.degree() for e in tables)))
        for g in self.gates:
            d = max(d, g.degree())
        return max(d, self.minimum_degree or 0)

    def blinding_factors(self) -> int:
        """max(3, most queries of any advice column) + 1 for the opening at x3 + 1 for the row the product columns end on"""
        most = max([sum(1 for c, _ in self.advice_queries if c == col) for col in range(self.num_advice)], default=1)
        return max(3, most) + 2

    def usable_rows(self, n: int) -> int:
        return n - (self.blinding_factors() + 1)

    def chunk_len(self) -> int:
        return self.degree() - 2

    def n_sets(self) -> int:
        return -(-len(self.permutation_columns) // self.chunk_len())

    def compressed(self, theta: int):
        """-> (inputs, tables): one Expression per lookup, its expressions folded by theta (acc * theta + e)"""
        def fold(es):
            acc = es[0]
            for e in es[1:]:
                acc = expr.Scaled(acc, theta) + e
            return acc
        return [fold(i) for i, _ in self.lookups], [fold(t) for _, t in self.lookups]

    def describe(self) -> str:
        return "|".join([self.field, f"{self.num_fixed},{self.num_advice},{self.num_instance},{self.minimum_degree}"] + [_describe(g) for g in self.gates]
                        + [";".join(_describe(e) for e in i) + "->" + ";".join(_describe(e) for e in t) for i, t in self.lookups]
                        + [f"{k}{c}" for k, c in self.permutation_columns])

    # the order of the evaluations in the proof and of the queries into multiopen: (key, rotation) pairs.  Keys: (kind, column) for the
    # circuit's columns, ("sigma", j), ("perm_z", set), ("lk_a" / "lk_s" / "lk_z", lookup) for A', S' and the product column, "h", "random"
    def last_rotation(self) -> int:
        return -(self.blinding_factors() + 1)

    def eval_plan(self):
        """every evaluation the prover writes, in order; "h" stands for the folded quotient pieces"""
        sets, last = self.n_sets(), self.last_rotation()
        plan = [((kind, c), r) for kind in ("instance", "advice", "fixed") for c, r in self.queries[kind]]
        plan += [("h", 0), ("random", 0)]
        plan += [(("sigma", j), 0) for j in range(len(self.permutation_columns))]
        for s in range(sets):
            plan += [(("perm_z", s), 0), (("perm_z", s), 1)] + ([(("perm_z", s), last)] if s + 1 < sets else [])
        for l in range(len(self.lookups)):
            plan += [(("lk_z", l), 0), (("lk_z", l), 1), (("lk_a", l), 0), (("lk_a", l), -1), (("lk_s", l), 0)]
        return plan

    def query_plan(self):
        """the queries into multiopen, in order"""
        sets, last = self.n_sets(), self.last_rotation()
        plan = [((kind, c), r) for kind in ("instance", "advice") for c, r in self.queries[kind]]
        for s in range(sets):
            plan += [(("perm_z", s), 0), (("perm_z", s), 1)]
        plan += [(("perm_z", s), last) for s in reversed(range(sets - 1))]
        for l in range(len(self.lookups)):
            plan += [(("lk_z", l), 0), (("lk_a", l), 0), (("lk_s", l), 0), (("lk_a", l), -1), (("lk_z", l), 1)]
        plan += [(("fixed", c), r) for c, r in self.fixed_queries]
        plan += [(("sigma", j), 0) for j in range(len(self.permutation_columns))]
        return plan + [("h", 0), ("random", 0)]


# ---- keygen --------------------------------------------------------------------------------------------------------------------------------
class VerifyingKey:
    def __init__(self, cs, domain, fixed_commitments, sigma_commitments):
        self.cs, self.domain = cs, domain
        self.fixed_commitments, self.sigma_commitments = fixed_commitments, sigma_commitments  # (count, 8) affine PODs
        digest = hashlib.blake2b(b"trh-plonk-vk" + cs.describe().encode() + bytes([domain.k]) + fixed_commitments.tobytes() + sigma_commitments.tobytes())
        self.transcript_repr = int.from_bytes(digest.digest(), "little") % _MODULUS[cs.field]


class ProvingKey:
    def __init__(self, vk, fixed_values, fixed_polys, permutations, sigma_polys):
        self.vk, self.fixed_values, self.fixed_polys, self.permutations, self.sigma_polys = vk, fixed_values, fixed_polys, permutations, sigma_polys
        self._basis = {}

    def basis(self, n_blocks):
        """l0, l_blind, l_last on the extended domain in the asked layout (quotient.lagrange_basis_columns), made once per layout"""
        if n_blocks not in self._basis:
            self._basis[n_blocks] = quotient.lagrange_basis_columns(self.vk.domain, self.vk.cs.blinding_factors(), n_blocks)
        return self._basis[n_blocks]


def _device():
    import torch
    return torch.device("cuda", max(int(api.lib().trh_ctx_device(None)), 0))


def _ones(field: str, count: int) -> np.ndarray:
    return np.tile(_mont(field, 1), (count, 1))  # Blind::default()


def keygen(params, cs: ConstraintSystem, fixed_columns, copies):
    """keygen_vk + keygen_pk.  fixed_columns: device tensor (num_fixed, n, 4) of Lagrange values (None when there is no fixed column); copies:
    (left column, left row, right column, right row) quads over the indices of cs.permutation_columns.  -> (VerifyingKey, ProvingKey)"""
    import torch
    sf, k, n = cs.field, params.k, params.n
    assert api.SCALAR_FIELD[params.curve] == sf
    if cs.blinding_factors() + 3 > n:
        raise ValueError(f"2^{k} rows leave no usable row beside {cs.blinding_factors()} blinding factors")
    dom = EvaluationDomain(sf, cs.degree(), k)
    dev = _device()
    if cs.num_fixed:
        fixed_values = fixed_columns.contiguous()
        assert fixed_values.shape == (cs.num_fixed, n, 4)
        fixed_commitments = params.commit_lagrange_batch(fixed_values, _ones(sf, cs.num_fixed))[:, :8].copy()
        fixed_polys = dom.lagrange_to_coeff(fixed_values.clone())
    else:
        fixed_values = fixed_polys = torch.empty((0, n, 4), dtype=torch.int64, device=dev)
        fixed_commitments = np.zeros((0, 8), dtype=np.uint64)
    p = len(cs.permutation_columns)
    if p:
        asm = permutation.Assembly(sf, k, p)
        copies = np.asarray(list(copies), dtype=np.int64).reshape(-1, 4)
        if copies.size:
            asm.copy_many(copies)
        sigma_commitments = asm.build_vk(params)[:, :8].copy()
        permutations, sigma_polys, _ = asm.build_pk(dom)
        asm.destroy()
    else:
        permutations = sigma_polys = torch.empty((0, n, 4), dtype=torch.int64, device=dev)
        sigma_commitments = np.zeros((0, 8), dtype=np.uint64)
    vk = VerifyingKey(cs, dom, fixed_commitments, sigma_commitments)
    return vk, ProvingKey(vk, fixed_values, fixed_polys, permutations, sigma_polys)


# ---- the prover ----------------------------------------------------------------------------------------------------------------------------
def _instance_columns(cs, n, instances, dev):
    import torch
    u = cs.usable_rows(n)
    if len(instances) != cs.num_instance:
        raise ValueError(f"{len(instances)} instance columns, the circuit has {cs.num_instance}")
    for i, values in enumerate(instances):
        if len(values) > u:
            raise ValueError(f"instance column {i}: {len(values)} values, {u} usable rows")
    is_words = [isinstance(values, np.ndarray) and values.dtype.kind == "u" for values in instances]
    if any(is_words):
        # columns given as machine words are expanded on the device (witness.columns_from_ints): no big integer per value on the host
        out = torch.zeros((cs.num_instance, n, 4), dtype=torch.int64, device=dev)
        for i, values in enumerate(instances):
            if is_words[i]:
                witness.columns_from_ints(cs.field, values.reshape(-1), n, out=out[i])
            elif len(values):
                out[i, :len(values)] = torch.from_numpy(multiopen._limbs_many(cs.field, list(values)).view(np.int64)).to(dev)
        return out
    cols = np.zeros((cs.num_instance, n, 4), dtype=np.uint64)
    for i, values in enumerate(instances):
        if len(values):
            cols[i, :len(values)] = multiopen._limbs_many(cs.field, list(values))
    return torch.from_numpy(cols.view(np.int64)).to(dev)


def _rotated(x: int, omega: int, omega_inv: int, r: int, m: int) -> int:
    return x * pow(omega if r >= 0 else omega_inv, abs(r), m) % m


def create_proof(params, pk: ProvingKey, instances, advice, rng: api.Rng, transcript, layout: str = "blocks", strict_lookups: bool = True) -> None:
    """plonk::create_proof for one circuit.  instances: per instance column a list of integers or a numpy array of unsigned machine words (the
    array is expanded on the device: witness.columns_from_ints); advice: device tensor (num_advice, n, 4) of
    Lagrange values, whose rows behind the usable ones are ignored (a copy gets the blinding rows); rng: the trh_rng stream every random
    scalar comes from; layout: "blocks" (coset blocks) or "flat" for the extended domain h(X) is built on -- the proofs are identical."""
    import torch
    vk = pk.vk
    cs, dom = vk.cs, vk.domain
    sf, k, n = cs.field, params.k, params.n
    m = _MODULUS[sf]
    bf, u = cs.blinding_factors(), cs.usable_rows(n)
    n_lookups, n_perm, sets, chunk = len(cs.lookups), len(cs.permutation_columns), cs.n_sets(), cs.chunk_len()
    assert layout in ("blocks", "flat") and api.SCALAR_FIELD[params.curve] == sf and dom.k == k
    assert advice.shape == (cs.num_advice, n, 4)
    dev = advice.device
    st = torch.cuda.current_stream(dev).cuda_stream
    blind = lambda: ipa._canon(sf, rng.next_scalar(sf))  # noqa: E731
    blinds_of = lambda count: [blind() for _ in range(count)]  # noqa: E731
    mont_rows = lambda values: multiopen._limbs_many(sf, values) if values else np.zeros((0, 4), dtype=np.uint64)  # noqa: E731
    lagrange, blinds = {}, {}  # key -> Lagrange column (n, 4) / the commitment's blind

    transcript.common_scalar(_mont(sf, vk.transcript_repr))
    inst = _instance_columns(cs, n, instances, dev)
    if cs.num_instance:
        for c in params.commit_lagrange_batch(inst, _ones(sf, cs.num_instance)):
            transcript.common_point(c)
    for i in range(cs.num_instance):
        lagrange[("instance", i)], blinds[("instance", i)] = inst[i], 1

    adv = advice.clone().contiguous()
    if cs.num_advice:
        rng.fill_rows(sf, adv, cs.num_advice, n, u, n - u, stream=st)
        b = blinds_of(cs.num_advice)
        for c in params.commit_lagrange_batch(adv, mont_rows(b)):
            transcript.write_point(c)
        for i in range(cs.num_advice):
            lagrange[("advice", i)], blinds[("advice", i)] = adv[i], b[i]
    for i in range(cs.num_fixed):
        lagrange[("fixed", i)], blinds[("fixed", i)] = pk.fixed_values[i], 1
    circuit_keys = list(lagrange)

    theta = transcript.squeeze_challenge_scalar()
    lookup_ev = None
    if n_lookups:
        inputs, tables = cs.compressed(theta)
        lookup_ev = expr.GateEvaluator(expr.compile_outputs(sf, inputs + tables), n_outputs=2 * n_lookups)
        compressed = lookup_ev.eval(lagrange, k, 1, stream=st)
        a_in, s_in = compressed[:n_lookups].contiguous(), compressed[n_lookups:].contiguous()
        try:
            a_perm, s_perm = permutation.lookup_permute_batch(sf, a_in, s_in, usable_rows=u)
        except api.TrhError:
            if strict_lookups:
                raise
            a_perm, s_perm = a_in.clone(), s_in.clone()
        permuted = torch.cat([a_perm, s_perm]).contiguous()
        rng.fill_rows(sf, permuted, 2 * n_lookups, n, u, n - u, stream=st)
        b = blinds_of(2 * n_lookups)
        commits = params.commit_lagrange_batch(permuted, mont_rows(b))
        for l in range(n_lookups):
            transcript.write_point(commits[l])
            transcript.write_point(commits[n_lookups + l])
            lagrange[("lk_a", l)], blinds[("lk_a", l)] = permuted[l], b[l]
            lagrange[("lk_s", l)], blinds[("lk_s", l)] = permuted[n_lookups + l], b[n_lookups + l]

    beta = transcript.squeeze_challenge_scalar()
    gamma = transcript.squeeze_challenge_scalar()
    if sets + n_lookups:
        num, den = [], []
        if n_perm:
            omega_powers = torch.empty((n, 4), dtype=torch.int64, device=dev)
            api.powers_dev(sf, omega_powers, n, _mont(sf, dom.omega), stream=st)
            values = [lagrange[key] for key in cs.permutation_columns]
            for s in range(0, n_perm, chunk):
                t_num, t_den = permutation.permutation_terms(sf, values[s:s + chunk], [pk.permutations[j] for j in range(s, min(s + chunk, n_perm))],
                                                             omega_powers, beta, gamma, first_column=s)
                num.append(t_num); den.append(t_den)
        for l in range(n_lookups):
            t_num, t_den = permutation.lookup_terms(sf, a_in[l], s_in[l], lagrange[("lk_a", l)], lagrange[("lk_s", l)], beta, gamma)
            num.append(t_num); den.append(t_den)
        z = permutation.grand_products_terms(sf, k, num, den)
        permutation.chain_products(sf, z, u, rows=sets)  # z_s[0] = z_(s-1)[u]; the lookups' columns behind the sets start from one
        rng.fill_rows(sf, z, sets + n_lookups, n, u + 1, bf, stream=st)
        b = blinds_of(sets + n_lookups)
        commits = params.commit_lagrange_batch(z, mont_rows(b))
        for i, c in enumerate(commits):
            transcript.write_point(c)
            key = ("perm_z", i) if i < sets else ("lk_z", i - sets)
            lagrange[key], blinds[key] = z[i], b[i]

    random_poly = torch.empty((n, 4), dtype=torch.int64, device=dev)
    rng.fill(sf, random_poly, n, stream=st)
    blinds["random"] = blind()
    transcript.write_point(params.commit(random_poly, _mont(sf, blinds["random"])))

    y = transcript.squeeze_challenge_scalar()
    # coefficient forms of everything made in this proof; the fixed and sigma columns have theirs in the key
    made = [key for key in lagrange if key[0] != "fixed"]
    coeff = dom.lagrange_to_coeff(torch.stack([lagrange[key] for key in made]).contiguous())
    polys = {key: coeff[i] for i, key in enumerate(made)}
    for i in range(cs.num_fixed):
        polys[("fixed", i)] = pk.fixed_polys[i]
    for j in range(n_perm):
        polys[("sigma", j)], blinds[("sigma", j)] = pk.sigma_polys[j], 1
    polys["random"] = random_poly

    # h(X): the gates' fold, continued by the permutation and lookup terms, over the extended domain
    n_blocks = dom.quotient_poly_degree if layout == "blocks" else None
    ext_keys = [key for key in polys if key != "random"]
    stack = torch.stack([polys[key] for key in ext_keys]).contiguous()
    ext_all = dom.coeff_to_extended_blocks(stack, n_blocks) if n_blocks else dom.coeff_to_extended(stack)
    ext = {key: ext_all[i] for i, key in enumerate(ext_keys)}
    circuit_ext = {key: ext[key] for key in circuit_keys}
    run = lambda ev: ev.eval_blocks(circuit_ext, k, n_blocks, stream=st) if n_blocks else ev.eval(circuit_ext, dom.extended_k, 1 << (dom.extended_k - k), stream=st)  # noqa: E731
    if cs.gates:
        acc = run(expr.GateEvaluator(expr.compile_gates(sf, cs.gates, y))).contiguous()
    else:
        acc = torch.zeros_like(ext_all[0])
    if n_perm or n_lookups:
        lookups_ext = []
        if n_lookups:
            compressed_ext = run(lookup_ev)
            lookups_ext = [[compressed_ext[l], compressed_ext[n_lookups + l], ext[("lk_a", l)], ext[("lk_s", l)], ext[("lk_z", l)]] for l in range(n_lookups)]
        l0, l_blind, l_last = pk.basis(n_blocks)
        terms = quotient.QuotientTerms(dom, n_perm, chunk, n_lookups, bf)
        terms.eval(acc, [ext[key] for key in cs.permutation_columns], [ext[("sigma", j)] for j in range(n_perm)], [ext[("perm_z", s)] for s in range(sets)],
                   lookups_ext, l0, l_blind, l_last, beta, gamma, y, n_blocks=n_blocks, stream=st)
        terms.destroy()
    d = dom.quotient_poly_degree
    if n_blocks:
        h = dom.blocks_to_quotient(acc.reshape(d, n, 4), divide_by_vanishing=True)
    else:
        flat = acc.reshape(1, dom.extended_len(), 4)
        h = dom.extended_to_coeff(dom.divide_by_vanishing_poly(flat))[0].contiguous()
    pieces = h.reshape(d, n, 4)
    piece_blinds = blinds_of(d)
    for c in params.commit_batch(pieces, mont_rows(piece_blinds)):
        transcript.write_point(c)

    x = transcript.squeeze_challenge_scalar()
    xn = pow(x, n, m)
    xn_powers = [pow(xn, i, m) for i in range(d)]
    polys["h"] = multiopen.lincomb(sf, pieces, xn_powers)  # sum_i x^(n i) h_i: one polynomial, opened at x
    blinds["h"] = sum(c * b for c, b in zip(xn_powers, piece_blinds)) % m
    keys = list(polys)
    every = torch.stack([polys[key] for key in keys]).contiguous()
    at = {}  # rotation -> the values of every polynomial at x omega^rotation
    for _, r in cs.eval_plan():
        if r not in at:
            values = api.poly_eval_batch_dev(sf, every, n, len(keys), _mont(sf, _rotated(x, dom.omega, dom.omega_inv, r, m)), stream=st)
            at[r] = {key: values[i] for i, key in enumerate(keys)}
    for key, r in cs.eval_plan():
        transcript.write_scalar(at[r][key])

    queries = [(_rotated(x, dom.omega, dom.omega_inv, r, m), key) for key, r in cs.query_plan()]
    s_poly = torch.empty((n, 4), dtype=torch.int64, device=dev)
    rng.fill(sf, s_poly, n, stream=st)
    multiopen.create_proof(params, blind, transcript, queries, polys, blinds, s_poly=s_poly)


# ---- the verifier --------------------------------------------------------------------------------------------------------------------------
def lagrange_evals(m: int, n: int, omega: int, x: int, rotations):
    """l_i(x) for the rows i (negative: counted from the end) of the 2^k-row domain: omega^i (x^n - 1) / (n (x - omega^i))"""
    xn = pow(x, n, m)
    n_inv = pow(n, -1, m)
    out = []
    for i in rotations:
        w = pow(omega, i % n, m)
        if (x - w) % m == 0:
            out.append(1)
            continue
        out.append(w * (xn - 1) % m * n_inv % m * pow((x - w) % m, -1, m) % m)
    return out


def verify_proof(params, vk: VerifyingKey, instances, transcript) -> ipa.Guard:
    """plonk::verify_proof for one circuit: reads the proof from `transcript` with the prover's absorbs and squeezes, tests the vanishing
    identity at x on the evaluations (VerifyError when it fails: no group work has been done by then) and returns the opening's guard"""
    cs, dom = vk.cs, vk.domain
    sf, k, n = cs.field, params.k, params.n
    m = _MODULUS[sf]
    assert api.SCALAR_FIELD[params.curve] == sf and dom.k == k
    bf, sets, chunk, n_lookups, n_perm = cs.blinding_factors(), cs.n_sets(), cs.chunk_len(), len(cs.lookups), len(cs.permutation_columns)
    d = dom.quotient_poly_degree
    try:
        inst = _instance_columns(cs, n, instances, _device())
    except ValueError as e:
        raise VerifyError(str(e)) from e
    commitments = {}
    transcript.common_scalar(_mont(sf, vk.transcript_repr))
    if cs.num_instance:
        for i, c in enumerate(params.commit_lagrange_batch(inst, _ones(sf, cs.num_instance))):
            transcript.common_point(c)
            commitments[("instance", i)] = [(1, c[:8].copy())]
    for i in range(cs.num_advice):
        commitments[("advice", i)] = [(1, transcript.read_point())]
    theta = transcript.squeeze_challenge_scalar()
    for l in range(n_lookups):
        commitments[("lk_a", l)] = [(1, transcript.read_point())]
        commitments[("lk_s", l)] = [(1, transcript.read_point())]
    beta = transcript.squeeze_challenge_scalar()
    gamma = transcript.squeeze_challenge_scalar()
    for s in range(sets):
        commitments[("perm_z", s)] = [(1, transcript.read_point())]
    for l in range(n_lookups):
        commitments[("lk_z", l)] = [(1, transcript.read_point())]
    commitments["random"] = [(1, transcript.read_point())]
    y = transcript.squeeze_challenge_scalar()
    pieces = [transcript.read_point() for _ in range(d)]
    x = transcript.squeeze_challenge_scalar()
    xn = pow(x, n, m)
    commitments["h"] = [(pow(xn, i, m), pt) for i, pt in enumerate(pieces)]
    for i in range(cs.num_fixed):
        commitments[("fixed", i)] = [(1, vk.fixed_commitments[i])]
    for j in range(n_perm):
        commitments[("sigma", j)] = [(1, vk.sigma_commitments[j])]
    evals = {}
    for key, r in cs.eval_plan():
        evals[(key, r)] = transcript.read_scalar()

    # the vanishing identity at x
    l_evals = lagrange_evals(m, n, dom.omega, x, range(-(bf + 1), 1))
    l_last, l_blind, l0 = l_evals[0], sum(l_evals[1:1 + bf]) % m, l_evals[1 + bf]
    active = (1 - l_last - l_blind) % m
    last = cs.last_rotation()
    query = lambda kind, column, rotation: evals[((kind, column), rotation)]  # noqa: E731
    terms = [evaluate(g, m, query) for g in cs.gates]
    if n_perm:
        z = lambda s, r: evals[(("perm_z", s), r)]  # noqa: E731
        delta = permutation.delta(sf)
        terms.append(l0 * (1 - z(0, 0)) % m)
        terms.append(l_last * (z(sets - 1, 0) * z(sets - 1, 0) - z(sets - 1, 0)) % m)
        for s in range(1, sets):
            terms.append(l0 * (z(s, 0) - z(s - 1, last)) % m)
        for s in range(sets):
            left, right = z(s, 1), z(s, 0)
            for j in range(s * chunk, min((s + 1) * chunk, n_perm)):
                v = evals[(cs.permutation_columns[j], 0)]
                left = left * (v + beta * evals[(("sigma", j), 0)] + gamma) % m
                right = right * (v + beta * pow(delta, j, m) % m * x + gamma) % m
            terms.append(active * (left - right) % m)
    inputs, tables = cs.compressed(theta)
    for l in range(n_lookups):
        a, s_ = evaluate(inputs[l], m, query), evaluate(tables[l], m, query)
        zl, zl_next = evals[(("lk_z", l), 0)], evals[(("lk_z", l), 1)]
        ap, ap_prev, sp = evals[(("lk_a", l), 0)], evals[(("lk_a", l), -1)], evals[(("lk_s", l), 0)]
        terms.append(l0 * (1 - zl) % m)
        terms.append(l_last * (zl * zl - zl) % m)
        terms.append(active * (zl_next * (ap + beta) % m * (sp + gamma) - zl * (a + beta) % m * (s_ + gamma)) % m)
        terms.append(l0 * (ap - sp) % m)
        terms.append(active * (ap - sp) % m * (ap - ap_prev) % m)
    folded = 0
    for t in terms:
        folded = (folded * y + t) % m
    if folded != evals[("h", 0)] * (xn - 1) % m:
        raise VerifyError("the vanishing identity does not hold at x")

    queries = [(_rotated(x, dom.omega, dom.omega_inv, r, m), key, evals[(key, r)]) for key, r in cs.query_plan()]
    return multiopen.verify_proof(params, transcript, queries, commitments)


def single_verify(params, guard: ipa.Guard) -> bool:
    """SingleVerifier: the guard's MSM with its challenges used evaluates to the identity"""
    msm = guard.use_challenges()
    ok, _ = msm.eval()
    msm.destroy()
    return ok


# ---- proofs as bytes -----------------------------------------------------------------------------------------------------------------------
def create_proof_bytes(params, pk: ProvingKey, instances, advice, rng: api.Rng, layout: str = "blocks", strict_lookups: bool = True) -> bytes:
    """create_proof into a Blake2bWrite, finalized: 32 bytes per item, points compressed, in the order create_proof writes them"""
    transcript = Blake2bWrite(params.curve)
    try:
        create_proof(params, pk, instances, advice, rng, transcript, layout=layout, strict_lookups=strict_lookups)
        return transcript.finalize()
    finally:
        transcript.destroy()


def verify_proof_bytes(params, vk: VerifyingKey, instances, proof: bytes) -> ipa.Guard:
    """verify_proof out of a Blake2bRead over `proof`.  VerifyError for bytes that are no point or no scalar where one is due, a proof that
    ends early, a proof with bytes left over, and whatever verify_proof refuses"""
    transcript = Blake2bRead(params.curve, proof)
    try:
        guard = verify_proof(params, vk, instances, transcript)
        if not transcript.finished():
            raise VerifyError(f"{transcript.remaining()} bytes of the proof are left over")
        return guard
    except TranscriptError as e:
        raise VerifyError(str(e)) from e
    finally:
        transcript.destroy()


def _random_weight(m: int) -> int:
    return 1 + secrets.randbelow(m - 1)  # upstream: Scalar::random(OsRng)


class BatchVerifier:
    """plonk::BatchVerifier for the proofs of one verifying key: add_proof(instances, proof), then finalize(params, vk) -> bool.  Every proof
    is read into its guard (a VerifyError makes the batch false) and the guards are folded by ipa.batch_verify, one random non-zero weight
    per proof.  weight_source(modulus) -> int replaces the default draw (the secrets module; upstream: OsRng), for tests."""

    def __init__(self, weight_source=None):
        self.items = []
        self.weight_source = weight_source or _random_weight

    def add_proof(self, instances, proof: bytes) -> None:
        self.items.append((instances, bytes(proof)))

    def finalize(self, params, vk: VerifyingKey) -> bool:
        m = _MODULUS[vk.cs.field]
        guards = []
        for instances, proof in self.items:
            try:
                guards.append(verify_proof_bytes(params, vk, instances, proof))
            except VerifyError:
                return False
        if not guards:
            return True
        weights = [self.weight_source(m) % m for _ in guards]
        if not all(weights):
            raise ValueError("a batch weight is zero")
        return ipa.batch_verify(params, guards, weights)


def verify_proofs(params, vk: VerifyingKey, instances_list, proofs, weight_source=None) -> None:
    """the verifying half of gen_proofs_and_verify: the batch first; when it fails, every proof alone (verify_proof_bytes + single_verify),
    and VerifyError names the first that fails in its text and in its `index`"""
    batch = BatchVerifier(weight_source)
    for instances, proof in zip(instances_list, proofs):
        batch.add_proof(instances, proof)
    if batch.finalize(params, vk):
        return
    for i, (instances, proof) in enumerate(zip(instances_list, proofs)):
        try:
            if single_verify(params, verify_proof_bytes(params, vk, instances, proof)):
                continue
            reason = "its opening does not hold"
        except VerifyError as e:
            reason = str(e)
        err = VerifyError(f"proof {i} of {len(proofs)} does not verify: {reason}")
        err.index = i
        raise err
    err = VerifyError("the batch does not verify although every proof does alone")
    err.index = None
    raise err


def gen_proofs_and_verify(params, vk: VerifyingKey, pk: ProvingKey, inputs, rng: api.Rng):
    """the reference's harness (src/test_utils.rs:21-68): a proof for every (instances, advice) of `inputs`, all from the one rng stream, then
    verify_proofs over them.  -> the proofs; VerifyError as verify_proofs raises it"""
    inputs = list(inputs)
    proofs = [create_proof_bytes(params, pk, instances, advice, rng) for instances, advice in inputs]
    verify_proofs(params, vk, [instances for instances, _ in inputs], proofs)
    return proofs
