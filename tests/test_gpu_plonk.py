"""keygen -> create_proof -> verify_proof end to end on the device (tiny_ram_halo2_amd.plonk), the reference's gen_proofs_and_verify and its
_should_fail twin, judged by two verifiers: the package's own (plonk.verify_proof + single_verify, group work on the device) and
tests/plonk_model.py (Python integers over the oracle, written without the package's plonk / multiopen modules).

Circuits (tests/plonk_circuits.py):  A on Pallas -- three permutation sets, copies across advice and instance cells, gates with
Rotation(+1) at the last usable row and Rotation(-1), a one-column and a two-column lookup;  B on Vesta -- the logic chip.

Every test of this file runs at k = 5 (32 rows, 26 usable): one workgroup per launch, one block per scan, msm_small_kernel for every MSM, an
opening without the generator collapse.  That is the size for what does not depend on n -- the exhaustive tamper sweep, the smallest shapes,
the integer model's own group arithmetic.  tests/test_gpu_plonk_sizes.py takes the same circuits, through the Setup of this file, to
k = 10, 13 and 14, where the kernels of the chain leave their first level.

  honest          both verifiers accept and squeeze the same challenges; ipa.batch_verify over two proofs accepts
  should_fail     an instance value changed at verification only: both refuse
  broken witness  one gate cell, one copy, one lookup input, one at a time: the prover returns, the verifier refuses
  tamper          every recorded item of A's proof, one at a time (scalar + 1, point doubled): the device verifier refuses each; the model
                  one commitment, one evaluation, one scalar of the opening
  layouts         h(X) over the flat extended domain and over coset blocks: the same proof
  rng             the same seed gives the same proof, another seed another one
  smallest        gates alone and copies alone (degree 3: two pieces of h(X), sets of one column): the branches the two circuits do not take"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import pasta as o
import plonk_circuits as pc
import plonk_model as pm
from tiny_ram_halo2_amd import api, ipa, plonk, poly

K = pc.K
CASES = {"A": "pallas", "B": "vesta"}
SMALL = {"G": "pallas", "P": "vesta"}  # gates alone, copies alone


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


def to_dev(field, columns):
    f = o.FIELDS[field]
    return torch.from_numpy(np.array([[f.limbs(v % f.m) for v in col] for col in columns], dtype=np.uint64).view(np.int64)).cuda()


class Setup:
    """one circuit at 2^k rows with its keys, a satisfying witness, and the parameters as the model wants them: affine tuples for its Python
    group (the default, for k = 5), the downloaded limb rows for group="cpp".  `params`: Params.new(curve, k) made elsewhere, to share them"""

    def __init__(self, name, k=K, group="python", params=None):
        self.name, self.curve, self.k, self.group = name, {**CASES, **SMALL}[name], k, group
        self.cv = o.CURVES[self.curve]
        self.field = api.SCALAR_FIELD[self.curve]
        self.params = params if params is not None else poly.Params.new(self.curve, k)
        assert (self.params.curve, self.params.k) == (self.curve, k)
        n = 1 << k
        if name == "A":
            self.circuit = pc.circuit_a(self.field)
            self.witness = pc.WitnessA(self.field, k)
            self.advice, self.fixed, self.copies, self.instances = self.witness.advice, self.witness.fixed, self.witness.copies, [self.witness.instance]
        elif name == "G":
            self.circuit = pc.circuit_gates_only(self.field)
            self.advice, self.fixed = pc.witness_gates_only(self.field, k)
            self.copies, self.instances = [], []
        elif name == "P":
            self.circuit = pc.circuit_copies_only(self.field)
            self.advice, self.copies = pc.witness_copies_only(self.field, k)
            self.fixed, self.instances = [], []
        else:
            self.circuit = pc.circuit_b(self.field)
            self.advice, self.fixed = pc.witness_b(self.field, k, used=20 if k == K else None)
            self.copies, self.instances = [], []
            self.names = pc.ADV_B
        self.cs = self.circuit.system()
        self.vk, self.pk = plonk.keygen(self.params, self.cs, to_dev(self.field, self.fixed) if self.fixed else None, self.copies)
        g, gl = self.params._g.download(), self.params._g_lagrange.download()
        # the model's points: rows of limbs as they are for the C++ group, affine tuples for the Python one
        self.pts = (lambda rows: np.asarray(rows, dtype=np.uint64).reshape(-1, 8)) if group == "cpp" else (lambda rows: [self.cv.affine_from_limbs(r) for r in rows])
        self.g, self.g_lagrange, self.w = self.pts(g[:n]), self.pts(gl[:n]), self.pts(g[n:n + 1])[0]
        self.u = self.pts(np.asarray(self.params.u, dtype=np.uint64).reshape(1, 8))[0]
        self.model = self.circuit.model()
        self._honest_advice = None

    def honest_advice(self):
        """the satisfying witness on the device, sent there once; create_proof works on a copy"""
        if self._honest_advice is None:
            self._honest_advice = to_dev(self.field, self.advice)
        return self._honest_advice

    def prove(self, advice=None, seed=7, layout="blocks", strict_lookups=True):
        """advice: lists of integers or a device tensor; None: the honest witness"""
        tr = pm.Writer(self.curve)
        advice = self.honest_advice() if advice is None else advice if torch.is_tensor(advice) else to_dev(self.field, advice)
        plonk.create_proof(self.params, self.pk, self.instances, advice, api.Rng(bytes([seed]) * 32), tr,
                           layout=layout, strict_lookups=strict_lookups)
        return tr.items, tr.squeezes

    def guard(self, items, instances=None):
        """-> (guard or None when the identity already fails, the reader)"""
        tr = pm.Reader(self.curve, items)
        try:
            return plonk.verify_proof(self.params, self.vk, self.instances if instances is None else instances, tr), tr
        except plonk.VerifyError:
            return None, tr

    def device_accepts(self, items, instances=None):
        g, tr = self.guard(items, instances)
        return g is not None and tr.finished() and plonk.single_verify(self.params, g)

    def model_verify(self, items, instances=None):
        """-> (accepted, squeezes, the refusing check or None)"""
        return pm.verify(self.curve, self.k, self.g, self.g_lagrange, self.w, self.u, self.model, self.pts(self.vk.fixed_commitments),
                         self.pts(self.vk.sigma_commitments), self.vk.transcript_repr, self.instances if instances is None else instances, items,
                         group=self.group)


@functools.lru_cache(maxsize=None)
def setup(name):
    return Setup(name)


@functools.lru_cache(maxsize=None)
def honest(name, seed=7, layout="blocks"):
    return setup(name).prove(seed=seed, layout=layout)


@pytest.mark.parametrize("name", list(CASES))
def test_an_honest_proof_is_accepted_by_both_verifiers(name):
    s = setup(name)
    assert s.cs.degree() == 6 and s.cs.blinding_factors() == pc.BLINDING and s.cs.n_sets() == (3 if name == "A" else 0)
    items, prover_squeezes = honest(name)
    g, tr = s.guard(items)
    assert g is not None and tr.finished()
    assert plonk.single_verify(s.params, g)
    ok, model_squeezes, refused = s.model_verify(items)
    assert ok and refused is None
    assert tr.squeezes == model_squeezes == prover_squeezes and len(set(model_squeezes)) == len(model_squeezes) >= 11 + K


@pytest.mark.parametrize("name", list(CASES))
def test_batch_verify_over_two_proofs(name):
    s = setup(name)
    first, second = honest(name)[0], honest(name, seed=8)[0]
    assert first != second
    guards = [s.guard(items)[0] for items in (first, second)]
    weights = [0x1234567 ** 7 % s.cv.scalar.m, 1]
    assert ipa.batch_verify(s.params, guards, weights)
    kind, last = second[-1]
    assert kind == "S"
    spoiled, _ = s.guard(second[:-1] + [("S", (last + 1) % s.cv.scalar.m)])  # f of the opening: the identity at x still holds
    assert spoiled is not None and not ipa.batch_verify(s.params, [guards[0], spoiled], weights)


def test_a_wrong_public_input_is_refused():
    """the reference's gen_proofs_and_verify_should_fail: the proof is honest, one instance value differs at verification"""
    s = setup("A")
    items, _ = honest("A")
    wrong = [list(s.instances[0])]
    wrong[0][2] = (wrong[0][2] + 1) % s.cv.scalar.m
    assert not s.device_accepts(items, wrong)
    assert not s.model_verify(items, wrong)[0]
    too_long = [list(s.instances[0]) + [0]]
    assert not s.device_accepts(items, too_long) and not s.model_verify(items, too_long)[0]


def _broken(s, what):
    adv = [list(c) for c in s.advice]
    m = s.cv.scalar.m
    if s.name == "A":
        column, row = {"gate": (8, 5), "copy": s.witness.copied_cell(), "lookup": (5, s.witness.free_cell(5))}[what]
        adv[column][row] = (adv[column][row] + 1) % m
    else:
        cols = dict(zip(s.names, adv))
        if what == "gate":
            row = next(r for r in range(20) if cols["s_xor"][r])
            cols["res"][row] += 1
        else:
            row = next(r for r in range(20) if cols["s_and"][r])
            cols["a_e"][row] |= 2  # no even-bits value any more
    return adv


@pytest.mark.parametrize("name,what", [("A", "gate"), ("A", "copy"), ("A", "lookup"), ("B", "gate"), ("B", "lookup")])
def test_a_broken_witness_gives_a_proof_the_verifier_refuses(name, what):
    s = setup(name)
    adv = _broken(s, what)
    if what == "lookup":
        with pytest.raises(api.TrhError):  # upstream's Error::ConstraintSystemFailure
            s.prove(advice=adv)
    items, _ = s.prove(advice=adv, strict_lookups=False)
    assert len(items) == len(honest(name)[0])
    assert not s.device_accepts(items)
    if (name, what) in (("A", "copy"), ("B", "lookup")):
        assert not s.model_verify(items)[0]


def _tampered(s, items, i):
    kind, value = items[i]
    if kind == "S":
        return items[:i] + [("S", (value + 1) % s.cv.scalar.m)] + items[i + 1:]
    assert value is not None, "a commitment of the proof is the identity"
    return items[:i] + [("P", s.cv.double(value))] + items[i + 1:]


def test_every_tampered_item_is_refused():
    s = setup("A")
    items, _ = honest("A")
    assert s.device_accepts(items)
    accepted = [i for i in range(len(items)) if s.device_accepts(_tampered(s, items, i))]
    assert accepted == [], f"items {accepted} of {len(items)} can be changed without the verifier noticing"
    # the model: one commitment, one evaluation, one scalar of the opening
    first_eval = next(i for i, (kind, _) in enumerate(items) if kind == "S")
    for i in (0, first_eval, len(items) - 1):
        assert not s.model_verify(_tampered(s, items, i))[0], i


@pytest.mark.parametrize("name", list(CASES))
def test_both_layouts_of_the_extended_domain_give_the_same_proof(name):
    assert honest(name, layout="flat") == honest(name)


def test_the_proof_is_a_function_of_the_seed():
    s = setup("A")
    assert s.prove(seed=7) == honest("A")
    assert s.prove(seed=9)[0] != honest("A")[0]


@pytest.mark.parametrize("name", list(SMALL))
def test_the_smallest_shapes(name):
    """gates alone: degree 3, h(X) of two pieces, no product column, no lookup; copies alone: no gate and no fixed column, two sets of one column"""
    s = setup(name)
    assert s.cs.degree() == 3 and s.vk.domain.quotient_poly_degree == 2 and s.cs.n_sets() == (0 if name == "G" else 2)
    items, _ = s.prove()
    assert s.prove(layout="flat")[0] == items
    assert s.device_accepts(items) and s.model_verify(items)[0]
    assert not s.device_accepts(_tampered(s, items, 0))
    adv = [list(c) for c in s.advice]
    adv[-1][3] = (adv[-1][3] + 1) % s.cv.scalar.m  # the gate's product cell / one end of a copy
    spoiled, _ = s.prove(advice=adv)
    assert not s.device_accepts(spoiled) and not s.model_verify(spoiled)[0]
