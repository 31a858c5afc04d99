"""Whole proofs as bytes (tiny_ram_halo2_amd.plonk create_proof_bytes / verify_proof_bytes / BatchVerifier / gen_proofs_and_verify over
tiny_ram_halo2_amd.transcript and the trh_tr_* entries): the reference's gen_proofs_and_verify harness.  The independent side is
tests/plonk_model.py's verifier reading the same bytes through tests/transcript_model.py (hashlib, Python integers).

Circuits A (Pallas) and B (Vesta) of tests/plonk_circuits.py at k = 5 -- 32 rows, three permutation sets, lookups, rotations +-1: every kind of
item a proof holds -- and circuit A once at k = 14, past msm_small_kernel and with the opening's generator collapse, where
trh_ipa_create_proof calls the library's own transcript functions from its collapsed rounds.

  honest      32 bytes per item; verify_proof_bytes + single_verify accept; the model accepts the bytes and squeezes the same challenges;
              both layouts of the extended domain give the same bytes
  callbacks   the same seed through Blake2bWrite (the library's functions inside trh_ipa_create_proof) and through transcript_model's
              writer (Python closures, the path of every other transcript object): identical bytes
  refusals    one bit flipped in each item in turn, the proof cut by 1 and by 32 bytes, one byte appended, a wrong public input:
              VerifyError or a false single_verify, never another exception
  batch       three honest proofs of different witnesses: true with injected and with default weights; one tampered in its last scalar:
              false, and verify_proofs names it; an empty batch is true; gen_proofs_and_verify end to end
  k = 14      an honest proof is accepted; L of the first round after the collapse negated: refused"""
import functools

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import plonk_circuits as pc
import transcript_model as tm
from test_gpu_plonk import CASES, Setup, to_dev
from tiny_ram_halo2_amd import api, multiopen, plonk, transcript

K = pc.K


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


@functools.lru_cache(maxsize=None)
def setup(name):
    return Setup(name)


def rng_of(seed):
    return api.Rng(bytes([seed]) * 32)


@functools.lru_cache(maxsize=None)
def honest(name, seed=7, layout="blocks"):
    s = setup(name)
    return plonk.create_proof_bytes(s.params, s.pk, s.instances, s.honest_advice(), rng_of(seed), layout=layout)


def n_items(cs, k):
    """the items of a proof, counted from the constraint system alone: the commitments, the evaluations, multiopen's q' and one evaluation per
    point set, the opening's S, L and R per round, c and f"""
    commitments = cs.num_advice + 2 * len(cs.lookups) + cs.n_sets() + len(cs.lookups) + 1 + (cs.degree() - 1)
    _, point_sets = multiopen.construct_intermediate_sets([(r, key) for key, r in cs.query_plan()])
    return commitments + len(cs.eval_plan()) + 1 + len(point_sets) + 1 + 2 * k + 2


def accepts(s, proof, instances=None):
    """the package's verifier: VerifyError and a false single_verify are its two ways to say no; anything else is a failure of the test"""
    try:
        guard = plonk.verify_proof_bytes(s.params, s.vk, s.instances if instances is None else instances, proof)
    except plonk.VerifyError:
        return False
    return plonk.single_verify(s.params, guard)


def model_verify(s, proof, instances=None):
    return tm.verify(s.curve, s.k, s.g, s.g_lagrange, s.w, s.u, s.model, s.pts(s.vk.fixed_commitments), s.pts(s.vk.sigma_commitments),
                     s.vk.transcript_repr, s.instances if instances is None else instances, proof, group=s.group)


def flipped(proof, item, bit):
    at = 32 * item + bit // 8
    return proof[:at] + bytes([proof[at] ^ 1 << bit % 8]) + proof[at + 1:]


def last_scalar_plus_one(s, proof):
    v = (int.from_bytes(proof[-32:], "little") + 1) % s.cv.scalar.m
    return proof[:-32] + v.to_bytes(32, "little")


@pytest.mark.parametrize("name", list(CASES))
def test_an_honest_proof_as_bytes(name):
    s = setup(name)
    proof = honest(name)
    assert isinstance(proof, bytes) and len(proof) == 32 * n_items(s.cs, K)
    assert honest(name, layout="flat") == proof
    assert accepts(s, proof)
    reader = transcript.Blake2bRead(s.curve, proof)
    guard = plonk.verify_proof(s.params, s.vk, s.instances, reader)
    assert reader.finished() and plonk.single_verify(s.params, guard)
    ok, model_squeezes, refused = model_verify(s, proof)
    assert ok and refused is None
    assert reader.squeezes == model_squeezes and len(set(model_squeezes)) == len(model_squeezes) >= 11 + K
    assert plonk.create_proof_bytes(s.params, s.pk, s.instances, s.honest_advice(), rng_of(9)) != proof


@pytest.mark.parametrize("name", list(CASES))
def test_native_callbacks_write_what_the_closures_write(name):
    s = setup(name)
    writer = tm.Writer(s.curve)  # no transcript.Blake2bWrite: ipa.create_proof_native calls it through three Python closures
    plonk.create_proof(s.params, s.pk, s.instances, s.honest_advice(), rng_of(7), writer)
    assert writer.finalize() == honest(name)


def test_refusals_are_verify_errors():
    s = setup("A")
    proof = honest("A")
    items = len(proof) // 32
    assert accepts(s, proof)
    taken = [i for i in range(items) if accepts(s, flipped(proof, i, (11 * i + 3) % 256))]
    assert taken == [], f"items {taken} of {items} can have a bit flipped without the verifier noticing"
    taken = [i for i in (0, items - 2 * K - 3, items - 2 * K - 2, items - 4) if accepts(s, flipped(proof, i, 255))]  # a point negated: still a point
    assert taken == []
    assert not accepts(s, proof[:-1]) and not accepts(s, proof[:-32]) and not accepts(s, proof + b"\x00") and not accepts(s, b"")
    with pytest.raises(plonk.VerifyError, match="left over"):
        plonk.verify_proof_bytes(s.params, s.vk, s.instances, proof + b"\x00")
    with pytest.raises(plonk.VerifyError, match="fewer than 32 bytes"):
        plonk.verify_proof_bytes(s.params, s.vk, s.instances, proof[:-1])
    wrong = [list(s.instances[0])]
    wrong[0][2] = (wrong[0][2] + 1) % s.cv.scalar.m
    assert not accepts(s, proof, wrong) and not accepts(s, proof, [list(s.instances[0]) + [0] * K * K])
    # the model reads the same refusals out of the bytes
    assert not model_verify(s, proof, wrong)[0]
    assert model_verify(s, proof + bytes(32))[2] == "transcript"
    with pytest.raises(tm.TranscriptError):
        model_verify(s, proof[:-1])


@functools.lru_cache(maxsize=None)
def three_proofs():
    """circuit A's witness and two more that differ from it in cells no gate, lookup or copy reads: one verifying key, three proofs"""
    s = setup("A")
    proofs = [honest("A")]
    for j in (1, 2):
        adv = [list(c) for c in s.advice]
        for column in (3, 6):
            row = s.witness.free_cell(column)
            adv[column][row] = (adv[column][row] + j) % s.cv.scalar.m
        proofs.append(plonk.create_proof_bytes(s.params, s.pk, s.instances, to_dev(s.field, adv), rng_of(20 + j)))
    return proofs


def test_batch_verifier():
    s = setup("A")
    proofs = three_proofs()
    assert len(set(proofs)) == 3 and all(accepts(s, p) for p in proofs)
    drawn = []

    def source(m):
        drawn.append(m)
        return 0x9E3779B97F4A7C15 ** (4 + len(drawn)) % m

    for batch in (plonk.BatchVerifier(source), plonk.BatchVerifier()):
        for p in proofs:
            batch.add_proof(s.instances, p)
        assert batch.finalize(s.params, s.vk)
    assert drawn == [s.cv.scalar.m] * 3
    assert plonk.BatchVerifier().finalize(s.params, s.vk), "an empty batch"
    # f of one opening changed: the vanishing identity of that proof still holds, its guard does not
    spoiled = [proofs[0], last_scalar_plus_one(s, proofs[1]), proofs[2]]
    for batch in (plonk.BatchVerifier(source), plonk.BatchVerifier()):
        for p in spoiled:
            batch.add_proof(s.instances, p)
        assert not batch.finalize(s.params, s.vk)
    with pytest.raises(plonk.VerifyError, match="proof 1 of 3") as e:
        plonk.verify_proofs(s.params, s.vk, [s.instances] * 3, spoiled)
    assert e.value.index == 1
    plonk.verify_proofs(s.params, s.vk, [s.instances] * 3, proofs)
    # a proof that is no proof makes the batch false as well, and is named
    cut = [proofs[0], proofs[1], proofs[2][:-32]]
    batch = plonk.BatchVerifier()
    for p in cut:
        batch.add_proof(s.instances, p)
    assert not batch.finalize(s.params, s.vk)
    with pytest.raises(plonk.VerifyError, match="proof 2 of 3") as e:
        plonk.verify_proofs(s.params, s.vk, [s.instances] * 3, cut)
    assert e.value.index == 2
    with pytest.raises(ValueError):
        b = plonk.BatchVerifier(lambda m: m)
        b.add_proof(s.instances, proofs[0])
        b.finalize(s.params, s.vk)


def test_gen_proofs_and_verify():
    s = setup("A")
    inputs = [(s.instances, s.honest_advice()), (s.instances, s.honest_advice())]
    proofs = plonk.gen_proofs_and_verify(s.params, s.vk, s.pk, inputs, rng_of(7))
    assert proofs[0] == honest("A") and proofs[1] != proofs[0], "one rng stream for all proofs"
    assert all(accepts(s, p) for p in proofs)
    # the reference's _should_fail twin: the same proofs against another public input
    wrong = [list(s.instances[0])]
    wrong[0][0] = (wrong[0][0] + 1) % s.cv.scalar.m
    with pytest.raises(plonk.VerifyError, match="proof 1 of 2"):
        plonk.verify_proofs(s.params, s.vk, [s.instances, wrong], proofs)


def test_k14_through_the_generator_collapse():
    from test_gpu_plonk_sizes import setup as setup_at
    k = 14
    s = setup_at("A", k)
    before = api.stat("ipa_generator_collapses")
    proof = plonk.create_proof_bytes(s.params, s.pk, s.instances, s.honest_advice(), rng_of(7))
    assert api.stat("ipa_generator_collapses") == before + 1
    items = n_items(s.cs, k)
    assert len(proof) == 32 * items
    assert accepts(s, proof)
    first_l_after_collapse = items - 2 - 2 * k + 2 * (k - 12)
    assert not accepts(s, flipped(proof, first_l_after_collapse, 255)), "-L in place of L"
    assert not accepts(s, flipped(proof, first_l_after_collapse, 0))
