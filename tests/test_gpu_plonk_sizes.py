"""keygen -> create_proof -> verify_proof of tests/test_gpu_plonk.py at the sizes where the kernels of the chain leave their first level.  At
k = 5 every launch is one workgroup, every scan one block, every MSM msm_small_kernel and the opening has no generator collapse, so a wrong
row offset or stride in the glue between the twenty device entries -- where the blinding rows land, the link row of chain_products, the
rotation step on the extended domain, the order the columns are stacked in, the blinds of the pieces of h(X) -- cannot show there.

  k = 10   the smallest size at which every launch of the chain has several workgroups; the extended domain (2^13) takes more than one NTT pass
  k = 13   copies alone: 8192 rows are exactly two scan blocks (SCAN_BLOCK = 4096) and n + 2 = 8194 pairs the largest opening that still
           goes through msm_small_kernel (SMALL_MAX_N = 8448)
  k = 14   the smallest size at which n + 2 exceeds SMALL_MAX_N: the commitments run the bucket pipeline over the fixed-base tables, the
           opening is the table plan with the generator collapse after k - 12 = 2 rounds, the scans have four blocks, the extended domain
           is 2^17

Circuits and witnesses: tests/plonk_circuits.py (A on Pallas, B on Vesta, P -- copies alone, degree 3 -- on Vesta).  The oracle is the
verification at random challenges by tests/plonk_model.py, its group work on the C++ oracle (group="cpp"), beside the package's own verifier:
one wrong word anywhere in the chain breaks the vanishing identity at x or the opening, and the model says which.

  honest          both verifiers accept, the reader is exhausted, prover / device verifier / model squeeze the same distinct challenges
  route           trh_stat: one generator collapse per k = 14 proof and none below; msm_small_kernel at work at k = 10 and 13;
                  ipa.batch_verify over two k = 14 proofs
  layouts         h(X) over the flat extended domain and over coset blocks, two device paths: the same proof
  seed            the proof is a function of the seed
  public input    the last instance value changed at verification: both refuse
  broken witness  one cell among the last 256 usable rows, one at a time: the Rotation(+1) gate's cell on the last usable row, one end of the
                  four-cell copy cycle, one lookup input; the logic chip's res and a_e
  tamper          k = 14: the first commitment, the first evaluation, L of the first round after the collapse, R of the last round, f
The exhaustive tamper sweep stays at k = 5: what is refused does not depend on n."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import plonk_circuits as pc
from test_gpu_plonk import Setup, _tampered
from tiny_ram_halo2_amd import api, ipa, plonk, poly

SIZES = [("A", 10), ("A", 14), ("B", 10), ("B", 14), ("P", 13)]
CURVE = {"A": "pallas", "B": "vesta", "P": "vesta"}
TAIL = 256  # the broken cells lie among the last TAIL usable rows


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


@functools.lru_cache(maxsize=None)
def params(curve, k):
    return poly.Params.new(curve, k)


@functools.lru_cache(maxsize=None)
def setup(name, k):
    return Setup(name, k, group="cpp", params=params(CURVE[name], k))


@functools.lru_cache(maxsize=None)
def honest(name, k, seed=7, layout="blocks"):
    return setup(name, k).prove(seed=seed, layout=layout)


def first_difference(a, b):
    """the first index at which two item lists differ (the shorter one's length when one is a prefix of the other), None when they are equal"""
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))


def verdicts(s, items, instances=None):
    """-> (the device verifier accepts, the model accepts, a sentence for the failure message, the two verifiers' squeezed challenges)"""
    guard, tr = s.guard(items, instances)
    device = "the vanishing identity fails" if guard is None else "the reader is not exhausted" if not tr.finished() else None
    if device is None and not plonk.single_verify(s.params, guard):
        device = "the opening fails"
    ok, model_squeezes, refused = s.model_verify(items, instances)
    said = f"circuit {s.name}, k = {s.k}: device verifier: {device or 'accepts'}; model: {'refuses at: ' + refused if refused else 'accepts'}"
    return device is None, ok, said, (tr.squeezes, model_squeezes)


@pytest.mark.parametrize("name,k", SIZES)
def test_an_honest_proof_is_accepted_by_both_verifiers(name, k):
    s = setup(name, k)
    assert s.cs.blinding_factors() == pc.BLINDING and s.cs.usable_rows(1 << k) == pc.usable(k)
    assert (s.cs.degree(), s.cs.n_sets()) == {"A": (6, 3), "B": (6, 0), "P": (3, 2)}[name]
    items, prover_squeezes = honest(name, k)
    device, model, said, (device_squeezes, model_squeezes) = verdicts(s, items)  # the device's verdict includes an exhausted reader
    assert device and model, said
    parted = first_difference(device_squeezes, prover_squeezes), first_difference(model_squeezes, prover_squeezes)
    assert device_squeezes == model_squeezes == prover_squeezes, f"circuit {name}, k = {k}: device verifier and model leave the prover's challenges at squeeze {parted}"
    assert len(set(model_squeezes)) == len(model_squeezes) == 11 + k


@pytest.mark.parametrize("name,k", SIZES)
def test_the_msms_of_a_proof_take_the_route_of_their_size(name, k):
    """one more proof from the honest seed, the counters read around it: the collapse exactly once from k = 14 on (the opening's table plan,
    hostplan::ipa_plan), msm_small_kernel for the openings of up to 2^13 + 2 pairs; and the proof is the first one again"""
    s = setup(name, k)
    first = honest(name, k)
    collapses, small = api.stat("ipa_generator_collapses"), api.stat("msm_small_launches")
    again = s.prove(seed=7)
    collapses, small = api.stat("ipa_generator_collapses") - collapses, api.stat("msm_small_launches") - small
    assert again == first, f"circuit {name}, k = {k}: the same seed gives another proof from item {first_difference(again[0], first[0])} on"
    if api.get_option("ipa_fold") == 1:
        assert collapses == (1 if k >= 14 else 0), f"circuit {name}, k = {k}"
    if k <= 13:
        assert small > 0, f"circuit {name}, k = {k}"


@pytest.mark.parametrize("name", ["A", "B"])
def test_batch_verify_over_two_proofs_with_the_collapse(name):
    s = setup(name, 14)
    first, second = honest(name, 14)[0], honest(name, 14, seed=8)[0]
    assert first != second
    guards = [s.guard(items)[0] for items in (first, second)]
    assert None not in guards, f"circuit {name}, k = 14: {verdicts(s, second)[2]}"
    weights = [0x1234567 ** 7 % s.cv.scalar.m, 1]
    assert ipa.batch_verify(s.params, guards, weights), f"circuit {name}, k = 14"
    kind, last = second[-1]
    assert kind == "S"
    spoiled, _ = s.guard(second[:-1] + [("S", (last + 1) % s.cv.scalar.m)])  # f of the opening: the identity at x still holds
    assert spoiled is not None and not ipa.batch_verify(s.params, [guards[0], spoiled], weights), f"circuit {name}, k = 14"


@pytest.mark.parametrize("name,k", [("A", 10), ("B", 10), ("A", 14)])
def test_both_layouts_of_the_extended_domain_give_the_same_proof(name, k):
    flat, blocks = honest(name, k, layout="flat")[0], honest(name, k)[0]
    at = first_difference(flat, blocks)
    assert at is None, f"circuit {name}, k = {k}: flat and blocks part at item {at} of {len(blocks)}; blocks: {verdicts(setup(name, k), blocks)[2]}; flat: {verdicts(setup(name, k), flat)[2]}"


def test_the_proof_is_a_function_of_the_seed():
    s = setup("A", 14)
    assert s.prove(seed=7) == honest("A", 14)
    other = s.prove(seed=9)[0]
    assert first_difference(other, honest("A", 14)[0]) == 0 and len(other) == len(honest("A", 14)[0])


@pytest.mark.parametrize("k", [10, 14])
def test_a_wrong_public_input_is_refused(k):
    """the proof is honest; the instance value on the last usable row differs at verification"""
    s = setup("A", k)
    items, u = honest("A", k)[0], pc.usable(k)
    assert len(s.instances[0]) == u
    wrong = [list(s.instances[0])]
    wrong[0][u - 1] = (wrong[0][u - 1] + 1) % s.cv.scalar.m
    device, model, said, _ = verdicts(s, items, wrong)
    assert not device and not model, said
    assert s.model_verify(items, wrong)[2] in ("opening", "vanishing identity"), said


def _broken(s, what):
    """-> the honest advice on the device with one cell changed, the cell"""
    u, m = pc.usable(s.k), s.cv.scalar.m
    if s.name == "A":
        w = s.witness
        column, row = {"gate": (2, u - 1), "cycle": w.cycle[-1], "lookup": (5, w.free_cell(5, tail=TAIL))}[what]
        assert (column, row) == (7, u - 1) if what == "cycle" else (column, row) not in w._tied()
        value = (s.advice[column][row] + 1) % m
    elif s.name == "P":
        column, row = 1, u - 1  # one end of a copy
        value = (s.advice[column][row] + 1) % m
    else:
        cols = dict(zip(s.names, s.advice))
        op, name = {"gate": ("s_xor", "res"), "lookup": ("s_and", "a_e")}[what]
        column, row = s.names.index(name), max(r for r in range(u) if s.fixed[0][r] and cols[op][r])  # the last enabled row
        value = s.advice[column][row] + 1 if what == "gate" else s.advice[column][row] | 2   # a_e | 2: no even-bits value any more
        assert value != s.advice[column][row]
    assert u - TAIL <= row < u
    adv = s.honest_advice().clone()
    adv[column, row] = torch.from_numpy(np.array(s.cv.scalar.limbs(value), dtype=np.uint64).view(np.int64)).to(adv.device)
    return adv, (column, row)


BROKEN = [("A", 10, "gate"), ("A", 10, "cycle"), ("A", 10, "lookup"), ("A", 14, "gate"), ("A", 14, "cycle"), ("A", 14, "lookup"),
          ("B", 10, "gate"), ("B", 10, "lookup"), ("B", 14, "gate"), ("B", 14, "lookup"), ("P", 13, "copy")]


@pytest.mark.parametrize("name,k,what", BROKEN)
def test_a_broken_witness_gives_a_proof_the_verifier_refuses(name, k, what):
    s = setup(name, k)
    adv, cell = _broken(s, what)
    if what == "lookup":
        with pytest.raises(api.TrhError):  # upstream's Error::ConstraintSystemFailure
            s.prove(advice=adv)
    items, _ = s.prove(advice=adv, strict_lookups=False)
    assert len(items) == len(honest(name, k)[0])
    device, model, said, _ = verdicts(s, items)
    assert not device, f"cell {cell}: {said}"
    if what in ("cycle", "copy") or (name, what) == ("B", "lookup"):
        assert not model, f"cell {cell}: {said}"


def test_tampered_items_around_the_collapse_are_refused():
    s, k = setup("A", 14), 14
    items, _ = honest("A", 14)
    kinds = [kind for kind, _ in items]
    # the tail of a proof: ... the evaluations of the multiopen's sets (S), the opening's S commitment (P), L and R of k rounds, c, f
    assert kinds[-2 * k - 4:] == ["S", "P"] + ["P", "P"] * k + ["S", "S"]
    rounds = len(items) - 2 - 2 * k
    first_eval = kinds.index("S")
    assert kinds[:first_eval] == ["P"] * first_eval and first_eval > s.cs.num_advice
    where = {"the first advice commitment": 0, "the first evaluation": first_eval, "L of round 2": rounds + 2 * (k - 12), "R of the last round": rounds + 2 * k - 1,
             "f": len(items) - 1}
    assert verdicts(s, items)[:2] == (True, True)
    for what, i in where.items():
        assert not s.device_accepts(_tampered(s, items, i)), f"circuit A, k = 14: {what} (item {i}) can be changed without the device verifier noticing"
    for what in ("the first advice commitment", "f"):
        ok, _, refused = s.model_verify(_tampered(s, items, where[what]))
        assert not ok and refused == ("opening" if what == "f" else "vanishing identity"), f"circuit A, k = 14: {what}: the model says {refused}"
