"""tests/quotient_model.py against itself, no device: on a satisfying witness the folded permutation and lookup terms are a polynomial
that X^n - 1 divides, of the degree the argument's shape gives, in both layouts of the extended domain; one changed value breaks the
division.  And the new entries fail loudly without a device."""
import ctypes

import pytest

import quotient_model as qm
from tiny_ram_halo2_amd import api
from tiny_ram_halo2_amd.poly import _MODULUS, EvaluationDomain

K, N_COLUMNS, CHUNK, N_LOOKUPS, BLINDING = 3, 5, 2, 2, 2
BETA, GAMMA, Y = 0x1234567 ** 5, 0x7654321 ** 7, 0xABCDEF ** 9


@pytest.fixture(scope="module", params=["fp", "fq"])
def case(request):
    field = request.param
    m = _MODULUS[field]
    dom = EvaluationDomain(field, CHUNK + 3, K)  # degree (chunk_len + 2)(n - 1): chunk_len + 2 blocks
    assert dom.extended_k == K + 2
    w = qm.Witness(field, K, N_COLUMNS, CHUNK, N_LOOKUPS, BLINDING, BETA % m, GAMMA % m, seed=11)
    return field, m, dom, w


def test_the_numerator_is_divisible_and_of_the_expected_degree(case):
    field, m, dom, w = case
    n = 1 << K
    num = w.numerator(qm.Layout(dom), BETA % m, GAMMA % m, Y % m)
    coeffs = qm.extended_to_coeff(dom, num)
    assert qm.residues_mod_vanishing(m, coeffs, n) == [0] * n
    assert qm.degree(coeffs) == (CHUNK + 2) * (n - 1)  # l_active * z * chunk_len factors, each of degree n - 1


def test_one_changed_value_breaks_the_division(case):
    field, m, dom, w = case
    n = 1 << K

    def residues(spoil):
        num = w.numerator(qm.Layout(dom), BETA % m, GAMMA % m, Y % m, spoil=spoil)
        return qm.residues_mod_vanishing(m, qm.extended_to_coeff(dom, num), n)

    def value(values, sigmas, zs, lookups):
        c = next(c for c in w.copies if c[:2] != c[2:])  # a cell that a copy ties to another one
        values[c[0]][c[1]] = (values[c[0]][c[1]] + 1) % m

    def product(values, sigmas, zs, lookups):
        zs[1][2] = (zs[1][2] + 1) % m

    def permuted(values, sigmas, zs, lookups):
        lookups[1][2][1] = (lookups[1][2][1] + 1) % m

    for spoil in (value, product, permuted):
        assert any(residues(spoil)), spoil.__name__


def test_the_block_layout_holds_the_rows_of_the_flat_one(case):
    field, m, dom, w = case
    n, shift = 1 << K, dom.extended_k - K
    flat = w.numerator(qm.Layout(dom), BETA % m, GAMMA % m, Y % m, acc=list(range(1, (n << shift) + 1)))
    for n_blocks in (1, 3, 4):
        acc = [1 + (q << shift) + r for r in range(n_blocks) for q in range(n)]
        blocks = w.numerator(qm.Layout(dom, n_blocks), BETA % m, GAMMA % m, Y % m, acc=acc)
        assert blocks == [flat[(q << shift) + r] for r in range(n_blocks) for q in range(n)]


def test_permute_expression_pair():
    a, s_ = [5, 3, 5, 5, 9, 3], [9, 3, 5, 7, 7, 1]
    ap, sp = qm.permute_expression_pair(97, a, s_)
    assert sorted(ap) == sorted(a) and sorted(sp) == sorted(s_) and ap[0] == sp[0]
    assert all(ap[i] == sp[i] or ap[i] == ap[i - 1] for i in range(1, len(a)))
    with pytest.raises(AssertionError):
        qm.permute_expression_pair(97, [2], [3])


def _has_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_no_device_fails_loudly():
    """without trh_init both entries return TRH_ENODEV (-2), whatever their arguments"""
    lib = api.lib()
    out = ctypes.c_void_p()
    assert lib.trh_quotient_create(None, 4, 4, 1, 5, ctypes.byref(out)) == -2
    assert b"trh_init" in lib.trh_last_error()
    assert lib.trh_quotient_terms_dev(None, None) == -2
