"""CPU tests of the IPA verifier accumulator's C ABI (include/trh.h, csrc/ipaverify.hip): the entries are exported and bound by the
Python mirror; without a GPU each of them fails loudly with TRH_ENODEV and a message (no CPU fallback)."""
import ctypes

import numpy as np
import pytest

from tiny_ram_halo2_amd import api

NEW_ENTRIES = (
    "trh_ipa_msm_create", "trh_ipa_msm_destroy", "trh_ipa_msm_append_term", "trh_ipa_msm_add_constant_term", "trh_ipa_msm_add_to_w_scalar",
    "trh_ipa_msm_add_to_u_scalar", "trh_ipa_msm_add_to_g_scalars_dev", "trh_ipa_msm_use_challenges", "trh_ipa_msm_scale", "trh_ipa_msm_add_msm",
    "trh_ipa_msm_eval", "trh_ipa_msm_g_scalars_dev",
)


def test_ipa_msm_entries_are_exported():
    lib = api.lib()
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported by libtrh.so"
        assert name in api.EXPORTED_SYMBOLS, f"{name} is not bound in api.py"


def _has_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_ipa_msm_entries_without_a_device():
    lib = api.lib()
    s = np.zeros(4, np.uint64)
    xy = np.zeros(8, np.uint64)
    out = np.zeros(12, np.uint64)
    h = ctypes.c_void_p()
    flag = ctypes.c_int(7)
    calls = {
        "create": lambda: lib.trh_ipa_msm_create(None, 4, api._p(xy), ctypes.byref(h)),
        "append_term": lambda: lib.trh_ipa_msm_append_term(None, api._p(s), api._p(xy)),
        "add_constant_term": lambda: lib.trh_ipa_msm_add_constant_term(None, api._p(s)),
        "add_to_w_scalar": lambda: lib.trh_ipa_msm_add_to_w_scalar(None, api._p(s)),
        "add_to_u_scalar": lambda: lib.trh_ipa_msm_add_to_u_scalar(None, api._p(s)),
        "add_to_g_scalars_dev": lambda: lib.trh_ipa_msm_add_to_g_scalars_dev(None, None, None),
        "use_challenges": lambda: lib.trh_ipa_msm_use_challenges(None, 1, api._p(s), api._p(s), None, None, None),
        "scale": lambda: lib.trh_ipa_msm_scale(None, api._p(s), None),
        "add_msm": lambda: lib.trh_ipa_msm_add_msm(None, None, None),
        "eval": lambda: lib.trh_ipa_msm_eval(None, None, ctypes.byref(flag), api._p(out)),
    }
    for what, call in calls.items():
        assert call() == -2, what
        assert b"trh_init" in lib.trh_last_error(), what
    assert not h.value and flag.value == 7
    assert lib.trh_ipa_msm_g_scalars_dev(None) is None and b"trh_init" in lib.trh_last_error()
    lib.trh_ipa_msm_destroy(None)  # a no-op, as free(NULL)
