"""GPU tests (-m gpu): every exported entry that takes a `field` or a `curve` id refuses an unknown one in the same way -- TRH_EINVAL,
"unknown field id 7" / "unknown curve id 7", the context as usable as before -- whichever file the entry lives in and
wherever its check stands among its other argument checks.  The list below is written out (from api._SIGNATURES and include/trh.h: the
entries whose first parameter is `int field` / `int curve`); test_the_list_is_complete fails when the header gains one that is missing
here.  Every case passes one-element arguments that are valid for id 0, and proves it by making that call straight after the refusal."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tiny_ram_halo2_amd import api, expr as expr_mod

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ID = 7
EINVAL = -1


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


class Args:
    """One-element operands, made once: device buffers hold the field element 1 (a valid, non-zero value in either field) or the
    identity point / its encoding (all zero); nothing here depends on the id."""

    def __init__(self):
        self.keep = []
        self.one = np.array([1, 0, 0, 0], np.uint64)
        self.h4, self.h8, self.h12 = np.zeros(4, np.uint64), np.zeros(8, np.uint64), np.zeros(12, np.uint64)
        self.bytes32 = ctypes.create_string_buffer(32)
        self.handle = ctypes.c_void_p()

    def ones(self, elems=1):  # `elems` field elements, each 1
        t = torch.zeros((elems, 4), dtype=torch.int64, device="cuda")
        t[:, 0] = 1
        self.keep.append(t)
        return ctypes.c_void_p(t.data_ptr())

    def zeros(self, nbytes):
        t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        self.keep.append(t)
        return ctypes.c_void_p(t.data_ptr())

    def out(self):  # a fresh handle slot; the valid call's handle is destroyed by the case's `free`
        self.handle = ctypes.c_void_p()
        return ctypes.byref(self.handle)


def _term(a):
    arr = (api.ProductTerm * 1)()
    arr[0].x = a.ones().value
    arr[0].y = None
    arr[0].g[:] = [1, 0, 0, 0]
    a.keep.append(arr)
    return ctypes.cast(arr, ctypes.c_void_p)


def _insns(a):
    arr = (expr_mod._Insn * 2)()
    arr[0] = expr_mod._Insn(expr_mod.OP["PUSH_COLUMN"], 0, 0)
    arr[1] = expr_mod._Insn(expr_mod.OP["STORE_TOP"], 0, 0)
    a.keep.append(arr)
    return ctypes.cast(arr, ctypes.c_void_p)


_P = api._p
_STARTS = (ctypes.c_uint32 * 2)(0, 1)
_FREE = {"bases": "trh_bases_destroy", "domain": "trh_domain_destroy", "expr": "trh_expr_destroy"}

# name -> (kind of id, what the valid call leaves to destroy, arguments after the id)
ENTRIES = {
    "trh_bases_wrap_device": ("curve", "bases", lambda a: (a.zeros(64), 1, a.out())),
    "trh_bases_generate": ("curve", "bases", lambda a: (0x1234, 0x10001, 0, 1, a.out())),
    "trh_bases_create_compressed": ("curve", "bases", lambda a: (ctypes.cast(a.bytes32, ctypes.c_void_p), 1, a.out())),
    "trh_point_sum": ("curve", None, lambda a: (_P(a.h12), 1, _P(a.h12.copy()))),
    "trh_point_to_bytes": ("curve", None, lambda a: (_P(a.h12), ctypes.cast(ctypes.create_string_buffer(32), ctypes.c_void_p))),
    "trh_point_from_bytes": ("curve", None, lambda a: (ctypes.cast(a.bytes32, ctypes.c_void_p), _P(a.h8))),
    "trh_point_op_dev": ("curve", None, lambda a: (api.POINT_OPS["dbl"], a.zeros(96), None, a.zeros(96), 1, None)),
    "trh_point_fft_dev": ("curve", None, lambda a: (a.zeros(64), 0, _P(a.one), None, None)),
    "trh_bases_fold_dev": ("curve", None, lambda a: (a.zeros(64), a.zeros(64), 1, _P(a.one), None)),
    "trh_points_compress_dev": ("curve", None, lambda a: (a.zeros(64), a.zeros(32), 1, None)),
    "trh_points_decompress_dev": ("curve", None, lambda a: (a.zeros(32), a.zeros(64), None, 1, None, None)),
    "trh_ntt_dev": ("field", None, lambda a: (a.ones(), 0, _P(a.one), 1, None)),
    "trh_field_scale_dev": ("field", None, lambda a: (a.ones(), 1, _P(a.one), None)),
    "trh_field_scale_periodic_dev": ("field", None, lambda a: (a.ones(), 1, _P(a.one), 1, None)),
    "trh_field_scale_rows_dev": ("field", None, lambda a: (a.ones(), 1, 1, 1, _P(a.one), 1, None)),
    "trh_domain_create": ("field", "domain", lambda a: (2, 4, a.out())),
    "trh_field_inner_product_dev": ("field", None, lambda a: (a.ones(), a.ones(), 1, None, _P(a.h4))),
    "trh_poly_eval_batch_dev": ("field", None, lambda a: (a.ones(), 1, 1, _P(a.one), None, _P(a.h4))),
    "trh_field_axpy_dev": ("field", None, lambda a: (a.ones(), a.ones(), 1, _P(a.one), None)),
    "trh_field_powers_dev": ("field", None, lambda a: (a.ones(), 1, _P(a.one), None)),
    "trh_field_batch_invert_dev": ("field", None, lambda a: (a.ones(), 1, None)),
    "trh_field_batch_invert_mul_dev": ("field", None, lambda a: (a.ones(), a.ones(), 1, None)),
    "trh_product_terms_dev": ("field", None, lambda a: (_term(a), _STARTS, 1, 1, a.ones(), None)),
    "trh_field_prefix_product_dev": ("field", None, lambda a: (a.ones(), a.ones(), 1, None)),
    "trh_field_prefix_product_rows_dev": ("field", None, lambda a: (a.ones(), a.ones(), 1, 1, None)),
    "trh_field_prefix_sum_dev": ("field", None, lambda a: (a.ones(), a.ones(), 1, None)),
    "trh_poly_lincomb_dev": ("field", None, lambda a: (a.ones(), 1, 1, _P(a.one), a.ones(), None)),
    "trh_poly_kate_division_dev": ("field", None, lambda a: (a.ones(), 1, a.ones(), a.ones(), a.ones(2), a.ones(), None)),
    "trh_lookup_permute_dev": ("field", None, lambda a: (a.ones(), a.ones(), 1, a.ones(), a.ones(), None)),
    "trh_lookup_permute_batch_dev": ("field", None, lambda a: (a.ones(), a.ones(), 1, 1, 1, a.ones(), a.ones(), None)),
    "trh_expr_create": ("field", "expr", lambda a: (_insns(a), 2, None, 0, 1, 1, 0, a.out())),
    "trh_field_sqrt_dev": ("field", None, lambda a: (a.ones(), a.ones(), a.zeros(16), 1, None)),
    "trh_field_op_dev": ("field", None, lambda a: (api.FIELD_OPS["add"], a.ones(), a.ones(), a.ones(), 1, None)),
}


def test_the_list_is_complete():
    header = open(os.path.join(ROOT, "include", "trh.h")).read()
    declared = set(re.findall(r"\bint (trh_\w+)\(int (?:field|curve)\b", header))
    assert declared == set(ENTRIES), sorted(declared ^ set(ENTRIES))
    for name, (kind, _, _) in ENTRIES.items():
        assert api._SIGNATURES[name][0][0] is ctypes.c_int and api._SIGNATURES[name][1] is ctypes.c_int, name
        assert re.search(r"\bint %s\(int %s\b" % (name, kind), header), name


@pytest.mark.parametrize("name", list(ENTRIES))
def test_unknown_id_is_refused_and_the_context_stays_usable(name):
    kind, leaves, make = ENTRIES[name]
    lib = api.lib()
    fn = getattr(lib, name)
    a = Args()
    args = make(a)
    torch.cuda.synchronize()
    assert fn(BAD_ID, *args) == EINVAL
    assert lib.trh_last_error().decode() == f"unknown {kind} id {BAD_ID}"
    assert a.handle.value is None  # no handle came out of the refusal
    rc = fn(0, *make(a))  # fresh operands: an output of the first call is not an input of the second
    assert rc == 0, lib.trh_last_error().decode()
    torch.cuda.synchronize()
    if leaves:
        assert a.handle.value is not None
        getattr(lib, _FREE[leaves])(a.handle)

