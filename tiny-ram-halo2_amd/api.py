"""ctypes binding of libtrh.so plus a host-side mirror of the halo2_proofs interface for the
MSM / NTT / commitment hot path (same names and argument meaning as the Rust functions the
reference reaches through create_proof, /root/reference/src/test_utils.rs:21-49):

    best_multiexp(coeffs, bases)            halo2_proofs::arithmetic::best_multiexp
    best_fft(a, omega, log_n)               halo2_proofs::arithmetic::best_fft
    Params(curve, g, g_lagrange, w, u)      halo2_proofs::poly::commitment::Params
        .commit(poly, r) / .commit_lagrange(poly, r)
    EvaluationDomain(field, k, j)           halo2_proofs::poly::EvaluationDomain
        .lagrange_to_coeff / .coeff_to_extended / .extended_to_coeff

Arrays are numpy uint64 (little-endian limbs, Montgomery form) on the host, or raw device
pointers (ints / torch tensors' data_ptr()) for the *_dev forms.  The library has no CPU
fallback: loading fails loudly if libtrh.so is missing, and every compute call raises
TrhError when no MI355X is bound.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TRH_LIB_PATH") or os.path.join(_HERE, "libtrh.so")  # the override serves same-box A/B measurements of two builds

PALLAS, VESTA = 0, 1
FP, FQ = 0, 1
CURVE_ID = {"pallas": PALLAS, "vesta": VESTA}
FIELD_ID = {"fp": FP, "fq": FQ}
# scalar field of each curve (pallas: base Fp / scalar Fq; vesta: base Fq / scalar Fp)
SCALAR_FIELD = {"pallas": "fq", "vesta": "fp"}
BASE_FIELD = {"pallas": "fp", "vesta": "fq"}
FIELD_OPS = {"add": 0, "sub": 1, "mul": 2, "sqr": 3, "neg": 4, "inv": 5, "to_mont": 6, "from_mont": 7}
POINT_OPS = {"add": 0, "madd": 1, "dbl": 2, "q4_add": 3, "q4_dbl": 4}  # q4_*: the quad-lane arithmetic of csrc/curve_q4.h

_u64p = ctypes.POINTER(ctypes.c_uint64)
_vp = ctypes.c_void_p


class TrhError(RuntimeError):
    pass


WRITE_POINT_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64))
WRITE_SCALAR_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64))
SQUEEZE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64))
RNG_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64))


class Transcript(ctypes.Structure):
    _fields_ = [("ctx", ctypes.c_void_p), ("write_point", WRITE_POINT_FN), ("write_scalar", WRITE_SCALAR_FN),
                ("squeeze_challenge_scalar", SQUEEZE_FN)]


class Timing(ctypes.Structure):
    _fields_ = [("total_ms", ctypes.c_float), ("digits_ms", ctypes.c_float), ("sort_ms", ctypes.c_float),
                ("accumulate_ms", ctypes.c_float), ("reduce_ms", ctypes.c_float),
                ("window_bits", ctypes.c_int), ("windows", ctypes.c_int), ("accumulate_kernel_ms", ctypes.c_float)]


class IoStats(ctypes.Structure):
    _fields_ = [("h2d_bytes", ctypes.c_double), ("d2h_bytes", ctypes.c_double), ("h2d_seconds", ctypes.c_double), ("d2h_seconds", ctypes.c_double),
                ("h2d_zero_bytes", ctypes.c_double)]


class QuotientArgs(ctypes.Structure):
    """trh_quotient_args_t"""
    _fields_ = [("perm_values", ctypes.POINTER(ctypes.c_void_p)), ("perm_sigmas", ctypes.POINTER(ctypes.c_void_p)), ("perm_z", ctypes.POINTER(ctypes.c_void_p)),
                ("lookups", ctypes.POINTER(ctypes.c_void_p)), ("l0", ctypes.c_void_p), ("l_blind", ctypes.c_void_p), ("l_last", ctypes.c_void_p),
                ("beta", ctypes.c_uint64 * 4), ("gamma", ctypes.c_uint64 * 4), ("y", ctypes.c_uint64 * 4), ("acc", ctypes.c_void_p),
                ("n_blocks", ctypes.c_uint32), ("stream", ctypes.c_void_p)]


class ProductChainArgs(ctypes.Structure):
    """trh_product_chain_args_t"""
    _fields_ = [("z", ctypes.c_void_p), ("n", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("link", ctypes.c_size_t), ("stream", ctypes.c_void_p)]


class IntsArgs(ctypes.Structure):
    """trh_ints_args_t"""
    _fields_ = [("kind", ctypes.c_int), ("src", ctypes.c_void_p), ("src_stride", ctypes.c_size_t), ("n_cols", ctypes.c_size_t), ("live_rows", ctypes.c_size_t),
                ("dst", ctypes.c_void_p), ("dst_odd", ctypes.c_void_p), ("n", ctypes.c_size_t), ("stream", ctypes.c_void_p)]


class EvenBitsTableArgs(ctypes.Structure):
    """trh_even_bits_table_args_t"""
    _fields_ = [("word_bits", ctypes.c_uint32), ("dst", ctypes.c_void_p), ("n", ctypes.c_size_t), ("stream", ctypes.c_void_p)]


class MemTableArgs(ctypes.Structure):
    """trh_mem_table_args_t"""
    _fields_ = [("word_bits", ctypes.c_uint32), ("address", ctypes.c_void_p), ("time", ctypes.c_void_p), ("value", ctypes.c_void_p), ("store_bits", ctypes.c_void_p),
                ("m", ctypes.c_size_t), ("tape", ctypes.c_void_p), ("t", ctypes.c_size_t), ("dst", ctypes.c_void_p), ("n", ctypes.c_size_t), ("max_rows", ctypes.c_size_t),
                ("src_index", ctypes.c_void_p), ("stream", ctypes.c_void_p), ("rows", ctypes.c_uint64), ("n_inconsistent", ctypes.c_uint64),
                ("first_inconsistent", ctypes.c_uint64)]


class ExeTableArgs(ctypes.Structure):
    """trh_exe_table_args_t"""
    _fields_ = [("word_bits", ctypes.c_uint32), ("reg_count", ctypes.c_uint32), ("pc", ctypes.c_void_p), ("inst", ctypes.c_void_p), ("a", ctypes.c_void_p),
                ("value", ctypes.c_void_p), ("regs", ctypes.c_void_p), ("flag_bits", ctypes.c_void_p), ("m", ctypes.c_size_t), ("selection", ctypes.c_uint32 * 32),
                ("dst", ctypes.c_void_p), ("n", ctypes.c_size_t), ("stream", ctypes.c_void_p)]


class ExeChipsArgs(ctypes.Structure):
    """trh_exe_chips_args_t"""
    _fields_ = [("word_bits", ctypes.c_uint32), ("reg_count", ctypes.c_uint32), ("pc", ctypes.c_void_p), ("inst", ctypes.c_void_p), ("a", ctypes.c_void_p),
                ("value", ctypes.c_void_p), ("regs", ctypes.c_void_p), ("flag_bits", ctypes.c_void_p), ("m", ctypes.c_size_t), ("selection", ctypes.c_uint32 * 32),
                ("chips", ctypes.c_uint32 * 32), ("dst", ctypes.c_void_p), ("n", ctypes.c_size_t), ("stream", ctypes.c_void_p)]


_SIGNATURES = {
    "trh_init": ([ctypes.c_int], ctypes.c_int),
    "trh_shutdown": ([], None),
    "trh_last_error": ([], ctypes.c_char_p),
    "trh_device_count": ([], ctypes.c_int),
    "trh_version": ([], ctypes.c_char_p),
    "trh_set_option": ([ctypes.c_char_p, ctypes.c_char_p], ctypes.c_int),
    "trh_get_option": ([ctypes.c_char_p, ctypes.POINTER(ctypes.c_long)], ctypes.c_int),
    "trh_init_multi": ([ctypes.POINTER(ctypes.c_int), ctypes.c_int], ctypes.c_int),
    "trh_group_size": ([], ctypes.c_int),
    "trh_group_peer_access": ([], ctypes.c_int),
    "trh_set_shard_min": ([ctypes.c_size_t], ctypes.c_int),
    "trh_ctx_create": ([ctypes.c_int, ctypes.POINTER(_vp)], ctypes.c_int),
    "trh_ctx_destroy": ([_vp], None),
    "trh_ctx_set_current": ([_vp], ctypes.c_int),
    "trh_ctx_device": ([_vp], ctypes.c_int),
    "trh_ctx_stream": ([_vp], _vp),
    "trh_best_multiexp_pallas": ([_u64p, _u64p, ctypes.c_size_t, _u64p], ctypes.c_int),
    "trh_best_multiexp_vesta": ([_u64p, _u64p, ctypes.c_size_t, _u64p], ctypes.c_int),
    "trh_best_fft_fp": ([_u64p, _u64p, ctypes.c_uint32], ctypes.c_int),
    "trh_best_fft_fq": ([_u64p, _u64p, ctypes.c_uint32], ctypes.c_int),
    "trh_bases_create_pallas": ([_u64p, ctypes.c_size_t, ctypes.POINTER(_vp)], ctypes.c_int),
    "trh_bases_create_vesta": ([_u64p, ctypes.c_size_t, ctypes.POINTER(_vp)], ctypes.c_int),
    "trh_bases_wrap_device": ([ctypes.c_int, _vp, ctypes.c_size_t, ctypes.POINTER(_vp)], ctypes.c_int),
    "trh_bases_generate": ([ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_size_t, ctypes.POINTER(_vp)], ctypes.c_int),
    "trh_bases_download": ([_vp, ctypes.c_size_t, ctypes.c_size_t, _u64p], ctypes.c_int),
    "trh_bases_device_ptr": ([_vp], _vp),
    "trh_bases_len": ([_vp], ctypes.c_size_t),
    "trh_bases_shards": ([_vp], ctypes.c_int),
    "trh_bases_destroy": ([_vp], None),
    "trh_bases_precompute": ([_vp, ctypes.c_int], ctypes.c_int),
    "trh_bases_precomputed_window_bits": ([_vp], ctypes.c_int),
    "trh_bases_reserve": ([_vp, ctypes.c_size_t, ctypes.c_size_t], ctypes.c_int),
    "trh_msm": ([_vp, ctypes.c_size_t, _u64p, ctypes.c_size_t, ctypes.c_int, _u64p], ctypes.c_int),
    "trh_msm_dev": ([_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp, _u64p], ctypes.c_int),
    "trh_msm_dev_enqueue": ([_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp], ctypes.c_int),
    "trh_msm_dev_finish": ([_vp, _vp, _u64p], ctypes.c_int),
    "trh_msm_batch_dev": ([_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, _vp, _u64p], ctypes.c_int),
    "trh_commit_batch_dev": ([_vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _u64p, _vp, _u64p], ctypes.c_int),
    "trh_msm_set_window_bits": ([ctypes.c_int], ctypes.c_int),
    "trh_point_sum": ([ctypes.c_int, _u64p, ctypes.c_size_t, _u64p], ctypes.c_int),
    "trh_ntt_dev": ([ctypes.c_int, _vp, ctypes.c_uint32, _u64p, ctypes.c_size_t, _vp], ctypes.c_int),
    "trh_field_scale_dev": ([ctypes.c_int, _vp, ctypes.c_size_t, _u64p, _vp], ctypes.c_int),
    "trh_field_scale_periodic_dev": ([ctypes.c_int, _vp, ctypes.c_size_t, _u64p, ctypes.c_uint32, _vp], ctypes.c_int),
    "trh_field_scale_rows_dev": ([ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, _u64p, ctypes.c_uint32, _vp], ctypes.c_int),
    "trh_field_inner_product_dev": ([ctypes.c_int, _vp, _vp, ctypes.c_size_t, _vp, _u64p], ctypes.c_int),
    "trh_field_axpy_dev": ([ctypes.c_int, _vp, _vp, ctypes.c_size_t, _u64p, _vp], ctypes.c_int),
    "trh_field_powers_dev": ([ctypes.c_int, _vp, ctypes.c_size_t, _u64p, _vp], ctypes.c_int),
    "trh_bases_fold_dev": ([ctypes.c_int, _vp, _vp, ctypes.c_size_t, _u64p, _vp], ctypes.c_int),
    "trh_point_fft_dev": ([ctypes.c_int, _vp, ctypes.c_uint32, _u64p, _u64p, _vp], ctypes.c_int),
    "trh_domain_create": ([ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_vp)], ctypes.c_int),
    "trh_domain_destroy": ([_vp], None),
    "trh_domain_reserve": ([_vp, ctypes.c_size_t], ctypes.c_int),
    "trh_domain_extended_k": ([_vp], ctypes.c_uint32),
    "trh_domain_constant": ([_vp, ctypes.c_int, _u64p], ctypes.c_int),
    "trh_domain_lagrange_to_coeff": ([_vp, _vp, ctypes.c_size_t, _vp], ctypes.c_int),
    "trh_domain_coeff_to_extended": ([_vp, _vp, _vp, ctypes.c_size_t, _vp], ctypes.c_int),
    "trh_domain_extended_to_coeff": ([_vp, _vp, ctypes.c_size_t, _vp], ctypes.c_int),
    "trh_domain_divide_by_vanishing_poly": ([_vp, _vp, ctypes.c_size_t, _vp], ctypes.c_int),
    "trh_ipa_create_proof": ([_vp, _u64p, ctypes.c_uint32, _vp, _u64p, _u64p, _vp, _u64p, ctypes.POINTER(Transcript), RNG_FN, _vp, _vp, _u64p, _u64p], ctypes.c_int),
    "trh_ipa_collapse_generators_dev": ([_vp, ctypes.c_uint32, ctypes.c_uint32, _u64p, _vp, _vp, _vp], ctypes.c_int),
    "trh_ipa_msm_create": ([_vp, ctypes.c_uint32, _u64p, ctypes.POINTER(_vp)], ctypes.c_int),
    "trh_ipa_msm_destroy": ([_vp], None),
    "trh_ipa_msm_append_term": ([_vp, _u64p, _u64p], ctypes.c_int),
    "trh_ipa_msm_add_constant_term": ([_vp, _u64p], ctypes.c_int),
    "trh_ipa_msm_add_to_w_scalar": ([_vp, _u64p], ctypes.c_int),
    "trh_ipa_msm_add_to_u_scalar": ([_vp, _u64p], ctypes.c_int),
    "trh_ipa_msm_add_to_g_scalars_dev": ([_vp, _vp, _vp], ctypes.c_int),
    "trh_ipa_msm_use_challenges": ([_vp, ctypes.c_size_t, _u64p, _u64p, _u64p, _u64p, _vp], ctypes.c_int),
    "trh_ipa_msm_scale": ([_vp, _u64p, _vp], ctypes.c_int),
    "trh_ipa_msm_add_msm": ([_vp, _vp, _vp], ctypes.c_int),
    "trh_ipa_msm_eval": ([_vp, _vp, ctypes.POINTER(ctypes.c_int), _u64p], ctypes.c_int),
    "trh_ipa_msm_g_scalars_dev": ([_vp], _vp),
    "trh_poly_eval_batch_dev": ([ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, _u64p, _vp, _u64p], ctypes.c_int),
    "trh_field_batch_invert_dev": ([ctypes.c_int, _vp, ctypes.c_size_t, _vp], ctypes.c_int),
    "trh_field_batch_invert_mul_dev": ([ctypes.c_int, _vp, _vp, ctypes.c_size_t, _vp], ctypes.c_int),
    "trh_product_terms_dev": ([ctypes.c_int, _vp, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.c_size_t, _vp, _vp], ctypes.c_int),
    "trh_field_prefix_product_dev": ([ctypes.c_int, _vp, _vp, ctypes.c_size_t, _vp], ctypes.c_int),
    "trh_lookup_permute_dev": ([ctypes.c_int, _vp, _vp, ctypes.c_size_t, _vp, _vp, _vp], ctypes.c_int),
    "trh_lookup_permute_batch_dev": ([ctypes.c_int, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp, _vp], ctypes.c_int),
    "trh_expr_create": ([ctypes.c_int, _vp, ctypes.c_size_t, _u64p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                         ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "trh_expr_destroy": ([_vp], None),
    "trh_expr_lds_slots": ([_vp], ctypes.c_uint32),
    "trh_expr_set_const": ([_vp, ctypes.c_uint32, _u64p], ctypes.c_int),
    "trh_expr_eval_dev": ([_vp, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_uint32, _vp], ctypes.c_int),
    "trh_expr_check_dev": ([_vp, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_size_t, _u64p, _u64p, _vp], ctypes.c_int),
    "trh_lookup_check_dev": ([ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_size_t, _u64p, _u64p, _vp],
                             ctypes.c_int),
    "trh_quotient_create": ([_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_vp)], ctypes.c_int),
    "trh_quotient_destroy": ([_vp], None),
    "trh_quotient_terms_dev": ([_vp, ctypes.POINTER(QuotientArgs)], ctypes.c_int),
    "trh_field_prefix_product_rows_dev": ([ctypes.c_int, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp], ctypes.c_int),
    "trh_product_chain_dev": ([ctypes.c_int, ctypes.POINTER(ProductChainArgs)], ctypes.c_int),
    "trh_field_prefix_sum_dev": ([ctypes.c_int, _vp, _vp, ctypes.c_size_t, _vp], ctypes.c_int),
    "trh_poly_lincomb_dev": ([ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, _u64p, _vp, _vp], ctypes.c_int),
    "trh_poly_kate_division_dev": ([ctypes.c_int, _vp, ctypes.c_size_t, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "trh_stat": ([ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
    "trh_event_create": ([ctypes.POINTER(_vp)], ctypes.c_int),
    "trh_event_record": ([_vp, _vp], ctypes.c_int),
    "trh_event_elapsed_ms": ([_vp, _vp, ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
    "trh_event_destroy": ([_vp], None),
    "trh_field_op_dev": ([ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, ctypes.c_size_t, _vp], ctypes.c_int),
    "trh_point_op_dev": ([ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, ctypes.c_size_t, _vp], ctypes.c_int),
    "trh_malloc": ([ctypes.POINTER(_vp), ctypes.c_size_t], ctypes.c_int),
    "trh_free": ([_vp], ctypes.c_int),
    "trh_pool_trim": ([], ctypes.c_int),
    "trh_pool_idle_bytes": ([], ctypes.c_size_t),
    "trh_memcpy_h2d": ([_vp, _vp, ctypes.c_size_t], ctypes.c_int),
    "trh_memcpy_d2h": ([_vp, _vp, ctypes.c_size_t], ctypes.c_int),
    "trh_stream_synchronize": ([_vp], ctypes.c_int),
    "trh_best_fft_batch_fp": ([ctypes.POINTER(_u64p), ctypes.c_size_t, _u64p, ctypes.c_uint32], ctypes.c_int),
    "trh_best_fft_batch_fq": ([ctypes.POINTER(_u64p), ctypes.c_size_t, _u64p, ctypes.c_uint32], ctypes.c_int),
    "trh_commit_batch_host": ([_vp, ctypes.POINTER(_u64p), ctypes.c_size_t, ctypes.c_size_t, _u64p, _u64p], ctypes.c_int),
    "trh_domain_quotient_blocks": ([_vp], ctypes.c_uint32),
    "trh_domain_coeff_to_extended_blocks": ([_vp, _vp, _vp, ctypes.c_size_t, ctypes.c_uint32, _vp], ctypes.c_int),
    "trh_domain_blocks_to_quotient": ([_vp, _vp, _vp, ctypes.c_int, _vp], ctypes.c_int),
    "trh_expr_eval_blocks_dev": ([_vp, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_uint32, _vp], ctypes.c_int),
    "trh_domain_lagrange_to_coeff_host": ([_vp, ctypes.POINTER(_u64p), ctypes.c_size_t], ctypes.c_int),
    "trh_domain_coeff_to_extended_host": ([_vp, ctypes.POINTER(_u64p), ctypes.POINTER(_u64p), ctypes.c_size_t], ctypes.c_int),
    "trh_domain_extended_to_coeff_host": ([_vp, _u64p, ctypes.c_int], ctypes.c_int),
    "trh_domain_coeff_to_extended_blocks_host": ([_vp, ctypes.POINTER(_u64p), ctypes.POINTER(_u64p), ctypes.c_size_t, ctypes.c_uint32], ctypes.c_int),
    "trh_domain_blocks_to_quotient_host": ([_vp, _u64p, _u64p, ctypes.c_int], ctypes.c_int),
    "trh_host_register": ([_vp, ctypes.c_size_t], ctypes.c_int),
    "trh_host_unregister": ([_vp], ctypes.c_int),
    "trh_host_alloc": ([ctypes.POINTER(_vp), ctypes.c_size_t], ctypes.c_int),
    "trh_host_free": ([_vp], ctypes.c_int),
    "trh_io_stats": ([ctypes.POINTER(IoStats), ctypes.c_int], ctypes.c_int),
    "trh_field_sqrt_dev": ([ctypes.c_int, _vp, _vp, _vp, ctypes.c_size_t, _vp], ctypes.c_int),
    "trh_points_compress_dev": ([ctypes.c_int, _vp, _vp, ctypes.c_size_t, _vp], ctypes.c_int),
    "trh_points_decompress_dev": ([ctypes.c_int, _vp, _vp, _vp, ctypes.c_size_t, _vp, _u64p], ctypes.c_int),
    "trh_bases_create_compressed": ([ctypes.c_int, _vp, ctypes.c_size_t, ctypes.POINTER(_vp)], ctypes.c_int),
    "trh_bases_download_compressed": ([_vp, ctypes.c_size_t, ctypes.c_size_t, _vp], ctypes.c_int),
    "trh_point_to_bytes": ([ctypes.c_int, _u64p, _vp], ctypes.c_int),
    "trh_point_from_bytes": ([ctypes.c_int, _vp, _u64p], ctypes.c_int),
    "trh_rng_create": ([_vp, ctypes.c_uint64, ctypes.POINTER(_vp)], ctypes.c_int),
    "trh_rng_destroy": ([_vp], None),
    "trh_rng_seek": ([_vp, ctypes.c_uint64], ctypes.c_int),
    "trh_rng_position": ([_vp, ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
    "trh_rng_next_scalar": ([_vp, ctypes.c_int, _u64p], ctypes.c_int),
    "trh_rng_fill_dev": ([_vp, ctypes.c_int, _vp, ctypes.c_size_t, _vp], ctypes.c_int),
    "trh_rng_fill_rows_dev": ([_vp, ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, _vp], ctypes.c_int),
    "trh_perm_create": ([ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_vp)], ctypes.c_int),
    "trh_perm_destroy": ([_vp], None),
    "trh_perm_copy": ([_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32], ctypes.c_int),
    "trh_perm_copy_batch": ([_vp, _vp, ctypes.c_size_t], ctypes.c_int),
    "trh_perm_mapping": ([_vp, ctypes.c_uint32, ctypes.c_uint32, _vp], ctypes.c_int),
    "trh_perm_sigma_dev": ([_vp, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp], ctypes.c_int),
    "trh_perm_check_dev": ([_vp, ctypes.c_int, ctypes.POINTER(_vp), _u64p, _u64p, _vp], ctypes.c_int),
    "trh_hash_to_curve": ([ctypes.c_int, ctypes.c_char_p, _vp, ctypes.c_size_t, _u64p], ctypes.c_int),
    "trh_hash_to_field_indexed_dev": ([ctypes.c_int, ctypes.c_char_p, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_size_t, _vp, _vp], ctypes.c_int),
    "trh_map_to_curve_dev": ([ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_int, _vp, _vp], ctypes.c_int),
    "trh_hash_to_curve_indexed_dev": ([ctypes.c_int, ctypes.c_char_p, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_size_t, _vp, _vp], ctypes.c_int),
    "trh_tr_create_writer": ([ctypes.c_int, ctypes.POINTER(_vp)], ctypes.c_int),
    "trh_tr_create_reader": ([ctypes.c_int, _vp, ctypes.c_size_t, ctypes.POINTER(_vp)], ctypes.c_int),
    "trh_tr_destroy": ([_vp], None),
    "trh_tr_common_point": ([_vp, _u64p], ctypes.c_int),
    "trh_tr_common_scalar": ([_vp, _u64p], ctypes.c_int),
    "trh_tr_write_point": ([_vp, _u64p], ctypes.c_int),
    "trh_tr_write_scalar": ([_vp, _u64p], ctypes.c_int),
    "trh_tr_read_point": ([_vp, _u64p], ctypes.c_int),
    "trh_tr_read_scalar": ([_vp, _u64p], ctypes.c_int),
    "trh_tr_squeeze_challenge_scalar": ([_vp, _u64p], ctypes.c_int),
    "trh_tr_callbacks": ([_vp, ctypes.POINTER(Transcript)], ctypes.c_int),
    "trh_tr_status": ([_vp], ctypes.c_int),
    "trh_tr_message": ([_vp, _vp, ctypes.c_size_t], ctypes.c_int),
    "trh_tr_bytes_len": ([_vp, ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "trh_tr_bytes": ([_vp, _vp, ctypes.c_size_t], ctypes.c_int),
    "trh_tr_remaining": ([_vp, ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "trh_columns_from_ints_dev": ([ctypes.c_int, ctypes.POINTER(IntsArgs)], ctypes.c_int),
    "trh_columns_from_ints_host": ([ctypes.c_int, ctypes.POINTER(IntsArgs)], ctypes.c_int),
    "trh_even_odd_split_dev": ([ctypes.c_int, ctypes.POINTER(IntsArgs)], ctypes.c_int),
    "trh_even_bits_table_dev": ([ctypes.c_int, ctypes.POINTER(EvenBitsTableArgs)], ctypes.c_int),
    "trh_mem_table_dev": ([ctypes.c_int, ctypes.POINTER(MemTableArgs)], ctypes.c_int),
    "trh_exe_table_dev": ([ctypes.c_int, ctypes.POINTER(ExeTableArgs)], ctypes.c_int),
    "trh_exe_chips_dev": ([ctypes.c_int, ctypes.POINTER(ExeChipsArgs)], ctypes.c_int),
    "trh_set_timing": ([ctypes.c_int], ctypes.c_int),
    "trh_last_timing": ([ctypes.POINTER(Timing)], ctypes.c_int),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def lib():
    """Loads libtrh.so; raises if the HIP extension has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TrhError(f"{LIB_PATH} is missing: build it with `make` (hipcc --offload-arch=gfx950); "
                           "there is no CPU fallback for the MSM/NTT path")
        _lib = ctypes.CDLL(LIB_PATH)
        for name, (argtypes, restype) in _SIGNATURES.items():
            try:
                fn = getattr(_lib, name)
            except AttributeError:
                if os.environ.get("TRH_LIB_PATH"):  # an older build loaded for a same-box A/B: entries added since are simply absent
                    continue
                raise
            fn.argtypes = argtypes
            fn.restype = restype
    return _lib


def _check(rc: int):
    if rc != 0:
        raise TrhError(f"libtrh error {rc}: {lib().trh_last_error().decode()}")


def init(device: int = 0):
    _check(lib().trh_init(device))


def set_option(name: str, value) -> None:
    """trh_set_option: a library switch; only while no context exists (before init / after shutdown)"""
    _check(lib().trh_set_option(name.encode(), str(int(value)).encode()))


def get_option(name: str) -> int:
    v = ctypes.c_long(0)
    _check(lib().trh_get_option(name.encode(), ctypes.byref(v)))
    return int(v.value)


def stat(name: str) -> int:
    v = ctypes.c_uint64(0)
    _check(lib().trh_stat(name.encode(), ctypes.byref(v)))
    return int(v.value)


def init_multi(devices):
    """trh_init_multi: the device group range-sharded base sets run on; devices[0] is the process default."""
    arr = (ctypes.c_int * len(devices))(*devices)
    _check(lib().trh_init_multi(arr, len(devices)))


def group_size() -> int:
    return int(lib().trh_group_size())


def set_shard_min(n_points: int):
    _check(lib().trh_set_shard_min(n_points))


class Context:
    """An independent libtrh context (own scratch, own lock) on one device; `with ctx:` binds the calling thread to it."""

    def __init__(self, device: int = 0):
        self.handle = _vp()
        _check(lib().trh_ctx_create(device, ctypes.byref(self.handle)))

    def bind(self):
        _check(lib().trh_ctx_set_current(self.handle))

    @staticmethod
    def unbind():
        _check(lib().trh_ctx_set_current(None))

    def __enter__(self):
        self.bind()
        return self

    def __exit__(self, *exc):
        self.unbind()

    def destroy(self):
        if self.handle:
            lib().trh_ctx_destroy(self.handle)
            self.handle = _vp()


def shutdown():
    lib().trh_shutdown()


def _c(a, cols=None):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a if cols is None else a.reshape(-1, cols)


def _p(a):
    return a.ctypes.data_as(_u64p)


# ---------------------------------------------------------------------------------------
# halo2_proofs::arithmetic
# ---------------------------------------------------------------------------------------
def best_multiexp(curve: str, coeffs, bases) -> np.ndarray:
    """coeffs: (n, 4) Montgomery scalars, bases: (n, 8) affine.  Returns Jacobian (12,) with Z = 1."""
    c, b = _c(coeffs, 4), _c(bases, 8)
    assert c.shape[0] == b.shape[0]  # reference: assert_eq!(coeffs.len(), bases.len())
    out = np.zeros(12, dtype=np.uint64)
    fn = lib().trh_best_multiexp_pallas if curve == "pallas" else lib().trh_best_multiexp_vesta
    _check(fn(_p(c), _p(b), c.shape[0], _p(out)))
    return out


def best_fft(field: str, a, omega, log_n: int) -> np.ndarray:
    """In-place semantics of the Rust function; returns the transformed copy."""
    a = _c(a, 4).copy()
    assert a.shape[0] == 1 << log_n  # reference: assert_eq!(a.len(), 1 << log_n)
    w = _c(omega).reshape(4)
    fn = lib().trh_best_fft_fp if field == "fp" else lib().trh_best_fft_fq
    _check(fn(_p(a), _p(w), log_n))
    return a


def _ptr_array(arrays):
    """host columns -> C array of pointers (the arrays must stay alive for the call)"""
    return (_u64p * len(arrays))(*[_p(a) for a in arrays])


def best_fft_batch(field: str, columns, omega, log_n: int):
    """best_fft over a list of host columns (each (2^log_n, 4) uint64, C-contiguous), IN PLACE, pipelined over PCIe"""
    for a in columns:
        assert a.dtype == np.uint64 and a.flags.c_contiguous and a.size == 4 << log_n  # reference: assert_eq!(a.len(), 1 << log_n)
    w = _c(omega).reshape(4)
    fn = lib().trh_best_fft_batch_fp if field == "fp" else lib().trh_best_fft_batch_fq
    _check(fn(_ptr_array(columns), len(columns), _p(w), log_n))


def io_stats(reset: bool = False) -> dict:
    """bytes moved by the host-pointer entry points and the host seconds spent in the copies, per direction"""
    st = IoStats()
    _check(lib().trh_io_stats(ctypes.byref(st), 1 if reset else 0))
    return {k: getattr(st, k) for k, _ in IoStats._fields_}


def best_fft_inplace(field: str, a: np.ndarray, omega, log_n: int) -> np.ndarray:
    """the Rust signature: transforms the caller's (2^log_n, 4) uint64 array in place"""
    assert a.dtype == np.uint64 and a.flags.c_contiguous and a.size == 4 << log_n  # reference: assert_eq!(a.len(), 1 << log_n)
    w = _c(omega).reshape(4)
    fn = lib().trh_best_fft_fp if field == "fp" else lib().trh_best_fft_fq
    _check(fn(_p(a), _p(w), log_n))
    return a


def point_sum(curve: str, points) -> np.ndarray:
    pts = _c(points, 12)
    out = np.zeros(12, dtype=np.uint64)
    _check(lib().trh_point_sum(CURVE_ID[curve], _p(pts), pts.shape[0], _p(out)))
    return out


def affine_of(jac) -> np.ndarray:
    """Normalised Jacobian (Z = 1 or identity) -> 8-limb affine POD."""
    return np.ascontiguousarray(jac, dtype=np.uint64).reshape(12)[:8].copy()


# ---------------------------------------------------------------------------------------
# device memory helpers
# ---------------------------------------------------------------------------------------
class DeviceBuffer:
    def __init__(self, nbytes: int):
        self.ptr = _vp()
        self.nbytes = nbytes
        _check(lib().trh_malloc(ctypes.byref(self.ptr), nbytes))

    @classmethod
    def from_host(cls, a: np.ndarray) -> "DeviceBuffer":
        a = np.ascontiguousarray(a)
        buf = cls(a.nbytes)
        if a.nbytes:
            _check(lib().trh_memcpy_h2d(buf.ptr, a.ctypes.data_as(_vp), a.nbytes))
        return buf

    def to_host(self, dtype=np.uint64, shape=None) -> np.ndarray:
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        if self.nbytes:
            _check(lib().trh_memcpy_d2h(out.ctypes.data_as(_vp), self.ptr, self.nbytes))
        return out if shape is None else out.reshape(shape)

    def free(self):
        if self.ptr:
            lib().trh_free(self.ptr)
            self.ptr = _vp()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _devptr(x):
    if isinstance(x, DeviceBuffer):
        return x.ptr
    if hasattr(x, "data_ptr"):
        return _vp(x.data_ptr())
    return _vp(int(x))


def field_op_dev(field: str, op: str, a, b=None) -> np.ndarray:
    a = _c(a, 4)
    da = DeviceBuffer.from_host(a)
    db = DeviceBuffer.from_host(_c(b, 4)) if b is not None else None
    do = DeviceBuffer(a.nbytes)
    _check(lib().trh_field_op_dev(FIELD_ID[field], FIELD_OPS[op], da.ptr, db.ptr if db else None, do.ptr, a.shape[0], None))
    _check(lib().trh_stream_synchronize(None))
    return do.to_host(shape=(-1, 4))


def point_op_dev(curve: str, op: str, p, q=None) -> np.ndarray:
    p = _c(p, 12)
    dp = DeviceBuffer.from_host(p)
    dq = DeviceBuffer.from_host(_c(q)) if q is not None else None
    do = DeviceBuffer(p.nbytes)
    _check(lib().trh_point_op_dev(CURVE_ID[curve], POINT_OPS[op], dp.ptr, dq.ptr if dq else None, do.ptr, p.shape[0], None))
    _check(lib().trh_stream_synchronize(None))
    return do.to_host(shape=(-1, 12))


def ntt_dev(field: str, a_dev, log_n: int, omega, batch: int = 1, stream=None):
    w = _c(omega).reshape(4)
    _check(lib().trh_ntt_dev(FIELD_ID[field], _devptr(a_dev), log_n, _p(w), batch, stream))


def field_scale_dev(field: str, a_dev, n: int, factor, stream=None):
    f = _c(factor).reshape(4)
    _check(lib().trh_field_scale_dev(FIELD_ID[field], _devptr(a_dev), n, _p(f), stream))


def field_scale_periodic_dev(field: str, a_dev, n: int, factors, stream=None):
    f = _c(factors, 4)
    _check(lib().trh_field_scale_periodic_dev(FIELD_ID[field], _devptr(a_dev), n, _p(f), f.shape[0], stream))


def field_scale_rows_dev(field: str, a_dev, rows: int, row_len: int, active_len: int, factors, stream=None):
    f = _c(factors, 4)
    _check(lib().trh_field_scale_rows_dev(FIELD_ID[field], _devptr(a_dev), rows, row_len, active_len, _p(f), f.shape[0], stream))


def inner_product_dev(field: str, a_dev, b_dev, n: int, stream=None) -> np.ndarray:
    """halo2_proofs::arithmetic::compute_inner_product on device vectors -> (4,) Montgomery limbs"""
    out = np.zeros(4, dtype=np.uint64)
    _check(lib().trh_field_inner_product_dev(FIELD_ID[field], _devptr(a_dev), _devptr(b_dev), n, stream, _p(out)))
    return out


def poly_eval_batch_dev(field: str, polys_dev, n: int, batch: int, point, stream=None) -> np.ndarray:
    """arithmetic::eval_polynomial of `batch` device polynomials at one point -> (batch, 4) limbs"""
    out = np.zeros((batch, 4), dtype=np.uint64)
    x = _c(point).reshape(4)
    _check(lib().trh_poly_eval_batch_dev(FIELD_ID[field], _devptr(polys_dev), n, batch, _p(x), stream, _p(out)))
    return out


def axpy_dev(field: str, y_dev, x_dev, n: int, c, stream=None):
    cc = _c(c).reshape(4)
    _check(lib().trh_field_axpy_dev(FIELD_ID[field], _devptr(y_dev), _devptr(x_dev), n, _p(cc), stream))


def powers_dev(field: str, out_dev, n: int, x, stream=None):
    xx = _c(x).reshape(4)
    _check(lib().trh_field_powers_dev(FIELD_ID[field], _devptr(out_dev), n, _p(xx), stream))


def bases_fold_dev(curve: str, g_lo_dev, g_hi_dev, half: int, u, stream=None):
    uu = _c(u).reshape(4)
    _check(lib().trh_bases_fold_dev(CURVE_ID[curve], _devptr(g_lo_dev), _devptr(g_hi_dev), half, _p(uu), stream))


def point_fft_dev(curve: str, points_dev, log_n: int, omega, scale=None, stream=None):
    """best_fft over curve points (Params::new's g -> g_lagrange); `scale` multiplies every output (n^-1)"""
    w = _c(omega).reshape(4)
    sc = None if scale is None else _c(scale).reshape(4)
    _check(lib().trh_point_fft_dev(CURVE_ID[curve], _devptr(points_dev), log_n, _p(w), None if sc is None else _p(sc), stream))


def batch_invert_dev(field: str, a_dev, n: int, stream=None):
    """ff::BatchInvert on a device vector, in place (zeros stay zero)"""
    _check(lib().trh_field_batch_invert_dev(FIELD_ID[field], _devptr(a_dev), n, stream))


class ProductTerm(ctypes.Structure):
    """trh_product_term_t: x[i] + c * y[i] + g (y null: x[i] + g); c / g Montgomery words"""
    _fields_ = [("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("c", ctypes.c_uint64 * 4), ("g", ctypes.c_uint64 * 4)]


def product_terms_dev(field: str, rows, n: int, out_dev, stream=None):
    """rows: a list of rows, each a list of terms (x_dev, y_dev or None, c limbs or None, g limbs); out[r][i] = prod of row r's terms
    at i -- the numerator / denominator products of every product column of a proof in one launch (trh_product_terms_dev)"""
    flat = [t for row in rows for t in row]
    arr = (ProductTerm * len(flat))()
    for d, (x, y, c, g) in zip(arr, flat):
        d.x = _devptr(x)
        d.y = _devptr(y) if y is not None else None
        if c is not None:
            d.c[:] = [int(v) for v in c]
        d.g[:] = [int(v) for v in g]
    starts = (ctypes.c_uint32 * (len(rows) + 1))()
    acc = 0
    for i, row in enumerate(rows):
        starts[i] = acc
        acc += len(row)
    starts[len(rows)] = acc
    _check(lib().trh_product_terms_dev(FIELD_ID[field], ctypes.cast(arr, ctypes.c_void_p), starts, len(rows), n, _devptr(out_dev), stream))


def batch_invert_mul_dev(field: str, a_dev, num_dev, n: int, stream=None):
    """a[i] <- num[i] / a[i] in place (a zero denominator stays zero): ff::BatchInvert and the multiply that follows it, one pass"""
    _check(lib().trh_field_batch_invert_mul_dev(FIELD_ID[field], _devptr(a_dev), _devptr(num_dev), n, stream))


def prefix_product_dev(field: str, a_dev, out_dev, n: int, stream=None):
    """out[i] = prod_{j < i} a[j] (out[0] = 1): the running product of the permutation / lookup z columns"""
    _check(lib().trh_field_prefix_product_dev(FIELD_ID[field], _devptr(a_dev), _devptr(out_dev), n, stream))


# ---------------------------------------------------------------------------------------
# ff::Field::sqrt and GroupEncoding (the 32-byte compressed points): csrc/fieldsqrt.h, csrc/encoding.hip
# ---------------------------------------------------------------------------------------
def field_sqrt_dev(field: str, a_dev, out_dev, is_square_dev, n: int, stream=None):
    """out[i] = the root of a[i] with an even canonical value (0 for a non-square), is_square[i] = 1 / 0; device memory, n x 4 u64 and n x u8"""
    _check(lib().trh_field_sqrt_dev(FIELD_ID[field], _devptr(a_dev), _devptr(out_dev), _devptr(is_square_dev), n, stream))


def points_compress_dev(curve: str, xy_dev, bytes_dev, n: int, stream=None):
    """n x 64-byte affine PODs -> n x 32-byte encodings (pasta `to_bytes`), device memory"""
    _check(lib().trh_points_compress_dev(CURVE_ID[curve], _devptr(xy_dev), _devptr(bytes_dev), n, stream))


def points_decompress_dev(curve: str, bytes_dev, xy_dev, n: int, ok_dev=None, stream=None, first_bad: bool = True):
    """n x 32-byte encodings -> n x 64-byte affine PODs (pasta `from_bytes`; an invalid encoding: all-zero POD, ok[i] = 0).  Returns the
    smallest invalid index, n when there is none (synchronises the stream); with first_bad=False nothing is read back and None is returned"""
    fb = ctypes.c_uint64(0)
    _check(lib().trh_points_decompress_dev(CURVE_ID[curve], _devptr(bytes_dev), _devptr(xy_dev), None if ok_dev is None else _devptr(ok_dev), n, stream,
                                           ctypes.byref(fb) if first_bad else None))
    return int(fb.value) if first_bad else None


def point_to_bytes(curve: str, xyz) -> bytes:
    """a Jacobian point (12 limbs, any Z) -> its 32-byte encoding; host-side, no device needed"""
    p = _c(xyz).reshape(12)
    out = ctypes.create_string_buffer(32)
    _check(lib().trh_point_to_bytes(CURVE_ID[curve], _p(p), out))
    return out.raw


def point_from_bytes(curve: str, data: bytes) -> np.ndarray:
    """a 32-byte encoding -> the 8-limb affine POD (identity: all zero); TrhError on an invalid encoding; host-side, no device needed"""
    assert len(data) == 32
    out = np.zeros(8, dtype=np.uint64)
    _check(lib().trh_point_from_bytes(CURVE_ID[curve], ctypes.c_char_p(bytes(data)), _p(out)))
    return out


# ---------------------------------------------------------------------------------------
# hash_to_curve (Params::new): csrc/blake2b.h, csrc/hashtocurve.h, csrc/hashtocurve.hip
# ---------------------------------------------------------------------------------------
HALO2_PARAMS_PREFIX = "Halo2-Parameters"


def _prefix(prefix) -> bytes:
    """the NUL-terminated string the C ABI takes; the library itself refuses more than 128 bytes"""
    b = prefix.encode() if isinstance(prefix, str) else bytes(prefix)
    assert b"\0" not in b, "the prefix is a C string"
    return b


def hash_to_curve(curve: str, prefix, msg: bytes) -> np.ndarray:
    """pasta_curves `C::hash_to_curve(prefix)(msg)` for one message -> the 8-limb affine POD; host-side, no device needed"""
    msg = bytes(msg)
    out = np.zeros(8, dtype=np.uint64)
    _check(lib().trh_hash_to_curve(CURVE_ID[curve], _prefix(prefix), ctypes.c_char_p(msg) if msg else None, len(msg), _p(out)))
    return out


def hash_to_field_indexed_dev(curve: str, prefix, tag: int, first: int, n: int, u_dev, stream=None) -> None:
    """u_dev[i] = the two base-field elements of the message tag || le32(first + i), i < n: (n, 2, 4) limbs on the device"""
    _check(lib().trh_hash_to_field_indexed_dev(CURVE_ID[curve], _prefix(prefix), tag, first, n, _devptr(u_dev), stream))


def map_to_curve_dev(curve: str, u_dev, n: int, per_point: int, xy_dev, stream=None) -> None:
    """xy_dev[i] = iso_map(sum of swu(u_dev[i * per_point + j])), per_point 1 or 2: (n, 8) affine PODs on the device"""
    _check(lib().trh_map_to_curve_dev(CURVE_ID[curve], _devptr(u_dev), n, per_point, _devptr(xy_dev), stream))


def hash_to_curve_indexed_dev(curve: str, prefix, tag: int, first: int, n: int, xy_dev, stream=None) -> None:
    """xy_dev[i] = hash_to_curve(prefix)(tag || le32(first + i)), i < n -- g[first .. first + n) of Params::new for tag 0"""
    _check(lib().trh_hash_to_curve_indexed_dev(CURVE_ID[curve], _prefix(prefix), tag, first, n, _devptr(xy_dev), stream))


# ---------------------------------------------------------------------------------------
# the prover's random scalars from a ChaCha20 seed: csrc/chacha.h, csrc/random.hip
# ---------------------------------------------------------------------------------------
class Rng:
    """trh_rng_t: the stream of field elements a 32-byte seed expands to (element i = ChaCha20 block i through from_u512; include/trh.h),
    with ONE position shared by the host draws and the device fills.  The handle is host memory: no device is needed to make one or to
    draw from it on the host, and it may be used with any context."""

    def __init__(self, seed: bytes, stream_id: int = 0):
        seed = bytes(seed)
        assert len(seed) == 32
        self.handle = _vp()
        _check(lib().trh_rng_create(ctypes.c_char_p(seed), stream_id, ctypes.byref(self.handle)))

    def seek(self, block: int) -> None:
        _check(lib().trh_rng_seek(self.handle, block))

    def position(self) -> int:
        v = ctypes.c_uint64(0)
        _check(lib().trh_rng_position(self.handle, ctypes.byref(v)))
        return int(v.value)

    def next_scalar(self, field: str) -> np.ndarray:
        """one element on the host -> (4,) Montgomery limbs (a commitment's blind, the opening's round blinds)"""
        out = np.zeros(4, dtype=np.uint64)
        _check(lib().trh_rng_next_scalar(self.handle, FIELD_ID[field], _p(out)))
        return out

    def fill(self, field: str, out_dev, n: int, stream=None) -> None:
        """out[i] = the next n elements, written on the device (asynchronous on `stream`)"""
        _check(lib().trh_rng_fill_dev(self.handle, FIELD_ID[field], _devptr(out_dev), n, stream))

    def fill_rows(self, field: str, cols_dev, rows: int, row_len: int, first: int, count: int, stream=None) -> None:
        """cells [first, first + count) of each of `rows` columns of row_len elements (back to back) = the next rows * count elements in
        row-major order; every other cell is left as it is (the blinding rows of resident columns)"""
        _check(lib().trh_rng_fill_rows_dev(self.handle, FIELD_ID[field], _devptr(cols_dev), rows, row_len, first, count, stream))

    def destroy(self):
        if self.handle:
            lib().trh_rng_destroy(self.handle)
            self.handle = _vp()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def set_timing(on: bool):
    _check(lib().trh_set_timing(1 if on else 0))


def last_timing() -> dict:
    t = Timing()
    _check(lib().trh_last_timing(ctypes.byref(t)))
    return {k: getattr(t, k) for k, _ in Timing._fields_}


def set_window_bits(c: int):
    _check(lib().trh_msm_set_window_bits(c))


# ---------------------------------------------------------------------------------------
# device-resident bases + MSM
# ---------------------------------------------------------------------------------------
class Bases:
    """Device-resident affine base set (Params.g / Params.g_lagrange)."""

    def __init__(self, curve: str, handle):
        self.curve = curve
        self.handle = handle

    @classmethod
    def from_host(cls, curve: str, xy) -> "Bases":
        xy = _c(xy, 8)
        h = _vp()
        fn = lib().trh_bases_create_pallas if curve == "pallas" else lib().trh_bases_create_vesta
        _check(fn(_p(xy), xy.shape[0], ctypes.byref(h)))
        return cls(curve, h)

    @classmethod
    def from_compressed(cls, curve: str, data) -> "Bases":
        """n x 32-byte encodings in host memory (bytes, or a uint8 array) -> a resident set; the points are decoded on the device
        (trh_bases_create_compressed).  TrhError names the first invalid encoding."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        assert buf.size % 32 == 0
        h = _vp()
        _check(lib().trh_bases_create_compressed(CURVE_ID[curve], buf.ctypes.data_as(_vp), buf.size // 32, ctypes.byref(h)))
        return cls(curve, h)

    @classmethod
    def wrap_device(cls, curve: str, dev_ptr, n: int) -> "Bases":
        h = _vp()
        _check(lib().trh_bases_wrap_device(CURVE_ID[curve], _devptr(dev_ptr), n, ctypes.byref(h)))
        return cls(curve, h)

    @classmethod
    def generate(cls, curve: str, s0: int, d: int, n: int, first: int = 0) -> "Bases":
        h = _vp()
        _check(lib().trh_bases_generate(CURVE_ID[curve], s0, d, first, n, ctypes.byref(h)))
        return cls(curve, h)

    def __len__(self):
        return int(lib().trh_bases_len(self.handle))

    def shards(self) -> int:
        return int(lib().trh_bases_shards(self.handle))

    def precompute(self, window_bits: int = 0) -> int:
        """Attach the fixed-base table (2^(c j) P_i for all windows j); returns the window width used."""
        _check(lib().trh_bases_precompute(self.handle, window_bits))
        return int(lib().trh_bases_precomputed_window_bits(self.handle))

    def reserve(self, n: int, batch: int = 1) -> None:
        """trh_bases_reserve: sizes the calling context's MSM scratch for batches of `batch` MSMs over the first n bases, without running one"""
        _check(lib().trh_bases_reserve(self.handle, n, batch))

    def collapse_generators(self, k: int, u, stream=None):
        """trh_ipa_collapse_generators_dev: the first 2^k points after the r = len(u) collapses of an IPA opening, from this set's
        fixed-base table.  u: (r, 4) Montgomery challenges in round order.  Returns (xy, rec) on the host: (2^(k-r), 8) uint64 affine
        points and (2^(k-r), 32) uint32 records of the MSM's accumulation"""
        uu = _c(u, 4)
        r = uu.shape[0]
        m = 1 << max(int(k) - r, 0)
        d_xy, d_rec = DeviceBuffer(m * 64), DeviceBuffer(m * 128)
        try:
            _check(lib().trh_ipa_collapse_generators_dev(self.handle, k, r, _p(uu), d_xy.ptr, d_rec.ptr, stream))
            return d_xy.to_host(np.uint64, (m, 8)), d_rec.to_host(np.uint32, (m, 32))
        finally:
            d_xy.free()
            d_rec.free()

    def download(self, offset: int = 0, n: int | None = None) -> np.ndarray:
        n = len(self) - offset if n is None else n
        out = np.empty((n, 8), dtype=np.uint64)
        _check(lib().trh_bases_download(self.handle, offset, n, _p(out)))
        return out

    def download_compressed(self, offset: int = 0, n: int | None = None) -> bytes:
        """bases [offset, offset + n) as n x 32-byte encodings, encoded on the device (trh_bases_download_compressed)"""
        n = len(self) - offset if n is None else n
        out = np.empty(n * 32, dtype=np.uint8)
        _check(lib().trh_bases_download_compressed(self.handle, offset, n, out.ctypes.data_as(_vp)))
        return out.tobytes()

    def msm(self, scalars, offset: int = 0, montgomery: bool = True) -> np.ndarray:
        s = _c(scalars, 4)
        out = np.zeros(12, dtype=np.uint64)
        _check(lib().trh_msm(self.handle, offset, _p(s), s.shape[0], 1 if montgomery else 0, _p(out)))
        return out

    def msm_dev(self, scalars_dev, n: int, offset: int = 0, montgomery: bool = True, stream=None) -> np.ndarray:
        out = np.zeros(12, dtype=np.uint64)
        _check(lib().trh_msm_dev(self.handle, offset, _devptr(scalars_dev), n, 1 if montgomery else 0, stream, _p(out)))
        return out

    def msm_dev_enqueue(self, scalars_dev, n: int, offset: int = 0, montgomery: bool = True, stream=None):
        _check(lib().trh_msm_dev_enqueue(self.handle, offset, _devptr(scalars_dev), n, 1 if montgomery else 0, stream))

    def msm_dev_finish(self, stream=None) -> np.ndarray:
        out = np.zeros(12, dtype=np.uint64)
        _check(lib().trh_msm_dev_finish(self.handle, stream, _p(out)))
        return out

    def msm_batch_dev(self, scalars_dev, n: int, batch: int, offset: int = 0, montgomery: bool = True, stream=None) -> np.ndarray:
        out = np.zeros((batch, 12), dtype=np.uint64)
        _check(lib().trh_msm_batch_dev(self.handle, offset, _devptr(scalars_dev), n, batch, 1 if montgomery else 0, stream, _p(out)))
        return out

    def commit_batch_dev(self, polys_dev, n: int, batch: int, blinds, stream=None) -> np.ndarray:
        """Params::commit(_lagrange) of `batch` device polynomials: MSM of polys[b] || blinds[b] over the n + 1 bases"""
        out = np.zeros((batch, 12), dtype=np.uint64)
        bl = _c(blinds, 4)
        assert bl.shape[0] == batch
        _check(lib().trh_commit_batch_dev(self.handle, _devptr(polys_dev), n, batch, _p(bl), stream, _p(out)))
        return out

    def commit_batch_host(self, polys, blinds) -> np.ndarray:
        """Params::commit(_lagrange) of a list of HOST polynomials ((n, 4) uint64 each): columns go up in chunks under the MSMs"""
        n = polys[0].shape[0]
        for a in polys:
            assert a.dtype == np.uint64 and a.flags.c_contiguous and a.shape == (n, 4)
        out = np.zeros((len(polys), 12), dtype=np.uint64)
        bl = _c(blinds, 4)
        assert bl.shape[0] == len(polys)
        _check(lib().trh_commit_batch_host(self.handle, _ptr_array(polys), n, len(polys), _p(bl), _p(out)))
        return out

    def destroy(self):
        if self.handle:
            lib().trh_bases_destroy(self.handle)
            self.handle = _vp()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
