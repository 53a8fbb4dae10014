"""ctypes binding of ``liblsa_hip.so`` (declared in ``include/lsa_hip.h``).

This is the thin host layer the SLEPc-shaped API in ``Solver/eigen.py`` sits on.  There is no CPU fallback:
importing works anywhere (so the symbol table can be checked without a GPU), but creating a
:class:`Context` raises ``RuntimeError`` when the library or a GPU is missing.
"""

from __future__ import annotations

import ctypes
import os
import re
from pathlib import Path

import numpy as np

LSA_F64, LSA_C128 = 0, 1

_STATUS_NAMES = {
    0: "LSA_OK",
    -1: "LSA_ERR_ARG",
    -2: "LSA_ERR_HIP",
    -3: "LSA_ERR_ZERO_PIVOT",
    -4: "LSA_ERR_DIVERGED",
    -5: "LSA_ERR_NONFINITE",
    -6: "LSA_ERR_TIMEOUT",
    -7: "LSA_ERR_COMM",
    -8: "LSA_ERR_OOM",
}

# the status codes of include/lsa_hip.h by name (LSA_OK, LSA_ERR_ARG, ... LSA_ERR_OOM)
globals().update({name: code for code, name in _STATUS_NAMES.items()})

LIB_PATH = Path(os.environ.get("LSA_HIP_LIB", Path(__file__).resolve().parent / "liblsa_hip.so"))


class LsaError(RuntimeError):
    """A device-side or numerical failure reported by the library (status < -1)."""

    def __init__(self, status: int, message: str):
        super().__init__(f"{_STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


class lsa_stats(ctypes.Structure):
    _fields_ = [
        ("op_applies", ctypes.c_int64),
        ("gmres_iters", ctypes.c_int64),
        ("spmv_calls", ctypes.c_int64),
        ("sptrsv_calls", ctypes.c_int64),
        ("last_rel_res", ctypes.c_double),
        ("max_rel_res", ctypes.c_double),
        ("seconds_factor", ctypes.c_double),
        ("seconds_solve", ctypes.c_double),
        ("stagnated_solves", ctypes.c_int32),
        ("pc_fallback", ctypes.c_int32),
        ("backward_accepted", ctypes.c_int32),
        ("analysis_reused", ctypes.c_int32),
        ("refined_solves", ctypes.c_int32),
        ("reserved0", ctypes.c_int32),
    ]


class lsa_op_options(ctypes.Structure):
    _fields_ = [
        ("ilu_levels", ctypes.c_int32),
        ("ilu_shift", ctypes.c_double),
        ("ksp_rtol", ctypes.c_double),
        ("ksp_restart", ctypes.c_int32),
        ("ksp_maxit", ctypes.c_int32),
        ("pc_type", ctypes.c_int32),
        ("antishift", ctypes.c_double * 2),
    ]


class lsa_ks_options(ctypes.Structure):
    _fields_ = [
        ("nev", ctypes.c_int32),
        ("max_restarts", ctypes.c_int32),
        ("tol", ctypes.c_double),
        ("which", ctypes.c_int32),
        ("transform", ctypes.c_int32),
        ("sigma", ctypes.c_double * 2),
        ("antishift", ctypes.c_double * 2),
        ("target", ctypes.c_double * 2),
        ("seed", ctypes.c_uint64),
        ("keep_fraction", ctypes.c_double),
    ]


class lsa_ks_result(ctypes.Structure):
    _fields_ = [
        ("nconv", ctypes.c_int32),
        ("nout", ctypes.c_int32),
        ("restarts", ctypes.c_int32),
        ("pad", ctypes.c_int32),
        ("op_applies", ctypes.c_int64),
        ("next_unconverged", ctypes.c_double),
        ("seconds_expand", ctypes.c_double),
        ("seconds_dense", ctypes.c_double),
        ("seconds_restart", ctypes.c_double),
    ]


class lsa_ks_batch_info(ctypes.Structure):
    _fields_ = [
        ("rounds", ctypes.c_int64),
        ("launches", ctypes.c_int64),
        ("periods", ctypes.c_int64),
        ("launches_per_round", ctypes.c_double),
        ("lockstep_steps", ctypes.c_int64 * 16),
        ("solo_steps", ctypes.c_int64 * 16),
    ]


class lsa_contour_result(ctypes.Structure):
    _fields_ = [
        ("iterations", ctypes.c_int32),
        ("rank", ctypes.c_int32),
        ("inside", ctypes.c_int32),
        ("converged_inside", ctypes.c_int32),
        ("complete", ctypes.c_int32),
        ("nout", ctypes.c_int32),
        ("estimate", ctypes.c_double),
        ("block_solves", ctypes.c_int64),
        ("refined_solves", ctypes.c_int64),
        ("backward_accepted", ctypes.c_int64),
        ("worst_rel_res", ctypes.c_double),
    ]


class lsa_contour_stats(ctypes.Structure):
    _fields_ = [
        ("kept", ctypes.c_int32),
        ("nodes", ctypes.c_int32),
        ("bytes", ctypes.c_int64),
        ("seconds_factor", ctypes.c_double),
        ("seconds_solve", ctypes.c_double),
        ("seconds_product", ctypes.c_double),
        ("seconds_gram", ctypes.c_double),
        ("seconds_dense", ctypes.c_double),
        ("solver", lsa_stats),
    ]


class lsa_contour_left_stats(ctypes.Structure):
    _fields_ = [
        ("solves", ctypes.c_int32),
        ("iterations", ctypes.c_int32),
        ("block_solves", ctypes.c_int64),
        ("refined_solves", ctypes.c_int64),
        ("backward_accepted", ctypes.c_int64),
        ("groups", ctypes.c_int64),
        ("batched_columns", ctypes.c_int64),
        ("serial_columns", ctypes.c_int64),
        ("seconds_factor", ctypes.c_double),
        ("seconds_solve", ctypes.c_double),
        ("seconds_product", ctypes.c_double),
        ("seconds_gram", ctypes.c_double),
        ("seconds_dense", ctypes.c_double),
    ]


class lsa_contour_batch_stats(ctypes.Structure):
    _fields_ = [
        ("enabled", ctypes.c_int32),
        ("pad0", ctypes.c_int32),
        ("groups", ctypes.c_int64),
        ("batched_columns", ctypes.c_int64),
        ("serial_columns", ctypes.c_int64),
    ]


class lsa_stochastic_stats(ctypes.Structure):
    _fields_ = [
        ("nodes", ctypes.c_int32),
        ("kind", ctypes.c_int32),
        ("bytes", ctypes.c_int64),
        ("seconds_factor", ctypes.c_double),
        ("seconds_solve", ctypes.c_double),
        ("seconds_product", ctypes.c_double),
        ("seconds_dense", ctypes.c_double),
        ("solver", lsa_stats),
        ("batch_adjoint", ctypes.c_int32),
        ("adjoint_batches", ctypes.c_int64),
        ("forward_batches", ctypes.c_int64),
        ("seconds_solve_adjoint", ctypes.c_double),
        ("seconds_product_adjoint", ctypes.c_double),
    ]


class lsa_stochastic_trace_stats(ctypes.Structure):
    _fields_ = [
        ("solves_adjoint", ctypes.c_int64),
        ("solves_forward", ctypes.c_int64),
        ("refined_solves", ctypes.c_int64),
        ("batches", ctypes.c_int64),
        ("grouped_sweeps", ctypes.c_int64),
        ("widest_pass", ctypes.c_int32),
        ("batch", ctypes.c_int32),
        ("seconds_solve", ctypes.c_double),
        ("seconds_product", ctypes.c_double),
        ("seconds_forms", ctypes.c_double),
        ("bytes", ctypes.c_int64),
    ]


_P = ctypes.c_void_p
_I32, _I64, _DBL = ctypes.c_int32, ctypes.c_int64, ctypes.c_double
_PP = ctypes.POINTER(ctypes.c_void_p)

# name -> (restype, argtypes); kept in step with include/lsa_hip.h (tests/test_abi.py checks both directions)
SIGNATURES = {
    "lsa_ctx_create": (ctypes.c_int, [ctypes.c_int, _PP]),
    "lsa_ctx_destroy": (None, [_P]),
    "lsa_last_error": (ctypes.c_char_p, [_P]),
    "lsa_ctx_synchronize": (ctypes.c_int, [_P]),
    "lsa_ctx_mem_info": (ctypes.c_int, [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "lsa_ctx_arch": (ctypes.c_char_p, [_P]),
    "lsa_vec_create": (ctypes.c_int, [_P, _I64, ctypes.c_int, _PP]),
    "lsa_vec_destroy": (None, [_P]),
    "lsa_vec_upload": (ctypes.c_int, [_P, _P, _P]),
    "lsa_vec_download": (ctypes.c_int, [_P, _P, _P]),
    "lsa_csr_upload": (ctypes.c_int, [_P, _I32, _I64, _P, _P, _P, ctypes.c_int, _PP]),
    "lsa_mat_destroy": (None, [_P]),
    "lsa_mat_download_values": (ctypes.c_int, [_P, _P, _P]),
    "lsa_csr_axpby": (ctypes.c_int, [_P, _P, _P, _DBL * 2, _DBL * 2, ctypes.c_int, _PP]),
    "lsa_csr_window": (ctypes.c_int, [_P, _P, _P, _P, _PP]),
    "lsa_spmv": (ctypes.c_int, [_P, _P, _P, _P]),
    "lsa_spmv_transpose": (ctypes.c_int, [_P, _P, ctypes.c_int, _P, _P]),
    "lsa_spmv_transpose_batch": (ctypes.c_int, [_P, _I32, _PP, ctypes.c_int, _PP, _PP]),
    "lsa_spmv_batch": (ctypes.c_int, [_P, _I32, _PP, _PP, _PP]),
    "lsa_spmv_info": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_char_p, _I32, ctypes.POINTER(_I64)]),
    "lsa_spmv_time": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_int, ctypes.POINTER(_DBL)]),
    "lsa_ilu_create": (ctypes.c_int, [_P, _P, ctypes.c_int, _DBL, _PP]),
    "lsa_ilu_destroy": (None, [_P]),
    "lsa_ilu_set_algorithm": (ctypes.c_int, [_P, _P, ctypes.c_int, _I32]),
    "lsa_ilu_solve": (ctypes.c_int, [_P, _P, ctypes.c_int, _P, _P]),
    "lsa_ilu_solve_time": (ctypes.c_int, [_P, _P, ctypes.c_int, _P, _P, ctypes.c_int, ctypes.POINTER(_DBL)]),
    "lsa_ilu_info": (ctypes.c_int, [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I32), ctypes.POINTER(_I32), ctypes.POINTER(_I32)]),
    "lsa_ilu_download": (ctypes.c_int, [_P, _P, _P, _P, _P]),
    "lsa_nd_analyse": (ctypes.c_int, [_I32, _P, _P, _I32, _P, _PP]),
    "lsa_nd_order": (ctypes.c_int, [_I32, _P, _P, _I32, _P, _PP]),
    "lsa_nd_analyse_tree": (ctypes.c_int, [_I32, _P, _P, _I32, _P, _P, _P, _P, _I32, _I32, _PP]),
    "lsa_nd_sym_export_dist": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "lsa_nd_sym_export_top": (ctypes.c_int, [_P, _P, _P, _P, _P]),
    "lsa_ndlu_inertia": (ctypes.c_int, [_P, _P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "lsa_dense_sym_inertia": (ctypes.c_int, [_I32, _P, _I32, _DBL, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "lsa_nd_sym_error": (ctypes.c_char_p, [_P]),
    "lsa_nd_sym_destroy": (None, [_P]),
    "lsa_nd_sym_info": (ctypes.c_int, [_P, ctypes.POINTER(_I32), ctypes.POINTER(_I32), ctypes.POINTER(_I32), ctypes.POINTER(_I64),
                                       ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_DBL)]),
    "lsa_nd_sym_export": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "lsa_nd_sym_memory": (ctypes.c_int, [_P, _I32, _I64, _P, _P, _P, _P]),
    "lsa_nd_sym_export_tables": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "lsa_ndlu_create": (ctypes.c_int, [_P, _P, _I32, _PP]),
    "lsa_ndlu_prepare": (ctypes.c_int, [_P, _P, ctypes.c_int, _I32, _P]),
    "lsa_ndlu_prepare_tree": (ctypes.c_int, [_P, _P, ctypes.c_int, _I32, _P, _P, _P]),
    "lsa_ndlu_create_tree": (ctypes.c_int, [_P, _P, _I32, _P, _P, _P, _P, _PP]),
    "lsa_ndlu_refactor": (ctypes.c_int, [_P, _P, _P]),
    "lsa_ndlu_destroy": (None, [_P]),
    "lsa_ndlu_solve": (ctypes.c_int, [_P, _P, _P, _P]),
    "lsa_ndlu_solve_batch": (ctypes.c_int, [_P, _I32, _PP, _PP, _PP]),
    "lsa_ndlu_solve_batch_adjoint": (ctypes.c_int, [_P, _I32, _PP, ctypes.c_int, _PP, _PP]),
    "lsa_ndlu_prepared_memory": (ctypes.c_int, [_P, _P]),
    "lsa_ndlu_solve_adjoint": (ctypes.c_int, [_P, _P, ctypes.c_int, _P, _P]),
    "lsa_ndlu_solve_time": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_int, ctypes.POINTER(_DBL)]),
    "lsa_ndlu_solve_multi": (ctypes.c_int, [_P, _P, ctypes.c_int, _I32, _P, _I64, _P, _I64]),
    "lsa_ndlu_solve_multi_time": (ctypes.c_int, [_P, _P, ctypes.c_int, _I32, _P, _I64, _P, _I64, ctypes.c_int, ctypes.POINTER(_DBL)]),
    "lsa_ndlu_solve_multi_batch": (ctypes.c_int, [_P, _I32, _PP, ctypes.c_int, _I32, _PP, _I64, _PP, _I64]),
    "lsa_ndlu_solve_multi_batch_time": (ctypes.c_int, [_P, _I32, _PP, ctypes.c_int, _I32, _PP, _I64, _PP, _I64, ctypes.c_int, ctypes.POINTER(_DBL)]),
    "lsa_ndlu_solve_multi_batch_adjoint": (ctypes.c_int, [_P, _I32, _PP, ctypes.c_int, _I32, _PP, _I64, _PP, _I64]),
    "lsa_ndlu_solve_multi_batch_adjoint_time": (ctypes.c_int, [_P, _I32, _PP, ctypes.c_int, _I32, _PP, _I64, _PP, _I64, ctypes.c_int, ctypes.POINTER(_DBL)]),
    "lsa_ndlu_set_multi_transposed": (ctypes.c_int, [_P, _P, ctypes.c_int]),
    "lsa_ndlu_multi_info": (ctypes.c_int, [_P, ctypes.POINTER(_I32), ctypes.POINTER(_I64), ctypes.POINTER(_I32)]),
    "lsa_ndlu_info": (ctypes.c_int, [_P, ctypes.POINTER(_I32), ctypes.POINTER(_I32), ctypes.POINTER(_I32), ctypes.POINTER(_I64),
                                     ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I32), ctypes.POINTER(_DBL), ctypes.POINTER(_DBL),
                                     ctypes.POINTER(_I32)]),
    "lsa_ndlu_sweep_level": (ctypes.c_int, [_P, _I32] + [ctypes.POINTER(_I32)] * 6),
    "lsa_gmres": (ctypes.c_int, [_P, _P, _P, _P, _P, ctypes.c_int, _DBL, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_I32), ctypes.POINTER(_DBL)]),
    "lsa_op_create": (ctypes.c_int, [_P, _P, _P, _DBL * 2, ctypes.c_int, ctypes.POINTER(lsa_op_options), _PP]),
    "lsa_op_create_sharded": (ctypes.c_int, [_P, _P, _P, _P, _P, _DBL * 2, ctypes.c_int, ctypes.POINTER(lsa_op_options), _PP]),
    "lsa_op_create_dist": (ctypes.c_int, [_P, _P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _DBL * 2, ctypes.c_int, ctypes.POINTER(lsa_op_options), _PP]),
    "lsa_op_destroy": (None, [_P]),
    "lsa_op_apply": (ctypes.c_int, [_P, _P, _P, _P]),
    "lsa_op_stats": (ctypes.c_int, [_P, ctypes.POINTER(lsa_stats)]),
    "lsa_op_set_adjoint": (ctypes.c_int, [_P, _P, ctypes.c_int]),
    "lsa_op_set_projection": (ctypes.c_int, [_P, _P, _P]),
    "lsa_krylov_create": (ctypes.c_int, [_P, _P, _I32, _PP]),
    "lsa_krylov_destroy": (None, [_P]),
    "lsa_krylov_set_row_permutation": (ctypes.c_int, [_P, _P, _P]),
    "lsa_krylov_set_start": (ctypes.c_int, [_P, _P, _P]),
    "lsa_krylov_inject": (ctypes.c_int, [_P, _P, _I32, _P]),
    "lsa_krylov_extend": (ctypes.c_int, [_P, _P, _I32, _I32, _P, _I32, ctypes.POINTER(_I32)]),
    "lsa_krylov_restart": (ctypes.c_int, [_P, _P, _I32, _I32, _P, _I32]),
    "lsa_krylov_ritz_vectors": (ctypes.c_int, [_P, _P, _I32, _I32, _P, _I32, ctypes.c_int, _P]),
    "lsa_krylov_imag_norms": (ctypes.c_int, [_P, _I32, _P]),
    "lsa_krylov_shape": (ctypes.c_int, [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I32)]),
    "lsa_mat_rows": (_I64, [_P]),
    "lsa_krylov_solve": (ctypes.c_int, [_P, _P, _P, _P, _P, _I32, _P, _P, _P, _P, _P]),
    "lsa_krylov_solve_batch": (ctypes.c_int, [_P, _I32, _PP, _PP, _PP, _I32, _PP, _PP, _PP, _PP, _P, _P, _P]),
    "lsa_eigs_sinvert": (ctypes.c_int, [_P, _P, _P, _DBL * 2, _I32, _I32, _DBL, _I32, ctypes.POINTER(lsa_op_options), _P, _P, _I32, _P, _P, _P, _P, _P]),
    "lsa_dense_schur": (ctypes.c_int, [_I32, _P, _I32, _P, _I32]),
    "lsa_dense_schur_reorder": (ctypes.c_int, [_I32, _P, _I32, _P, _I32, _P, ctypes.POINTER(_I32)]),
    "lsa_dense_tri_eigenvectors": (ctypes.c_int, [_I32, _P, _I32, _P, _I32]),
    "lsa_eig_residuals": (ctypes.c_int, [_P, _P, _P, _I32, _P, _P, _P]),
    "lsa_eig_biorth": (ctypes.c_int, [_P, _P, _I64, _I32, _P, _P, _P, _P, _P]),
    "lsa_lanczos_create": (ctypes.c_int, [_P, _P, _I32, _PP]),
    "lsa_lanczos_destroy": (None, [_P]),
    "lsa_lanczos_set_row_permutation": (ctypes.c_int, [_P, _P, _P]),
    "lsa_lanczos_set_start": (ctypes.c_int, [_P, _P, _P]),
    "lsa_lanczos_extend": (ctypes.c_int, [_P, _P, _I32, _I32, _P, _I32, ctypes.POINTER(_I32)]),
    "lsa_lanczos_basis": (ctypes.c_int, [_P, _P, _I32, _P]),
    "lsa_lanczos_solve": (ctypes.c_int, [_P, _P, ctypes.POINTER(lsa_ks_options), _P, _I32, _P, _P, _P, _P, ctypes.POINTER(lsa_ks_result)]),
    "lsa_dense_syev": (ctypes.c_int, [_I32, _P, _I32, _P]),
    "lsa_resolvent_create": (ctypes.c_int, [_P, _P, _I32, _PP]),
    "lsa_resolvent_destroy": (None, [_P]),
    "lsa_resolvent_set_row_permutation": (ctypes.c_int, [_P, _P, _P]),
    "lsa_resolvent_set_block_forcings": (ctypes.c_int, [_P, _P, ctypes.c_int]),
    "lsa_resolvent_set_weights": (ctypes.c_int, [_P, _P, _P, _P]),
    "lsa_resolvent_set_start": (ctypes.c_int, [_P, _P, _P]),
    "lsa_resolvent_extend": (ctypes.c_int, [_P, _P, _I32, _I32, _P, _I32, ctypes.POINTER(_I32)]),
    "lsa_resolvent_basis": (ctypes.c_int, [_P, _P, _I32, _P]),
    "lsa_resolvent_solve": (ctypes.c_int, [_P, _P, ctypes.POINTER(lsa_ks_options), _P, _I32, _P, _P, _P, _P, _P, ctypes.POINTER(lsa_ks_result), _P]),
    "lsa_resolvent_extend_batch": (ctypes.c_int, [_P, _I32, _PP, _P, _P, _I32, _PP, _I32, _P, _P]),
    "lsa_resolvent_solve_batch": (ctypes.c_int, [_P, _I32, _PP, _PP, _PP, _I32, _PP, _PP, _PP, _PP, _PP, _P, _P, _P, _P]),
    "lsa_growth_create": (ctypes.c_int, [_P, _P, _I32, _I32, _P, _PP]),
    "lsa_growth_destroy": (None, [_P]),
    "lsa_growth_set_row_permutation": (ctypes.c_int, [_P, _P, _P]),
    "lsa_growth_set_steps": (ctypes.c_int, [_P, _P, _I32]),
    "lsa_growth_set_scheme": (ctypes.c_int, [_P, _P, _I32]),
    "lsa_growth_set_response_weight": (ctypes.c_int, [_P, _P, _P]),
    "lsa_growth_response_energy": (ctypes.c_int, [_P, _P, _I32, _P]),
    "lsa_growth_set_start": (ctypes.c_int, [_P, _P, _P]),
    "lsa_growth_extend": (ctypes.c_int, [_P, _P, _I32, _I32, _P, _I32, ctypes.POINTER(_I32)]),
    "lsa_growth_basis": (ctypes.c_int, [_P, _P, _I32, _P]),
    "lsa_growth_solve": (ctypes.c_int, [_P, _P, ctypes.POINTER(lsa_ks_options), _P, _I32, _P, _P, _P, _P, _P, _P, ctypes.POINTER(lsa_ks_result), _P]),
    "lsa_spmm": (ctypes.c_int, [_P, _P, _I32, _P, _I64, _P, _I64]),
    "lsa_spmm_transpose": (ctypes.c_int, [_P, _P, ctypes.c_int, _I32, _P, _I64, _P, _I64]),
    "lsa_block_gram": (ctypes.c_int, [_P, _I64, _I32, _P, _I64, _I32, _P, _I64, _P]),
    "lsa_contour_create": (ctypes.c_int, [_P, _P, _P, _I32, _DBL * 2, _DBL * 2, _I32, ctypes.c_int, _DBL, _PP]),
    "lsa_contour_destroy": (None, [_P]),
    "lsa_contour_set_row_permutation": (ctypes.c_int, [_P, _P, _P]),
    "lsa_contour_solve": (ctypes.c_int, [_P, _P, _DBL, _I32, _P, _I32, _P, _P, _P, ctypes.POINTER(lsa_contour_result)]),
    "lsa_contour_info": (ctypes.c_int, [_P, ctypes.POINTER(lsa_contour_stats)]),
    "lsa_contour_set_batch_nodes": (ctypes.c_int, [_P, _P, ctypes.c_int]),
    "lsa_contour_batch_info": (ctypes.c_int, [_P, ctypes.POINTER(lsa_contour_batch_stats)]),
    "lsa_contour_solve_left": (ctypes.c_int, [_P, _P, _DBL, _I32, _P, _I32, _P, _P, _P, ctypes.POINTER(lsa_contour_result)]),
    "lsa_contour_left_info": (ctypes.c_int, [_P, ctypes.POINTER(lsa_contour_left_stats)]),
    "lsa_shifted_spmm": (ctypes.c_int, [_P, _P, _P, _I32, _P, _P, _P]),
    "lsa_shifted_spmm_transpose": (ctypes.c_int, [_P, _P, _P, _I32, _P, _P, _P]),
    "lsa_stochastic_create": (ctypes.c_int, [_P, _P, _P, _I32, _P, _P, _I32, _DBL, _PP]),
    "lsa_stochastic_destroy": (None, [_P]),
    "lsa_stochastic_set_row_permutation": (ctypes.c_int, [_P, _P, _P]),
    "lsa_stochastic_set_weights": (ctypes.c_int, [_P, _P, _P, _P]),
    "lsa_stochastic_set_kind": (ctypes.c_int, [_P, _P, _I32]),
    "lsa_stochastic_set_batch_forward": (ctypes.c_int, [_P, _P, ctypes.c_int]),
    "lsa_stochastic_set_batch_adjoint": (ctypes.c_int, [_P, _P, ctypes.c_int]),
    "lsa_stochastic_set_refinement": (ctypes.c_int, [_P, _P, ctypes.c_int]),
    "lsa_stochastic_apply": (ctypes.c_int, [_P, _P, _P, _P, _P]),
    "lsa_stochastic_solve": (ctypes.c_int, [_P, _P, ctypes.POINTER(lsa_ks_options), _P, _I32, _P, _P, _P, ctypes.POINTER(lsa_ks_result), _P]),
    "lsa_stochastic_info": (ctypes.c_int, [_P, ctypes.POINTER(lsa_stochastic_stats)]),
    "lsa_stochastic_trace": (ctypes.c_int, [_P, _P, _I32, ctypes.c_uint64, _P, _I32, _P, _I32, _P, _P, ctypes.POINTER(lsa_stochastic_trace_stats)]),
    "lsa_stochastic_probes": (ctypes.c_int, [_P, _P, _I32, ctypes.c_uint64, _P]),
    "lsa_mm_open": (ctypes.c_int, [ctypes.c_char_p, _PP, ctypes.POINTER(_I32), ctypes.POINTER(_I32), ctypes.POINTER(_I64), ctypes.POINTER(ctypes.c_int)]),
    "lsa_mm_read_csr": (ctypes.c_int, [_P, _P, _P, _P]),
    "lsa_mm_error": (ctypes.c_char_p, [_P]),
    "lsa_mm_close": (None, [_P]),
    "lsa_comm_unique_id": (ctypes.c_int, [_P]),
    "lsa_comm_init": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P]),
    "lsa_comm_init_host": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P, _P]),
    "lsa_comm_stats": (ctypes.c_int, [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "lsa_comm_selftest": (ctypes.c_int, [_P, _I64]),
    "lsa_csr_upload_shard": (ctypes.c_int, [_P, _I32, _I32, _I32, _I64, _P, _P, _P, ctypes.c_int, _PP]),
}

_HOST_GATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p)
_lib = None


def load_library() -> ctypes.CDLL:
    """dlopen liblsa_hip.so and attach the signatures; raises RuntimeError (never falls back) if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `make -C lsa-fw_amd/csrc` (or __graft_entry__.build()). "
            "There is no CPU fallback for the eigen path."
        )
    lib = ctypes.CDLL(str(LIB_PATH))
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here means the header and the library disagree
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def _dtype_code(dt) -> int:
    dt = np.dtype(dt)
    if dt == np.float64:
        return LSA_F64
    if dt == np.complex128:
        return LSA_C128
    raise ValueError(f"unsupported dtype {dt}: use float64 or complex128")


def _np_dtype(code: int):
    return np.complex128 if code == LSA_C128 else np.float64


_host_blas_limit = None


def _calm_host_blas() -> None:
    """Opt-in (``LSA_HOST_BLAS_THREADS=<n>``): pin the host BLAS pools to ``n`` threads for the life of the process.

    The GPU path is a chain of dependent launches and leans on the HIP runtime's helper thread.  numpy's OpenBLAS workers
    spin for ~0.1 s after any threaded call; on a 16-core share of a GPU node 64 of them starve that thread and the next
    factorisation is 1.3-2x slower (``tools/micro/after_solve.py``).  A library must not change its caller's thread pools
    behind its back, so nothing happens unless the variable is set (``bench.py`` and the examples set it to 1); the dense
    80 x 80 algebra of the Krylov-Schur driver limits the pools only for the duration of its own LAPACK calls."""
    global _host_blas_limit
    want = os.environ.get("LSA_HOST_BLAS_THREADS", "keep")
    if _host_blas_limit is not None or want == "keep":
        return
    try:
        from threadpoolctl import threadpool_limits

        _host_blas_limit = threadpool_limits(limits=max(1, int(want)), user_api="blas")
    except Exception:  # threadpoolctl missing or an unknown BLAS: the path still works, only slower under oversubscription
        _host_blas_limit = False


class Context:
    """One GPU + one HIP stream.  Not thread-safe (mirrors the single blocking ``eps.solve()`` of the reference)."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        _calm_host_blas()
        h = ctypes.c_void_p()
        rc = self._lib.lsa_ctx_create(int(device), ctypes.byref(h))
        if rc != 0:
            raise RuntimeError(
                f"lsa_ctx_create(device={device}) failed with {_STATUS_NAMES.get(rc, rc)}: no usable AMD GPU. "
                "The eigen path has no CPU fallback."
            )
        self.handle = h
        self.device = device

    @property
    def arch(self) -> str:
        return self._lib.lsa_ctx_arch(self.handle).decode()

    def check(self, rc: int) -> None:
        if rc == 0:
            return
        msg = self._lib.lsa_last_error(self.handle).decode(errors="replace")
        if rc == -1:
            raise ValueError(msg)
        raise LsaError(rc, msg)

    def synchronize(self) -> None:
        self.check(self._lib.lsa_ctx_synchronize(self.handle))

    def prepared_lu_bytes(self) -> int:
        """Device bytes the next factorisation on the analysis this context holds prepared allocates (``lsa_ndlu_prepared_memory``:
        the memory plan of ``lsa_nd_sym_memory`` -- factors, working and update arenas, sweep buffers, index tables)."""
        out = np.zeros(8, np.int64)
        self.check(self._lib.lsa_ndlu_prepared_memory(self.handle, _ptr(out)))
        return int(out[0] + out[1] + out[2] + out[4] + out[7])

    def mem_info(self) -> tuple[int, int]:
        """``(free, total)`` bytes of the device memory right now."""
        free, total = _I64(0), _I64(0)
        self.check(self._lib.lsa_ctx_mem_info(self.handle, ctypes.byref(free), ctypes.byref(total)))
        return int(free.value), int(total.value)

    def close(self) -> None:
        if getattr(self, "handle", None):
            self._lib.lsa_ctx_destroy(self.handle)
            self.handle = None

    # multi-GPU bootstrap -------------------------------------------------------------------------------
    def unique_id(self) -> bytes:
        buf = ctypes.create_string_buffer(128)
        rc = self._lib.lsa_comm_unique_id(buf)
        if rc != 0:
            raise LsaError(rc, "RCCL unavailable")
        return buf.raw

    def comm_init(self, nranks: int, rank: int, uid: bytes) -> None:
        buf = ctypes.create_string_buffer(uid, 128)
        self.check(self._lib.lsa_comm_init(self.handle, nranks, rank, buf))

    def comm_init_host(self, nranks: int, rank: int, exchange) -> None:
        """Host-staged all-gather: ``exchange(buffer)`` receives a writable uint8 numpy view of ``nranks`` equal blocks with
        this rank's block filled in and must fill the others (``lsa_comm_init_host``)."""

        def _cb(host_buf, bytes_per_rank, _user):
            try:
                view = np.ctypeslib.as_array((ctypes.c_uint8 * (int(bytes_per_rank) * nranks)).from_address(host_buf))
                exchange(view.reshape(nranks, int(bytes_per_rank)))
                return 0
            except Exception:  # noqa: BLE001  (must not propagate through the C frame)
                import traceback

                traceback.print_exc()
                return 1

        self._host_cb = _HOST_GATHER_FN(_cb)  # keep the trampoline alive as long as the context
        self.check(self._lib.lsa_comm_init_host(self.handle, nranks, rank, ctypes.cast(self._host_cb, ctypes.c_void_p), None))

    def comm_selftest(self, nbytes: int = 1 << 20) -> None:
        """RCCL with one rank on this device: open, unique id, communicator, one in-place all-gather, destroy (raises on failure)."""
        self.check(self._lib.lsa_comm_selftest(self.handle, int(nbytes)))

    def comm_stats(self) -> dict:
        calls, nbytes = _I64(0), _I64(0)
        self._lib.lsa_comm_stats(self.handle, ctypes.byref(calls), ctypes.byref(nbytes))
        return {"allgather_calls": calls.value, "allgather_bytes_received": nbytes.value}


class _Handle:
    """An object of the library in a context ``self.ctx``: ``self.handle`` from ``lsa_<_prefix>_create`` (or a like entry), given back
    to ``lsa_<_prefix>_destroy`` once, while the context lives.  An object whose constructor raised before the handle existed calls
    nothing."""

    _prefix = ""

    def _call(self, entry: str, *args) -> None:
        """``lsa_<_prefix>_<entry>(ctx, handle, *args)``, checked."""
        self.ctx.check(getattr(self.ctx._lib, f"lsa_{self._prefix}_{entry}")(self.ctx.handle, self.handle, *args))

    def __del__(self):
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            getattr(self.ctx._lib, f"lsa_{self._prefix}_destroy")(self.handle)
            self.handle = None


def _ks_options(nev, tol, max_restarts, which=0, transform=0, sigma=0.0, antishift=0.0, target=None, seed=0) -> lsa_ks_options:
    """The options of a library loop (``target=None``: the shift).  The Lanczos-type loops on an operator of their own leave
    ``which``, ``transform`` and the three complex fields at zero."""
    pair = lambda z: (_DBL * 2)(complex(z).real, complex(z).imag)  # noqa: E731
    return lsa_ks_options(nev=int(nev), max_restarts=int(max_restarts), tol=float(tol), which=int(which), transform=int(transform), sigma=pair(sigma),
                          antishift=pair(antishift), target=pair(sigma if target is None else target), seed=int(seed), keep_fraction=0.5)


class _LanczosHandle(_Handle):
    """A handle that runs the library's restarted Lanczos loop (``lsa_lanczos_*`` itself, or a handle that owns one and brings the
    operator): ``n`` rows, ``ncv`` columns, scalars of ``_dtype``.  :meth:`_set_start`, :meth:`_extend` and :meth:`_basis` are
    published (as ``set_start``, ``extend``, ``basis``) by the classes whose C API has these entries."""

    _dtype = np.float64
    _counters: tuple = ()  # the names of the four solve counters ``lsa_<_prefix>_solve`` fills, in its order (none: it has no such argument)
    _has_perm = False

    @property
    def basis_bytes(self) -> int:
        """Device bytes of the ``n x (ncv + 1)`` arrays of the iteration: the basis, the restart's second basis and, with a row
        permutation, the output vectors in the caller's numbering."""
        return np.dtype(self._dtype).itemsize * self.n * (self.ncv + 1) * (3 if self._has_perm else 2)

    def set_row_permutation(self, perm: np.ndarray | None) -> None:
        """``perm[i]`` = the caller's index of basis row ``i``: the vectors of :meth:`solve` come back in the caller's numbering."""
        p = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
        self._call("set_row_permutation", None if p is None else _ptr(p))
        self._has_perm = p is not None

    def _start(self, v) -> np.ndarray:
        return _start_vector(v, self.n, self._dtype)

    def _set_start(self, v: np.ndarray) -> None:
        self._call("set_start", _ptr(self._start(v)))

    def _extend(self, j0: int, j1: int, T: np.ndarray) -> int:
        """Steps j0..j1-1 of the iteration writing ``alpha_j``, ``beta_j`` into the Fortran-ordered (ncv+1, ncv) real T; returns the
        breakdown step or -1."""
        assert T.flags.f_contiguous and T.dtype == np.float64
        bd = _I32(-1)
        self._call("extend", int(j0), int(j1), _ptr(T), T.shape[0], ctypes.byref(bd))
        return bd.value

    def _basis(self, ncols: int) -> np.ndarray:
        """The first ``ncols`` basis vectors on the host, in the basis' own row numbering."""
        V = np.empty((self.n, int(ncols)), dtype=self._dtype, order="F")
        self._call("basis", int(ncols), _ptr(V))
        return V

    def _max_out(self, max_out) -> int:
        return self.ncv if max_out is None else min(int(max_out), self.ncv)

    def _solve(self, o: lsa_ks_options, v0, max_out: int, *outputs):
        """``lsa_<_prefix>_solve`` from ``v0`` (``None``: the library's start) into ``outputs``, the arrays of ``max_out`` columns or
        entries between ``max_out`` and the estimates in the entry's argument list (``None``: a null pointer).  Returns ``(k, tail)``:
        the columns written, and what every result ends with -- ``estimates``, the seven fields of ``lsa_ks_result`` and the solve
        counters under this class' names."""
        est = np.zeros(max(max_out, 1), dtype=np.float64)
        counts = np.zeros(4, dtype=np.int64)
        res = lsa_ks_result()
        v = None if v0 is None else self._start(v0)
        self._call("solve", ctypes.byref(o), None if v is None else _ptr(v), max_out, *[None if a is None else _ptr(a) for a in outputs], _ptr(est),
                   ctypes.byref(res), *([_ptr(counts)] if self._counters else []))
        tail = {"estimates": est[:res.nout].copy(), "nconv": int(res.nconv), "restarts": int(res.restarts), "applies": int(res.op_applies),
                "next_unconverged": float(res.next_unconverged), "seconds_expand": res.seconds_expand, "seconds_dense": res.seconds_dense,
                "seconds_restart": res.seconds_restart, **{name: int(c) for name, c in zip(self._counters, counts)}}
        return res.nout, tail


def _start_vector(v, n: int, dtype) -> np.ndarray:
    """A start vector as a contiguous ``dtype`` array; ``ValueError`` unless it has shape ``(n,)``."""
    v = np.ascontiguousarray(v, dtype=dtype)
    if v.shape != (n,):
        raise ValueError(f"start vector must have shape ({n},)")
    return v


class DeviceVector(_Handle):
    _prefix = "vec"

    def __init__(self, ctx: Context, n: int, dtype=np.complex128):
        self.ctx = ctx
        self.n = int(n)
        self.dtype = np.dtype(dtype)
        h = ctypes.c_void_p()
        ctx.check(ctx._lib.lsa_vec_create(ctx.handle, self.n, _dtype_code(dtype), ctypes.byref(h)))
        self.handle = h

    @classmethod
    def from_numpy(cls, ctx: Context, a: np.ndarray) -> "DeviceVector":
        a = np.ascontiguousarray(a)
        if a.dtype not in (np.float64, np.complex128):
            a = a.astype(np.complex128 if a.dtype.kind == "c" else np.float64)
        v = cls(ctx, a.shape[0], a.dtype)
        v.upload(a)
        return v

    def upload(self, a: np.ndarray) -> None:
        a = np.ascontiguousarray(a, dtype=self.dtype)
        if a.shape != (self.n,):
            raise ValueError(f"expected shape ({self.n},), got {a.shape}")
        self.ctx.check(self.ctx._lib.lsa_vec_upload(self.ctx.handle, self.handle, _ptr(a)))

    def numpy(self) -> np.ndarray:
        out = np.empty(self.n, dtype=self.dtype)
        self.ctx.check(self.ctx._lib.lsa_vec_download(self.ctx.handle, self.handle, _ptr(out)))
        return out


class CsrMatrix(_Handle):
    """CSR matrix resident in HBM (int32 indices, float64 or complex128 values, sorted columns)."""

    _prefix = "mat"

    def __init__(self, ctx: Context, handle, shape, nnz: int, dtype, keep=()):
        self.ctx, self.handle, self.shape, self.nnz, self.dtype = ctx, handle, shape, int(nnz), np.dtype(dtype)
        self._keep = keep  # matrices whose index arrays this one shares

    @classmethod
    def from_scipy(cls, ctx: Context, A) -> "CsrMatrix":
        import scipy.sparse as sp

        A = sp.csr_matrix(A)
        if A.shape[0] != A.shape[1]:
            raise ValueError("lsa_csr_upload handles square matrices; use from_scipy_shard for row blocks")
        if not A.has_sorted_indices:
            A = A.copy()
            A.sort_indices()
        dt = np.complex128 if A.dtype.kind == "c" else np.float64
        rp = np.ascontiguousarray(A.indptr, dtype=np.int32)
        ci = np.ascontiguousarray(A.indices, dtype=np.int32)
        val = np.ascontiguousarray(A.data, dtype=dt)
        h = ctypes.c_void_p()
        ctx.check(
            ctx._lib.lsa_csr_upload(ctx.handle, A.shape[0], A.nnz, _ptr(rp), _ptr(ci), _ptr(val), _dtype_code(dt), ctypes.byref(h))
        )
        return cls(ctx, h, A.shape, A.nnz, dt)

    @classmethod
    def from_scipy_shard(cls, ctx: Context, A_rows, n_global: int, row0: int) -> "CsrMatrix":
        import scipy.sparse as sp

        A = sp.csr_matrix(A_rows)
        A.sort_indices()
        dt = np.complex128 if A.dtype.kind == "c" else np.float64
        rp = np.ascontiguousarray(A.indptr, dtype=np.int32)
        ci = np.ascontiguousarray(A.indices, dtype=np.int32)
        val = np.ascontiguousarray(A.data, dtype=dt)
        h = ctypes.c_void_p()
        ctx.check(
            ctx._lib.lsa_csr_upload_shard(
                ctx.handle, n_global, row0, row0 + A.shape[0], A.nnz, _ptr(rp), _ptr(ci), _ptr(val), _dtype_code(dt), ctypes.byref(h)
            )
        )
        return cls(ctx, h, (A.shape[0], n_global), A.nnz, dt)

    def prepare_lu(self, complex_factors: bool, leaf_size: int = 0, constraint=None) -> None:
        """Pattern-only phase of the nested-dissection LU for matrices with this pattern (``lsa_ndlu_prepare``);
        ``constraint``: optional mask of the zero-diagonal unknowns to eliminate after their neighbours."""
        flags = None if constraint is None else np.ascontiguousarray(constraint, dtype=np.int8)
        self.ctx.check(self.ctx._lib.lsa_ndlu_prepare(self.ctx.handle, self.handle, LSA_C128 if complex_factors else LSA_F64, int(leaf_size),
                                                      None if flags is None else _ptr(flags)))

    def prepare_lu_tree(self, complex_factors: bool, first, size, parent) -> None:
        """The same phase with the caller's forest (``lsa_ndlu_prepare_tree``): for a matrix already permuted into the
        elimination order of :func:`nd_order`, whose forest this is."""
        first, size, parent = (np.ascontiguousarray(a, dtype=np.int32) for a in (first, size, parent))
        self.ctx.check(self.ctx._lib.lsa_ndlu_prepare_tree(self.ctx.handle, self.handle, LSA_C128 if complex_factors else LSA_F64, len(parent),
                                                           _ptr(first), _ptr(size), _ptr(parent)))

    def axpby(self, other: "CsrMatrix", alpha: complex, beta: complex, dtype=None) -> "CsrMatrix":
        """alpha*self + beta*other on the shared pattern (MatAXPY, Solver/eigen2.py:110-111)."""
        alpha, beta = complex(alpha), complex(beta)
        if dtype is None:
            cplx = alpha.imag != 0 or beta.imag != 0 or self.dtype.kind == "c" or other.dtype.kind == "c"
            dtype = np.complex128 if cplx else np.float64
        h = ctypes.c_void_p()
        self.ctx.check(
            self.ctx._lib.lsa_csr_axpby(
                self.ctx.handle, self.handle, other.handle, (_DBL * 2)(alpha.real, alpha.imag), (_DBL * 2)(beta.real, beta.imag),
                _dtype_code(dtype), ctypes.byref(h),
            )
        )
        return CsrMatrix(self.ctx, h, self.shape, self.nnz, dtype, keep=(self, other))

    def windowed(self, left, right=None) -> "CsrMatrix":
        """``diag(left) @ self @ diag(right)`` on this matrix' pattern (``lsa_csr_window``; ``right=None``: ``left``): the values
        ``(left[i] * a_ij) * right[j]``, the bits of ``scipy.sparse.diags(left) @ A @ scipy.sparse.diags(right)``.  Real square
        matrices only; the result shares this matrix' index arrays and SpMV kernel form and keeps it alive."""
        n = self.shape[0]
        vecs = []
        for name, v in (("left", left), ("right", right)):
            if v is None and name == "right":
                vecs.append(None)
                continue
            a = np.asarray(v)
            if a.dtype.kind == "c":
                raise ValueError(f"lsa_csr_window: {name} is complex")
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape != (n,):
                raise ValueError(f"lsa_csr_window: {name} must have shape ({n},), got {a.shape}")
            vecs.append(a)
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx._lib.lsa_csr_window(self.ctx.handle, self.handle, _ptr(vecs[0]), None if vecs[1] is None else _ptr(vecs[1]),
                                                    ctypes.byref(h)))
        return CsrMatrix(self.ctx, h, self.shape, self.nnz, np.float64, keep=(self,))

    def values(self) -> np.ndarray:
        out = np.empty(self.nnz, dtype=self.dtype)
        self.ctx.check(self.ctx._lib.lsa_mat_download_values(self.ctx.handle, self.handle, _ptr(out)))
        return out

    def matvec(self, x: DeviceVector, y: DeviceVector) -> None:
        self.ctx.check(self.ctx._lib.lsa_spmv(self.ctx.handle, self.handle, x.handle, y.handle))

    def rmatvec(self, x: DeviceVector, y: DeviceVector, conj: bool = True) -> None:
        self.ctx.check(self.ctx._lib.lsa_spmv_transpose(self.ctx.handle, self.handle, int(conj), x.handle, y.handle))

    @staticmethod
    def spmv_transpose_batch(mats: "list[CsrMatrix]", xs: "list[DeviceVector]", ys: "list[DeviceVector]", conj: bool = False) -> None:
        """``ys[z] = mats[z]^T xs[z]`` (``conj``: ``mats[z]^H xs[z]``) for up to 16 matrices of one pattern and dtype in one launch
        (``lsa_spmv_transpose_batch``), each result bit-identical to :meth:`rmatvec`."""
        J = len(mats)
        if J == 0 or len(xs) != J or len(ys) != J:
            raise ValueError("spmv_transpose_batch needs as many inputs and outputs as matrices (at least one)")
        ctx = mats[0].ctx
        if any(m.ctx is not ctx for m in mats) or any(v.ctx is not ctx for v in list(xs) + list(ys)):
            raise ValueError("spmv_transpose_batch: the matrices and vectors must live in one context")
        arr = lambda objs: (ctypes.c_void_p * J)(*[o.handle.value for o in objs])  # noqa: E731
        ctx.check(ctx._lib.lsa_spmv_transpose_batch(ctx.handle, J, arr(mats), int(conj), arr(xs), arr(ys)))

    @staticmethod
    def spmv_batch(mats: "list[CsrMatrix]", xs: "list[DeviceVector]", ys: "list[DeviceVector]") -> None:
        """``ys[z] = mats[z] xs[z]`` for up to 16 whole square matrices of one pattern and dtype in one launch (``lsa_spmv_batch``);
        the same matrix may stand in several slots.  Each result is bit-identical to :meth:`matvec`."""
        J = len(mats)
        if J == 0 or len(xs) != J or len(ys) != J:
            raise ValueError("spmv_batch needs as many inputs and outputs as matrices (at least one)")
        ctx = mats[0].ctx
        if any(m.ctx is not ctx for m in mats) or any(v.ctx is not ctx for v in list(xs) + list(ys)):
            raise ValueError("spmv_batch: the matrices and vectors must live in one context")
        arr = lambda objs: (ctypes.c_void_p * J)(*[o.handle.value for o in objs])  # noqa: E731
        ctx.check(ctx._lib.lsa_spmv_batch(ctx.handle, J, arr(mats), arr(xs), arr(ys)))

    def matmat(self, X: DeviceVector, Y: DeviceVector, ncols: int, ldx: int | None = None, ldy: int | None = None) -> None:
        """``Y[:, c] = self @ X[:, c]`` for ``ncols`` columns (``lsa_spmm``).  ``X`` and ``Y`` are column-major complex128 blocks in
        one vector each (column ``c`` at ``c * ld``, ``ld`` defaulting to ``n``).  Two calls give the same bytes; a column need not
        hold the bytes of :meth:`matvec`."""
        n = self.shape[0]
        self.ctx.check(self.ctx._lib.lsa_spmm(self.ctx.handle, self.handle, int(ncols), X.handle, int(n if ldx is None else ldx), Y.handle,
                                              int(n if ldy is None else ldy)))

    def matmat_transpose(self, X: DeviceVector, Y: DeviceVector, ncols: int, conj: bool = True, ldx: int | None = None,
                         ldy: int | None = None) -> None:
        """``Y[:, c] = self^H @ X[:, c]`` (``conj``) or ``self^T @ X[:, c]`` for ``ncols`` columns (``lsa_spmm_transpose``), blocks as
        in :meth:`matmat`.  No atomics: two calls give the same bytes; a column need not hold the bytes of :meth:`rmatvec`."""
        n = self.shape[0]
        self.ctx.check(self.ctx._lib.lsa_spmm_transpose(self.ctx.handle, self.handle, int(bool(conj)), int(ncols), X.handle,
                                                        int(n if ldx is None else ldx), Y.handle, int(n if ldy is None else ldy)))

    def matvec_info(self, vector_dtype=np.complex128) -> dict:
        """Kernel ``lsa_spmv`` launches for this matrix / vector type and the bytes it moves per launch."""
        name = ctypes.create_string_buffer(128)
        nbytes = _I64(0)
        self.ctx.check(self.ctx._lib.lsa_spmv_info(self.ctx.handle, self.handle, _dtype_code(vector_dtype), name, 128, ctypes.byref(nbytes)))
        return {"kernel": name.value.decode(), "bytes_moved": nbytes.value}

    def time_matvec(self, x: DeviceVector, y: DeviceVector, iters: int) -> float:
        """Mean milliseconds per SpMV launch over ``iters`` back-to-back launches (HIP events on the library's stream)."""
        ms = _DBL(0.0)
        self.ctx.check(self.ctx._lib.lsa_spmv_time(self.ctx.handle, self.handle, x.handle, y.handle, int(iters), ctypes.byref(ms)))
        return ms.value


class Ilu(_Handle):
    """ILU(k) factors + triangular-solve schedule on the device."""

    _prefix = "ilu"

    def __init__(self, ctx: Context, C: CsrMatrix, levels: int = 0, shift_tol: float = 0.0):
        self.ctx, self._C = ctx, C
        h = ctypes.c_void_p()
        ctx.check(ctx._lib.lsa_ilu_create(ctx.handle, C.handle, int(levels), float(shift_tol), ctypes.byref(h)))
        self.handle = h
        self.n = C.shape[0]
        self.dtype = C.dtype

    def info(self) -> dict:
        nnz, ll, lu, ns = _I64(0), _I32(0), _I32(0), _I32(0)
        self.ctx._lib.lsa_ilu_info(self.handle, ctypes.byref(nnz), ctypes.byref(ll), ctypes.byref(lu), ctypes.byref(ns))
        return {"nnz": nnz.value, "levels_lower": ll.value, "levels_upper": lu.value, "nshift": ns.value}

    def set_algorithm(self, algo: int, block_size: int = 0) -> None:
        """0 = level launches, 1 = sync-free, 2 = blocked with inverted diagonal blocks (see include/lsa_hip.h)."""
        self.ctx.check(self.ctx._lib.lsa_ilu_set_algorithm(self.ctx.handle, self.handle, int(algo), int(block_size)))

    def solve(self, b: DeviceVector, x: DeviceVector, which: int = 2) -> None:
        self.ctx.check(self.ctx._lib.lsa_ilu_solve(self.ctx.handle, self.handle, int(which), b.handle, x.handle))

    def time_solve(self, b: DeviceVector, x: DeviceVector, iters: int, which: int = 2) -> float:
        """Mean milliseconds per triangular solve (HIP events on the library's stream)."""
        ms = _DBL(0.0)
        self.ctx.check(self.ctx._lib.lsa_ilu_solve_time(self.ctx.handle, self.handle, int(which), b.handle, x.handle, int(iters), ctypes.byref(ms)))
        return ms.value

    def factors(self):
        """(rowptr, col, val) of the combined L\\U factor."""
        nnz = self.info()["nnz"]
        rp = np.empty(self.n + 1, dtype=np.int32)
        ci = np.empty(nnz, dtype=np.int32)
        val = np.empty(nnz, dtype=self.dtype)
        self.ctx.check(self.ctx._lib.lsa_ilu_download(self.ctx.handle, self.handle, _ptr(rp), _ptr(ci), _ptr(val)))
        return rp, ci, val


class NdAnalysis:
    """Host-only analysis of the nested-dissection multifrontal LU (``lsa_nd_analyse``): ordering, elimination forest
    and the index tables of the device kernels.  Needs no GPU; used by the tests and by sizing tools."""

    def __init__(self, A, leaf_size: int = 0, constraint=None, tree=None, rank: int = 0, nranks: int = 1, order_only: bool = False):
        """``order_only``: the elimination order and the forest without the index tables (``lsa_nd_order``).
        ``constraint``: optional boolean mask of the unknowns with a numerically zero diagonal (eliminated after all
        their neighbours: the pressure rows of a saddle-point matrix).  ``tree``: instead of dissecting, take the forest
        ``{"first", "size", "parent"[, "owner"]}`` (``lsa_nd_analyse_tree``), localised for ``rank`` of ``nranks``."""
        import scipy.sparse as sp

        A = sp.csr_matrix(A)
        if A.shape[0] != A.shape[1]:
            raise ValueError("the analysis needs a square pattern")
        self._lib = load_library()
        self.n, self.nnz = A.shape[0], A.nnz
        rp = np.ascontiguousarray(A.indptr, dtype=np.int32)
        ci = np.ascontiguousarray(A.indices, dtype=np.int32)
        h = ctypes.c_void_p()
        flags = None if constraint is None else np.ascontiguousarray(constraint, dtype=np.int8)
        if flags is not None and flags.shape != (self.n,):
            raise ValueError("constraint mask must have one entry per row")
        if tree is None and order_only:
            rc = self._lib.lsa_nd_order(self.n, _ptr(rp), _ptr(ci), int(leaf_size), None if flags is None else _ptr(flags), ctypes.byref(h))
        elif tree is None:
            rc = self._lib.lsa_nd_analyse(self.n, _ptr(rp), _ptr(ci), int(leaf_size), None if flags is None else _ptr(flags), ctypes.byref(h))
        else:
            first, size, parent = (np.ascontiguousarray(tree[k], dtype=np.int32) for k in ("first", "size", "parent"))
            owner = None if tree.get("owner") is None else np.ascontiguousarray(tree["owner"], dtype=np.int32)
            rc = self._lib.lsa_nd_analyse_tree(self.n, _ptr(rp), _ptr(ci), len(parent), _ptr(first), _ptr(size), _ptr(parent),
                                               None if owner is None else _ptr(owner), int(rank), int(nranks), ctypes.byref(h))
        self.handle = h
        if rc != 0:
            msg = self._lib.lsa_nd_sym_error(h).decode(errors="replace")
            raise ValueError(msg)
        nt, nl, mf = _I32(0), _I32(0), _I32(0)
        ie, fe, fre, fl = _I64(0), _I64(0), _I64(0), _DBL(0.0)
        self._lib.lsa_nd_sym_info(h, ctypes.byref(nt), ctypes.byref(nl), ctypes.byref(mf), ctypes.byref(ie), ctypes.byref(fe), ctypes.byref(fre),
                                  ctypes.byref(fl))
        self.ntree, self.nlevels, self.max_front = nt.value, nl.value, mf.value
        self.index_entries, self.factor_entries, self.front_entries, self.flops = ie.value, fe.value, fre.value, fl.value

    def export(self) -> dict:
        """perm, node_start, parent, level, front_size, idx (see include/lsa_hip.h)."""
        out = {"perm": np.empty(self.n, np.int32), "node_start": np.empty(self.ntree + 1, np.int32), "parent": np.empty(self.ntree, np.int32),
               "level": np.empty(self.ntree, np.int32), "front_size": np.empty(self.ntree, np.int32), "idx": np.empty(self.index_entries, np.int32)}
        self._lib.lsa_nd_sym_export(self.handle, *[_ptr(out[k]) for k in ("perm", "node_start", "parent", "level", "front_size", "idx")])
        return out

    def memory(self, scalar_bytes: int = 16, work_budget_bytes: int = 0, detail: bool = False) -> dict:
        """Device memory a factorisation of this analysis allocates, in bytes (``lsa_nd_sym_memory``); with ``detail`` also the
        per-node plan (update-arena and working-arena offsets in scalars, chunk of every node)."""
        out = np.zeros(8, np.int64)
        upd = np.zeros(self.ntree, np.int64) if detail else None
        work = np.zeros(self.ntree, np.int64) if detail else None
        chunk = np.full(self.ntree, -1, np.int32) if detail else None
        rc = self._lib.lsa_nd_sym_memory(self.handle, int(scalar_bytes), int(work_budget_bytes), _ptr(out), None if upd is None else _ptr(upd),
                                         None if work is None else _ptr(work), None if chunk is None else _ptr(chunk))
        if rc != 0:
            raise ValueError("lsa_nd_sym_memory: bad argument")
        rec = {"factors": int(out[0]), "working_arena": int(out[1]), "update_arena": int(out[2]), "exchange_region": int(out[3]), "sweep_buffers": int(out[4]),
               "chunks": int(out[5]), "largest_front": int(out[6]), "index_tables": int(out[7])}
        rec["total"] = rec["factors"] + rec["working_arena"] + rec["update_arena"] + rec["sweep_buffers"] + rec["index_tables"]
        if detail:
            rec.update({"upd_off": upd, "work_off": work, "chunk_of": chunk})
        return rec

    def export_tables(self) -> dict:
        """cmap, gptr, gidx, asm_dst, lvl_ptr, lvl_nodes (the tables the device kernels walk)."""
        ex = self.export()
        m = np.diff(ex["node_start"])
        b = ex["front_size"] - m
        scal = np.zeros(6, np.int64)
        self._lib.lsa_nd_sym_export_dist(self.handle, None, None, None, None, None, None, _ptr(scal))
        nlist = int(np.count_nonzero(np.ones(self.ntree)))  # lvl_nodes holds the nodes this rank works on (ghosts excluded)
        out = {"cmap": np.empty(int(b.sum()), np.int32), "gptr": np.empty(int((ex["front_size"] + 1).sum()), np.int32),
               "gidx": np.empty(int(b.sum()), np.int32), "asm_dst": np.empty(int(scal[3]), np.int64), "lvl_ptr": np.empty(self.nlevels + 1, np.int32),
               "lvl_nodes": np.full(nlist, -1, np.int32), "kind": np.empty(self.ntree, np.int32), "front_off": np.empty(self.ntree + 1, np.int64),
               "u_off": np.empty(self.ntree + 1, np.int64), "asm_src": np.empty(int(scal[3]), np.int32), "child_ptr": np.empty(self.ntree + 1, np.int32)}
        self._lib.lsa_nd_sym_export_tables(self.handle, *[_ptr(out[k]) for k in ("cmap", "gptr", "gidx", "asm_dst", "lvl_ptr", "lvl_nodes")])
        out["lvl_nodes"] = out["lvl_nodes"][: int(out["lvl_ptr"][-1])]
        self._lib.lsa_nd_sym_export_dist(self.handle, _ptr(out["kind"]), _ptr(out["front_off"]), _ptr(out["u_off"]), _ptr(out["asm_src"]),
                                         _ptr(out["child_ptr"]), None, None)
        out["child_idx"] = np.empty(int(out["child_ptr"][-1]), np.int32)
        self._lib.lsa_nd_sym_export_dist(self.handle, None, None, None, None, None, _ptr(out["child_idx"]), None)
        out["owner"] = np.zeros(self.ntree, np.int32)
        rows, exch, totals = np.zeros(4 * self.ntree, np.int32), np.zeros(4 * self.ntree, np.int64), np.zeros(2, np.int64)
        self._lib.lsa_nd_sym_export_top(self.handle, _ptr(out["owner"]), _ptr(rows), _ptr(exch), _ptr(totals))
        rows, exch = rows.reshape(-1, 4), exch.reshape(-1, 4)
        out.update({"brow0": rows[:, 0].copy(), "brow": rows[:, 1].copy(), "orow0": rows[:, 2].copy(), "orows": rows[:, 3].copy(),
                    "ux_base": exch[:, 0].copy(), "ux_stride": exch[:, 1].copy(), "xg_base": exch[:, 2].copy(), "xg_stride": exch[:, 3].copy(),
                    "u_entries": int(totals[0]), "xg_entries": int(totals[1])})
        out.update(ex)
        out.update({"front_slot": int(scal[0]), "u_slot": int(scal[1]), "phase_b_level": int(scal[2]), "nranks": int(scal[4]), "rank": int(scal[5])})
        return out

    def __del__(self):
        if getattr(self, "handle", None):
            self._lib.lsa_nd_sym_destroy(self.handle)
            self.handle = None


def nd_order(A, leaf_size: int = 0, constraint=None) -> dict:
    """Elimination order of the nested-dissection LU for the pattern of ``A`` (host only): ``perm`` (new -> old index) and the
    forest ``first`` / ``size`` / ``parent`` of contiguous index ranges of the permuted matrix ``A[perm][:, perm]``."""
    an = NdAnalysis(A, leaf_size, constraint=constraint, order_only=True)
    ex = {"perm": np.empty(an.n, np.int32), "node_start": np.empty(an.ntree + 1, np.int32), "parent": np.empty(an.ntree, np.int32),
          "level": np.empty(an.ntree, np.int32)}
    an._lib.lsa_nd_sym_export(an.handle, _ptr(ex["perm"]), _ptr(ex["node_start"]), _ptr(ex["parent"]), _ptr(ex["level"]), None, None)
    return {"perm": ex["perm"].astype(np.int64), "first": ex["node_start"][:-1].copy(), "size": np.diff(ex["node_start"]).astype(np.int32),
            "parent": ex["parent"], "level": ex["level"]}


NDLU_BATCH_MAX = 16  # factorisations of one lsa_ndlu_solve_batch call (kNdBatchMax in csrc/ndlu_internal.h)
NDLU_MULTI_MAX = 8  # most columns of one pass of lsa_ndlu_solve_multi (kNdMultiMax: real vectors; complex vectors run passes of at most 4)
NDLU_MULTI_CHUNK = 256  # vector entries per column a multi-column sweep tile stages in LDS at a time (kMCH)
_TRANS = {"N": 0, "T": 1, "H": 2}


class NdLu(_Handle):
    """Nested-dissection multifrontal LU of a CSR matrix, resident on the device (``lsa_ndlu_*``)."""

    _prefix = "ndlu"

    def __init__(self, ctx: Context, C: CsrMatrix, leaf_size: int = 0, tree: dict | None = None):
        """``tree``: ``{"first", "size", "parent"[, "owner"]}`` selects ``lsa_ndlu_create_tree`` (subtree-parallel when
        the context has more than one rank and ``owner`` is given)."""
        self.ctx, self._C = ctx, C
        h = ctypes.c_void_p()
        if tree is None:
            ctx.check(ctx._lib.lsa_ndlu_create(ctx.handle, C.handle, int(leaf_size), ctypes.byref(h)))
        else:
            first, size, parent = (np.ascontiguousarray(tree[k], dtype=np.int32) for k in ("first", "size", "parent"))
            owner = None if tree.get("owner") is None else np.ascontiguousarray(tree["owner"], dtype=np.int32)
            ctx.check(ctx._lib.lsa_ndlu_create_tree(ctx.handle, C.handle, len(parent), _ptr(first), _ptr(size), _ptr(parent),
                                                    None if owner is None else _ptr(owner), ctypes.byref(h)))
        self.handle = h
        self.n = C.shape[0]

    def refactor(self, C: CsrMatrix) -> None:
        self.ctx.check(self.ctx._lib.lsa_ndlu_refactor(self.ctx.handle, self.handle, C.handle))
        self._C = C

    def info(self) -> dict:
        nt, nl, mf, nla, nfl = _I32(0), _I32(0), _I32(0), _I32(0), _I32(0)
        fe, fre, ab = _I64(0), _I64(0), _I64(0)
        sa, sn = _DBL(0.0), _DBL(0.0)
        self.ctx._lib.lsa_ndlu_info(self.handle, ctypes.byref(nt), ctypes.byref(nl), ctypes.byref(mf), ctypes.byref(fe), ctypes.byref(fre),
                                    ctypes.byref(ab), ctypes.byref(nla), ctypes.byref(sa), ctypes.byref(sn), ctypes.byref(nfl))
        return {"tree_nodes": nt.value, "levels": nl.value, "max_front": mf.value, "factor_entries": fe.value, "front_entries": fre.value,
                "apply_bytes": ab.value, "apply_launches": nla.value, "seconds_analyse": sa.value, "seconds_numeric": sn.value,
                "factor_launches": nfl.value}

    def sweep_levels(self) -> list[dict]:
        """Per tree level (leaves first) what the sweeps launch: nodes, the widest pivot block, the rows of an upward and of a
        downward tile, and the tiles of the tallest node upwards and downwards (``lsa_ndlu_sweep_level``)."""
        keys = ("nodes", "max_pivot", "fwd_rows", "bwd_rows", "fwd_tiles", "bwd_tiles")
        out = []
        for level in range(self.info()["levels"]):
            v = [_I32(0) for _ in keys]
            if self.ctx._lib.lsa_ndlu_sweep_level(self.handle, level, *[ctypes.byref(a) for a in v]) != 0:
                break
            out.append({k: a.value for k, a in zip(keys, v)})
        return out

    def solve(self, b: DeviceVector, x: DeviceVector) -> None:
        self.ctx.check(self.ctx._lib.lsa_ndlu_solve(self.ctx.handle, self.handle, b.handle, x.handle))

    @staticmethod
    def solve_batch(factors: "list[NdLu]", bs: "list[DeviceVector]", xs: "list[DeviceVector]", trans: str = "N") -> None:
        """``xs[z] = C_z^-1 bs[z]`` for up to 16 factorisations of one analysis in one context (``lsa_ndlu_solve_batch``): one
        launch per tree level and direction for the whole batch, each result bit-identical to :meth:`solve`.  ``trans="T"`` /
        ``"H"``: ``C_z^-T`` / ``C_z^-H`` through the batched transposed sweeps (``lsa_ndlu_solve_batch_adjoint``), each result
        bit-identical to :meth:`solve_adjoint`."""
        if trans not in _TRANS:
            raise ValueError(f"trans must be 'N', 'T' or 'H', got {trans!r}")
        ctx, args = NdLu._sets_args("solve_batch", factors, bs, xs, None if trans == "N" else int(trans == "H"))
        ctx.check((ctx._lib.lsa_ndlu_solve_batch if trans == "N" else ctx._lib.lsa_ndlu_solve_batch_adjoint)(*args))

    def solve_adjoint(self, b: DeviceVector, x: DeviceVector, conj: bool = True) -> None:
        """x = C^-H b (``conj``) or C^-T b on the same factors."""
        self.ctx.check(self.ctx._lib.lsa_ndlu_solve_adjoint(self.ctx.handle, self.handle, int(conj), b.handle, x.handle))

    def time_solve(self, b: DeviceVector, x: DeviceVector, iters: int) -> float:
        ms = _DBL(0.0)
        self.ctx.check(self.ctx._lib.lsa_ndlu_solve_time(self.ctx.handle, self.handle, b.handle, x.handle, int(iters), ctypes.byref(ms)))
        return ms.value

    def _multi_args(self, B: DeviceVector, X: DeviceVector, nrhs: int, ldb, ldx, trans: str):
        if trans not in _TRANS:
            raise ValueError(f"trans must be 'N', 'T' or 'H', got {trans!r}")
        return (self.ctx.handle, self.handle, _TRANS[trans], int(nrhs), B.handle, int(self.n if ldb is None else ldb), X.handle,
                int(self.n if ldx is None else ldx))

    def solve_multi(self, B: DeviceVector, X: DeviceVector, nrhs: int, ldb: int | None = None, ldx: int | None = None, trans: str = "N") -> None:
        """``X[:, q] = op(C)^-1 B[:, q]`` for ``nrhs`` columns on this factorisation (``lsa_ndlu_solve_multi``).  ``B`` and ``X``
        are column-major blocks in one vector each (column ``q`` at ``q * ld``, ``ld`` defaulting to ``n``); ``B is X`` solves in
        place.  ``trans``: ``"N"``, ``"T"`` or ``"H"``.  Every column is bit-identical to :meth:`solve` / :meth:`solve_adjoint`."""
        self.ctx.check(self.ctx._lib.lsa_ndlu_solve_multi(*self._multi_args(B, X, nrhs, ldb, ldx, trans)))

    def time_solve_multi(self, B: DeviceVector, X: DeviceVector, nrhs: int, iters: int, ldb: int | None = None, ldx: int | None = None,
                         trans: str = "N") -> float:
        """Mean milliseconds of one block solve over ``iters`` back-to-back repetitions (``lsa_ndlu_solve_multi_time``)."""
        ms = _DBL(0.0)
        self.ctx.check(self.ctx._lib.lsa_ndlu_solve_multi_time(*self._multi_args(B, X, nrhs, ldb, ldx, trans), int(iters), ctypes.byref(ms)))
        return ms.value

    @staticmethod
    def _sets_args(name, factors, Bs, Xs, flag, nrhs=None, ldb=None, ldx=None, refuse=None):
        """The arguments of a C entry for a batch of factor sets, behind the checks of the method ``name``: the lists, the
        one-context rule, the handle arrays, and for blocks (``nrhs`` given) the leading dimensions, ``n`` by default.  ``flag``:
        the entry's ``trans`` or ``conj`` argument (``None``: it has none); ``refuse``: an argument error of the caller's, raised
        in its place among the checks."""
        # (the argument errors come first: nothing of the library, not even a context, is touched before them)
        J = len(factors)
        if nrhs is None:  # one vector per problem
            if J == 0 or len(Bs) != J or len(Xs) != J:
                raise ValueError(f"{name} needs as many right-hand sides and outputs as factorisations (at least one)")
            if J > NDLU_BATCH_MAX:
                raise ValueError(f"{name} takes at most {NDLU_BATCH_MAX} factorisations, got {J}")
        else:
            if J < 1 or J > NDLU_BATCH_MAX:
                raise ValueError(f"{name} takes between 1 and {NDLU_BATCH_MAX} factorisations, got {J}")
            if len(Bs) != J or len(Xs) != J:
                raise ValueError(f"{name} needs as many blocks B and X as factorisations ({J}), got {len(Bs)} and {len(Xs)}")
        if refuse:
            raise ValueError(refuse)
        ctx = factors[0].ctx
        if any(f.ctx is not ctx for f in factors) or any(v.ctx is not ctx for v in list(Bs) + list(Xs)):
            raise ValueError(f"{name}: the factorisations and vectors must live in one context")
        arr = lambda objs: (ctypes.c_void_p * J)(*[o.handle.value for o in objs])  # noqa: E731
        head = (ctx.handle, J, arr(factors)) + (() if flag is None else (flag,))
        if nrhs is None:
            return ctx, head + (arr(Bs), arr(Xs))
        n = factors[0].n
        return ctx, head + (int(nrhs), arr(Bs), int(n if ldb is None else ldb), arr(Xs), int(n if ldx is None else ldx))

    @staticmethod
    def solve_multi_batch(factors: "list[NdLu]", Bs: "list[DeviceVector]", Xs: "list[DeviceVector]", nrhs: int, ldb: int | None = None,
                          ldx: int | None = None, trans: str = "N") -> None:
        """``Xs[z][:, q] = C_z^-1 Bs[z][:, q]`` for ``nrhs`` columns on up to 16 factorisations of one analysis
        (``lsa_ndlu_solve_multi_batch``): every launch of the sweeps carries all columns of a pass for all sets.  The blocks share
        ``ldb`` and ``ldx`` (default ``n``); several sets may read one ``B``; ``Bs[z] is Xs[z]`` solves in place.  Every column is
        bit-identical to :meth:`solve`.  ``trans`` must be ``"N"``: the transposed form is :meth:`solve_multi_batch_adjoint`."""
        refuse = None if trans == "N" else f"solve_multi_batch: trans must be 'N', got {trans!r}: the transposed form on a batch of factor sets is not built"
        ctx, args = NdLu._sets_args("solve_multi_batch", factors, Bs, Xs, 0, nrhs, ldb, ldx, refuse)
        ctx.check(ctx._lib.lsa_ndlu_solve_multi_batch(*args))

    @staticmethod
    def time_solve_multi_batch(factors: "list[NdLu]", Bs: "list[DeviceVector]", Xs: "list[DeviceVector]", nrhs: int, iters: int,
                               ldb: int | None = None, ldx: int | None = None) -> float:
        """Mean milliseconds of one block solve on all sets over ``iters`` back-to-back repetitions (``lsa_ndlu_solve_multi_batch_time``)."""
        ctx, args = NdLu._sets_args("solve_multi_batch", factors, Bs, Xs, 0, nrhs, ldb, ldx)
        ms = _DBL(0.0)
        ctx.check(ctx._lib.lsa_ndlu_solve_multi_batch_time(*args, int(iters), ctypes.byref(ms)))
        return ms.value

    @staticmethod
    def solve_multi_batch_adjoint(factors: "list[NdLu]", Bs: "list[DeviceVector]", Xs: "list[DeviceVector]", nrhs: int, conj: bool = True,
                                  ldb: int | None = None, ldx: int | None = None) -> None:
        """``Xs[z][:, q] = C_z^-H Bs[z][:, q]`` (``conj``) or ``C_z^-T Bs[z][:, q]`` for ``nrhs`` columns on up to 16 factorisations of
        one analysis (``lsa_ndlu_solve_multi_batch_adjoint``): every launch of the transposed sweeps carries all columns of a pass for
        all sets.  The rules for the blocks are those of :meth:`solve_multi_batch`.  Every column is bit-identical to
        :meth:`solve_adjoint`."""
        ctx, args = NdLu._sets_args("solve_multi_batch_adjoint", factors, Bs, Xs, int(bool(conj)), nrhs, ldb, ldx)
        ctx.check(ctx._lib.lsa_ndlu_solve_multi_batch_adjoint(*args))

    @staticmethod
    def time_solve_multi_batch_adjoint(factors: "list[NdLu]", Bs: "list[DeviceVector]", Xs: "list[DeviceVector]", nrhs: int, iters: int,
                                       conj: bool = True, ldb: int | None = None, ldx: int | None = None) -> float:
        """Mean milliseconds of one transposed block solve on all sets over ``iters`` back-to-back repetitions
        (``lsa_ndlu_solve_multi_batch_adjoint_time``)."""
        ctx, args = NdLu._sets_args("solve_multi_batch_adjoint", factors, Bs, Xs, int(bool(conj)), nrhs, ldb, ldx)
        ms = _DBL(0.0)
        ctx.check(ctx._lib.lsa_ndlu_solve_multi_batch_adjoint_time(*args, int(iters), ctypes.byref(ms)))
        return ms.value

    def set_multi_transposed(self, on: bool) -> None:
        """``True``: :meth:`solve_multi` and :meth:`time_solve_multi` with ``trans`` ``"T"`` / ``"H"`` run in the wide passes of
        ``trans="N"`` (``lsa_ndlu_set_multi_transposed``; same bits per column).  Off by default: column by column."""
        self.ctx.check(self.ctx._lib.lsa_ndlu_set_multi_transposed(self.ctx.handle, self.handle, int(bool(on))))

    def multi_info(self) -> dict:
        """What the last :meth:`solve_multi` used, in either direction: ``width`` (columns of its widest pass; 1 = column by column, 0 = none yet),
        ``extra_bytes`` (per-column sweep buffers), ``launches_per_pass``."""
        w, la, eb = _I32(0), _I32(0), _I64(0)
        self.ctx.check(self.ctx._lib.lsa_ndlu_multi_info(self.handle, ctypes.byref(w), ctypes.byref(eb), ctypes.byref(la)))
        return {"width": w.value, "extra_bytes": eb.value, "launches_per_pass": la.value}

    def inertia(self) -> tuple[int, int, int]:
        """(negative, zero, positive) eigenvalue counts of a REAL SYMMETRIC matrix from its factors (``lsa_ndlu_inertia``): for
        ``C = A - sigma M`` of a definite pencil, ``negative`` is the number of eigenvalues below ``sigma``."""
        ng, ze, ps = _I64(0), _I64(0), _I64(0)
        self.ctx.check(self.ctx._lib.lsa_ndlu_inertia(self.ctx.handle, self.handle, ctypes.byref(ng), ctypes.byref(ze), ctypes.byref(ps)))
        return ng.value, ze.value, ps.value


def gmres(ctx: Context, C: CsrMatrix, pc: Ilu | None, b: DeviceVector, x: DeviceVector, *, rtol=1e-10, restart=200, maxit=2000,
          use_x0=False):
    """Right-preconditioned GMRES on the device; returns (iterations, relative residual)."""
    its, rr = _I32(0), _DBL(0.0)
    rc = ctx._lib.lsa_gmres(ctx.handle, C.handle, pc.handle if pc else None, b.handle, x.handle, int(use_x0), float(rtol), int(restart),
                            int(maxit), ctypes.byref(its), ctypes.byref(rr))
    ctx.check(rc)
    return its.value, rr.value


class ShiftInvertOperator(_Handle):
    """``y = (A - sigma M)^-1 M x`` (mode 0, iSTType.SINVERT), ``y = M^-1 (A - sigma M) x`` (mode 1, iSTType.SHIFT) or
    ``y = (A - sigma M)^-1 (A + nu M) x`` (mode 2, iSTType.CAYLEY with antishift ``nu``)."""

    _prefix = "op"

    def __init__(self, ctx: Context, A: CsrMatrix, M: CsrMatrix | None, sigma: complex, *, mode: int = 0, antishift: complex = 0.0,
                 ilu_levels: int = 0,
                 ilu_shift: float = 0.0, ksp_rtol: float = 1e-11, ksp_restart: int = 200, ksp_maxit: int = 2000, pc_type: int = 1,
                 A_diag: CsrMatrix | None = None, M_diag: CsrMatrix | None = None, forest=None, rows: tuple[int, int] | None = None):
        """With ``A_diag`` (and ``M_diag``) given, ``A`` / ``M`` are this rank's row shards in the padded block layout
        (:mod:`lsa_hip.sharding`) and the preconditioner is block-Jacobi over ranks.  With ``forest`` (a
        :class:`lsa_hip.sharding.ForestPartition`) and ``rows`` (this rank's padded row range), ``A`` / ``M`` are the WHOLE
        padded matrices and the inner solve is the subtree-parallel exact LU (``lsa_op_create_dist``)."""
        self.ctx, self._A, self._M, self._Ad, self._Md = ctx, A, M, A_diag, M_diag
        sigma = complex(sigma)
        antishift = complex(antishift)
        opts = lsa_op_options(int(ilu_levels), float(ilu_shift), float(ksp_rtol), int(ksp_restart), int(ksp_maxit), int(pc_type),
                              (_DBL * 2)(antishift.real, antishift.imag))
        h = ctypes.c_void_p()
        sig = (_DBL * 2)(sigma.real, sigma.imag)
        if forest is not None:
            self._forest = tuple(np.ascontiguousarray(getattr(forest, k), dtype=np.int32) for k in ("first", "size", "parent", "owner"))
            f0, f1, f2, f3 = self._forest
            ctx.check(ctx._lib.lsa_op_create_dist(ctx.handle, A.handle, M.handle if M is not None else None, int(rows[0]), int(rows[1]), len(f2),
                                                  _ptr(f0), _ptr(f1), _ptr(f2), _ptr(f3), sig, int(mode), ctypes.byref(opts), ctypes.byref(h)))
        elif A_diag is None:
            ctx.check(ctx._lib.lsa_op_create(ctx.handle, A.handle, M.handle if M is not None else None, sig, int(mode), ctypes.byref(opts), ctypes.byref(h)))
        else:
            ctx.check(
                ctx._lib.lsa_op_create_sharded(ctx.handle, A.handle, M.handle if M is not None else None, A_diag.handle,
                                               M_diag.handle if M_diag is not None else None, sig, int(mode), ctypes.byref(opts), ctypes.byref(h))
            )
        self.handle = h
        self.n = A.shape[1]  # vector length (padded global length when sharded)
        self.sigma = sigma
        self.mode = mode

    def apply(self, x: DeviceVector, y: DeviceVector) -> None:
        self.ctx.check(self.ctx._lib.lsa_op_apply(self.ctx.handle, self.handle, x.handle, y.handle))

    def set_adjoint(self, on: bool = True) -> None:
        """Apply ``(A - sigma M)^-H M^H`` on the same factors (``lsa_op_set_adjoint``)."""
        self.ctx.check(self.ctx._lib.lsa_op_set_adjoint(self.ctx.handle, self.handle, int(on)))

    def set_projection(self, keep: np.ndarray | None) -> None:
        """Projected operator ``y = P Kfac^-1 Kmul x``, ``P = diag(keep)`` with 0/1 entries (``None`` removes it)."""
        if keep is None:
            self.ctx.check(self.ctx._lib.lsa_op_set_projection(self.ctx.handle, self.handle, None))
            return
        keep = np.ascontiguousarray(keep, dtype=np.float64)
        if keep.shape != (self.n,):
            raise ValueError(f"projection mask must have shape ({self.n},)")
        self.ctx.check(self.ctx._lib.lsa_op_set_projection(self.ctx.handle, self.handle, _ptr(keep)))

    def stats(self) -> dict:
        st = lsa_stats()
        self.ctx._lib.lsa_op_stats(self.handle, ctypes.byref(st))
        return {name: getattr(st, name) for name, _ in lsa_stats._fields_}


class KrylovBasis(_Handle):
    """Arnoldi basis in HBM + the recurrences Krylov-Schur needs.  Implements the backend protocol of
    :func:`lsa_hip.krylov_schur.krylov_schur` (``n``, ``ncv``, ``inject``, ``extend``, ``restart``, ``ritz_vectors``)."""

    _prefix = "krylov"

    def __init__(self, ctx: Context, op: ShiftInvertOperator, ncv: int, mask: np.ndarray | None = None):
        """``mask`` (0/1 per slot) zeroes the padding slots of injected vectors in the sharded block layout."""
        self.ctx, self._op, self._mask = ctx, op, mask
        self.n, self.ncv = op.n, int(ncv)
        h = ctypes.c_void_p()
        ctx.check(ctx._lib.lsa_krylov_create(ctx.handle, op.handle, self.ncv, ctypes.byref(h)))
        self.handle = h

    def set_row_permutation(self, perm: np.ndarray | None) -> None:
        """``perm[i]`` = the caller's index of basis row ``i``: Ritz vectors then come back in the caller's numbering."""
        p = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
        self.ctx.check(self.ctx._lib.lsa_krylov_set_row_permutation(self.ctx.handle, self.handle, None if p is None else _ptr(p)))

    def inject(self, j: int, v: np.ndarray) -> None:
        v = _start_vector(v, self.n, np.complex128)
        if self._mask is not None:
            v = np.ascontiguousarray(v * self._mask)
        self.ctx.check(self.ctx._lib.lsa_krylov_inject(self.ctx.handle, self.handle, int(j), _ptr(v)))

    def extend(self, j0: int, j1: int, H: np.ndarray) -> int:
        """Arnoldi steps j0..j1-1 writing columns of the Fortran-ordered (ncv+1, ncv) complex H; returns the
        breakdown step or -1."""
        assert H.flags.f_contiguous and H.dtype == np.complex128
        bd = _I32(-1)
        self.ctx.check(self.ctx._lib.lsa_krylov_extend(self.ctx.handle, self.handle, int(j0), int(j1), _ptr(H), H.shape[0], ctypes.byref(bd)))
        return bd.value

    def restart(self, m: int, Q: np.ndarray) -> None:
        Q = np.asfortranarray(Q, dtype=np.complex128)
        self.ctx.check(self.ctx._lib.lsa_krylov_restart(self.ctx.handle, self.handle, int(m), Q.shape[1], _ptr(Q), Q.shape[0]))

    def ritz_vectors(self, m: int, Y: np.ndarray, normalise: bool = True, canonical_phase: bool = True) -> np.ndarray:
        """``X = V[:, :m] Y`` on the host; unit columns when ``normalise``; with ``canonical_phase`` also rotated so that the
        entry of largest magnitude is real and positive, and ``self.imag_norms`` = the 2-norms of the imaginary parts."""
        Y = np.asfortranarray(Y, dtype=np.complex128)
        X = np.empty((self.n, Y.shape[1]), dtype=np.complex128, order="F")
        mode = (1 if normalise else 0) | (2 if (normalise and canonical_phase) else 0)
        self.ctx.check(self.ctx._lib.lsa_krylov_ritz_vectors(self.ctx.handle, self.handle, int(m), Y.shape[1], _ptr(Y), Y.shape[0], mode, _ptr(X)))
        self.imag_norms = None
        if mode & 2:
            out = np.zeros(Y.shape[1], dtype=np.float64)
            if self.ctx._lib.lsa_krylov_imag_norms(self.handle, Y.shape[1], _ptr(out)) == 0:
                self.imag_norms = out
        return X

    def _ks_start(self, v0):
        return None if v0 is None else _start_vector(v0, self.n, np.complex128)

    def _ks_collect(self, res: lsa_ks_result, theta, lam, est, X, max_out):
        """What a library solve left in its output arrays, as a :class:`lsa_hip.krylov_schur.KrylovSchurResult` plus ``lam``."""
        from .krylov_schur import KrylovSchurResult

        k = res.nout
        self.imag_norms = None
        if X is not None and k > 0:
            out = np.zeros(k, dtype=np.float64)
            if self.ctx._lib.lsa_krylov_imag_norms(self.handle, k, _ptr(out)) == 0:
                self.imag_norms = out
        vec = np.zeros((self.n, 0), dtype=np.complex128) if X is None else (X[:, :k] if k == max_out else np.asfortranarray(X[:, :k]))
        r = KrylovSchurResult(theta[:k].copy(), vec, est[:k].copy(), int(res.nconv), int(res.restarts), int(res.op_applies),
                              [{"nconv": int(res.nconv), "next_unconverged": float(res.next_unconverged), "seconds_expand": res.seconds_expand,
                                "seconds_dense": res.seconds_dense, "seconds_restart": res.seconds_restart}])
        r.lam = lam[:k].copy()
        return r

    def solve(self, nev: int, tol: float, max_restarts: int, which: int, transform: int, sigma: complex, *, antishift: complex = 0.0,
              target: complex | None = None, v0: np.ndarray | None = None, seed: int = 0, max_out: int | None = None, vectors: bool = True):
        """The whole Krylov-Schur iteration inside the library (``lsa_krylov_solve``: the dense algebra on the projected
        matrix is the library's own).  ``which``: EPSWhich code (``iEpsWhich.value``); ``transform``: 0 shift-invert,
        1 shift, 2 Cayley.  Returns a :class:`lsa_hip.krylov_schur.KrylovSchurResult` plus the eigenvalues ``lam``."""
        max_out = self.ncv if max_out is None else int(max_out)
        o = _ks_options(nev, tol, max_restarts, which, transform, sigma, antishift, target, seed)
        theta = np.zeros(max(max_out, 1), dtype=np.complex128)
        lam = np.zeros(max(max_out, 1), dtype=np.complex128)
        est = np.zeros(max(max_out, 1), dtype=np.float64)
        X = np.empty((self.n, max_out), dtype=np.complex128, order="F") if vectors else None
        res = lsa_ks_result()
        v = self._ks_start(v0)
        mask = None if self._mask is None else np.ascontiguousarray(self._mask, dtype=np.float64)
        self.ctx.check(self.ctx._lib.lsa_krylov_solve(self.ctx.handle, self.handle, ctypes.byref(o), None if v is None else _ptr(v),
                                                      None if mask is None else _ptr(mask), max_out, _ptr(theta), _ptr(lam),
                                                      None if X is None else _ptr(X), _ptr(est), ctypes.byref(res)))
        return self._ks_collect(res, theta, lam, est, X, max_out)

    @staticmethod
    def solve_batch(bases: "list[KrylovBasis]", nev: int, tol: float, max_restarts: int, which: int, transform: int, sigmas, *, antishift=0.0,
                    targets=None, v0s=None, seed: int = 0, max_out: int | None = None, vectors: bool = True, raise_on_error: bool = True, ctx: Context | None = None):
        """:meth:`solve` for up to 16 bases of one context and one shape in one library call (``lsa_krylov_solve_batch``): problems
        whose Arnoldi steps take the pipelined DCGS2 tail form on factors of one LU analysis advance in lockstep (one batched
        sweep pair and one batched reduction, update and tail launch per round for all of them), every problem returns the bits
        of its own :meth:`solve`.  ``sigmas`` (and ``targets``, ``v0s``, ``antishift`` when sequences): one per basis.

        Returns ``(results, info)``: the results in order, and the counters of ``lsa_ks_batch_info`` (``rounds``, ``launches``,
        ``periods``, ``launches_per_round``, ``lockstep_steps`` and ``solo_steps`` per problem).  A problem that failed raises
        (the first failing problem's status, with the texts of all failed problems, each naming its problem) unless
        ``raise_on_error`` is off: then its entry is its own exception and the others are results."""
        bases = list(bases)
        J = len(bases)
        per = lambda x, z: x[z] if isinstance(x, (list, tuple, np.ndarray)) and not np.isscalar(x) else x  # noqa: E731
        if any(b._mask is not None for b in bases):
            raise ValueError("solve_batch: bases with a mask (projected operators, sharded layout) are solved one by one")
        ctx = bases[0].ctx if J else ctx  # (``ctx``: only needed for an empty list, whose refusal is the library's too)
        max_out = (bases[0].ncv if J else 0) if max_out is None else int(max_out)
        opts = [_ks_options(nev, tol, max_restarts, which, transform, per(sigmas, z), per(antishift, z), None if targets is None else per(targets, z), seed)
                for z in range(J)]
        vs = [None if v0s is None else bases[z]._ks_start(v0s if isinstance(v0s, np.ndarray) and v0s.ndim == 1 else v0s[z]) for z in range(J)]
        theta = [np.zeros(max(max_out, 1), dtype=np.complex128) for _ in range(J)]
        lam = [np.zeros(max(max_out, 1), dtype=np.complex128) for _ in range(J)]
        est = [np.zeros(max(max_out, 1), dtype=np.float64) for _ in range(J)]
        X = [np.empty((b.n, max_out), dtype=np.complex128, order="F") if vectors else None for b in bases]
        res = (lsa_ks_result * max(J, 1))()
        status = (ctypes.c_int32 * max(J, 1))()
        info = lsa_ks_batch_info()
        arr = lambda ptrs: (ctypes.c_void_p * max(J, 1))(*ptrs)  # noqa: E731
        addr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        if ctx is None:
            raise ValueError("solve_batch needs at least one basis")
        rc = ctx._lib.lsa_krylov_solve_batch(ctx.handle, J, arr([b.handle.value for b in bases]), arr([ctypes.addressof(o) for o in opts]),
                                             arr([addr(v) for v in vs]), max_out, arr([addr(a) for a in theta]), arr([addr(a) for a in lam]),
                                             arr([addr(a) for a in X]), arr([addr(a) for a in est]), ctypes.byref(res), ctypes.byref(status),
                                             ctypes.byref(info))
        # (the context's error text after a failure: the texts of all failed problems in order, each naming its problem)
        text = ctx._lib.lsa_last_error(ctx.handle).decode(errors="replace") if rc != 0 else ""
        if rc != 0 and (raise_on_error or all(st == 0 for st in status)):
            ctx.check(rc)
        out = []
        for z, b in enumerate(bases):
            if status[z] != 0:
                mine = next((t for t in text.split("; ") if t.startswith(f"problem {z}:")), f"problem {z} failed: {text}")
                out.append(ValueError(mine) if status[z] == -1 else LsaError(status[z], mine))
            else:
                out.append(b._ks_collect(res[z], theta[z], lam[z], est[z], X[z], max_out))
        counters = {"rounds": int(info.rounds), "launches": int(info.launches), "periods": int(info.periods),
                    "launches_per_round": float(info.launches_per_round), "lockstep_steps": [int(info.lockstep_steps[z]) for z in range(J)],
                    "solo_steps": [int(info.solo_steps[z]) for z in range(J)]}
        return out, counters


class LanczosBasis(_LanczosHandle):
    """Real ``M``-orthonormal Lanczos basis in HBM for a symmetric-definite pencil (``lsa_lanczos_*``): the symmetric counterpart of
    :class:`KrylovBasis`.  ``op`` must be a shift-invert operator with real exact factors (``pc_type=2``, real shift)."""

    _prefix = "lanczos"
    set_start, extend, basis = _LanczosHandle._set_start, _LanczosHandle._extend, _LanczosHandle._basis

    def __init__(self, ctx: Context, op: ShiftInvertOperator, ncv: int):
        self.ctx, self._op = ctx, op
        self.n, self.ncv = op.n, int(ncv)
        h = ctypes.c_void_p()
        ctx.check(ctx._lib.lsa_lanczos_create(ctx.handle, op.handle, self.ncv, ctypes.byref(h)))
        self.handle = h

    def solve(self, nev: int, tol: float, max_restarts: int, which: int, sigma: float, *, target: float | None = None,
              v0: np.ndarray | None = None, seed: int = 0, max_out: int | None = None, vectors: bool = True):
        """The whole thick-restart Lanczos iteration inside the library (``lsa_lanczos_solve``).  Returns a
        :class:`lsa_hip.krylov_schur.KrylovSchurResult` with real ``theta``, real ``M``-orthonormal ``vectors`` and ``lam``."""
        from .krylov_schur import KrylovSchurResult

        max_out = self._max_out(max_out)
        o = _ks_options(nev, tol, max_restarts, which, sigma=float(sigma), target=None if target is None else float(target), seed=seed)
        theta = np.zeros(max(max_out, 1), dtype=np.float64)
        lam = np.zeros(max(max_out, 1), dtype=np.float64)
        X = np.empty((self.n, max_out), dtype=np.float64, order="F") if vectors else None
        k, t = self._solve(o, v0, max_out, theta, lam, X)
        vec = np.zeros((self.n, 0), dtype=np.float64) if X is None else (X[:, :k] if k == max_out else np.asfortranarray(X[:, :k]))
        r = KrylovSchurResult(theta[:k].copy(), vec, t["estimates"], t["nconv"], t["restarts"], t["applies"],
                              [{key: t[key] for key in ("nconv", "next_unconverged", "seconds_expand", "seconds_dense", "seconds_restart")}])
        r.lam = lam[:k].copy()
        return r


class ResolventBasis(_LanczosHandle):
    """Complex ``M``-orthonormal Lanczos basis in HBM for the resolvent's ``W = C^-1 M C^-H M``, ``C = A - i omega M``
    (``lsa_resolvent_*``): the counterpart of :class:`LanczosBasis` for optimal gains.  ``op`` must be a shift-invert operator
    (mode 0) at ``sigma = 1j * omega`` (or ``beta + 1j * omega``: the discounted resolvent) with exact factors (``pc_type=2``) and a
    real ``M``.  :meth:`set_weights` puts a forcing and a response weight where ``M`` stands: ``W = C^-1 Qf C^-H Qq``."""

    _prefix, _dtype, _counters = "resolvent", np.complex128, ("adjoint_solves", "forward_solves", "refined_adjoint", "refined_forward")
    set_start, extend, basis = _LanczosHandle._set_start, _LanczosHandle._extend, _LanczosHandle._basis

    def __init__(self, ctx: Context, op: ShiftInvertOperator, ncv: int):
        self.ctx, self._op = ctx, op
        self._weights = (None, None)
        self.n, self.ncv = op.n, int(ncv)
        h = ctypes.c_void_p()
        ctx.check(ctx._lib.lsa_resolvent_create(ctx.handle, op.handle, self.ncv, ctypes.byref(h)))
        self.handle = h

    def set_block_forcings(self, on: bool) -> None:
        """``True``: the forcings of :meth:`solve` take their adjoint solves as one block solve on the factors
        (``lsa_resolvent_set_block_forcings``); the results are those of the default, bit for bit."""
        self._call("set_block_forcings", int(bool(on)))

    def set_weights(self, forcing: "CsrMatrix | None" = None, response: "CsrMatrix | None" = None) -> None:
        """Forcing weight ``Q_f`` and response weight ``Q_q`` in place of ``M`` (``None``: ``M``; ``lsa_resolvent_set_weights``): real
        symmetric positive semidefinite ``n x n`` device matrices, which this object keeps alive.  A start vector (or :meth:`solve`)
        must follow."""
        self._call("set_weights", None if forcing is None else forcing.handle, None if response is None else response.handle)
        self._weights = (forcing, response)

    def solve(self, nev: int, tol: float, max_restarts: int, *, v0: np.ndarray | None = None, seed: int = 0, max_out: int | None = None,
              forcings: bool = True) -> dict:
        """The whole iteration inside the library (``lsa_resolvent_solve``).  Returns a dict: ``theta`` (``sigma_j^2``), ``gains``
        (descending), ``responses`` and ``forcings`` (n x k complex, ``M``-orthonormal; ``forcings`` is ``None`` when not asked for),
        ``estimates``, ``nconv``, ``restarts``, ``applies``, the loop's phase times and the handle's solve counts so far."""
        max_out = self._max_out(max_out)
        theta = np.zeros(max(max_out, 1), dtype=np.float64)
        gains = np.zeros(max(max_out, 1), dtype=np.float64)
        Q = np.empty((self.n, max_out), dtype=np.complex128, order="F")
        F = np.empty((self.n, max_out), dtype=np.complex128, order="F") if forcings else None
        k, tail = self._solve(_ks_options(nev, tol, max_restarts, seed=seed), v0, max_out, theta, gains, Q, F)
        return {"theta": theta[:k].copy(), "gains": gains[:k].copy(), "responses": np.asfortranarray(Q[:, :k]),
                "forcings": None if F is None else np.asfortranarray(F[:, :k]), **tail}

    @staticmethod
    def extend_batch(bases: "list[ResolventBasis]", j0s, j1: int, Ts: "list[np.ndarray]", raise_on_error: bool = True):
        """:meth:`extend` for up to 16 bases of one context and shape in one library call (``lsa_resolvent_extend_batch``): basis ``z``
        from its own ``j0s[z]`` to the common ``j1`` into its own Fortran-ordered ``Ts[z]``, in lockstep rounds where the members'
        factors allow; every basis is left with the bits of its own :meth:`extend`.  Returns ``(breakdowns, statuses)``.  For tests."""
        bases = list(bases)
        J = len(bases)
        if J == 0 or len(j0s) != J or len(Ts) != J:
            raise ValueError("extend_batch needs one start column and one T per basis (at least one)")
        ctx = bases[0].ctx
        for T in Ts:
            assert T.flags.f_contiguous and T.dtype == np.float64 and T.shape[0] == Ts[0].shape[0]
        j0 = (ctypes.c_int32 * J)(*[int(j) for j in j0s])
        bd = (ctypes.c_int32 * J)()
        status = (ctypes.c_int32 * J)()
        arr = lambda ptrs: (ctypes.c_void_p * J)(*ptrs)  # noqa: E731
        rc = ctx._lib.lsa_resolvent_extend_batch(ctx.handle, J, arr([b.handle.value for b in bases]), None, j0, int(j1), arr([T.ctypes.data for T in Ts]),
                                                 Ts[0].shape[0], bd, status)
        if rc != 0 and (raise_on_error or all(st == 0 for st in status)):
            ctx.check(rc)
        return [int(b) for b in bd], [int(s) for s in status]

    @staticmethod
    def solve_batch(bases: "list[ResolventBasis]", nevs, tol, max_it, *, v0s=None, seed: int = 0, max_out: int | None = None, forcings=True,
                    raise_on_error: bool = True, ctx: Context | None = None):
        """:meth:`solve` for up to 16 bases of one context and one shape in one library call (``lsa_resolvent_solve_batch``): the
        frequencies whose factors are complex and of one LU analysis advance in lockstep -- one batched launch per launch of a solo
        step and one read-back per round for all of them --, every basis returns the bits of its own :meth:`solve`.  ``nevs``,
        ``tol``, ``max_it`` (the restarts allowed), ``forcings`` and ``v0s``: one value for all, or one per basis.

        Returns ``(results, info)``: the dicts of :meth:`solve` in order, and the counters of ``lsa_ks_batch_info`` (``rounds``,
        ``launches``, ``periods``, ``launches_per_round``, ``lockstep_steps`` and ``solo_steps`` per basis).  A basis that failed
        raises (the first failing one's status, with the texts of all failed ones, each naming its problem) unless
        ``raise_on_error`` is off: then its entry is its own exception and the others are results."""
        bases = list(bases)
        J = len(bases)
        per = lambda x, z: x[z] if isinstance(x, (list, tuple, np.ndarray)) and not np.isscalar(x) else x  # noqa: E731
        ctx = bases[0].ctx if J else ctx  # (``ctx``: only needed for an empty list, whose refusal is the library's too)
        if ctx is None:
            raise ValueError("solve_batch needs at least one basis")
        max_out = (bases[0].ncv if J else 0) if max_out is None else min(int(max_out), bases[0].ncv if J else 0)
        opts = [_ks_options(int(per(nevs, z)), float(per(tol, z)), int(per(max_it, z)), seed=seed) for z in range(J)]
        vs = [None if v0s is None else bases[z]._start(v0s if isinstance(v0s, np.ndarray) and v0s.ndim == 1 else v0s[z]) for z in range(J)]
        theta = [np.zeros(max(max_out, 1), dtype=np.float64) for _ in range(J)]
        gains = [np.zeros(max(max_out, 1), dtype=np.float64) for _ in range(J)]
        est = [np.zeros(max(max_out, 1), dtype=np.float64) for _ in range(J)]
        Q = [np.empty((b.n, max_out), dtype=np.complex128, order="F") for b in bases]
        F = [np.empty((b.n, max_out), dtype=np.complex128, order="F") if per(forcings, z) else None for z, b in enumerate(bases)]
        res = (lsa_ks_result * max(J, 1))()
        status = (ctypes.c_int32 * max(J, 1))()
        counts = np.zeros((max(J, 1), 4), dtype=np.int64)
        info = lsa_ks_batch_info()
        arr = lambda ptrs: (ctypes.c_void_p * max(J, 1))(*ptrs)  # noqa: E731
        addr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        rc = ctx._lib.lsa_resolvent_solve_batch(ctx.handle, J, arr([None if b is None else b.handle.value for b in bases]),
                                                arr([ctypes.addressof(o) for o in opts]), arr([addr(v) for v in vs]), max_out, arr([addr(a) for a in theta]),
                                                arr([addr(a) for a in gains]), arr([addr(a) for a in Q]), arr([addr(a) for a in F]),
                                                arr([addr(a) for a in est]), ctypes.byref(res), _ptr(counts), ctypes.byref(status), ctypes.byref(info))
        text = ctx._lib.lsa_last_error(ctx.handle).decode(errors="replace") if rc != 0 else ""
        if rc != 0 and (raise_on_error or all(st == 0 for st in status)):
            ctx.check(rc)
        out = []
        for z, b in enumerate(bases):
            if status[z] != 0:
                # (the joined text is cut only in front of a problem's prefix: a member's own message may hold "; ")
                mine = next((t for t in re.split(r"; (?=problem \d+: )", text) if t.startswith(f"problem {z}:")), f"problem {z} failed: {text}")
                out.append(ValueError(mine) if status[z] == -1 else LsaError(status[z], mine))
                continue
            r, k = res[z], res[z].nout
            out.append({"theta": theta[z][:k].copy(), "gains": gains[z][:k].copy(), "responses": np.asfortranarray(Q[z][:, :k]),
                        "forcings": None if F[z] is None else np.asfortranarray(F[z][:, :k]), "estimates": est[z][:k].copy(), "nconv": int(r.nconv),
                        "restarts": int(r.restarts), "applies": int(r.op_applies), "next_unconverged": float(r.next_unconverged),
                        "seconds_expand": r.seconds_expand, "seconds_dense": r.seconds_dense, "seconds_restart": r.seconds_restart,
                        **{name: int(c) for name, c in zip(ResolventBasis._counters, counts[z])}})
        counters = {"rounds": int(info.rounds), "launches": int(info.launches), "periods": int(info.periods),
                    "launches_per_round": float(info.launches_per_round), "lockstep_steps": [int(info.lockstep_steps[z]) for z in range(J)],
                    "solo_steps": [int(info.solo_steps[z]) for z in range(J)]}
        return out, counters


class ContourSolver(_Handle):
    """Contour-integral subspace iteration for the eigenvalues of ``(A, M)`` inside an ellipse (``lsa_contour_*``): ``nodes``
    factorisations of ``A - z_k M`` on one LU analysis, kept alive (``keep_factors=True``) or refactorised node by node in every
    iteration; both return the same bytes.  ``A`` and ``M`` share one pattern, ``M`` is real."""

    _prefix = "contour"

    def __init__(self, ctx: Context, A: CsrMatrix, M: CsrMatrix, nodes: int, centre: complex, rx: float, ry: float, subspace: int, *,
                 keep_factors: bool = True, ksp_rtol: float = 1e-12, batch_nodes: bool = False):
        self.ctx, self._keep = ctx, (A, M)  # (the handle borrows both matrices)
        self.n, self.subspace, self.nodes = A.shape[0], int(subspace), int(nodes)
        centre = complex(centre)
        h = ctypes.c_void_p()
        ctx.check(ctx._lib.lsa_contour_create(ctx.handle, A.handle, None if M is None else M.handle, self.nodes, (_DBL * 2)(centre.real, centre.imag),
                                              (_DBL * 2)(float(rx), float(ry)), self.subspace, int(bool(keep_factors)), float(ksp_rtol), ctypes.byref(h)))
        self.handle = h
        if batch_nodes:
            self.set_batch_nodes(True)

    def set_batch_nodes(self, on: bool) -> None:
        """``True``: an iteration solves its block on all nodes in lockstep, in runs of up to 16 factor sets per launch
        (``lsa_contour_set_batch_nodes``); needs ``keep_factors`` and one more ``n x subspace`` block per node.  Same bytes as off."""
        self.ctx.check(self.ctx._lib.lsa_contour_set_batch_nodes(self.ctx.handle, self.handle, int(bool(on))))

    def batch_info(self) -> dict:
        """``lsa_contour_batch_info``: ``enabled``, ``groups`` (batched groups launched), ``batched_columns`` and
        ``serial_columns`` (column solves done in batches / node by node)."""
        st = lsa_contour_batch_stats()
        self.ctx.check(self.ctx._lib.lsa_contour_batch_info(self.handle, ctypes.byref(st)))
        return {"enabled": bool(st.enabled), "groups": st.groups, "batched_columns": st.batched_columns, "serial_columns": st.serial_columns}

    def set_row_permutation(self, perm: np.ndarray | None) -> None:
        """``perm[i]`` = the caller's index of row ``i``: the vectors of :meth:`solve` come back in the caller's numbering."""
        p = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
        self.ctx.check(self.ctx._lib.lsa_contour_set_row_permutation(self.ctx.handle, self.handle, None if p is None else _ptr(p)))

    def solve(self, tol: float, max_it: int, Y0: np.ndarray, max_out: int | None = None, _entry: str = "lsa_contour_solve") -> dict:
        """The iteration from the start block ``Y0`` (``n x subspace``, the matrices' own row numbering).  Returns the Ritz pairs
        inside the ellipse (``eigenvalues``, ``eigenvectors``, ``residuals``) and the fields of ``lsa_contour_result``."""
        Y0 = np.asfortranarray(Y0, dtype=np.complex128)
        if Y0.shape != (self.n, self.subspace):
            raise ValueError(f"the start block must have shape ({self.n}, {self.subspace}), got {Y0.shape}")
        max_out = self.subspace if max_out is None else min(int(max_out), self.subspace)
        lam = np.zeros(max(max_out, 1), dtype=np.complex128)
        res = np.zeros(max(max_out, 1), dtype=np.float64)
        X = np.empty((self.n, max_out), dtype=np.complex128, order="F")
        out = lsa_contour_result()
        self.ctx.check(getattr(self.ctx._lib, _entry)(self.ctx.handle, self.handle, float(tol), int(max_it), _ptr(Y0), max_out, _ptr(lam), _ptr(X),
                                                      _ptr(res), ctypes.byref(out)))
        k = out.nout
        d = {name: getattr(out, name) for name, _ in lsa_contour_result._fields_}
        d["complete"] = bool(out.complete)
        d.update(eigenvalues=lam[:k].copy(), eigenvectors=np.asfortranarray(X[:, :k]), residuals=res[:k].copy())
        return d

    def solve_left(self, tol: float, max_it: int, Y0: np.ndarray, max_out: int | None = None) -> dict:
        """The left phase on the same factor sets (``lsa_contour_solve_left``): the iteration of :meth:`solve` on the adjoint pencil.
        ``eigenvalues`` are the values in the caller's region, ``eigenvectors`` the left eigenvectors ``w`` (``w^H A = lambda w^H M``),
        ``residuals`` those of ``A^H w = conj(lambda) M^H w``.  The books of :meth:`info` and :meth:`batch_info` are left as they were:
        the left phases' are in :meth:`left_info`."""
        return self.solve(tol, max_it, Y0, max_out, _entry="lsa_contour_solve_left")

    def left_info(self) -> dict:
        """``lsa_contour_left_info``: what the left phases of this handle did and took."""
        st = lsa_contour_left_stats()
        self.ctx.check(self.ctx._lib.lsa_contour_left_info(self.handle, ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in lsa_contour_left_stats._fields_}

    def info(self) -> dict:
        """``lsa_contour_info``: kept or refactorised factor sets, device bytes of the handle's own buffers, the phase times, and the
        column solves' counters under ``"solver"``."""
        st = lsa_contour_stats()
        self.ctx.check(self.ctx._lib.lsa_contour_info(self.handle, ctypes.byref(st)))
        d = {name: getattr(st, name) for name, _ in lsa_contour_stats._fields_ if name != "solver"}
        d["kept"] = bool(st.kept)
        d["solver"] = {name: getattr(st.solver, name) for name, _ in lsa_stats._fields_}
        return d


def shifted_spmm(ctx: Context, A: CsrMatrix, M: CsrMatrix, shifts, X: np.ndarray, *, _entry: str = "lsa_shifted_spmm") -> np.ndarray:
    """``Y[:, k] = (A - shifts[k] M) X[:, k]`` for all columns in one launch (``lsa_shifted_spmm``): ``A``, ``M`` real on one
    pattern, ``X`` an ``n x N`` complex block on the host; returns ``Y`` on the host."""
    z = np.ascontiguousarray(shifts, dtype=np.complex128).ravel()
    X = np.asfortranarray(X, dtype=np.complex128)
    n = A.shape[0]
    if X.shape != (n, z.size):
        raise ValueError(f"the block must have shape ({n}, {z.size}), got {X.shape}")
    dX = DeviceVector.from_numpy(ctx, X.ravel(order="F"))
    dY = DeviceVector(ctx, n * z.size, np.complex128)
    ctx.check(getattr(ctx._lib, _entry)(ctx.handle, A.handle, M.handle, z.size, _ptr(z), dX.handle, dY.handle))
    return dY.numpy().reshape((n, z.size), order="F")


def shifted_spmm_transpose(ctx: Context, A: CsrMatrix, M: CsrMatrix, shifts, X: np.ndarray) -> np.ndarray:
    """``Y[:, k] = (A - shifts[k] M)^H X[:, k]`` for all columns in one launch on the pattern's transposed index
    (``lsa_shifted_spmm_transpose``); arguments as :func:`shifted_spmm`."""
    return shifted_spmm(ctx, A, M, shifts, X, _entry="lsa_shifted_spmm_transpose")


class StochasticBasis(_LanczosHandle):
    """Real Lanczos basis in HBM for the stochastic-forcing operator ``S = (1 / pi) sum_k w_k Re(C_k^-1 Qf C_k^-H Qq)``,
    ``C_k = A - z_k M`` (``lsa_stochastic_*``): ``len(shifts)`` factorisations kept alive on one LU analysis behind every step.
    ``A`` and ``M`` are real and share one pattern.  ``kind`` 0: EOFs (``Qq`` the inner product), 1: stochastic optimals (the two
    solves and the two weights swapped, ``Qf`` the inner product).  The results are those of the quadrature given."""

    _prefix, _counters = "stochastic", ("adjoint_solves", "forward_solves", "refined_adjoint", "refined_forward")

    def __init__(self, ctx: Context, A: CsrMatrix, M: CsrMatrix, shifts, weights, ncv: int, *, ksp_rtol: float = 1e-12):
        self.ctx, self._keep = ctx, (A, M)  # (the handle borrows both matrices)
        self._weights = (None, None)
        self.shifts = np.ascontiguousarray(shifts, dtype=np.complex128).ravel()
        self.weights = np.ascontiguousarray(weights, dtype=np.float64).ravel()
        if self.shifts.size != self.weights.size:
            raise ValueError(f"{self.shifts.size} nodes and {self.weights.size} weights")
        self.n, self.ncv, self.nodes = A.shape[0], int(ncv), int(self.shifts.size)
        h = ctypes.c_void_p()
        ctx.check(ctx._lib.lsa_stochastic_create(ctx.handle, A.handle, None if M is None else M.handle, self.nodes, _ptr(self.shifts), _ptr(self.weights),
                                                 self.ncv, float(ksp_rtol), ctypes.byref(h)))
        self.handle = h

    def set_weights(self, forcing: "CsrMatrix | None" = None, response: "CsrMatrix | None" = None) -> None:
        """Forcing weight ``Q_f`` and response weight ``Q_q`` in place of ``M`` (``None``: ``M``; ``lsa_stochastic_set_weights``): real
        symmetric positive semidefinite ``n x n`` device matrices, which this object keeps alive."""
        self._call("set_weights", None if forcing is None else forcing.handle, None if response is None else response.handle)
        self._weights = (forcing, response)

    def set_kind(self, kind: int) -> None:
        self._call("set_kind", int(kind))

    def set_batch_forward(self, on: bool) -> None:
        """``True``: the forward solves of a step run through the batched sweeps of ``lsa_ndlu_solve_batch``; same bits."""
        self._call("set_batch_forward", int(bool(on)))

    def set_batch_adjoint(self, on: bool) -> None:
        """``True``: the adjoint solves of a step run through the batched transposed sweeps of ``lsa_ndlu_solve_batch_adjoint`` and
        their check products through ``lsa_spmv_transpose_batch``; same bits."""
        self._call("set_batch_adjoint", int(bool(on)))

    def set_refinement(self, on: bool) -> None:
        """``True``: every solve carries the refinement step from the start (for tests)."""
        self._call("set_refinement", int(bool(on)))

    def apply(self, v: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """``(S v, node terms)`` for a host vector in the matrices' own row numbering (``lsa_stochastic_apply``); the node terms sum
        to ``v^T Q S v``."""
        v = np.ascontiguousarray(v, dtype=np.float64)
        if v.shape != (self.n,):
            raise ValueError(f"the vector must have shape ({self.n},)")
        y, terms = np.empty(self.n), np.zeros(self.nodes)
        self._call("apply", _ptr(v), _ptr(y), _ptr(terms))
        return y, terms

    def solve(self, nev: int, tol: float, max_restarts: int, *, v0: np.ndarray | None = None, seed: int = 0, max_out: int | None = None) -> dict:
        """The whole iteration inside the library (``lsa_stochastic_solve``).  Returns a dict: ``variances`` (descending), ``modes``
        (n x k real, orthonormal in the kind's weight), ``estimates``, ``nconv``, ``restarts``, ``applies``, the loop's phase times
        and the handle's solve counts so far."""
        max_out = self._max_out(max_out)
        theta = np.zeros(max(max_out, 1), dtype=np.float64)
        X = np.empty((self.n, max_out), dtype=np.float64, order="F")
        k, tail = self._solve(_ks_options(nev, tol, max_restarts, seed=seed), v0, max_out, theta, X)
        return {"variances": theta[:k].copy(), "modes": np.asfortranarray(X[:, :k]), **tail}

    def probes(self, nprobes: int, seed: int = 0) -> np.ndarray:
        """The ``n x nprobes`` Rademacher probes of ``seed`` in the caller's row numbering (``lsa_stochastic_probes``): entry ``(i, p)``
        is a pure function of ``(seed, p, i)``, whatever the row permutation."""
        nprobes = int(nprobes)
        if nprobes < 1:
            raise ValueError(f"nprobes = {nprobes} must be at least 1")
        Z = np.empty((self.n, nprobes), dtype=np.float64, order="F")
        self._call("probes", nprobes, ctypes.c_uint64(int(seed)), _ptr(Z))
        return Z

    def trace(self, nprobes: int, seed: int = 0, probes: np.ndarray | None = None, modes: np.ndarray | None = None, batch: int = 0) -> dict:
        """Block-probe forms for the trace of the quadrature operator (``lsa_stochastic_trace``): ``forms[r] = z_r^T S p_r`` (kind 1:
        ``S'``) with ``p = z - U (U^T Q z)`` for the modes ``U`` given (``n x d``, the caller's numbering, orthonormal in the kind's
        weight; ``None``: ``p = z``), so that ``tr S = sum(theta) + E[forms]``.  ``probes``: ``n x nprobes`` real in the caller's
        numbering (``None``: the Rademacher probes of ``seed``).  Returns a dict: ``forms`` (``nprobes``), ``node_terms``
        (``nodes x nprobes``, the columns sum to ``forms``) and ``stats`` (``lsa_stochastic_trace_stats``)."""
        nprobes = int(nprobes)
        Z = U = None
        if probes is not None:
            Z = np.asfortranarray(probes, dtype=np.float64)
            if Z.shape != (self.n, nprobes):
                raise ValueError(f"the probes must have shape ({self.n}, {nprobes}), got {Z.shape}")
        d = 0
        if modes is not None:
            U = np.asfortranarray(modes, dtype=np.float64)
            if U.ndim != 2 or U.shape[0] != self.n:
                raise ValueError(f"the modes must have shape ({self.n}, d), got {U.shape}")
            d = U.shape[1]
        forms, terms = np.zeros(max(nprobes, 1)), np.zeros((self.nodes, max(nprobes, 1)))
        st = lsa_stochastic_trace_stats()
        self._call("trace", nprobes, ctypes.c_uint64(int(seed)), None if Z is None else _ptr(Z), d, None if U is None or d == 0 else _ptr(U), int(batch),
                   _ptr(forms), _ptr(terms), ctypes.byref(st))
        return {"forms": forms[:nprobes], "node_terms": terms[:, :nprobes], "stats": {name: getattr(st, name) for name, _ in lsa_stochastic_trace_stats._fields_}}

    def info(self) -> dict:
        """``lsa_stochastic_info``: nodes, kind, device bytes, the phase times, and the inner solves' counters under ``"solver"``."""
        st = lsa_stochastic_stats()
        self.ctx.check(self.ctx._lib.lsa_stochastic_info(self.handle, ctypes.byref(st)))
        d = {name: getattr(st, name) for name, _ in lsa_stochastic_stats._fields_ if name != "solver"}
        d["solver"] = {name: getattr(st.solver, name) for name, _ in lsa_stats._fields_}
        return d


class GrowthBasis(_LanczosHandle):
    """Real ``M``-orthonormal Lanczos basis in HBM for the transient-growth operator ``W = Phi+ Phi``, ``Phi = (-sigma C^-1 M)^N``,
    ``C = A - sigma M``, ``sigma = 1 / dt`` (``lsa_growth_*``): a march of ``2 N`` solves on one factorisation behind every step.
    ``op`` must be a shift-invert operator (mode 0) at the real positive ``sigma`` with real exact factors (``pc_type=2``) and a real
    ``M``; ``keep`` is the 0/1 mask of the free dofs in the operator's row numbering (``None``: all ones).  ``scheme="sdirk2"``
    (``lsa_growth_set_scheme``) marches by the L-stable two-stage SDIRK method with ``gamma = 1 - 1/sqrt(2)`` instead of implicit Euler:
    second order in ``dt``, ``sigma = 1 / (gamma dt)``, ``Phi = (S (a S + b I))^N`` with ``S = -sigma C^-1 M``, ``4 N`` solves a step."""

    SCHEMES = {"euler": 0, "sdirk2": 1}
    _prefix, _counters = "growth", ("forward_solves", "transposed_solves", "refined_forward", "refined_transposed")
    set_start, extend, basis = _LanczosHandle._set_start, _LanczosHandle._extend, _LanczosHandle._basis

    def __init__(self, ctx: Context, op: ShiftInvertOperator, ncv: int, nsteps: int, keep: np.ndarray | None = None, scheme: str = "euler"):
        if scheme not in self.SCHEMES:
            raise ValueError(f"scheme must be one of {sorted(self.SCHEMES)}, got {scheme!r}")
        self.ctx, self._op = ctx, op
        self._weight = None
        self.n, self.ncv, self.nsteps = op.n, int(ncv), int(nsteps)
        self.scheme = "euler"
        k = None
        if keep is not None:
            k = np.ascontiguousarray(keep, dtype=np.float64)
            if k.shape != (self.n,):
                raise ValueError(f"keep must have shape ({self.n},)")
        h = ctypes.c_void_p()
        ctx.check(ctx._lib.lsa_growth_create(ctx.handle, op.handle, self.ncv, self.nsteps, None if k is None else _ptr(k), ctypes.byref(h)))
        self.handle = h
        if scheme != "euler":
            self.set_scheme_code(self.SCHEMES[scheme])

    def set_scheme_code(self, code: int) -> None:
        """``lsa_growth_set_scheme`` with the bare code (0: implicit Euler, 1: SDIRK2); any other is the library's ``ValueError``."""
        self._call("set_scheme", int(code))
        self.scheme = {v: k for k, v in self.SCHEMES.items()}[int(code)]

    def set_response_weight(self, Q: "CsrMatrix | None") -> None:
        """The response weight ``Q`` in place of ``M`` at the horizon (``None``: ``M``; ``lsa_growth_set_response_weight``): the gains
        become ``max ||q(T)||_Q^2 / ||q(0)||_M^2``.  A real symmetric positive semidefinite ``n x n`` device matrix, kept alive here."""
        self._call("set_response_weight", None if Q is None else Q.handle)
        self._weight = Q

    def set_steps(self, nsteps: int) -> None:
        """Another horizon of ``nsteps`` steps on the same handle and factors."""
        self._call("set_steps", int(nsteps))
        self.nsteps = int(nsteps)

    def solve(self, nev: int, tol: float, max_restarts: int, *, v0: np.ndarray | None = None, seed: int = 0, max_out: int | None = None) -> dict:
        """The whole iteration inside the library (``lsa_growth_solve``).  Returns a dict: ``gains`` (descending), ``initial``
        (n x k, ``M``-orthonormal), ``responses`` (n x k, ``Phi q0``), ``energy`` (k x (nsteps + 1), the ``M``-energy),
        ``response_energy`` (k, the energy at ``T`` in the response weight), ``estimates``, ``nconv``,
        ``restarts``, ``applies``, the loop's phase times and the handle's solve counts so far."""
        max_out = self._max_out(max_out)
        theta = np.zeros(max(max_out, 1), dtype=np.float64)
        gains = np.zeros(max(max_out, 1), dtype=np.float64)
        Q0 = np.zeros((self.n, max_out), dtype=np.float64, order="F")
        QT = np.zeros((self.n, max_out), dtype=np.float64, order="F")
        energy = np.zeros((max(max_out, 1), self.nsteps + 1), dtype=np.float64)
        k, tail = self._solve(_ks_options(nev, tol, max_restarts, seed=seed), v0, max_out, theta, gains, Q0, QT, energy)
        renergy = np.zeros(max(k, 1), dtype=np.float64)
        self._call("response_energy", k, _ptr(renergy))
        return {"gains": gains[:k].copy(), "initial": np.asfortranarray(Q0[:, :k]), "responses": np.asfortranarray(QT[:, :k]),
                "energy": energy[:k].copy(), "response_energy": renergy[:k].copy(), **tail}


def dense_syev(A: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Eigenvalues (ascending) and orthonormal eigenvectors of a real symmetric matrix by the library's own host routine
    (``lsa_dense_syev``: Householder tridiagonalisation + implicit QL; the lower triangle is read).  No GPU needed."""
    lib = load_library()
    Q = np.array(A, dtype=np.float64, order="F", copy=True)
    if Q.ndim != 2 or Q.shape[0] != Q.shape[1]:
        raise ValueError("dense_syev needs a square matrix")
    n = Q.shape[0]
    w = np.zeros(max(n, 1), dtype=np.float64)
    rc = lib.lsa_dense_syev(n, _ptr(Q), max(n, 1), _ptr(w))
    if rc != 0:
        raise LsaError(rc, "lsa_dense_syev failed")
    return w[:n], Q


def eigs_sinvert(ctx: Context, A: CsrMatrix, M: CsrMatrix | None, sigma: complex, nev: int, *, ncv: int = 0, tol: float = 1e-10, max_restarts: int = 500,
                 pc_type: int = 2, ksp_rtol: float = 1e-12, v0: np.ndarray | None = None, row_perm: np.ndarray | None = None):
    """``lsa_eigs_sinvert``: the eigenpairs of ``A x = lam M x`` nearest ``sigma`` from ONE library call on uploaded matrices
    (factorisation, Krylov-Schur, Ritz vectors).  Returns ``(lam, X, estimates, result dict, stats dict)``."""
    n = A.shape[0]
    nout = int(ncv) if ncv > 0 else max(2 * nev, nev + 15)
    nout = min(nout, n)
    opts = lsa_op_options(ilu_levels=2, ilu_shift=0.0, ksp_rtol=float(ksp_rtol), ksp_restart=min(200, max(n, 1)), ksp_maxit=4000, pc_type=int(pc_type),
                          antishift=(_DBL * 2)(0.0, 0.0))
    lam = np.zeros(max(nout, 1), dtype=np.complex128)
    est = np.zeros(max(nout, 1), dtype=np.float64)
    X = np.empty((n, nout), dtype=np.complex128, order="F")
    res, st = lsa_ks_result(), lsa_stats()
    v = None if v0 is None else np.ascontiguousarray(v0, dtype=np.complex128)
    p = None if row_perm is None else np.ascontiguousarray(row_perm, dtype=np.int32)
    sg = (_DBL * 2)(complex(sigma).real, complex(sigma).imag)
    ctx.check(ctx._lib.lsa_eigs_sinvert(ctx.handle, A.handle, None if M is None else M.handle, sg, int(nev), int(ncv), float(tol), int(max_restarts),
                                        ctypes.byref(opts), None if v is None else _ptr(v), None if p is None else _ptr(p), nout, _ptr(lam), _ptr(X),
                                        _ptr(est), ctypes.byref(res), ctypes.byref(st)))
    k = res.nout
    return (lam[:k].copy(), np.asfortranarray(X[:, :k]), est[:k].copy(),
            {"nconv": res.nconv, "restarts": res.restarts, "op_applies": res.op_applies, "next_unconverged": res.next_unconverged,
             "seconds_expand": res.seconds_expand, "seconds_dense": res.seconds_dense, "seconds_restart": res.seconds_restart},
            {name: getattr(st, name) for name, _ in lsa_stats._fields_})


def read_matrix_market(path) -> "scipy.sparse.csr_matrix":  # noqa: F821
    """Parse a MatrixMarket coordinate file with the native reader (host only, no GPU needed)."""
    import scipy.sparse as sp

    lib = load_library()
    h = ctypes.c_void_p()
    nr, nc, nnz, cx = _I32(0), _I32(0), _I64(0), ctypes.c_int(0)
    rc = lib.lsa_mm_open(str(path).encode(), ctypes.byref(h), ctypes.byref(nr), ctypes.byref(nc), ctypes.byref(nnz), ctypes.byref(cx))
    try:
        if rc != 0:
            raise ValueError(f"{path}: {lib.lsa_mm_error(h).decode(errors='replace')}")
        rp = np.empty(nr.value + 1, dtype=np.int32)
        ci = np.empty(nnz.value, dtype=np.int32)
        val = np.empty(nnz.value, dtype=np.complex128 if cx.value else np.float64)
        lib.lsa_mm_read_csr(h, _ptr(rp), _ptr(ci), _ptr(val))
    finally:
        lib.lsa_mm_close(h)
    return sp.csr_matrix((val, ci, rp), shape=(nr.value, nc.value))


def eig_residuals(ctx: Context, A: CsrMatrix, M: CsrMatrix | None, lam: np.ndarray, X: np.ndarray) -> np.ndarray:
    """Relative residuals of Solver/eigen2.py:48-56, evaluated on the device."""
    lam = np.ascontiguousarray(lam, dtype=np.complex128)
    X = np.asfortranarray(X, dtype=np.complex128)
    res = np.empty(lam.shape[0], dtype=np.float64)
    ctx.check(ctx._lib.lsa_eig_residuals(ctx.handle, A.handle, M.handle if M is not None else None, lam.shape[0], _ptr(lam), _ptr(X), _ptr(res)))
    return res


def eig_biorth(ctx: Context, M: CsrMatrix | None, X: np.ndarray, Z: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``lsa_eig_biorth``: ``G = Z^H M X`` (k x k), ``||z_j||`` and ``||M x_j||`` for host blocks ``X``, ``Z`` (n x k), evaluated on the
    device; ``M=None`` is the identity.  The products ``M x_j`` stay on the device (they are those of :meth:`CsrMatrix.matvec`)."""
    X = np.asfortranarray(X, dtype=np.complex128)
    Z = np.asfortranarray(Z, dtype=np.complex128)
    if X.ndim != 2 or X.shape != Z.shape:
        raise ValueError(f"eig_biorth: X {X.shape} and Z {Z.shape} must be two blocks of one shape (n, k)")
    n, k = X.shape
    G = np.zeros((k, k), dtype=np.complex128, order="F")
    norm_z, norm_mx = np.zeros(k, dtype=np.float64), np.zeros(k, dtype=np.float64)
    ctx.check(ctx._lib.lsa_eig_biorth(ctx.handle, M.handle if M is not None else None, n, k, _ptr(X), _ptr(Z), _ptr(G), _ptr(norm_z), _ptr(norm_mx)))
    return G, norm_z, norm_mx


def block_gram(ctx: Context, n: int, U: DeviceVector, p: int, W: DeviceVector, q: int, ldu: int | None = None, ldw: int | None = None) -> np.ndarray:
    """``lsa_block_gram``: ``G = U^H W`` (``p x q``, both at most 128) over ``n`` rows of two column-major complex128 blocks (column
    ``c`` at ``c * ld``, ``ld`` defaulting to ``n``), summed on the device in a fixed order.  ``U is W`` with one ``ld`` and one
    column count returns an exactly real diagonal."""
    G = np.zeros((int(p), int(q)), dtype=np.complex128, order="F")
    ctx.check(ctx._lib.lsa_block_gram(ctx.handle, int(n), int(p), U.handle, int(n if ldu is None else ldu), int(q), W.handle,
                                      int(n if ldw is None else ldw), _ptr(G)))
    return G
