"""m4ri_amd -- MI355X-native drop-in for M4RI's dense GF(2) multiply path.

The product is `libm4ri_amd.so` (HIP kernels for gfx950 + the host scheduler + a C ABI that exports
M4RI's own entry points, see include/m4ri_amd.h).  This package is the thin Python binding over that
C ABI: the functions below have M4RI's names and argument meaning (reference m4ri/strassen.h:52-126,
m4ri/brilliantrussian.h:274-317) and simply forward `Mzd` host matrices to the library.

There is no CPU implementation here: if the shared library is missing or there is no GPU, calls
fail loudly.
"""
from __future__ import annotations

import ctypes
import os

from .mzd import Mzd, MzdPtr, MzdStruct, from_struct_ptr, splitmix_words  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libm4ri_amd.so")
_lib = None


class Mzp(ctypes.Structure):
    """mzp_t (include/m4ri_amd.h; reference m4ri/mzp.h:37-49)."""

    _fields_ = [("values", ctypes.POINTER(ctypes.c_int32)), ("length", ctypes.c_int32)]


class ShardPlan(ctypes.Structure):
    """m4ri_amd_shard_plan (include/m4ri_amd.h part 4)."""

    _fields_ = [("world", ctypes.c_int32), ("levels", ctypes.c_int32), ("nprod", ctypes.c_int32), ("blocks", ctypes.c_int32),
                ("m", ctypes.c_int64), ("l", ctypes.c_int64), ("n", ctypes.c_int64),
                ("M", ctypes.c_int64), ("L", ctypes.c_int64), ("N", ctypes.c_int64),
                ("bm", ctypes.c_int64), ("bl", ctypes.c_int64), ("cwl", ctypes.c_int64), ("cwn", ctypes.c_int64)]


class ShardPiece(ctypes.Structure):
    """m4ri_amd_shard_piece."""

    _fields_ = [("holder", ctypes.c_int32), ("owner", ctypes.c_int32),
                ("holder_off", ctypes.c_int64), ("owner_off", ctypes.c_int64), ("words", ctypes.c_int64)]


(BUF_LOCAL_A, BUF_LOCAL_B, BUF_LOCAL_C, BUF_CHILD_A, BUF_CHILD_B, BUF_SLABS_P, BUF_OPER_A, BUF_OPER_B, BUF_PROD) = range(9)


class Stats(ctypes.Structure):
    """m4ri_amd_stats (include/m4ri_amd.h)."""

    _fields_ = [
        ("levels", ctypes.c_int32),
        ("leaf_launches", ctypes.c_int32),
        ("leaf_products", ctypes.c_int64),
        ("leaf_m", ctypes.c_int32),
        ("leaf_l", ctypes.c_int32),
        ("leaf_n", ctypes.c_int32),
        ("leaf_gen", ctypes.c_int32),
        ("leaf_ms", ctypes.c_double),
        ("leaf_bytes", ctypes.c_double),
        ("aux_bytes", ctypes.c_double),
        ("workspace_bytes", ctypes.c_double),
        ("cum_leaf_ms", ctypes.c_double),
        ("cum_leaf_launches", ctypes.c_int64),
    ]


class LeafPlan(ctypes.Structure):
    """m4ri_amd_leaf_plan (include/m4ri_amd.h): what one leaf launch of the engine does."""

    _fields_ = [("gen", ctypes.c_int32), ("rg", ctypes.c_int32), ("tile_rows", ctypes.c_int32), ("tile_words", ctypes.c_int32),
                ("tiles_m", ctypes.c_int64), ("tiles_n", ctypes.c_int64), ("tiles", ctypes.c_int64),
                ("ksplit", ctypes.c_int32), ("tail_ksplit", ctypes.c_int32), ("tail_tiles", ctypes.c_int64),
                ("mode", ctypes.c_int32), ("tail_mode", ctypes.c_int32),
                ("slabs", ctypes.c_int32), ("zero", ctypes.c_int32), ("pack_a", ctypes.c_int32), ("reserved", ctypes.c_int32)]

    def __repr__(self):
        return "LeafPlan(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_ if n != "reserved") + ")"


(ZERO_NOTHING, ZERO_ALL, ZERO_TAIL) = range(3)  # LeafPlan.zero


class DmatInfo(ctypes.Structure):
    """m4ri_amd_dmat_info_t."""

    _fields_ = [("rows", ctypes.c_int64), ("ncols", ctypes.c_int64), ("stride", ctypes.c_int64),
                ("layout", ctypes.c_int32), ("world", ctypes.c_int32), ("alive", ctypes.c_int32)]


class MultiStats(ctypes.Structure):
    """m4ri_amd_multi_stats."""

    _fields_ = [("world", ctypes.c_int32), ("variant", ctypes.c_int32), ("levels", ctypes.c_int32), ("sub_products", ctypes.c_int32),
                ("chunks", ctypes.c_int32), ("overlap", ctypes.c_int32), ("converted", ctypes.c_int32), ("pairs_staged", ctypes.c_int32),
                ("m", ctypes.c_int64), ("l", ctypes.c_int64), ("n", ctypes.c_int64), ("link_bytes", ctypes.c_double),
                ("group", ctypes.c_int32), ("reserved", ctypes.c_int32)]


(LAYOUT_ROWS, LAYOUT_CYCLIC1, LAYOUT_CYCLIC2, LAYOUT_REPLICATED) = range(4)
(VARIANT_AUTO, VARIANT_SLABS, VARIANT_STRASSEN) = range(3)
VARIANT_NAMES = {VARIANT_AUTO: "auto", VARIANT_SLABS: "slabs", VARIANT_STRASSEN: "strassen"}

# every symbol include/m4ri_amd.h declares, with its ctypes signature
_P = ctypes.c_void_p
_I64 = ctypes.c_int64
_I = ctypes.c_int
_MULSIG = (MzdPtr, [MzdPtr, MzdPtr, MzdPtr, _I])
_DEVSIG = (_I, [_P, _I64, _P, _I64, _P, _I64, _I64, _I64, _I64, _I, _I, _P])
SYMBOLS = {
    "mzd_mul": _MULSIG,
    "mzd_addmul": _MULSIG,
    "_mzd_mul_even": _MULSIG,
    "_mzd_addmul_even": _MULSIG,
    "_mzd_addmul": _MULSIG,
    "_mzd_sqr_even": (MzdPtr, [MzdPtr, MzdPtr, _I]),
    "_mzd_addsqr_even": (MzdPtr, [MzdPtr, MzdPtr, _I]),
    "mzd_mul_m4rm": _MULSIG,
    "mzd_addmul_m4rm": _MULSIG,
    "_mzd_mul_m4rm": (MzdPtr, [MzdPtr, MzdPtr, MzdPtr, _I, _I]),
    "mzd_mul_mp": _MULSIG,
    "mzd_addmul_mp": _MULSIG,
    "mzd_trsm_lower_left": (None, [MzdPtr, MzdPtr, _I]),
    "_mzd_trsm_lower_left": (None, [MzdPtr, MzdPtr, _I]),
    "_mzd_trsm_lower_left_russian": (None, [MzdPtr, MzdPtr, _I]),
    "mzd_trsm_upper_left": (None, [MzdPtr, MzdPtr, _I]),
    "_mzd_trsm_upper_left": (None, [MzdPtr, MzdPtr, _I]),
    "_mzd_trsm_upper_left_russian": (None, [MzdPtr, MzdPtr, _I]),
    "mzd_trsm_upper_right": (None, [MzdPtr, MzdPtr, _I]),
    "_mzd_trsm_upper_right": (None, [MzdPtr, MzdPtr, _I]),
    "mzd_trsm_lower_right": (None, [MzdPtr, MzdPtr, _I]),
    "_mzd_trsm_lower_right": (None, [MzdPtr, MzdPtr, _I]),
    "m4ri_amd_trsm_upper_right_dev": (_I, [_P, _I64, _P, _I64, _I64, _I64, _I, _P]),
    "m4ri_amd_trsm_lower_right_dev": (_I, [_P, _I64, _P, _I64, _I64, _I64, _I, _P]),
    "m4ri_amd_trsm_lower_left_dev": (_I, [_P, _I64, _P, _I64, _I64, _I64, _I, _P]),
    "m4ri_amd_trsm_upper_left_dev": (_I, [_P, _I64, _P, _I64, _I64, _I64, _I, _P]),
    "mzd_fprint_row": (None, [_P, MzdPtr, _I]),
    "mzd_fprint": (None, [_P, MzdPtr]),
    "mzd_print": (None, [MzdPtr]),
    "mzd_from_str": (MzdPtr, [_I, _I, ctypes.c_char_p]),
    "mzd_from_jcf": (MzdPtr, [ctypes.c_char_p, _I]),
    "mzd_from_png": (MzdPtr, [ctypes.c_char_p, _I]),
    "mzd_to_png": (_I, [MzdPtr, ctypes.c_char_p, _I, ctypes.c_char_p, _I]),
    "mzd_make_table": (None, [MzdPtr, _I, _I, _I, MzdPtr, _P]),
    "mzd_process_rows": (None, [MzdPtr, _I, _I, _I, _I] + [MzdPtr, _P] * 1),
    "mzd_process_rows2": (None, [MzdPtr, _I, _I, _I, _I] + [MzdPtr, _P] * 2),
    "mzd_process_rows3": (None, [MzdPtr, _I, _I, _I, _I] + [MzdPtr, _P] * 3),
    "mzd_process_rows4": (None, [MzdPtr, _I, _I, _I, _I] + [MzdPtr, _P] * 4),
    "mzd_process_rows5": (None, [MzdPtr, _I, _I, _I, _I] + [MzdPtr, _P] * 5),
    "mzd_process_rows6": (None, [MzdPtr, _I, _I, _I, _I] + [MzdPtr, _P] * 6),
    "m4ri_amd_process_rows_dev": (_I, [_P, _I64, _I64, _I64, _I64, _I64, _I, _P, _P, _P, _P, _P, _P]),
    "m4ri_amd_make_table_dev": (_I, [_P, _I64, _I64, _I64, _I64, _I64, _I, _P, _P, _I64, _P, _P]),
    "mzd_ple": (_I, [MzdPtr, ctypes.POINTER(Mzp), ctypes.POINTER(Mzp), _I]),
    "_mzd_ple": (_I, [MzdPtr, ctypes.POINTER(Mzp), ctypes.POINTER(Mzp), _I]),
    "_mzd_ple_russian": (_I, [MzdPtr, ctypes.POINTER(Mzp), ctypes.POINTER(Mzp), _I]),
    "mzd_pluq": (_I, [MzdPtr, ctypes.POINTER(Mzp), ctypes.POINTER(Mzp), _I]),
    "_mzd_pluq": (_I, [MzdPtr, ctypes.POINTER(Mzp), ctypes.POINTER(Mzp), _I]),
    "_mzd_pluq_russian": (_I, [MzdPtr, ctypes.POINTER(Mzp), ctypes.POINTER(Mzp), _I]),
    "mzd_apply_p_right_trans_tri": (None, [MzdPtr, ctypes.POINTER(Mzp)]),
    "mzd_apply_p_right": (None, [MzdPtr, ctypes.POINTER(Mzp)]),
    "mzd_apply_p_right_trans": (None, [MzdPtr, ctypes.POINTER(Mzp)]),
    "mzd_apply_p_left": (None, [MzdPtr, ctypes.POINTER(Mzp)]),
    "mzd_apply_p_left_trans": (None, [MzdPtr, ctypes.POINTER(Mzp)]),
    "mzd_solve_left": (_I, [MzdPtr, MzdPtr, _I, _I]),
    "_mzd_solve_left": (_I, [MzdPtr, MzdPtr, _I, _I]),
    "mzd_pluq_solve_left": (_I, [MzdPtr, _I, ctypes.POINTER(Mzp), ctypes.POINTER(Mzp), MzdPtr, _I, _I]),
    "_mzd_pluq_solve_left": (_I, [MzdPtr, _I, ctypes.POINTER(Mzp), ctypes.POINTER(Mzp), MzdPtr, _I, _I]),
    "mzd_kernel_left_pluq": (MzdPtr, [MzdPtr, _I]),
    "mzd_inv_m4ri": (MzdPtr, [MzdPtr, MzdPtr, _I]),
    "mzd_echelonize": (_I, [MzdPtr, _I]),
    "mzd_echelonize_m4ri": (_I, [MzdPtr, _I, _I]),
    "mzd_echelonize_pluq": (_I, [MzdPtr, _I]),
    "mzd_echelonize_naive": (_I, [MzdPtr, _I]),
    "_mzd_echelonize_m4ri": (_I, [MzdPtr, _I, _I, _I, ctypes.c_double]),
    "m4ri_amd_ple_dev": (_I, [_P, _I64, _I64, _I64, _P, _P, _P, _I64, _P]),
    "m4ri_amd_pluq_dev": (_I, [_P, _I64, _I64, _I64, _P, _P, _P, _I64, _P]),
    "m4ri_amd_apply_p_right_trans_tri_dev": (_I, [_P, _I64, _I64, _I64, _P, _P]),
    "m4ri_amd_apply_p_left_dev": (_I, [_P, _I64, _I64, _I64, _P, _I64, _I, _P]),
    "m4ri_amd_pluq_solve_left_dev": (_I, [_P, _I64, _I64, _I64, ctypes.c_int32, _P, _P, _P, _I64, _I64, _I64, _I, _I, _P, _P]),
    "m4ri_amd_solve_left_dev": (_I, [_P, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I, _I, _P, _P]),
    "m4ri_amd_kernel_left_pluq_dev": (_I, [_P, _I64, _I64, _I64, _P, _I64, _I, _P, _P]),
    "m4ri_amd_inv_dev": (_I, [_P, _I64, _P, _I64, _I64, _P]),
    "mzd_transpose": (MzdPtr, [MzdPtr, MzdPtr]),
    "mzd_trtri_upper": (MzdPtr, [MzdPtr]),
    "mzd_trtri_upper_russian": (MzdPtr, [MzdPtr, _I]),
    "m4ri_amd_transpose_dev": (_I, [_P, _I64, _P, _I64, _I64, _I64, _P]),
    "m4ri_amd_transpose_batch_dev": (_I, [_P, _I64, _I64, _P, _I64, _I64, _I64, _I64, _I64, _P]),
    "m4ri_amd_plan_transpose_batch": (_I, [_I64, _I64]),
    "m4ri_amd_weight_batch_dev": (_I, [_P, _I64, _I64, _P, _I64, _I64, _I64, _I64, _I64, _P, _P, _P, _P]),
    "m4ri_amd_mismatch_batch_dev": (_I, [_P, _I64, _I64, _P, _I64, _I64, _I64, _I64, _I64, _P, _P]),
    "m4ri_amd_row_span_batch_dev": (_I, [_P, _I64, _I64, _I64, _I64, _I64, _P, _P, _P]),
    "m4ri_amd_plan_reduce_batch": (_I, [_I64, _I64]),
    "m4ri_amd_rowspace_weights_batch_dev": (_I, [_P, _I64, _I64, _I64, _I64, _P, _I64, _I64, _I64, _P, _P, _P]),
    "m4ri_amd_plan_rowspace_weights_batch": (_I, [_I64, _I64]),
    "m4ri_amd_row_sums_weights_batch_dev": (_I, [_P, _I64, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I64, _P, _P, _P]),
    "m4ri_amd_plan_row_sums_weights_batch": (_I, [_I64, _I64, _I64]),
    "m4ri_amd_row_sums_collide_batch_dev": (_I, [_P, _I64, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _I64, _P, _P, _P]),
    "m4ri_amd_row_sums_collide_list_batch_dev": (_I, [_P, _I64, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I64, _P, _P, _P,
                                                      _I64, _I64, _P, _P]),
    "m4ri_amd_row_sums_words_batch_dev": (_I, [_P, _I64, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _P, _P, _I64, _I64, _P, _P]),
    "m4ri_amd_plan_row_sums_collide_batch": (_I, [_I64, _I64, _I64, _I64, _I64, _I64]),
    "m4ri_amd_row_sums_collide_slices": (_I64, [_I64, _I64, _I64, _I64, _I64, _I64, _I64]),
    "m4ri_amd_lists_collide_batch_dev": (_I, [_P, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _I64, _I64, _P, _P, _P, _I64,
                                              _I64, _P, _P]),
    "m4ri_amd_plan_lists_collide_batch": (_I, [_I64, _I64, _I64, _I64, _I64]),
    "m4ri_amd_lists_collide_units": (_I, [_I64, _I64, _I64, _I64, _I64, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "m4ri_amd_lists_words_batch_dev": (_I, [_P, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _P, _P, _I64, _I64, _P, _P]),
    "m4ri_amd_sort_rows_batch_dev": (_I, [_P, _I64, _I64, _I64, _I64, _P, _I64, _P, _I64, _I64, _P, _P, _P, _P, _I64, _P, _I64, _P]),
    "m4ri_amd_plan_sort_rows_batch": (_I, [_I64, _I64, _I64, _I64]),
    "m4ri_amd_sort_rows_units": (_I, [_I64, _I64, _I64, _I64, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "m4ri_amd_sort_rows_scratch_bytes": (_I64, [_I64, _I64, _I64, _I64]),
    "m4ri_amd_copy_block_batch_dev": (_I, [_P, _I64, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _P]),
    "m4ri_amd_extract_tri_batch_dev": (_I, [_P, _I64, _I64, _P, _I64, _I64, _I64, _I64, _I64, _I, _I, _P, _P]),
    "m4ri_amd_apply_p_left_batch_dev": (_I, [_P, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _I, _P, _P]),
    "m4ri_amd_apply_p_right_batch_dev": (_I, [_P, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _I, _P, _P]),
    "m4ri_amd_plan_perm_batch": (_I, [_I64, _I64, _I]),
    "m4ri_amd_m4rm_batch_dev": (_I, [_P, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _I64, _I64, _I64, _I64, _I, _P]),
    "m4ri_amd_mul_batch_dev": (_I, [_P, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _I64, _I64, _I64, _I64, _I, _I, _P]),
    "m4ri_amd_mul_small_batch_dev": (_I, [_P, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _I64, _I64, _I64, _I64, _I, _P]),
    "m4ri_amd_plan_mul_small_batch": (_I, [_I64, _I64, _I64]),
    "m4ri_amd_mul_small_batch_op_dev": (_I, [_P, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _I64, _I64, _I64, _I64, _I, _I, _I, _P]),
    "m4ri_amd_plan_mul_small_batch_op": (_I, [_I64, _I64, _I64, _I, _I]),
    "m4ri_amd_model_seconds_batch": (ctypes.c_double, [_I64, _I64, _I64, _I, _I64]),
    "m4ri_amd_trtri_upper_dev": (_I, [_P, _I64, _I64, _P]),
    "m4ri_amd_echelonize_dev": (_I, [_P, _I64, _I64, _I64, _I, _P, _P]),
    "m4ri_amd_echelonize_batch_dev": (_I, [_P, _I64, _I64, _I64, _I64, _I64, _I, _P, _P, _P]),
    "m4ri_amd_plan_echelonize_batch": (_I, [_I64, _I64]),
    "m4ri_amd_echelonize_order_batch_dev": (_I, [_P, _I64, _I64, _P, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I, _P, _P, _P]),
    "m4ri_amd_plan_echelonize_order_batch": (_I, [_I64, _I64]),
    "m4ri_amd_random_orders_batch_dev": (_I, [_P, _I64, _I64, _I64, ctypes.c_uint64, _P]),
    "m4ri_amd_pivot_exchange_batch_dev": (_I, [_P, _I64, _I64, _I64, _I64, _I64, _P, _P, _I64, _P, _I64, _I64, ctypes.c_uint64, _P, _I64, _I64, _P, _P]),
    "m4ri_amd_plan_pivot_exchange_batch": (_I, [_I64, _I64, _I64]),
    "m4ri_amd_isd_search_dev": (_I, [_P, _I64, _I64, _I64, _I64, _I64, _P, _P, _I64, _I64, _I64, ctypes.c_uint64, _I64, _I64, _I64, _P, _I64, _I64, _P, _P, _P,
                                     _P, _P, _I64, _P]),
    "m4ri_amd_plan_isd_search": (_I, [_I64, _I64, _I64, _I64]),
    "m4ri_amd_isd_collide_search_dev": (_I, [_P, _I64, _I64, _I64, _I64, _I64, _P, _P, _I64, _I64, _I64, ctypes.c_uint64, _I64, _I64, _I64, _I64, _I64, _I64, _P,
                                             _I64, _I64, _P, _P, _P, _P, _P, _I64, _P]),
    "m4ri_amd_plan_isd_collide_search": (_I, [_I64, _I64, _I64, _I64, _I64, _I64, _I64]),
    "m4ri_amd_solve_left_batch_dev": (_I, [_P, _I64, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I64, _P, _P, _P]),
    "m4ri_amd_inv_batch_dev": (_I, [_P, _I64, _I64, _P, _I64, _I64, _I64, _I64, _P, _P]),
    "m4ri_amd_plan_solve_batch": (_I, [_I64, _I64, _I64]),
    "m4ri_amd_kernel_left_batch_dev": (_I, [_P, _I64, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I64, _P, _P]),
    "m4ri_amd_plan_kernel_batch": (_I, [_I64, _I64]),
    "m4ri_amd_ple_batch_dev": (_I, [_P, _I64, _I64, _I64, _I64, _I64, _I, _P, _P, _P, _P]),
    "m4ri_amd_plan_ple_batch": (_I, [_I64, _I64]),
    "m4ri_amd_pluq_solve_left_batch_dev": (_I, [_P, _I64, _I64, _I64, _I64, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _P, _P]),
    "m4ri_amd_plan_pluq_solve_batch": (_I, [_I64, _I64, _I64]),
    "m4ri_amd_apply_p_right_dev": (_I, [_P, _I64, _I64, _I64, _P, _I64, _I, _P]),
    "m4ri_amd_mzd_init": (MzdPtr, [_I, _I]),
    "m4ri_amd_mzd_free": (None, [MzdPtr]),
    "m4ri_amd_result_free": (None, [MzdPtr]),
    "m4ri_amd_init": (_I, [_I]),
    "m4ri_amd_device_count": (_I, []),
    "m4ri_amd_mul_dev": _DEVSIG,
    "m4ri_amd_m4rm_dev": _DEVSIG,
    "m4ri_amd_xor_dev": (_I, [_P, _I64, _P, _I64, _P, _I64, _I64, _I64, _P]),
    "m4ri_amd_fill_dev": (_I, [_P, _I64, _I64, _I64, ctypes.c_uint64, _P]),
    "m4ri_amd_mask_tail_dev": (_I, [_P, _I64, _I64, _I64, _P]),
    "m4ri_amd_set_profiling": (None, [_I]),
    "m4ri_amd_set_max_fuse": (_I, [_I]),
    "m4ri_amd_plan_levels": (_I, [_I64, _I64, _I64, _I]),
    "m4ri_amd_plan_small_leaf": (_I, [_I64, _I64, _I64, _I64, _I]),
    "m4ri_amd_plan_leaf_launch": (_I, [_I64, _I64, _I64, _I64, _I, _I, _I, _I, _I, ctypes.POINTER(LeafPlan)]),
    "m4ri_amd_plan_row_blocks": (_I, [_I64, _I64, _I64, ctypes.c_void_p, ctypes.c_void_p, _I]),
    "m4ri_amd_model_seconds": (ctypes.c_double, [_I64, _I64, _I64, _I]),
    "m4ri_amd_set_workspace_budget": (_I64, [_I64]),
    "m4ri_amd_set_host_pipeline": (_I64, [_I64]),
    "m4ri_amd_plan_host_pipeline": (_I, [_I64, _I64, _I64, _I64, _I, _I, _I, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _I, ctypes.c_void_p, ctypes.c_void_p]),
    "m4ri_amd_pin": (_I, [MzdPtr]),
    "m4ri_amd_sync": (_I, [MzdPtr]),
    "m4ri_amd_host_modified": (_I, [MzdPtr]),
    "m4ri_amd_unpin": (_I, [MzdPtr]),
    "m4ri_amd_is_pinned": (_I, [MzdPtr]),
    "m4ri_amd_get_stats": (_I, [ctypes.POINTER(Stats)]),
    "m4ri_amd_shard_plan_make": (_I, [ctypes.POINTER(ShardPlan), _I, _I64, _I64, _I64, _I]),
    "m4ri_amd_shard_cut": (_I64, [_I64, _I, _I]),
    "m4ri_amd_shard_owner": (_I, [ctypes.POINTER(ShardPlan), _I]),
    "m4ri_amd_shard_group": (_I, [ctypes.POINTER(ShardPlan), _I]),
    "m4ri_amd_shard_slab_rows": (_I64, [ctypes.POINTER(ShardPlan), _I, _I]),
    "m4ri_amd_shard_buffer_words": (_I64, [ctypes.POINTER(ShardPlan), _I, _I]),
    "m4ri_amd_shard_piece_of": (_I, [ctypes.POINTER(ShardPlan), _I, _I, _I, ctypes.POINTER(ShardPiece)]),
    "m4ri_amd_shard_down_dev": (_I, [ctypes.POINTER(ShardPlan), _I, _P, _I64, _P, _I64, _P, _P, _P]),
    "m4ri_amd_shard_up_dev": (_I, [ctypes.POINTER(ShardPlan), _I, _P, _P, _I64, _I, _P]),
    "m4ri_amd_fill_rows_dev": (_I, [_P, _I64, _I64, _I64, _I64, ctypes.c_uint64, _P]),
    "m4ri_amd_mul_multi": (_I, [MzdPtr, MzdPtr, MzdPtr, _I, _I, _I]),
    "m4ri_amd_set_devices": (_I, [_I, ctypes.POINTER(_I)]),
    "m4ri_amd_get_device_list": (_I, [ctypes.POINTER(_I), _I]),
    "m4ri_amd_set_multi_threshold": (_I64, [_I64]),
    "m4ri_amd_release_workspace": (None, []),
    "m4ri_amd_set_small_product_threshold": (_I64, [_I64]),
    "m4ri_amd_small_product_count": (_I64, []),
    "m4ri_amd_small_product_wanted": (_I, [_I64, _I64, _I64]),
    "m4ri_amd_small_mul_host": (_I, [MzdPtr, MzdPtr, MzdPtr, _I]),
    "m4ri_amd_dmat_create": (_P, [_I64, _I64, _I]),
    "m4ri_amd_dmat_free": (None, [_P]),
    "m4ri_amd_dmat_info": (_I, [_P, ctypes.POINTER(DmatInfo)]),
    "m4ri_amd_dmat_local": (_I, [_P, _I, ctypes.POINTER(_P), ctypes.POINTER(_I64), ctypes.POINTER(_I)]),
    "m4ri_amd_dmat_fill": (_I, [_P, ctypes.c_uint64]),
    "m4ri_amd_dmat_upload": (_I, [_P, MzdPtr]),
    "m4ri_amd_dmat_download": (_I, [_P, MzdPtr]),
    "m4ri_amd_dmat_convert": (_I, [_P, _P]),
    "m4ri_amd_dmat_mul": (_I, [_P, _P, _P, _I, _I, _I]),
    "m4ri_amd_dmat_mul_lane": (_I, [_P, _P, _P, _I, _I, _I, _I]),
    "m4ri_amd_multi_sync": (_I, []),
    "m4ri_amd_multi_pair_table": (None, [_I, ctypes.POINTER(ctypes.c_int), _I, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_char_p]),
    "m4ri_amd_multi_link_probe": (_I, [_I64, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]),
    "m4ri_amd_multi_get_stats": (_I, [ctypes.POINTER(MultiStats)]),
    "m4ri_amd_multi_timeline": (_I, [_I, ctypes.POINTER(ctypes.c_double), _I]),
    "m4ri_amd_multi_default_variant": (_I, [_I, _I64, _I64, _I64]),
    "m4ri_amd_multi_layout_for": (_I, [_I, _I, _I64, _I64, _I64]),
    "m4ri_amd_layout_local_rows": (_I64, [_I, _I, _I, _I64]),
    "m4ri_amd_layout_runs": (_I, [_I, _I, _I, _I64, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64), _I]),
    "m4ri_amd_set_multi_variant": (_I, [_I]),
}


def lib() -> ctypes.CDLL:
    """Load libm4ri_amd.so (RTLD_LOCAL: its M4RI-named symbols must not interpose a libm4ri that
    happens to be loaded in the same process, e.g. the reference build used as the test oracle)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m m4ri_amd.build` (hipcc, gfx950). "
                "m4ri_amd has no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_LOCAL)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the ABI lost a symbol
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def _p(m: Mzd | None):
    return m.ptr if m is not None else None


def _ret(C: Mzd | None, r) -> Mzd:
    if C is not None:
        return C
    return from_struct_ptr(r, lib().m4ri_amd_result_free)


# ---- M4RI-named host entry points ---------------------------------------------------------------
def mzd_mul(C: Mzd | None, A: Mzd, B: Mzd, cutoff: int = 0) -> Mzd:
    """C = A*B (strassen.h:52).  C=None allocates.  Fatal (abort) on dimension mismatch, like M4RI."""
    return _ret(C, lib().mzd_mul(_p(C), A.ptr, B.ptr, cutoff))


def mzd_addmul(C: Mzd | None, A: Mzd, B: Mzd, cutoff: int = 0) -> Mzd:
    """C += A*B (strassen.h:68)."""
    return _ret(C, lib().mzd_addmul(_p(C), A.ptr, B.ptr, cutoff))


def _mzd_mul_even(C: Mzd, A: Mzd, B: Mzd, cutoff: int) -> Mzd:
    lib()._mzd_mul_even(C.ptr, A.ptr, B.ptr, cutoff)
    return C


def _mzd_addmul_even(C: Mzd, A: Mzd, B: Mzd, cutoff: int) -> Mzd:
    lib()._mzd_addmul_even(C.ptr, A.ptr, B.ptr, cutoff)
    return C


def _mzd_addmul(C: Mzd, A: Mzd, B: Mzd, cutoff: int) -> Mzd:
    lib()._mzd_addmul(C.ptr, A.ptr, B.ptr, cutoff)
    return C


def mzd_mul_m4rm(C: Mzd | None, A: Mzd, B: Mzd, k: int = 0) -> Mzd:
    """C = A*B by one M4RM leaf, no Strassen (brilliantrussian.h:274).  k is a hint only."""
    return _ret(C, lib().mzd_mul_m4rm(_p(C), A.ptr, B.ptr, k))


def mzd_addmul_m4rm(C: Mzd, A: Mzd, B: Mzd, k: int = 0) -> Mzd:
    lib().mzd_addmul_m4rm(C.ptr, A.ptr, B.ptr, k)
    return C


def _mzd_mul_m4rm(C: Mzd, A: Mzd, B: Mzd, k: int, clear: int) -> Mzd:
    lib()._mzd_mul_m4rm(C.ptr, A.ptr, B.ptr, k, clear)
    return C


def mzd_mul_mp(C: Mzd | None, A: Mzd, B: Mzd, cutoff: int = 0) -> Mzd:
    return _ret(C, lib().mzd_mul_mp(_p(C), A.ptr, B.ptr, cutoff))


def mzd_addmul_mp(C: Mzd | None, A: Mzd, B: Mzd, cutoff: int = 0) -> Mzd:
    return _ret(C, lib().mzd_addmul_mp(_p(C), A.ptr, B.ptr, cutoff))


# ---- triangular solves (reference m4ri/triangular.h:115-153, m4ri/triangular_russian.h:43, :55) -------
def mzd_trsm_lower_left(L: Mzd, B: Mzd, cutoff: int = 0) -> Mzd:
    """B <- L^-1 B in place, L unit lower triangular (only the bits below its diagonal are read)."""
    lib().mzd_trsm_lower_left(L.ptr, B.ptr, cutoff)
    return B


def mzd_trsm_upper_left(U: Mzd, B: Mzd, cutoff: int = 0) -> Mzd:
    """B <- U^-1 B in place, U unit upper triangular (only the bits above its diagonal are read)."""
    lib().mzd_trsm_upper_left(U.ptr, B.ptr, cutoff)
    return B


def mzd_ple(A: Mzd, cutoff: int = 0, which: str = "mzd_ple"):
    """PLE decomposition of A in place (reference m4ri/ple.h:103); returns (rank, P, Q) with P, Q numpy int32
    arrays of A.nrows / A.ncols transpositions."""
    import numpy as np
    P, Q = np.zeros(max(1, A.nrows), dtype=np.int32), np.zeros(max(1, A.ncols), dtype=np.int32)
    mp, mq = Mzp(), Mzp()
    mp.values, mp.length = P.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), A.nrows
    mq.values, mq.length = Q.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), A.ncols
    r = getattr(lib(), which)(A.ptr, ctypes.byref(mp), ctypes.byref(mq), cutoff)
    return int(r), P[:A.nrows], Q[:A.ncols]


def mzd_echelonize(A: Mzd, full: int, which: str = "mzd_echelonize", k: int = 0) -> int:
    """(Reduced) row echelon form of A in place, returns the rank (reference m4ri/echelonform.h:50, :63, :79)."""
    if which == "mzd_echelonize_m4ri":
        return int(lib().mzd_echelonize_m4ri(A.ptr, int(full), k))
    if which == "_mzd_echelonize_m4ri":
        return int(lib()._mzd_echelonize_m4ri(A.ptr, int(full), k, 0, 1.0))
    return int(getattr(lib(), which)(A.ptr, int(full)))


def mzd_apply_p_right(A: Mzd, P, trans: bool = False) -> None:
    """A <- A * P (or A * P^T): the column transpositions (i, P[i]) on every row (reference m4ri/mzp.h:142, :153)."""
    import numpy as np
    p = np.ascontiguousarray(P, dtype=np.int32)
    mp = Mzp()
    mp.values, mp.length = p.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(p)
    (lib().mzd_apply_p_right_trans if trans else lib().mzd_apply_p_right)(A.ptr, ctypes.byref(mp))


def _mzp(values):
    import numpy as np
    v = np.ascontiguousarray(values, dtype=np.int32)
    mp = Mzp()
    mp.values, mp.length = v.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(v)
    return mp, v


def mzd_apply_p_left(A: Mzd, P, trans: bool = False) -> None:
    """The row transpositions (i, P[i]) on A, ascending (or descending: trans) -- reference m4ri/mzp.h:120, :131."""
    mp, keep = _mzp(P)
    (lib().mzd_apply_p_left_trans if trans else lib().mzd_apply_p_left)(A.ptr, ctypes.byref(mp))


def mzd_solve_left(A: Mzd, B: Mzd, cutoff: int = 0, inconsistency_check: bool = False, which: str = "mzd_solve_left") -> int:
    """A X = B in place (reference m4ri/solve.h:50): A <- its PLUQ, B <- X with the undefined rows zero; 0 or -1."""
    return int(getattr(lib(), which)(A.ptr, B.ptr, cutoff, int(inconsistency_check)))


def mzd_pluq_solve_left(A: Mzd, rank: int, P, Q, B: Mzd, cutoff: int = 0, inconsistency_check: bool = False, which: str = "mzd_pluq_solve_left") -> int:
    mp, kp = _mzp(P)
    mq, kq = _mzp(Q)
    return int(getattr(lib(), which)(A.ptr, rank, ctypes.byref(mp), ctypes.byref(mq), B.ptr, cutoff, int(inconsistency_check)))


def mzd_kernel_left_pluq(A: Mzd, cutoff: int = 0):
    """A <- its PLUQ; returns the ncols x (ncols - rank) kernel basis or None (reference m4ri/solve.h:140)."""
    r = lib().mzd_kernel_left_pluq(A.ptr, cutoff)
    return from_struct_ptr(r, lib().m4ri_amd_result_free) if r else None


def mzd_inv_m4ri(A: Mzd, B: Mzd = None) -> Mzd:
    """B <- A^-1 (reference m4ri/brilliantrussian.h:256)."""
    r = lib().mzd_inv_m4ri(B.ptr if B is not None else None, A.ptr, 0)
    return B if B is not None else from_struct_ptr(r, lib().m4ri_amd_result_free)


def mzd_transpose(A: Mzd, DST: Mzd = None) -> Mzd:
    """DST <- A^T (reference m4ri/mzd.h:611)."""
    r = lib().mzd_transpose(DST.ptr if DST is not None else None, A.ptr)
    return DST if DST is not None else from_struct_ptr(r, lib().m4ri_amd_result_free)


def mzd_trtri_upper(A: Mzd, which: str = "mzd_trtri_upper") -> Mzd:
    """A <- A^-1 in place, A unit upper triangular (reference m4ri/triangular.h:163, triangular_russian.h:66)."""
    if which == "mzd_trtri_upper":
        lib().mzd_trtri_upper(A.ptr)
    else:
        lib().mzd_trtri_upper_russian(A.ptr, 0)
    return A


def mzd_apply_p_right_trans_tri(A: Mzd, Q) -> None:
    """Row r of A <- its columns under the transpositions (i, Q[i]), i > r (reference m4ri/mzp.h:202)."""
    import numpy as np
    q = np.ascontiguousarray(Q, dtype=np.int32)
    mq = Mzp()
    mq.values, mq.length = q.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(q)
    lib().mzd_apply_p_right_trans_tri(A.ptr, ctypes.byref(mq))


# ---- I/O formats (reference m4ri/io.h) ---------------------------------------------------------------
def mzd_from_str(m: int, n: int, s: str) -> Mzd:
    return from_struct_ptr(lib().mzd_from_str(m, n, s.encode()), lib().m4ri_amd_result_free)


def mzd_from_jcf(path: str, verbose: int = 0):
    r = lib().mzd_from_jcf(os.fsencode(path), verbose)
    return from_struct_ptr(r, lib().m4ri_amd_result_free) if r else None


def mzd_from_png(path: str, verbose: int = 0):
    r = lib().mzd_from_png(os.fsencode(path), verbose)
    return from_struct_ptr(r, lib().m4ri_amd_result_free) if r else None


def mzd_to_png(A: Mzd, path: str, compression_level: int = -1, comment: str = "", verbose: int = 0) -> int:
    return int(lib().mzd_to_png(A.ptr, os.fsencode(path), compression_level, comment.encode(), verbose))


# ---- device-resident API -------------------------------------------------------------------------
def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"m4ri_amd: {what} failed with hipError_t {rc}")


def init(device: int = 0) -> None:
    _check(lib().m4ri_amd_init(device), "m4ri_amd_init")


def mul_dev(C: int, c_stride: int, A: int, a_stride: int, B: int, b_stride: int, m: int, l: int, n: int,
            add: bool = False, cutoff: int = 0, stream: int = 0) -> None:
    """C (+)= A*B on device pointers (ints), Strassen-Winograd over batched M4RM leaves."""
    _check(lib().m4ri_amd_mul_dev(C, c_stride, A, a_stride, B, b_stride, m, l, n, int(add), cutoff, stream), "m4ri_amd_mul_dev")


def mul_batch_dev(C: int, c_stride: int, c_bs: int, A: int, a_stride: int, a_bs: int, B: int, b_stride: int, b_bs: int, m: int, l: int, n: int,
                  batch: int, add: bool = False, cutoff: int = 0, stream: int = 0) -> None:
    """`batch` products of one shape, X_b = X + b * x_bs words, with the levels of mul_dev and every launch shared by the batch."""
    _check(lib().m4ri_amd_mul_batch_dev(C, c_stride, c_bs, A, a_stride, a_bs, B, b_stride, b_bs, m, l, n, batch, int(add), cutoff, stream),
           "m4ri_amd_mul_batch_dev")


def mul_small_batch_dev(C: int, c_stride: int, c_bs: int, A: int, a_stride: int, a_bs: int, B: int, b_stride: int, b_bs: int, m: int, l: int,
                        n: int, batch: int, add: bool = False, stream: int = 0) -> None:
    """`batch` products of tiny matrices, C_b (+)= A_b * B_b with X_b = X + b * x_bs words (a_bs = 0 / b_bs = 0: one shared A / B; A == B
    allowed), only the valid bits of C written.  Asynchronous, lock-free and capturable on paths 0-1 of plan_mul_small_batch; path 2 is
    m4ri_amd_m4rm_batch_dev's launch."""
    _check(lib().m4ri_amd_mul_small_batch_dev(C, c_stride, c_bs, A, a_stride, a_bs, B, b_stride, b_bs, m, l, n, batch, int(bool(add)), stream),
           "m4ri_amd_mul_small_batch_dev")


def plan_mul_small_batch(m: int, l: int, n: int) -> int:
    """The path mul_small_batch_dev takes for (m, l, n) (0 wave per member, 1 wave per 64 x 64 block of C, 2 forwarded). Host arithmetic."""
    return int(lib().m4ri_amd_plan_mul_small_batch(m, l, n))


def mul_small_batch_op_dev(C: int, c_stride: int, c_bs: int, A: int, a_stride: int, a_bs: int, B: int, b_stride: int, b_bs: int, m: int, l: int,
                           n: int, batch: int, trans_a: bool = False, trans_b: bool = False, add: bool = False, stream: int = 0) -> None:
    """mul_small_batch_dev with transposed operands, C_b (m x n) (+)= op(A_b) * op(B_b): trans_a: A_b is stored l x m, trans_b: B_b is
    stored n x l (B == A allowed: A A^T, A^T A).  One launch, no scratch, only the valid bits of C written.  With a transposed operand
    there is no path 2: beyond plan_mul_small_batch_op's bound the call raises (hipErrorNotSupported, 801) and touches nothing."""
    _check(lib().m4ri_amd_mul_small_batch_op_dev(C, c_stride, c_bs, A, a_stride, a_bs, B, b_stride, b_bs, m, l, n, batch, int(bool(trans_a)),
                                                 int(bool(trans_b)), int(bool(add)), stream), "m4ri_amd_mul_small_batch_op_dev")


def plan_mul_small_batch_op(m: int, l: int, n: int, trans_a: bool = False, trans_b: bool = False) -> int:
    """The path mul_small_batch_op_dev takes (0 wave per member, 1 wave per 64 x 64 block of C, 2 forwarded -- with a transposed operand:
    not supported). Host arithmetic."""
    return int(lib().m4ri_amd_plan_mul_small_batch_op(m, l, n, int(bool(trans_a)), int(bool(trans_b))))


def transpose_batch_dev(D: int, d_stride: int, d_bs: int, A: int, a_stride: int, a_bs: int, nrows: int, ncols: int, batch: int, stream: int = 0) -> None:
    """`batch` transposes of small matrices, D_b = (A_b)^T with X_b = X + b * x_bs words (A_b nrows x ncols, D_b ncols x nrows); D == A
    allowed for square members up to 1024 with equal strides.  Asynchronous, lock-free and capturable on every path of
    plan_transpose_batch; paths 0-1 write only the valid bits of D, path 2 whole last words (m4ri_amd_transpose_dev's contract)."""
    _check(lib().m4ri_amd_transpose_batch_dev(D, d_stride, d_bs, A, a_stride, a_bs, nrows, ncols, batch, stream), "m4ri_amd_transpose_batch_dev")


def plan_transpose_batch(nrows: int, ncols: int) -> int:
    """The path an out-of-place transpose_batch_dev takes for (nrows, ncols) (0 wave per member, 1 wave per 64 x 64 block, 2 the tile
    kernel). Host arithmetic."""
    return int(lib().m4ri_amd_plan_transpose_batch(nrows, ncols))


def weight_batch_dev(A: int, a_stride: int, a_bs: int, B: int, b_stride: int, b_bs: int, nrows: int, ncols: int, batch: int, total: int = 0,
                     row_weight: int = 0, lightest: int = 0, stream: int = 0) -> None:
    """Hamming weights of `batch` matrices A_b (B = 0) or distances of A_b ^ B_b, X_b = X + b * x_bs words (x_bs = 0: one shared
    operand), valid bits only, operands read only.  DEVICE outputs, each 0 = not wanted, not all: total (int64 per member), row_weight
    (int32, batch * nrows), lightest (int64 per member: (smallest row weight << 32) | its first row).  Asynchronous, lock-free and
    capturable on every path of plan_reduce_batch."""
    _check(lib().m4ri_amd_weight_batch_dev(A, a_stride, a_bs, B or None, b_stride, b_bs, nrows, ncols, batch, total or None, row_weight or None,
                                           lightest or None, stream), "m4ri_amd_weight_batch_dev")


def mismatch_batch_dev(A: int, a_stride: int, a_bs: int, B: int, b_stride: int, b_bs: int, nrows: int, ncols: int, batch: int, first_row: int,
                       stream: int = 0) -> None:
    """first_row[b] (DEVICE int32 per member) = the first row at which A_b and B_b differ in a valid bit, -1 if none (mzd_equal).
    Asynchronous, lock-free and capturable on every path of plan_reduce_batch."""
    _check(lib().m4ri_amd_mismatch_batch_dev(A, a_stride, a_bs, B, b_stride, b_bs, nrows, ncols, batch, first_row or None, stream),
           "m4ri_amd_mismatch_batch_dev")


def row_span_batch_dev(A: int, a_stride: int, a_bs: int, nrows: int, ncols: int, batch: int, first_nonzero: int = 0, end_nonzero: int = 0,
                       stream: int = 0) -> None:
    """DEVICE int32 outputs per member, each 0 = not wanted, not both: first_nonzero[b] = the first non-zero row of A_b (nrows if none),
    end_nonzero[b] = one past the last (mzd_first_zero_row; 0 = mzd_is_zero).  Asynchronous, lock-free and capturable on every path of
    plan_reduce_batch."""
    _check(lib().m4ri_amd_row_span_batch_dev(A, a_stride, a_bs, nrows, ncols, batch, first_nonzero or None, end_nonzero or None, stream),
           "m4ri_amd_row_span_batch_dev")


def plan_reduce_batch(nrows: int, ncols: int) -> int:
    """The path weight_batch_dev, mismatch_batch_dev and row_span_batch_dev take for (nrows, ncols) (0 wave per member, 1 workgroup per
    member, 2 chunks of rows and atomics). Host arithmetic."""
    return int(lib().m4ri_amd_plan_reduce_batch(nrows, ncols))


def rowspace_weights_batch_dev(G: int, g_stride: int, g_bs: int, k: int, n: int, V: int, v_bs: int, batch: int, w_min: int = 0, hist: int = 0,
                               lightest: int = 0, stream: int = 0) -> None:
    """The weights of all 2^k words c_b(x) = V_b ^ x * G_b of `batch` generators G_b (k x n, k <= 40, n <= 1024; g_bs = 0: one shared G;
    V = 0: no V; v_bs = 0: one shared V), valid bits only, operands read only.  DEVICE int64 outputs, each 0 = not wanted, not both:
    hist (batch * (n + 1): the number of messages x per weight), lightest (per member: the minimum of (wt << 40) | x over wt >= w_min,
    -1 if none).  Asynchronous, lock-free and capturable on both paths of plan_rowspace_weights_batch."""
    _check(lib().m4ri_amd_rowspace_weights_batch_dev(G or None, g_stride, g_bs, k, n, V or None, v_bs, batch, w_min, hist or None, lightest or None,
                                                     stream), "m4ri_amd_rowspace_weights_batch_dev")


def plan_rowspace_weights_batch(k: int, n: int) -> int:
    """The path rowspace_weights_batch_dev takes for (k, n) (0 a wave per member, 1 a member's messages spread over many waves and
    global atomics). Host arithmetic."""
    return int(lib().m4ri_amd_plan_rowspace_weights_batch(k, n))


def row_sums_weights_batch_dev(G: int, g_stride: int, g_bs: int, k: int, n: int, V: int, v_bs: int, batch: int, t: int, w_min: int = 0,
                               hist: int = 0, lightest: int = 0, stream: int = 0) -> None:
    """The weights of all C(k, t) words c_b(S) = V_b ^ (the sum of the t rows of G_b in S) of `batch` generators G_b (k x n, k <= 1024,
    n <= 1024, t <= 8, C(k, t) <= 2^40; g_bs = 0: one shared G; V = 0: no V; v_bs = 0: one shared V), valid bits only, operands read
    only.  DEVICE int64 outputs, each 0 = not wanted, not both: hist (batch * (n + 1): the number of sets S per weight), lightest (per
    member: the minimum of (wt << 40) | colexicographic rank of S over wt >= w_min, -1 if none; row_subset_unrank gives the rows).
    Asynchronous, lock-free and capturable on both paths of plan_row_sums_weights_batch."""
    _check(lib().m4ri_amd_row_sums_weights_batch_dev(G or None, g_stride, g_bs, k, n, V or None, v_bs, batch, t, w_min, hist or None,
                                                     lightest or None, stream), "m4ri_amd_row_sums_weights_batch_dev")


def plan_row_sums_weights_batch(k: int, n: int, t: int) -> int:
    """The path row_sums_weights_batch_dev takes for (k, n, t) (0 a wave per member, 1 a member's sums spread over many waves and
    global atomics). Host arithmetic."""
    return int(lib().m4ri_amd_plan_row_sums_weights_batch(k, n, t))


def row_subset_rank(rows) -> int:
    """The colexicographic rank sum_j C(i_j, j + 1) of the set of distinct row indices `rows` (any order): the low 40 bits of
    row_sums_weights_batch_dev's lightest."""
    from math import comb
    s = sorted(int(i) for i in rows)
    if any(i < 0 for i in s) or any(a == b for a, b in zip(s, s[1:])):
        raise ValueError("row_subset_rank: the rows must be distinct and not negative")
    return sum(comb(i, j + 1) for j, i in enumerate(s))


def row_subset_unrank(rank: int, t: int) -> tuple:
    """The t row indices i_0 < ... < i_{t-1} of colexicographic rank `rank`: the inverse of row_subset_rank."""
    from math import comb
    if rank < 0 or t < 0 or (t == 0 and rank != 0):
        raise ValueError("row_subset_unrank: no such set")
    out = []
    for m in range(t, 0, -1):  # the largest i with C(i, m) <= rank
        lo, hi = m - 1, m
        while comb(hi, m) <= rank:
            lo, hi = hi, 2 * hi
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if comb(mid, m) <= rank else (lo, mid)
        out.append(lo)
        rank -= comb(lo, m)
    return tuple(reversed(out))


def row_sums_collide_batch_dev(G: int, g_stride: int, g_bs: int, k: int, n: int, V: int, v_bs: int, batch: int, k1: int, t1: int, t2: int,
                               cols: int = 0, c_bs: int = 0, ell: int = 0, w_min: int = 0, hist: int = 0, lightest: int = 0, stream: int = 0) -> None:
    """Stern's collision step on `batch` generators G_b (k x n; operands as in row_sums_weights_batch_dev): of the N1 * N2 pairs (S1: t1
    of the left rows 0 .. k1-1, rank r1 < N1 = C(k1, t1); S2: t2 of the right rows k1 .. k-1, rank r2 < N2 = C(k - k1, t2) of {i - k1})
    those whose word V_b ^ rows S1 ^ rows S2 is 0 at the ell window columns (cols: DEVICE int32, member b's at cols + b * c_bs entries,
    c_bs = 0: one window, cols = 0: columns 0 .. ell-1) are weighed over all n columns.  DEVICE int64 outputs, each 0 = not wanted, not
    both: hist (batch * (n + 1): the number of colliding pairs per weight), lightest (per member: the minimum of
    (wt << 40) | (r1 * N2 + r2) over wt >= w_min, -1 if none; row_pair_unrank gives the rows).  A member with a window entry outside
    0 .. n-1 is refused on the device: hist all -1, lightest -2.  k, n <= 1024, t1, t2 <= 8, ell <= 64, N1 <= 8192, N1 * N2 <= 2^40: the
    half with fewer sums belongs first.  Asynchronous, lock-free and capturable on both paths of plan_row_sums_collide_batch."""
    _check(lib().m4ri_amd_row_sums_collide_batch_dev(G or None, g_stride, g_bs, k, n, V or None, v_bs, batch, k1, t1, t2, cols or None, c_bs, ell,
                                                     w_min, hist or None, lightest or None, stream), "m4ri_amd_row_sums_collide_batch_dev")


def row_sums_collide_list_batch_dev(G: int, g_stride: int, g_bs: int, k: int, n: int, V: int, v_bs: int, batch: int, k1: int, t1: int, t2: int,
                                    cols: int = 0, c_bs: int = 0, ell: int = 0, w_min: int = 0, w_max: int = 1024, hist: int = 0, lightest: int = 0,
                                    list: int = 0, l_bs: int = 0, cap: int = 0, count: int = 0, stream: int = 0) -> None:
    """row_sums_collide_batch_dev with a list: the colliding pairs with w_min <= wt <= w_max (w_max above n is n; lightest ignores it).
    DEVICE int64 outputs: count (batch entries: the true number of qualifying pairs per member, -1 for a refused member) and list (member
    b's at list + b * l_bs entries: the first min(count[b], cap) are distinct keys (wt << 40) | (r1 * N2 + r2) of qualifying pairs in no
    order, all of them if count[b] <= cap; the entries behind are not written).  They come together; list = 0 only with cap = 0 (a
    filtered count).  hist and lightest as in row_sums_collide_batch_dev, each 0 = not wanted; one of hist, lightest, count is required.
    row_sums_words_batch_dev turns the keys into words.  Asynchronous, lock-free and capturable on both paths."""
    _check(lib().m4ri_amd_row_sums_collide_list_batch_dev(G or None, g_stride, g_bs, k, n, V or None, v_bs, batch, k1, t1, t2, cols or None, c_bs, ell,
                                                          w_min, w_max, hist or None, lightest or None, list or None, l_bs, cap, count or None,
                                                          stream), "m4ri_amd_row_sums_collide_list_batch_dev")


def row_sums_words_batch_dev(G: int, g_stride: int, g_bs: int, k: int, n: int, V: int, v_bs: int, batch: int, k1: int, t1: int, t2: int, keys: int,
                             l_bs: int, cap: int, count: int, W: int, w_stride: int, w_bs: int, skipped: int = 0, stream: int = 0) -> None:
    """The words of listed keys on the device: for i < m_b = min(max(count[b], 0), cap) (count = 0: cap keys per member) row i of W_b
    (rows w_stride words apart, members w_bs) becomes V_b ^ rows S1 ^ rows S2 of the pair of rank keys[b * l_bs + i] & (2^40 - 1); only the
    n valid bits are written.  t2 = 0, k1 = k: the keys of row_sums_weights_batch_dev.  A key < 0 or with a rank >= N1 * N2 is skipped
    on the device (its row is not written) and counted in skipped (DEVICE int32, batch entries, 0 = not wanted).  k, n <= 1024,
    t1, t2 <= 8, N1 * N2 <= 2^40.  Asynchronous, lock-free and capturable."""
    _check(lib().m4ri_amd_row_sums_words_batch_dev(G or None, g_stride, g_bs, k, n, V or None, v_bs, batch, k1, t1, t2, keys or None, l_bs, cap,
                                                   count or None, W or None, w_stride, w_bs, skipped or None, stream), "m4ri_amd_row_sums_words_batch_dev")


def plan_row_sums_collide_batch(k: int, n: int, k1: int, t1: int, t2: int, ell: int) -> int:
    """The path row_sums_collide_batch_dev takes (0 one workgroup per member, plain stores; 1 the right list in slices, a workgroup each,
    and global atomics). Host arithmetic."""
    return int(lib().m4ri_amd_plan_row_sums_collide_batch(k, n, k1, t1, t2, ell))


def row_sums_collide_slices(k: int, n: int, k1: int, t1: int, t2: int, ell: int, batch: int) -> int:
    """The workgroups per member of row_sums_collide_batch_dev on path 1: the slices of the right list. Host arithmetic."""
    return int(lib().m4ri_amd_row_sums_collide_slices(k, n, k1, t1, t2, ell, batch))


def lists_collide_batch_dev(X: int, x_stride: int, x_bs: int, nx: int, Y: int, y_stride: int, y_bs: int, ny: int, n: int, V: int = 0, v_bs: int = 0,
                            batch: int = 1, cols: int = 0, c_bs: int = 0, ell: int = 0, w_min: int = 0, w_max: int = 1024, hist: int = 0, lightest: int = 0,
                            list: int = 0, l_bs: int = 0, cap: int = 0, count: int = 0, stream: int = 0) -> None:
    """The join of two explicit lists on a window, for `batch` members: X_b (nx rows of n bits, rows x_stride words apart, members x_bs),
    Y_b (ny rows), an optional word V_b; a batch stride of 0 shares an operand, X and Y may be the same memory.  The pair (i, j), rank
    i * ny + j (divmod(rank, ny) gives it back), collides iff V_b ^ X_b[i] ^ Y_b[j] is 0 at the ell window columns (cols: DEVICE int32,
    member b's at cols + b * c_bs entries, cols = 0: columns 0 .. ell-1).  DEVICE int64 outputs as in row_sums_collide_list_batch_dev, each
    0 = not wanted, one required: hist (batch * (n + 1)), lightest (the minimum of (wt << 40) | rank over wt >= w_min, -1 if none), count
    and list (the keys of the pairs with w_min <= wt <= w_max; count the true total, the first min(count, cap) entries distinct, the
    entries behind not written; list = 0 only with cap = 0).  A member with a window entry outside 0 .. n-1 is refused on the device:
    hist all -1, lightest -2, count -1.  n <= 1024, ell <= 64, nx, ny < 2^31, nx * ny <= 2^40; no bound on nx by LDS.  Asynchronous,
    lock-free and capturable on both paths of plan_lists_collide_batch."""
    _check(lib().m4ri_amd_lists_collide_batch_dev(X or None, x_stride, x_bs, nx, Y or None, y_stride, y_bs, ny, n, V or None, v_bs, batch, cols or None,
                                                  c_bs, ell, w_min, w_max, hist or None, lightest or None, list or None, l_bs, cap, count or None, stream),
           "m4ri_amd_lists_collide_batch_dev")


def lists_words_batch_dev(X: int, x_stride: int, x_bs: int, nx: int, Y: int, y_stride: int, y_bs: int, ny: int, n: int, V: int, v_bs: int, batch: int,
                          keys: int, l_bs: int, cap: int, count: int, W: int, w_stride: int, w_bs: int, skipped: int = 0, stream: int = 0) -> None:
    """The words of listed keys of two explicit lists on the device: for i < m_b = min(max(count[b], 0), cap) (count = 0: cap keys per
    member) and r = keys[b * l_bs + i] & (2^40 - 1), row i of W_b (rows w_stride words apart, members w_bs) becomes
    V_b ^ X_b[r // ny] ^ Y_b[r % ny]; only the n valid bits are written.  A key < 0 or with r >= nx * ny is skipped on the device (its row
    is not written) and counted in skipped (DEVICE int32, batch entries, 0 = not wanted).  The limits of lists_collide_batch_dev.
    Asynchronous, lock-free and capturable."""
    _check(lib().m4ri_amd_lists_words_batch_dev(X or None, x_stride, x_bs, nx, Y or None, y_stride, y_bs, ny, n, V or None, v_bs, batch, keys or None, l_bs,
                                                cap, count or None, W or None, w_stride, w_bs, skipped or None, stream), "m4ri_amd_lists_words_batch_dev")


def plan_lists_collide_batch(nx: int, ny: int, n: int, ell: int, batch: int) -> int:
    """The path lists_collide_batch_dev takes (0 one chunk and one slice per member: one workgroup, plain stores; 1 several workgroups per
    member and global atomics; -1 negative sizes). Host arithmetic."""
    return int(lib().m4ri_amd_plan_lists_collide_batch(nx, ny, n, ell, batch))


def lists_collide_units(nx: int, ny: int, n: int, ell: int, batch: int) -> tuple:
    """(chunk_rows, chunks, slices) of lists_collide_batch_dev: the left rows of one workgroup's table, the chunks of the left list and the
    slices of the right list per member. Host arithmetic; ValueError for negative sizes."""
    c, ch, sl = _I64(0), _I64(0), _I64(0)
    if lib().m4ri_amd_lists_collide_units(nx, ny, n, ell, batch, ctypes.byref(c), ctypes.byref(ch), ctypes.byref(sl)) != 0:
        raise ValueError("lists_collide_units: negative sizes")
    return int(c.value), int(ch.value), int(sl.value)


def sort_rows_batch_dev(X: int, x_stride: int, x_bs: int, nx: int, n: int, xcount: int = 0, batch: int = 1, cols: int = 0, c_bs: int = 0, ell: int = 0,
                        order: int = 0, ucount: int = 0, uniq: int = 0, mult: int = 0, l_bs: int = 0, scratch: int = 0, scratch_bytes: int = 0,
                        stream: int = 0) -> None:
    """The rows of the lists X_b (nx rows of n bits, rows x_stride words apart, members x_bs, x_bs = 0 one shared list; the first
    m_b = min(max(xcount[b], 0), nx) rows count, xcount = 0: nx) sorted and deduplicated on the device.  Row i goes before row j iff
    (key_i, words of row i as unsigned numbers, i) is lexicographically smaller; key = the bits at the ell window columns (cols: DEVICE
    int32, member b's at cols + b * c_bs, cols = 0: columns 0 .. ell-1), bit t = column cols[t].  DEVICE int64 outputs, member b's at
    + b * l_bs, each 0 = not wanted, order or ucount required: order (the row indices in that order), ucount (batch entries: the number
    of distinct rows), uniq (needs ucount: the smallest index of each class, a valid key of lists_words_batch_dev with ny = 1), mult
    (needs uniq: the class sizes).  Entries behind m_b / ucount[b] are not written.  A member with a window entry outside 0 .. n-1 is
    refused on the device: ucount -1, nothing else written.  scratch: DEVICE memory of sort_rows_scratch_bytes(nx, n, ell, batch) bytes
    (0 on path 0).  n <= 1024, ell <= 64, nx <= 2^24.  Asynchronous, lock-free, no atomics, capturable."""
    _check(lib().m4ri_amd_sort_rows_batch_dev(X or None, x_stride, x_bs, nx, n, xcount or None, batch, cols or None, c_bs, ell, order or None, ucount or None,
                                              uniq or None, mult or None, l_bs, scratch or None, scratch_bytes, stream), "m4ri_amd_sort_rows_batch_dev")


def plan_sort_rows_batch(nx: int, n: int, ell: int, batch: int) -> int:
    """The path sort_rows_batch_dev takes (0 one workgroup per member sorts in LDS, one launch, no scratch; 1 the entries in the caller's
    scratch, chunk sorts and merge levels; -1 negative sizes). Host arithmetic."""
    return int(lib().m4ri_amd_plan_sort_rows_batch(nx, n, ell, batch))


def sort_rows_units(nx: int, n: int, ell: int, batch: int) -> tuple:
    """(chunk_rows, padded, launches) of sort_rows_batch_dev: the entries one workgroup sorts in LDS (the longest list of path 0), the
    power of two the host sizes a member's network by, and the kernel launches of a call that asks for every output. Host arithmetic;
    ValueError for negative sizes."""
    c, pd, ln = _I64(0), _I64(0), _I64(0)
    if lib().m4ri_amd_sort_rows_units(nx, n, ell, batch, ctypes.byref(c), ctypes.byref(pd), ctypes.byref(ln)) != 0:
        raise ValueError("sort_rows_units: negative sizes")
    return int(c.value), int(pd.value), int(ln.value)


def sort_rows_scratch_bytes(nx: int, n: int, ell: int, batch: int) -> int:
    """The bytes of device scratch sort_rows_batch_dev needs (0 on path 0). Host arithmetic; ValueError for negative sizes or a size
    beyond int64."""
    r = int(lib().m4ri_amd_sort_rows_scratch_bytes(nx, n, ell, batch))
    if r < 0:
        raise ValueError("sort_rows_scratch_bytes: negative sizes, or beyond int64")
    return r


def row_pair_rank(S1, S2, k1: int, k: int, t2: int) -> int:
    """The pair rank r1 * N2 + r2 of row_sums_collide_batch_dev's lightest: S1 of the rows 0 .. k1-1, S2 (t2 of them) of the rows
    k1 .. k-1, both as absolute row indices in any order; N2 = C(k - k1, t2)."""
    from math import comb
    S1, S2 = [int(i) for i in S1], [int(i) for i in S2]
    if not 0 <= k1 <= k or len(S2) != t2 or any(not 0 <= i < k1 for i in S1) or any(not k1 <= i < k for i in S2):
        raise ValueError("row_pair_rank: S1 lies in the rows below k1, S2 has t2 of the rows k1 .. k-1")
    return row_subset_rank(S1) * comb(k - k1, t2) + row_subset_rank(i - k1 for i in S2)


def row_pair_unrank(rank: int, k1: int, k: int, t1: int, t2: int) -> tuple:
    """The inverse of row_pair_rank: (S1, S2), the absolute row indices of both sets, each ascending."""
    from math import comb
    if not 0 <= k1 <= k or t1 < 0 or t2 < 0:
        raise ValueError("row_pair_unrank: no such pair")
    n1, n2 = comb(k1, t1), comb(k - k1, t2)
    if not 0 <= rank < n1 * n2:
        raise ValueError("row_pair_unrank: no such pair")
    return row_subset_unrank(rank // n2, t1), tuple(i + k1 for i in row_subset_unrank(rank % n2, t2))


def copy_block_batch_dev(D: int, d_stride: int, d_bs: int, d_row: int, d_col: int, A: int, a_stride: int, a_bs: int, a_row: int, a_col: int,
                         rows: int, cols: int, batch: int, stream: int = 0) -> None:
    """Bits (d_row + i, d_col + j) of every D_b <- bits (a_row + i, a_col + j) of A_b, i < rows, j < cols, X_b = X + b * x_bs words; any
    bit offsets, nothing else of D written, a_bs = 0 broadcasts one block.  Asynchronous, lock-free and capturable."""
    _check(lib().m4ri_amd_copy_block_batch_dev(D, d_stride, d_bs, d_row, d_col, A, a_stride, a_bs, a_row, a_col, rows, cols, batch, stream),
           "m4ri_amd_copy_block_batch_dev")


def submatrix_batch_dev(S: int, s_stride: int, s_bs: int, A: int, a_stride: int, a_bs: int, lowr: int, lowc: int, highr: int, highc: int,
                        batch: int, stream: int = 0) -> None:
    """mzd_submatrix for a batch: S_b ((highr - lowr) x (highc - lowc)) <- rows lowr .. highr-1, columns lowc .. highc-1 of A_b; lowc
    may be any column."""
    copy_block_batch_dev(S, s_stride, s_bs, 0, 0, A, a_stride, a_bs, lowr, lowc, highr - lowr, highc - lowc, batch, stream)


def concat_batch_dev(C: int, c_stride: int, c_bs: int, A: int, a_stride: int, a_bs: int, a_cols: int, B: int, b_stride: int, b_bs: int, b_cols: int,
                     nrows: int, batch: int, stream: int = 0) -> None:
    """mzd_concat for a batch: C_b (nrows x (a_cols + b_cols)) <- [A_b | B_b]."""
    copy_block_batch_dev(C, c_stride, c_bs, 0, 0, A, a_stride, a_bs, 0, 0, nrows, a_cols, batch, stream)
    copy_block_batch_dev(C, c_stride, c_bs, 0, a_cols, B, b_stride, b_bs, 0, 0, nrows, b_cols, batch, stream)


def stack_batch_dev(C: int, c_stride: int, c_bs: int, A: int, a_stride: int, a_bs: int, a_rows: int, B: int, b_stride: int, b_bs: int, b_rows: int,
                    ncols: int, batch: int, stream: int = 0) -> None:
    """mzd_stack for a batch: C_b ((a_rows + b_rows) x ncols) <- A_b on top of B_b."""
    copy_block_batch_dev(C, c_stride, c_bs, 0, 0, A, a_stride, a_bs, 0, 0, a_rows, ncols, batch, stream)
    copy_block_batch_dev(C, c_stride, c_bs, a_rows, 0, B, b_stride, b_bs, 0, 0, b_rows, ncols, batch, stream)


def extract_tri_batch_dev(D: int, d_stride: int, d_bs: int, A: int, a_stride: int, a_bs: int, nrows: int, ncols: int, batch: int, upper: bool,
                          diag: int = 2, rank: int = 0, stream: int = 0) -> None:
    """The upper (D_b k x ncols) or lower (D_b nrows x k) triangle of every A_b, k = min(nrows, ncols); diag 0 / 1 / 2 = the diagonal
    zero / one / A's; rank (DEVICE int32 per member, 0 = none) cuts U's rows and L's columns behind it.  On ple_batch_dev(pluq=1)'s
    output (upper=False, diag=1, rank) is L and (upper=True, diag=2, rank) is U.  Asynchronous, lock-free and capturable."""
    _check(lib().m4ri_amd_extract_tri_batch_dev(D, d_stride, d_bs, A, a_stride, a_bs, nrows, ncols, batch, int(bool(upper)), diag, rank or None, stream),
           "m4ri_amd_extract_tri_batch_dev")


def apply_p_left_batch_dev(A: int, stride: int, a_bs: int, nrows: int, ncols: int, batch: int, P: int, p_bs: int, length: int, trans: bool = False,
                           status: int = 0, stream: int = 0) -> None:
    """mzd_apply_p_left (trans: _trans) on every member, P a DEVICE int32 array, member b's at P + b * p_bs entries (0: shared);
    status (DEVICE int32 per member, 0 = not wanted): -1 and the member untouched where an entry is out of range.  Asynchronous on
    paths 0-1 of plan_perm_batch, blocking on path 2."""
    _check(lib().m4ri_amd_apply_p_left_batch_dev(A, stride, a_bs, nrows, ncols, batch, P or None, p_bs, length, int(bool(trans)), status or None, stream),
           "m4ri_amd_apply_p_left_batch_dev")


def apply_p_right_batch_dev(A: int, stride: int, a_bs: int, nrows: int, ncols: int, batch: int, P: int, p_bs: int, length: int, trans: bool = False,
                            status: int = 0, stream: int = 0) -> None:
    """mzd_apply_p_right (trans: _trans) on every member; arguments as apply_p_left_batch_dev, the entries are columns."""
    _check(lib().m4ri_amd_apply_p_right_batch_dev(A, stride, a_bs, nrows, ncols, batch, P or None, p_bs, length, int(bool(trans)), status or None, stream),
           "m4ri_amd_apply_p_right_batch_dev")


def plan_perm_batch(nrows: int, ncols: int, right: bool) -> int:
    """The path apply_p_left_batch_dev (right False) / apply_p_right_batch_dev takes for members of this shape (0 wave, 1 LDS, 2 one by
    one). Host arithmetic."""
    return int(lib().m4ri_amd_plan_perm_batch(nrows, ncols, int(bool(right))))


def model_seconds_batch(m: int, l: int, n: int, levels: int = -1, batch: int = 1) -> float:
    """The engine's time model for `batch` products scheduled as one (levels < 0: at the depth the model picks). Host arithmetic."""
    return float(lib().m4ri_amd_model_seconds_batch(m, l, n, levels, batch))


def echelonize_batch_dev(A: int, stride: int, a_bs: int, nrows: int, ncols: int, batch: int, full: int, rank: int, pivots: int = 0,
                         stream: int = 0) -> None:
    """`batch` (reduced) row echelon forms in place, member b at A + b * a_bs words; rank / pivots: DEVICE int32 arrays (pivots 0 =
    not wanted).  Asynchronous on paths 0-2 of plan_echelonize_batch, blocking on path 3."""
    _check(lib().m4ri_amd_echelonize_batch_dev(A, stride, a_bs, nrows, ncols, batch, int(full), rank, pivots or None, stream),
           "m4ri_amd_echelonize_batch_dev")


def plan_echelonize_batch(nrows: int, ncols: int) -> int:
    """The path echelonize_batch_dev takes for members of this shape (0 wave, 1 LDS, 2 global, 3 one by one). Host arithmetic."""
    return int(lib().m4ri_amd_plan_echelonize_batch(nrows, ncols))


def echelonize_order_batch_dev(D: int, d_stride: int, d_bs: int, A: int, a_stride: int, a_bs: int, nrows: int, ncols: int, pivot_rows: int,
                               order: int, o_bs: int, olen: int, batch: int, full: int, rank: int, pivots: int = 0, stream: int = 0) -> None:
    """`batch` (reduced) row echelon forms on column orders chosen per member, no column moved: D_b <- the form of A_b (a_bs = 0: one
    shared A; D == A with equal strides: in place) with the columns visited in the order of member b's olen DEVICE int32 entries at
    order + b * o_bs (o_bs = 0: one order; order 0: the natural order).  Rows from pivot_rows on only follow.  rank / pivots: DEVICE
    int32 arrays (pivots 0 = not wanted, else batch * min(pivot_rows, ncols) pivot COLUMNS); a member with an entry out of range has
    rank -1 and is not written.  Asynchronous, lock-free and capturable on paths 0-2 of plan_echelonize_order_batch; path 3: 801."""
    _check(lib().m4ri_amd_echelonize_order_batch_dev(D or None, d_stride, d_bs, A or None, a_stride, a_bs, nrows, ncols, pivot_rows, order or None, o_bs,
                                                     olen, batch, int(full), rank or None, pivots or None, stream), "m4ri_amd_echelonize_order_batch_dev")


def plan_echelonize_order_batch(nrows: int, ncols: int) -> int:
    """The path echelonize_order_batch_dev takes for members of this shape (0 wave, 1 LDS, 2 global, 3 not supported). Host
    arithmetic."""
    return int(lib().m4ri_amd_plan_echelonize_order_batch(nrows, ncols))


def random_orders_batch_dev(order: int, o_bs: int, n: int, batch: int, seed: int, stream: int = 0) -> None:
    """order + b * o_bs (DEVICE int32) <- random_order(seed, b, n) for every member, n <= 4096.  Asynchronous and capturable."""
    _check(lib().m4ri_amd_random_orders_batch_dev(order or None, o_bs, n, batch, seed & 0xFFFFFFFFFFFFFFFF, stream), "m4ri_amd_random_orders_batch_dev")


def random_order(seed: int, b: int, n: int):
    """The permutation of 0 .. n-1 (NumPy int32) that random_orders_batch_dev gives member b: outputs b * n .. b * n + n - 1 of the
    splitmix64 stream seeded `seed`, the low 12 bits of output j replaced by j, sorted ascending; the low 12 bits of the sorted keys."""
    import numpy as np
    if not 0 <= n <= 4096:
        raise ValueError("random_order: 0 <= n <= 4096")
    keys = (splitmix_words(seed, b * n, n) & ~np.uint64(4095)) | np.arange(n, dtype=np.uint64)
    return (np.sort(keys) & np.uint64(4095)).astype(np.int32)


def pivot_exchange_batch_dev(D: int, d_stride: int, d_bs: int, nrows: int, ncols: int, pivot_rows: int, pivots: int, rank: int, batch: int,
                             req: int = 0, r_bs: int = 0, steps: int = 0, seed: int = 0, order: int = 0, o_bs: int = 0, olen: int = 0, done: int = 0,
                             stream: int = 0) -> None:
    """`steps` pivot exchanges in place on the reduced forms echelonize_order_batch_dev(full=1) left in D_b, with its pivots (DEVICE
    int32, in/out) and rank (DEVICE int32, read only).  Step s of member b takes the request (r, c) = the DEVICE int32 entries 2 s and
    2 s + 1 at req + b * r_bs (r_bs = 0: one list for all), or with req 0 draws it from the stream seeded `seed` (exchange_draw); a
    request that is not valid -- r not a pivot row, c not a column, bit (r, c) clear, c the row's own pivot -- is skipped.  A performed
    step adds row r into every other row with bit c, sets pivots[r] = c and swaps the old and the new pivot column in member b's olen
    DEVICE int32 entries at order + b * o_bs (order 0: none kept).  done (DEVICE int32, 0 = not wanted): the steps performed per
    member.  Asynchronous, lock-free and capturable on paths 0-2 of plan_pivot_exchange_batch; path 3: 801."""
    _check(lib().m4ri_amd_pivot_exchange_batch_dev(D or None, d_stride, d_bs, nrows, ncols, pivot_rows, pivots or None, rank or None, batch, req or None,
                                                   r_bs, steps, seed & 0xFFFFFFFFFFFFFFFF, order or None, o_bs, olen, done or None, stream),
           "m4ri_amd_pivot_exchange_batch_dev")


def plan_pivot_exchange_batch(nrows: int, ncols: int, steps: int) -> int:
    """The path pivot_exchange_batch_dev takes for members of this shape and this many steps (0 wave, 1 LDS, 2 global, 3 not supported).
    Host arithmetic."""
    return int(lib().m4ri_amd_plan_pivot_exchange_batch(nrows, ncols, steps))


def exchange_draw(seed: int, b: int, steps: int, s: int, rank: int, ncols: int):
    """(r, start) of step s of member b in a call of pivot_exchange_batch_dev without requests: output number b * steps + s of the
    splitmix64 stream seeded `seed`, its high half mod the member's rank and its low half mod ncols.  The column exchanged is the first
    one from start on, cyclically, at which row r has a bit and which is not its own pivot."""
    if rank < 1 or ncols < 1 or not 0 <= s < steps or b < 0:
        raise ValueError("exchange_draw: rank >= 1, ncols >= 1, 0 <= s < steps, b >= 0")
    h = int(splitmix_words(seed, b * steps + s, 1)[0])
    return (h >> 32) % rank, (h & 0xFFFFFFFF) % ncols


def isd_search_dev(D: int, d_stride: int, d_bs: int, nrows: int, ncols: int, pivot_rows: int, pivots: int, rank: int, batch: int, iters: int,
                   steps: int, seed: int, t: int, w_min: int, w_stop: int, best: int, order: int = 0, o_bs: int = 0, olen: int = 0, best_iter: int = 0,
                   iters_run: int = 0, done: int = 0, W: int = 0, w_bs: int = 0, stream: int = 0) -> None:
    """A whole information-set decoding search in one launch, on the state of pivot_exchange_batch_dev: up to `iters` times "`steps`
    exchanges drawn from the stream seeded isd_iteration_seed(seed, it) (none before iteration 0), then the lightest sum of t of the
    pivot_rows pivot rows against row pivot_rows (the received word; the zero word if nrows == pivot_rows) with weight >= w_min", as
    pivot_exchange_batch_dev and row_sums_weights_batch_dev give them.  best (DEVICE int64, required): the key of the lightest word over
    the iterations, the earliest among equal weights, -1 for none; best_iter, iters_run, done (DEVICE int32, 0 = not wanted): its
    iteration, the iterations run (a member stops once its best weight is <= w_stop; w_stop < 0: never) and the steps performed; W
    (0 = not wanted): the word itself, member b's at W + b * w_bs.  Asynchronous, lock-free and capturable on paths 0-1 of
    plan_isd_search; path 2: 801."""
    _check(lib().m4ri_amd_isd_search_dev(D or None, d_stride, d_bs, nrows, ncols, pivot_rows, pivots or None, rank or None, batch, iters, steps,
                                         seed & 0xFFFFFFFFFFFFFFFF, t, w_min, w_stop, order or None, o_bs, olen, best or None, best_iter or None,
                                         iters_run or None, done or None, W or None, w_bs, stream), "m4ri_amd_isd_search_dev")


def plan_isd_search(nrows: int, ncols: int, pivot_rows: int, t: int) -> int:
    """The path isd_search_dev takes for members of this shape at this t (0 wave, 1 LDS, 2 not supported).  Host arithmetic."""
    return int(lib().m4ri_amd_plan_isd_search(nrows, ncols, pivot_rows, t))


def isd_collide_search_dev(D: int, d_stride: int, d_bs: int, nrows: int, ncols: int, pivot_rows: int, pivots: int, rank: int, batch: int, iters: int,
                           steps: int, seed: int, k1: int, t1: int, t2: int, ell: int, w_min: int, w_stop: int, best: int, order: int = 0, o_bs: int = 0,
                           olen: int = 0, best_iter: int = 0, iters_run: int = 0, done: int = 0, W: int = 0, w_bs: int = 0, stream: int = 0) -> None:
    """A whole Stern collision decoding search in one launch, on the state of pivot_exchange_batch_dev: up to `iters` times "`steps`
    exchanges drawn from the stream seeded isd_iteration_seed(seed, it) (none before iteration 0), then the lightest colliding pair of a
    sum of t1 of the first k1 pivot rows and a sum of t2 of the others against row pivot_rows (the received word; the zero word if
    nrows == pivot_rows) on the window order[pivot_rows : pivot_rows + ell] with weight >= w_min", as pivot_exchange_batch_dev and
    row_sums_collide_batch_dev give them.  best (DEVICE int64, required): the key (wt << 40) | pair rank (row_pair_unrank splits it) of
    the lightest word over the iterations, the earliest among equal weights, -1 for none; best_iter, iters_run, done (DEVICE int32,
    0 = not wanted): its iteration, the iterations run (a member stops once its best weight is <= w_stop; w_stop < 0: never) and the
    steps performed; W (0 = not wanted): the word itself, member b's at W + b * w_bs.  ell > 0 needs the order (DEVICE int32, in/out)
    with olen >= pivot_rows + ell.  Asynchronous, lock-free and capturable where plan_isd_collide_search gives 1; otherwise 801."""
    _check(lib().m4ri_amd_isd_collide_search_dev(D or None, d_stride, d_bs, nrows, ncols, pivot_rows, pivots or None, rank or None, batch, iters, steps,
                                                 seed & 0xFFFFFFFFFFFFFFFF, k1, t1, t2, ell, w_min, w_stop, order or None, o_bs, olen, best or None,
                                                 best_iter or None, iters_run or None, done or None, W or None, w_bs, stream),
           "m4ri_amd_isd_collide_search_dev")


def plan_isd_collide_search(nrows: int, ncols: int, pivot_rows: int, k1: int, t1: int, t2: int, ell: int) -> int:
    """Whether isd_collide_search_dev places members of this shape and this split (1 a workgroup per member in LDS, 2 not supported,
    -1 negative sizes or k1 > pivot_rows).  Host arithmetic."""
    return int(lib().m4ri_amd_plan_isd_collide_search(nrows, ncols, pivot_rows, k1, t1, t2, ell))


def isd_iteration_seed(seed: int, it: int) -> int:
    """The seed of the exchanges before iteration `it` >= 1 of isd_search_dev: output number `it` of the splitmix64 stream seeded
    `seed`.  exchange_draw(isd_iteration_seed(seed, it), b, steps, s, rank, ncols) is the draw of step s of member b there."""
    if it < 0:
        raise ValueError("isd_iteration_seed: it >= 0")
    return int(splitmix_words(seed, it, 1)[0])


def solve_left_batch_dev(A: int, a_stride: int, a_bs: int, m: int, n: int, B: int, b_stride: int, b_bs: int, k: int, batch: int, status: int,
                         rank: int = 0, stream: int = 0) -> None:
    """`batch` systems A_b X_b = B_b, A_b at A + b * a_bs words (read only; a_bs = 0: one shared A), B_b (max(m, n) x k) at B + b * b_bs
    overwritten by X where status[b] = 0, untouched where it is -1 (no solution); status / rank: DEVICE int32 arrays (rank 0 = not
    wanted).  Asynchronous on paths 0-1 of plan_solve_batch, blocking on path 2."""
    _check(lib().m4ri_amd_solve_left_batch_dev(A, a_stride, a_bs, m, n, B, b_stride, b_bs, k, batch, status, rank or None, stream),
           "m4ri_amd_solve_left_batch_dev")


def inv_batch_dev(Binv: int, b_stride: int, b_bs: int, A: int, a_stride: int, a_bs: int, n: int, batch: int, rank: int = 0,
                  stream: int = 0) -> None:
    """`batch` inverses, Binv_b <- the right half of the reduced echelon form of [A_b | I] (Binv == A in place allowed); rank: DEVICE
    int32 array (0 = not wanted).  Asynchronous on paths 0-1 of plan_solve_batch(n, n, n), blocking on path 2."""
    _check(lib().m4ri_amd_inv_batch_dev(Binv, b_stride, b_bs, A, a_stride, a_bs, n, batch, rank or None, stream), "m4ri_amd_inv_batch_dev")


def plan_solve_batch(m: int, n: int, k: int) -> int:
    """The path solve_left_batch_dev takes for (m, n, k), and inv_batch_dev for (n, n, n) (0 wave, 1 LDS, 2 one by one). Host arithmetic."""
    return int(lib().m4ri_amd_plan_solve_batch(m, n, k))


def kernel_left_batch_dev(A: int, a_stride: int, a_bs: int, m: int, n: int, R: int, r_stride: int, r_bs: int, kc: int, batch: int, rank: int,
                          stream: int = 0) -> None:
    """`batch` null-space bases, A_b (m x n) at A + b * a_bs words (read only; a_bs = 0: one shared A), R_b (n x kc) at R + b * r_bs <- the
    first min(kc, n - rank[b]) vectors of mzd_kernel_left_pluq's basis, zero columns up to kc; rank: DEVICE int32 array (required).
    Asynchronous on paths 0-1 of plan_kernel_batch, blocking on path 2."""
    _check(lib().m4ri_amd_kernel_left_batch_dev(A, a_stride, a_bs, m, n, R, r_stride, r_bs, kc, batch, rank or None, stream),
           "m4ri_amd_kernel_left_batch_dev")


def plan_kernel_batch(m: int, n: int) -> int:
    """The path kernel_left_batch_dev takes for m x n members (0 wave, 1 LDS, 2 one by one). Host arithmetic."""
    return int(lib().m4ri_amd_plan_kernel_batch(m, n))


def ple_batch_dev(A: int, stride: int, a_bs: int, nrows: int, ncols: int, batch: int, pluq: bool, P: int, Q: int, rank: int,
                  stream: int = 0) -> None:
    """`batch` PLE (pluq false) or PLUQ decompositions in place, member b at A + b * a_bs words; P (batch * nrows), Q (batch * ncols) and
    rank (batch): DEVICE int32 arrays, all required.  Asynchronous on paths 0-2 of plan_ple_batch, blocking on path 3."""
    _check(lib().m4ri_amd_ple_batch_dev(A, stride, a_bs, nrows, ncols, batch, int(bool(pluq)), P or None, Q or None, rank or None, stream),
           "m4ri_amd_ple_batch_dev")


def plan_ple_batch(nrows: int, ncols: int) -> int:
    """The path ple_batch_dev takes for members of this shape (0 wave, 1 LDS, 2 global, 3 one by one). Host arithmetic."""
    return int(lib().m4ri_amd_plan_ple_batch(nrows, ncols))


def pluq_solve_left_batch_dev(A: int, a_stride: int, a_bs: int, m: int, n: int, rank: int, P: int, Q: int, B: int, b_stride: int, b_bs: int,
                              k: int, batch: int, status: int, stream: int = 0) -> None:
    """`batch` systems A_b X_b = B_b from what ple_batch_dev(pluq=True) left in A, rank, P and Q (read only; a_bs = 0: one decomposition
    for all), B_b (max(m, n) x k) at B + b * b_bs <- X, exactly as solve_left_batch_dev on the original A; status: DEVICE int32 array
    (0, or -1 = no solution, B_b untouched).  Asynchronous on paths 0-1 of plan_pluq_solve_batch, blocking on path 2."""
    _check(lib().m4ri_amd_pluq_solve_left_batch_dev(A, a_stride, a_bs, m, n, rank or None, P or None, Q or None, B, b_stride, b_bs, k, batch,
                                                    status or None, stream), "m4ri_amd_pluq_solve_left_batch_dev")


def plan_pluq_solve_batch(m: int, n: int, k: int) -> int:
    """The path pluq_solve_left_batch_dev takes for (m, n, k) (0 wave, 1 LDS, 2 one by one). Host arithmetic."""
    return int(lib().m4ri_amd_plan_pluq_solve_batch(m, n, k))


def m4rm_dev(C: int, c_stride: int, A: int, a_stride: int, B: int, b_stride: int, m: int, l: int, n: int,
             add: bool = False, ksplit: int = 0, stream: int = 0) -> None:
    _check(lib().m4ri_amd_m4rm_dev(C, c_stride, A, a_stride, B, b_stride, m, l, n, int(add), ksplit, stream), "m4ri_amd_m4rm_dev")


def xor_dev(C: int, c_stride: int, A: int, a_stride: int, B: int, b_stride: int, rows: int, ncols: int, stream: int = 0) -> None:
    _check(lib().m4ri_amd_xor_dev(C, c_stride, A, a_stride, B, b_stride, rows, ncols, stream), "m4ri_amd_xor_dev")


def fill_dev(M: int, stride: int, rows: int, ncols: int, seed: int, stream: int = 0) -> None:
    _check(lib().m4ri_amd_fill_dev(M, stride, rows, ncols, seed, stream), "m4ri_amd_fill_dev")


def fill_rows_dev(M: int, stride: int, row0: int, rows: int, ncols: int, seed: int, stream: int = 0) -> None:
    """Rows [row0, row0 + rows) of the matrix fill_dev(seed) would produce, written from M's row 0."""
    _check(lib().m4ri_amd_fill_rows_dev(M, stride, row0, rows, ncols, seed, stream), "m4ri_amd_fill_rows_dev")


# ---- several GPUs (include/m4ri_amd.h part 4) ------------------------------------------------------
def shard_plan(world: int, m: int, l: int, n: int, levels: int = 0) -> ShardPlan:
    """Plan of one product over `world` ranks (pure host arithmetic, no GPU needed)."""
    p = ShardPlan()
    if lib().m4ri_amd_shard_plan_make(ctypes.byref(p), world, m, l, n, levels) != 0:
        raise ValueError(f"m4ri_amd_shard_plan_make({world}, {m}, {l}, {n}, {levels}) rejected its arguments")
    return p


def shard_group(plan: ShardPlan, cutoff: int = 0) -> int:
    """Rounds of a rank's sub-products that go into one batched product (mul_batch_dev); 1 = one at a time.  Host arithmetic."""
    return int(lib().m4ri_amd_shard_group(ctypes.byref(plan), cutoff))


def shard_piece(plan: ShardPlan, side: int, j: int, r: int) -> ShardPiece:
    pc = ShardPiece()
    if lib().m4ri_amd_shard_piece_of(ctypes.byref(plan), side, j, r, ctypes.byref(pc)) != 0:
        raise ValueError("m4ri_amd_shard_piece_of: bad arguments")
    return pc


def shard_buffer_words(plan: ShardPlan, rank: int, which: int) -> int:
    return int(lib().m4ri_amd_shard_buffer_words(ctypes.byref(plan), rank, which))


def shard_slab_rows(plan: ShardPlan, rank: int, which: int) -> int:
    return int(lib().m4ri_amd_shard_slab_rows(ctypes.byref(plan), rank, which))


def shard_down_dev(plan: ShardPlan, rank: int, A_local: int, a_stride: int, B_local: int, b_stride: int,
                   child_a: int, child_b: int, stream: int = 0) -> None:
    _check(lib().m4ri_amd_shard_down_dev(ctypes.byref(plan), rank, A_local, a_stride, B_local, b_stride, child_a, child_b, stream),
           "m4ri_amd_shard_down_dev")


def shard_up_dev(plan: ShardPlan, rank: int, slabs_p: int, C_local: int, c_stride: int, add: bool = False, stream: int = 0) -> None:
    _check(lib().m4ri_amd_shard_up_dev(ctypes.byref(plan), rank, slabs_p, C_local, c_stride, int(add), stream), "m4ri_amd_shard_up_dev")


def mul_multi(C: Mzd, A: Mzd, B: Mzd, add: bool = False, cutoff: int = 0, levels: int = 0) -> Mzd:
    """C (+)= A*B over the configured devices (set_devices), host matrices in and out."""
    _check(lib().m4ri_amd_mul_multi(C.ptr, A.ptr, B.ptr, int(add), cutoff, levels), "m4ri_amd_mul_multi")
    return C


def set_devices(ids) -> None:
    """Devices mzd_mul_mp / mul_multi spread a product over; an id may repeat (ranks sharing a GPU);
    an empty list restores the default (M4RI_AMD_DEVICES or every visible device)."""
    arr = (ctypes.c_int * max(1, len(ids)))(*ids)
    if lib().m4ri_amd_set_devices(len(ids), arr) != 0:
        raise ValueError(f"m4ri_amd_set_devices({list(ids)}): unknown device id")


def get_devices() -> list:
    arr = (ctypes.c_int * 64)()
    n = lib().m4ri_amd_get_device_list(arr, 64)
    return [int(arr[i]) for i in range(min(n, 64))]


def set_multi_threshold(min_dim: int) -> int:
    return int(lib().m4ri_amd_set_multi_threshold(int(min_dim)))


# ---- residency (include/m4ri_amd.h part 3) --------------------------------------------------------
class Dmat:
    """A matrix distributed over the configured devices and resident in HBM (m4ri_amd_dmat, include/m4ri_amd.h part 4)."""

    def __init__(self, rows: int, ncols: int, layout: int = LAYOUT_ROWS):
        self.h = lib().m4ri_amd_dmat_create(rows, ncols, layout)
        if not self.h:
            raise RuntimeError(f"m4ri_amd_dmat_create({rows}, {ncols}, {layout}) failed")
        self.rows, self.ncols, self.layout = rows, ncols, layout

    def free(self):
        if self.h:
            lib().m4ri_amd_dmat_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def info(self) -> DmatInfo:
        out = DmatInfo()
        _check(lib().m4ri_amd_dmat_info(self.h, ctypes.byref(out)), "m4ri_amd_dmat_info")
        return out

    def local(self, rank: int):
        """(device pointer, rows incl. padding, HIP device) of rank `rank`'s local buffer."""
        ptr, rows, dev = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int()
        _check(lib().m4ri_amd_dmat_local(self.h, rank, ctypes.byref(ptr), ctypes.byref(rows), ctypes.byref(dev)), "m4ri_amd_dmat_local")
        return ptr.value, rows.value, dev.value

    def fill(self, seed: int) -> "Dmat":
        _check(lib().m4ri_amd_dmat_fill(self.h, seed), "m4ri_amd_dmat_fill")
        return self

    def upload(self, M: Mzd) -> "Dmat":
        _check(lib().m4ri_amd_dmat_upload(self.h, M.ptr), "m4ri_amd_dmat_upload")
        return self

    def download(self, M: Mzd = None) -> Mzd:
        M = M if M is not None else Mzd(self.rows, self.ncols)
        _check(lib().m4ri_amd_dmat_download(self.h, M.ptr), "m4ri_amd_dmat_download")
        return M

    def convert_from(self, src: "Dmat") -> "Dmat":
        _check(lib().m4ri_amd_dmat_convert(self.h, src.h), "m4ri_amd_dmat_convert")
        return self


def dmat_mul(C: Dmat, A: Dmat, B: Dmat, add: bool = False, cutoff: int = 0, variant: int = VARIANT_AUTO, lane: int = 0) -> Dmat:
    """C (+)= A*B on distributed operands; asynchronous (multi_sync).  lane 0 / 1: independent products issued alternately on the two
    lanes keep two in flight (m4ri_amd_dmat_mul_lane)."""
    if lane:
        _check(lib().m4ri_amd_dmat_mul_lane(C.h, A.h, B.h, int(add), cutoff, variant, lane), "m4ri_amd_dmat_mul_lane")
    else:
        _check(lib().m4ri_amd_dmat_mul(C.h, A.h, B.h, int(add), cutoff, variant), "m4ri_amd_dmat_mul")
    return C


def multi_pair_table(devices, can_access, no_peer: str = "") -> list:
    """The pure rule behind the multi-device path's pair table (no GPU): staged[dst][src] = 1 where copies dst <- src go through the
    host.  `can_access`: ndev x ndev nested lists (hipDeviceCanAccessPeer)."""
    w, ndev = len(devices), len(can_access)
    dev = (ctypes.c_int * w)(*devices)
    can = (ctypes.c_int * (ndev * ndev))(*[int(x) for row in can_access for x in row])
    out = ctypes.create_string_buffer(w * w)
    lib().m4ri_amd_multi_pair_table(w, dev, ndev, can, no_peer.encode() if no_peer else None, out)
    return [[out.raw[i * w + j] for j in range(w)] for i in range(w)]


def multi_link_probe(nbytes: int = 256 << 20) -> dict:
    """Every ordered pair of ranks copies `nbytes` one pair at a time, then all pairs at once (m4ri_amd_multi_link_probe)."""
    w = len(get_devices())
    pair = (ctypes.c_double * (w * w))()
    allg, same = ctypes.c_double(0.0), ctypes.c_int(0)
    staged = ctypes.create_string_buffer(w * w)
    _check(lib().m4ri_amd_multi_link_probe(nbytes, pair, ctypes.byref(allg), staged, ctypes.byref(same)), "m4ri_amd_multi_link_probe")
    rates = sorted(pair[i * w + j] for i in range(w) for j in range(w) if i != j)
    return {"bytes_per_copy": nbytes, "pairs": len(rates), "gbs_per_direction_min": rates[0] if rates else None,
            "gbs_per_direction_median": rates[len(rates) // 2] if rates else None, "gbs_per_direction_max": rates[-1] if rates else None,
            "all_at_once_gbs": allg.value, "all_at_once_gbs_per_direction": allg.value / max(1, len(rates)),
            "pair_gbs": [[round(pair[i * w + j], 2) for j in range(w)] for i in range(w)],
            "peer_access": [[int(i == j or not staged.raw[i * w + j]) for j in range(w)] for i in range(w)],
            "ranks_share_devices": bool(same.value)}


def multi_sync() -> None:
    _check(lib().m4ri_amd_multi_sync(), "m4ri_amd_multi_sync")


def multi_stats() -> MultiStats:
    out = MultiStats()
    _check(lib().m4ri_amd_multi_get_stats(ctypes.byref(out)), "m4ri_amd_multi_get_stats")
    return out


def multi_timeline(rank: int, cap: int = 256) -> list:
    buf = (ctypes.c_double * cap)()
    n = lib().m4ri_amd_multi_timeline(rank, buf, cap)
    if n < 0:
        raise RuntimeError("m4ri_amd_multi_timeline failed")
    return [buf[i] for i in range(n)]


def multi_default_variant(world: int, m: int, l: int, n: int) -> int:
    return lib().m4ri_amd_multi_default_variant(world, m, l, n)


def multi_layout_for(variant: int, world: int, m: int, l: int, n: int) -> int:
    return lib().m4ri_amd_multi_layout_for(variant, world, m, l, n)


def layout_runs(layout: int, world: int, rank: int, rows: int) -> list:
    """[(global first row, rows, local first row)] of the valid rows rank `rank` holds."""
    g0, nr, l0 = (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 4)()
    n = lib().m4ri_amd_layout_runs(layout, world, rank, rows, g0, nr, l0, 4)
    if n < 0:
        raise ValueError("m4ri_amd_layout_runs: bad arguments")
    return [(g0[i], nr[i], l0[i]) for i in range(n)]


def set_multi_variant(variant: int) -> int:
    return lib().m4ri_amd_set_multi_variant(variant)


def set_small_product_threshold(ops: int) -> int:
    """m * l * n at or below which a product from host memory is computed on the host (0: never); returns the previous value."""
    return int(lib().m4ri_amd_set_small_product_threshold(int(ops)))


def small_product_count() -> int:
    return int(lib().m4ri_amd_small_product_count())


def small_mul_host(C: Mzd, A: Mzd, B: Mzd, add: bool = False) -> Mzd:
    """The host Four Russians of the small-product path, called directly (no device involved)."""
    if lib().m4ri_amd_small_mul_host(C.ptr, A.ptr, B.ptr, int(add)) != 0:
        raise ValueError("m4ri_amd_small_mul_host: mismatched dimensions")
    return C


def pin(M: Mzd) -> None:
    """Keep a device copy of M (which must own its block); products then read it, and windows into it,
    in place and leave results there.  The host copy is stale after a product wrote into it until sync()."""
    if lib().m4ri_amd_pin(M.ptr) != 0:
        raise ValueError("m4ri_amd_pin: matrix is a window, empty or NULL")


def sync(M: Mzd) -> None:
    if lib().m4ri_amd_sync(M.ptr) != 0:
        raise ValueError("m4ri_amd_sync: matrix is not pinned")


def host_modified(M: Mzd) -> None:
    if lib().m4ri_amd_host_modified(M.ptr) != 0:
        raise ValueError("m4ri_amd_host_modified: matrix is not pinned")


def unpin(M: Mzd) -> None:
    if lib().m4ri_amd_unpin(M.ptr) != 0:
        raise ValueError("m4ri_amd_unpin: matrix is not pinned")


def is_pinned(M: Mzd) -> int:
    return int(lib().m4ri_amd_is_pinned(M.ptr))


def plan_row_blocks(m: int, l: int, n: int):
    """The engine's own plan (cutoff 0): [(rows, levels), ...], largest block of rows first (m4ri_amd_plan_row_blocks)."""
    rows = (ctypes.c_int64 * 16)()
    levels = (ctypes.c_int * 16)()
    k = int(lib().m4ri_amd_plan_row_blocks(m, l, n, ctypes.cast(rows, ctypes.c_void_p), ctypes.cast(levels, ctypes.c_void_p), 16))
    return [(int(rows[i]), int(levels[i])) for i in range(min(k, 16))]


def plan_leaf_launch(m: int, l: int, n: int, batch: int = 1, add: bool = False, ksplit: int = 0, cus: int = 0, a_prepacked: bool = False,
                     scratch_ok: bool = True) -> LeafPlan:
    """What one leaf launch of `batch` products of m x l x n does in this process (m4ri_amd_plan_leaf_launch; host arithmetic only).
    scratch_ok: the engine's packed-A scratch and slab region hold the launch (every entry but m4rm_batch_dev reserves them)."""
    p = LeafPlan()
    _check(lib().m4ri_amd_plan_leaf_launch(m, l, n, batch, int(bool(add)), ksplit, cus, int(bool(a_prepacked)), int(bool(scratch_ok)), ctypes.byref(p)),
           "m4ri_amd_plan_leaf_launch")
    return p


def model_seconds(m: int, l: int, n: int, levels: int) -> float:
    """The engine's time model for one product at a depth (m4ri_amd_model_seconds)."""
    return float(lib().m4ri_amd_model_seconds(m, l, n, levels))


def plan_levels(m: int, l: int, n: int, cutoff: int = 0) -> int:
    """Strassen-Winograd levels the engine would use (host logic only, no GPU needed)."""
    return int(lib().m4ri_amd_plan_levels(m, l, n, cutoff))


def set_workspace_budget(nbytes: int) -> int:
    """Bytes the breadth-first workspace may take (0 = automatic); returns the previous value."""
    return int(lib().m4ri_amd_set_workspace_budget(int(nbytes)))


def set_host_pipeline(min_bytes: int) -> int:
    """A + B + C bytes from which host-memory products are pipelined over row slabs (0 = never); returns the previous value."""
    return int(lib().m4ri_amd_set_host_pipeline(int(min_bytes)))


class HostPipelinePlan:
    """The blocks of a pipelined product from host memory: C_ij (+)= A_ik * B_kj between the cuts, and the staging arena's words."""

    def __init__(self, rcut, ccut, kcut, arena_words):
        self.rcut, self.ccut, self.kcut, self.arena_words = rcut, ccut, kcut, arena_words

    @property
    def grid(self):
        return (len(self.rcut) - 1, len(self.ccut) - 1, len(self.kcut) - 1)

    def __repr__(self):
        return f"HostPipelinePlan(rcut={self.rcut}, ccut={self.ccut}, kcut={self.kcut}, arena_words={self.arena_words})"


def plan_host_pipeline(m: int, l: int, n: int, min_bytes=None, grid=None):
    """What mzd_mul on m x l and l x n host matrices does (m4ri_amd_plan_host_pipeline; host arithmetic only): None when the product is
    not pipelined, else its HostPipelinePlan.  min_bytes: the pipeline's threshold (None: the library's current setting); grid: a
    requested block grid (gi, gj) or (gi, gj, gk), as M4RI_AMD_PIPE_GRID gives one."""
    if min_bytes is None:
        min_bytes = lib().m4ri_amd_set_host_pipeline(-1)
    gi, gj, gk = (0, 0, 0) if grid is None or len(grid) < 2 else (tuple(grid) + (1,))[:3]   # fewer than two numbers: no request
    cap, counts, words = 64, (ctypes.c_int * 3)(), ctypes.c_int64()
    while True:
        cuts = [(ctypes.c_int64 * cap)() for _ in range(3)]
        r = int(lib().m4ri_amd_plan_host_pipeline(m, l, n, int(min_bytes), gi, gj, gk, *[ctypes.cast(c, ctypes.c_void_p) for c in cuts], cap,
                                                  ctypes.cast(counts, ctypes.c_void_p), ctypes.cast(ctypes.pointer(words), ctypes.c_void_p)))
        if r == 0:
            return None
        if r > 0:
            return HostPipelinePlan(*[[int(c[q]) for q in range(k + 1)] for c, k in zip(cuts, counts)], int(words.value))
        cap = max(counts) + 1


def set_max_fuse(levels: int) -> int:
    """Deepest Strassen-Winograd levels covered by one fused pass (1..4); returns the previous value."""
    return int(lib().m4ri_amd_set_max_fuse(int(levels)))


def set_profiling(on) -> None:
    """0/False off, 1/True per product, 2 cumulative over products (Stats.cum_leaf_ms / cum_leaf_launches)."""
    lib().m4ri_amd_set_profiling(int(on))


def get_stats() -> Stats:
    s = Stats()
    _check(lib().m4ri_amd_get_stats(ctypes.byref(s)), "m4ri_amd_get_stats")
    return s
