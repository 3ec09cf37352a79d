"""ctypes binding of libamg_hip.so (C ABI: include/amg_hip.h).

Thin host-side mirror used by tests/, bench.py and the multi-GPU driver.  It
contains no arithmetic: every operation is a call through the C ABI into the
HIP kernels.  If the shared library is missing the import fails loudly; if no
HIP device is present every compute call raises AmgHipError (status EHIP) --
there is no CPU fallback.
"""
import collections
import contextlib
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libamg_hip.so")

OK, EINVAL, EHIP, ENOMEM, EUNSUPPORTED, ECOMM = 0, 1, 2, 3, 4, 5
SM_SPGS, SM_REF_JACOBI, SM_SOR, SM_JACOBI, SM_MULTICOLOR_GS, SM_CHEBYSHEV, SM_LINE_JACOBI = 0, 1, 2, 3, 4, 5, 6
SM_LINE_ALT = 7
LAYOUT_AUTO, LAYOUT_CSR, LAYOUT_SELL, LAYOUT_DICT = 0, 1, 2, 3
# AMG_HIP_LEG_*: the launch forms of the cycle plan, by value (Multigrid.leg_form returns these names)
LEG_FORMS = ("none", "plain", "pair", "duo_fine", "duo_coarse", "patch", "mc_patch", "mc_strip", "tail_head",
             "in_tail")
StripGeometry = collections.namedtuple("StripGeometry", "T tiles stages halo_down halo_up")

_i32p = C.POINTER(C.c_int32)
_f64p = C.POINTER(C.c_double)
_i64p = C.POINTER(C.c_int64)


class AmgHipError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"amg_hip status {status}: {msg}")
        self.status = status
        self.message = msg


class Options(C.Structure):
    _fields_ = [("smoother", C.c_int32), ("smoother_iters", C.c_int32),
                ("omega", C.c_double), ("device", C.c_int32), ("use_graph", C.c_int32),
                ("stencil_transfers", C.c_int32), ("layout", C.c_int32),
                ("host_only", C.c_int32), ("keep_structural_zeros", C.c_int32),
                ("no_fusion", C.c_int32), ("fuse_prolong", C.c_int32),
                ("fast_coarse_solve", C.c_int32), ("host_galerkin", C.c_int32),
                ("keep_residual", C.c_int32), ("exact_coarse_solve", C.c_int32),
                ("exact_gs", C.c_int32),
                ("cyclic_lines", C.c_int32),  # in the former alignment padding in front of `stream`
                ("stream", C.c_void_p), ("window", C.c_int32), ("cheb_degree", C.c_int32),
                ("cheb_lower", C.c_double), ("cheb_upper", C.c_double),
                ("natural_sides", C.c_int32), ("singular", C.c_int32)]


SLAB_MAX_LEVELS = 8


class SlabInfo(C.Structure):
    """amg_hip_slab_info (include/amg_hip.h)"""
    _fields_ = [("levels", C.c_int32), ("halo_lines", C.c_int32), ("lines", C.c_int64),
                ("chunk_lines", C.c_int64), ("line_begin", C.c_int64), ("line_end", C.c_int64),
                ("pitch0", C.c_int64), ("gather_pitch", C.c_int64), ("gather_rows", C.c_int64),
                ("down_lo", C.c_int64 * SLAB_MAX_LEVELS), ("down_hi", C.c_int64 * SLAB_MAX_LEVELS),
                ("up_lo", C.c_int64 * SLAB_MAX_LEVELS), ("up_hi", C.c_int64 * SLAB_MAX_LEVELS),
                ("u0", C.c_void_p), ("f_gather", C.c_void_p)]


class WindowPlanC(C.Structure):
    """amg_hip_window_plan (include/amg_hip.h)"""
    _fields_ = [(k, C.c_int64) for k in ("own0_off", "own0_end", "send_prev_cnt", "recv_prev_cnt",
                                         "send_next_cnt", "recv_next_cnt", "own_k_off", "own_k_cnt",
                                         "block_k", "uk_off")]


class HaloDesc(C.Structure):
    _fields_ = [("dst_prev", C.c_void_p), ("src_prev", C.c_void_p), ("bytes_prev", C.c_int64),
                ("dst_next", C.c_void_p), ("src_next", C.c_void_p), ("bytes_next", C.c_int64),
                ("data_flag_at_prev", C.c_void_p), ("data_flag_at_next", C.c_void_p),
                ("my_data_from_prev", C.c_void_p), ("my_data_from_next", C.c_void_p),
                ("ack_flag_at_prev", C.c_void_p), ("ack_flag_at_next", C.c_void_p),
                ("my_ack_from_prev", C.c_void_p), ("my_ack_from_next", C.c_void_p),
                ("epoch", C.c_uint32), ("recv_from_prev", C.c_int32), ("recv_from_next", C.c_int32)]


class HaloKDesc(C.Structure):
    _fields_ = [("dst_prev", C.c_void_p), ("src_prev", C.c_void_p), ("cnt_prev", C.c_int64),
                ("dst_next", C.c_void_p), ("src_next", C.c_void_p), ("cnt_next", C.c_int64),
                ("my_free_from_prev", C.c_void_p), ("my_free_from_next", C.c_void_p),
                ("data_at_prev", C.c_void_p), ("data_at_next", C.c_void_p),
                ("my_data_from_prev", C.c_void_p), ("my_data_from_next", C.c_void_p),
                ("recv_prev", C.c_int32), ("recv_next", C.c_int32), ("timeout", C.c_void_p)]


class GatherKDesc(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("src", C.c_void_p),
                ("cnt", C.c_int64), ("off", C.c_int64), ("dst", C.c_void_p * 16),
                ("data_at", C.c_void_p * 16), ("free_at", C.c_void_p * 16),
                ("my_data_from", C.c_void_p), ("my_free_from", C.c_void_p),
                ("timeout", C.c_void_p)]


# name -> (restype, argtypes).  Must list EVERY symbol include/amg_hip.h declares
# (tests/test_cabi_symbols.py checks the header against this table).
_SIGS = {
    "amg_hip_last_error": (C.c_char_p, []),
    "amg_hip_default_options": (None, [C.POINTER(Options)]),
    "amg_hip_device_count": (C.c_int, []),
    "amg_hip_set_default_layout": (None, [C.c_int32]),
    "amg_hip_create": (C.c_int, [C.c_int64, _i32p, _i32p, _f64p, _f64p, C.c_int32,
                                 C.POINTER(Options), C.POINTER(C.c_void_p)]),
    "amg_hip_create_custom": (C.c_int, [C.c_int64, _i32p, _i32p, _f64p, _f64p, C.c_int32,
                                        C.POINTER(_i32p), C.POINTER(_i32p), C.POINTER(_f64p),
                                        C.POINTER(_i32p), C.POINTER(_i32p), C.POINTER(_f64p),
                                        C.POINTER(Options), C.POINTER(C.c_void_p)]),
    "amg_hip_create_poisson": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.POINTER(Options),
                                         C.POINTER(C.c_void_p)]),
    "amg_hip_create_poisson_tensor": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.POINTER(Options),
                                                C.POINTER(C.c_void_p)]),
    "amg_hip_setup_on_device": (C.c_int, [C.c_void_p, _i32p]),
    "amg_hip_create_tensor": (C.c_int, [C.c_int64, _i32p, _i32p, _f64p, _f64p, C.c_int32, _i64p,
                                        C.c_int32, C.POINTER(Options), C.POINTER(C.c_void_p)]),
    "amg_hip_create_tensor_dev": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int32, _i64p, C.c_int32, C.POINTER(Options),
                                            C.POINTER(C.c_void_p)]),
    "amg_hip_get_level_dims": (C.c_int, [C.c_void_p, C.c_int32, _i64p]),
    "amg_hip_create_tensor_semi": (C.c_int, [C.c_int64, _i32p, _i32p, _f64p, _f64p, C.c_int32, _i64p,
                                             C.c_int32, _i32p, C.c_double, C.c_int64, C.POINTER(Options),
                                             C.POINTER(C.c_void_p)]),
    "amg_hip_create_tensor_semi_dev": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_int32, _i64p, C.c_int32, _i32p, C.c_double, C.c_int64,
                                                 C.POINTER(Options), C.POINTER(C.c_void_p)]),
    "amg_hip_get_level_axes": (C.c_int, [C.c_void_p, C.c_int32, _i32p]),
    "amg_hip_create_tensor_opdep": (C.c_int, [C.c_int64, _i32p, _i32p, _f64p, _f64p, C.c_int32, _i64p,
                                              C.c_int32, _i32p, C.c_int64, C.POINTER(Options),
                                              C.POINTER(C.c_void_p)]),
    "amg_hip_create_tensor_opdep_dev": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_int32, _i64p, C.c_int32, _i32p, C.c_int64,
                                                  C.POINTER(Options), C.POINTER(C.c_void_p)]),
    "amg_hip_create_tensor_opdep_periodic": (C.c_int, [C.c_int64, _i32p, _i32p, _f64p, _f64p, C.c_int32, _i64p,
                                                       C.c_int32, C.c_int32, _i32p, C.c_int64,
                                                       C.POINTER(Options), C.POINTER(C.c_void_p)]),
    "amg_hip_create_tensor_opdep_periodic_dev": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                           C.c_void_p, C.c_int32, _i64p, C.c_int32, C.c_int32,
                                                           _i32p, C.c_int64, C.POINTER(Options),
                                                           C.POINTER(C.c_void_p)]),
    "amg_hip_axis_restrict_per": (C.c_int, [C.c_int32, _i64p, C.c_int32, C.c_int32, _f64p, _f64p, _f64p,
                                            C.c_int32]),
    "amg_hip_axis_prolong_add_per": (C.c_int, [C.c_int32, _i64p, C.c_int32, C.c_int32, _f64p, _f64p, _f64p,
                                               C.c_int32]),
    "amg_hip_set_axis_stencil": (None, [C.c_int32]),
    "amg_hip_get_axis_weights": (C.c_int, [C.c_void_p, C.c_int32, _f64p]),
    "amg_hip_axis_restrict": (C.c_int, [C.c_int32, _i64p, C.c_int32, _f64p, _f64p, _f64p]),
    "amg_hip_axis_prolong_add": (C.c_int, [C.c_int32, _i64p, C.c_int32, _f64p, _f64p, _f64p]),
    "amg_hip_get_natural_sides": (C.c_int, [C.c_void_p, _i32p]),
    "amg_hip_create_tensor_periodic": (C.c_int, [C.c_int64, _i32p, _i32p, _f64p, _f64p, C.c_int32, _i64p,
                                                 C.c_int32, C.c_int32, _i32p, C.POINTER(Options),
                                                 C.POINTER(C.c_void_p)]),
    "amg_hip_create_tensor_periodic_dev": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_int32, _i64p, C.c_int32, C.c_int32, _i32p,
                                                     C.POINTER(Options), C.POINTER(C.c_void_p)]),
    "amg_hip_get_periodic_axes": (C.c_int, [C.c_void_p, _i32p]),
    "amg_hip_tensor_restrict_per": (C.c_int, [C.c_int32, _i64p, C.c_int32, C.c_int32, C.c_int32, _f64p, _f64p]),
    "amg_hip_tensor_prolong_add_per": (C.c_int, [C.c_int32, _i64p, C.c_int32, C.c_int32, C.c_int32, _f64p, _f64p]),
    "amg_hip_tensor_restrict_bc": (C.c_int, [C.c_int32, _i64p, C.c_int32, C.c_int32, _f64p, _f64p]),
    "amg_hip_tensor_prolong_add_bc": (C.c_int, [C.c_int32, _i64p, C.c_int32, C.c_int32, _f64p, _f64p]),
    "amg_hip_tensor_axis_strength": (C.c_int, [C.c_int64, _i32p, _i32p, _f64p, C.c_int32, _i64p, _f64p]),
    "amg_hip_tensor_restrict_axes": (C.c_int, [C.c_int32, _i64p, C.c_int32, _f64p, _f64p]),
    "amg_hip_tensor_prolong_add_axes": (C.c_int, [C.c_int32, _i64p, C.c_int32, _f64p, _f64p]),
    "amg_hip_level_transfer_kind": (C.c_int, [C.c_void_p, C.c_int32, _i32p]),
    "amg_hip_tensor_restrict": (C.c_int, [C.c_int32, _i64p, _f64p, _f64p]),
    "amg_hip_tensor_prolong_add": (C.c_int, [C.c_int32, _i64p, _f64p, _f64p]),
    "amg_hip_destroy": (None, [C.c_void_p]),
    "amg_hip_vcycle": (C.c_int, [C.c_void_p]),
    "amg_hip_vcycles": (C.c_int, [C.c_void_p, C.c_int32]),
    "amg_hip_sync": (C.c_int, [C.c_void_p]),
    "amg_hip_solve": (C.c_int, [C.c_void_p, C.c_double, C.c_int64, C.c_int64, _i64p, _f64p,
                                _i32p]),
    "amg_hip_rss": (C.c_int, [C.c_void_p, _f64p]),
    "amg_hip_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "amg_hip_pcg": (C.c_int, [C.c_void_p, C.c_double, C.c_int64, _i64p, _f64p]),
    "amg_hip_set_mean_projection": (C.c_int, [C.c_void_p, C.c_int32]),
    "amg_hip_get_mean_projection": (C.c_int, [C.c_void_p, _i32p]),
    "amg_hip_center_vec": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "amg_hip_block_vcycles": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]),
    "amg_hip_block_rss": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, _f64p]),
    "amg_hip_block_pcg": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_int64,
                                    _i64p, _f64p]),
    "amg_hip_block_must_move": (C.c_int, [C.c_void_p, C.c_int32, _f64p]),
    "amg_hip_apply_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "amg_hip_pcg_mixed": (C.c_int, [C.c_void_p, C.c_double, C.c_int64, _i64p, _f64p]),
    "amg_hip_f32_must_move": (C.c_int, [C.c_void_p, _f64p]),
    "amg_hip_f32_get_vec": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_float)]),
    "amg_hip_f32_set_vec": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_float)]),
    "amg_hip_f32_level_op": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "amg_hip_f32_line_subsweep": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "amg_hip_f32_line_factors": (C.c_int, [C.c_void_p, C.c_int32] + [C.POINTER(C.c_float)] * 3),
    "amg_hip_set_f32_lines": (None, [C.c_int32]),
    "amg_hip_set_f32_dict": (None, [C.c_int32]),
    "amg_hip_set_block_lines": (None, [C.c_int32]),
    "amg_hip_n_levels": (C.c_int32, [C.c_void_p]),
    "amg_hip_get_n_dofs": (C.c_int64, [C.c_void_p, C.c_int32]),
    "amg_hip_get_level_nnz": (C.c_int64, [C.c_void_p, C.c_int32]),
    "amg_hip_get_level_matrix": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i32p, _f64p]),
    "amg_hip_get_transfer_nnz": (C.c_int64, [C.c_void_p, C.c_int32, C.c_int32]),
    "amg_hip_get_transfer": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _i32p, _i32p, _f64p]),
    "amg_hip_get_vec": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _f64p]),
    "amg_hip_set_vec": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _f64p]),
    "amg_hip_copy_vec_dev": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]),
    "amg_hip_zero_vec": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "amg_hip_coarse_halfbw": (C.c_int64, [C.c_void_p]),
    "amg_hip_coarse_solve_kind": (C.c_int32, [C.c_void_p]),
    "amg_hip_fine_sweep_info": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, _i32p, _f64p]),
    "amg_hip_set_patch_min_rows": (None, [C.c_int64]),
    "amg_hip_set_band_chain": (None, [C.c_int32]),
    "amg_hip_set_tail_fusion": (None, [C.c_int32]),
    "amg_hip_set_pair_duo": (None, [C.c_int32]),
    "amg_hip_pair_duo_partner": (C.c_int32, [C.c_void_p, C.c_int32]),
    "amg_hip_duo_windows": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, _i32p]),
    "amg_hip_duo_owned": (C.c_int32, [C.c_int32, C.c_int32, _i32p]),
    "amg_hip_duo_tile_rows": (C.c_int32, [C.c_int32]),
    "amg_hip_set_periodic_device_setup": (None, [C.c_int32]),
    "amg_hip_set_patch_tile_flags": (None, [C.c_int32]),
    "amg_hip_set_patch_xf": (None, [C.c_int32]),
    "amg_hip_set_patch_tall": (None, [C.c_int32]),
    "amg_hip_set_patch_coltype": (None, [C.c_int32]),
    "amg_hip_patch_tile_classes": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _i64p]),
    "amg_hip_set_patch_seam": (None, [C.c_int32]),
    "amg_hip_patch_leg_lines": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32]),
    "amg_hip_level_leg_form": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i32p]),
    "amg_hip_strip_geometry": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i32p, _i32p, _i32p, _i32p]),
    "amg_hip_create_rs": (C.c_int, [C.c_int64, _i32p, _i32p, _f64p, _f64p, C.c_int32, C.c_double, C.c_int64,
                                    C.POINTER(Options), C.POINTER(C.c_void_p)]),
    "amg_hip_slab_plan": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(SlabInfo)]),
    "amg_hip_slab_setup": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(SlabInfo)]),
    "amg_hip_slab_run": (C.c_int, [C.c_void_p, C.c_int32]),
    "amg_hip_create_poisson_window": (C.c_int, [C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                                C.POINTER(Options), C.POINTER(C.c_void_p)]),
    "amg_hip_window_setup": (C.c_int, [C.c_void_p, _i64p, _i64p, _i64p, _i64p]),
    "amg_hip_window_run": (C.c_int, [C.c_void_p, C.c_int32]),
    "amg_hip_vec_dev_ptr": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), _i64p]),
    "amg_hip_get_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "amg_hip_comm_unique_id": (C.c_int, [C.c_char_p]),
    "amg_hip_comm_create": (C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "amg_hip_comm_destroy": (None, [C.c_void_p]),
    "amg_hip_comm_rank": (C.c_int32, [C.c_void_p]),
    "amg_hip_comm_world": (C.c_int32, [C.c_void_p]),
    "amg_hip_comm_neighbor_exchange": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                 C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "amg_hip_comm_all_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "amg_hip_slab_cycle": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(SlabInfo)]),
    "amg_hip_window_cycle": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(WindowPlanC)]),
    "amg_hip_level_layout": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "amg_hip_get_colors": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i32p]),
    "amg_hip_level_op": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "amg_hip_cheb_bounds": (C.c_int, [C.c_void_p, C.c_int32, _f64p, _f64p]),
    "amg_hip_line_stride": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]),
    "amg_hip_smooth_line": (C.c_int, [C.c_int64, _i32p, _i32p, _f64p, C.c_int64, C.c_double, C.c_int64,
                                      _f64p, _f64p]),
    "amg_hip_line_directions": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "amg_hip_smooth_line_alt": (C.c_int, [C.c_int64, _i32p, _i32p, _f64p, C.c_int32, C.POINTER(C.c_int64),
                                          C.c_double, C.c_int64, C.c_int32, _f64p, _f64p]),
    "amg_hip_line_cyclic": (C.c_int, [C.c_void_p, C.c_int32, _i32p]),
    "amg_hip_smooth_line_alt_per": (C.c_int, [C.c_int64, _i32p, _i32p, _f64p, C.c_int32, C.POINTER(C.c_int64),
                                              C.c_int32, C.c_double, C.c_int64, C.c_int32, _f64p, _f64p]),
    "amg_hip_smooth_chebyshev": (C.c_int, [C.c_int64, _i32p, _i32p, _f64p, _f64p, _f64p, C.c_int32,
                                           C.c_double, C.c_double, C.c_int64]),
    "amg_hip_cycle_bytes": (C.c_int, [C.c_void_p, _f64p, _f64p]),
    "amg_hip_cycle_must_move": (C.c_int, [C.c_void_p, C.c_int32, _f64p]),
    "amg_hip_profile_fine_sweep": (C.c_int, [C.c_void_p, C.c_int32, _f64p, _f64p]),
    "amg_hip_smooth": (C.c_int, [C.c_int32, C.c_int64, _i32p, _i32p, _f64p, _f64p, _f64p,
                                 C.c_double, C.c_double, C.c_int64, C.c_int64, _i64p, _i32p]),
    "amg_hip_spgs_sweep": (C.c_int, [C.c_int32, C.c_int64, _i32p, _i32p, _f64p, _f64p, _f64p]),
    "amg_hip_residual": (C.c_int, [C.c_int64, _i32p, _i32p, _f64p, _f64p, _f64p, _f64p]),
    "amg_hip_spmv": (C.c_int, [C.c_int64, C.c_int64, _i32p, _i32p, _f64p, _f64p, _f64p]),
    "amg_hip_linear_restrict": (C.c_int, [C.c_int64, C.c_int64, _f64p, _f64p]),
    "amg_hip_linear_prolong_add": (C.c_int, [C.c_int64, C.c_int64, _f64p, _f64p]),
    "amg_hip_rss_host": (C.c_int, [C.c_int64, _i32p, _i32p, _f64p, _f64p, _f64p, _f64p]),
    "amg_hip_coarse_solve": (C.c_int, [C.c_int64, _i32p, _i32p, _f64p, _f64p, _f64p, _i64p]),
    "amg_hip_coarse_solve_fast": (C.c_int, [C.c_int64, _i32p, _i32p, _f64p, _f64p, _f64p, _i64p,
                                            _i32p]),
    "amg_hip_laplacian": (C.c_int64, [C.c_int32, C.c_int64, _i32p, _i32p, _f64p]),
    "amg_hip_rhs": (C.c_int, [C.c_int32, C.c_int64, _f64p]),
    "amg_hip_csr_shape": (C.c_int, [C.c_int64, _i32p, _i32p, _i32p]),
    "amg_hip_dev_residual": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "amg_hip_dev_jacobi": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_double, C.c_int64, C.c_void_p]),
    "amg_hip_dev_spmv": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "amg_hip_devmat_create": (C.c_int, [C.c_int64, C.c_int64, _i32p, _i32p, _f64p, C.c_int32,
                                        C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]),
    "amg_hip_set_index16": (None, [C.c_int32]),
    "amg_hip_set_nontemporal": (None, [C.c_int32]),
    "amg_hip_set_dict_rows": (None, [C.c_int32]),
    "amg_hip_set_dict_stencil": (None, [C.c_int32]),
    "amg_hip_set_xcd_mapping": (None, [C.c_int32]),
    "amg_hip_set_row_types": (None, [C.c_int32]),
    "amg_hip_dict_probe": (C.c_int, [C.c_int64, C.c_int64, _i32p, _i32p, _f64p, C.c_int64,
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "amg_hip_devmat_destroy": (None, [C.c_void_p]),
    "amg_hip_devmat_layout": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "amg_hip_devmat_apply": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_double, C.c_int64, C.c_void_p]),
    "amg_hip_dev_jacobi_from_zero": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_double, C.c_void_p]),
    "amg_hip_dev_axpy1": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "amg_hip_arena_create": (C.c_int, [C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]),
    "amg_hip_arena_destroy": (None, [C.c_void_p]),
    "amg_hip_arena_base": (C.c_void_p, [C.c_void_p]),
    "amg_hip_arena_export": (C.c_int, [C.c_void_p, C.c_char_p]),
    "amg_hip_arena_open_peer": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "amg_hip_arena_close_peer": (C.c_int, [C.c_void_p]),
    "amg_hip_halo_push_wait": (C.c_int, [C.POINTER(HaloDesc), C.c_void_p]),
    "amg_hip_halo_ack": (C.c_int, [C.POINTER(HaloDesc), C.c_void_p]),
    "amg_hip_halo_exchange_kernel": (C.c_int, [C.POINTER(HaloKDesc), C.c_void_p]),
    "amg_hip_halo_ack_kernel": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "amg_hip_gather_kernel": (C.c_int, [C.POINTER(GatherKDesc), C.c_void_p]),
    "amg_hip_gather_ack_kernel": (C.c_int, [C.POINTER(GatherKDesc), C.c_void_p]),
    "amg_hip_fill_u32": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p]),
    "amg_hip_capture_begin": (C.c_int, [C.c_void_p]),
    "amg_hip_capture_end": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "amg_hip_graph_launch": (C.c_int, [C.c_void_p, C.c_void_p]),
    "amg_hip_graph_destroy": (None, [C.c_void_p]),
    "amg_hip_dev_sumsq": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.environ.get("AMG_HIP_LIBRARY", LIB_PATH)   # another build of the same ABI
        if not os.path.exists(path):
            raise ImportError(
                f"{path} not found: build it with `make -C {_HERE}` "
                "(or __graft_entry__.build()); there is no fallback implementation")
        L = C.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _chk(status):
    if status != OK:
        raise AmgHipError(status, lib().amg_hip_last_error().decode())


def _a32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _a64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p32(a):
    return a.ctypes.data_as(_i32p)


def _p64(a):
    return a.ctypes.data_as(_f64p)


def device_count():
    return lib().amg_hip_device_count()


def set_default_layout(layout):
    lib().amg_hip_set_default_layout(layout)


def set_index16(on):
    lib().amg_hip_set_index16(int(on))


def set_nontemporal(on):
    lib().amg_hip_set_nontemporal(int(on))


def set_dict_rows(rows_per_lane):
    lib().amg_hip_set_dict_rows(int(rows_per_lane))


def set_dict_stencil(on):
    lib().amg_hip_set_dict_stencil(int(on))


def dict_probe(rowptr, col, val, ncols, diag_shift=0):
    """Host-only: (n_pairs, n_row_types, words) of the dictionary coding of a CSR block, or
    None when the block does not qualify.  Raises when the coding does not round-trip."""
    rowptr, col, val = _a32(rowptr), _a32(col), _a64(val)
    a, b, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    st = lib().amg_hip_dict_probe(rowptr.size - 1, ncols, _p32(rowptr), _p32(col), _p64(val),
                                  diag_shift, C.byref(a), C.byref(b), C.byref(c))
    if st == EUNSUPPORTED:
        return None
    _chk(st)
    return a.value, b.value, c.value


class Comm:
    """amg_hip_comm: the library's own RCCL communicator (include/amg_hip.h "communicator").
    id_bytes: the 128 bytes rank 0 got from Comm.unique_id(), handed to every rank by the caller."""

    def __init__(self, id_bytes, rank, world, device=-1):
        h = C.c_void_p()
        _chk(lib().amg_hip_comm_create(bytes(id_bytes), int(rank), int(world), int(device), C.byref(h)))
        self._h, self.rank, self.world = h, rank, world

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        _chk(lib().amg_hip_comm_unique_id(buf))
        return buf.raw

    def slab_cycle(self, mg, info):
        _chk(lib().amg_hip_slab_cycle(mg._h, self._h, C.byref(info)))

    def window_cycle(self, window_mg, tail_mg, plan_c):
        _chk(lib().amg_hip_window_cycle(window_mg._h, tail_mg._h, self._h, C.byref(plan_c)))

    def close(self):
        if getattr(self, "_h", None):
            lib().amg_hip_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def slab_plan(lines, rank, world, levels):
    """Host arithmetic of the slab sharding (no device): SlabInfo with the line ranges."""
    info = SlabInfo()
    _chk(lib().amg_hip_slab_plan(int(lines), int(rank), int(world), int(levels), C.byref(info)))
    return info


def set_patch_tile_flags(on):
    lib().amg_hip_set_patch_tile_flags(int(bool(on)))


def set_axis_stencil(on):
    """A/B switch: False makes solvers created by Multigrid.tensor_opdep from now on run their transfers
    as CSR SpMV (kind 0) instead of K-AxisRestrict / K-AxisProlong (kind 3); same bits either way."""
    lib().amg_hip_set_axis_stencil(int(bool(on)))


def set_patch_xf(on):
    lib().amg_hip_set_patch_xf(int(bool(on)))


def set_patch_tall(on):
    lib().amg_hip_set_patch_tall(int(bool(on)))


def set_patch_coltype(on):
    """K-Patch column-typed tiles (flag 254: the tiles at the line ends) on (the default) / off; process-wide,
    read when a solver is created, same bits either way"""
    lib().amg_hip_set_patch_coltype(int(bool(on)))


def set_patch_seam(on):
    lib().amg_hip_set_patch_seam(int(bool(on)))


def set_tail_fusion(on):
    lib().amg_hip_set_tail_fusion(int(bool(on)))


def set_pair_duo(on):
    """K-Duo (two consecutive pair levels per launch) on (the default) / off; process-wide, read when a
    solver is created, same bits either way"""
    lib().amg_hip_set_pair_duo(int(bool(on)))


DUO_WINDOWS_LEN = 31


def duo_windows(hb_l, hb_l1, tile_rows=510):
    """(fits, windows): amg_hip_duo_windows -- the 31 numbers described in include/amg_hip.h"""
    out = np.zeros(DUO_WINDOWS_LEN, np.int32)
    rc = lib().amg_hip_duo_windows(int(hb_l), int(hb_l1), int(tile_rows), out.ctypes.data_as(_i32p))
    return rc == 0, out


def duo_owned(tile, tile_rows=510):
    """three half-open row ranges (levels l, l+1, l+2) that K-Duo tile number `tile` owns, unclipped"""
    out = np.zeros(6, np.int32)
    if lib().amg_hip_duo_owned(int(tile), int(tile_rows), out.ctypes.data_as(_i32p)) != 0:
        raise ValueError("amg_hip_duo_owned: bad argument")
    return [(int(out[0]), int(out[1])), (int(out[2]), int(out[3])), (int(out[4]), int(out[5]))]


def duo_tile_rows(hb_l):
    """rows of level l per tile that the K-Duo launchers use under half-bandwidth hb_l"""
    return int(lib().amg_hip_duo_tile_rows(int(hb_l)))


def set_periodic_device_setup(on):
    """Multigrid.tensor_periodic_dev and Multigrid.tensor_opdep_periodic_dev build on the device (1) or
    through the host constructor (0, the default); process-wide, read when a solver is created, the same
    solver bit for bit."""
    lib().amg_hip_set_periodic_device_setup(int(bool(on)))


def set_f32_lines(on):
    """The single-precision entry points accept line-smoother solvers (1) or refuse them (0, the
    default); process-wide, read whenever a float entry point runs its checks."""
    lib().amg_hip_set_f32_lines(int(bool(on)))


@contextlib.contextmanager
def f32_lines():
    """with amg.f32_lines(): ... -- set_f32_lines(1) inside the block, 0 again after it."""
    set_f32_lines(1)
    try:
        yield
    finally:
        set_f32_lines(0)


def set_f32_dict(on):
    """The single-precision entry points accept solvers with dictionary-coded levels (1) or refuse them
    (0, the default); process-wide, read when a float entry point first makes a solver's float copies."""
    lib().amg_hip_set_f32_dict(int(bool(on)))


@contextlib.contextmanager
def f32_dict():
    """with amg.f32_dict(): ... -- set_f32_dict(1) inside the block, 0 again after it."""
    set_f32_dict(1)
    try:
        yield
    finally:
        set_f32_dict(0)


def set_block_lines(on):
    """The block entry points accept line-smoother solvers (1) or refuse them (0, the default);
    process-wide, read whenever a block entry point runs its checks."""
    lib().amg_hip_set_block_lines(int(bool(on)))


@contextlib.contextmanager
def block_lines():
    """with amg.block_lines(): ... -- set_block_lines(1) inside the block, 0 again after it."""
    set_block_lines(1)
    try:
        yield
    finally:
        set_block_lines(0)


def set_band_chain(on):
    lib().amg_hip_set_band_chain(int(bool(on)))


PATCH_MIN_ROWS_DEFAULT = 1000000   # the library's default K-Patch threshold (amg_hip_set_patch_min_rows)


def set_patch_min_rows(rows):
    lib().amg_hip_set_patch_min_rows(int(rows))


def set_row_types(on):
    lib().amg_hip_set_row_types(int(on))


def set_xcd_mapping(on):
    lib().amg_hip_set_xcd_mapping(int(on))


class DevMat:
    """amg_hip_devmat: a CSR block (rows x ncols, row i's diagonal in column i + diag_shift) uploaded
    in one of the solver's device layouts; exact zeros are pruned.  The operations take and return
    numpy arrays and move them through torch tensors on `device`."""

    RESIDUAL, JACOBI, SPMV = 0, 1, 2

    def __init__(self, rowptr, col, val, ncols, layout=LAYOUT_AUTO, diag_shift=0, device=0):
        rowptr, col, val = _a32(rowptr), _a32(col), _a64(val)
        self.rows, self.cols = int(rowptr.size - 1), int(ncols)
        self.diag_shift, self.device = int(diag_shift), int(device)
        self._h = C.c_void_p()
        st = lib().amg_hip_devmat_create(self.rows, self.cols, _p32(rowptr), _p32(col), _p64(val), int(layout),
                                         self.diag_shift, self.device, C.byref(self._h))
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)

    def layout(self):
        """(LAYOUT_CSR / _SELL / _DICT, bytes of the matrix stream of one application)."""
        lay, nb = C.c_int32(0), C.c_int64(0)
        _chk(lib().amg_hip_devmat_layout(self._h, C.byref(lay), C.byref(nb)))
        return lay.value, int(nb.value)

    def apply(self, op, x, f=None, omega=1.0, diag_shift=None):
        """RESIDUAL: f - A x;  JACOBI: one sweep x_i + omega ((f_i - sum_{j != i} a_ij x_j) / a_ii - x_i)
        for the rows' own entries x[diag_shift : diag_shift + rows] (rows without a diagonal keep
        theirs);  SPMV: A x.  x has `ncols` entries, f and the result `rows`."""
        import torch
        if not self._h:
            raise ValueError("DevMat is closed")
        x = _a64(x)
        if x.size != self.cols:
            raise ValueError(f"`x` must have {self.cols} entries, got {x.size}")
        if op != self.SPMV:
            if f is None:
                raise ValueError("`f` is required for this operation")
            f = _a64(f)
            if f.size != self.rows:
                raise ValueError(f"`f` must have {self.rows} entries, got {f.size}")
        shift = self.diag_shift if diag_shift is None else int(diag_shift)
        if op == self.JACOBI and (shift < 0 or self.rows + shift > self.cols):
            raise ValueError("a Jacobi sweep needs rows + diag_shift <= ncols")
        dev = torch.device("cuda", self.device)
        xt = torch.tensor(x, device=dev)    # copies: x may be read-only
        ft = torch.tensor(f, device=dev) if op != self.SPMV else None
        out = torch.empty(self.rows, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        st = lib().amg_hip_devmat_apply(self._h, int(op), xt.data_ptr(), ft.data_ptr() if ft is not None else None,
                                        out.data_ptr(), float(omega), shift, None)
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        torch.cuda.synchronize(dev)
        return out.cpu().numpy()

    def close(self):
        if self._h:
            lib().amg_hip_devmat_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- Grid<double> ------------------------------------------------------------
def laplacian(n, dim=2):
    """grid.hpp:88-98.  Returns (colptr, rowind, val) of the CSC matrix."""
    nnz = lib().amg_hip_laplacian(dim, n, None, None, None)
    if nnz < 0:
        raise AmgHipError(EINVAL, lib().amg_hip_last_error().decode())
    N = n ** dim
    colptr = np.empty(N + 1, np.int32)
    rowind = np.empty(nnz, np.int32)
    val = np.empty(nnz, np.float64)
    got = lib().amg_hip_laplacian(dim, n, _p32(colptr), _p32(rowind), _p64(val))
    assert got == nnz
    return colptr, rowind, val


def rhs(n, dim=2):
    b = np.empty(n ** dim, np.float64)
    _chk(lib().amg_hip_rhs(dim, n, _p64(b)))
    return b


# ---- AMG::Multigrid<double> ----------------------------------------------------
class Multigrid:
    """Mirror of AMG::Multigrid<double> (multigrid.hpp) over the C ABI."""

    def __init__(self, colptr, rowind, val, b, n_levels, smoother=SM_SPGS,
                 smoother_iters=1, omega=1.0, tolerance=1e-9, compute_error_every_n_iters=10,
                 n_iters=100, device=-1, use_graph=True, stencil_transfers=True,
                 transfers=None, layout=None, host_only=False, keep_structural_zeros=False,
                 no_fusion=False, fuse_prolong=False, stream=None, fast_coarse_solve=False,
                 host_galerkin=False, keep_residual=False, exact_coarse_solve=False,
                 exact_gs=False, cheb_degree=2, cheb_lower=0.3, cheb_upper=1.0):
        # multigrid.hpp:165-178 (same checks, same order)
        if compute_error_every_n_iters > n_iters:
            raise ValueError("`compute_error_every_n_iters` must be leq to `n_iters`, got "
                             f"{compute_error_every_n_iters} and {n_iters}")
        colptr, rowind, val, b = _a32(colptr), _a32(rowind), _a64(val), _a64(b)
        n = colptr.size - 1
        if n != b.size:
            raise ValueError("`A` and `b` must have the same number of degrees of freedom, "
                             f"got {n} and {b.size}")
        self.tolerance = tolerance
        self.every = compute_error_every_n_iters
        self.n_iters = n_iters
        o = self._options(smoother, smoother_iters, omega, device, use_graph, stencil_transfers, layout,
                          host_only, keep_structural_zeros, no_fusion, fuse_prolong, stream,
                          fast_coarse_solve, host_galerkin, keep_residual, exact_coarse_solve, exact_gs,
                          cheb_degree, cheb_lower, cheb_upper)
        h = C.c_void_p()
        if transfers is None:
            st = lib().amg_hip_create(n, _p32(colptr), _p32(rowind), _p64(val), _p64(b),
                                      n_levels, C.byref(o), C.byref(h))
        else:
            # transfers: list over levels of (P_csc, R_csc), each (colptr,rowind,val)
            keep = []
            arrs = [[], [], [], [], [], []]
            for (P, R) in transfers:
                for k, a in enumerate((_a32(P[0]), _a32(P[1]), _a64(P[2]),
                                       _a32(R[0]), _a32(R[1]), _a64(R[2]))):
                    keep.append(a)
                    arrs[k].append(a)
            nl = len(transfers)

            def tab(lst, ptr_t, conv):
                t = (ptr_t * max(nl, 1))()
                for i, a in enumerate(lst):
                    t[i] = conv(a)
                return t
            st = lib().amg_hip_create_custom(
                n, _p32(colptr), _p32(rowind), _p64(val), _p64(b), n_levels,
                tab(arrs[0], _i32p, _p32), tab(arrs[1], _i32p, _p32), tab(arrs[2], _f64p, _p64),
                tab(arrs[3], _i32p, _p32), tab(arrs[4], _i32p, _p32), tab(arrs[5], _f64p, _p64),
                C.byref(o), C.byref(h))
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        self._h = h
        self._device = device

    @staticmethod
    def _options(smoother, smoother_iters, omega, device, use_graph, stencil_transfers, layout,
                 host_only, keep_structural_zeros, no_fusion, fuse_prolong, stream,
                 fast_coarse_solve, host_galerkin, keep_residual, exact_coarse_solve, exact_gs,
                 cheb_degree=2, cheb_lower=0.3, cheb_upper=1.0):
        o = Options()
        lib().amg_hip_default_options(C.byref(o))
        o.smoother, o.smoother_iters, o.omega = smoother, smoother_iters, omega
        o.device, o.use_graph, o.stencil_transfers = device, int(use_graph), int(stencil_transfers)
        if layout is not None:
            o.layout = layout
        o.host_only = int(host_only)
        o.keep_structural_zeros = int(keep_structural_zeros)
        o.no_fusion = int(no_fusion)
        o.fuse_prolong = int(fuse_prolong)
        o.fast_coarse_solve = int(fast_coarse_solve)
        o.host_galerkin = int(host_galerkin)
        o.keep_residual = int(keep_residual)
        o.exact_coarse_solve = int(exact_coarse_solve)
        o.exact_gs = int(exact_gs)
        o.cheb_degree, o.cheb_lower, o.cheb_upper = int(cheb_degree), float(cheb_lower), float(cheb_upper)
        if stream:
            o.stream = C.c_void_p(stream)
        return o

    @classmethod
    def ruge_stueben(cls, colptr, rowind, val, b, max_levels=25, theta=0.25, min_coarse=500,
                     smoother=SM_SPGS, smoother_iters=1, omega=1.0, tolerance=1e-9,
                     compute_error_every_n_iters=10, n_iters=100, device=-1, use_graph=True, layout=None,
                     host_only=False, stream=None, host_galerkin=False, exact_coarse_solve=False,
                     exact_gs=False, cheb_degree=2, cheb_lower=0.3, cheb_upper=1.0):
        """AMG::Multigrid on a strength-based C/F hierarchy (amg_hip_create_rs): same V-cycle,
        coarsening by the classical Ruge-Stueben first pass with direct interpolation.
        `self.n_levels` tells how many levels were built."""
        colptr, rowind, val, b = _a32(colptr), _a32(rowind), _a64(val), _a64(b)
        n = colptr.size - 1
        if n != b.size:
            raise ValueError("`A` and `b` must have the same number of degrees of freedom, "
                             f"got {n} and {b.size}")
        self = cls.__new__(cls)
        self.tolerance, self.every, self.n_iters = tolerance, compute_error_every_n_iters, n_iters
        o = cls._options(smoother, smoother_iters, omega, device, use_graph, True, layout, host_only,
                         False, False, False, stream, False, host_galerkin, False, exact_coarse_solve,
                         exact_gs, cheb_degree, cheb_lower, cheb_upper)
        h = C.c_void_p()
        st = lib().amg_hip_create_rs(n, _p32(colptr), _p32(rowind), _p64(val), _p64(b), int(max_levels),
                                     float(theta), int(min_coarse), C.byref(o), C.byref(h))
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        self._h = h
        self._device = device
        return self

    @classmethod
    def tensor(cls, colptr, rowind, val, b, dims, n_levels, smoother=SM_SPGS, smoother_iters=1, omega=1.0,
               tolerance=1e-9, compute_error_every_n_iters=10, n_iters=100, device=-1, use_graph=True,
               stencil_transfers=True, layout=None, host_only=False, keep_structural_zeros=False,
               no_fusion=False, stream=None, fast_coarse_solve=False, keep_residual=False,
               exact_coarse_solve=False, exact_gs=False, cheb_degree=2, cheb_lower=0.3, cheb_upper=1.0,
               window=False, natural_sides=0, singular=False, cyclic_lines=False, _semi=None, _periodic=None,
               _opdep=None, _opdep_per=None):
        """AMG::Multigrid on a FULL-coarsening hierarchy of the grid `dims` = (nx, ny) or (nx, ny, nz),
        x fastest (amg_hip_create_tensor): every axis m -> m // 2, tensor-product linear interpolation,
        matrix-free transfer kernels unless stencil_transfers=False.  A is the caller's matrix on
        that grid.  natural_sides: mask of the sides without a Dirichlet condition (bit 2a = low side
        of axis a, bit 2a + 1 = high side); singular=True (all sides natural): A has the constants as
        its null space and the coarsest solve pins its last unknown."""
        if compute_error_every_n_iters > n_iters:
            raise ValueError("`compute_error_every_n_iters` must be leq to `n_iters`, got "
                             f"{compute_error_every_n_iters} and {n_iters}")
        colptr, rowind, val, b = _a32(colptr), _a32(rowind), _a64(val), _a64(b)
        n = colptr.size - 1
        if n != b.size:
            raise ValueError("`A` and `b` must have the same number of degrees of freedom, "
                             f"got {n} and {b.size}")
        dim, d3 = _dims3(dims)
        self = cls.__new__(cls)
        self.tolerance, self.every, self.n_iters = tolerance, compute_error_every_n_iters, n_iters
        o = cls._options(smoother, smoother_iters, omega, device, use_graph, stencil_transfers, layout,
                         host_only, keep_structural_zeros, no_fusion, False, stream, fast_coarse_solve,
                         False, keep_residual, exact_coarse_solve, exact_gs, cheb_degree, cheb_lower,
                         cheb_upper)
        o.window = int(window)
        o.natural_sides, o.singular = int(natural_sides), int(singular)
        o.cyclic_lines = int(cyclic_lines)
        h = C.c_void_p()
        if _periodic is not None:  # tensor_periodic
            per, masks = _periodic
            st = lib().amg_hip_create_tensor_periodic(n, _p32(colptr), _p32(rowind), _p64(val), _p64(b), dim,
                                                      d3.ctypes.data_as(_i64p), int(per), int(n_levels),
                                                      None if masks is None else _p32(masks), C.byref(o),
                                                      C.byref(h))
        elif _opdep_per is not None:  # tensor_opdep_periodic
            per, (masks, _, min_coarse) = _opdep_per
            st = lib().amg_hip_create_tensor_opdep_periodic(n, _p32(colptr), _p32(rowind), _p64(val), _p64(b), dim,
                                                            d3.ctypes.data_as(_i64p), int(per), int(n_levels),
                                                            None if masks is None else _p32(masks),
                                                            int(min_coarse), C.byref(o), C.byref(h))
        elif _opdep is not None:  # tensor_opdep
            masks, _, min_coarse = _opdep
            st = lib().amg_hip_create_tensor_opdep(n, _p32(colptr), _p32(rowind), _p64(val), _p64(b), dim,
                                                   d3.ctypes.data_as(_i64p), int(n_levels),
                                                   None if masks is None else _p32(masks), int(min_coarse),
                                                   C.byref(o), C.byref(h))
        elif _semi is not None:  # tensor_semi
            masks, theta, min_coarse = _semi
            st = lib().amg_hip_create_tensor_semi(n, _p32(colptr), _p32(rowind), _p64(val), _p64(b), dim,
                                                  d3.ctypes.data_as(_i64p), int(n_levels),
                                                  None if masks is None else _p32(masks), float(theta),
                                                  int(min_coarse), C.byref(o), C.byref(h))
        else:
            st = lib().amg_hip_create_tensor(n, _p32(colptr), _p32(rowind), _p64(val), _p64(b), dim,
                                             d3.ctypes.data_as(_i64p), int(n_levels), C.byref(o), C.byref(h))
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        self._h = h
        self._device = device
        return self

    @classmethod
    def tensor_dev(cls, crow, col, val, b, dims, n_levels, smoother=SM_SPGS, smoother_iters=1, omega=1.0,
                   tolerance=1e-9, compute_error_every_n_iters=10, n_iters=100, device=-1, use_graph=True,
                   stencil_transfers=True, layout=None, host_only=False, keep_structural_zeros=False,
                   no_fusion=False, stream=None, fast_coarse_solve=False, keep_residual=False,
                   exact_coarse_solve=False, exact_gs=False, cheb_degree=2, cheb_lower=0.3, cheb_upper=1.0,
                   window=False, host_galerkin=False, fuse_prolong=False, natural_sides=0, singular=False,
                   cyclic_lines=False, _semi=None, _periodic=None, _opdep=None, _opdep_per=None):
        """Multigrid.tensor for a matrix that sits on the device, with the set-up on the device
        (amg_hip_create_tensor_dev).  A is in CSR: crow (n + 1 int32 row pointers), col (int32,
        ascending inside a row), val (float64), and b (n float64), each a contiguous 1-D torch tensor
        on the GPU (e.g. the crow_indices() / col_indices() / values() of a torch CSR tensor, cast to
        int32) or a numpy array, which is uploaded through torch first.  The arrays are copied.
        Options that need host structures silently take the host constructor: see setup_on_device."""
        if compute_error_every_n_iters > n_iters:
            raise ValueError("`compute_error_every_n_iters` must be leq to `n_iters`, got "
                             f"{compute_error_every_n_iters} and {n_iters}")
        import torch
        want = (("crow", crow, torch.int32, np.int32), ("col", col, torch.int32, np.int32),
                ("val", val, torch.float64, np.float64), ("b", b, torch.float64, np.float64))
        given = []
        for name, a, tdt, ndt in want:
            if isinstance(a, np.ndarray):
                if a.dtype != ndt:
                    raise ValueError(f"{name}: expected dtype {np.dtype(ndt).name}, got {a.dtype}")
            elif isinstance(a, torch.Tensor):
                if a.dtype != tdt:
                    raise ValueError(f"{name}: expected dtype {tdt}, got {a.dtype}")
                if not a.is_contiguous():
                    raise ValueError(f"{name}: expected a contiguous tensor")
            else:
                raise ValueError(f"{name}: expected a torch tensor or a numpy array, got {type(a).__name__}")
            if a.ndim != 1:
                raise ValueError(f"{name}: expected a 1-D array, got {a.ndim} dimensions")
            given.append(a)
        n = given[0].shape[0] - 1
        if n != given[3].shape[0]:
            raise ValueError("`A` and `b` must have the same number of degrees of freedom, "
                             f"got {n} and {given[3].shape[0]}")
        if given[1].shape[0] != given[2].shape[0]:
            raise ValueError(f"`col` and `val` must have the same length, got {given[1].shape[0]} and "
                             f"{given[2].shape[0]}")
        dim, d3 = _dims3(dims)
        o = cls._options(smoother, smoother_iters, omega, device, use_graph, stencil_transfers, layout,
                         host_only, keep_structural_zeros, no_fusion, fuse_prolong, stream, fast_coarse_solve,
                         host_galerkin, keep_residual, exact_coarse_solve, exact_gs, cheb_degree, cheb_lower,
                         cheb_upper)
        o.window = int(window)
        o.natural_sides, o.singular = int(natural_sides), int(singular)
        o.cyclic_lines = int(cyclic_lines)
        if device_count() > 0:
            tdev = torch.device("cuda", device if device >= 0 else torch.cuda.current_device())
            dev = []
            for (name, _, _, _), a in zip(want, given):
                if isinstance(a, np.ndarray):
                    a = torch.from_numpy(np.ascontiguousarray(a)).to(tdev)
                elif a.device != tdev:
                    raise ValueError(f"{name}: expected a tensor on {tdev}, got {a.device}")
                dev.append(a)
            torch.cuda.current_stream(tdev).synchronize()  # the tensors are torch's work; the copy is the solver's
            ptrs = [C.c_void_p(a.data_ptr() or 8) for a in dev]  # an empty tensor has no storage: never read
        else:  # no device: the library words the refusal (after its argument checks); nothing is dereferenced
            dev, ptrs = [], [C.c_void_p(8)] * 4
        self = cls.__new__(cls)
        self.tolerance, self.every, self.n_iters = tolerance, compute_error_every_n_iters, n_iters
        h = C.c_void_p()
        if _periodic is not None:  # tensor_periodic_dev
            per, masks = _periodic
            st = lib().amg_hip_create_tensor_periodic_dev(n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], dim,
                                                          d3.ctypes.data_as(_i64p), int(per), int(n_levels),
                                                          None if masks is None else _p32(masks), C.byref(o),
                                                          C.byref(h))
        elif _opdep_per is not None:  # tensor_opdep_periodic_dev
            per, (masks, _, min_coarse) = _opdep_per
            st = lib().amg_hip_create_tensor_opdep_periodic_dev(n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], dim,
                                                                d3.ctypes.data_as(_i64p), int(per), int(n_levels),
                                                                None if masks is None else _p32(masks),
                                                                int(min_coarse), C.byref(o), C.byref(h))
        elif _opdep is not None:  # tensor_opdep_dev
            masks, _, min_coarse = _opdep
            st = lib().amg_hip_create_tensor_opdep_dev(n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], dim,
                                                       d3.ctypes.data_as(_i64p), int(n_levels),
                                                       None if masks is None else _p32(masks), int(min_coarse),
                                                       C.byref(o), C.byref(h))
        elif _semi is not None:  # tensor_semi_dev
            masks, theta, min_coarse = _semi
            st = lib().amg_hip_create_tensor_semi_dev(n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], dim,
                                                      d3.ctypes.data_as(_i64p), int(n_levels),
                                                      None if masks is None else _p32(masks), float(theta),
                                                      int(min_coarse), C.byref(o), C.byref(h))
        else:
            st = lib().amg_hip_create_tensor_dev(n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], dim,
                                                 d3.ctypes.data_as(_i64p), int(n_levels), C.byref(o), C.byref(h))
        del dev
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        self._h = h
        self._device = device
        return self

    @staticmethod
    def _semi_rule(n_levels, axis_masks, theta, min_coarse):
        if axis_masks is None:
            return (None, theta, min_coarse)
        masks = np.ascontiguousarray([int(m) for m in axis_masks], dtype=np.int32)
        if masks.size != int(n_levels) - 1:
            raise ValueError(f"`axis_masks` must have n_levels - 1 = {int(n_levels) - 1} entries, got {masks.size}")
        return (masks, theta, min_coarse)

    @classmethod
    def tensor_semi(cls, colptr, rowind, val, b, dims, n_levels, axis_masks=None, theta=0.5, min_coarse=32,
                    **opts):
        """AMG::Multigrid on a SEMI-coarsening hierarchy of the grid `dims` (amg_hip_create_tensor_semi):
        level l coarsens the axes of its mask (bit 0 = x, 1 = y, 2 = z) and leaves the others alone.
        axis_masks: n_levels - 1 explicit masks, or None for the automatic rule -- coarsen the axes
        whose strongest coupling is at least theta times the strongest of all, until n_levels, a level
        of at most min_coarse rows, or no axis of 2 points (n_levels tells).  For operators that are
        anisotropic along a grid axis; options as for Multigrid.tensor."""
        return cls.tensor(colptr, rowind, val, b, dims, n_levels,
                          _semi=cls._semi_rule(n_levels, axis_masks, theta, min_coarse), **opts)

    @classmethod
    def tensor_opdep(cls, colptr, rowind, val, b, dims, n_levels, axis_masks=None, min_coarse=32, **opts):
        """AMG::Multigrid on a hierarchy with OPERATOR-DEPENDENT interpolation (amg_hip_create_tensor_opdep):
        every level coarsens exactly one axis of the grid `dims`, and the 1-D interpolation weights along
        it come from the rows of the level's matrix, collapsed onto that axis.  axis_masks: n_levels - 1
        masks of one bit each (1 = x, 2 = y, 4 = z), or None for the automatic rule -- coarsen the axis
        with the strongest coupling (the lowest on a tie) until n_levels, a level of at most min_coarse
        rows, or no axis of 2 points (n_levels tells).  For coefficients that jump from cell to cell;
        options as for Multigrid.tensor."""
        return cls.tensor(colptr, rowind, val, b, dims, n_levels,
                          _opdep=cls._semi_rule(n_levels, axis_masks, 1.0, min_coarse), **opts)

    @classmethod
    def tensor_opdep_periodic(cls, colptr, rowind, val, b, dims, n_levels, periodic_axes, axis_masks=None,
                              min_coarse=32, **opts):
        """Multigrid.tensor_opdep for an operator with PERIODIC axes (amg_hip_create_tensor_opdep_periodic).
        periodic_axes: bit a = axis a wraps around (1 = x, 2 = y, 4 = z); A holds the wrap entries.  A
        coarsened periodic axis needs an even length of at least 4 on its level; every even point of it
        has both weights, fine point 0 taking its low one from coarse point m/2 - 1.  The automatic rule
        (axis_masks=None) leaves out a periodic axis that is odd or shorter than 4.  natural_sides names
        sides of the other axes only; singular=True needs all of those (none when every axis is
        periodic).  periodic_axes=0: Multigrid.tensor_opdep's solver.  Options as for Multigrid.tensor."""
        return cls.tensor(colptr, rowind, val, b, dims, n_levels,
                          _opdep_per=(int(periodic_axes), cls._semi_rule(n_levels, axis_masks, 1.0, min_coarse)),
                          **opts)

    @classmethod
    def tensor_opdep_periodic_dev(cls, crow, col, val, b, dims, n_levels, periodic_axes, axis_masks=None,
                                  min_coarse=32, **opts):
        """Multigrid.tensor_opdep_periodic for a CSR matrix that sits on the device
        (amg_hip_create_tensor_opdep_periodic_dev); arguments as for Multigrid.tensor_dev.  The arrays are
        checked on the device.  After set_periodic_device_setup(1) the hierarchy is built there too
        (K-AxisWeights / K-AxisGalerkin with the seam; smoothers, layouts and silent fallbacks of
        Multigrid.tensor_opdep_dev) and setup_on_device reports 1 unless it fell back; by default the
        host constructor builds it and setup_on_device reports 0.  The same solver bit for bit either way."""
        return cls.tensor_dev(crow, col, val, b, dims, n_levels,
                              _opdep_per=(int(periodic_axes), cls._semi_rule(n_levels, axis_masks, 1.0, min_coarse)),
                              **opts)

    def axis_weights(self, level):
        """The compact weights of `level` of a tensor_opdep solver (amg_hip_get_axis_weights): an array of
        shape (n_l - n_{l+1}, 2), row e = (w_lo, w_hi) of the e-th fine point (x fastest) whose coordinate
        on the level's axis is even."""
        ok = 0 <= int(level) < self.n_levels - 1  # else the library words the refusal
        n_h, n_H = (self.get_n_dofs(level), self.get_n_dofs(level + 1)) if ok else (0, 0)
        W = np.zeros((max(n_h - n_H, 0), 2), np.float64)
        st = lib().amg_hip_get_axis_weights(self._h, int(level), _p64(W))
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        return W

    @classmethod
    def tensor_semi_dev(cls, crow, col, val, b, dims, n_levels, axis_masks=None, theta=0.5, min_coarse=32,
                        **opts):
        """Multigrid.tensor_semi for a CSR matrix that sits on the device, with the set-up on the device
        (amg_hip_create_tensor_semi_dev); arguments as for Multigrid.tensor_dev."""
        return cls.tensor_dev(crow, col, val, b, dims, n_levels,
                              _semi=cls._semi_rule(n_levels, axis_masks, theta, min_coarse), **opts)

    @classmethod
    def tensor_opdep_dev(cls, crow, col, val, b, dims, n_levels, axis_masks=None, min_coarse=32, **opts):
        """Multigrid.tensor_opdep for a CSR matrix that sits on the device, with the set-up on the device
        (amg_hip_create_tensor_opdep_dev: K-AxisWeights and K-AxisGalerkin per level); arguments as for
        Multigrid.tensor_dev.  The same solver bit for bit as Multigrid.tensor_opdep on the CSC arrays;
        the silent fall-backs of Multigrid.tensor_dev apply, and set_axis_stencil(0) is one more."""
        return cls.tensor_dev(crow, col, val, b, dims, n_levels,
                              _opdep=cls._semi_rule(n_levels, axis_masks, 1.0, min_coarse), **opts)

    @classmethod
    def tensor_periodic(cls, colptr, rowind, val, b, dims, n_levels, periodic_axes, axis_masks=None, **opts):
        """Multigrid.tensor / tensor_semi for an operator with PERIODIC axes (amg_hip_create_tensor_periodic).
        periodic_axes: bit a = axis a wraps around (1 = x, 2 = y, 4 = z); a coarsened periodic axis needs
        an even length of at least 4 on its level and interpolates fine point 0 between coarse points 0
        and m/2 - 1.  axis_masks=None: full coarsening with exactly n_levels levels, else n_levels - 1
        explicit masks (there is no automatic rule).  natural_sides names sides of the other axes only;
        singular=True needs all of those (none when every axis is periodic).  cyclic_lines=True
        (smoother SM_LINE_ALT only): the line directions along a periodic axis of 3 points or more are
        solved as cyclic tridiagonal systems, wrap entries included (line_cyclic tells which).  Options as
        for Multigrid.tensor."""
        masks = cls._semi_rule(n_levels, axis_masks, 0.5, 1)[0]
        return cls.tensor(colptr, rowind, val, b, dims, n_levels, _periodic=(int(periodic_axes), masks), **opts)

    @classmethod
    def tensor_periodic_dev(cls, crow, col, val, b, dims, n_levels, periodic_axes, axis_masks=None, **opts):
        """Multigrid.tensor_periodic for a CSR matrix that sits on the device
        (amg_hip_create_tensor_periodic_dev); arguments as for Multigrid.tensor_dev.  After
        set_periodic_device_setup(1) the hierarchy is built on the device (K-TensorGalerkin with the
        seam; the silent fall-backs of Multigrid.tensor_dev apply) and setup_on_device() reports 1.
        By default it is built by the host constructor and setup_on_device() reports 0.  The same
        solver bit for bit either way."""
        masks = cls._semi_rule(n_levels, axis_masks, 0.5, 1)[0]
        return cls.tensor_dev(crow, col, val, b, dims, n_levels, _periodic=(int(periodic_axes), masks), **opts)

    @classmethod
    def poisson_tensor(cls, n, n_levels, dim=2, device_setup=False, **opts):
        """Multigrid.tensor on A = Grid::laplacian(n), b = Grid::rhs(n) (the n^dim grid).
        device_setup=True: amg_hip_create_poisson_tensor, the same solver with the generator, the
        Galerkin chain (K-TensorGalerkin) and the encoder on the device (options that need host
        structures silently take the host constructor: see setup_on_device)."""
        if not device_setup:
            cp, ri, v = laplacian(n, dim)
            return cls.tensor(cp, ri, v, rhs(n, dim), (n,) * dim, n_levels, **opts)
        return cls._poisson_tensor_device(n, n_levels, dim, **opts)

    @classmethod
    def _poisson_tensor_device(cls, n, n_levels, dim, smoother=SM_SPGS, smoother_iters=1, omega=1.0,
                               tolerance=1e-9, compute_error_every_n_iters=10, n_iters=100, device=-1,
                               use_graph=True, stencil_transfers=True, layout=None, host_only=False,
                               keep_structural_zeros=False, no_fusion=False, stream=None,
                               fast_coarse_solve=False, keep_residual=False, exact_coarse_solve=False,
                               exact_gs=False, cheb_degree=2, cheb_lower=0.3, cheb_upper=1.0, window=False,
                               host_galerkin=False, fuse_prolong=False):
        if compute_error_every_n_iters > n_iters:
            raise ValueError("`compute_error_every_n_iters` must be leq to `n_iters`, got "
                             f"{compute_error_every_n_iters} and {n_iters}")
        self = cls.__new__(cls)
        self.tolerance, self.every, self.n_iters = tolerance, compute_error_every_n_iters, n_iters
        o = cls._options(smoother, smoother_iters, omega, device, use_graph, stencil_transfers, layout,
                         host_only, keep_structural_zeros, no_fusion, fuse_prolong, stream, fast_coarse_solve,
                         host_galerkin, keep_residual, exact_coarse_solve, exact_gs, cheb_degree, cheb_lower,
                         cheb_upper)
        o.window = int(window)
        h = C.c_void_p()
        st = lib().amg_hip_create_poisson_tensor(int(dim), int(n), int(n_levels), C.byref(o), C.byref(h))
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        self._h = h
        self._device = device
        return self

    @property
    def setup_on_device(self):
        """1: the hierarchy was built by a device-only path (Multigrid.poisson, poisson_tensor with
        device_setup=True), 0: by the host constructor, the silent fallbacks included."""
        on = C.c_int32(-1)
        _chk(lib().amg_hip_setup_on_device(self._h, C.byref(on)))
        return on.value

    def level_dims(self, level):
        """(nx, ny, nz) of `level` of a Multigrid.tensor solver (amg_hip_get_level_dims)."""
        d = np.zeros(3, np.int64)
        st = lib().amg_hip_get_level_dims(self._h, int(level), d.ctypes.data_as(_i64p))
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        return tuple(int(x) for x in d)

    def periodic_axes(self):
        """The solver's mask of periodic axes (amg_hip_get_periodic_axes); 0 on solvers that were not
        made by tensor_periodic / tensor_periodic_dev."""
        m = C.c_int32(0)
        _chk(lib().amg_hip_get_periodic_axes(self._h, C.byref(m)))
        return int(m.value)

    def natural_sides(self):
        """The solver's mask of natural boundary sides (amg_hip_get_natural_sides); 0 on solvers that
        are not tensor hierarchies."""
        m = C.c_int32(-1)
        _chk(lib().amg_hip_get_natural_sides(self._h, C.byref(m)))
        return m.value

    def level_axes(self, level):
        """Axis mask (bit 0 = x, 1 = y, 2 = z) of the transfers between `level` and `level` + 1 of a
        tensor solver (amg_hip_get_level_axes)."""
        m = C.c_int32(-1)
        st = lib().amg_hip_get_level_axes(self._h, int(level), C.byref(m))
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        return m.value

    def level_transfer_kind(self, level):
        """0 = CSR SpMV transfers, 1 = the flat stride-2 kernels, 2 = the tensor-product kernels,
        3 = the single-axis kernels with per-point weights of tensor_opdep."""
        k = C.c_int32(-1)
        st = lib().amg_hip_level_transfer_kind(self._h, int(level), C.byref(k))
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        return k.value

    @classmethod
    def poisson(cls, n, n_levels, dim=2, smoother=SM_SPGS, smoother_iters=1, omega=1.0, tolerance=1e-9,
                compute_error_every_n_iters=10, n_iters=100, device=-1, use_graph=True,
                stencil_transfers=True, layout=None, keep_structural_zeros=False, no_fusion=False,
                stream=None, fast_coarse_solve=False, keep_residual=False, exact_coarse_solve=False,
                exact_gs=False, cheb_degree=2, cheb_lower=0.3, cheb_upper=1.0):
        """AMG::Multigrid on A = Grid::laplacian(n), b = Grid::rhs(n) with the setup on the device
        end to end (amg_hip_create_poisson): no host matrices."""
        if compute_error_every_n_iters > n_iters:
            raise ValueError("`compute_error_every_n_iters` must be leq to `n_iters`, got "
                             f"{compute_error_every_n_iters} and {n_iters}")
        self = cls.__new__(cls)
        self.tolerance, self.every, self.n_iters = tolerance, compute_error_every_n_iters, n_iters
        o = cls._options(smoother, smoother_iters, omega, device, use_graph, stencil_transfers, layout,
                         False, keep_structural_zeros, no_fusion, False, stream, fast_coarse_solve,
                         False, keep_residual, exact_coarse_solve, exact_gs, cheb_degree, cheb_lower,
                         cheb_upper)
        h = C.c_void_p()
        st = lib().amg_hip_create_poisson(dim, n, n_levels, C.byref(o), C.byref(h))
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        self._h = h
        self._device = device
        return self

    @classmethod
    def poisson_window(cls, n, unit_begin, unit_end, n_levels, dim=2, smoother=SM_JACOBI, smoother_iters=2,
                       omega=0.6, device=-1, use_graph=True, layout=None, no_fusion=False, stream=None,
                       host_only=False):
        """One rank's WINDOW of a sharded Grid::laplacian(n) hierarchy (amg_hip_create_poisson_window):
        units [unit_begin, unit_end) of the slowest axis, n_levels - 1 distributed levels; runs by
        parts (window_run)."""
        self = cls.__new__(cls)
        self.tolerance, self.every, self.n_iters = 1e-9, 10, 100
        o = cls._options(smoother, smoother_iters, omega, device, use_graph, True, layout, host_only, False,
                         no_fusion, False, stream, False, False, False, False, False)
        o.window = 1
        h = C.c_void_p()
        st = lib().amg_hip_create_poisson_window(dim, n, int(unit_begin), int(unit_end), n_levels,
                                                 C.byref(o), C.byref(h))
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        self._h = h
        self._device = device
        return self

    def window_setup(self, down_lo=None, down_hi=None, up_lo=None, up_hi=None):
        if down_lo is None:
            _chk(lib().amg_hip_window_setup(self._h, None, None, None, None))
            return
        arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (down_lo, down_hi, up_lo, up_hi)]
        _chk(lib().amg_hip_window_setup(self._h, *[a.ctypes.data_as(_i64p) for a in arrs]))

    def window_run(self, part):
        _chk(lib().amg_hip_window_run(self._h, int(part)))

    def vec_dev_ptr(self, level, which):
        """(device pointer, n) of a level vector; which: "u", "f" or "r"."""
        p, n = C.c_void_p(), C.c_int64(0)
        _chk(lib().amg_hip_vec_dev_ptr(self._h, level, {"u": 0, "f": 1, "r": 2}[which], C.byref(p), C.byref(n)))
        return int(p.value), int(n.value)

    def close(self):
        if getattr(self, "_h", None):
            lib().amg_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @property
    def n_levels(self):
        return lib().amg_hip_n_levels(self._h)

    def get_n_dofs(self, level):
        return int(lib().amg_hip_get_n_dofs(self._h, level))

    def get_coefficient_matrix(self, level):
        n = self.get_n_dofs(level)
        nnz = lib().amg_hip_get_level_nnz(self._h, level)
        colptr = np.empty(n + 1, np.int32)
        rowind = np.empty(nnz, np.int32)
        val = np.empty(nnz, np.float64)
        _chk(lib().amg_hip_get_level_matrix(self._h, level, _p32(colptr), _p32(rowind), _p64(val)))
        return colptr, rowind, val

    def get_transfer(self, level, which):
        w = 1 if which == "R" else 0
        nnz = lib().amg_hip_get_transfer_nnz(self._h, level, w)
        if nnz < 0:
            raise ValueError("level out of range")
        n_h, n_H = self.get_n_dofs(level), self.get_n_dofs(level + 1)
        cols = n_h if w else n_H
        colptr = np.empty(cols + 1, np.int32)
        rowind = np.empty(nnz, np.int32)
        val = np.empty(nnz, np.float64)
        _chk(lib().amg_hip_get_transfer(self._h, level, w, _p32(colptr), _p32(rowind), _p64(val)))
        return colptr, rowind, val

    def _get(self, level, which):
        out = np.empty(self.get_n_dofs(level), np.float64)
        _chk(lib().amg_hip_get_vec(self._h, level, which, _p64(out)))
        return out

    def get_soln(self, level=0):
        return self._get(level, 0)

    def get_rhs(self, level=0):
        return self._get(level, 1)

    def get_residual(self, level=0):
        return self._get(level, 2)

    def set_vec(self, level, which, v):
        v = _a64(v)
        assert v.size == self.get_n_dofs(level)
        _chk(lib().amg_hip_set_vec(self._h, level, {"u": 0, "f": 1, "r": 2}[which], _p64(v)))

    def copy_vec_dev(self, level, which, dev_ptr, to_solver):
        _chk(lib().amg_hip_copy_vec_dev(self._h, level, {"u": 0, "f": 1, "r": 2}[which],
                                        C.c_void_p(dev_ptr), int(to_solver)))

    def zero_vec(self, level, which):
        _chk(lib().amg_hip_zero_vec(self._h, level, {"u": 0, "f": 1, "r": 2}[which]))

    def get_tolerance(self):
        return self.tolerance

    def level_layout(self, level):
        """(layout, matrix stream bytes per sweep) of the level's device operator."""
        lay, nb = C.c_int32(0), C.c_int64(0)
        _chk(lib().amg_hip_level_layout(self._h, level, C.byref(lay), C.byref(nb)))
        return int(lay.value), int(nb.value)

    def coarse_halfbw(self):
        return int(lib().amg_hip_coarse_halfbw(self._h))

    def get_colors(self, level):
        color = np.empty(self.get_n_dofs(level), np.int32)
        nc = C.c_int32(0)
        _chk(lib().amg_hip_get_colors(self._h, level, _p32(color), C.byref(nc)))
        return color, nc.value

    def cycle_bytes(self):
        a, b = C.c_double(0), C.c_double(0)
        _chk(lib().amg_hip_cycle_bytes(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def cycle_must_move(self, part=0):
        """bytes the launches of one V-cycle (or of one part of a sharded one) have to move; part 4: of one
        steady-state cycle of vcycle(n >= 2), which the K-Patch seam makes 25 n_0 bytes lighter"""
        b = C.c_double(0)
        _chk(lib().amg_hip_cycle_must_move(self._h, int(part), C.byref(b)))
        return b.value

    def pair_duo_partner(self, level):
        """the other level of `level`'s K-Duo pair, or -1"""
        return int(lib().amg_hip_pair_duo_partner(self._h, int(level)))

    def patch_leg_lines(self, level, leg):
        """lines of the K-Patch tiles of `level`'s down-leg (leg 0) / up-leg (leg 1); 0 = no K-Patch level.
        leg 2: of the seam launch that vcycle(n >= 2) runs on level 0; 0 = this solver runs none"""
        return int(lib().amg_hip_patch_leg_lines(self._h, int(level), int(leg)))

    def leg_form(self, level):
        """(down, up): the launch forms the cycle plan gives `level`, as names of LEG_FORMS
        (amg_hip_level_leg_form); ValueError for a level the solver does not have"""
        d, u = C.c_int32(0), C.c_int32(0)
        st = lib().amg_hip_level_leg_form(self._h, int(level), C.byref(d), C.byref(u))
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        return LEG_FORMS[d.value], LEG_FORMS[u.value]

    def strip_geometry(self, level):
        """StripGeometry(T, tiles, stages, halo_down, halo_up) of a K-Strip level
        (amg_hip_strip_geometry); ValueError where the level runs in another form"""
        v = [C.c_int32(0) for _ in range(5)]
        st = lib().amg_hip_strip_geometry(self._h, int(level), *[C.byref(x) for x in v])
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        return StripGeometry(*[int(x.value) for x in v])

    def patch_tile_classes(self, level, rings):
        """(one-type, column-typed, general) tile counts of `level` for the launches with `rings` halo rings
        (2: 44-line tiles, 3: 42, 5: the seam's); ValueError where the level is no K-Patch level"""
        out = np.zeros(3, np.int64)
        st = lib().amg_hip_patch_tile_classes(self._h, int(level), int(rings), out.ctypes.data_as(_i64p))
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        return tuple(int(v) for v in out)

    def profile_fine_sweep(self, n_launches):
        """(avg_ms, min_ms, sweeps per launch, kernel name) of the level-0 Jacobi sweep
        kernel, HIP events on the solver's stream."""
        a, b = C.c_double(0), C.c_double(0)
        _chk(lib().amg_hip_profile_fine_sweep(self._h, n_launches, C.byref(a), C.byref(b)))
        name = C.create_string_buffer(256)
        k, nb = C.c_int32(0), C.c_double(0)
        _chk(lib().amg_hip_fine_sweep_info(self._h, name, 256, C.byref(k), C.byref(nb)))
        return a.value, b.value, k.value, name.value.decode(), nb.value

    def fine_sweep_info(self):
        """(kernel name, sweeps per launch, bytes one launch has to move) of the level-0 smoother
        launch (amg_hip_fine_sweep_info); no launch is made."""
        name = C.create_string_buffer(256)
        k, nb = C.c_int32(0), C.c_double(0)
        _chk(lib().amg_hip_fine_sweep_info(self._h, name, 256, C.byref(k), C.byref(nb)))
        return name.value.decode(), k.value, nb.value

    def cheb_bounds(self, level):
        """(lo, hi): the interval the Chebyshev smoother uses on `level` (amg_hip_cheb_bounds)."""
        lo, hi = C.c_double(0), C.c_double(0)
        st = lib().amg_hip_cheb_bounds(self._h, int(level), C.byref(lo), C.byref(hi))
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        return lo.value, hi.value

    def line_stride(self, level):
        """The stride s of the line smoother's lines on `level` (amg_hip_line_stride)."""
        s = C.c_int64(0)
        st = lib().amg_hip_line_stride(self._h, int(level), C.byref(s))
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        return s.value

    def line_directions(self, level):
        """The strides of the alternating line smoother's directions on `level`, ascending
        (amg_hip_line_directions): a list of 0 to 3 integers."""
        nd = C.c_int32(0)
        st3 = (C.c_int64 * 3)()
        st = lib().amg_hip_line_directions(self._h, int(level), C.byref(nd), st3)
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        return [int(st3[d]) for d in range(nd.value)]

    def line_cyclic(self, level):
        """The mask of the axes of `level` whose lines the alternating line smoother solves cyclically
        (amg_hip_line_cyclic; bit a = axis a); 0 without cyclic_lines."""
        m = C.c_int32(0)
        st = lib().amg_hip_line_cyclic(self._h, int(level), C.byref(m))
        if st == EINVAL:
            raise ValueError(lib().amg_hip_last_error().decode())
        _chk(st)
        return m.value

    def coarse_solve_kind(self):
        return {0: "band (one wave, sequential, bit-exact)", 1: "spike (partitioned, parallel)",
                2: "band-wide (blocked sequential, any half-bandwidth, bit-exact)",
                3: "band-chain (LDS-resident scalar recurrence, half-bandwidth <= 3, bit-exact)"}[
                    int(lib().amg_hip_coarse_solve_kind(self._h))]

    def level_op(self, level, op):
        """op: 0 smooth (built-in), 1 residual, 2 zero+restrict, 3 prolong+add, 4 coarse solve."""
        _chk(lib().amg_hip_level_op(self._h, level, op))

    def vcycle(self, n=1):
        _chk(lib().amg_hip_vcycles(self._h, n))

    def sync(self):
        _chk(lib().amg_hip_sync(self._h))

    def rss(self):
        out = C.c_double(0)
        _chk(lib().amg_hip_rss(self._h, C.byref(out)))
        return out.value

    def slab_setup(self, rank, world, max_levels=-1):
        """Row-block sharding of the K-Patch levels over `world` ranks (amg_hip_slab_setup)."""
        info = SlabInfo()
        _chk(lib().amg_hip_slab_setup(self._h, int(rank), int(world), int(max_levels), C.byref(info)))
        return info

    def slab_run(self, part):
        """1: down-legs of the slab levels, 2: replicated rest, 3: up-legs (amg_hip_slab_run)."""
        _chk(lib().amg_hip_slab_run(self._h, int(part)))

    def apply_dev(self, v_dev, z_dev):
        """z = M^-1 v (one V-cycle from zero); device pointers."""
        _chk(lib().amg_hip_apply(self._h, C.c_void_p(v_dev), C.c_void_p(z_dev)))

    def pcg(self, rtol=1e-10, max_iters=100):
        """CG on A_0 x = b preconditioned with one V-cycle; returns (x, iters, relres)."""
        it, rel = C.c_int64(0), C.c_double(0)
        _chk(lib().amg_hip_pcg(self._h, rtol, max_iters, C.byref(it), C.byref(rel)))
        return self.get_soln(0), it.value, rel.value

    def set_mean_projection(self, on):
        """singular solvers: pcg(), pcg_mixed() and block_pcg() project b, every preconditioned residual
        and the result onto the complement of the constants (amg_hip_set_mean_projection)"""
        _chk(lib().amg_hip_set_mean_projection(self._h, int(on)))

    @property
    def mean_projection(self):
        on = C.c_int32(0)
        _chk(lib().amg_hip_get_mean_projection(self._h, C.byref(on)))
        return on.value

    def center_vec(self, level, which):
        """v = v - sum(v) / n on a level vector, which = "u" / 0 or "f" / 1 (amg_hip_center_vec)"""
        _chk(lib().amg_hip_center_vec(self._h, int(level), {"u": 0, "f": 1}.get(which, which)))

    def apply_f32(self, v_dev, z_dev):
        """z = M32^-1 v: apply_dev with the whole cycle in single precision (amg_hip_apply_f32);
        device pointers to float64 vectors.  The solver's own vectors are not touched."""
        _chk(lib().amg_hip_apply_f32(self._h, C.c_void_p(v_dev), C.c_void_p(z_dev)))

    def pcg_mixed(self, rtol=1e-10, max_iters=100):
        """pcg() with the single-precision cycle as M^-1, everything else in float64
        (amg_hip_pcg_mixed); returns (x, iters, relres)."""
        it, rel = C.c_int64(0), C.c_double(0)
        _chk(lib().amg_hip_pcg_mixed(self._h, rtol, max_iters, C.byref(it), C.byref(rel)))
        return self.get_soln(0), it.value, rel.value

    def f32_must_move(self):
        """bytes one apply_f32 has to move (amg_hip_f32_must_move)"""
        b = C.c_double(0)
        _chk(lib().amg_hip_f32_must_move(self._h, C.byref(b)))
        return b.value

    # ---- test hooks on the float cycle (amg_hip_f32_get_vec / _set_vec / _level_op) ----------
    def f32_get_vec(self, level, which):
        """float32 copy of the float cycle's vector `which` ("u", "f" or "r") of `level`."""
        out = np.empty(self.get_n_dofs(level), np.float32)
        _chk(lib().amg_hip_f32_get_vec(self._h, int(level), {"u": 0, "f": 1, "r": 2}[which],
                                       out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def f32_set_vec(self, level, which, v):
        """Set the float cycle's vector `which` of `level`; v must be float32 already (no rounding here)."""
        v = np.asarray(v)
        if v.dtype != np.float32 or v.shape != (self.get_n_dofs(level),):
            raise ValueError("f32_set_vec: expected a float32 vector of n_dofs(level) entries")
        v = np.ascontiguousarray(v)
        _chk(lib().amg_hip_f32_set_vec(self._h, int(level), {"u": 0, "f": 1, "r": 2}[which],
                                       v.ctypes.data_as(C.POINTER(C.c_float))))

    def f32_level_op(self, level, op):
        """One step of the float cycle on the float vectors; op as level_op's."""
        _chk(lib().amg_hip_f32_level_op(self._h, int(level), int(op)))

    def f32_line_subsweep(self, level, d=0, reverse=False):
        """One float sub-sweep of direction index d of a line smoother on the float vectors of `level`
        (amg_hip_f32_line_subsweep; needs set_f32_lines(1))."""
        _chk(lib().amg_hip_f32_line_subsweep(self._h, int(level), int(d), int(bool(reverse))))

    def f32_line_factors(self, level):
        """(dl, ip, cp): the float K-LineX factors of `level` (amg_hip_f32_line_factors)."""
        out = [np.empty(self.get_n_dofs(level), np.float32) for _ in range(3)]
        _chk(lib().amg_hip_f32_line_factors(self._h, int(level),
                                            *(a.ctypes.data_as(C.POINTER(C.c_float)) for a in out)))
        return tuple(out)

    # ---- block (multi-right-hand-side) cycles: amg_hip_block_* ---------------------------
    def _block_check(self, name, t, k=None):
        """ValueError unless t is a contiguous float64 tensor of shape (n_0, k), 1 <= k <= 16;
        returns k.  No block call reaches C when a check fails."""
        import torch
        n0 = self.get_n_dofs(0)
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: expected a torch tensor, got {type(t).__name__}")
        if t.dim() != 2 or t.shape[0] != n0 or not 1 <= t.shape[1] <= 16 or (k is not None and t.shape[1] != k):
            want = f"({n0}, {k})" if k is not None else f"({n0}, k) with 1 <= k <= 16"
            raise ValueError(f"{name}: expected shape {want}, got {tuple(t.shape)}")
        if t.dtype != torch.float64:
            raise ValueError(f"{name}: expected dtype torch.float64, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous (row-major) tensor")
        return int(t.shape[1])

    def _block_device(self, **tensors):
        dev = getattr(self, "_device", -1)
        for name, t in tensors.items():
            if not t.is_cuda or (dev is not None and dev >= 0 and t.device.index != dev):
                raise ValueError(f"{name}: expected a tensor on the solver's device, got {t.device}")

    def _block_call(self, device, fn):
        """fn() on the solver's stream, ordered after torch's current stream, and torch's current
        stream ordered after it (the tensors are torch's, the work is the solver's)."""
        import torch
        sp = C.c_void_p()
        _chk(lib().amg_hip_get_stream(self._h, C.byref(sp)))
        cur = torch.cuda.current_stream(device)
        ext = torch.cuda.ExternalStream(sp.value or 0, device=device)
        ext.wait_stream(cur)
        try:
            return fn()
        finally:
            cur.wait_stream(ext)

    def block_vcycles(self, U, F, n=1):
        """n V-cycles on every column of U (n_0 x k, in place) with right-hand sides F: column j
        ends with the bits of vcycle(n) on column j (amg_hip_block_vcycles).  Returns U."""
        k = self._block_check("U", U)
        self._block_check("F", F, k)
        self._block_device(U=U, F=F)
        self._block_call(U.device, lambda: _chk(lib().amg_hip_block_vcycles(
            self._h, k, C.c_void_p(F.data_ptr()), C.c_void_p(U.data_ptr()), int(n))))
        return U

    def block_rss(self, U, F):
        """rss() of every column (amg_hip_block_rss): a numpy array of k values."""
        k = self._block_check("U", U)
        self._block_check("F", F, k)
        self._block_device(U=U, F=F)
        out = np.zeros(k, np.float64)
        self._block_call(U.device, lambda: _chk(lib().amg_hip_block_rss(
            self._h, k, C.c_void_p(F.data_ptr()), C.c_void_p(U.data_ptr()), _p64(out))))
        return out

    def block_pcg(self, B, X=None, rtol=1e-10, max_iters=100):
        """pcg() on every column of B from X (zero when None), sharing the SpMVs and V-cycles
        (amg_hip_block_pcg).  Returns (X, iters, relres); X is updated in place when given."""
        import torch
        k = self._block_check("B", B)
        if X is None:
            X = torch.zeros_like(B)
        self._block_check("X", X, k)
        self._block_device(B=B, X=X)
        it = np.zeros(k, np.int64)
        rel = np.zeros(k, np.float64)
        self._block_call(B.device, lambda: _chk(lib().amg_hip_block_pcg(
            self._h, k, C.c_void_p(B.data_ptr()), C.c_void_p(X.data_ptr()), float(rtol), int(max_iters),
            it.ctypes.data_as(_i64p), _p64(rel))))
        return X, it, rel

    def block_must_move(self, k):
        """bytes one block cycle on k columns has to move (amg_hip_block_must_move)"""
        b = C.c_double(0)
        _chk(lib().amg_hip_block_must_move(self._h, int(k), C.byref(b)))
        return b.value

    def solve(self):
        """multigrid.hpp:311-337.  Returns (u, iters, converged, last_rss) and
        prints the reference's convergence line."""
        it, last, conv = C.c_int64(0), C.c_double(0), C.c_int32(0)
        _chk(lib().amg_hip_solve(self._h, self.tolerance, self.every, self.n_iters,
                                 C.byref(it), C.byref(last), C.byref(conv)))
        if conv.value:
            print(f"AMG converged after {it.value} iterations.")
        else:
            print(f"AMG did not converge after {it.value} iterations.")
        return self.get_soln(0), it.value, bool(conv.value), last.value


# ---- stand-alone plug-in operations ---------------------------------------------
def smooth(kind, colptr, rowind, val, u, b, n_iters=1, omega=1.0, tol=1e-9, every=0):
    colptr, rowind, val, b = _a32(colptr), _a32(rowind), _a64(val), _a64(b)
    u = np.array(u, dtype=np.float64, copy=True)
    it, conv = C.c_int64(0), C.c_int32(0)
    st = lib().amg_hip_smooth(kind, colptr.size - 1, _p32(colptr), _p32(rowind), _p64(val),
                              _p64(u), _p64(b), omega, tol, every, n_iters, C.byref(it),
                              C.byref(conv))
    if st == EINVAL:
        raise ValueError(lib().amg_hip_last_error().decode())
    _chk(st)
    return u, it.value, bool(conv.value)


def smooth_chebyshev(colptr, rowind, val, u, b, degree=2, lower=0.3, upper=1.0, n_iters=1):
    """amg_hip_smooth_chebyshev: n_iters applications of the Chebyshev polynomial; returns the new u."""
    colptr, rowind, val, b = _a32(colptr), _a32(rowind), _a64(val), _a64(b)
    u = np.array(u, dtype=np.float64, copy=True)
    st = lib().amg_hip_smooth_chebyshev(colptr.size - 1, _p32(colptr), _p32(rowind), _p64(val), _p64(u),
                                        _p64(b), int(degree), float(lower), float(upper), int(n_iters))
    if st == EINVAL:
        raise ValueError(lib().amg_hip_last_error().decode())
    _chk(st)
    return u


def smooth_line(colptr, rowind, val, u, f, stride=0, omega=0.7, iters=1):
    """amg_hip_smooth_line: `iters` sweeps u <- u + omega T^-1 (f - A u) of the line smoother with the
    lines at distance `stride` (0: the automatic rule); returns the new u."""
    colptr, rowind, val, f = _a32(colptr), _a32(rowind), _a64(val), _a64(f)
    u = np.array(u, dtype=np.float64, copy=True)
    st = lib().amg_hip_smooth_line(colptr.size - 1, _p32(colptr), _p32(rowind), _p64(val), int(stride),
                                   float(omega), int(iters), _p64(u), _p64(f))
    if st == EINVAL:
        raise ValueError(lib().amg_hip_last_error().decode())
    _chk(st)
    return u


def smooth_line_alt(colptr, rowind, val, u, f, dims, omega=0.8, iters=1, reverse=False, periodic_axes=None):
    """amg_hip_smooth_line_alt: `iters` applications of the alternating line smoother on the grid
    `dims` (2 or 3 entries, x fastest), directions ascending (descending with `reverse`); returns the
    new u.  periodic_axes (a mask, bit a = axis a): amg_hip_smooth_line_alt_per, cyclic lines along
    those axes where they have 3 points or more."""
    colptr, rowind, val, f = _a32(colptr), _a32(rowind), _a64(val), _a64(f)
    u = np.array(u, dtype=np.float64, copy=True)
    dims = [int(d) for d in dims]
    d3 = (C.c_int64 * 3)(*(dims + [1] * (3 - len(dims)))[:3]) if 1 <= len(dims) <= 3 else (C.c_int64 * 3)(0, 0, 0)
    if periodic_axes is None:
        st = lib().amg_hip_smooth_line_alt(colptr.size - 1, _p32(colptr), _p32(rowind), _p64(val), len(dims), d3,
                                           float(omega), int(iters), 1 if reverse else 0, _p64(u), _p64(f))
    else:
        st = lib().amg_hip_smooth_line_alt_per(colptr.size - 1, _p32(colptr), _p32(rowind), _p64(val), len(dims),
                                               d3, int(periodic_axes), float(omega), int(iters),
                                               1 if reverse else 0, _p64(u), _p64(f))
    if st == EINVAL:
        raise ValueError(lib().amg_hip_last_error().decode())
    _chk(st)
    return u


def spgs_sweep(direction, colptr, rowind, val, u, b):
    colptr, rowind, val, b = _a32(colptr), _a32(rowind), _a64(val), _a64(b)
    u = np.array(u, dtype=np.float64, copy=True)
    _chk(lib().amg_hip_spgs_sweep(direction, colptr.size - 1, _p32(colptr), _p32(rowind),
                                  _p64(val), _p64(u), _p64(b)))
    return u


def residual(colptr, rowind, val, u, f):
    colptr, rowind, val, u, f = _a32(colptr), _a32(rowind), _a64(val), _a64(u), _a64(f)
    r = np.empty(colptr.size - 1, np.float64)
    _chk(lib().amg_hip_residual(colptr.size - 1, _p32(colptr), _p32(rowind), _p64(val),
                                _p64(u), _p64(f), _p64(r)))
    return r


def spmv(rows, cols, colptr, rowind, val, v):
    colptr, rowind, val, v = _a32(colptr), _a32(rowind), _a64(val), _a64(v)
    out = np.empty(rows, np.float64)
    _chk(lib().amg_hip_spmv(rows, cols, _p32(colptr), _p32(rowind), _p64(val), _p64(v), _p64(out)))
    return out


def linear_restrict(n_h, n_H, r):
    r = _a64(r)
    out = np.empty(n_H, np.float64)
    _chk(lib().amg_hip_linear_restrict(n_h, n_H, _p64(r), _p64(out)))
    return out


def linear_prolong_add(n_h, n_H, u_H, u_h):
    u_H = _a64(u_H)
    u_h = np.array(u_h, dtype=np.float64, copy=True)
    _chk(lib().amg_hip_linear_prolong_add(n_h, n_H, _p64(u_H), _p64(u_h)))
    return u_h


def _dims3(dims):
    """(dim, int64[3]) of a 2- or 3-tuple of grid sizes, x fastest."""
    dims = tuple(int(x) for x in dims)
    if len(dims) not in (2, 3):
        raise ValueError(f"`dims` must have 2 or 3 entries, got {len(dims)}")
    return len(dims), np.array(dims + (1,) * (3 - len(dims)), np.int64)


def _tensor_sizes(d3, dim, axes=None):
    m = (7 if dim == 3 else 3) if axes is None else int(axes)
    c = [int(d3[a]) // 2 if (m >> a) & 1 and a < dim else int(d3[a]) for a in range(3)]
    return int(d3[0] * d3[1] * d3[2]), c[0] * c[1] * c[2]


def tensor_axis_strength(colptr, rowind, val, dims):
    """w of the automatic semi-coarsening rule: per axis the largest |a_ij| between neighbours along
    that axis alone (amg_hip_tensor_axis_strength; host only)."""
    colptr, rowind, val = _a32(colptr), _a32(rowind), _a64(val)
    dim, d3 = _dims3(dims)
    w = np.zeros(3, np.float64)
    st = lib().amg_hip_tensor_axis_strength(colptr.size - 1, _p32(colptr), _p32(rowind), _p64(val), dim,
                                            d3.ctypes.data_as(_i64p), _p64(w))
    if st == EINVAL:
        raise ValueError(lib().amg_hip_last_error().decode())
    _chk(st)
    return w


def tensor_restrict(dims, r, axes=None, natural_sides=0, periodic_axes=0):
    """f_H = R r for the full-coarsening transfer of the fine grid `dims` (amg_hip_tensor_restrict);
    axes: the mask of coarsened axes instead (amg_hip_tensor_restrict_axes); natural_sides != 0: the
    mask of sides without a Dirichlet condition (amg_hip_tensor_restrict_bc); periodic_axes != 0: the
    mask of periodic axes (amg_hip_tensor_restrict_per)."""
    dim, d3 = _dims3(dims)
    r = _a64(r)
    n_h, n_H = _tensor_sizes(d3, dim, axes)
    if r.size != n_h:
        raise ValueError(f"`r` must have {n_h} entries, got {r.size}")
    out = np.empty(max(n_H, 0), np.float64)
    if periodic_axes:
        st = lib().amg_hip_tensor_restrict_per(dim, d3.ctypes.data_as(_i64p), (7 if dim == 3 else 3) if axes is None
                                               else int(axes), int(natural_sides), int(periodic_axes), _p64(r),
                                               _p64(out))
    elif natural_sides:
        st = lib().amg_hip_tensor_restrict_bc(dim, d3.ctypes.data_as(_i64p), (7 if dim == 3 else 3) if axes is None
                                              else int(axes), int(natural_sides), _p64(r), _p64(out))
    elif axes is not None:
        st = lib().amg_hip_tensor_restrict_axes(dim, d3.ctypes.data_as(_i64p), int(axes), _p64(r), _p64(out))
    else:
        st = lib().amg_hip_tensor_restrict(dim, d3.ctypes.data_as(_i64p), _p64(r), _p64(out))
    if st == EINVAL:
        raise ValueError(lib().amg_hip_last_error().decode())
    _chk(st)
    return out


def tensor_prolong_add(dims, u_H, u_h, axes=None, natural_sides=0, periodic_axes=0):
    """u_h + P u_H for the same transfer (amg_hip_tensor_prolong_add, amg_hip_tensor_prolong_add_axes
    with the mask `axes`, amg_hip_tensor_prolong_add_bc with natural_sides != 0,
    amg_hip_tensor_prolong_add_per with periodic_axes != 0); returns a new array."""
    dim, d3 = _dims3(dims)
    u_H = _a64(u_H)
    u_h = np.array(u_h, dtype=np.float64, copy=True)
    n_h, n_H = _tensor_sizes(d3, dim, axes)
    if u_h.size != n_h or u_H.size != n_H:
        raise ValueError(f"`u_h` / `u_H` must have {n_h} / {n_H} entries, got {u_h.size} / {u_H.size}")
    if periodic_axes:
        st = lib().amg_hip_tensor_prolong_add_per(dim, d3.ctypes.data_as(_i64p), (7 if dim == 3 else 3) if axes is None
                                                  else int(axes), int(natural_sides), int(periodic_axes), _p64(u_H),
                                                  _p64(u_h))
    elif natural_sides:
        st = lib().amg_hip_tensor_prolong_add_bc(dim, d3.ctypes.data_as(_i64p), (7 if dim == 3 else 3) if axes is None
                                                 else int(axes), int(natural_sides), _p64(u_H), _p64(u_h))
    elif axes is not None:
        st = lib().amg_hip_tensor_prolong_add_axes(dim, d3.ctypes.data_as(_i64p), int(axes), _p64(u_H), _p64(u_h))
    else:
        st = lib().amg_hip_tensor_prolong_add(dim, d3.ctypes.data_as(_i64p), _p64(u_H), _p64(u_h))
    if st == EINVAL:
        raise ValueError(lib().amg_hip_last_error().decode())
    _chk(st)
    return u_h


def _axis_sizes(dims, axis):
    dim, d3 = _dims3(dims)
    axis = int(axis)
    n_h = int(d3[0] * d3[1] * d3[2])
    n_H = n_h // int(d3[axis]) * (int(d3[axis]) // 2) if 0 <= axis < dim else 0
    return dim, d3, axis, n_h, n_H


def axis_restrict(dims, axis, W, r, periodic=None, vec_shift=0):
    """f_H = R r for the single-axis transfer of the fine grid `dims` with the compact weights W of
    Multigrid.axis_weights, 2 (n_h - n_H) doubles (amg_hip_axis_restrict: K-AxisRestrict).
    periodic (not None: amg_hip_axis_restrict_per): True = the axis wraps (even, at least 4 points; W[0]
    of a line is w_lo of fine point 0 from the last coarse point); vec_shift=1 puts the device vectors 8
    bytes past a 16-byte boundary."""
    dim, d3, axis, n_h, n_H = _axis_sizes(dims, axis)
    W, r = _a64(np.ravel(W)), _a64(r)
    if n_H and (r.size != n_h or W.size != 2 * (n_h - n_H)):
        raise ValueError(f"`r` / `W` must have {n_h} / {2 * (n_h - n_H)} entries, got {r.size} / {W.size}")
    out = np.empty(n_H, np.float64)
    if periodic is None and not vec_shift:
        st = lib().amg_hip_axis_restrict(dim, d3.ctypes.data_as(_i64p), axis, _p64(W), _p64(r), _p64(out))
    else:
        st = lib().amg_hip_axis_restrict_per(dim, d3.ctypes.data_as(_i64p), axis, int(periodic or 0), _p64(W),
                                             _p64(r), _p64(out), int(vec_shift))
    if st == EINVAL:
        raise ValueError(lib().amg_hip_last_error().decode())
    _chk(st)
    return out


def axis_prolong_add(dims, axis, W, u_H, u_h, periodic=None, vec_shift=0):
    """u_h + P u_H for the same transfer (amg_hip_axis_prolong_add: K-AxisProlong); returns a new array.
    periodic / vec_shift: as for axis_restrict (amg_hip_axis_prolong_add_per)."""
    dim, d3, axis, n_h, n_H = _axis_sizes(dims, axis)
    W, u_H = _a64(np.ravel(W)), _a64(u_H)
    u_h = np.array(u_h, dtype=np.float64, copy=True)
    if n_H and (u_h.size != n_h or u_H.size != n_H or W.size != 2 * (n_h - n_H)):
        raise ValueError(f"`u_h` / `u_H` / `W` must have {n_h} / {n_H} / {2 * (n_h - n_H)} entries, got "
                         f"{u_h.size} / {u_H.size} / {W.size}")
    if periodic is None and not vec_shift:
        st = lib().amg_hip_axis_prolong_add(dim, d3.ctypes.data_as(_i64p), axis, _p64(W), _p64(u_H), _p64(u_h))
    else:
        st = lib().amg_hip_axis_prolong_add_per(dim, d3.ctypes.data_as(_i64p), axis, int(periodic or 0), _p64(W),
                                                _p64(u_H), _p64(u_h), int(vec_shift))
    if st == EINVAL:
        raise ValueError(lib().amg_hip_last_error().decode())
    _chk(st)
    return u_h


def rss(colptr, rowind, val, u, b):
    colptr, rowind, val, u, b = _a32(colptr), _a32(rowind), _a64(val), _a64(u), _a64(b)
    out = C.c_double(0)
    _chk(lib().amg_hip_rss_host(colptr.size - 1, _p32(colptr), _p32(rowind), _p64(val),
                                _p64(u), _p64(b), C.byref(out)))
    return out.value


def coarse_solve(colptr, rowind, val, f):
    colptr, rowind, val, f = _a32(colptr), _a32(rowind), _a64(val), _a64(f)
    x = np.empty(f.size, np.float64)
    w = C.c_int64(0)
    _chk(lib().amg_hip_coarse_solve(f.size, _p32(colptr), _p32(rowind), _p64(val), _p64(f),
                                    _p64(x), C.byref(w)))
    return x, w.value


def coarse_solve_fast(colptr, rowind, val, f):
    colptr, rowind, val, f = _a32(colptr), _a32(rowind), _a64(val), _a64(f)
    x = np.empty(f.size, np.float64)
    w, c = C.c_int64(0), C.c_int32(0)
    _chk(lib().amg_hip_coarse_solve_fast(f.size, _p32(colptr), _p32(rowind), _p64(val), _p64(f),
                                         _p64(x), C.byref(w), C.byref(c)))
    return x, w.value, c.value


def csr_shape(rowptr):
    rowptr = _a32(rowptr)
    mb, mr = C.c_int32(0), C.c_int32(0)
    _chk(lib().amg_hip_csr_shape(rowptr.size - 1, _p32(rowptr), C.byref(mb), C.byref(mr)))
    return mb.value, mr.value
