"""ctypes binding of liblcs_hip.so -- one prototype per symbol of include/lcs_hip.h.

The library is the product; there is no Python or CPU fallback.  If it is not
built, loading fails loudly with the command that builds it.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "liblcs_hip.so")

LC_VERSION = 104     # include/lcs_hip.h: the ABI these prototypes describe (checked against lc_version() in load())
LC_F32, LC_F64, LC_F64_WIND_F32, LC_F64_WIND_F32_LIN32 = 0, 1, 2, 3
LC_OK, LC_EINVAL, LC_EUNSUPPORTED, LC_EHIP, LC_ENOMEM, LC_ERCCL = 0, -1, -2, -3, -4, -5
LC_LAYOUT_REFERENCE, LC_LAYOUT_PHYSICAL = 0, 1
LC_X_CLAMP_POINT, LC_X_CYCLIC, LC_X_CLAMP_REFERENCE_OUTER = 0, 1, 2
LC_GRID_REGULAR, LC_GRID_GAUSSIAN = 0, 1
LC_F64_AUTO, LC_F64_EXACT_ORDER, LC_F64_FAST = 0, 1, 2
LC_EXACT_ORDER_MAX_SEEDS = 1 << 18
LC_TRACK_MAX_REACH = 16

_vp, _i, _d, _sz = C.c_void_p, C.c_int, C.c_double, C.c_size_t

# name -> (restype, argtypes); mirrors include/lcs_hip.h declaration by declaration
PROTOTYPES = {
    "lc_version": (_i, []),
    "lc_last_error": (C.c_char_p, []),
    "lc_build_id": (C.c_char_p, []),
    "lc_ctx_create": (_i, [_i, C.POINTER(_vp)]),
    "lc_ctx_destroy": (_i, [_vp]),
    "lc_ctx_set_stream": (_i, [_vp, _vp]),
    "lc_ctx_use_own_stream": (_i, [_vp]),
    "lc_sync": (_i, [_vp]),
    "lc_ctx_set_lds_tiles": (_i, [_vp, _i]),
    "lc_ctx_set_sigma_march": (_i, [_vp, _i]),
    "lc_ctx_set_level_chunk": (_i, [_vp, _i]),
    "lc_ctx_get_level_chunk": (_i, [_vp, C.POINTER(_i)]),
    "lc_ctx_set_level_grading": (_i, [_vp, _i, _i, _i]),
    "lc_ctx_get_level_grading": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "lc_ctx_set_f64_fidelity": (_i, [_vp, _i]),
    "lc_ctx_get_f64_fidelity": (_i, [_vp, C.POINTER(_i)]),
    "lc_ctx_set_host_pipeline": (_i, [_vp, _i]),
    "lc_ctx_last_host_marks": (_i, [_vp, C.POINTER(C.c_double)]),
    "lc_copy_to_device": (_i, [_vp, _vp, _vp, C.c_size_t]),
    "lc_copy_to_host": (_i, [_vp, _vp, _vp, C.c_size_t]),
    "lc_ctx_set_host_cache": (_i, [_vp, _i]),
    "lc_ctx_trim": (_i, [_vp]),
    "lc_ctx_set_xcd_split": (_i, [_vp, _i]),
    "lc_ctx_set_flag_allreduce": (_i, [_vp, _vp, _vp]),
    "lc_ctx_last_advect_kernel": (C.c_char_p, [_vp]),
    "lc_ctx_last_advect_launches": (_i, [_vp]),
    "lc_ctx_last_sigma_kernel": (C.c_char_p, [_vp]),
    "lc_ctx_last_pack_kernel": (C.c_char_p, [_vp]),
    "lc_ctx_last_tracer_kernel": (C.c_char_p, [_vp]),
    "lc_ctx_set_verify": (_i, [_vp, _i]),
    "lc_ctx_read_verify": (_i, [_vp, C.POINTER(C.c_uint), _i]),
    "lc_malloc": (_i, [_vp, _sz, C.POINTER(_vp)]),
    "lc_free": (_i, [_vp, _vp]),
    "lc_memcpy_h2d": (_i, [_vp, _vp, _vp, _sz]),
    "lc_memcpy_d2h": (_i, [_vp, _vp, _vp, _sz]),
    "lc_packed_elems": (_sz, [_i, _i, _i]),
    "lc_field_pack": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "lc_field_pack_deferred": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "lc_ctx_flush_pack": (_i, [_vp]),
    "lc_ctx_pack_pending": (_i, [_vp]),
    "lc_ctx_set_deferred_pack": (_i, [_vp, _i]),
    "lc_ctx_set_deferred_pack_mix": (_i, [_vp, _i, _i, _i]),
    "lc_field_extrapolate": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "lc_regrid_common_grid": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _vp]),
    "lc_spectral_truncate": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "lc_inspect_gridtype": (_i, [_vp, _i, C.POINTER(_i)]),
    "lc_advect": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _d, _d, _d, _d, _vp, _i, _vp, _i, _i, _i,
                       _d, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "lc_advect_from": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _d, _d, _d, _d, _vp, _i, _vp, _i, _i, _i, _vp, _vp,
                            _d, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "lc_advect_batch": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _d, _d, _d, _d, _vp, _i, _vp, _i, _i, _i, _vp, _vp,
                             _d, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "lc_sample": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _d, _d, _d, _d, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "lc_sample_raw": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _d, _d, _d, _d, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "lc_sigma": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _d, _d, _i, _i, _i, _i, _vp]),
    "lc_sigma_batch": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _d, _d, _i, _i, _i, _vp]),
    "lc_strain": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _d, _d, _i, _i, _vp, _vp, _vp, _vp]),
    "lc_ctx_last_strain_kernel": (C.c_char_p, [_vp]),
    "lc_flowmap_gradient": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _d, _d, _i, _vp]),
    "lc_fourth_order_derivative": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "lc_gaussian_filter": (_i, [_vp, _vp, _i, _i, _i, _d, _vp, _vp]),
    "lc_ridge_classify": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _d, _vp, _vp, _vp, _vp]),
    "lc_comm_unique_id": (_i, [_vp, _sz]),
    "lc_comm_create": (_i, [_vp, _i, _i, _vp, _sz, C.POINTER(_vp)]),
    "lc_comm_destroy": (_i, [_vp]),
    "lc_comm_count": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "lc_comm_flag_allreduce": (_i, [_vp, _vp, _sz]),
    "lc_halo_exchange": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "lc_common_grid": (_i, [C.POINTER(_i), C.POINTER(_i), _vp, _vp]),
    "lc_lcs_global_host": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _d, _i, _i, _d, _i, _i, _vp, _vp, _vp]),
    "lc_lcs_host": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _i,
                         _d, _i, _i, _i, _i, _i, _d, _i, _i, _vp, _vp, _vp, _vp, _vp]),
}

FLAG_ALLREDUCE_FN = C.CFUNCTYPE(_i, _vp, _vp, _sz)   # lc_flag_allreduce_fn of include/lcs_hip.h


class AdvectArgs(C.Structure):
    """``lc_advect_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("packed_lin", _vp), ("packed_cub", _vp), ("packed_ext", _vp),
                ("u_raw", _vp), ("v_raw", _vp),
                ("dtype", _i), ("nt", _i), ("ny_f", _i), ("nx_f", _i),
                ("lat_min", _d), ("lat_max", _d), ("lon_min", _d), ("lon_max", _d),
                ("seed_lat_dev", _vp), ("ny", _i), ("seed_lon_dev", _vp), ("nx", _i),
                ("row0", _i), ("ny_global", _i),
                ("x_start", _vp), ("y_start", _vp),
                ("timestep", _d),
                ("settls_order", _i), ("interp_order", _i), ("cyclic_x", _i),
                ("t0", _i), ("nsteps", _i), ("n_members", _i), ("t0_stride", _i),
                ("x_out", _vp), ("y_out", _vp), ("traj_x", _vp), ("traj_y", _vp),
                ("fuse_levels_raw", _i)]


PROTOTYPES["lc_advect_ex"] = (_i, [_vp, C.POINTER(AdvectArgs)])
PROTOTYPES["lc_advect_series"] = (_i, [_vp, C.POINTER(AdvectArgs)])
PROTOTYPES["lc_advect_series_dirs"] = (_i, [_vp, C.POINTER(AdvectArgs), _i])


class TracerArgs(C.Structure):
    """``lc_tracer_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("tracer_lin", _vp), ("tracer_cub", _vp), ("c1_raw", _vp), ("c2_raw", _vp),
                ("dtype", _i), ("nt", _i), ("ny_f", _i), ("nx_f", _i),
                ("lat_min", _d), ("lat_max", _d), ("lon_min", _d), ("lon_max", _d),
                ("ny", _i), ("nx", _i), ("row0", _i), ("ny_global", _i), ("interp_order", _i),
                ("traj_x", _vp), ("traj_y", _vp),
                ("level0", _i), ("n_levels", _i),
                ("c1_out", _vp), ("c2_out", _vp),
                ("sum1", _vp), ("sum2", _vp),
                ("mean1_out", _vp), ("mean2_out", _vp),
                ("mean_count", _i)]


PROTOTYPES["lc_tracer_sample"] = (_i, [_vp, C.POINTER(TracerArgs)])


class ComponentSumsArgs(C.Structure):
    """``lc_component_sums_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("labels", _vp), ("counts", _vp), ("intensity", _vp),
                ("dtype", _i), ("ny", _i), ("nx", _i), ("n_members", _i),
                ("cyclic_x", _i), ("n_max", _i),
                ("root_out", _vp), ("area_out", _vp), ("moments_out", _vp),
                ("sum_out", _vp), ("max_out", _vp), ("min_out", _vp)]


PROTOTYPES["lc_label_work_elems"] = (_sz, [_i, _i, _i])
PROTOTYPES["lc_label_components"] = (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp])
PROTOTYPES["lc_component_sums"] = (_i, [_vp, C.POINTER(ComponentSumsArgs)])
PROTOTYPES["lc_component_apply"] = (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _d, _vp])


class ComponentSphereSumsArgs(C.Structure):
    """``lc_component_sphere_sums_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("labels", _vp), ("counts", _vp), ("intensity", _vp),
                ("dtype", _i), ("ny", _i), ("nx", _i), ("n_members", _i),
                ("n_max", _i),
                ("cos_lat", _vp), ("sin_lat", _vp), ("row_weight", _vp),
                ("cos_lon", _vp), ("sin_lon", _vp), ("col_weight", _vp),
                ("radius", _d),
                ("root_out", _vp), ("sums_out", _vp), ("max_out", _vp), ("min_out", _vp), ("props_out", _vp)]


PROTOTYPES["lc_component_sphere_sums"] = (_i, [_vp, C.POINTER(ComponentSphereSumsArgs)])


class TrackSpansArgs(C.Structure):
    """``lc_track_spans_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("labels", _vp), ("count", _vp),
                ("ny", _i), ("nx", _i), ("n_times", _i),
                ("n_max", _i),
                ("first_out", _vp), ("last_out", _vp), ("volume_out", _vp)]


PROTOTYPES["lc_track_work_elems"] = (_sz, [_i, _i, _i])
PROTOTYPES["lc_label_tracks"] = (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp])
PROTOTYPES["lc_track_spans"] = (_i, [_vp, C.POINTER(TrackSpansArgs)])


class DistanceArgs(C.Structure):
    """``lc_distance_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("mask", _vp),
                ("dtype", _i), ("ny", _i), ("nx", _i), ("n_members", _i),
                ("cyclic_x", _i),
                ("sampling_y", _d), ("sampling_x", _d),
                ("max_distance", _d),
                ("dist_out", _vp), ("nearest_out", _vp), ("work_dev", _vp)]


PROTOTYPES["lc_distance_work_elems"] = (_sz, [_i, _i, _i])
PROTOTYPES["lc_distance_transform"] = (_i, [_vp, C.POINTER(DistanceArgs)])


class SphereDistanceArgs(C.Structure):
    """``lc_sphere_distance_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("mask", _vp),
                ("dtype", _i), ("ny", _i), ("nx", _i), ("n_members", _i),
                ("cos_lat", _vp), ("sin_lat", _vp), ("cos_lon", _vp), ("sin_lon", _vp),
                ("radius", _d), ("max_chord2", _d), ("max_distance", _d),
                ("dist_out", _vp), ("nearest_out", _vp), ("cost_out", _vp), ("work_dev", _vp)]


PROTOTYPES["lc_sphere_distance_work_elems"] = (_sz, [_i, _i, _i])
PROTOTYPES["lc_sphere_distance"] = (_i, [_vp, C.POINTER(SphereDistanceArgs)])

LC_MORPH_THIN, LC_MORPH_DILATE = 0, 1


class MorphArgs(C.Structure):
    """``lc_morph_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("mask", _vp),
                ("dtype", _i), ("ny", _i), ("nx", _i), ("n_members", _i),
                ("op", _i), ("cyclic_x", _i),
                ("table", _vp),
                ("structure", _i), ("max_iterations", _i), ("iterations_per_launch", _i),
                ("out", _vp), ("launches_out", C.POINTER(_i)), ("work_dev", _vp)]


PROTOTYPES["lc_morph_work_elems"] = (_sz, [_i, _i, _i])
PROTOTYPES["lc_mask_morphology"] = (_i, [_vp, C.POINTER(MorphArgs)])


LC_LINE_STATE, LC_LINE_CANONICAL, LC_LINE_HEAD_IS_END, LC_LINE_RING, LC_LINE_CORNER_LINK = 1, 2, 4, 8, 16


class LinesArgs(C.Structure):
    """``lc_lines_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("mask", _vp),
                ("dtype", _i), ("ny", _i), ("nx", _i), ("n_members", _i),
                ("cyclic_x", _i),
                ("cos_lat", _vp), ("sin_lat", _vp), ("cos_lon", _vp), ("sin_lon", _vp),
                ("radius", _d),
                ("links_out", _vp), ("counts_out", _vp),
                ("key_out", _vp), ("pos_out", _vp), ("ndiag_out", _vp), ("head_out", _vp),
                ("flags_out", _vp),
                ("dist_out", _vp), ("link_length_out", _vp),
                ("rounds_out", C.POINTER(_i)), ("work_dev", _vp)]


PROTOTYPES["lc_lines_work_elems"] = (_sz, [_i, _i, _i])
PROTOTYPES["lc_trace_lines"] = (_i, [_vp, C.POINTER(LinesArgs)])


class LinkLengthsArgs(C.Structure):
    """``lc_link_lengths_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("from_", _vp), ("to", _vp),
                ("n_pairs", C.c_longlong),
                ("ny", _i), ("nx", _i),
                ("cos_lat", _vp), ("sin_lat", _vp), ("cos_lon", _vp), ("sin_lon", _vp),
                ("radius", _d),
                ("length_out", _vp)]


PROTOTYPES["lc_line_link_lengths"] = (_i, [_vp, C.POINTER(LinkLengthsArgs)])


class LocalThresholdArgs(C.Structure):
    """``lc_local_threshold_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("f", _vp),
                ("dtype", _i), ("ny", _i), ("nx", _i), ("n_members", _i),
                ("sigma_y", _d), ("sigma_x", _d),
                ("offset", _d),
                ("cyclic", _i),
                ("work", _vp), ("threshold_out", _vp), ("mask_out", _vp)]


PROTOTYPES["lc_local_threshold_work_elems"] = (_sz, [_i, _i, _i])
PROTOTYPES["lc_local_threshold"] = (_i, [_vp, C.POINTER(LocalThresholdArgs)])
PROTOTYPES["lc_ctx_last_threshold_kernel"] = (C.c_char_p, [_vp])


class IdwArgs(C.Structure):
    """``lc_idw_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("src_x", _vp), ("src_y", _vp), ("src_z", _vp),
                ("values", _vp),
                ("tgt_x", _vp), ("tgt_y", _vp), ("tgt_z", _vp),
                ("dtype", _i), ("n_src", _i), ("n_tgt", _i), ("n_planes", _i),
                ("power", _d), ("radius", _d), ("max_chord2", _d), ("max_distance", _d),
                ("out", _vp), ("weight_out", _vp), ("count_out", _vp), ("work_dev", _vp)]


PROTOTYPES["lc_idw_work_elems"] = (_sz, [_i, _i, _i])
PROTOTYPES["lc_idw_interp"] = (_i, [_vp, C.POINTER(IdwArgs)])
PROTOTYPES["lc_ctx_last_idw_kernel"] = (C.c_char_p, [_vp])


LC_ORIENT_LEFT, LC_ORIENT_NORTH, LC_ORIENT_EAST = 0, 1, 2
LC_TRANSECT_LINEAR, LC_TRANSECT_NEAREST = 0, 1


class TransectsArgs(C.Structure):
    """``lc_transects_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("pixel", _vp), ("point_line", _vp),
                ("line_offset", _vp), ("line_count", _vp), ("line_plane", _vp), ("line_closed", _vp),
                ("cos_lat", _vp), ("sin_lat", _vp), ("cos_lon", _vp), ("sin_lon", _vp),
                ("lat_deg", _vp), ("lon_deg", _vp), ("cos_off", _vp), ("sin_off", _vp),
                ("fields", _vp),
                ("dtype", _i), ("ny", _i), ("nx", _i), ("n_planes", _i), ("n_points", _i), ("n_lines", _i), ("n_offsets", _i),
                ("n_fields", _i),
                ("smooth", _i), ("orient", _i), ("method", _i), ("cyclic_x", _i),
                ("normal_out", _vp), ("lat_out", _vp), ("lon_out", _vp), ("values_out", _vp), ("mean_out", _vp), ("count_out", _vp)]


PROTOTYPES["lc_ridge_transects"] = (_i, [_vp, C.POINTER(TransectsArgs)])
PROTOTYPES["lc_ctx_last_transects_kernel"] = (C.c_char_p, [_vp])



class RidgesArgs(C.Structure):
    """``lc_ridges_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("f", _vp),
                ("ny", _i), ("nx", _i), ("n_members", _i),
                ("dx_dev", _vp),
                ("dy", _d), ("sigma", _d), ("tolerance", _d),
                ("isglobal", _i),
                ("work_dev", _vp),
                ("mask_out", _vp), ("eigmin_out", _vp), ("dt_out", _vp),
                ("eigvec_out", _vp), ("grad_out", _vp)]


PROTOTYPES["lc_ridges_work_elems"] = (_sz, [_i, _i, _i])
PROTOTYPES["lc_ridges_batch"] = (_i, [_vp, C.POINTER(RidgesArgs)])
PROTOTYPES["lc_ctx_last_ridges_kernel"] = (C.c_char_p, [_vp])


class AuxGradientArgs(C.Structure):
    """``lc_aux_gradient_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("x_e", _vp), ("y_e", _vp), ("x_w", _vp), ("y_w", _vp), ("x_n", _vp), ("y_n", _vp), ("x_s", _vp), ("y_s", _vp),
                ("dtype", _i), ("ny", _i), ("nx", _i), ("n_members", _i),
                ("seed_lat_dev", _vp), ("sep_lat_dev", _vp), ("sep_lon_dev", _vp),
                ("tensor_layout", _i),
                ("sigma_out", _vp), ("s1_out", _vp), ("s2_out", _vp), ("e_lon_out", _vp), ("e_lat_out", _vp)]


PROTOTYPES["lc_aux_gradient"] = (_i, [_vp, C.POINTER(AuxGradientArgs)])
PROTOTYPES["lc_ctx_last_aux_kernel"] = (C.c_char_p, [_vp])


class FsleArgs(C.Structure):
    """``lc_fsle_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("traj_x", _vp), ("traj_y", _vp),
                ("dtype", _i), ("ny", _i), ("nx", _i), ("n_levels", _i), ("level0", _i),
                ("seed_lat_dev", _vp), ("seed_lon_dev", _vp),
                ("mode", _i), ("n_thr", _i),
                ("thresholds", C.c_double * 8),
                ("radius", C.c_double), ("timestep", C.c_double),
                ("cyclic_x", _i),
                ("tau", _vp), ("fsle", _vp)]


LC_FSLE_RATIO, LC_FSLE_DISTANCE = 0, 1
PROTOTYPES["lc_fsle_update"] = (_i, [_vp, C.POINTER(FsleArgs)])
PROTOTYPES["lc_ctx_last_fsle_kernel"] = (C.c_char_p, [_vp])


class VorticityArgs(C.Structure):
    """``lc_vorticity_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("u", _vp), ("v", _vp),
                ("dtype", _i), ("nt", _i), ("ny_f", _i), ("nx_f", _i),
                ("lat_min", C.c_double), ("lat_max", C.c_double), ("lon_min", C.c_double), ("lon_max", C.c_double),
                ("cyclic_x", _i), ("deviation", _i),
                ("radius", C.c_double),
                ("given_dev", _vp),
                ("omega", _vp), ("level_mean", _vp), ("work_dev", _vp)]


LC_VORT_DEVIATION_DOMAIN, LC_VORT_DEVIATION_NONE, LC_VORT_DEVIATION_GIVEN = 0, 1, 2
PROTOTYPES["lc_vorticity_work_elems"] = (_sz, [_i, _i, _i])
PROTOTYPES["lc_vorticity"] = (_i, [_vp, C.POINTER(VorticityArgs)])
PROTOTYPES["lc_ctx_last_vorticity_kernel"] = (C.c_char_p, [_vp])


class LavdArgs(C.Structure):
    """``lc_lavd_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("traj_x", _vp), ("traj_y", _vp), ("c", _vp),
                ("dtype", _i), ("n", _i), ("n_levels", _i), ("level0", _i),
                ("timestep", C.c_double), ("radius", C.c_double),
                ("acc", _vp),
                ("lavd", _vp), ("rotation", _vp), ("length", _vp)]


PROTOTYPES["lc_lavd_update"] = (_i, [_vp, C.POINTER(LavdArgs)])
PROTOTYPES["lc_ctx_last_lavd_kernel"] = (C.c_char_p, [_vp])


class FootprintArgs(C.Structure):
    """``lc_footprint_args`` of include/lcs_hip.h, field for field."""
    _fields_ = [("struct_size", _sz),
                ("traj_x", _vp), ("traj_y", _vp), ("c", _vp),
                ("q", _vp),
                ("dtype", _i), ("ny", _i), ("nx", _i), ("n", _i), ("n_levels", _i), ("level0", _i), ("final", _i),
                ("ny_t", _i), ("nx_t", _i),
                ("lat0", C.c_double), ("lat1", C.c_double), ("lon0", C.c_double), ("lon1", C.c_double),
                ("cyclic_x", _i),
                ("c_scale", C.c_double),
                ("zero_first", _i),
                ("hits", _vp), ("mass", _vp), ("csum", _vp), ("chits", _vp),
                ("stats", _vp)]


LC_FOOTPRINT_AUTO, LC_FOOTPRINT_DIRECT, LC_FOOTPRINT_TILED, LC_FOOTPRINT_TILED_CENSUS = -1, 0, 1, 2
PROTOTYPES["lc_footprint_update"] = (_i, [_vp, C.POINTER(FootprintArgs)])
PROTOTYPES["lc_ctx_last_footprint_kernel"] = (C.c_char_p, [_vp])
PROTOTYPES["lc_ctx_set_footprint_form"] = (_i, [_vp, _i])

_lib = None


class LCSError(RuntimeError):
    """A C-ABI call returned LC_EHIP / LC_ERCCL."""


def load(path: str | None = None, import_torch: bool = True):
    """Load liblcs_hip.so and attach prototypes.  Raises if it is not built.  ``import_torch=False``: a torch-free host
    process (ctypes only, e.g. the one-call routes or tests/fake_rccl_driver.py) skips the torch import below."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # LCS_LIB: an experiment build of the same library (python -m lagrangiancoherence_amd.build --out ...)
    p = path or os.environ.get("LCS_LIB") or LIB_PATH
    # One HIP runtime per process: torch wheels bundle their own ROCm libraries, and loading ours
    # (linked against /opt/rocm) first leaves the process with two HSA runtimes and "no ROCm-capable
    # device".  Importing torch first makes our DT_NEEDED entries resolve to the copies torch loaded.
    if import_torch:
        try:
            import torch  # noqa: F401
        except ImportError:  # torch-free hosts use lc_lcs_host only
            pass
    if not os.path.exists(p):
        raise RuntimeError(
            f"{p} is missing: the HIP extension is the only compute path of this package "
            "(no CPU fallback). Build it with `python -m lagrangiancoherence_amd.build`.")
    lib = C.CDLL(p)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.lc_version() != LC_VERSION:   # an argument list changed between ABI versions: never call across them
        raise RuntimeError(f"{p} is ABI version {lib.lc_version()}, these bindings are for {LC_VERSION}: rebuild it with "
                           "`python -m lagrangiancoherence_amd.build --force`")
    if path is None:
        _lib = lib
    return lib


def check(status: int, lib=None):
    """Translate an lc_status into the exception the reference would raise."""
    if status == LC_OK:
        return
    lib = lib or load()
    msg = lib.lc_last_error().decode("utf-8", "replace")
    if status in (LC_EINVAL, LC_EUNSUPPORTED):
        raise ValueError(msg)
    if status == LC_ENOMEM:
        raise MemoryError(msg)
    raise LCSError(msg)
