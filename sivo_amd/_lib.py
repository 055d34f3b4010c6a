"""ctypes binding of libsivo_hip.so (the C ABI declared in include/sivo_hip.h).

There is no CPU fallback: if the HIP library is missing, or no HIP device is
visible when a compute entry point is called, the call fails loudly.
"""
import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsivo_hip.so")

OK = 0
ERR_INVALID_ARGUMENT = 1
ERR_RUNTIME = 2
ERR_UNSUPPORTED = 3
ERR_IMAGE_TOO_SMALL = 4
ERR_CAPACITY = 5


class SivoError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libsivo_hip error {code}: {msg}")
        self.code = code


class SivoInvalidArgument(SivoError, ValueError):
    """SIVO_ERR_INVALID_ARGUMENT: where the reference throws std::invalid_argument."""


class KeyPoint(C.Structure):  # == cv::KeyPoint / SivoKeyPoint (28 bytes)
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("size", C.c_float), ("angle", C.c_float),
                ("response", C.c_float), ("octave", C.c_int32), ("class_id", C.c_int32)]


class OpProfile(C.Structure):  # == SivoOpProfile
    _fields_ = [("layer", C.c_char * 64), ("kernel", C.c_char * 96), ("samples", C.c_int32), ("launches", C.c_int32),
                ("flops_per_sample", C.c_double), ("bytes_per_sample", C.c_double), ("ms_total", C.c_double),
                ("kernel_launches", C.c_int32), ("pad_", C.c_int32)]


class SegnetOptions(C.Structure):   # == SivoSegnetOptions
    _fields_ = [("struct_size", C.c_uint32), ("lanes", C.c_int32), ("gemm", C.c_int32), ("no_direct_f16x3", C.c_int32),
                ("no_packed_activations", C.c_int32), ("conv7_fp32", C.c_int32), ("wino4_workspace_mb", C.c_int32), ("debug_sync", C.c_int32)]


class BaOptions(C.Structure):   # == SivoBaOptions
    _fields_ = [("size", C.c_uint32), ("solver", C.c_int32)]


class SearchQuery(C.Structure):   # == SivoSearchQuery (36 bytes)
    _fields_ = [("u", C.c_float), ("v", C.c_float), ("radius", C.c_float), ("lvl_lo", C.c_int32), ("lvl_hi", C.c_int32),
                ("ur", C.c_float), ("gate", C.c_float), ("angle", C.c_float), ("flags", C.c_int32)]


class SearchRule(C.Structure):    # == SivoSearchRule
    _fields_ = [("th_dist", C.c_int32), ("accept_lt", C.c_int32), ("ratio_mode", C.c_int32), ("nn_ratio", C.c_float),
                ("gate_mode", C.c_int32), ("check_orientation", C.c_int32), ("dynamic", C.c_int32), ("tie_last", C.c_int32),
                ("F12", C.c_float * 9), ("ex", C.c_float), ("ey", C.c_float)]


class Edge(C.Structure):      # == SivoEdge (48 bytes)
    _fields_ = [("pose", C.c_int32), ("point", C.c_int32), ("stereo", C.c_int32), ("pad_", C.c_int32),
                ("obs", C.c_double * 3), ("inv_sigma2", C.c_double)]


class Sim3Match(C.Structure):  # == SivoSim3Match (96 bytes)
    _fields_ = [("obs1", C.c_double * 2), ("inv_sigma2_1", C.c_double), ("obs2", C.c_double * 2), ("inv_sigma2_2", C.c_double),
                ("x1c", C.c_double * 3), ("x2c", C.c_double * 3)]


class Sim3Problem(C.Structure):  # == SivoSim3Problem (one problem of sivo_sim3_optimize_batch)
    _fields_ = [("s12", C.c_double * 8), ("k1", C.c_double * 4), ("k2", C.c_double * 4), ("matches", C.c_void_p),
                ("n", C.c_int32), ("th2", C.c_float), ("fix_scale", C.c_int32), ("n_inliers", C.c_int32),
                ("outlier", C.c_void_p), ("chi2_12", C.c_void_p), ("chi2_21", C.c_void_p),
                ("iterations", C.c_int32), ("trials", C.c_int32)]


class Sim3Pair(C.Structure):  # == SivoSim3Pair (32 bytes): one correspondence of sivo_sim3_ransac
    _fields_ = [("x1c", C.c_float * 3), ("x2c", C.c_float * 3), ("max_err1", C.c_float), ("max_err2", C.c_float)]


class Sim3RansacProblem(C.Structure):  # == SivoSim3RansacProblem (one problem of sivo_sim3_ransac_batch)
    _fields_ = [("pairs", C.c_void_p), ("n", C.c_int32), ("k1", C.c_float * 4), ("k2", C.c_float * 4), ("triples", C.c_void_p),
                ("n_hyp", C.c_int32), ("min_inliers", C.c_int32), ("fix_scale", C.c_int32), ("count", C.c_void_p), ("T", C.c_void_p),
                ("inlier_bits", C.c_void_p), ("first_accept", C.c_int32), ("best", C.c_int32)]


class PnpPoint(C.Structure):  # == SivoPnpPoint (24 bytes): one correspondence of sivo_pnp_ransac
    _fields_ = [("xw", C.c_float * 3), ("u", C.c_float), ("v", C.c_float), ("max_err", C.c_float)]


class PnpRansacProblem(C.Structure):  # == SivoPnpRansacProblem (one problem of sivo_pnp_ransac_batch)
    _fields_ = [("points", C.c_void_p), ("n", C.c_int32), ("K", C.c_float * 4), ("min_inliers", C.c_int32), ("best_in", C.c_int32),
                ("samples", C.c_void_p), ("n_hyp", C.c_int32), ("count", C.c_void_p), ("T", C.c_void_p), ("inlier_bits", C.c_void_p),
                ("refined", C.c_void_p), ("refined_T", C.c_void_p), ("refined_bits", C.c_void_p), ("n_records", C.c_int32)]


class TriKeyFrame(C.Structure):  # == SivoTriKeyFrame (272 bytes): one keyframe header of sivo_triangulate
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3), ("Twc", C.c_float * 12),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("invfx", C.c_float), ("invfy", C.c_float),
                ("mb", C.c_float), ("mbf", C.c_float), ("nlevels", C.c_int32), ("scale_factors", C.c_float * 16),
                ("level_sigma2", C.c_float * 16)]


class TriMatch(C.Structure):  # == SivoTriMatch (64 bytes): one match of sivo_triangulate
    _fields_ = [("x1", C.c_float), ("y1", C.c_float), ("octave1", C.c_int32), ("r1", C.c_float), ("depth1", C.c_float),
                ("x2", C.c_float), ("y2", C.c_float), ("octave2", C.c_int32), ("r2", C.c_float), ("depth2", C.c_float),
                ("entropy1", C.c_double), ("confidence1", C.c_double), ("class1", C.c_uint8), ("class2", C.c_uint8),
                ("pad_", C.c_uint8 * 6)]


class TriProblem(C.Structure):  # == SivoTriProblem (one keyframe pair of sivo_triangulate_batch)
    _fields_ = [("kf1", TriKeyFrame), ("kf2", TriKeyFrame), ("ratio_factor", C.c_float), ("pad_", C.c_int32),
                ("state_cov", C.c_double * 36), ("th_confidence", C.c_double), ("th_entropy", C.c_double),
                ("matches", C.c_void_p), ("n", C.c_int32), ("pad2_", C.c_int32), ("status", C.c_void_p), ("wP", C.c_void_p),
                ("detected_class", C.c_void_p)]


class Frustum(C.Structure):  # == SivoFrustum (96 bytes): the camera of sivo_frustum_cull / sivo_search_local_points
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("bf", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("log_scale_factor", C.c_float), ("nlevels", C.c_int32), ("cos_limit", C.c_float)]


class FuseCamera(C.Structure):  # == SivoFuseCamera (108 bytes): one keyframe's camera of sivo_fuse_batch
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("bf", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("log_scale_factor", C.c_float), ("nlevels", C.c_int32), ("scw_variant", C.c_int32)]


class Sim3Edge(C.Structure):   # == SivoSim3Edge (72 bytes): one EdgeSim3 of sivo_essential_graph_optimize
    _fields_ = [("i", C.c_int32), ("j", C.c_int32), ("meas", C.c_double * 8)]


_vp, _i, _i64, _u64, _sz, _f, _d = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_size_t, C.c_float, C.c_double
_pi32 = C.POINTER(C.c_int32)

# name -> argtypes; every function returns int status unless listed in _RESTYPE
SIGNATURES = {
    "sivo_version": [],
    "sivo_device_count": [],
    "sivo_segnet_create": [C.c_char_p, _sz, _i, _vp, _sz, _i, C.POINTER(_vp)],
    "sivo_segnet_create_opts": [C.c_char_p, _sz, _i, _vp, _sz, _i, _vp, C.POINTER(_vp)],
    "sivo_segnet_create_from_files_opts": [C.c_char_p, C.c_char_p, _i, _i, _vp, C.POINTER(_vp)],
    "sivo_segnet_create_multi_opts": [C.c_char_p, _sz, _i, _vp, _sz, _pi32, _i, _vp, C.POINTER(_vp)],
    "sivo_segnet_create_multi_from_files_opts": [C.c_char_p, C.c_char_p, _i, _pi32, _i, _vp, C.POINTER(_vp)],
    "sivo_caffemodel_weights": [C.c_char_p, _sz, _vp, _sz, _vp, _sz, C.POINTER(_sz)],
    "sivo_segnet_create_from_files": [C.c_char_p, C.c_char_p, _i, _i, C.POINTER(_vp)],
    "sivo_segnet_create_multi": [C.c_char_p, _sz, _i, _vp, _sz, _pi32, _i, C.POINTER(_vp)],
    "sivo_segnet_create_multi_from_files": [C.c_char_p, C.c_char_p, _i, _pi32, _i, C.POINTER(_vp)],
    "sivo_segnet_num_devices": [_vp, _pi32],
    "sivo_segnet_destroy": [_vp],
    "sivo_segnet_shape": [_vp, _pi32, _pi32, _pi32, _pi32, _pi32],
    "sivo_segnet_num_params": [C.c_char_p, _sz, C.POINTER(_sz)],
    "sivo_segnet_forward_dev": [_vp, _vp, _i, _i, _u64, _vp, _vp, _vp, _vp],
    "sivo_mc_finalize_dev": [_vp, _i, _i64, _i, _vp, _vp, _vp, _vp],
    "sivo_mc_reduce_dev": [_vp, _i, _i, _i64, _vp, _vp, _i, _vp],
    "sivo_mc_variance_dev": [_vp, _i, _i, _i64, _vp, _vp, _vp],
    "sivo_segnet_segment": [_vp, _vp, _i, _i, _u64, _vp, _vp, _vp],
    "sivo_segnet_segment_dev": [_vp, _vp, _u64, _vp, _vp, _vp, _vp],
    "sivo_segnet_segment_logits_dev": [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp],
    "sivo_mc_segment_dev": [_vp, _i, _i, _i64, _vp, _vp, _vp, _vp],
    "sivo_segnet_blob": [_vp, C.c_char_p, _vp, _sz, _pi32],
    "sivo_segnet_flops": [_vp, C.POINTER(_d), C.POINTER(_d)],
    "sivo_segnet_profile": [_vp, _i],
    "sivo_segnet_profile_read": [_vp, _vp, _i, _pi32],
    "sivo_segnet_gemm_status": [_vp, _pi32, _pi32, _vp, _i, _pi32],
    "sivo_segnet_prefix_bands": [_vp, _i, _vp, _vp, _vp],
    "sivo_segnet_prefix_band_dev": [_vp, _vp, _i, _i, _vp, _vp],
    "sivo_segnet_forward_banded_dev": [_vp, _vp, _i, _i, _i, C.c_uint64, _vp, _vp, _vp],
    "sivo_segnet_guard_report": [_vp, _vp, _i, _pi32, _vp, _vp, _vp, _vp, _pi32],
    "sivo_segnet_take_overflow": [_vp, _pi32],
    "sivo_orb_create": [_i, _f, _i, _i, _i, _i, C.POINTER(_vp)],
    "sivo_orb_destroy": [_vp],
    "sivo_orb_set_gaussian": [_vp, _i],
    "sivo_orb_set_launch_mode": [_vp, _i],
    "sivo_orb_tables": [_vp, _vp, _vp, _vp, _vp, _vp],
    "sivo_orb_extract": [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _pi32],
    "sivo_orb_extract_dev": [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _pi32, _vp],
    "sivo_orb_extract_pair_dev": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _pi32, _vp, _vp, _i, _pi32, _vp],
    "sivo_orb_profile": [_vp, _i],
    "sivo_orb_profile_read": [_vp, C.POINTER(_d), _pi32, C.POINTER(_d)],
    "sivo_orb_level": [_vp, _i, _vp, _sz, _pi32, _pi32],
    "sivo_orb_candidates": [_vp, _i, _vp, _i, _pi32],
    "sivo_orb_distribute": [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _pi32],
    "sivo_orb_distribute_batch_dev": [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp, _i],
    "sivo_hamming_matrix_dev": [_vp, _i, _vp, _i, _vp, _vp],
    "sivo_hamming_matrix": [_vp, _i, _vp, _i, _vp],
    "sivo_hamming_argmin2_dev": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "sivo_hamming_argmin2": [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    "sivo_hamming_bruteforce_dev": [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp],
    "sivo_mframe_create": [_vp, _i, _vp, _vp, _f, _f, _f, _f, _vp, _vp, _vp, _i, _i, C.POINTER(_vp)],
    "sivo_mframe_destroy": [_vp],
    "sivo_mframe_slab_bytes": [_vp, C.POINTER(_i64)],
    "sivo_mframe_features_in_area": [_vp, _f, _f, _f, _i, _i, _vp, _i, _pi32],
    "sivo_search": [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _pi32, _pi32],
    "sivo_search_by_projection_mappoints": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp, _pi32],
    "sivo_search_by_projection_frame": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _i, _f, _i, _vp, _vp, _pi32],
    "sivo_search_by_projection_reloc": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _i, _vp, _vp, _pi32],
    "sivo_search_by_projection_kf": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _pi32],
    "sivo_fuse": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _vp, _vp, _pi32],
    "sivo_fuse_batch": [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "sivo_search_by_sim3_dir": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp],
    "sivo_search_by_bow_kf_frame": [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _f, _i, _vp, _pi32],
    "sivo_search_by_bow_kf_kf": [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _f, _i, _vp, _pi32],
    "sivo_search_for_triangulation": [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _f, _f, _i, _i, _vp, _pi32],
    "sivo_stereo_match": [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _f, _f, _vp, _vp, _vp],
    "sivo_stereo_match_begin": [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _f, _f, _vp, _vp, _vp, _vp],
    "sivo_stereo_match_cull": [_i, _vp, _vp, _vp, _vp],
    "sivo_entropy_gate_dev": [_i, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(_d), _d, _d, _d, _vp, _i, _d, _vp, _vp, _vp, _vp],
    "sivo_entropy_gate_map_dev": [_i, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(_d), _d, _d, _d, _vp, _i, _d, _vp, _vp, _vp],
    "sivo_entropy_gate": [_i, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(_d), _d, _d, _d, _vp, _i, _d, _vp, _vp, _vp],
    "sivo_check_semantics_dev": [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(_d), _d, _d, _d, _vp, _i, _d, _d, _vp, _vp, _vp, _vp],
    "sivo_check_semantics": [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(_d), _d, _d, _d, _vp, _i, _d, _d, _vp, _vp, _vp],
    "sivo_ba_optimize": [_vp, _vp, _i, _vp, _i, _vp, _i64, C.POINTER(_d), _d, _d, _vp, _vp, _i, _vp, _vp, _vp, C.POINTER(_i), C.POINTER(_i)],
    "sivo_local_ba": [_vp, _vp, _i, _vp, _i, _vp, _i64, C.POINTER(_d), _vp, _vp, _i, _vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)],
    "sivo_ba_optimize_opts": [_vp, _vp, _i, _vp, _i, _vp, _i64, C.POINTER(_d), _d, _d, _vp, _vp, _i, _vp, _vp, _vp, C.POINTER(_i), C.POINTER(_i), _vp],
    "sivo_local_ba_opts": [_vp, _vp, _i, _vp, _i, _vp, _i64, C.POINTER(_d), _vp, _vp, _i, _vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _vp],
    "sivo_ba_analyze": [_vp, _i, _i, _vp, _i64, _vp, _vp],
    "sivo_pose_optimize": [_vp, _vp, _i, _vp, _i64, C.POINTER(_d), _vp, _vp, _vp, C.POINTER(_i), _vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)],
    "sivo_sim3_optimize": [_vp, C.POINTER(_d), C.POINTER(_d), _vp, _i, _f, _i, _vp, C.POINTER(_i), _vp, _vp, C.POINTER(_i), C.POINTER(_i)],
    "sivo_sim3_optimize_batch": [_vp, _i],
    "sivo_sim3_ransac_batch": [_vp, _i],
    "sivo_sim3_ransac": [_vp],
    "sivo_pnp_ransac_batch": [_vp, _i],
    "sivo_pnp_ransac": [_vp],
    "sivo_triangulate_batch": [_vp, _i],
    "sivo_triangulate": [_vp],
    "sivo_mappoint_refresh": [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "sivo_frustum_cull": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _pi32],
    "sivo_frustum_cull_dev": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "sivo_search_local_points": [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _pi32, _pi32],
    "sivo_covis_count": [_vp, _i, _vp, _vp, _vp, _vp],
    "sivo_keyframe_culling": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp],
    "sivo_mappoint_culling": [_i, _vp, _vp, _vp, _vp, _vp, _i64, _i, _vp],
    "sivo_localmap_create": [_vp, C.POINTER(_vp)],
    "sivo_localmap_replace": [_vp, _vp],
    "sivo_localmap_set_bad": [_vp, _i, _vp, _vp, _i, _vp, _vp],
    "sivo_localmap_destroy": [_vp],
    "sivo_localmap_apply": [_vp, _vp],
    "sivo_localmap_sizes": [_vp, _vp],
    "sivo_localmap_export": [_vp, _vp],
    "sivo_localmap_update": [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp],
    "sivo_localmap_set_points": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "sivo_localmap_get_points": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "sivo_localmap_search_local_points": [_vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _f, _f, _vp, _vp, _i, _vp, _vp, _vp, _i,
                                          _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _pi32, _pi32],
    "sivo_localmap_ba_window": [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _i64, _vp, _vp, _vp],
    "sivo_voc_create_from_text": [C.c_char_p, C.POINTER(_vp)],
    "sivo_voc_create": [_i, _i, _i64, _vp, _vp, _vp, _vp, C.POINTER(_vp)],
    "sivo_voc_info": [_vp, _pi32, _pi32, C.POINTER(_i64), C.POINTER(_i64)],
    "sivo_voc_destroy": [_vp],
    "sivo_bow_transform": [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _pi32, _vp, _vp, _vp, _pi32],
    "sivo_bow_transform_batch": [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "sivo_bowdb_create": [_vp, C.POINTER(_vp)],
    "sivo_bowdb_add": [_vp, _vp, _vp, _i, _pi32],
    "sivo_bowdb_erase": [_vp, C.c_int32],
    "sivo_bowdb_clear": [_vp],
    "sivo_bowdb_destroy": [_vp],
    "sivo_bowdb_size": [_vp, _pi32],
    "sivo_bowdb_query": [_vp, _vp, _vp, _i, _vp, _vp, _vp, _pi32],
    "sivo_essential_graph_optimize": [_vp, _vp, _i, _vp, _i, _i, _i, _vp, C.POINTER(_i), C.POINTER(_i)],
    "sivo_essential_graph_analyze": [_vp, _i, _vp, _i, _vp],
    "sivo_sim3_correct_points": [_vp, _vp, _i, _vp, _vp, _i, _vp],
    "sivo_loop_correct": [_vp],
    "sivo_gba_propagate": [_vp],
    "sivo_ba_linearize_dev": [_vp, _vp, _vp, _i64, C.POINTER(_d), _d, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "sivo_ba_linearize": [_vp, _i, _vp, _i, _vp, _i64, C.POINTER(_d), _d, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
}

# test / diagnostic entry points (include/sivo_hip_debug.h): libsivo_hip_dbg.so, a thin library over the product's kernels
DEBUG_SIGNATURES = {
    "sivo_debug_conv": [_i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_d)],
    "sivo_debug_h3_gemm": [_i, _i, _i, _vp, _vp, _f, _vp, _i, C.POINTER(_d)],
    "sivo_debug_conv3_h3_dev": [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _f, _vp, _i, C.POINTER(_d), C.POINTER(_i)],
    "sivo_debug_conv3_h3_pk_dev": [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _f, _f, _i, _vp, _i, C.POINTER(_d), C.POINTER(_i)],
    "sivo_debug_lds_claims": [_vp, _i],
    "sivo_debug_conv_cls_h3_dev": [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _i, C.POINTER(_d)],
    "sivo_debug_local_ba_budget": [_vp, _vp, _i, _vp, _i, _vp, _i64, C.POINTER(_d), _vp, _vp, _i, _vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _i, _i, _vp],
}
DBG_PATH = os.path.join(_HERE, "libsivo_hip_dbg.so")

DIAG_PATH = os.path.join(_HERE, "libsivo_hip_diag.so")

_libs = {}            # "product" / "diag" -> CDLL
_tls = threading.local()
_current = "product"
_dbg = None


def dbg():
    """The sivo_debug_* entry points the kernel tests and tools call: libsivo_hip_dbg.so (`make -C sivo_amd/csrc dbg`), a thin library
    that links libsivo_hip.so (loaded first, so that both share one copy) and runs the PRODUCT's kernels — or, inside
    `with use("diag")`, the diagnostic build itself, which carries the same entry points."""
    global _dbg
    if _current == "diag":
        L = lib()
        if not getattr(L, "_sivo_debug_bound", False):
            for name, args in DEBUG_SIGNATURES.items():
                fn = getattr(L, name)
                fn.argtypes = args
                fn.restype = C.c_int
            L._sivo_debug_bound = True
        return L
    if _dbg is None:
        lib()
        if not os.path.exists(DBG_PATH):
            raise ImportError(f"{DBG_PATH} is missing: make -C sivo_amd/csrc dbg")
        L = C.CDLL(DBG_PATH)
        for name, args in DEBUG_SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = C.c_int
        _dbg = L
    return _dbg


def _load(path):
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build the HIP extension first (make -C sivo_amd/csrc all); "
                          "sivo_amd has no CPU fallback")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64.  Loaded first, libsivo_hip.so
    # (linked against the same sonames) binds to that copy; loaded after /opt/rocm's, torch finds no device
    # ("No HIP GPUs are available", seen when a test touched this library before anything had imported torch).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    L.sivo_last_error.restype = C.c_char_p

    def note(result, func, args, L=L):      # every call remembers the library it went into: check() reads THAT library's error text
        _tls.last = L
        return result
    for name, args in SIGNATURES.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = C.c_int
        fn.errcheck = note
    return L


def lib():
    """The library the calling code should use: libsivo_hip.so (build it with `python -c 'import __graft_entry__ as g; g.build()'`),
    or — inside a `with use("diag")` block — libsivo_hip_diag.so, the same sources compiled with -DSIVO_DIAG: the only build that
    reads the A/B / fault-injection switches (SIVO_NO_FUSE_*, SIVO_D3_FORM, SIVO_H3_BOOST, SIVO_MULTI_EMULATE, ...; the product
    reads eight documented ones).  Every handle-owning object (BayesianSegNet, ORBextractor, MatchFrame) keeps the library it was created
    in (`._L`): its methods, the functions that take it as an argument, its error text and its destructor go there, whatever the current
    context is — a handle never crosses into a library with other statics or a -DSIVO_DIAG struct layout."""
    if _current not in _libs:
        _libs[_current] = _load(LIB_PATH if _current == "product" else DIAG_PATH)
    return _libs[_current]


class use:
    """Context manager: `with _lib.use("diag"):` makes lib() return the diagnostic build inside the block (tests that compare kernel
    forms bit for bit, force the fp16 overflow path or emulate several devices on one)."""

    def __init__(self, which):
        assert which in ("product", "diag")
        self.which = which

    def __enter__(self):
        global _current
        self.prev, _current = _current, self.which
        return lib()

    def __exit__(self, *exc):
        global _current
        _current = self.prev
        return False


def check(rc):
    """The error text comes from the library the failing call went into (this thread's last call: product or diagnostic build)."""
    if rc == OK:
        return
    L = getattr(_tls, "last", None) or lib()
    if rc == ERR_INVALID_ARGUMENT:      # the reference throws std::invalid_argument there
        raise SivoInvalidArgument(rc, L.sivo_last_error().decode(errors="replace"))
    raise SivoError(rc, L.sivo_last_error().decode(errors="replace"))


def require_gpu():
    if lib().sivo_device_count() < 1:
        raise SivoError(ERR_RUNTIME, "no HIP device visible: sivo_amd has no CPU fallback")
