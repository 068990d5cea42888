"""ctypes binding of libfmpnp.so (include/fmpnp.h).

The library is the only compute path of this package: if it is missing, or no
gfx950 device is visible, every entry point raises -- there is no CPU fallback.
torch is imported first so that the process has exactly one HIP runtime
(libamdhip64.so.7 is shared by SONAME with torch's bundled copy).
"""
import ctypes
import os

import torch  # noqa: F401  (load torch's HIP runtime before libfmpnp)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FMPNP_LIB_PATH") or os.path.join(HERE, "lib", "libfmpnp.so")  # override: A/B builds

# enums / constants (include/fmpnp.h)
SQUARED, HUBER, CAUCHY, GEMAN_MCCLURE, BARRON = 0, 1, 2, 3, 4
NEAREST, BILINEAR = 0, 1
LAYOUT_FGRAD, LAYOUT_F = 0, 1
F32, F64 = 0, 1
F16 = 2  # opt-in binary16 storage of the packed map and fref (include/fmpnp.h)
MODE_FORWARD, MODE_COMPUTE_COST = 0, 1
STATUS_OK, STATUS_NO_SUPPORT, STATUS_NAN, STATUS_NO_SUPPORT_TRIAL, STATUS_SYNC_TIMEOUT = 0, 1, 2, 4, 8
STATUS_HELPER_WAIT = 16  # informational: a first-evaluation helper did not publish in time (results unaffected)
STATUS_WINDOW = 32  # a point left its packed window (fmpnp_pack_features_f_window_batch): result invalid, re-run
ABI_VERSION = 4
# LM kernel builds and variants (fmpnp_launch_info)
BUILD_WIDE, BUILD_LATENCY, BUILD_THROUGHPUT = 1, 2, 4
BUILD_NAMES = {BUILD_WIDE: "wide", BUILD_LATENCY: "latency", BUILD_THROUGHPUT: "throughput"}
VARIANT_NAMES = ["NEAREST", "GM", "BILINEAR", "F_NEAREST", "F_GM", "BIL_DIRECT", "GM_SPEC", "NEAREST_SPEC",
                 "GM_SPEC_H", "NEAREST_SPEC_H", "GM_H", "NEAREST_H", "GM_SPEC_512", "GM_SPEC_H_512", "GM_W", "NEAREST_W",
                 "GM_H_W", "NEAREST_H_W"]
ERRORS = {-1: "EINVAL", -2: "EALIGN", -3: "ENOMEM", -4: "ETOOBIG", -5: "ENODEV", -6: "ERANGE"}
# per-problem status bits of the P3P RANSAC + polish stage (fmpnp_pnp_result.status)
PNP_OK, PNP_TOO_FEW, PNP_NO_MODEL, PNP_POLISH_FAILED = 0, 1, 2, 4
# flags of the hypercolumn assembly (fmpnp_hypercolumn_assemble)
HC_NORMALIZE, HC_DWORD_STORES, HC_VECTOR_STORES = 1, 2, 4
# how fmpnp_hypercolumn_sparse reads its points
HC_AT_TEXEL, HC_AT_REFERENCE, HC_AT_CELL = 0, 1, 2
# flags of the encoder's convolution (fmpnp_conv3x3)
CONV_BIAS, CONV_RELU = 1, 2
# flag of the dense features' pyramid step (fmpnp_dense_pyramid_step)
PYR_NORMALIZE = 1
# modes and flag of the image front end's value transforms (fmpnp_image_to_tensor)
IMAGE_TORCH, IMAGE_CAFFE, IMAGE_RAW, IMAGE_GRAY = 0, 1, 2, 3
IMAGE_SWAP_RB = 1
# retrieval (fmpnp_netvlad_pool, fmpnp_rank_topn): the aggregation's segment length, the measured bound of
# the shared exponential in ulp, and the largest n of the top-n selection
NETVLAD_SEGMENT, NETVLAD_EXP_MAX_ULP, RANK_TOPN_CAP = 256, 1.011, 1024
ETOOBIG = -4
EINVAL = -1
ERANGE = -6  # fmpnp_feature_pnp: a reference inlier outside the reference map (IndexError)


class Options(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("n_iters", ctypes.c_int), ("lambda0", ctypes.c_double),
                ("use_ratio", ctypes.c_int), ("ratio_threshold", ctypes.c_double), ("loss", ctypes.c_int),
                ("barron_alpha", ctypes.c_double), ("sampling", ctypes.c_int), ("dtype", ctypes.c_int),
                ("wgs_per_problem", ctypes.c_int), ("max_teams", ctypes.c_int), ("no_memo", ctypes.c_int),
                ("layout", ctypes.c_int), ("sobel_flags", ctypes.c_int), ("helpers", ctypes.c_int)]


class Problem(ctypes.Structure):
    _fields_ = [("feat", ctypes.c_void_p), ("fref", ctypes.c_void_p), ("pts3d", ctypes.c_void_p),
                ("Hf", ctypes.c_int), ("Wf", ctypes.c_int), ("cstride", ctypes.c_int), ("c_begin", ctypes.c_int),
                ("c_end", ctypes.c_int), ("ld_ref", ctypes.c_int), ("N", ctypes.c_int),
                ("im_width", ctypes.c_int), ("im_height", ctypes.c_int),
                ("K", ctypes.c_double * 9), ("R0", ctypes.c_double * 9), ("t0", ctypes.c_double * 3),
                ("window", ctypes.c_void_p)]


class Level(ctypes.Structure):
    _fields_ = [("c_begin", ctypes.c_int), ("c_end", ctypes.c_int)]


class Result(ctypes.Structure):
    _fields_ = [("R", ctypes.c_double * 9), ("t", ctypes.c_double * 3), ("initial_cost", ctypes.c_double),
                ("best_cost", ctypes.c_double), ("final_lambda", ctypes.c_double), ("final_lr", ctypes.c_double),
                ("best_num_inliers", ctypes.c_int), ("n_evals", ctypes.c_int), ("n_steps", ctypes.c_int),
                ("n_accepted", ctypes.c_int), ("status", ctypes.c_int), ("has_best", ctypes.c_int),
                ("texel_gathers", ctypes.c_longlong)]


class TraceEntry(ctypes.Structure):
    _fields_ = [("R", ctypes.c_double * 9), ("t", ctypes.c_double * 3), ("cost", ctypes.c_double),
                ("lambda_after", ctypes.c_double), ("lr_after", ctypes.c_double), ("n_supported", ctypes.c_int),
                ("n_kept", ctypes.c_int), ("accepted", ctypes.c_int)]


class PnpProblem(ctypes.Structure):
    _fields_ = [("points3d", ctypes.c_void_p), ("points2d", ctypes.c_void_p), ("K", ctypes.c_double * 9),
                ("dist", ctypes.c_double * 4), ("threshold", ctypes.c_double), ("seed", ctypes.c_ulonglong),
                ("mask_offset", ctypes.c_longlong), ("M", ctypes.c_int), ("iters", ctypes.c_int),
                ("n_dist", ctypes.c_int), ("reserved", ctypes.c_int)]


class PnpResult(ctypes.Structure):
    _fields_ = [("R", ctypes.c_double * 9), ("t", ctypes.c_double * 3), ("R_hyp", ctypes.c_double * 9),
                ("t_hyp", ctypes.c_double * 3), ("cost", ctypes.c_double), ("num_inliers", ctypes.c_int),
                ("best_h", ctypes.c_int), ("status", ctypes.c_int), ("polish_iters", ctypes.c_int)]


# the SuperPoint baseline (fmpnp/superpoint.py): the detector's cell, SuperPointFrontend.border_remove, the
# largest nms_dist and the most keypoints an image may keep
SP_CELL, SP_BORDER, SP_MAX_NMS_DIST, SP_MAX_KEYPOINTS = 8, 4, 16, 65536


# the localisation chain's glue (fmpnp/localize.py): the best pair's kind (fmpnp_loc_record.kind)
LOC_NONE, LOC_SOLVED, LOC_FALLBACK = 0, 1, 2


class LocPair(ctypes.Structure):
    _fields_ = [("points3d", ctypes.c_void_p), ("points2d", ctypes.c_void_p), ("K", ctypes.c_double * 9),
                ("dist", ctypes.c_double * 4), ("fallback_R", ctypes.c_double * 9), ("fallback_t", ctypes.c_double * 3),
                ("row_offset", ctypes.c_longlong), ("image_shape", ctypes.c_float * 2), ("dim", ctypes.c_int * 2),
                ("n_rows", ctypes.c_int), ("has_fallback", ctypes.c_int)]


class LocQuery(ctypes.Structure):
    _fields_ = [("out_offset", ctypes.c_longlong), ("pair_begin", ctypes.c_int), ("pair_count", ctypes.c_int),
                ("out_cap", ctypes.c_int), ("reserved", ctypes.c_int)]


class LocParams(ctypes.Structure):
    _fields_ = [("threshold", ctypes.c_double), ("seed", ctypes.c_ulonglong), ("iters", ctypes.c_int),
                ("minimum_matches", ctypes.c_int), ("minimum_inliers", ctypes.c_int), ("return_masked", ctypes.c_int)]


class LocMatches(ctypes.Structure):
    _fields_ = [("query2d_f32", ctypes.c_void_p), ("query2d", ctypes.c_void_p), ("points3d", ctypes.c_void_p),
                ("ref2d", ctypes.c_void_p), ("src_row", ctypes.c_void_p), ("counts", ctypes.c_void_p)]


class LocRecord(ctypes.Structure):
    _fields_ = [("R0", ctypes.c_double * 9), ("t0", ctypes.c_double * 3), ("best", ctypes.c_int),
                ("kind", ctypes.c_int), ("num_matches", ctypes.c_int), ("num_inliers", ctypes.c_int),
                ("N", ctypes.c_int), ("reserved", ctypes.c_int)]


class LocSource(ctypes.Structure):
    _fields_ = [("dense_chw", ctypes.c_void_p), ("sparse", ctypes.c_void_p), ("cell0", ctypes.c_double),
                ("cell1", ctypes.c_double), ("D1", ctypes.c_int), ("D2", ctypes.c_int), ("ld_sparse", ctypes.c_int),
                ("reserved", ctypes.c_int)]


class LocBest(ctypes.Structure):
    _fields_ = [("pts3d", ctypes.c_void_p), ("ref2d", ctypes.c_void_p), ("query2d", ctypes.c_void_p),
                ("idx", ctypes.c_void_p), ("records", ctypes.c_void_p)]


# the chain's batched refinement stage (fmpnp_localize_refine_async / fmpnp_localize_refined)
LOC_K_LAST, LOC_K_BEST, LOC_REFINE_MAX_LEVELS = 0, 1, 32


class LocRefineSource(ctypes.Structure):
    _fields_ = [("ref_chw", ctypes.c_void_p), ("dtype", ctypes.c_int), ("H_ref", ctypes.c_int), ("W_ref", ctypes.c_int),
                ("reserved", ctypes.c_int)]


class LocRefineMap(ctypes.Structure):
    _fields_ = [("feat", ctypes.c_void_p), ("Hf", ctypes.c_int), ("Wf", ctypes.c_int)]


class LocRefineParams(ctypes.Structure):
    _fields_ = [("C", ctypes.c_int), ("cstride", ctypes.c_int), ("img0", ctypes.c_int), ("img1", ctypes.c_int),
                ("intrinsics", ctypes.c_int), ("n_levels", ctypes.c_int), ("levels", ctypes.POINTER(Level))]


class LocRefineBuffers(ctypes.Structure):
    _fields_ = [("probs", ctypes.c_void_p), ("fref", ctypes.c_void_p), ("cost", ctypes.c_void_p),
                ("supported", ctypes.c_void_p), ("results", ctypes.c_void_p), ("flags", ctypes.c_void_p)]


class HcLayer(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("reserved", ctypes.c_int), ("stride_b", ctypes.c_longlong), ("stride_c", ctypes.c_longlong),
                ("stride_y", ctypes.c_longlong)]


class LocQueryLayers(ctypes.Structure):  # fmpnp_loc_query_layers
    _fields_ = [("layers", ctypes.POINTER(HcLayer)), ("L", ctypes.c_int), ("B", ctypes.c_int), ("item", ctypes.c_int),
                ("H", ctypes.c_int), ("W", ctypes.c_int), ("flags", ctypes.c_int)]


class LaunchInfo(ctypes.Structure):
    _fields_ = [("teams", ctypes.c_int), ("wgs_per_problem", ctypes.c_int), ("grid", ctypes.c_int),
                ("lds_bytes", ctypes.c_int), ("build", ctypes.c_int), ("variant", ctypes.c_int),
                ("team", ctypes.c_int), ("ratio", ctypes.c_int), ("dtype", ctypes.c_int), ("helpers", ctypes.c_int),
                ("speculate", ctypes.c_int)]


EXPORTS = ["fmpnp_abi_version", "fmpnp_build_info", "fmpnp_device_check", "fmpnp_pack_features",
           "fmpnp_gather_reference", "fmpnp_gather_reference_async", "fmpnp_pack_features_batch", "fmpnp_pack_features_f",
           "fmpnp_gather_reference_batch", "fmpnp_workspace_size", "fmpnp_refine_batch_async", "fmpnp_refine_batch",
           "fmpnp_last_launch", "fmpnp_debug_stamps", "fmpnp_plan", "fmpnp_last_launch_info",
           "fmpnp_pack_features_f_window_batch", "fmpnp_feature_pnp", "fmpnp_compute_cost_async",
           "fmpnp_feature_pnp_reruns", "fmpnp_refine_batch_cpu", "fmpnp_match_workspace_size",
           "fmpnp_exhaustive_match_async", "fmpnp_exhaustive_match", "fmpnp_exhaustive_match_cpu",
           "fmpnp_gather_sparse_descriptors", "fmpnp_correlation_async", "fmpnp_pnp_workspace_size",
           "fmpnp_pnp_ransac_async", "fmpnp_pnp_ransac", "fmpnp_pnp_ransac_cpu", "fmpnp_p3p_cpu",
           "fmpnp_hypercolumn_assemble_async", "fmpnp_hypercolumn_assemble", "fmpnp_hypercolumn_assemble_cpu",
           "fmpnp_netvlad_workspace_size", "fmpnp_netvlad_pool_async", "fmpnp_netvlad_pool", "fmpnp_netvlad_pool_cpu",
           "fmpnp_rank_topn_async", "fmpnp_rank_topn", "fmpnp_rank_topn_cpu", "fmpnp_localize_workspace_size",
           "fmpnp_localize_async", "fmpnp_localize", "fmpnp_localize_build_cpu", "fmpnp_localize_pick_cpu",
           "fmpnp_sp_heatmap_async", "fmpnp_sp_heatmap", "fmpnp_sp_heatmap_cpu", "fmpnp_sp_nms_capacity",
           "fmpnp_sp_nms_workspace_size", "fmpnp_sp_nms_async", "fmpnp_sp_nms", "fmpnp_sp_nms_cpu",
           "fmpnp_sp_describe_async", "fmpnp_sp_describe", "fmpnp_sp_describe_cpu", "fmpnp_sp_match_async",
           "fmpnp_sp_match", "fmpnp_sp_match_cpu", "fmpnp_sp_assemble_async", "fmpnp_sp_assemble",
           "fmpnp_sp_assemble_cpu", "fmpnp_match_workspace_size_ex", "fmpnp_exhaustive_match_ex_async",
           "fmpnp_correlation_ex_async", "fmpnp_exhaustive_match_ex", "fmpnp_exhaustive_match_ex_cpu",
           "fmpnp_localize_ex", "fmpnp_hypercolumn_sparse_async", "fmpnp_hypercolumn_sparse",
           "fmpnp_hypercolumn_sparse_cpu", "fmpnp_feature_pnp_layers", "fmpnp_hypercolumn_pack_workspace_size",
           "fmpnp_hypercolumn_pack_async", "fmpnp_hypercolumn_pack", "fmpnp_hypercolumn_pack_cpu",
           "fmpnp_feature_pnp_query_layers", "fmpnp_localize_refine_workspace_size", "fmpnp_localize_refine_async",
           "fmpnp_localize_refined", "fmpnp_localize_refine_prep_cpu", "fmpnp_conv3x3_async", "fmpnp_conv3x3",
           "fmpnp_conv3x3_cpu", "fmpnp_relu_async", "fmpnp_relu_cpu", "fmpnp_maxpool2x2_async", "fmpnp_maxpool2x2",
           "fmpnp_maxpool2x2_cpu", "fmpnp_conv3x3_f16_weights_size", "fmpnp_conv3x3_pack_weights_f16_async",
           "fmpnp_conv3x3_pack_weights_f16_cpu", "fmpnp_conv3x3_f16_async", "fmpnp_conv3x3_f16", "fmpnp_conv3x3_f16_cpu",
           "fmpnp_match_layers_workspace_size", "fmpnp_exhaustive_match_layers_async", "fmpnp_correlation_layers_async",
           "fmpnp_exhaustive_match_layers", "fmpnp_exhaustive_match_layers_cpu", "fmpnp_localize_layers",
           "fmpnp_conv1x1_async", "fmpnp_conv1x1", "fmpnp_conv1x1_cpu", "fmpnp_conv3x3_dilated_async",
           "fmpnp_conv3x3_dilated", "fmpnp_conv3x3_dilated_cpu", "fmpnp_avgpool2x2s1_async", "fmpnp_avgpool2x2s1",
           "fmpnp_avgpool2x2s1_cpu", "fmpnp_dense_pyramid_step_async", "fmpnp_dense_pyramid_step",
           "fmpnp_dense_pyramid_step_cpu", "fmpnp_image_resize_u8_async", "fmpnp_image_resize_u8",
           "fmpnp_image_resize_u8_cpu", "fmpnp_image_to_tensor_async", "fmpnp_image_to_tensor",
           "fmpnp_image_to_tensor_cpu"]

# fmpnp_match_precision
MATCH_F32, MATCH_F16 = 0, 1
MATCH_PRECISIONS = {"f32": MATCH_F32, "f16": MATCH_F16}


def match_precision(name):
    """"f32" / "f16" -> fmpnp_match_precision; anything else is a ValueError."""
    if not isinstance(name, str) or name not in MATCH_PRECISIONS:
        raise ValueError(f'precision must be "f32" or "f16", not {name!r}')
    return MATCH_PRECISIONS[name]

_LIB = None


class FmpnpError(RuntimeError):
    pass


def load():
    """Load libfmpnp.so (no device needed to load it)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise FmpnpError(f"libfmpnp.so not built ({LIB_PATH}); run `python -c 'import __graft_entry__ as g; "
                         f"g.build()'` or `make -C featuremetric-pnp_amd`")
    L = ctypes.CDLL(LIB_PATH)
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.fmpnp_abi_version.restype = i
    L.fmpnp_build_info.restype = ctypes.c_char_p
    L.fmpnp_device_check.argtypes = [i]
    L.fmpnp_device_check.restype = i
    L.fmpnp_pack_features.argtypes = [vp, vp, vp, i, i, i, i, vp, i, i, i, i, vp]
    L.fmpnp_pack_features.restype = i
    L.fmpnp_gather_reference.argtypes = [vp, i, i, i, i, vp, i, i, i, vp, i, i, vp]
    L.fmpnp_gather_reference.restype = i
    L.fmpnp_gather_reference_async.argtypes = [vp, i, i, i, i, vp, i, i, i, vp, i, i, vp, vp]
    L.fmpnp_gather_reference_async.restype = i
    L.fmpnp_pack_features_batch.argtypes = [i, vp, vp, vp, i, i, i, i, i, vp]
    L.fmpnp_pack_features_f.argtypes = [vp, i, i, i, i, vp, i, i, vp]
    L.fmpnp_pack_features_f.restype = i
    L.fmpnp_pack_features_batch.restype = i
    L.fmpnp_gather_reference_batch.argtypes = [i, vp, vp, vp, vp, i, i, vp, vp, i, i, vp, vp]
    L.fmpnp_gather_reference_batch.restype = i
    L.fmpnp_pack_features_f_window_batch.argtypes = [vp, vp, i, vp, i, i, vp]
    L.fmpnp_pack_features_f_window_batch.restype = i
    L.fmpnp_point_costs.argtypes = [ctypes.POINTER(Problem), i, i, vp, vp, vp]
    L.fmpnp_point_costs.restype = i
    L.fmpnp_workspace_size.argtypes = [ctypes.POINTER(Problem), i, ctypes.POINTER(Options)]
    L.fmpnp_workspace_size.restype = ctypes.c_size_t
    L.fmpnp_refine_batch_async.argtypes = [vp, ctypes.POINTER(Problem), i, i, ctypes.POINTER(Options), vp, vp, i, vp,
                                           ctypes.c_size_t, vp]
    L.fmpnp_refine_batch_async.restype = i
    L.fmpnp_refine_batch.argtypes = [ctypes.POINTER(Problem), i, ctypes.POINTER(Options), ctypes.POINTER(Result),
                                     ctypes.POINTER(TraceEntry), i, vp]
    L.fmpnp_refine_batch.restype = i
    if hasattr(L, "fmpnp_refine_batch_cpu"):  # (A/B builds of earlier sources lack it)
        L.fmpnp_refine_batch_cpu.argtypes = [ctypes.POINTER(Problem), i, ctypes.POINTER(Options),
                                             ctypes.POINTER(Result), ctypes.POINTER(TraceEntry), i, i]
        L.fmpnp_refine_batch_cpu.restype = i
    L.fmpnp_last_launch.argtypes = [ctypes.POINTER(i)] * 4
    L.fmpnp_last_launch.restype = i
    L.fmpnp_plan.argtypes = [ctypes.POINTER(Problem), i, ctypes.POINTER(Options), ctypes.POINTER(LaunchInfo)]
    L.fmpnp_plan.restype = i
    L.fmpnp_last_launch_info.argtypes = [ctypes.POINTER(LaunchInfo)]
    L.fmpnp_last_launch_info.restype = i
    L.fmpnp_compute_cost_async.argtypes = [ctypes.POINTER(Problem), i, i, i, d, vp, vp, vp, vp]
    L.fmpnp_compute_cost_async.restype = i
    dp = ctypes.POINTER(ctypes.c_double)
    L.fmpnp_feature_pnp.argtypes = [vp, i, i, i, i, vp, i, i, i, i, vp, vp, i, dp, dp, dp, i, i,
                                    ctypes.POINTER(Level), i, ctypes.POINTER(Options), i, vp, vp, i, vp]
    L.fmpnp_feature_pnp.restype = i
    if hasattr(L, "fmpnp_feature_pnp_reruns"):  # (A/B builds of earlier sources lack it)
        L.fmpnp_feature_pnp_reruns.restype = ctypes.c_longlong
    # dense exhaustive matching (fmpnp/match.py)
    L.fmpnp_match_workspace_size.argtypes = [i, i]
    L.fmpnp_match_workspace_size.restype = ctypes.c_size_t
    L.fmpnp_exhaustive_match_async.argtypes = [vp, i, i, vp, i, i, i, i, d, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    L.fmpnp_exhaustive_match_async.restype = i
    L.fmpnp_exhaustive_match.argtypes = [vp, i, i, vp, i, i, i, i, d, vp, vp, vp, vp, vp, vp]
    L.fmpnp_exhaustive_match.restype = i
    L.fmpnp_exhaustive_match_cpu.argtypes = [vp, i, i, vp, i, i, i, i, d, vp, vp, vp, vp, vp, i]
    L.fmpnp_exhaustive_match_cpu.restype = i
    L.fmpnp_correlation_async.argtypes = [vp, i, i, vp, i, i, i, vp, vp]
    L.fmpnp_correlation_async.restype = i
    # ... with a precision (fmpnp_match_precision; A/B builds of earlier sources lack them)
    if hasattr(L, "fmpnp_match_workspace_size_ex"):
        L.fmpnp_match_workspace_size_ex.argtypes = [i, i, i, i]
        L.fmpnp_match_workspace_size_ex.restype = ctypes.c_size_t
        L.fmpnp_exhaustive_match_ex_async.argtypes = [vp, i, i, vp, i, i, i, i, d, vp, vp, vp, vp, vp, vp, ctypes.c_size_t,
                                                      i, vp]
        L.fmpnp_exhaustive_match_ex_async.restype = i
        L.fmpnp_correlation_ex_async.argtypes = [vp, i, i, vp, i, i, i, vp, vp, ctypes.c_size_t, i, vp]
        L.fmpnp_correlation_ex_async.restype = i
        L.fmpnp_exhaustive_match_ex.argtypes = [vp, i, i, vp, i, i, i, i, d, vp, vp, vp, vp, vp, i, vp]
        L.fmpnp_exhaustive_match_ex.restype = i
        L.fmpnp_exhaustive_match_ex_cpu.argtypes = [vp, i, i, vp, i, i, i, i, d, vp, vp, vp, vp, vp, i, i]
        L.fmpnp_exhaustive_match_ex_cpu.restype = i
    L.fmpnp_gather_sparse_descriptors.argtypes = [vp, i, i, i, vp, i, d, d, vp, i, vp]
    L.fmpnp_gather_sparse_descriptors.restype = i
    # P3P RANSAC + polish (fmpnp/pnp.py)
    sz = ctypes.c_size_t
    L.fmpnp_pnp_workspace_size.argtypes = [i]
    L.fmpnp_pnp_workspace_size.restype = sz
    L.fmpnp_pnp_ransac_async.argtypes = [vp, ctypes.POINTER(PnpProblem), i, vp, vp, sz, vp, sz, vp]
    L.fmpnp_pnp_ransac_async.restype = i
    L.fmpnp_pnp_ransac.argtypes = [ctypes.POINTER(PnpProblem), i, i, ctypes.POINTER(PnpResult), vp, sz, vp]
    L.fmpnp_pnp_ransac.restype = i
    L.fmpnp_pnp_ransac_cpu.argtypes = [ctypes.POINTER(PnpProblem), i, ctypes.POINTER(PnpResult), vp, sz, i]
    L.fmpnp_pnp_ransac_cpu.restype = i
    L.fmpnp_p3p_cpu.argtypes = [vp, vp, vp, vp]
    L.fmpnp_p3p_cpu.restype = i
    # hypercolumn assembly (fmpnp/hypercolumn.py)
    ll = ctypes.c_longlong
    L.fmpnp_hypercolumn_assemble_async.argtypes = [ctypes.POINTER(HcLayer), i, i, vp, i, i, ll, ll, ll, i, vp]
    L.fmpnp_hypercolumn_assemble_async.restype = i
    L.fmpnp_hypercolumn_assemble.argtypes = [ctypes.POINTER(HcLayer), i, i, vp, i, i, ll, ll, ll, i, vp]
    L.fmpnp_hypercolumn_assemble.restype = i
    L.fmpnp_hypercolumn_assemble_cpu.argtypes = [ctypes.POINTER(HcLayer), i, i, vp, i, i, ll, ll, ll, i, i]
    L.fmpnp_hypercolumn_assemble_cpu.restype = i
    if hasattr(L, "fmpnp_hypercolumn_sparse"):  # (A/B builds of earlier sources lack them)
        sparse = [ctypes.POINTER(HcLayer), i, i, i, i, vp, vp, i, i, d, d, vp, i, ll, i, vp]
        L.fmpnp_hypercolumn_sparse_async.argtypes = sparse + [vp]
        L.fmpnp_hypercolumn_sparse_async.restype = i
        L.fmpnp_hypercolumn_sparse.argtypes = sparse + [vp]
        L.fmpnp_hypercolumn_sparse.restype = i
        L.fmpnp_hypercolumn_sparse_cpu.argtypes = sparse + [i]
        L.fmpnp_hypercolumn_sparse_cpu.restype = i
        L.fmpnp_feature_pnp_layers.argtypes = [vp, i, i, i, i, ctypes.POINTER(HcLayer), i, i, i, i, vp, vp, i, dp, dp, dp,
                                               i, i, ctypes.POINTER(Level), i, ctypes.POINTER(Options), i, vp, vp, i, vp]
        L.fmpnp_feature_pnp_layers.restype = i
    if hasattr(L, "fmpnp_hypercolumn_pack"):  # (A/B builds of earlier sources lack them)
        pack = [ctypes.POINTER(HcLayer), i, i, i, i, i, i, i, i, i, i, i, i, i, vp, vp]
        L.fmpnp_hypercolumn_pack_workspace_size.argtypes = [i, i]
        L.fmpnp_hypercolumn_pack_workspace_size.restype = sz
        L.fmpnp_hypercolumn_pack_async.argtypes = pack + [vp, sz, vp]
        L.fmpnp_hypercolumn_pack_async.restype = i
        L.fmpnp_hypercolumn_pack.argtypes = pack + [vp, sz, vp]
        L.fmpnp_hypercolumn_pack.restype = i
        L.fmpnp_hypercolumn_pack_cpu.argtypes = pack + [i]
        L.fmpnp_hypercolumn_pack_cpu.restype = i
        L.fmpnp_feature_pnp_query_layers.argtypes = [
            ctypes.POINTER(HcLayer), i, i, i, i, vp, i, ctypes.POINTER(HcLayer), i, i, i, i, vp, vp, i, dp, dp, dp, i, i,
            ctypes.POINTER(Level), i, ctypes.POINTER(Options), i, vp, vp, i, vp]
        L.fmpnp_feature_pnp_query_layers.restype = i
    # retrieval (fmpnp/retrieval.py)
    L.fmpnp_netvlad_workspace_size.argtypes = [i, i, i, i]
    L.fmpnp_netvlad_workspace_size.restype = sz
    L.fmpnp_netvlad_pool_async.argtypes = [vp, i, i, i, ll, ll, vp, i, i, vp, i, i, vp, ll, vp, sz, vp]
    L.fmpnp_netvlad_pool_async.restype = i
    L.fmpnp_netvlad_pool.argtypes = [vp, i, i, i, ll, ll, vp, i, i, vp, i, i, vp, ll, vp]
    L.fmpnp_netvlad_pool.restype = i
    L.fmpnp_netvlad_pool_cpu.argtypes = [vp, i, i, i, ll, ll, vp, i, i, vp, i, i, vp, ll, i]
    L.fmpnp_netvlad_pool_cpu.restype = i
    L.fmpnp_rank_topn_async.argtypes = [vp, i, i, vp, i, i, i, i, vp, vp, vp, vp, sz, vp]
    L.fmpnp_rank_topn_async.restype = i
    L.fmpnp_rank_topn.argtypes = [vp, i, i, vp, i, i, i, i, vp, vp, vp, vp]
    L.fmpnp_rank_topn.restype = i
    L.fmpnp_rank_topn_cpu.argtypes = [vp, i, i, vp, i, i, i, i, vp, vp, vp, i]
    L.fmpnp_rank_topn_cpu.restype = i
    # the localisation chain's glue (fmpnp/localize.py)
    P = ctypes.POINTER
    if hasattr(L, "fmpnp_localize"):  # (A/B builds of earlier sources lack it)
        L.fmpnp_localize_workspace_size.argtypes = [i]
        L.fmpnp_localize_workspace_size.restype = sz
        L.fmpnp_localize_async.argtypes = [vp, P(LocPair), i, vp, P(LocQuery), i, P(LocParams), vp, vp, ll, P(LocMatches),
                                           P(LocBest), vp, vp, vp, sz, vp]
        L.fmpnp_localize_async.restype = i
        L.fmpnp_localize.argtypes = [P(LocPair), P(LocSource), i, P(LocQuery), P(vp), P(i), i, i, d, P(LocParams), ll,
                                     P(LocBest), P(LocMatches), vp, vp, vp]
        L.fmpnp_localize.restype = i
        L.fmpnp_localize_build_cpu.argtypes = [P(LocPair), i, P(LocParams), vp, vp, ll, P(LocMatches), P(PnpProblem)]
        L.fmpnp_localize_build_cpu.restype = i
        L.fmpnp_localize_pick_cpu.argtypes = [P(LocPair), i, P(LocQuery), i, P(LocParams), P(PnpResult), vp, ll,
                                              P(LocMatches), P(LocBest)]
        L.fmpnp_localize_pick_cpu.restype = i
    if hasattr(L, "fmpnp_localize_ex"):  # (with the match stage's precision)
        L.fmpnp_localize_ex.argtypes = [P(LocPair), P(LocSource), i, P(LocQuery), P(vp), P(i), i, i, d, P(LocParams), ll,
                                        P(LocBest), P(LocMatches), vp, vp, i, vp]
        L.fmpnp_localize_ex.restype = i
    if hasattr(L, "fmpnp_localize_refined"):  # (the chain's batched refinement stage)
        L.fmpnp_localize_refine_workspace_size.argtypes = [P(LocQuery), i, P(LocRefineMap), P(LocRefineParams), P(Options)]
        L.fmpnp_localize_refine_workspace_size.restype = sz
        L.fmpnp_localize_refine_async.argtypes = [vp, i, vp, P(LocQuery), i, vp, vp, P(LocRefineMap), P(LocRefineParams),
                                                  P(Options), P(LocBest), P(LocRefineBuffers), vp, sz, vp]
        L.fmpnp_localize_refine_async.restype = i
        L.fmpnp_localize_refined.argtypes = [P(LocPair), P(LocSource), i, P(LocQuery), P(vp), P(i), i, i, d, P(LocParams),
                                             ll, P(LocBest), P(LocMatches), vp, vp, i, P(LocRefineSource), P(i),
                                             P(LocRefineParams), P(Options), vp, vp, vp]
        L.fmpnp_localize_refined.restype = i
        L.fmpnp_localize_refine_prep_cpu.argtypes = [P(LocPair), i, P(LocQuery), i, P(LocRefineSource), P(LocRefineMap),
                                                     P(LocRefineParams), i, P(LocBest), P(Problem), vp, vp]
        L.fmpnp_localize_refine_prep_cpu.restype = i
    if hasattr(L, "fmpnp_exhaustive_match_layers"):  # (layered matching; A/B builds of earlier sources lack it)
        lay = [vp, i, i, P(HcLayer), i, i, i, i, i, i]  # sparse, N, ld_sparse, layers, L, B, item, H, W, flags
        L.fmpnp_match_layers_workspace_size.argtypes = [P(HcLayer), i, i, i, i]
        L.fmpnp_match_layers_workspace_size.restype = sz
        L.fmpnp_exhaustive_match_layers_async.argtypes = lay + [i, d, vp, vp, vp, vp, vp, vp, sz, vp]
        L.fmpnp_exhaustive_match_layers_async.restype = i
        L.fmpnp_correlation_layers_async.argtypes = lay + [vp, vp, sz, vp]
        L.fmpnp_correlation_layers_async.restype = i
        L.fmpnp_exhaustive_match_layers.argtypes = lay + [i, d, vp, vp, vp, vp, vp, vp]
        L.fmpnp_exhaustive_match_layers.restype = i
        L.fmpnp_exhaustive_match_layers_cpu.argtypes = lay + [i, d, vp, vp, vp, vp, vp, i]
        L.fmpnp_exhaustive_match_layers_cpu.restype = i
        L.fmpnp_localize_layers.argtypes = [P(LocPair), P(LocSource), i, P(LocQuery), P(LocQueryLayers), P(i), i, i, d,
                                            P(LocParams), ll, P(LocBest), P(LocMatches), vp, vp, vp]
        L.fmpnp_localize_layers.restype = i
    # the SuperPoint baseline (fmpnp/superpoint.py)
    if hasattr(L, "fmpnp_sp_heatmap"):  # (A/B builds of earlier sources lack it)
        L.fmpnp_sp_heatmap_async.argtypes = [vp, i, i, vp, vp]
        L.fmpnp_sp_heatmap.argtypes = [vp, i, i, vp, vp]
        L.fmpnp_sp_heatmap_cpu.argtypes = [vp, i, i, vp]
        L.fmpnp_sp_nms_capacity.argtypes = [i, i, i]
        L.fmpnp_sp_nms_capacity.restype = ll
        L.fmpnp_sp_nms_workspace_size.argtypes = [i, i, i]
        L.fmpnp_sp_nms_workspace_size.restype = sz
        L.fmpnp_sp_nms_async.argtypes = [vp, i, i, d, i, i, vp, ll, vp, i, P(i), P(i), vp, sz, vp]
        L.fmpnp_sp_nms.argtypes = [vp, i, i, d, i, i, vp, ll, i, P(i), P(i), vp]
        L.fmpnp_sp_nms_cpu.argtypes = [vp, i, i, d, i, i, vp, ll, P(i)]
        L.fmpnp_sp_describe_async.argtypes = [vp, i, i, i, vp, ll, i, i, i, i, vp, ll, vp]
        L.fmpnp_sp_describe.argtypes = [vp, i, i, i, vp, ll, i, i, i, i, vp, ll, vp]
        L.fmpnp_sp_describe_cpu.argtypes = [vp, i, i, i, vp, ll, i, i, i, i, vp, ll]
        L.fmpnp_sp_match_async.argtypes = [vp, i, i, vp, i, i, i, d, vp, vp, vp, vp, vp, vp, sz, vp]
        L.fmpnp_sp_match.argtypes = [vp, i, i, vp, i, i, i, d, vp, vp, vp, vp, P(i), vp]
        L.fmpnp_sp_match_cpu.argtypes = [vp, i, i, vp, i, i, i, d, vp, vp, vp, vp, P(i)]
        L.fmpnp_sp_assemble_async.argtypes = [vp, i, ll, vp, i, ll, vp, vp, i, vp, i, vp, vp, vp, vp, vp, vp, sz, vp]
        L.fmpnp_sp_assemble.argtypes = [vp, i, ll, vp, i, ll, vp, vp, i, vp, i, vp, vp, vp, vp, P(i), vp]
        L.fmpnp_sp_assemble_cpu.argtypes = [vp, i, ll, vp, i, ll, vp, vp, i, vp, i, vp, vp, vp, vp, P(i)]
        for name in EXPORTS:
            if name.startswith("fmpnp_sp_") and name not in ("fmpnp_sp_nms_capacity", "fmpnp_sp_nms_workspace_size"):
                getattr(L, name).restype = i
    # the encoder's operators (fmpnp/encoder.py)
    if hasattr(L, "fmpnp_conv3x3"):  # (A/B builds of earlier sources lack them)
        conv = [vp, i, i, i, i, vp, vp, i, i, vp]
        L.fmpnp_conv3x3_async.argtypes = conv + [vp]
        L.fmpnp_conv3x3.argtypes = conv + [vp]
        L.fmpnp_conv3x3_cpu.argtypes = conv + [i]
        L.fmpnp_relu_async.argtypes = [vp, vp, ll, vp]
        L.fmpnp_relu_cpu.argtypes = [vp, vp, ll, i]
        L.fmpnp_maxpool2x2_async.argtypes = [vp, i, i, i, i, vp, vp]
        L.fmpnp_maxpool2x2.argtypes = [vp, i, i, i, i, vp, vp]
        L.fmpnp_maxpool2x2_cpu.argtypes = [vp, i, i, i, i, vp, i]
        for name in EXPORTS:
            if name.startswith(("fmpnp_conv3x3", "fmpnp_relu", "fmpnp_maxpool2x2")) and hasattr(L, name):
                getattr(L, name).restype = i
    if hasattr(L, "fmpnp_conv3x3_f16"):  # (the convolution's fp16 precision: the packed image in the weight's place)
        L.fmpnp_conv3x3_f16_weights_size.argtypes = [i, i]
        L.fmpnp_conv3x3_f16_weights_size.restype = sz
        L.fmpnp_conv3x3_pack_weights_f16_async.argtypes = [vp, i, i, vp, vp]
        L.fmpnp_conv3x3_pack_weights_f16_async.restype = i
        L.fmpnp_conv3x3_pack_weights_f16_cpu.argtypes = [vp, i, i, vp]
        L.fmpnp_conv3x3_pack_weights_f16_cpu.restype = i
        L.fmpnp_conv3x3_f16_async.argtypes = conv + [vp]
        L.fmpnp_conv3x3_f16.argtypes = conv + [vp]
        L.fmpnp_conv3x3_f16_cpu.argtypes = conv + [i]
    if hasattr(L, "fmpnp_conv1x1"):  # (the 1x1 convolution: the 3x3's arguments)
        L.fmpnp_conv1x1_async.argtypes = conv + [vp]
        L.fmpnp_conv1x1.argtypes = conv + [vp]
        L.fmpnp_conv1x1_cpu.argtypes = conv + [i]
        for name in ("fmpnp_conv1x1_async", "fmpnp_conv1x1", "fmpnp_conv1x1_cpu"):
            getattr(L, name).restype = i
    if hasattr(L, "fmpnp_dense_pyramid_step"):  # (dense features: the dilated convolution, the average pool, the step)
        dil = [vp, i, i, i, i, vp, vp, i, i, vp, i]
        L.fmpnp_conv3x3_dilated_async.argtypes = dil + [vp]
        L.fmpnp_conv3x3_dilated.argtypes = dil + [vp]
        L.fmpnp_conv3x3_dilated_cpu.argtypes = dil + [i]
        L.fmpnp_avgpool2x2s1_async.argtypes = [vp, i, i, i, i, vp, vp]
        L.fmpnp_avgpool2x2s1.argtypes = [vp, i, i, i, i, vp, vp]
        L.fmpnp_avgpool2x2s1_cpu.argtypes = [vp, i, i, i, i, vp, i]
        step = [vp, vp, i, i, i, i, i, i, vp, i]
        L.fmpnp_dense_pyramid_step_async.argtypes = step + [vp]
        L.fmpnp_dense_pyramid_step.argtypes = step + [vp]
        L.fmpnp_dense_pyramid_step_cpu.argtypes = step + [i]
        for name in EXPORTS:
            if name.startswith(("fmpnp_avgpool2x2s1", "fmpnp_dense_pyramid_step")):
                getattr(L, name).restype = i
    if hasattr(L, "fmpnp_image_to_tensor"):  # (the image front end: Lanczos resize and the value transforms)
        rs = [vp, ll, ll, i, i, i, i, i, vp]
        tt = [vp, ll, ll, i, i, i, i, i, i, i, vp, vp, vp]
        L.fmpnp_image_resize_u8_async.argtypes = rs + [vp]
        L.fmpnp_image_resize_u8.argtypes = rs + [vp]
        L.fmpnp_image_resize_u8_cpu.argtypes = rs + [i]
        L.fmpnp_image_to_tensor_async.argtypes = tt + [vp]
        L.fmpnp_image_to_tensor.argtypes = tt + [vp]
        L.fmpnp_image_to_tensor_cpu.argtypes = tt + [i]
        for name in EXPORTS:
            if name.startswith("fmpnp_image_"):
                getattr(L, name).restype = i
    if L.fmpnp_abi_version() != ABI_VERSION:
        raise FmpnpError("libfmpnp ABI mismatch")
    _LIB = L
    return L


def check(rc, what):
    if rc != 0:
        name = ERRORS.get(rc, f"hipError {rc}")
        raise FmpnpError(f"{what} failed: {name}")


_DEVICE_OK = {}


def require_device(device):
    """The HIP path needs a gfx950 device; anything else is a hard error."""
    if not torch.cuda.is_available():
        raise FmpnpError("fmpnp needs an AMD MI355X (gfx950) GPU; none is visible (no CPU fallback)")
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    if idx not in _DEVICE_OK:
        rc = load().fmpnp_device_check(idx)
        if rc != 0:
            raise FmpnpError(f"device {idx} is not a gfx950 (fmpnp_device_check -> {rc})")
        _DEVICE_OK[idx] = True
    return idx


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def spec_build():
    """True when libfmpnp.so has the speculative next-texel gathers compiled in (the default;
    a -DFMPNP_SPEC=0 build leaves them out).  Per launch, fmpnp_options.no_memo = 2 turns them off."""
    return b"speculative_gathers=1" in load().fmpnp_build_info()


def _info_dict(info):
    d = {name: getattr(info, name) for name, _ in LaunchInfo._fields_}
    d["build_name"] = BUILD_NAMES.get(info.build, str(info.build))
    d["variant_name"] = VARIANT_NAMES[info.variant] if 0 <= info.variant < len(VARIANT_NAMES) else str(info.variant)
    d["dtype_name"] = {F64: "f64", F16: "f16"}.get(info.dtype, "f32")
    return d


from .build_id import kernel_name, source_digest  # noqa: E402,F401  (profile matching: bench.py)


def library_digest():
    """The source digest compiled into the loaded libfmpnp.so ("unknown" outside the Makefile)."""
    info = load().fmpnp_build_info().decode()
    return info.split("source_digest=", 1)[1].split(";")[0].strip() if "source_digest=" in info else "unknown"


def last_launch():
    """Plan of this thread's last LM launch: geometry, build, kernel variant, helpers."""
    info = LaunchInfo()
    load().fmpnp_last_launch_info(ctypes.byref(info))
    return _info_dict(info)


def plan(descs, n, options):
    """The launch plan (as last_launch()) for n fmpnp_problem descriptors and options, without
    launching (needs the device)."""
    info = LaunchInfo()
    check(load().fmpnp_plan(descs, n, ctypes.byref(options), ctypes.byref(info)), "fmpnp_plan")
    return _info_dict(info)
