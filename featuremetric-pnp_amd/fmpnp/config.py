"""Defaults that the reference binds through gin (featurePnP/model.gin,
input_configs/*.gin: sparseFeaturePnP.*, optimize_feature_pnp.*).

gin is not part of this build; `configure()` sets the same bindings in-process.
"""
from . import losses

_MODEL = dict(n_iters=50, loss_fn=losses.squared_loss, lambda_=0.01, verbose=False, ratio_threshold=None,
              useGPU=True)  # featurePnP/model.gin:1-5
_ADAPTER = dict(image_shape=(1024, 1024), feature_pyramid=None)
# find_inliers.* (featurePnP/model.py:131; input_configs/robotcar_inlier_GN.gin:42 binds 0.8)
_FIND_INLIERS = dict(threshold=None, loss_fn=losses.squared_loss, mode="ratio_max")
# exhaustive_search.* (s2dhm/pose_prediction/exhaustive_search.py:23-29: factor has no default; the
# reference's gins bind 0.006 for RobotCar and 0.12 for CMU)
_EXHAUSTIVE_SEARCH = dict(factor=None)
# solve_pnp.* (s2dhm/pose_prediction/solve_pnp.py:11-23: no defaults; the reference's gins bind threshold 12.0;
# iters = cv2.solvePnPRansac's iterationsCount there, seed = this library's sampler seed)
_SOLVE_PNP = dict(reprojection_threshold=None, minimum_matches=None, minimum_inliers=None, return_masked=None,
                  iters=5000, seed=0)
# compute_ranks.* (s2dhm/image_retrieval/rank_images.py:57-61: use_pca has no default; the reference's
# configs/network/network.gin:22 binds True)
_COMPUTE_RANKS = dict(use_pca=None)
# SuperPointPredictor.* (s2dhm/pose_prediction/superpoint_predictor.py:21-22: no defaults; the reference's
# configs/pose_prediction/superpoint_prediction.gin binds top_N 15, nms_dist 4, conf_thresh 0.005, nn_thresh 0.7,
# ratio 0.9)
_SUPERPOINT = dict(top_N=None, nms_dist=None, conf_thresh=None, nn_thresh=None, ratio=None)


def configure(**kwargs):
    """configure(n_iters=50, loss_fn=..., ratio_threshold=..., image_shape=..., feature_pyramid=...,
    find_inliers_threshold=..., find_inliers_loss_fn=..., find_inliers_mode=...,
    exhaustive_search_factor=..., solve_pnp_reprojection_threshold=..., solve_pnp_minimum_matches=...,
    solve_pnp_minimum_inliers=..., solve_pnp_return_masked=..., solve_pnp_iters=..., solve_pnp_seed=...,
    compute_ranks_use_pca=..., superpoint_top_N=..., superpoint_nms_dist=..., superpoint_conf_thresh=...,
    superpoint_nn_thresh=..., superpoint_ratio=...)."""
    for k, v in kwargs.items():
        if k.startswith("superpoint_"):
            k = k[len("superpoint_"):]
            if k not in _SUPERPOINT:
                raise KeyError(f"SuperPointPredictor has no parameter {k!r}")
            _SUPERPOINT[k] = v
        elif k.startswith("compute_ranks_"):
            k = k[len("compute_ranks_"):]
            if k not in _COMPUTE_RANKS:
                raise KeyError(f"compute_ranks has no parameter {k!r}")
            _COMPUTE_RANKS[k] = v
        elif k.startswith("solve_pnp_"):
            k = k[len("solve_pnp_"):]
            if k not in _SOLVE_PNP:
                raise KeyError(f"solve_pnp has no parameter {k!r}")
            _SOLVE_PNP[k] = v
        elif k.startswith("exhaustive_search_"):
            k = k[len("exhaustive_search_"):]
            if k not in _EXHAUSTIVE_SEARCH:
                raise KeyError(f"exhaustive_search has no parameter {k!r}")
            _EXHAUSTIVE_SEARCH[k] = v
        elif k.startswith("find_inliers_"):
            k = k[len("find_inliers_"):]
            if k not in _FIND_INLIERS:
                raise KeyError(f"find_inliers has no parameter {k!r}")
            if isinstance(v, str) and k == "loss_fn":
                v = losses.by_name(v)
            _FIND_INLIERS[k] = v
        elif k in _ADAPTER:
            _ADAPTER[k] = v
        else:
            if isinstance(v, str) and k == "loss_fn":
                v = losses.by_name(v)
            _MODEL[k] = v


def model_kwargs():
    return dict(_MODEL)


def adapter_kwargs():
    return dict(_ADAPTER)


def find_inliers_kwargs():
    return dict(_FIND_INLIERS)


def exhaustive_search_kwargs():
    return dict(_EXHAUSTIVE_SEARCH)


def solve_pnp_kwargs():
    return dict(_SOLVE_PNP)


def compute_ranks_kwargs():
    return dict(_COMPUTE_RANKS)


def superpoint_kwargs():
    return dict(_SUPERPOINT)
