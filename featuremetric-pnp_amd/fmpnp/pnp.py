"""P3P RANSAC and reprojection polish on the GPU: the initial pose between the matches and feature_pnp
(s2dhm/pose_prediction/solve_pnp.py; called per retrieved reference image by
sparse_to_dense_predictor.py:140-191).

solve_pnp / solve_pnp_multi keep the reference's signature and its Prediction namedtuple and run
libfmpnp's fmpnp_pnp_ransac (include/fmpnp.h states the numeric contract: fp64, a counter-based sampler
keyed on (seed, h), Lambda Twist, an integer-maximum score reduction, a fixed-order polish).
solve_pnp_cpu runs the CPU twin (bit-identical results), an explicit entry point and never a fallback.
Parity with OpenCV's solvePnPRansac is unpinned: cv2 is not importable where this package is built.
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib, config
from .matrix_utils import matrix_quaternion

Prediction = namedtuple(
    "Prediction",
    "success num_matches num_inliers reference_inliers query_inliers points_3d quaternion matrix "
    "reference_filename reference_keypoints inlier_mask")  # solve_pnp.py:7-8

RESULT_FIELDS = ("R", "t", "R_hyp", "t_hyp", "cost", "num_inliers", "best_h", "status", "polish_iters")


def _distortion(d):
    d = np.zeros(4) if d is None else np.asarray(d, np.float64)
    if d.size != 4 or d.ndim > 2:
        raise ValueError(f"distortion_coefficients must be OpenCV's four (k1, k2, p1, p2), got shape {d.shape}")
    return d.reshape(4)


def make_problems(problems):
    """problems: dicts(points3d [M, 3], points2d [M, 2], K, dist, threshold, iters, seed) -> (the
    fmpnp_pnp_problem array with HOST point pointers, the arrays it points into, the mask's size); problem
    i's mask bytes start at the sum of the earlier problems' M."""
    arr = (_lib.PnpProblem * max(len(problems), 1))()
    keep, at = [], 0
    for i, p in enumerate(problems):
        x3 = np.ascontiguousarray(np.asarray(p["points3d"], np.float64).reshape(-1, 3))
        x2 = np.ascontiguousarray(np.asarray(p["points2d"], np.float64).reshape(-1, 2))
        if x3.shape[0] != x2.shape[0]:
            raise ValueError(f"{x3.shape[0]} 3D points for {x2.shape[0]} 2D points")
        K = np.asarray(p["K"], np.float64)
        if K.shape != (3, 3):
            raise ValueError("intrinsics must be 3x3")
        keep += [x3, x2]
        a = arr[i]
        a.points3d, a.points2d = x3.ctypes.data, x2.ctypes.data
        a.K[:] = K.reshape(-1).tolist()
        a.dist[:] = _distortion(p.get("dist")).tolist()
        a.threshold, a.seed, a.mask_offset = float(p["threshold"]), int(p.get("seed", 0)), at
        a.M, a.iters, a.n_dist = x3.shape[0], int(p.get("iters", 5000)), 4
        at += x3.shape[0]
    return arr, keep, at


def _unpack(arr, res, mask, n):
    out = []
    for i in range(n):
        r = res[i]
        d = dict(R=np.array(r.R[:]).reshape(3, 3), t=np.array(r.t[:]), R_hyp=np.array(r.R_hyp[:]).reshape(3, 3),
                 t_hyp=np.array(r.t_hyp[:]), cost=r.cost, num_inliers=r.num_inliers, best_h=r.best_h,
                 status=r.status, polish_iters=r.polish_iters)
        d["mask"] = mask[arr[i].mask_offset:arr[i].mask_offset + arr[i].M].copy()
        out.append(d)
    return out


def ransac(problems, device=None):
    """fmpnp_pnp_ransac on host arrays: all problems in one launch sequence on `device`'s current stream
    (waits for it).  Returns one dict per problem: the fmpnp_pnp_result fields and mask (uint8 [M])."""
    n = len(problems)
    arr, keep, total = make_problems(problems)
    res, mask = (_lib.PnpResult * max(n, 1))(), np.zeros(max(total, 1), np.uint8)
    device = torch.device("cuda" if device is None else device)
    _lib.require_device(device)
    with torch.cuda.device(device):
        rc = _lib.load().fmpnp_pnp_ransac(arr, n, 0, res, mask.ctypes.data, total, _lib.stream_ptr(device))
    _lib.check(rc, "fmpnp_pnp_ransac")
    return _unpack(arr, res, mask, n)


def ransac_cpu(problems, n_threads=0):
    """fmpnp_pnp_ransac_cpu (the CPU twin: the GPU's results bit for bit)."""
    n = len(problems)
    arr, keep, total = make_problems(problems)
    res, mask = (_lib.PnpResult * max(n, 1))(), np.zeros(max(total, 1), np.uint8)
    rc = _lib.load().fmpnp_pnp_ransac_cpu(arr, n, res, mask.ctypes.data, total, int(n_threads))
    _lib.check(rc, "fmpnp_pnp_ransac_cpu")
    return _unpack(arr, res, mask, n)


class AsyncRansac:
    """fmpnp_pnp_ransac_async on the current stream of `device`: points, descriptors, results, mask and
    workspace in device tensors; nothing waits.  results_fill / mask_fill: the bytes the result and mask
    buffers hold before the launch.  read() waits for the stream and returns what ransac() returns."""

    def __init__(self, problems, device="cuda", results_fill=0, mask_fill=0):
        self.n = n = len(problems)
        self.arr, keep, self.total = make_problems(problems)
        self.device = device = torch.device(device)
        _lib.require_device(device)
        self.host = (_lib.PnpProblem * max(n, 1)).from_buffer_copy(self.arr)
        self.points = []
        for i in range(n):
            x3, x2 = (torch.from_numpy(a).to(device) for a in keep[2 * i:2 * i + 2])
            self.points += [x3, x2]
            self.host[i].points3d, self.host[i].points2d = x3.data_ptr() or None, x2.data_ptr() or None
        raw = np.frombuffer(bytes(self.host), np.uint8).copy()
        self.probs = torch.from_numpy(raw).to(device)
        self.results = torch.full((max(n, 1) * ctypes.sizeof(_lib.PnpResult),), results_fill, dtype=torch.uint8,
                                  device=device)
        self.mask = torch.full((max(self.total, 1),), mask_fill, dtype=torch.uint8, device=device)
        self.ws = torch.empty(max(_lib.load().fmpnp_pnp_workspace_size(n), 8) // 8, dtype=torch.int64, device=device)
        self.launch()

    def launch(self):
        """Queue the launch sequence (again) on the current stream of the device."""
        with torch.cuda.device(self.device):
            rc = _lib.load().fmpnp_pnp_ransac_async(
                self.probs.data_ptr(), self.host, self.n, self.results.data_ptr(), self.mask.data_ptr(), self.total,
                self.ws.data_ptr(), self.ws.numel() * 8, _lib.stream_ptr(self.device))
        _lib.check(rc, "fmpnp_pnp_ransac_async")

    def read(self):
        torch.cuda.current_stream(self.device).synchronize()
        res = (_lib.PnpResult * max(self.n, 1)).from_buffer_copy(self.results.cpu().numpy().tobytes())
        return _unpack(self.arr, res, self.mask.cpu().numpy(), self.n)


def p3p_cpu(bearings, points):
    """fmpnp_p3p_cpu: bearings [3, 3] and world points [3, 3] -> the kept solutions (R [n, 3, 3], t [n, 3])."""
    y = np.ascontiguousarray(np.asarray(bearings, np.float64).reshape(3, 3))
    x = np.ascontiguousarray(np.asarray(points, np.float64).reshape(3, 3))
    R, t = np.zeros((4, 3, 3)), np.zeros((4, 3))
    n = _lib.load().fmpnp_p3p_cpu(y.ctypes.data, x.ctypes.data, R.ctypes.data, t.ctypes.data)
    if n < 0:
        _lib.check(n, "fmpnp_p3p_cpu")
    return R[:n], t[:n]


def _bound(name, value):
    if value is None:
        value = config.solve_pnp_kwargs()[name]
    if value is None:
        raise TypeError(f"solve_pnp: {name} is not bound (pass it, or fmpnp.config.configure(solve_pnp_{name}=...))")
    return value


def _no_prediction(num_matches, reference_filename, reference_keypoints):
    return Prediction(success=False, num_matches=num_matches, num_inliers=None, reference_inliers=None,
                      query_inliers=None, points_3d=None, quaternion=None, matrix=None,
                      reference_filename=reference_filename, reference_keypoints=reference_keypoints, inlier_mask=None)


def _solve_many(run, items, intrinsics, distortion_coefficients, reprojection_threshold, minimum_matches,
                minimum_inliers, return_masked, iters, seed):
    """items: (points_2D, points_3D, reference_filename, reference_2D_points, reference_keypoints) per
    reference image; solve_pnp.py:44-111 for each, with one launch sequence for those that have enough matches."""
    threshold = float(_bound("reprojection_threshold", reprojection_threshold))
    minimum_matches = _bound("minimum_matches", minimum_matches)
    minimum_inliers = _bound("minimum_inliers", minimum_inliers)
    return_masked = _bound("return_masked", return_masked)
    iters, seed = int(_bound("iters", iters)), int(_bound("seed", seed))
    dist = _distortion(distortion_coefficients)
    launch = [k for k, it in enumerate(items) if np.asarray(it[0]).shape[0] > minimum_matches]  # :44
    results = run([dict(points3d=items[k][1], points2d=items[k][0], K=intrinsics, dist=dist, threshold=threshold,
                        iters=iters, seed=seed) for k in launch]) if launch else []
    by_item = dict(zip(launch, results))
    out = []
    for k, (points_2D, points_3D, reference_filename, reference_2D_points, reference_keypoints) in enumerate(items):
        points_2D, points_3D = np.asarray(points_2D), np.asarray(points_3D)
        r = by_item.get(k)
        if r is None or r["status"] != _lib.PNP_OK or r["num_inliers"] < minimum_inliers:    # :50-62, :99-111
            out.append(_no_prediction(points_2D.shape[0], reference_filename, reference_keypoints))
            continue
        inliers = np.flatnonzero(r["mask"]).astype(np.int32)  # np.squeeze(inliers): ascending indices
        matrix = np.eye(4)                                    # matrix_from_se3 (matrix_utils.py:76-81)
        matrix[:3, 3] = r["t"]
        matrix[:3, :3] = r["R"]
        quaternion = matrix_quaternion(matrix)
        masked = bool(return_masked)
        out.append(Prediction(
            success=True, num_matches=points_2D.shape[0], num_inliers=len(inliers),
            reference_inliers=(reference_2D_points[inliers] if masked and reference_2D_points is not None
                               else reference_2D_points),
            query_inliers=np.squeeze(points_2D[inliers]) if masked else np.squeeze(points_2D),
            points_3d=points_3D[inliers] if masked else points_3D,
            quaternion=quaternion, matrix=matrix, reference_filename=reference_filename,
            reference_keypoints=reference_keypoints, inlier_mask=inliers))
    return out


def solve_pnp(points_2D, points_3D, intrinsics, distortion_coefficients, reprojection_threshold=None,
              minimum_matches=None, minimum_inliers=None, reference_filename=None, reference_2D_points=None,
              reference_keypoints=None, use_ransac=None, return_masked=None, iters=None, seed=None):
    """solve_pnp (solve_pnp.py:12-111) on the GPU.  use_ransac is accepted and ignored, as the reference's
    body ignores it.  Arguments left None come from fmpnp.config (configure(solve_pnp_...=...))."""
    return _solve_many(ransac, [(points_2D, points_3D, reference_filename, reference_2D_points, reference_keypoints)],
                       intrinsics, distortion_coefficients, reprojection_threshold, minimum_matches, minimum_inliers,
                       return_masked, iters, seed)[0]


def solve_pnp_multi(items, intrinsics, distortion_coefficients, reprojection_threshold=None, minimum_matches=None,
                    minimum_inliers=None, use_ransac=None, return_masked=None, iters=None, seed=None):
    """The top_N reference images of one query (sparse_to_dense_predictor.py:140-191) in one launch sequence.
    items: (points_2D, points_3D, reference_filename, reference_2D_points, reference_keypoints) per reference.
    Returns [Prediction, ...], each equal to solve_pnp's on that reference bit for bit."""
    return _solve_many(ransac, list(items), intrinsics, distortion_coefficients, reprojection_threshold,
                       minimum_matches, minimum_inliers, return_masked, iters, seed)


def solve_pnp_cpu(points_2D, points_3D, intrinsics, distortion_coefficients, reprojection_threshold=None,
                  minimum_matches=None, minimum_inliers=None, reference_filename=None, reference_2D_points=None,
                  reference_keypoints=None, use_ransac=None, return_masked=None, iters=None, seed=None, n_threads=0):
    """solve_pnp through the CPU twin (fmpnp_pnp_ransac_cpu)."""
    return _solve_many(lambda ps: ransac_cpu(ps, n_threads),
                       [(points_2D, points_3D, reference_filename, reference_2D_points, reference_keypoints)],
                       intrinsics, distortion_coefficients, reprojection_threshold, minimum_matches, minimum_inliers,
                       return_masked, iters, seed)[0]
