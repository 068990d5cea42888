"""Seeded scenes and the staged yardstick for the localisation chain's tests (test_localize_cpu.py,
test_gpu_localize.py).

A scene is one query: a ground-truth pose, a random unit-norm query map [C, W, H] and a list of references.
A reference's row is one of three kinds:

    "in"      a 3D point in front of the camera; its descriptor is the query map's column at the cell that
              holds the point's projection, plus noise of 1e-3: it passes the ratio test and its quantised
              match is a PnP inlier (half a cell is 2 px, the threshold 12 px);
    "wrong"   the column of a random other cell plus the same noise: it passes the ratio test and is a PnP
              outlier unless the random cell happens to lie within the threshold;
    "reject"  the normalised sum of two columns: its two best scores are nearly equal, so with top_k = 2
              the ratio test (0.81 d1 >= d2) rejects it.

The smallest shapes at which things can still go wrong: C = 32, a 16 x 16 map, image 64 x 64, threshold
12 px, iters = 256, factor = 2 / 256 (top_k = 2).  The per-reference row counts cross the wave (64) and
workgroup (256) boundaries of the compaction: 1, 63, 64, 65, 257 and 1000.

The yardstick is the staged composition of the public pieces that existed before fmpnp.localize
(exhaustive_search_multi or exhaustive_match_cpu -> numpy masking as sparse_to_dense_predictor.py:161-175
-> solve_pnp_multi or solve_pnp_cpu -> a numpy restatement of :177-191 and predictor.py:51 -> feature_pnp).
"""
import functools

import numpy as np

import pnp_cases as pc

C, W, H = 32, 16, 16
IMAGE = (64, 64)
CELL = 4.0
FACTOR = 2.0 / 256.0
PNP = dict(reprojection_threshold=12.0, minimum_matches=5, minimum_inliers=12, iters=256, seed=0)
K0 = np.array([[60.0, 0.0, 32.0], [0.0, 60.0, 32.0], [0.0, 0.0, 1.0]])
K1 = np.array([[66.0, 0.0, 31.0], [0.0, 63.0, 33.0], [0.0, 0.0, 1.0]])  # "differing intrinsics"
ROW_COUNTS = (1, 63, 64, 65, 257, 1000)


def _unit(a, axis):
    return (a / np.linalg.norm(a, axis=axis, keepdims=True)).astype(np.float32)


def _pose(rng):
    return pc.rodrigues(rng.normal(0.0, 0.2, 3)), rng.normal(0.0, 0.5, 3)


def _reference(rng, name, qmap, R, t, K, kinds, dense, fallback, seed_ref_map):
    """One reference: kinds = (n_in, n_wrong, n_reject), shuffled over the rows."""
    n = sum(kinds)
    kind = np.array(["in"] * kinds[0] + ["wrong"] * kinds[1] + ["reject"] * kinds[2])
    kind = kind[rng.permutation(n)]
    cols = qmap.reshape(C, W * H)
    # 3D points whose projection under (R, t, K) is the pixel (u, v), away from the border
    uv = rng.uniform(3.0, 61.0, (n, 2))
    z = rng.uniform(4.0, 20.0, n)
    Pc = np.stack([(uv[:, 0] - K[0, 2]) / K[0, 0] * z, (uv[:, 1] - K[1, 2]) / K[1, 1] * z, z], 1)
    X = (Pc - t) @ R
    cell = (np.floor(uv[:, 1] / CELL) * H + np.floor(uv[:, 0] / CELL)).astype(np.int64)  # a_y * height + a_x
    other = (cell + rng.integers(1, W * H, n)) % (W * H)
    desc = np.empty((n, C), np.float32)
    for i in range(n):
        if kind[i] == "in":
            d = cols[:, cell[i]] + rng.normal(0.0, 1e-3, C)
        elif kind[i] == "wrong":
            d = cols[:, other[i]] + rng.normal(0.0, 1e-3, C)
        else:
            d = cols[:, cell[i]] + cols[:, other[i]]
        desc[i] = _unit(d, 0)
    ref_rng = np.random.Generator(np.random.PCG64(seed_ref_map))
    ref_map = _unit(ref_rng.normal(0.0, 1.0, (C, W, H)), 0)
    if dense:
        # at most one point per reference cell: the gathered descriptor of row i is desc[i]
        assert n <= W * H
        rc = ref_rng.permutation(W * H)[:n]
        i1, i0 = rc // H, rc % H  # coordinate 0 runs along the map's last dimension
        p2 = np.stack([(i0 + ref_rng.uniform(0.1, 0.9, n)) * CELL, (i1 + ref_rng.uniform(0.1, 0.9, n)) * CELL], 1)
        ref_map.reshape(C, W * H)[:, rc] = desc.T
    else:
        p2 = ref_rng.uniform(1.0, 62.0, (n, 2))
    ref = dict(points_2D=p2, points_3D=X, intrinsics=K, distortion_coefficients=np.zeros(4),
               image_resolution=IMAGE, filename=name, hypercolumn=ref_map, kind=kind)
    if not dense:
        ref["sparse_descriptors"] = desc
    if fallback:
        Rf, tf = pc.rodrigues(pc.rotvec(R) + 0.01), t + 0.05
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = Rf, tf
        from fmpnp.matrix_utils import matrix_quaternion
        ref["fallback_pose"] = (matrix_quaternion(m), m)
    return ref


# name: (seed, [reference spec]); a spec is (kinds, K, dense, fallback) or ("same", j): reference j's data again
GOOD63, GOOD64, GOOD65 = (40, 13, 10), (45, 9, 10), (30, 20, 15)
SCENES = {
    # the row counts 1 .. 1000, the all-zero mask, count <= minimum_matches, too few inliers without a fallback
    "mixed": (101, [((0, 0, 1), K0, True, False), (GOOD63, K0, True, False), ((0, 0, 64), K0, True, False),
                    ((3, 0, 62), K0, True, False), ((20, 7, 230), K0, False, False), ((600, 300, 100), K0, False, False),
                    ((0, 9, 20), K0, True, False)]),
    # the best pair's inliers cross the workgroup tile in the pick kernel too; equal num_inliers: the earlier wins
    "tie": (102, [((3, 0, 20), K0, True, False), ((300, 37, 20), K0, False, False), ("same", 1),
                  (GOOD65, K0, True, False)]),
    # too few inliers with a fallback (it enters with score 0) beside a solved pair; the last K differs
    "fallback_loses": (103, [((0, 9, 10), K0, True, True), (GOOD64, K0, True, False), ((0, 0, 30), K1, True, False)]),
    # nothing solves; the second fallback (count <= minimum_matches) ties the first at score 0: the first wins
    "fallback_wins": (104, [((0, 0, 12), K0, True, False), ((0, 10, 30), K0, True, True), ((2, 0, 30), K0, True, True)]),
    # every reference fails and none has a fallback
    "none": (105, [((0, 0, 40), K0, True, False), ((4, 0, 1), K0, True, False), ((0, 10, 0), K0, False, False)]),
}
# the queries of localize_multi: three different branch mixes
MULTI = ("tie", "none", "fallback_wins")


@functools.lru_cache(maxsize=None)
def scene(name):
    """dict(query [C, W, H] float32, references [dict], R, t)."""
    seed, specs = SCENES[name]
    rng = np.random.Generator(np.random.PCG64(seed))
    qmap = _unit(rng.normal(0.0, 1.0, (C, W, H)), 0)
    R, t = _pose(rng)
    refs = []
    for j, spec in enumerate(specs):
        if spec[0] == "same":
            r = dict(refs[spec[1]])
            r["filename"] = f"{name}/ref{j}.png"
            refs.append(r)
            continue
        kinds, K, dense, fallback = spec
        refs.append(_reference(rng, f"{name}/ref{j}.png", qmap, R, t, K, kinds, dense, fallback, 1000 * seed + j))
    return dict(query=qmap, references=refs, R=R, t=t)


def public(ref):
    """The reference without the builder's bookkeeping."""
    return {k: v for k, v in ref.items() if k != "kind"}


# ---- the staged yardstick ------------------------------------------------------------------------

def choose(predictions):
    """sparse_to_dense_predictor.py:233 on predictor.py:51-54: (export, best) or (None, None)."""
    if not predictions:
        return None, None
    best = predictions[int(np.argmax([p.num_inliers for p in predictions]))]
    return [*best.quaternion, *list(np.asarray(best.matrix)[:3, 3])], best


def staged(refs, matches, solve):
    """sparse_to_dense_predictor.py:161-191 per reference: matches = [(points [n, 2] float32, mask bool [n])],
    solve(points_2D, points_3D, ref, reference_2D_points) -> Prediction.  Returns (every pair's prediction
    after the fallback, None where absent; the list the best is chosen from, with each entry's reference
    index; every pair's masked arrays)."""
    from fmpnp.pnp import Prediction
    every, eligible, arrays = [], [], []
    for j, (ref, (pts, mask)) in enumerate(zip(refs, matches)):
        points_2D = np.reshape(np.asarray(pts)[mask], (-1, 1, 2))
        points_3D = np.reshape(np.asarray(ref["points_3D"])[mask], (-1, 1, 3))
        ref_2D = np.asarray(ref["points_2D"])[mask]
        prediction = solve(points_2D, points_3D, ref, ref_2D)
        if not prediction.success:
            fb = ref.get("fallback_pose")
            if fb is not None:  # _nearest_neighbor_prediction, then :184-188
                prediction = Prediction(success=True, num_matches=points_2D.shape[0], num_inliers=0,
                                        reference_inliers=ref_2D, query_inliers=np.squeeze(points_2D),
                                        points_3d=points_3D, quaternion=fb[0], matrix=fb[1],
                                        reference_filename=ref["filename"], reference_keypoints=None, inlier_mask=None)
                eligible.append((j, prediction))
        else:
            eligible.append((j, prediction))
        every.append(prediction)
        arrays.append((points_2D, ref_2D, points_3D))
    return every, eligible, arrays


def branches(refs, every, eligible, arrays, minimum_matches):
    """The branches the yardstick's outputs reach, as a set of names."""
    out = set()
    for ref, pred, (p2, _, _) in zip(refs, every, arrays):
        n, fb = p2.shape[0], ref.get("fallback_pose") is not None
        if n == 0:
            out.add("mask_all_zero")
        if n <= minimum_matches:
            out.add("count_le_minimum_matches")
        solved = pred.success and pred.inlier_mask is not None
        if n >= 4 and n > minimum_matches and not solved:
            out.add("too_few_inliers_with_fallback" if fb else "too_few_inliers_absent")
        if solved:
            out.add("solved")
    if not eligible:
        out.add("none")
    else:
        scores = [p.num_inliers for _, p in eligible]
        k = int(np.argmax(scores))
        if scores[k] == 0:
            out.add("fallback_wins")
        if scores[k] > 0 and scores.count(scores[k]) > 1:
            out.add("tie_earlier_wins")
    return out


def equal(a, b, what=""):
    """Exact equality of two values of a Prediction / Localization: None-ness, type class, dtype, shape, bytes."""
    if a is None or b is None:
        assert a is None and b is None, (what, a, b)
        return
    if isinstance(a, (str, bool)) or isinstance(b, (str, bool)):
        assert a == b and type(a) is type(b), (what, a, b)
        return
    if isinstance(a, (list, tuple)) and not isinstance(b, np.ndarray):
        assert len(a) == len(b), (what, a, b)
        for x, y in zip(a, b):
            equal(x, y, what)
        return
    x, y = np.asarray(a), np.asarray(b)
    assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, x, y)


def equal_prediction(a, b, what=""):
    if a is None or b is None:
        assert a is None and b is None, (what, a, b)
        return
    for f in a._fields:
        equal(getattr(a, f), getattr(b, f), f"{what}.{f}")
