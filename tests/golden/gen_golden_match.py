#!/usr/bin/env python3
"""Generate tests/golden/match_*.npz from the reference's dense matching code.

TEST INFRASTRUCTURE ONLY, like gen_golden.py: it imports the *reference*
s2dhm/pose_prediction/exhaustive_search.py and keypoint_association.py unmodified (read-only at
/root/reference) and records what they compute on small seeded inputs; it refuses to run where the
reference is absent.  Stand-ins are written into a temporary directory OUTSIDE the repository, ahead
of the reference on sys.path: a no-op `gin` (exhaustive_search is gin.configurable; factor is passed
explicitly), an empty `cv2` when cv2 is not installed (keypoint_association uses it only for KeyPoint
objects), and `np.bool = bool` (retrieve_argmax casts with np.bool, which numpy 2 dropped).

The generator asserts about its own inputs what lets the tests compare every row with no exclusions:
in match_main, for every row and factor, the fp64 gap between the two largest scores and the fp64
margin |0.81 d1 - d_k| are >= 1e-4 (three orders above the fp32 summation error of unit-norm
descriptors), the reference agrees with fp64 on every row, and both mask values occur in >= 5 rows
at each factor.  The edge cases assert the behaviour they are there to pin.

Run:  python tests/golden/gen_golden_match.py
"""
import importlib.util
import os
import sys
import tempfile

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
PP = os.path.join(REF, "s2dhm", "pose_prediction")

if not os.path.isfile(os.path.join(PP, "exhaustive_search.py")):
    raise SystemExit("gen_golden_match.py needs the reference at /root/reference; use the committed fixtures instead")


def _install_shims():
    d = tempfile.mkdtemp(prefix="fmpnp_refshims_")
    with open(os.path.join(d, "gin.py"), "w") as f:
        f.write(
            "def _deco(*a, **k):\n"
            "    if len(a) == 1 and callable(a[0]) and not k:\n"
            "        return a[0]\n"
            "    return lambda f: f\n"
            "configurable = _deco\n"
            "register = _deco\n")
    if importlib.util.find_spec("cv2") is None:
        with open(os.path.join(d, "cv2.py"), "w") as f:
            f.write("# empty stand-in: keypoint_association uses cv2 only for KeyPoint objects\n")
    sys.path[:0] = [d, PP]


_install_shims()
if not hasattr(np, "bool"):
    np.bool = bool  # exhaustive_search.py:21 (numpy 2 dropped the alias)

import torch  # noqa: E402

torch.set_num_threads(1)

import exhaustive_search as ref_es  # noqa: E402  s2dhm/pose_prediction/exhaustive_search.py
import keypoint_association as ref_ka  # noqa: E402  s2dhm/pose_prediction/keypoint_association.py

FACTORS = (0.006, 0.05, 0.12)
RATIO2 = 0.9 ** 2


def unit(x, axis):
    return x / np.linalg.norm(x, axis=axis, keepdims=True)


def run_ref(dense, sparse, image_shape, map_size, factor):
    pts, mask = ref_es.exhaustive_search(torch.from_numpy(dense), torch.from_numpy(sparse), list(image_shape),
                                         list(map_size), [8, 8], factor)
    assert pts.dtype == torch.float32 and mask.dtype == bool
    return pts.numpy().copy(), np.asarray(mask).copy()


def fp64_rows(dense, sparse, top_k):
    s = sparse.astype(np.float64) @ dense.astype(np.float64)
    srt = -np.sort(-s, axis=1)
    return s, np.argmax(s, axis=1), srt[:, 0], srt[:, 1] if s.shape[1] > 1 else srt[:, 0], srt[:, top_k - 1]


def points_of(argmax, image_shape, map_size):
    w, h = map_size
    idx = torch.from_numpy(np.stack([argmax % h, argmax // h], 1).astype(np.float32))
    q = torch.FloatTensor(list(image_shape)) / torch.FloatTensor([w, h])
    return (idx * q + q / 2).numpy()


def gen_main():
    """Unit-norm Gaussians, C = 40, a 24 x 20 map (non-square: an x / y swap shows), N = 37 rows of three
    kinds: planted near-copies of a dense column (True at every factor), rows sharing the map's strong
    common component (scores crowd together: False even at large k), plain random rows (False at
    small k)."""
    rng = np.random.default_rng(20260101)
    C, W, H, N = 40, 24, 20, 37
    u = unit(rng.standard_normal(C), 0)
    dense = unit(rng.standard_normal((C, W * H)) / np.sqrt(C) + 1.2 * u[:, None], 0).astype(np.float32)
    kinds = np.array([0] * 19 + [1] * 9 + [2] * 9)
    cols = rng.choice(W * H, N, replace=False)
    sparse = np.zeros((N, C))
    for i, kind in enumerate(kinds):
        g = rng.standard_normal(C) / np.sqrt(C)
        if kind == 0:
            sparse[i] = dense[:, cols[i]] + 0.15 * g
        elif kind == 1:
            sparse[i] = g + 2.5 * u
        else:
            sparse[i] = g - (g @ u) * u
    sparse = unit(sparse, 1).astype(np.float32)
    image_shape, map_size = (192, 120), (W, H)
    out = dict(dense=dense, sparse=sparse, image_shape=np.array(image_shape), map_size=np.array(map_size),
               factors=np.array(FACTORS), kinds=kinds, planted_cols=cols)
    for f in FACTORS:
        top_k = int(f * W * H)
        pts, mask = run_ref(dense, sparse, image_shape, map_size, f)
        s, am, d1, d2, dk = fp64_rows(dense, sparse, top_k)
        gap, margin = (d1 - d2).min(), np.abs(RATIO2 * d1 - dk).min()
        assert gap >= 1e-4 and margin >= 1e-4, (f, gap, margin)
        assert np.array_equal(pts, points_of(am, image_shape, map_size)), f
        assert np.array_equal(mask, RATIO2 * d1 >= dk), f
        assert mask.sum() >= 5 and (~mask).sum() >= 5, (f, mask.sum())
        assert np.array_equal(am[kinds == 0], cols[kinds == 0])
        print(f"match_main factor {f}: top_k {top_k}, min gap {gap:.3g}, min mask margin {margin:.3g}, "
              f"{mask.sum()} True / {(~mask).sum()} False")
        out[f"points_{f}"], out[f"mask_{f}"], out[f"argmax_{f}"] = pts, mask, am.astype(np.int32)
    np.savez_compressed(os.path.join(HERE, "match_main.npz"), **out)


def save_edge(name, dense, sparse, image_shape, map_size, factor, tie_rows=(), **extra):
    pts, mask = run_ref(dense, sparse, image_shape, map_size, factor)
    # every finite quantity a test compares has the main case's margins (the reference's mm sums in
    # another order than the fmaf chain); the rows of a deliberate tie are exempt from the gap
    top_k = int(factor * map_size[0] * map_size[1])
    with np.errstate(invalid="ignore", over="ignore"):
        sc = sparse.astype(np.float64) @ dense.astype(np.float64)
        for i, row in enumerate(sc):
            if np.isnan(row).any():
                continue
            srt = -np.sort(-row)
            if np.isfinite(srt[0]) and i not in tie_rows:
                assert srt[0] - srt[1] >= 1e-4, (name, i, srt[0] - srt[1])
            m = RATIO2 * srt[0] - srt[top_k - 1]
            if np.isfinite(m):
                assert abs(m) >= 1e-4, (name, i, m)
    np.savez_compressed(os.path.join(HERE, f"match_edge_{name}.npz"), dense=dense, sparse=sparse,
                        image_shape=np.array(image_shape), map_size=np.array(map_size), factor=np.float64(factor),
                        points=pts, mask=mask, **extra)
    return pts, mask


def gen_edges():
    rng = np.random.default_rng(20260102)
    C, W, H, N = 12, 9, 7, 11
    image_shape, map_size = (72, 42), (W, H)
    base_d = unit(rng.standard_normal((C, W * H)), 0).astype(np.float32)
    base_s = unit(rng.standard_normal((N, C)), 1).astype(np.float32)

    # a NaN in one dense column: every row's argmax is that column, every mask False
    d = base_d.copy()
    col = 4 * H + 3
    d[5, col] = np.nan
    pts, mask = save_edge("nan", d, base_s, image_shape, map_size, 0.1, column=np.int64(col))
    assert np.array_equal(pts, points_of(np.full(N, col), image_shape, map_size)) and not mask.any()

    # a +Inf in one dense entry: rows with a positive coefficient there peak at it (d1 = +Inf, mask
    # True), rows with a negative one see -Inf at the bottom of the row
    d = base_d.copy()
    col, ch = 2 * H + 6, 7
    d[ch, col] = np.inf
    pos = base_s[:, ch] > 0
    assert pos.any() and (~pos).any() and np.all(base_s[:, ch] != 0)
    pts, mask = save_edge("inf", d, base_s, image_shape, map_size, 0.1, column=np.int64(col))
    assert np.array_equal(pts[pos], points_of(np.full(pos.sum(), col), image_shape, map_size)) and mask[pos].all()

    # two identical dense columns, sparse rows equal to them: the lower flat index wins
    d = base_d.copy()
    lo, hi = 1 * H + 2, 6 * H + 5
    d[:, hi] = d[:, lo]
    s = base_s.copy()
    s[0], s[3] = d[:, lo], d[:, hi]
    pts, mask = save_edge("tie", d, s, image_shape, map_size, 0.1, tie_rows=(0, 3), column=np.int64(lo))
    assert np.array_equal(pts[[0, 3]], points_of(np.array([lo, lo]), image_shape, map_size))

    # top_k = 1: d_k = d1, so the mask is True only where d1 <= 0 (rows opposing the map's common component)
    u = unit(rng.standard_normal(C), 0)
    d = unit(rng.standard_normal((C, W * H)) / np.sqrt(C) + 1.5 * u[:, None], 0).astype(np.float32)
    s = base_s.copy()
    s[:5] = unit(-u[None, :] + 0.05 * rng.standard_normal((5, C)), 1)
    factor = 1.5 / (W * H)
    assert int(factor * W * H) == 1
    pts, mask = save_edge("top1", d, s, image_shape, map_size, factor)
    d1 = (s.astype(np.float64) @ d.astype(np.float64)).max(1)
    assert np.abs(d1).min() > 1e-3 and np.array_equal(mask, d1 <= 0) and mask.sum() >= 5 and (~mask).sum() >= 5

    # top_k = W * H: d_k is the row minimum
    assert int(1.0 * W * H) == W * H
    pts, mask = save_edge("topall", d, s, image_shape, map_size, 1.0)
    sc = s.astype(np.float64) @ d.astype(np.float64)
    margin = np.abs(RATIO2 * sc.max(1) - sc.min(1)).min()
    assert margin > 1e-4 and np.array_equal(mask, RATIO2 * sc.max(1) >= sc.min(1)), margin
    print(f"match_edge_*: written (topall: {mask.sum()} True / {(~mask).sum()} False)")


def gen_assoc():
    """fast_closest_points' argmins over generate_dense_keypoints' grid: random points (some outside
    the image), and on the exact-cell grid every cell edge and centre per axis (ties: the lower cell)."""
    rng = np.random.default_rng(20260103)
    out = {}
    for tag, (fmap, res) in (("exact", ((24, 20), (192, 120))), ("ragged", ((7, 9), (100, 50)))):
        grid, cells = ref_ka.generate_dense_keypoints(list(fmap), list(res))
        assert grid.shape == (fmap[0] * fmap[1], 2), grid.shape
        # keypoint coordinate 0 runs along the grid's second axis (keypoint_association.py:33)
        pts = np.stack([rng.uniform(-6, res[1] + 6, 300), rng.uniform(-6, res[0] + 6, 300)], 1)
        if tag == "exact":
            a1 = np.arange(0, res[1] + cells[1] / 4, cells[1] / 2)  # every edge and centre along coordinate 0
            a0 = np.arange(0, res[0] + cells[0] / 4, cells[0] / 2)
            e0 = np.stack([a1, rng.uniform(0, res[0], a1.size)], 1)
            e1 = np.stack([rng.uniform(0, res[1], a0.size), a0], 1)
            e2 = np.stack([rng.choice(a1, 60), rng.choice(a0, 60)], 1)  # edges on both axes at once
            pts = np.concatenate([pts, e0, e1, e2])
        argmin = ref_ka.fast_closest_points(torch.from_numpy(np.ascontiguousarray(pts.T)), torch.from_numpy(grid))
        out[f"{tag}_fmap"], out[f"{tag}_res"], out[f"{tag}_cells"] = np.array(fmap), np.array(res), np.array(cells)
        out[f"{tag}_grid"], out[f"{tag}_points"], out[f"{tag}_argmin"] = grid, pts, argmin.numpy()
    # the whole fast_sparse_keypoint_descriptor on a small batch (CPU branch of the reference)
    fmap, res = (24, 20), (192, 120)
    grid, _ = ref_ka.generate_dense_keypoints(list(fmap), list(res))
    desc = rng.standard_normal((2, 5, fmap[0], fmap[1])).astype(np.float32)
    kps = [np.stack([rng.uniform(0, res[1], n), rng.uniform(0, res[0], n), rng.uniform(0, 1, n)], 0) for n in (13, 6)]
    assert not torch.cuda.is_available()
    sd = ref_ka.fast_sparse_keypoint_descriptor(kps, torch.from_numpy(grid), torch.from_numpy(desc))
    out["fsk_desc"], out["fsk_kp0"], out["fsk_kp1"] = desc, kps[0], kps[1]
    out["fsk_out0"], out["fsk_out1"] = sd[0].numpy(), sd[1].numpy()
    np.savez_compressed(os.path.join(HERE, "match_assoc.npz"), **out)
    print("match_assoc: written")


if __name__ == "__main__":
    gen_main()
    gen_edges()
    gen_assoc()
