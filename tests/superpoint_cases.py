"""Shared inputs of the SuperPoint baseline's tests (test_superpoint_cpu.py, test_gpu_superpoint.py) and of the
generator of their goldens (tests/golden/gen_golden_superpoint.py): seed-driven detector maps with planted
peaks, descriptor sets with planted correspondences, keypoints and landmarks.  The generator picks, per case,
the first seed for which the reference's own outputs keep the margins the issue names (no tie the reference's
sorts could break either way) and records it; the tests rebuild the inputs from that seed.  Every array is
built once and never modified."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BORDER = 4

# name -> (H, W, D, nms_dist, conf_thresh, dustbin logit, planted peaks as (x, y, logit))
DETECTOR = {
    # three chains of descending peaks 3 pixels apart: each peak suppresses the next, which frees the one after
    "main": (64, 96, 256, 4, 0.015, 4.0,
             [(20 + 3 * k, 30 + (k % 2), 9.0 - 0.5 * k) for k in range(9)]
             + [(70, 10 + 3 * k, 8.8 - 0.45 * k) for k in range(8)]
             + [(50 - 4 * k, 50 - 2 * k, 7.9 - 0.3 * k) for k in range(6)]),
    "dense": (120, 160, 64, 1, 0.005, 7.5,
              [(31 + k, 40, 9.5 - 0.4 * k) for k in range(10)] + [(100, 60 + k, 9.1 - 0.35 * k) for k in range(9)]
              + [(60 + k, 90 + k, 8.7 - 0.3 * k) for k in range(7)]),
    "none": (32, 40, 16, 4, 0.015, 12.0, []),
    # a peak inside the border band, a weaker interior one in its window: the first suppresses, then is dropped
    "border": (48, 64, 32, 4, 0.015, 6.0, [(2, 20, 9.0), (5, 22, 8.0), (40, 1, 8.5), (43, 5, 7.5), (30, 30, 7.0)]),
}

# name -> (N1, N2, D, ratio)
MATCHING = {
    "two": (2, 2, 64, 0.9),
    "n63_65": (63, 65, 256, 0.9),
    "n64_64": (64, 64, 64, 0.7),
    "n65_257": (65, 257, 256, 0.7),
    "n257_63": (257, 63, 64, 0.9),
    "n1000_1000": (1000, 1000, 256, 0.9),
    "n1000_257": (1000, 257, 64, 0.7),
}
ASSEMBLY_LANDMARKS = 301  # points_2D / points_3D rows of a matching case's reference


def _rng(kind, name, seed):
    return np.random.default_rng([sum(ord(c) for c in kind + name), 20261019, int(seed)])


@functools.lru_cache(maxsize=None)
def detector_inputs(name, seed):
    """(semi [65, Hc, Wc], coarse_desc [D, Hc, Wc]) fp32."""
    H, W, D, _, _, dust, peaks = DETECTOR[name]
    rng = _rng("det", name, seed)
    Hc, Wc = H // 8, W // 8
    semi = rng.standard_normal((65, Hc, Wc)).astype(np.float32)
    semi[64] = np.float32(dust) + 0.25 * rng.standard_normal((Hc, Wc)).astype(np.float32)
    for x, y, logit in peaks:
        semi[(y % 8) * 8 + x % 8, y // 8, x // 8] = np.float32(logit + 0.05 * rng.standard_normal())
    coarse = rng.standard_normal((D, Hc, Wc)).astype(np.float32)
    coarse /= np.linalg.norm(coarse, axis=0, keepdims=True)
    semi.setflags(write=False)
    coarse.setflags(write=False)
    return semi, coarse


@functools.lru_cache(maxsize=None)
def matching_inputs(name, seed):
    """(desc1 [N1, D], desc2 [N2, D]) fp32 unit rows.  A third of the query rows are noisy copies of reference
    rows at three noise levels (a clear pass, a clear fail and in between); rows 0 and 1 copy the same reference
    row where the sizes allow, so one reference keypoint is matched by several query rows."""
    N1, N2, D, _ = MATCHING[name]
    rng = _rng("match", name, seed)
    desc2 = rng.standard_normal((N2, D))
    desc2 /= np.linalg.norm(desc2, axis=1, keepdims=True)
    desc1 = rng.standard_normal((N1, D))
    for i in range(0, N1, 3):
        j = 0 if i < 2 else int(rng.integers(N2))
        desc1[i] = desc2[j] + (0.02, 0.06, 0.12)[(i // 3) % 3] * rng.standard_normal(D)
    if N1 >= 2:
        desc1[1] = desc2[0] + 0.03 * rng.standard_normal(D)
    desc1 /= np.linalg.norm(desc1, axis=1, keepdims=True)
    a, b = desc1.astype(np.float32), desc2.astype(np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def assembly_inputs(name, seed):
    """(query keypoints [3, N1], reference keypoints [3, N2], points_2D [M, 2], points_3D [M, 3]) fp64 for the
    matching case: integer pixel keypoints with a confidence row, landmarks at non-integer positions."""
    N1, N2, _, _ = MATCHING[name]
    rng = _rng("asm", name, seed)

    def keypoints(n):
        k = np.stack([rng.integers(4, 1020, n).astype(np.float64), rng.integers(4, 1020, n).astype(np.float64),
                      np.sort(rng.uniform(0.005, 0.5, n))[::-1].astype(np.float32).astype(np.float64)])
        k.setflags(write=False)
        return k
    p2 = rng.uniform(0.0, 1024.0, (ASSEMBLY_LANDMARKS, 2))
    p3 = rng.standard_normal((ASSEMBLY_LANDMARKS, 3)) * 10.0
    p2.setflags(write=False)
    p3.setflags(write=False)
    return keypoints(N1), keypoints(N2), p2, p3


@functools.lru_cache(maxsize=None)
def golden(kind):
    """tests/golden/superpoint_<kind>.npz as a dict of arrays."""
    with np.load(os.path.join(GOLDEN, f"superpoint_{kind}.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def heat64(semi):
    """The detector head restated in fp64 (demo_superpoint.py:240-250)."""
    d = np.exp(semi.astype(np.float64))
    d = d / (d.sum(axis=0) + .00001)
    Hc, Wc = semi.shape[1:]
    return d[:-1].transpose(1, 2, 0).reshape(Hc, Wc, 8, 8).transpose(0, 2, 1, 3).reshape(Hc * 8, Wc * 8)


def desc64(coarse, pts, H, W, align_corners):
    """Descriptor sampling restated in fp64 (demo_superpoint.py:273-283 on grid_sample's formulas)."""
    c = coarse.astype(np.float64)
    D, Hc, Wc = c.shape
    out = np.zeros((D, pts.shape[1]))
    for p in range(pts.shape[1]):
        g = [np.float64(np.float32(pts[0, p] / (W / 2.) - 1.)), np.float64(np.float32(pts[1, p] / (H / 2.) - 1.))]
        ij = [(((g[k] + 1) / 2) * (s - 1)) if align_corners else (((g[k] + 1) * s - 1) / 2) for k, s in ((0, Wc), (1, Hc))]
        x0, y0 = int(np.floor(ij[0])), int(np.floor(ij[1]))
        for dy in (0, 1):
            for dx in (0, 1):
                x, y = x0 + dx, y0 + dy
                if 0 <= x < Wc and 0 <= y < Hc:
                    out[:, p] += c[:, y, x] * (1 - abs(ij[0] - x)) * (1 - abs(ij[1] - y))
    return out / np.linalg.norm(out, axis=0, keepdims=True)


def ulps32(a, b):
    """The distance of two fp32 arrays of one sign in units of the last place."""
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


# ---- a small localisation scene ----------------------------------------------------------------------------
PNP = dict(reprojection_threshold=12.0, minimum_matches=5, minimum_inliers=12, iters=256, seed=0)
K0 = np.array([[900.0, 0.0, 512.0], [0.0, 900.0, 512.0], [0.0, 0.0, 1.0]])
K1 = np.array([[880.0, 0.0, 500.0], [0.0, 905.0, 520.0], [0.0, 0.0, 1.0]])  # a second camera: a second PnP call


def _rodrigues(r):
    th = np.linalg.norm(r)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


@functools.lru_cache(maxsize=None)
def localize_scene():
    """(query (pts [3, N], desc [D, N]), references): four references in rank order -- 40 and 70 true
    correspondences (the second wins), one with unrelated descriptors and a fallback pose, one with unrelated
    descriptors and none; the last two use a second camera.  Reference keypoints sit on their landmarks."""
    rng = _rng("loc", "scene", 0)
    D = 64
    R, t = _rodrigues(rng.normal(0.0, 0.1, 3)), rng.normal(0.0, 0.3, 3)
    q_pts, q_desc, refs = [], [], []
    for j, (n_true, n_noise, K, fallback) in enumerate(((40, 25, K0, True), (70, 30, K0, False), (0, 50, K1, True),
                                                        (0, 45, K1, False))):
        n = n_true + n_noise
        uv = np.round(rng.uniform(20.0, 1000.0, (n, 2)))
        z = rng.uniform(4.0, 20.0, n)
        Pc = np.stack([(uv[:, 0] - K[0, 2]) / K[0, 0] * z, (uv[:, 1] - K[1, 2]) / K[1, 1] * z, z], 1)
        X = (Pc - t) @ R  # the points whose projection under (R, t, K) is the query pixel uv
        desc = rng.standard_normal((n, D))
        desc /= np.linalg.norm(desc, axis=1, keepdims=True)
        ref_uv = np.round(rng.uniform(20.0, 1000.0, (n, 2)))
        ref = dict(filename=f"ref{j}.jpg", intrinsics=K, distortion_coefficients=np.zeros(4),
                   points_2D=ref_uv + rng.uniform(-0.3, 0.3, (n, 2)), points_3D=X,
                   keypoints=np.vstack([ref_uv.T, np.linspace(0.5, 0.01, n)[None]]),
                   descriptors=desc.T.astype(np.float32))
        if fallback:
            m = np.eye(4)
            m[:3, :3], m[:3, 3] = _rodrigues(rng.normal(0.0, 0.1, 3)), rng.normal(0.0, 0.3, 3)
            ref["fallback_pose"] = ([1.0, 0.0, 0.0, 0.0], m)
        refs.append(ref)
        for i in range(n_true):
            q_pts.append(uv[i])
            v = desc[i] + 0.03 * rng.standard_normal(D)
            q_desc.append(v / np.linalg.norm(v))
    for _ in range(30):  # query keypoints of nothing
        q_pts.append(np.round(rng.uniform(20.0, 1000.0, 2)))
        v = rng.standard_normal(D)
        q_desc.append(v / np.linalg.norm(v))
    q_pts = np.vstack([np.array(q_pts).T, np.linspace(0.6, 0.01, len(q_pts))[None]])
    return (q_pts, np.array(q_desc).T.astype(np.float32)), refs
