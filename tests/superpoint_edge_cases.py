"""Shared inputs and independent references of the SuperPoint baseline's decision clauses (ties, -0, NaN, Inf,
taps outside the map, unordered match lists): test_superpoint_edges_cpu.py holds the CPU twins to the references
here, test_gpu_superpoint_edges.py holds the kernels to the twins.  The references are plain numpy written from
the contract text of include/fmpnp.h ("SuperPoint baseline", stages 1-5), not from the library's code.  Every
input is seeded, built once and never modified; nothing here touches a device."""
import functools

import numpy as np

f32 = np.float32


def frozen(a):
    a.setflags(write=False)
    return a


# ---- references ------------------------------------------------------------------------------------------------
def greedy_nms(heat, conf, d, border):
    """Stage 2 as the contract words it: (pts [3, n] fp64 rows x, y, heat in the walk's order, the number kept
    before the border drop)."""
    heat = np.asarray(heat, f32)
    H, W = heat.shape
    flat = heat.ravel()
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(flat >= f32(conf))  # (a NaN is none)
    heat64 = flat[cand].astype(np.float64)
    order = cand[np.argsort(-(heat64 + 0.0), kind="stable")]  # descending, -0 as +0, equal heats by pixel index
    blocked = np.zeros((H, W), bool)  # within Chebyshev distance d of a kept point
    kept = []
    for i in order:
        y, x = divmod(int(i), W)
        if blocked[y, x]:
            continue
        kept.append((x, y))
        blocked[max(0, y - d):y + d + 1, max(0, x - d):x + d + 1] = True
    inside = [(x, y) for x, y in kept if border <= x < W - border and border <= y < H - border]
    pts = np.zeros((3, len(inside)))
    for k, (x, y) in enumerate(inside):
        pts[:, k] = (x, y, np.float64(heat[y, x]))
    return pts, len(kept)


def two_nearest_ref(desc1, desc2, ratio):
    """Stage 4 for integer-valued operands (every score is exact, so any summation order gives the contract's
    bits): dict(idx [N1, 2] int32, dist [N1, 2] fp32, ok [N1] bool, matches [n, 2] int64, all [N1, N2] fp32)."""
    a, b = np.asarray(desc1, np.float64), np.asarray(desc2, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (a[:, None, :] * b[None, :, :]).sum(axis=2).astype(f32)
        dist = f32(2) * (f32(1) - s)  # two fp32 roundings
    N1, N2 = dist.shape
    nan = np.isnan(dist)
    value = np.where(nan, f32(0), dist) + f32(0)  # (-0 counts as +0)
    idx = np.zeros((N1, 2), np.int32)
    for i in range(N1):
        idx[i] = np.lexsort((np.arange(N2), value[i], nan[i]))[:2]  # NaN last, then the value, then the index
    two = np.take_along_axis(dist, idx.astype(np.int64), 1)
    ratio2 = f32(np.float64(ratio) * np.float64(ratio))
    with np.errstate(invalid="ignore"):
        ok = two[:, 0] <= ratio2 * two[:, 1]
    rows = np.flatnonzero(ok)
    matches = np.stack([rows, idx[rows, 0]], 1).astype(np.int64).reshape(-1, 2)
    return dict(idx=idx, dist=two, ok=ok, matches=matches, all=dist)


def assemble_ref(query_pts, ref_pts, points2d, points3d, matches):
    """Stage 5: (argmin [N2] int32, x2d [n, 2], x2d_ref [n, 2], x3d [n, 3])."""
    q, r = np.asarray(query_pts, np.float64), np.asarray(ref_pts, np.float64)
    p2, p3 = np.asarray(points2d, np.float64), np.asarray(points3d, np.float64)
    N1, N2 = q.shape[1], r.shape[1]
    argmin = np.zeros(N2, np.int32)
    for i in range(N2):
        with np.errstate(invalid="ignore"):
            dx, dy = p2[:, 0] - r[0, i], p2[:, 1] - r[1, i]
            a, b = dx * dx, dy * dy
            dist = a + b  # two products, one sum
        if not np.isnan(dist).all():
            argmin[i] = np.flatnonzero(dist == np.nanmin(dist))[0]  # the lowest index among equal minima
    first = {}
    for row, j in np.asarray(matches, np.int64).reshape(-1, 2).tolist():
        if 0 <= row < N1 and 0 <= j < N2:
            first[j] = min(first.get(j, row), row)
    keys = sorted(first)
    x2d = np.array([[q[0, first[j]], q[1, first[j]]] for j in keys]).reshape(-1, 2)
    x2d_ref = np.array([[r[0, j], r[1, j]] for j in keys]).reshape(-1, 2)
    x3d = np.array([p3[argmin[j]] for j in keys]).reshape(-1, 3)
    return argmin, x2d, x2d_ref, x3d


def desc64_padded(coarse, pts, H, W, align_corners):
    """Stage 3 in fp64 on grid_sample's formulas with zero padding (superpoint_cases.desc64 with a non-finite
    coordinate treated as "no tap"): (the un-normalised samples [D, N], their norms [N], taps inside [N])."""
    c = np.asarray(coarse, np.float64)
    D, Hc, Wc = c.shape
    out, taps = np.zeros((D, pts.shape[1])), np.zeros(pts.shape[1], int)
    for p in range(pts.shape[1]):
        with np.errstate(invalid="ignore", over="ignore"):
            g = [np.float64(f32(pts[0, p] / (W / 2.) - 1.)), np.float64(f32(pts[1, p] / (H / 2.) - 1.))]
            ij = [(((g[k] + 1) / 2) * (s - 1)) if align_corners else (((g[k] + 1) * s - 1) / 2)
                  for k, s in ((0, Wc), (1, Hc))]
        if not (np.isfinite(ij[0]) and np.isfinite(ij[1])):
            continue
        x0, y0 = int(np.floor(ij[0])), int(np.floor(ij[1]))
        for dy in (0, 1):
            for dx in (0, 1):
                x, y = x0 + dx, y0 + dy
                if 0 <= x < Wc and 0 <= y < Hc:
                    out[:, p] += c[:, y, x] * (1 - abs(ij[0] - x)) * (1 - abs(ij[1] - y))
                    taps[p] += 1
    return out, np.linalg.norm(out, axis=0), taps


# ---- NMS ---------------------------------------------------------------------------------------------------------
PLATEAU_SHAPES = ((20, 37), (1, 200), (33, 8), (1, 1))
PLATEAU_DISTS = (0, 1, 4, 16)
PLATEAU_BORDERS = (0, 4)
PLATEAU_CONF = 0.25
CHAIN = ((1, 200), 1)  # the long chain: point 2k of the row can be kept only after 2k - 2


@functools.lru_cache(maxsize=None)
def plateau(H, W):
    return frozen(np.full((H, W), 0.5, f32))


def capacity(H, W, d):
    """One kept point per (d + 1) x (d + 1) cell at the most."""
    return -(-H // (d + 1)) * -(-W // (d + 1))


LEVEL_SHAPES = ((67, 70), (17, 33))  # 4690 pixels: two compaction chunks, 9 x 3 tiles, no multiple of either
LEVEL_CONFS = (0.25, 0.0, -1.0)
LEVEL_DISTS = (0, 2, 4, 16)
LEVEL_BORDER = 4
# A -0 is kept by chance only at the smallest distances (it ranks with the zeros, behind three quarters of the
# map), so one is planted: a -0 pixel alone in a window of NaN (no candidate there can suppress it).  Up to
# distance 4 the window is 9 x 9 around a pixel in the map's middle -- in the larger map pixel 4096, the first of
# the compaction's second chunk; at 16 it is the map's corner up to row and column 20 around the first interior
# pixel.
LEVEL_PLANTS = {(67, 70): (58, 36), (17, 33): (8, 16)}
LEVEL_CORNER_PLANT = (4, 4)


def level_plant(H, W, d):
    """(y, x, radius) of the planted -0 of levels(H, W, d)."""
    return LEVEL_PLANTS[(H, W)] + (4,) if d <= 4 else LEVEL_CORNER_PLANT + (16,)


@functools.lru_cache(maxsize=None)
def levels(H, W, d=0):
    """Four heat levels with 5 % NaN, 10 % -0 and 2 % +Inf: plateaus of bit-equal values everywhere; one planted
    -0 (the same map for every d <= 4)."""
    rng = np.random.default_rng([20261021, H, W])
    heat = (rng.integers(0, 4, (H, W)) / 4).astype(f32)
    r = rng.random((H, W))
    heat[r < 0.05] = np.nan
    heat[(r >= 0.05) & (r < 0.15)] = -0.0
    heat[(r >= 0.15) & (r < 0.17)] = np.inf
    y, x, radius = level_plant(H, W, d)
    heat[max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1] = np.nan
    heat[y, x] = -0.0
    return frozen(heat)


# ---- heat extremes -----------------------------------------------------------------------------------------------
HEAT_HC, HEAT_WC = 2, 3
# (yc, xc) of the cells, in turn
CELL_OVERFLOW, CELL_LARGE, CELL_TINY, CELL_NAN, CELL_EQUAL, CELL_DUST = ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2))
OVERFLOW_CHANNEL, LARGE_CHANNEL, TINY_CHANNEL, NAN_CHANNEL = 5, 6, 7, 40


@functools.lru_cache(maxsize=None)
def heat_extremes():
    """semi [65, 2, 3]: a logit of 89 (its exponential is +Inf in fp32), one of 88.5 (finite), one of -200, a NaN
    logit, a cell of 65 equal logits and a dustbin of +60."""
    rng = np.random.default_rng(20261022)
    semi = rng.standard_normal((65, HEAT_HC, HEAT_WC)).astype(f32)
    semi[(OVERFLOW_CHANNEL,) + CELL_OVERFLOW] = 89.0
    semi[(LARGE_CHANNEL,) + CELL_LARGE] = 88.5
    semi[(TINY_CHANNEL,) + CELL_TINY] = -200.0
    semi[(NAN_CHANNEL,) + CELL_NAN] = np.nan
    semi[(slice(None),) + CELL_EQUAL] = 0.3
    semi[(64,) + CELL_DUST] = 60.0
    return frozen(semi)


def cell_pixels(cell):
    """The (rows, columns) slices of a cell's 8 x 8 heat values."""
    return slice(8 * cell[0], 8 * cell[0] + 8), slice(8 * cell[1], 8 * cell[1] + 8)


# ---- descriptor points -------------------------------------------------------------------------------------------
DESC_D, DESC_HC, DESC_WC = 70, 5, 7  # D is no multiple of the 64 chains
DESC_H, DESC_W = 8 * DESC_HC, 8 * DESC_WC
DESC_PAD = 4096  # NaN floats on either side of the map


def _along(S):
    return [0, 1, 3, 3.999, 4, S - 5, S - 4, S - 1, S, S + 3.5, S + 4.01, -3.9, -4.0, -4.5, -20, 1e30, np.nan,
            27.25 * S / DESC_W, np.inf]


# which y of _along(H) goes with each x of _along(W).  With align_corners 0 a coordinate of S + 3.5 leaves its one
# tap a weight of 1/16 and -3.9 one of 1/80: the first is paired with a coordinate whose tap has (nearly) the whole
# weight, the second with one that has no tap, so that every column is either clearly a descriptor or clearly
# none.  The huge, NaN and interior coordinates are crossed: one axis alone has to switch a column's taps off.
DESC_PAIRING = (0, 1, 2, 9, 4, 5, 6, 7, 8, 3, 11, 10, 12, 13, 14, 17, 15, 16, 18)


@functools.lru_cache(maxsize=None)
def desc_points():
    """pts [3, 19] fp64: x on, next to and beyond either edge of the map, huge, NaN and +Inf; y the same along H."""
    x, y = _along(DESC_W), _along(DESC_H)
    return frozen(np.array([x, [y[k] for k in DESC_PAIRING], np.linspace(0.9, 0.1, len(x))], np.float64))


@functools.lru_cache(maxsize=None)
def desc_coarse():
    """(buffer, coarse): coarse [70, 5, 7] fp32 with unit cells, a view of the middle of a NaN-filled buffer, so
    that a read outside the map shows up as a NaN."""
    rng = np.random.default_rng(20261023)
    c = rng.standard_normal((DESC_D, DESC_HC, DESC_WC))
    c /= np.linalg.norm(c, axis=0, keepdims=True)
    buf = np.full(2 * DESC_PAD + c.size, np.nan, f32)
    buf[DESC_PAD:DESC_PAD + c.size] = c.astype(f32).ravel()
    buf.setflags(write=False)
    return buf, buf[DESC_PAD:DESC_PAD + c.size].reshape(c.shape)


# ---- two nearest -------------------------------------------------------------------------------------------------
NN_D, NN_N1, NN_N2 = 12, 70, 600
NN_RATIOS = (0.7, 1.0, 1.5)
NN_DUPLICATES = (5, 69, 261, 599)  # one reference row: a lane of another wave, the same thread's next stride, a later wave
NN_NAN_COLUMN, NN_INF_COLUMN, NN_INF_ENTRY = 300, 301, 4
# query rows and what the contract gives them
NN_ROW_DUP, NN_ROW_SECONDS, NN_ROW_ZERO, NN_ROW_NAN = 0, 1, 2, 3
NN_EXPECT = {NN_ROW_DUP: (5, 69), NN_ROW_SECONDS: (500, 64), NN_ROW_ZERO: (0, 1), NN_ROW_NAN: (0, 1)}


@functools.lru_cache(maxsize=None)
def nn_inputs():
    """(desc1 [70, 12], desc2 [600, 12]) fp32 with entries in {-1, 0, 1}: norms above 1, so many distances are
    negative and equal."""
    rng = np.random.default_rng(20261024)
    d1 = rng.integers(-1, 2, (NN_N1, NN_D)).astype(f32)
    d2 = rng.integers(-1, 2, (NN_N2, NN_D)).astype(f32)
    u = np.array([1, -1, 1, 1, -1, -1, 1, -1, -1, 1, 1, 1], f32)  # full support: only a copy scores 12
    v = np.array([-1, -1, 1, -1, -1, 1, 1, 1, -1, -1, 1, -1], f32)
    for j in NN_DUPLICATES:
        d2[j] = u
    d2[500] = v  # the unique nearest of row 1 ...
    d2[64] = d2[257] = v * (np.arange(NN_D) != 9)  # ... and its equal seconds: a lane, and another wave's
    d2[NN_NAN_COLUMN, 3] = np.nan  # never chosen
    d2[NN_INF_COLUMN, NN_INF_ENTRY] = np.inf  # -Inf, +Inf and NaN distances down one column of the score map
    d1[NN_ROW_DUP], d1[NN_ROW_SECONDS], d1[NN_ROW_ZERO] = u, v, 0
    d1[NN_ROW_NAN, 7] = np.nan  # the whole row is NaN
    return frozen(d1), frozen(d2)


# ---- association and assembly ------------------------------------------------------------------------------------
ASM_N1, ASM_N2, ASM_M = 40, 300, 260
ASM_SAME = (3, 67, 70, 200)  # one point: the same lane's next stride, another lane, a far one
ASM_NAN_LANDMARKS = (0, 1)
ASM_ON, ASM_NEAR, ASM_NAN_KEYPOINT = 17, 18, 19  # reference keypoints on that point, one unit away, with a NaN
ASM_NAMED = {10: (31, 12, 7), 255: (20, 20, 5), 256: (39, 1, 0), 299: (8, 8, 3, 2)}  # keypoint: query rows, lowest last
ASM_LANDMARK_SETS = ("all", "one", "nan")


@functools.lru_cache(maxsize=None)
def asm_inputs():
    """(query keypoints [3, 40], reference keypoints [3, 300], points_2D [260, 2], points_3D [260, 3], matches
    [n, 2] int64) fp64; the match list is unordered, has duplicates and entries outside [0, N1) x [0, N2)."""
    rng = np.random.default_rng(20261025)
    q = np.vstack([rng.integers(4, 500, (2, ASM_N1)).astype(np.float64), np.linspace(0.9, 0.1, ASM_N1)[None]])
    r = np.vstack([rng.integers(4, 500, (2, ASM_N2)).astype(np.float64), np.linspace(0.9, 0.1, ASM_N2)[None]])
    p2 = rng.integers(0, 500, (ASM_M, 2)).astype(np.float64) + 0.5
    p3 = rng.standard_normal((ASM_M, 3)) * 10.0
    for m in ASM_SAME:
        p2[m] = (250.5, 120.5)
    for m in ASM_NAN_LANDMARKS:
        p2[m] = np.nan
    r[:2, ASM_ON] = (250.5, 120.5)
    r[:2, ASM_NEAR] = (251.5, 120.5)
    r[0, ASM_NAN_KEYPOINT] = np.nan
    m = [(int(rng.integers(ASM_N1)), int(rng.integers(ASM_N2))) for _ in range(120)]
    m = [(a, b) for a, b in m if b not in ASM_NAMED and not 11 <= b <= 15]
    for j, rows in ASM_NAMED.items():
        for k, row in enumerate(rows):
            m.insert(int(rng.integers(len(m) // 2)) if k < len(rows) - 1 else len(m), (row, j))
    m += [(-1, 12), (ASM_N1, 13), (4, ASM_N2), (5, -5), (2 ** 40, 14), (6, 2 ** 40 + 15), (7, 256), (3, 11), (3, 11)]
    return frozen(q), frozen(r), frozen(p2), frozen(p3), frozen(np.array(m, np.int64))


def asm_landmarks(which):
    """(points_2D, points_3D) of a landmark set: all 260, the first real one alone, or every landmark NaN."""
    _, _, p2, p3, _ = asm_inputs()
    if which == "one":
        return frozen(p2[2:3].copy()), frozen(p3[2:3].copy())
    if which == "nan":
        return frozen(np.full_like(p2, np.nan)), p3
    return p2, p3


# ---- the references of the cases, computed once ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plateau_ref(H, W, d, border):
    pts, kept = greedy_nms(plateau(H, W), PLATEAU_CONF, d, border)
    return frozen(pts), kept


@functools.lru_cache(maxsize=None)
def levels_ref(H, W, conf, d):
    pts, kept = greedy_nms(levels(H, W, d), conf, d, LEVEL_BORDER)
    return frozen(pts), kept


@functools.lru_cache(maxsize=None)
def nn_ref(ratio):
    return {k: frozen(v) for k, v in two_nearest_ref(*nn_inputs(), ratio).items()}


@functools.lru_cache(maxsize=None)
def asm_ref(which, with_matches):
    q, r, _, _, m = asm_inputs()
    return tuple(frozen(a) for a in assemble_ref(q, r, *asm_landmarks(which), m if with_matches else m[:0]))
