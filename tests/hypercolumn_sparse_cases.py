"""Shared inputs of the sparse-hypercolumn tests (test_hypercolumn_sparse_cpu.py, test_gpu_hypercolumn_sparse.py).

The expectation everywhere is the DENSE twin (hypercolumn_cases.twin: fmpnp_hypercolumn_assemble_cpu) indexed on
the host by the numpy restatement of the three index rules below, compared bit for bit (hc.same_floats).  The
cases are hypercolumn_cases.ALL plus "big": 70 000 channels over two layers, 280 KB of values per point, more
than gfx950's LDS holds, so the kernel must take its chunked path.  Every input is seeded and computed once."""
import functools

import numpy as np
import torch

import fmpnp
import hypercolumn_cases as hc

BIG = "big"
BIG_LAYERS = [(40000, 2, 2), (30000, 1, 1)]
ALL = tuple(hc.ALL) + (BIG,)
CELL = (4.0, 2.25)  # (cell0 for the rows, cell1 for the columns): binary fractions, so a cell edge is exact
SUBSETS = (1, 63, 64, 65, 257)


@functools.lru_cache(maxsize=None)
def inputs(name):
    if name == BIG:
        g = torch.Generator().manual_seed(20252)
        return [torch.randn(1, c, h, w, generator=g) for c, h, w in BIG_LAYERS], None
    return hc.inputs(name)


@functools.lru_cache(maxsize=None)
def dense(name, normalize=True):
    """The dense twin's [B, C, H, W] map of a case (read-only)."""
    if name == BIG:
        maps, size = inputs(name)
        return fmpnp.assemble_hypercolumn_cpu(maps, size=size, normalize=normalize)
    return hc.twin(name, normalize)


def shape(name):
    return tuple(dense(name).shape)


# ---- the index rules, restated in numpy ---------------------------------------------------------------------

def index_texel(tex, H, W):
    tex = np.asarray(tex, np.int64).reshape(-1, 2)
    ok = (tex[:, 0] >= 0) & (tex[:, 0] < H) & (tex[:, 1] >= 0) & (tex[:, 1] < W)
    return np.where(ok, tex[:, 0], 0), np.where(ok, tex[:, 1], 0), ok


def index_reference(pts, H, W, img0, img1):
    """gather_ref_kernel's rule: col = trunc(H / img0 * x), row = trunc(W / img1 * y) (the swap is the
    reference's), one wrap of a negative index, everything else outside the map and NaN an error."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        colf, rowf = float(H) / float(img0) * pts[:, 0], float(W) / float(img1) * pts[:, 1]
        finite = np.isfinite(colf) & np.isfinite(rowf) & (np.abs(colf) < 2.0 ** 31) & (np.abs(rowf) < 2.0 ** 31)
        col = np.trunc(np.where(finite, colf, 0.0)).astype(np.int64)
        row = np.trunc(np.where(finite, rowf, 0.0)).astype(np.int64)
    row = np.where((row < 0) & (row >= -H), row + H, row)
    col = np.where((col < 0) & (col >= -W), col + W, col)
    ok = finite & (row >= 0) & (row < H) & (col >= 0) & (col < W)
    return np.where(ok, row, 0), np.where(ok, col, 0), ok


def index_cell(pts, H, W, cell0, cell1):
    """nearest_cell's rule per axis: clip(ceil(p / cell - 1), 0, n - 1), NaN -> 0; never an error."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)

    def axis(p, cell, n):
        with np.errstate(invalid="ignore"):
            c = np.ceil(p / cell - 1.0)
        c = np.where(np.isnan(c), 0.0, c)
        return np.clip(c, 0, n - 1).astype(np.int64)
    return axis(pts[:, 1], cell0, H), axis(pts[:, 0], cell1, W), np.ones(len(pts), bool)


def expected(name, item, row, col, ok, normalize=True, dtype=torch.float32):
    """The dense twin at the points; error rows are zero."""
    d = dense(name, normalize)
    B = d.shape[0]
    item = np.zeros(len(row), np.int64) if item is None else np.asarray(item, np.int64)
    ok = np.asarray(ok) & (item >= 0) & (item < B)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int64))  # noqa: E731
    rows = d[t(np.where(ok, item, 0)), :, t(row), t(col)].clone()
    rows[torch.from_numpy(~ok)] = 0.0
    return rows.to(dtype), ok


# ---- the points ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def all_texels(name):
    """Every texel of every item once: (tex int32 [N, 2], item int32 [N]), items interleaved (mixed order)."""
    B, _, H, W = shape(name)
    b, r, c = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    order = np.random.Generator(np.random.PCG64(7)).permutation(B * H * W)
    tex = np.stack([r.reshape(-1), c.reshape(-1)], 1).astype(np.int32)[order]
    return tex, b.reshape(-1).astype(np.int32)[order]


def image_shape(name):
    """(img0, img1) for at="reference": with the swapped rule col = H / img0 * x and row = W / img1 * y, this
    choice makes both factors 1 / 4, so x in [0, 4 W) and y in [0, 4 H) stay in a non-square map."""
    _, _, H, W = shape(name)
    return 4 * H, 4 * W


def cell_resolution(name):
    """The image_resolution whose generate_dense_keypoints cell sizes are CELL on this case's map."""
    _, _, H, W = shape(name)
    return CELL[0] * H, CELL[1] * W


@functools.lru_cache(maxsize=None)
def good_points(name, mode, n=40):
    """Seeded fp64 points inside the map for "reference" / "cell", the deliberate specials first: the four
    corners, a duplicate, a point exactly on a cell edge (the lower cell; for "reference" exactly on a texel
    edge), a negative coordinate that wraps ("reference") or clips ("cell"), coordinates just inside the last
    texel.  (pts [N, 2], item [N])."""
    B, _, H, W = shape(name)
    sx, sy = (4.0, 4.0) if mode == "reference" else (CELL[1], CELL[0])
    xmax, ymax = sx * W, sy * H
    eps = 1e-9
    special = [(0.0, 0.0), (xmax - eps, 0.0), (0.0, ymax - eps), (xmax - eps, ymax - eps),
               (0.0, 0.0),                                   # a duplicate
               (sx * min(2, W), sy * min(1, H)),             # exactly on an edge
               (-1.5 * sx, 0.25 * sy),                       # wraps to the last column / clips to the first
               (np.nextafter(xmax, 0.0), np.nextafter(ymax, 0.0))]
    if mode == "reference":  # (x = sx * W is out of the map there: keep the edge point inside)
        special[5] = (sx * min(2, W - 1), sy * min(1, H - 1))
    rng = np.random.Generator(np.random.PCG64(sum(ord(c) for c in name + mode)))
    rand = np.stack([rng.uniform(0.0, xmax, n), rng.uniform(0.0, ymax, n)], 1)
    pts = np.concatenate([np.array(special, np.float64), rand])
    item = rng.integers(0, B, len(pts)).astype(np.int32)
    item[:B] = np.arange(B)[::-1]  # every item, in mixed order
    return pts, item


def bad_points(name):
    """at="reference" points that must be error rows: right of the map, below it, beyond the wrap, NaN, huge."""
    _, _, H, W = shape(name)
    return np.array([(4.0 * W + 1.0, 0.0), (0.0, 4.0 * H), (-4.0 * W - 4.0, 0.0), (np.nan, 1.0), (1.0, np.nan),
                     (1e300, 0.0), (0.0, -1e300)], np.float64)


def index(name, mode, pts):
    _, _, H, W = shape(name)
    if mode == "texel":
        return index_texel(pts, H, W)
    if mode == "reference":
        return index_reference(pts, H, W, *image_shape(name))
    return index_cell(pts, H, W, *CELL)


def kwargs(name, mode):
    """sparse_hypercolumn's keyword arguments of a mode on this case."""
    _, size = inputs(name)
    kw = dict(at=mode, size=size)
    if mode == "reference":
        kw["image_shape"] = image_shape(name)
    elif mode == "cell":
        kw["cell_size"] = CELL
    return kw
