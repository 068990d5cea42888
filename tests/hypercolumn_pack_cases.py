"""Shared inputs of the fused hypercolumn pack's tests (test_hypercolumn_pack_cpu.py, test_gpu_hypercolumn_pack.py):
every case of hypercolumn_cases (every batch item of the batched ones), the few shapes the pack's tiling adds, and
the numpy restatement of the composed path -- assemble_hypercolumn_cpu's map, the Sobel in the Sobel pack's fp64
association for fp32 maps, one rounding to the storage type, the channels moved last.  Every comparison made with
these is an equality (NaNs by position)."""
import functools

import numpy as np
import torch

import fmpnp

import hypercolumn_cases as hc

# name -> (batch, [(C, H, W) per layer], output size or None): what the tiles of 64 channels x 32 columns x rs rows need
SHAPES = {
    "cols33": (1, [(5, 3, 33), (3, 2, 17)], None),  # W = 33: the halo crosses a column-tile edge, a one-column last tile
    "rows": (1, [(4, 19, 4), (3, 10, 2)], None),    # H = 19: row-tile edges whatever rows-per-tile the host picks
    "one": (1, [(3, 1, 1), (2, 2, 2)], None),       # a 1 x 1 output: every neighbour is padding
    "c30": (1, [(20, 6, 5), (10, 3, 3)], None),     # 30 channels: cstride 32 > C
}
ALL = tuple(hc.ALL) + tuple(SHAPES)
SENTINEL = -7.0
FLAG_PAIRS = [(False, False), (True, False), (False, True), (True, True)]  # (sobel_normalized, sobel_replicate_pad)
DTYPES = {torch.float32: np.float32, torch.float64: np.float64}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(feature maps (CPU float32 tensors, never modified), output size or None)."""
    if name in SHAPES:
        batch, layers, size = SHAPES[name]
        g = torch.Generator().manual_seed(sum(ord(ch) for ch in name) + 20260)
        return [torch.randn(batch, c, h, w, generator=g) for c, h, w in layers], size
    return hc.inputs(name)


def items(name):
    return range(int(inputs(name)[0][0].shape[0]))


@functools.lru_cache(maxsize=None)
def dense(name, normalize=True):
    """assemble_hypercolumn_cpu's map of the case, [B, C, H, W] float32 numpy (computed once; read-only)."""
    maps, size = inputs(name)
    out = fmpnp.assemble_hypercolumn_cpu(maps, size=size, normalize=normalize).numpy()
    out.setflags(write=False)
    return out


def shape(name):
    """(C, H, W, cstride) of the case's hypercolumn."""
    _, C, H, W = dense(name).shape
    return C, H, W, (C + 3) // 4 * 4


@functools.lru_cache(maxsize=None)
def restated(name, item=0, normalize=True, layout="fgrad", sobel_normalized=False, replicate=False,
             storage=torch.float32):
    """The composed path in numpy: [H][W][3][cstride] (f, gx, gy) or [H][W][cstride], padding channels zero."""
    m32 = dense(name, normalize)[item]
    C, H, W = m32.shape
    cs = (C + 3) // 4 * 4
    dt = DTYPES[storage]
    f = np.moveaxis(m32, 0, -1)
    if layout == "f":
        out = np.zeros((H, W, cs), np.float32)
        out[:, :, :C] = f
        out.setflags(write=False)
        return out
    with np.errstate(all="ignore"):
        p = np.pad(m32.astype(np.float64), ((0, 0), (1, 1), (1, 1)), mode="edge" if replicate else "constant")
        a, d, g = p[:, :-2, :], p[:, 1:-1, :], p[:, 2:, :]  # rows y - 1, y, y + 1 at columns -1 .. W
        sx, sy = (a + 2.0 * d) + g, g - a
        gx = sx[:, :, 2:] - sx[:, :, :-2]
        gy = (sy[:, :, :-2] + 2.0 * sy[:, :, 1:-1]) + sy[:, :, 2:]
        if sobel_normalized:
            gx, gy = gx * 0.125, gy * 0.125
        out = np.zeros((H, W, 3, cs), dt)
        out[:, :, 0, :C] = f.astype(dt)
        out[:, :, 1, :C] = np.moveaxis(gx, 0, -1).astype(dt)
        out[:, :, 2, :C] = np.moveaxis(gy, 0, -1).astype(dt)
    out.setflags(write=False)
    return out


def expected(name, item, channels=None, marks=None, fill=SENTINEL, **kw):
    """What a buffer prefilled with `fill` must hold afterwards: the restatement in channels [c_begin, c_end) of the
    marked texels, the fill everywhere else (padding channels included)."""
    want = restated(name, item, **kw)
    C = shape(name)[0]
    c0, c1 = (0, C) if channels is None else channels
    out = np.full_like(want, fill)
    sel = np.ones(want.shape[:2], bool) if marks is None else np.asarray(marks).astype(bool)
    out[sel, ..., c0:c1] = want[sel, ..., c0:c1]
    return out


def same(a, b):
    return hc.same_floats(torch.from_numpy(np.array(a)), torch.from_numpy(np.array(b)))  # (copies: read-only inputs)


def random_marks(name, seed=5, density=0.3):
    _, H, W, _ = shape(name)
    g = np.random.default_rng(seed + sum(ord(ch) for ch in name))
    return (g.random((H, W)) < density).astype(np.uint8)


def single_mark(name):
    _, H, W, _ = shape(name)
    m = np.zeros((H, W), np.uint8)
    m[H // 2, W - 1] = 1
    return m


MARK_KINDS = ("random", "zero", "single")


def marks_of(name, kind):
    if kind is None:
        return None
    if kind == "zero":
        return np.zeros(shape(name)[1:3], np.uint8)
    return random_marks(name) if kind == "random" else single_mark(name)


@functools.lru_cache(maxsize=None)
def twin(name, item=0, normalize=True, layout="fgrad", sobel_normalized=False, replicate=False,
         storage=torch.float32, channels=None, marks=None):
    """The CPU twin's buffer of a case, packed into one prefilled with the sentinel (computed once; read-only).
    marks: None or one of MARK_KINDS."""
    maps, size = inputs(name)
    _, H, W, cs = shape(name)
    out = np.full((H, W, 3, cs) if layout == "fgrad" else (H, W, cs), SENTINEL, DTYPES[storage])
    fmpnp.pack_hypercolumn_cpu(maps, size=size, normalize=normalize, item=item, storage=storage, layout=layout,
                               sobel_normalized=sobel_normalized, sobel_replicate_pad=replicate, channels=channels,
                               marks=marks_of(name, marks), out=out)
    out.setflags(write=False)
    return out


# the channel ranges beyond the whole map: (case, (c_begin, c_end))
RANGES = [("blocks", (5, 100)), ("blocks", (70, 71)), ("vgg16x", (640, 1664)), ("vgg16x", (128, 640)),
          ("vgg16x", (0, 128)), ("c30", (7, 30))]
