"""Shapes, inputs and restatements shared by the image front end's tests (test_image_cpu.py, test_gpu_image.py) and by
the fixture's generator (tests/golden/gen_image_golden.py).

The inputs are rebuilt from seeds with numpy's legacy RandomState, whose streams are frozen; the fixture
tests/golden/image_lanczos.npz holds, per (shape, kind), Pillow's Image.resize(..., Image.LANCZOS) output and the CRC-32
of the input it was computed from, so an input that came out differently is reported as such and not as a kernel's
fault.  (The inputs themselves are not in the file: with them it would pass the 256 KB it may have.)

restate_resize is a numpy restatement of the contract of include/fmpnp.h ("image front end"), written from the text and
independent of the library's code: an independent yardstick beside the recorded Pillow results.
"""
import functools
import math
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_lanczos.npz")

# (H, W, h, w): what each exercises.  The vertical pass's tile is 256 pixels x 4 rows, the horizontal pass's 64 columns x
# 16 rows: the last shape spans two and more tiles of both in each axis, with ragged last tiles (270 = 256 + 14 =
# 4 * 64 + 14, and 14 pixels are three whole threads and half of one; 70 = 17 * 4 + 2; 150 = 9 * 16 + 6).
SHAPES = [
    (37, 53, 16, 24),     # both passes
    (37, 53, 37, 20),     # horizontal pass only
    (37, 53, 11, 53),     # vertical pass only
    (40, 40, 40, 40),     # neither pass: the bytes pass through
    (23, 31, 64, 80),     # upscale, 7 taps
    (7, 5, 3, 2),         # windows clipped on both sides
    (5, 7, 1, 1),
    (96, 128, 25, 33),    # shrink 3.9, 25 taps
    (128, 96, 16, 12),    # shrink 8: the fair resampling
    (150, 300, 70, 270),  # tile edges
]
KINDS = ("random", "ramp", "binary")
CASES = [(s, k) for s in SHAPES for k in KINDS]
CASE_IDS = ["%dx%d-%dx%d-%s" % (s + (k,)) for s, k in CASES]
SHAPE_IDS = ["%dx%d-%dx%d" % s for s in SHAPES]


def key(shape, kind):
    return "%dx%d_%dx%d_%s" % (tuple(shape) + (kind,))


def make_input(hw, kind, seed=0):
    """The uint8 [H, W, 3] input of a kind: random bytes; a smooth ramp (a different direction per channel); random
    0 / 255 bytes, whose Lanczos overshoot reaches both ends of the clamp."""
    h, w = hw
    rng = np.random.RandomState(1000 * h + w + 7919 * KINDS.index(kind) + 104729 * seed)
    if kind == "random":
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "binary":
        return (rng.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    y = np.arange(h, dtype=np.float64)[:, None] / max(h - 1, 1)
    x = np.arange(w, dtype=np.float64)[None, :] / max(w - 1, 1)
    planes = [255 * (0.5 * x + 0.5 * y), 255 * (1 - x) * y + 20 * np.sin(6 * x), 255 * (0.5 + 0.5 * np.cos(3 * x + 2 * y))]
    return np.clip(np.rint(np.stack(planes, axis=2)), 0, 255).astype(np.uint8)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def fixture(shape, kind):
    """(input, Pillow's output) of a case; the input is checked against the recorded CRC."""
    g = golden()
    a = make_input(shape[:2], kind)
    k = key(shape, kind)
    assert crc(a) == int(g["crc_" + k]), f"the seeded input of {k} is not the one the fixture was recorded from"
    return a, g["out_" + k]


# ---- the numpy restatement of the contract ----
def _lanczos(t):
    def sinc(v):
        return 1.0 if v == 0.0 else math.sin(v * math.pi) / (v * math.pi)
    return sinc(t) * sinc(t / 3) if -3.0 <= t < 3.0 else 0.0


def restate_coeffs(n_in, n_out):
    """[(xmin, k[0 .. xmax))] per output sample: the contract's table of one axis."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support, ss = 3.0 * fs, 1.0 / fs
    table = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(-0.5 + v * 4194304.0) if v < 0 else int(0.5 + v * 4194304.0) for v in w]
        table.append((xmin, np.array(k, dtype=np.int64)))
    return table


def _pass(a, n_out, axis):
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + a.shape[1:], dtype=np.uint8)
    for xx, (xmin, k) in enumerate(restate_coeffs(a.shape[0], n_out)):
        acc = (1 << 21) + np.tensordot(k, a[xmin:xmin + len(k)], axes=(0, 0))
        out[xx] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def restate_resize(a, size):
    """uint8 [H, W, 3] -> [h, w, 3]: the horizontal pass if the width changes, rounded to uint8, then the vertical one."""
    h, w = size
    if w != a.shape[1]:
        a = _pass(a, w, 1)
    if h != a.shape[0]:
        a = _pass(a, h, 0)
    return a


# ---- the value transforms in torch's own CPU operations ----
TORCH_MEAN, TORCH_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CAFFE_MEAN = (103.939, 116.779, 123.68)
TRANSFORMS = ("torch", "caffe", None, "gray")


def torch_transform(u8, preprocessing, mean=None, std=None, swap_rb=True):
    """uint8 [B, H, W, 3] tensor -> float32 [B, C, H, W] by the contract's expressions, each one torch CPU operation on
    float32 tensors (true divisions, nothing fused)."""
    import torch
    f = u8.permute(0, 3, 1, 2).to(torch.float32)
    col = lambda v: torch.tensor(v, dtype=torch.float32).view(1, 3, 1, 1)  # noqa: E731
    if preprocessing == "torch":
        return ((f / 255.0) - col(mean or TORCH_MEAN)) / col(std or TORCH_STD)
    if preprocessing == "caffe":
        return f.flip(1) - col(mean or CAFFE_MEAN)
    if preprocessing is None:
        return f.contiguous()
    p = u8.to(torch.int64)
    a, b = (p[..., 2], p[..., 0]) if swap_rb else (p[..., 0], p[..., 2])
    y = (9798 * a + 19235 * p[..., 1] + 3735 * b + 16384) >> 15
    return (y.to(torch.float32) / 255.0)[:, None]


def all_bytes_image():
    """[1, 16, 48, 3] uint8: every byte value in every channel, the three channels running in different orders."""
    v = np.arange(256)
    img = np.stack([v, (v * 7 + 3) % 256, 255 - v], axis=1).reshape(16, 16, 3)
    img = np.concatenate([img, np.roll(img, 5, axis=2), img[::-1]], axis=1)
    return img.astype(np.uint8)[None]
