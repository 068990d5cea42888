"""Shared inputs of the hypercolumn assembly tests (test_hypercolumn_cpu.py, test_gpu_hypercolumn.py): the
smallest shapes that reach each branch of the kernel and its CPU twin, the PyTorch restatement of the
reference's two library calls (interpolate, torch.norm) and the tolerance derived from that restatement's own
fp32 error.  Every input is seeded; the twin's result per case is computed once and shared."""
import functools

import torch
import torch.nn.functional as F

import fmpnp

# name -> (batch, [(C, H, W) per layer], output size or None for layer 0's)
SHAPES = {
    "ragged3": (1, [(5, 9, 7), (3, 5, 4), (4, 3, 2)], None),
    "single": (1, [(7, 6, 5)], None),                         # equal size: a copy
    "blocks": (1, [(70, 4, 5), (3, 2, 3), (64, 2, 2)], None),  # blocks of 64 straddle both boundaries; 137 = 2 * 64 + 9
    "line": (1, [(4, 1, 6), (3, 3, 3)], None),                # output H = 1: the n_out == 1 scale
    "dot": (1, [(3, 3, 4), (5, 1, 1)], None),                 # a 1 x 1 source
    "down": (1, [(3, 4, 3), (4, 9, 7)], None),                # a source larger than the output
    "wide": (1, [(3, 2, 257), (2, 1, 129)], None),            # W = 257: no multiple of a tile or a vector
    "vgg16x": (1, [(128, 16, 16), (256, 8, 8), (256, 4, 4), (512, 4, 4), (512, 2, 2)], None),  # 1664 = 26 blocks
    "vec": (1, [(9, 3, 260), (66, 2, 130)], None),            # W = 260: 16-byte stores, a second, partly filled tile
    "batch3": (3, [(5, 9, 8), (3, 5, 4)], None),
    "sized": (1, [(4, 3, 5), (2, 6, 2)], (7, 4)),             # an explicit output size: layer 0 is resized too
}
VIEW_CASES = ("views",)
POISONED = ("zero_texel", "nonfinite")
ALL = tuple(SHAPES) + VIEW_CASES + POISONED


def _gen(name):
    return torch.Generator().manual_seed(sum(ord(ch) for ch in name) + 20250)


def _dense(name, batch, layers):
    g = _gen(name)
    return [torch.randn(batch, c, h, w, generator=g) for c, h, w in layers]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(feature maps (CPU float32 tensors, never modified), output size or None)."""
    if name in SHAPES:
        batch, layers, size = SHAPES[name]
        return _dense(name, batch, layers), size
    if name == "views":
        # B = 2; every source is a slice of a wider tensor: storage offset, batch, channel and row strides
        g = _gen(name)
        maps = []
        for c, h, w in [(5, 9, 8), (3, 5, 4), (4, 3, 2)]:
            big = torch.randn(3, c + 2, h + 1, w + 3, generator=g)
            maps.append(big[1:, 1:c + 1, :h, 2:2 + w])
        assert not any(m.is_contiguous() for m in maps)
        return maps, None
    if name == "zero_texel":
        # the sources' texel (0, 0) is zero in every channel: output texel (0, 0) takes that texel with weight 1
        # and its neighbours with weight 0, so it is zero in every channel and nowhere else
        maps = _dense(name, 1, SHAPES["ragged3"][1])
        for m in maps:
            m[:, :, 0, 0] = 0.0
        return maps, None
    if name == "nonfinite":
        # one NaN and one Inf, both in resized layers whose scales (4 / 8 and 2 / 8 along y, 3 / 6 along x) are
        # the same numbers in fp32 and fp64, so the restatement picks the same taps in both precisions; the Inf
        # meets taps of weight 0 (Inf * 0 = NaN) in the twin and the restatement alike.  (In an equal-size layer
        # the contract's second tap, weight 0, is the next texel; interpolate's CPU path takes the texel itself.)
        maps = _dense(name, 1, [(5, 9, 7), (3, 5, 4), (4, 3, 4)])
        maps[1][0, 1, 2, 1] = float("nan")
        maps[2][0, 3, 1, 1] = float("inf")
        return maps, None
    raise KeyError(name)


def view_out(batch, channels, height, width, device="cpu", fill=-7.0):
    """(buffer, view): a [B, C, H, W] output view that starts one float into a larger buffer, with 3 unused
    floats after every row: no 16-byte alignment anywhere."""
    buf = torch.full((1 + batch * channels * height * (width + 3) + 2,), fill, dtype=torch.float32, device=device)
    view = buf[1:1 + batch * channels * height * (width + 3)].view(batch, channels, height, width + 3)[..., :width]
    return buf, view


def ref(maps, dtype, size=None, normalize=True):
    """network.py:149-173 restated: zeros, per layer interpolate(bilinear, align_corners=True) into its channel
    slice, then the division by torch.norm(p=2, dim=1) -- in `dtype`, on the maps' device."""
    maps = [m.to(dtype) for m in maps]
    b, _, h, w = maps[0].shape
    if size is not None:
        h, w = size
    hyper = torch.zeros(b, sum(m.shape[1] for m in maps), h, w, dtype=dtype, device=maps[0].device)
    at = 0
    for m in maps:
        hyper[:, at:at + m.shape[1]] = F.interpolate(m, size=(h, w), mode="bilinear", align_corners=True)
        at += m.shape[1]
    if normalize:
        hyper = hyper / torch.norm(hyper, p=2, dim=1, keepdim=True)
    return hyper


def tolerance(ref32, ref64):
    """(bound, e_ref): e_ref = max |ref(fp32) - ref(fp64)| is the restatement's own fp32 error; a result must
    lie within 4 e_ref + 2^-23 max |ref(fp64)| of ref(fp64) -- 4x because the contract makes the same number of
    fp32 roundings in another order, the floor one fp32 rounding at the largest magnitude for the cases the
    restatement computes exactly.  Over the elements finite in both."""
    ok = torch.isfinite(ref32) & torch.isfinite(ref64)
    if not ok.any():
        return 0.0, 0.0
    e_ref = float((ref32.double() - ref64)[ok].abs().max())
    return 4.0 * e_ref + 2.0 ** -23 * float(ref64[ok].abs().max()), e_ref


def max_error(got, ref64):
    ok = torch.isfinite(got) & torch.isfinite(ref64)
    return float((got.double() - ref64)[ok].abs().max()) if ok.any() else 0.0


@functools.lru_cache(maxsize=None)
def twin(name, normalize=True):
    """The CPU twin's result of a case (computed once; read-only)."""
    maps, size = inputs(name)
    return fmpnp.assemble_hypercolumn_cpu(maps, size=size, normalize=normalize)


def same_floats(a, b):
    """Equal under == with NaNs at the same positions."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and bool((na == nb).all()) and bool((a[~na] == b[~nb]).all())


def tiny_encoder():
    """A seeded nn.Sequential: conv3->8, ReLU, pool, conv8->12, ReLU, pool, conv12->6 (children 0..6)."""
    import torch.nn as nn
    torch.manual_seed(20251)
    net = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2), nn.Conv2d(8, 12, 3, padding=1),
                        nn.ReLU(), nn.MaxPool2d(2), nn.Conv2d(12, 6, 3, padding=1))
    return net.eval()


ENCODER_LAYERS = [2, 5, 6]


def tiny_image():
    return torch.randn(1, 3, 20, 28, generator=_gen("image"))


def restated_walk(net, image):
    """network.py:134-147 in its own words: the input of children 2, 5 and 6."""
    maps, x = [], image
    with torch.no_grad():
        for i, layer in enumerate(net.children()):
            if i in ENCODER_LAYERS:
                maps.append(x)
            x = layer(x)
    return maps
