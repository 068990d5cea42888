"""Shared, seeded cases of the encoder's operators (fmpnp/encoder.py): the convolution shapes that cross every
boundary of the kernel at the smallest size, their operands (small integers, or Gaussians), the fp64 references
and the chain's derived error bound, the three-conv integer net of the walk tests and the VGG-16 topology at small
widths.  Everything is computed once and handed out read-only."""
import copy
import functools

import torch
from torch import nn

import fmpnp

# (B, Cin, Cout, H, W)
SHAPES = [
    (1, 3, 5, 5, 7),        # K = 27: a k tail; everything ragged
    (1, 1, 1, 1, 1),        # only the centre tap is inside
    (2, 33, 130, 3, 131),   # crosses the k tile, the Cout tile and the pixel tile; rows shorter than the halo
    (1, 8, 64, 2, 258),     # two pixel tiles plus a remainder
    (3, 4, 4, 9, 4),        # W far below a tile: several rows per tile
    (1, 2, 65, 3, 5),       # one output channel past the 64 up to which the kernel takes its 64 x 256 form
]
IDS = ["x".join(map(str, s)) for s in SHAPES]
U = 2.0 ** -24


def _gen(shape, kind):
    return torch.Generator().manual_seed(1000 * SHAPES.index(shape) + (7 if kind == "int" else 11))


@functools.lru_cache(maxsize=None)
def operands(shape, kind):
    """(x, weight, bias) fp32 on the CPU.  kind "int": inputs in [-2, 2], weights in [-1, 1], biases in [-3, 3],
    so every partial sum of every summation order is exact in fp32; "gauss": standard normal."""
    b, cin, cout, h, w = shape
    g = _gen(shape, kind)
    if kind == "int":
        x = torch.randint(-2, 3, (b, cin, h, w), generator=g).float()
        wt = torch.randint(-1, 2, (cout, cin, 3, 3), generator=g).float()
        bias = torch.randint(-3, 4, (cout,), generator=g).float()
    else:
        x = torch.randn((b, cin, h, w), generator=g)
        wt = torch.randn((cout, cin, 3, 3), generator=g)
        bias = torch.randn((cout,), generator=g)
    return x, wt, bias


@functools.lru_cache(maxsize=None)
def ref64(shape, kind, bias, relu):
    """torch.nn.functional.conv2d in fp64 (padding 1), then the ReLU."""
    x, w, b = operands(shape, kind)
    r = torch.nn.functional.conv2d(x.double(), w.double(), b.double() if bias else None, padding=1)
    return torch.relu(r) if relu else r


@functools.lru_cache(maxsize=None)
def bound(shape, kind, bias):
    """The chain's bound per element: gamma * (sum |a||w| + |b|), gamma = (K + 1) u / (1 - (K + 1) u), K = 9 Cin,
    u = 2^-24: K fmaf roundings and the bias add; the sum of absolute products by an fp64 conv2d of |x| with |w|."""
    x, w, b = operands(shape, kind)
    k1 = 9 * shape[1] + 1
    gamma = k1 * U / (1.0 - k1 * U)
    mag = torch.nn.functional.conv2d(x.double().abs(), w.double().abs(), b.double().abs() if bias else None, padding=1)
    return gamma * mag


@functools.lru_cache(maxsize=None)
def twin(shape, kind, bias, relu):
    x, w, b = operands(shape, kind)
    return fmpnp.conv3x3_cpu(x, w, b if bias else None, relu=relu)


def guarded(shape, device, pad=64):
    """A contiguous tensor of `shape` inside a larger NaN-filled buffer -> (buffer, view, pad): a store outside the
    tensor lands on a NaN that the caller can find gone."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * pad,), float("nan"), device=device)
    return buf, buf[pad:pad + n].view(shape), pad


def guards_intact(buf, pad):
    return bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[-pad:]).all())


# ---- the walk: conv-ReLU-conv-ReLU-pool-conv on integers (3 -> 8 -> 8 -> 6 channels) ----
# |values| <= 2, then 9 * 3 * 2 + 3 = 57, then 9 * 8 * 57 + 3 = 4107, then 9 * 8 * 4107 + 3 < 2^19: every partial
# sum of any summation order is an integer below 2^24, exact in fp32, so torch's walk is exact on any backend.
def walk_net(inplace):
    g = torch.Generator().manual_seed(99)
    layers = [nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(inplace=inplace), nn.Conv2d(8, 8, 3, padding=1),
              nn.ReLU(inplace=inplace), nn.MaxPool2d(2, 2), nn.Conv2d(8, 6, 3, padding=1)]
    with torch.no_grad():
        for m in layers:
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(torch.randint(-1, 2, m.weight.shape, generator=g).float())
                m.bias.copy_(torch.randint(-3, 4, m.bias.shape, generator=g).float())
    return nn.Sequential(*layers).eval()


def walk_batch():
    return torch.randint(-2, 3, (2, 3, 6, 10), generator=torch.Generator().manual_seed(5)).float()


WALK_TAPS = [[0], [1], [2], [3], [4], [5], [1, 3], [0, 1, 2, 3, 4, 5], [2, 4], [3, 5]]


def torch_walk(net, batch, taps):
    """The reference's own loop (network.py:134-147) on a private copy of the net and the batch."""
    net, fm = copy.deepcopy(net), batch.clone()
    maps, j = [], 0
    with torch.no_grad():
        for i, layer in enumerate(net.children()):
            if j == len(taps):
                break
            if i == taps[j]:
                maps.append(fm)
                j += 1
            fm = layer(fm)
    return maps


# ---- the topology: VGG-16's features[:-2], 29 children ending in a bare convolution ----
# the widths of the eleven convolutions up to child 24 (the last tap); the two behind it keep the last width, as
# VGG-16's own last block does
VGG_WIDTHS = (8, 8, 16, 16, 24, 24, 24, 40, 40, 40, 40, 40, 40)
VGG_BLOCKS = (2, 2, 3, 3, 3)
VGG_TAPS = [9, 14, 17, 21, 24]


def vgg16_topology(seed=3):
    torch.manual_seed(seed)
    layers, cin, widths = [], 3, iter(VGG_WIDTHS)
    for n in VGG_BLOCKS:
        for _ in range(n):
            cout = next(widths)
            layers += [nn.Conv2d(cin, cout, 3, padding=1), nn.ReLU(inplace=True)]
            cin = cout
        layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
    layers = layers[:-2]
    assert len(layers) == 29 and isinstance(layers[-1], nn.Conv2d)
    return nn.Sequential(*layers).eval()


def vgg_batch():
    return torch.randn((2, 3, 32, 32), generator=torch.Generator().manual_seed(17))


@functools.lru_cache(maxsize=None)
def vgg_twin_maps():
    """The twin's maps at VGG_TAPS (an encoder on the CPU runs the twins)."""
    return tuple(fmpnp.HipEncoder(vgg16_topology()).feature_maps(vgg_batch(), VGG_TAPS))
