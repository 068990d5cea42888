"""Shared, seeded cases of the 1x1 convolution (fmpnp.conv1x1, fmpnp.conv1x1_cpu): the shapes that cross every
boundary of the kernel at the smallest size, their operands (small integers, or Gaussians), the fp64 references and
the chain's derived error bound.  Everything is computed once and handed out read-only.

The kernel's tiles (csrc/fmpnp_conv1x1.hip): 128 output channels x 128 flat pixels per block, or 64 x 256 when
Cout <= 64; k advances 32 input channels at a time; the input tile is loaded 16 bytes at a time when H * W % 4 == 0
(and the base pointer allows), 4 bytes otherwise."""
import functools

import torch

import fmpnp

from encoder_cases import U, guarded, guards_intact  # noqa: F401  (handed on to the tests)

# (B, Cin, Cout, H, W); P = H * W
SHAPES = [
    (1, 1, 1, 1, 1),        # the minimum: one real element in every tile
    (1, 3, 5, 5, 7),        # everything ragged; P = 35: the 4-byte path, a k tail of 3, the 64 x 256 form
    (2, 33, 130, 3, 131),   # one channel past the 32-channel k tile, two past the 128-channel tile, P = 393: four
                            # 128-pixel tiles with a tail; P odd, so image 1's planes are misaligned (4-byte path)
    (1, 8, 64, 2, 258),     # the Cout <= 64 form at its last width: two 256-pixel tiles plus 4; P % 4 == 0: the
                            # 16-byte path
    (1, 2, 65, 3, 5),       # one output channel past 64: the 128 x 128 form
    (3, 70, 4, 9, 4),       # two k tiles and a tail of 6, B = 3, P = 36: the 16-byte path with a partial tile
    (1, 256, 65, 2, 3),     # convPb's channel counts on a 16 x 24 image's map: eight full k tiles
    (1, 256, 256, 2, 3),    # convDb's: two channel tiles, both full
    (1, 5, 66, 4, 33),      # the 128 x 128 form on the 16-byte path (the heads' own at 1024 x 1024): P = 132, one
                            # 128-pixel tile plus 4
]
IDS = ["x".join(map(str, s)) for s in SHAPES]
FLAGS = [(False, False), (True, False), (False, True), (True, True)]
FLAG_IDS = ["plain", "bias", "relu", "bias-relu"]


def _gen(shape, kind):
    return torch.Generator().manual_seed(2000 * SHAPES.index(shape) + (7 if kind == "int" else 11))


@functools.lru_cache(maxsize=None)
def operands(shape, kind):
    """(x, weight [Cout, Cin, 1, 1], bias) fp32 on the CPU.  kind "int": inputs in [-2, 2], weights in [-1, 1],
    biases in [-3, 3], so every partial sum of every order stays at or below 2 * 256 + 3 and is exact in fp32;
    "gauss": standard normal."""
    b, cin, cout, h, w = shape
    g = _gen(shape, kind)
    if kind == "int":
        x = torch.randint(-2, 3, (b, cin, h, w), generator=g).float()
        wt = torch.randint(-1, 2, (cout, cin, 1, 1), generator=g).float()
        bias = torch.randint(-3, 4, (cout,), generator=g).float()
    else:
        x = torch.randn((b, cin, h, w), generator=g)
        wt = torch.randn((cout, cin, 1, 1), generator=g)
        bias = torch.randn((cout,), generator=g)
    return x, wt, bias


@functools.lru_cache(maxsize=None)
def ref64(shape, kind, bias, relu):
    """torch.nn.functional.conv2d in fp64 on the CPU, then the ReLU."""
    x, w, b = operands(shape, kind)
    r = torch.nn.functional.conv2d(x.double(), w.double(), b.double() if bias else None)
    return torch.relu(r) if relu else r


def chain_bound(x, w, b, k):
    """gamma_{k+1} (sum |a||w| + |b|) per element, gamma_n = n u / (1 - n u), u = 2^-24: k fmaf roundings and the
    bias add (encoder_cases.bound's derivation); the sum of absolute products by an fp64 conv2d of |x| with |w|.
    For any kernel size: padding is the weight's own."""
    gamma = (k + 1) * U / (1.0 - (k + 1) * U)
    pad = w.shape[-1] // 2
    mag = torch.nn.functional.conv2d(x.double().abs(), w.double().abs(), None if b is None else b.double().abs(),
                                     padding=pad)
    return gamma * mag


@functools.lru_cache(maxsize=None)
def bound(shape, kind, bias):
    """The chain's bound per element with K = Cin."""
    x, w, b = operands(shape, kind)
    return chain_bound(x, w, b if bias else None, shape[1])


@functools.lru_cache(maxsize=None)
def twin(shape, kind, bias, relu):
    x, w, b = operands(shape, kind)
    return fmpnp.conv1x1_cpu(x, w, b if bias else None, relu=relu)
