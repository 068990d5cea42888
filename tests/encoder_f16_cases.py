"""Shared, seeded cases of the encoder's fp16 precision (fmpnp.conv3x3(..., precision="f16")): encoder_cases' shapes
plus the smallest ones that cross the fp16 kernel's own edges, operands without fp16 subnormals, the fp64 references on
the rounded operands, the contract's bound (include/fmpnp.h, "the encoder's fp16 precision"), the conversion values
and an integer net whose activations stay exact in fp16.  Everything is computed once and handed out read-only."""
import functools

import torch
from torch import nn

import encoder_cases as ec

# The fp16 kernel's k tile is 16 input channels (one 16-deep MFMA step per tap): Cin one below, at and one above it
# (17 is also one past a 16-deep step); Cout = 3 and 2 x 5 pixels keep them tiny.
K_TILE = 16
EDGE_SHAPES = [(1, K_TILE - 1, 3, 2, 5), (1, K_TILE, 3, 2, 5), (1, K_TILE + 1, 3, 2, 5)]
SHAPES = list(ec.SHAPES) + EDGE_SHAPES
IDS = ["x".join(map(str, s)) for s in SHAPES]
FLAGS = [(False, False), (True, False), (False, True), (True, True)]  # (bias, relu)
FLAG_IDS = ["plain", "bias", "relu", "bias-relu"]
TINY = 2.0 ** -14  # the smallest fp16 normal


def _gen(shape, kind):
    return torch.Generator().manual_seed(77000 + 1000 * SHAPES.index(shape) + (7 if kind == "int" else 11))


@functools.lru_cache(maxsize=None)
def operands(shape, kind):
    """(x, weight, bias) fp32 on the CPU.  "int": inputs in [-2, 2], weights in [-1, 1], biases in [-3, 3]: exact in
    fp16, every partial sum of every order exact in fp32.  "gauss": standard normal with every |v| < 2^-14 of the
    inputs and the weights set to 0 (fp16-subnormal operands are unspecified; they do occur in randn at these sizes)."""
    if shape in ec.SHAPES:
        x, w, b = ec.operands(shape, kind)
    else:
        bsz, cin, cout, h, wd = shape
        g = _gen(shape, kind)
        if kind == "int":
            x = torch.randint(-2, 3, (bsz, cin, h, wd), generator=g).float()
            w = torch.randint(-1, 2, (cout, cin, 3, 3), generator=g).float()
            b = torch.randint(-3, 4, (cout,), generator=g).float()
        else:
            x = torch.randn((bsz, cin, h, wd), generator=g)
            w = torch.randn((cout, cin, 3, 3), generator=g)
            b = torch.randn((cout,), generator=g)
    if kind == "gauss":
        x = torch.where(x.abs() < TINY, torch.zeros_like(x), x)
        w = torch.where(w.abs() < TINY, torch.zeros_like(w), w)
    return x, w, b


def k_padded(cin):
    """K_p = 16 * 9 * ceil(Cin / 16): the products an output's MFMA steps hold."""
    return 16 * 9 * ((cin + 15) // 16)


@functools.lru_cache(maxsize=None)
def sum64(shape, kind):
    """s: torch's fp64 conv2d (padding 1) of the operands rounded to fp16, without the bias."""
    x, w, _ = operands(shape, kind)
    return torch.nn.functional.conv2d(x.half().double(), w.half().double(), padding=1)


@functools.lru_cache(maxsize=None)
def mag64(shape, kind):
    """sum |fl16(a)| |fl16(w)| per output, in fp64."""
    x, w, _ = operands(shape, kind)
    return torch.nn.functional.conv2d(x.half().double().abs(), w.half().double().abs(), padding=1)


def ref64(shape, kind, bias, relu):
    """The exact value: s (+ b), then the ReLU."""
    r = sum64(shape, kind)
    if bias:
        r = r + operands(shape, kind)[2].double().view(1, -1, 1, 1)
    return torch.relu(r) if relu else r


def rounding_terms(shape, kind, bias):
    """2^-24 |s| + 2^-24 |s + b|: the reference's one rounding of the sum and the fp32 bias add (the second term only
    with a bias; without one the contract's 2^-24 |s + b| is still granted to the GPU side, see gpu_bound)."""
    s = sum64(shape, kind)
    t = ec.U * s.abs()
    if bias:
        t = t + ec.U * (s + operands(shape, kind)[2].double().view(1, -1, 1, 1)).abs()
    return t


def gpu_bound(shape, kind, bias):
    """|gpu - reference| <= K_p 2^-23 sum |fl16(a)| |fl16(w)| + 2^-24 |s| + 2^-24 |s + b| (the contract; b = 0 without
    a bias).  The ReLU is 1-Lipschitz: the same bound holds behind it."""
    s = sum64(shape, kind)
    sb = s + operands(shape, kind)[2].double().view(1, -1, 1, 1) if bias else s
    return k_padded(shape[1]) * 2.0 ** -23 * mag64(shape, kind) + ec.U * s.abs() + ec.U * sb.abs()


def reference_bound(shape, kind, bias):
    """|reference - fp64 conv2d on the rounded operands| (before or behind the ReLU): the two fp32 roundings above
    plus one fp64-order term: the reference and conv2d each sum the K = 9 Cin exact products in fp64 in an order of
    their own, each within K 2^-53 sum |a||w| of the true sum; and 2^-47 sum |a||w| for the second-order terms of the
    two fp32 roundings (they are taken of values that already carry the errors before them)."""
    return rounding_terms(shape, kind, bias) + (2 * 9 * shape[1] * 2.0 ** -53 + 2.0 ** -47) * mag64(shape, kind)


@functools.lru_cache(maxsize=None)
def reference(shape, kind, bias, relu):
    import fmpnp
    x, w, b = operands(shape, kind)
    return fmpnp.conv3x3_cpu(x, w, b if bias else None, relu=relu, precision="f16")


# ---- the conversion: value -> fl16(value), checked with torch.half ----
_CONV_POS = [
    (1.0 + 2.0 ** -11, 1.0),                                   # a tie: to even, down
    (1.0 + 2.0 ** -11 + 2.0 ** -23, 1.0 + 2.0 ** -10),          # just above the tie: up
    (1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -9),                    # a tie: to even, up
    (65504.0, 65504.0),                                        # the largest fp16
    (65519.99609375, 65504.0),                                 # the largest fp32 below the overflow threshold
    (2.0 ** -14, 2.0 ** -14),                                  # the smallest normal
]
CONVERSIONS = _CONV_POS + [(-v, -r) for v, r in _CONV_POS]


# ---- the walk on integers that stay exact in fp16: conv-ReLU-conv-ReLU-pool-conv, 3 -> 3 -> 3 -> 4 channels ----
# |inputs| <= 2, then 9 * 3 * 2 + 3 = 57, then 9 * 3 * 57 + 3 = 1542 <= 2048 (every integer up to 2048 is an fp16
# value), and the last sums stay below 9 * 3 * 1542 + 3 < 2^24: exact in fp32 in any order.
def int_net(inplace):
    g = torch.Generator().manual_seed(123)
    layers = [nn.Conv2d(3, 3, 3, padding=1), nn.ReLU(inplace=inplace), nn.Conv2d(3, 3, 3, padding=1),
              nn.ReLU(inplace=inplace), nn.MaxPool2d(2, 2), nn.Conv2d(3, 4, 3, padding=1)]
    with torch.no_grad():
        for m in layers:
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(torch.randint(-1, 2, m.weight.shape, generator=g).float())
                m.bias.copy_(torch.randint(-3, 4, m.bias.shape, generator=g).float())
    return nn.Sequential(*layers).eval()


def int_batch():
    return torch.randint(-2, 3, (2, 3, 6, 10), generator=torch.Generator().manual_seed(6)).float()


def chained(net, batch, conv, relu, pool):
    """The net's children through the given operators, one call per child (no fusion); the last output."""
    x = batch
    for m in net.children():
        if isinstance(m, nn.Conv2d):
            x = conv(x, m.weight.detach().contiguous(), m.bias.detach().contiguous(), precision="f16")
        elif isinstance(m, nn.ReLU):
            x = relu(x)
        else:
            x = pool(x)
    return x
