"""Shared, seeded cases of the dense-feature operators (fmpnp.conv3x3(dilation=...), fmpnp.avgpool2x2s1,
fmpnp.dense_pyramid_step, fmpnp.DenseFeatureExtractor): the shapes that cross every boundary of the kernels at the
smallest size, their operands (small integers, or Gaussians), the fp64 references and the derived error bounds.
Everything is computed once, on the CPU, and handed out read-only.

The convolution's tiles (csrc/fmpnp_encoder.hip): 128 output channels x 128 pixels per block, or 64 x 256 when
Cout <= 64; the pixel tile is TR rows x TW columns, TW a power of two: at dilation 1 the smallest that holds a row (up
to a whole 128- or 256-pixel row of one image row), at dilation 2 at most 32, so a tile is several rows tall; k
advances 4 input channels at a time.  The halo is (TR + 2 d) x (TW + 2 d)."""
import copy
import functools

import torch
from torch import nn
import torch.nn.functional as F

import fmpnp

from encoder_cases import U, guarded, guards_intact  # noqa: F401  (handed on to the tests)

# ---- the dilated convolution -----------------------------------------------------------------------------------
# (B, Cin, Cout, H, W)
CONV_SHAPES = [
    (1, 1, 1, 1, 1),        # the image is smaller than the dilated footprint: only the centre tap is on the map
    (1, 3, 5, 2, 3),        # the same with a k tail; at dilation 1 the neighbours are on the map
    (2, 5, 64, 7, 9),       # Cin no multiple of the k tile; the 64-channel form; TW = 16 below a tile: several tile
                            # rows; B = 2
    (1, 4, 65, 5, 130),     # the 128-channel form with one channel in the second tile; W crosses a 128-pixel tile (and,
                            # at dilation 2, four 32-pixel tiles): the +-2 taps read across the tile's edge
    (1, 9, 33, 19, 17),     # H exceeds TR: the taps cross a tile's top and bottom edge; two k tiles and a tail
    (3, 8, 130, 4, 260),    # three channel tiles, B = 3, a third 128-pixel column tile
    (1, 6, 40, 3, 258),     # the Cout <= 64 form's 256-pixel tile crossed by W
    (1, 2, 3, 37, 35),      # the dilated form's 8 x 32 tile (Cout <= 64) crossed in both directions, ragged in both
]
CONV_IDS = ["x".join(map(str, s)) for s in CONV_SHAPES]
DILATIONS = [1, 2]
FLAGS = [(False, False), (True, False), (True, True)]
FLAG_IDS = ["plain", "bias", "bias-relu"]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def conv_operands(shape, kind):
    """(x, weight, bias) fp32 on the CPU.  kind "int": inputs in [-2, 2], weights in [-1, 1], biases in [-3, 3], so every
    partial sum of every summation order is exact in fp32; "gauss": standard normal."""
    b, cin, cout, h, w = shape
    g = _gen(3000 * CONV_SHAPES.index(shape) + (7 if kind == "int" else 11))
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
def conv_ref64(shape, kind, d, bias, relu):
    """torch.nn.functional.conv2d in fp64 (dilation d, padding d), then the ReLU."""
    x, w, b = conv_operands(shape, kind)
    r = F.conv2d(x.double(), w.double(), b.double() if bias else None, padding=d, dilation=d)
    return torch.relu(r) if relu else r


def conv_chain_bound(x, w, b, d):
    """gamma_{K+1} (sum |a||w| + |b|) per element, K = 9 Cin, gamma_n = n u / (1 - n u), u = 2^-24: the chain's K fmaf
    roundings (taps off the map add exact zeros) and the bias add (encoder_cases.bound's derivation); the sum of
    absolute products by an fp64 conv2d of |x| with |w| at the same dilation.  The ReLU is 1-Lipschitz."""
    k1 = 9 * x.shape[1] + 1
    gamma = k1 * U / (1.0 - k1 * U)
    return gamma * F.conv2d(x.double().abs(), w.double().abs(), None if b is None else b.double().abs(), padding=d,
                            dilation=d)


@functools.lru_cache(maxsize=None)
def conv_bound(shape, kind, d, bias):
    x, w, b = conv_operands(shape, kind)
    return conv_chain_bound(x, w, b if bias else None, d)


@functools.lru_cache(maxsize=None)
def conv_twin(shape, kind, d, bias, relu):
    x, w, b = conv_operands(shape, kind)
    return fmpnp.conv3x3_cpu(x, w, b if bias else None, relu=relu, dilation=d)


def same_bits(a, b):
    """torch.equal that also takes a NaN in both for equal (the payload of a NaN is unspecified)."""
    a, b = a.cpu(), b.cpu()
    nan = torch.isnan(a)
    return bool(torch.equal(nan, torch.isnan(b))) and bool(torch.equal(a[~nan], b[~nan]))


# ---- the average pool -------------------------------------------------------------------------------------------
# (B, C, H, W)
POOL_SHAPES = [(1, 1, 2, 2), (2, 3, 5, 7), (1, 4, 9, 260), (1, 2, 2, 1000)]
POOL_IDS = ["x".join(map(str, s)) for s in POOL_SHAPES]


@functools.lru_cache(maxsize=None)
def pool_operand(shape, kind):
    g = _gen(500 + POOL_SHAPES.index(shape) + (0 if kind == "int" else 50))
    return torch.randint(-8, 9, shape, generator=g).float() if kind == "int" else torch.randn(shape, generator=g)


def pool_ref64(x):
    return F.avg_pool2d(x.double(), 2, 1)


def pool_bound(x):
    """(((a + b) + c) + d) * 0.25f: three fp32 additions, each a relative rounding of at most u, and a multiplication
    by a power of two (exact short of underflow): |error| <= gamma_3 (|a| + |b| + |c| + |d|) / 4.  The fp64 reference's
    own error is 2^-29 of that."""
    gamma3 = 3 * U / (1.0 - 3 * U)
    return gamma3 * (1 + 2.0 ** -28) * F.avg_pool2d(x.double().abs(), 2, 1)


# ---- the pyramid step ---------------------------------------------------------------------------------------------
STEP_CHANNELS = [1, 64, 65, 130]       # the 64-channel blocks of the norm: below one, one, one past, two and a tail
STEP_PAIRS = [((5, 9), (3, 5)),        # an upsize whose scales (1/2, 1/2) are dyadic: the taps are exact
              ((4, 7), (9, 13)),       # a downsize
              ((1, 1), (3, 3)),        # one texel: the scale is 0, the tap the corner
              ((6, 6), (6, 6)),        # the same size: weights 1 and 0
              ((3, 70), (2, 33)),      # a row past the kernel's 64-texel tile
              ((5, 9), None)]          # no prev: nothing is added
STEP_IDS = [f"{a[0]}x{a[1]}<-" + (f"{b[0]}x{b[1]}" if b else "none") for a, b in STEP_PAIRS]


@functools.lru_cache(maxsize=None)
def step_operands(c, pair, kind="gauss", batch=2):
    """(cur [B, C, h, w], prev [B, C, hp, wp] or None): Gaussians, or integers in [-4, 4]."""
    (h, w), p = pair
    g = _gen(9000 + 10 * c + STEP_PAIRS.index(pair) + (0 if kind == "gauss" else 5))
    make = (lambda s: torch.randn(s, generator=g)) if kind == "gauss" else (
        lambda s: torch.randint(-4, 5, s, generator=g).float())
    cur = make((batch, c, h, w))
    return cur, (make((batch, c, p[0], p[1])) if p else None)


def step_sum64(cur, prev):
    """cur + F.interpolate(prev, align_corners=True) in fp64."""
    v = cur.double()
    if prev is not None:
        v = v + F.interpolate(prev.double(), size=cur.shape[2:], mode="bilinear", align_corners=True)
    return v


def resize_bound(prev, e_prev, size):
    """A bound on |kernel's resize(prev + e) - exact resize(prev)| per plane [B, C, 1, 1], |e| <= e_prev elementwise.
    With M the plane's largest |prev| + e_prev:
      * the coordinates: scale = fl((n_in - 1) / (n_out - 1)) and src = fl(scale * d) are off by at most
        (2 u + u^2)(n_in - 1) per axis; the bilinear interpolant (constant beyond the border, where the kernel's clamp
        puts a coordinate that rounded past it) is continuous and piecewise linear with slope at most 2 M per axis, so
        the value moves by at most 2 M (2 u + u^2)((hp - 1) + (wp - 1));
      * the weights: w1 = src - i0 is exact, w0 = fl(1 - w1) one rounding;
      * the evaluation: two products and a sum per row (the two roundings of the bilerp rows after the products'),
        the same for the combine: with w0's rounding at most 7 roundings on terms whose magnitudes sum to at most M:
        gamma_7 M;
      * the operand's own error passes through a convex combination: at most the plane's largest e_prev (inside M's
        slope term too)."""
    hp, wp = prev.shape[2:]
    m = (prev.double().abs() + e_prev).amax(dim=(2, 3), keepdim=True)
    e_max = e_prev.amax(dim=(2, 3), keepdim=True) if torch.is_tensor(e_prev) else e_prev
    gamma7 = 7 * U / (1.0 - 7 * U)
    coord = 2.0 * (2 * U + U * U) * ((hp - 1) + (wp - 1))
    return (coord + gamma7) * m + e_max


def step_bound(cur, prev, e_cur=0.0, e_prev=0.0, normalize=True):
    """(the fp64 reference, a bound on |kernel - reference| per element) of dense_pyramid_step on operands known to
    within e_cur, e_prev (0: the operands themselves).
      v^ = fl(cur^ + r^):  E_v = e_cur + E_r + u (|v| + e_cur + E_r)                       (the add)
      n^ = fl32(sqrt(sum v^^2)), the sum and the root in fp64 (their error is below 2^-40 n): with ||.|| the 2-norm
           over the channels, | ||v^|| - ||v|| | <= ||E_v||, so |n^ - n| <= ||E_v|| + 2 u n, n^ >= n_lo = n (1 - 2 u)
           - ||E_v|| (which the cases keep positive and far above the clamp 1e-12)      (the fp32 norm)
      o^ = fl(v^ / n^):  |o^ - v / n| <= E_v / n_lo + |v| (||E_v|| + 2 u n) / (n n_lo) + 2 u (|v| + E_v) / n_lo
                                                                                          (the division)"""
    v = step_sum64(cur, prev)
    e_r = resize_bound(prev, e_prev, cur.shape[2:]) if prev is not None else 0.0
    e_v = e_cur + e_r + U * (v.abs() + e_cur + e_r)
    if not normalize:
        return v, e_v
    n = v.norm(dim=1, keepdim=True)
    e_n = e_v.norm(dim=1, keepdim=True)
    n_lo = n * (1 - 2 * U) - e_n
    assert bool((n_lo > 1e-6).all()), "the case's norms must stay clear of zero"
    bound = e_v / n_lo + v.abs() * (e_n + 2 * U * n) / (n * n_lo) + 2 * U * (v.abs() + e_v) / n_lo
    return v / n, bound * (1 + 1e-9)


# ---- the walk -------------------------------------------------------------------------------------------------------
WALK_WIDTHS = (4, 4, 6, 6, 8, 8, 8, 8, 8, 8)
WALK_IMAGE = (38, 52)   # scales .5 / 1 / 2: images 19 x 26, 38 x 52, 76 x 104; trunk outputs 3 x 5, 8 x 12, 18 x 25
WALK_SIZES = {0.5: (3, 5), 1: (8, 12), 2: (18, 25)}


def walk_trunk(kind="gauss"):
    """d2net_trunk at WALK_WIDTHS.  "gauss": the framework's default initialisation, seeded, with the biases drawn
    too; "pos": its magnitudes, every convolution's weights scaled to a mean gain of 1, and non-negative biases -- on a
    non-negative image no sum cancels, so sum |a||w| is the value itself and a worst-case running error bound stays a
    small multiple of u relative to the values it bounds (with signed weights it grows by sum |w|, about 4, per layer
    while the values do not: rigorous, but it would bound nothing); "int": biases in [-3, 3]; weights in [-1, 1] on
    the first two convolutions (on an image in [-2, 2]: |values| <= 57, then <= 9 * 4 * 57 + 3 = 2055), and from there on one weight of +-1 per output channel, at a random
    (input channel, tap): a signed, shifted copy, which pins the taps of every later layer, the dilated ones included,
    and lets nothing grow beyond 2055 + 8 * 3.  Every partial sum of any order is then an integer (behind the average
    pool a multiple of 1/4) far below 2^24: torch's walk is exact."""
    torch.manual_seed(41)
    net = fmpnp.d2net_trunk(WALK_WIDTHS)
    g = _gen(77)
    with torch.no_grad():
        convs = [m for m in net if isinstance(m, nn.Conv2d)]
        for k, m in enumerate(convs):
            if kind == "int":
                if k < 2:
                    m.weight.copy_(torch.randint(-1, 2, m.weight.shape, generator=g).float())
                else:
                    cout, cin = m.weight.shape[:2]
                    hot = torch.randint(0, cin * 9, (cout,), generator=g)
                    sign = torch.randint(0, 2, (cout,), generator=g).float() * 2 - 1
                    m.weight.zero_()
                    m.weight.view(cout, -1)[torch.arange(cout), hot] = sign
                m.bias.copy_(torch.randint(-3, 4, m.bias.shape, generator=g).float())
            elif kind == "pos":
                w = m.weight.abs()
                m.weight.copy_(w / w.sum(dim=(1, 2, 3)).mean())
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g).abs())
            else:
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
    return net.eval()


def walk_image(kind="gauss", size=WALK_IMAGE):
    g = _gen(78)
    if kind == "pos":
        return torch.rand((1, 3) + tuple(size), generator=g)
    if kind == "int":
        return torch.randint(-2, 3, (1, 3) + tuple(size), generator=g).float()
    return torch.randn((1, 3) + tuple(size), generator=g)


def twin_walk(net, x, relu_last=False):
    """The composition of the CPU twins over the trunk's children, by hand (no HipEncoder)."""
    children = list(net.children())
    for i, m in enumerate(children):
        if isinstance(m, nn.Conv2d):
            last = relu_last and i == len(children) - 1
            x = fmpnp.conv3x3_cpu(x, m.weight.detach(), m.bias.detach(), dilation=m.dilation[0])
            if last:
                x = fmpnp.relu_cpu(x)
        elif isinstance(m, nn.ReLU):
            x = fmpnp.relu_cpu(x)
        elif isinstance(m, nn.MaxPool2d):
            x = fmpnp.maxpool2x2_cpu(x)
        else:
            x = fmpnp.avgpool2x2s1_cpu(x)
    return x


def trunk_bound(net, x, e, relu_last):
    """(trunk(x) in fp64, a bound on |HipEncoder's walk - it| per element) for an input known to within e: a running
    error analysis, child by child.  Convolution: the incoming error passes through |w| (conv2d of e with |w|) and the
    chain adds gamma_{K+1} (sum (|a| + e)|w| + |b|); ReLU: 1-Lipschitz; max-pool: the largest error of the window;
    average pool: the window's mean error plus pool_bound on |a| + e."""
    v = x.double()
    e = torch.zeros_like(v) + e
    for m in net.children():
        if isinstance(m, nn.Conv2d):
            d = m.dilation[0]
            w, b = m.weight.detach().double(), m.bias.detach().double()
            k1 = 9 * w.shape[1] + 1
            gamma = k1 * U / (1.0 - k1 * U)
            e = F.conv2d(e, w.abs(), padding=d, dilation=d) + gamma * F.conv2d(v.abs() + e, w.abs(), b.abs(), padding=d,
                                                                               dilation=d)
            v = F.conv2d(v, w, b, padding=d, dilation=d)
        elif isinstance(m, nn.ReLU):
            v = torch.relu(v)
        elif isinstance(m, nn.MaxPool2d):
            v, e = F.max_pool2d(v, 2, 2), F.max_pool2d(e, 2, 2)
        else:
            gamma3 = 3 * U / (1.0 - 3 * U)
            e = F.avg_pool2d(e, 2, 1) + gamma3 * F.avg_pool2d(v.abs() + e, 2, 1)
            v = F.avg_pool2d(v, 2, 1)
    return (torch.relu(v) if relu_last else v), e


def extractor_bound(net, image, scales, use_relu=True):
    """(DenseFeatureExtractor(backend="torch") on the fp64 trunk, a bound on |backend="hip" - it| per element): the
    image resize's bound (resize_bound; scale 1 is the image itself), trunk_bound, then step_bound with the previous
    scale's bound, scale by scale."""
    net64 = copy.deepcopy(net).double()
    h, w = image.shape[2:]
    prev = e_prev = None
    for s in scales:
        size = (int(h * s), int(w * s))
        if size == (h, w):
            scaled, e_img = image.double(), 0.0
        else:
            scaled = F.interpolate(image.double(), size=size, mode="bilinear", align_corners=True)
            e_img = resize_bound(image, 0.0, size)
        cur, e_cur = trunk_bound(net64, scaled, e_img, use_relu)
        if prev is None:
            prev, e_prev = _normalised_bound(cur, e_cur, None, None)
        else:
            prev, e_prev = _normalised_bound(cur, e_cur, prev, e_prev)
    return prev, e_prev


def _normalised_bound(cur, e_cur, prev, e_prev):
    # (step_bound on fp64 operands: its references are formed from .double() of what it is given)
    return step_bound(cur, prev, e_cur, e_prev if e_prev is not None else 0.0)
