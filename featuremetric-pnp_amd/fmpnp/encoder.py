"""The encoder on the GPU (opt-in): 3x3 convolution, ReLU and 2x2 max-pool, the three operators VGG-16's
features[:-2] (s2dhm/network/network.py:47-51) is made of, as libfmpnp's kernels (include/fmpnp.h, "the encoder's
operators", states the numeric contract).

conv3x3 is an exact-fp32 implicit GEMM on the matrix cores: every output is one fmaf chain over the weight's own
flat order, so its bits depend on its operands only, never on the batch, the tile, the stream or the machine's
choice of algorithm.  conv3x3_cpu, relu_cpu and maxpool2x2_cpu are the CPU twins (bit-identical results; explicit
entry points, never a fallback).  conv1x1 and conv1x1_cpu are the same chain for a 1x1 / padding 0 convolution
(SuperPoint's heads; fmpnp/superpoint.py's HipSuperPointNet walks that network through these operators; HipEncoder
takes no 1x1 child).  precision="f16" (opt-in, everywhere "f32" by default) runs the convolution on
the fp16 matrix cores instead: operands rounded to binary16, fp32 accumulation in a fixed order, a stated error
bound against conv3x3_cpu(precision="f16"), which is its reference and not a twin (include/fmpnp.h, "the encoder's
fp16 precision").  HipEncoder runs an nn.Sequential of such layers through them and reproduces the
layer walk of network.py:134-147; HypercolumnExtractor(backend="hip") routes its walk through one.

conv3x3(..., dilation=2) is the same chain with the taps two texels apart and padding 2 (fmpnp_conv3x3_dilated; exact
fp32 only), avgpool2x2s1 the 2x2 / stride 1 average pool: with them HipEncoder also walks a D2-Net style trunk (VGG-16
to conv4_3 with pool3 an AvgPool2d(2, stride=1) and conv4 dilated by 2; fmpnp/dense.py builds the dense features on
it).
"""
import ctypes

import torch
from torch import nn

from . import _lib


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _tensor4(x, name, kind):
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError(f"{name} must be a 4-D tensor [B, C, H, W]")
    if x.dtype != torch.float32 or x.device.type != kind:
        raise ValueError(f"{name} must be a float32 {kind} tensor")
    if not x.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if min(x.shape) < 1:
        raise ValueError(f"empty {name} {tuple(x.shape)}")
    return x.detach()


def _out(out, shape, like, name="out"):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    if (not torch.is_tensor(out) or tuple(out.shape) != tuple(shape) or out.dtype != torch.float32
            or out.device != like.device or not out.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous float32 tensor {tuple(shape)} on {like.device}")
    return out


def _conv_args(x, weight, bias, relu, out, kind, ksize=3):
    """The checked arguments of a ksize x ksize convolution (3: conv3x3, 1: conv1x1, whose weight may be [Cout, Cin])."""
    x = _tensor4(x, "x", kind)
    if ksize == 1 and torch.is_tensor(weight) and weight.dim() == 2:
        weight = weight[:, :, None, None]  # (a view: [Cout, Cin, 1, 1] as it lies)
    weight = _tensor4(weight, "weight", kind)
    if tuple(weight.shape[2:]) != (ksize, ksize):
        raise ValueError(f"weight must be [Cout, Cin, {ksize}, {ksize}]{' or [Cout, Cin]' if ksize == 1 else ''}, "
                         f"not {tuple(weight.shape)}")
    if weight.shape[1] != x.shape[1]:
        raise ValueError(f"x has {x.shape[1]} channels, weight takes {weight.shape[1]}")
    if weight.device != x.device:
        raise ValueError("x and weight must share one device")
    cout = int(weight.shape[0])
    if bias is not None:
        if (not torch.is_tensor(bias) or tuple(bias.shape) != (cout,) or bias.dtype != torch.float32
                or bias.device != x.device or not bias.is_contiguous()):
            raise ValueError(f"bias must be a contiguous float32 tensor [{cout}] on {x.device}")
        bias = bias.detach()
    b, cin, h, w = (int(s) for s in x.shape)
    out = _out(out, (b, cout, h, w), x)
    flags = (_lib.CONV_BIAS if bias is not None else 0) | (_lib.CONV_RELU if relu else 0)
    return x, weight, bias, out, (b, cin, h, w, cout), flags


def _launch(device, stream, tensors, call):
    """Run call(stream pointer) on `stream` (default: the device's current stream) and keep the tensors alive there."""
    _lib.require_device(device)
    s = torch.cuda.current_stream(device) if stream is None else stream
    with torch.cuda.device(device):
        rc = call(ctypes.c_void_p(s.cuda_stream))
    for t in tensors:
        if t is not None:
            t.record_stream(s)  # (the caching allocator must not hand the memory on before the kernel has run)
    return rc


PRECISIONS = ("f32", "f16")
F16_LIMIT = 65520.0  # fl16 of a magnitude from here on is Inf


def _precision(name):
    if not isinstance(name, str) or name not in PRECISIONS:
        raise ValueError(f'precision must be "f32" or "f16", not {name!r}')
    return name


def _image_shape(cin, cout):
    """[Cout_p, CB, 9, 16] of the packed fp16 weight image (fmpnp_conv3x3_f16_weights_size)."""
    cb = (cin + 15) // 16
    nbytes = _lib.load().fmpnp_conv3x3_f16_weights_size(cin, cout)
    if nbytes == 0:
        _lib.check(_lib.ETOOBIG, "fmpnp_conv3x3_f16_weights_size")
    return (nbytes // (cb * 9 * 32), cb, 9, 16)


def conv3x3_f16_weights(weight, stream=None):
    """The packed fp16 image of a float32 weight [Cout, Cin, 3, 3] for conv3x3(..., precision="f16"): a float16 tensor
    [Cout_p, CB, 9, 16] on the weight's device, image[co, cb, t, c] = weight[co, 16 cb + c, t // 3, t % 3].half(),
    zeros where 16 cb + c >= Cin or co >= Cout (Cout_p: Cout up to a multiple of 32).  On a CUDA weight the kernel
    builds it (asynchronous on `stream`), on a CPU weight fmpnp_conv3x3_pack_weights_f16_cpu: the same bits.  The
    image remembers Cout (image.fmpnp_cout); one image serves every batch and image size."""
    if not torch.is_tensor(weight) or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError("weight must be a 4-D tensor [Cout, Cin, 3, 3]")
    if weight.dtype != torch.float32 or weight.device.type not in ("cuda", "cpu"):
        raise ValueError("weight must be a float32 CUDA or CPU tensor")
    if not weight.is_contiguous():
        raise ValueError("weight must be contiguous")
    if min(weight.shape) < 1:
        raise ValueError(f"empty weight {tuple(weight.shape)}")
    weight = weight.detach()
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    image = torch.empty(_image_shape(cin, cout), dtype=torch.float16, device=weight.device)
    if weight.is_cuda:
        rc = _launch(weight.device, stream, (weight, image), lambda s: _lib.load().fmpnp_conv3x3_pack_weights_f16_async(
            _vp(weight), cin, cout, _vp(image), s))
        _lib.check(rc, "fmpnp_conv3x3_pack_weights_f16_async")
    else:
        _lib.check(_lib.load().fmpnp_conv3x3_pack_weights_f16_cpu(_vp(weight), cin, cout, _vp(image)),
                   "fmpnp_conv3x3_pack_weights_f16_cpu")
    image.fmpnp_cout = cout
    return image


def _is_image(weight):
    return torch.is_tensor(weight) and weight.dtype == torch.float16


def _image_args(x, image, bias, relu, out, cout, kind):
    """_conv_args for a packed image in the weight's place.  Cout: `cout`, else what conv3x3_f16_weights recorded on
    the image, else the bias's or out's length."""
    x = _tensor4(x, "x", kind)
    b, cin, h, w = (int(s) for s in x.shape)
    if cout is None:
        cout = getattr(image, "fmpnp_cout", None)
    if cout is None and torch.is_tensor(bias) and bias.dim() == 1:
        cout = int(bias.shape[0])
    if cout is None and torch.is_tensor(out) and out.dim() == 4:
        cout = int(out.shape[1])
    if cout is None:
        raise ValueError("a packed weight image needs cout (it is padded in Cout)")
    cout = int(cout)
    if cout < 1:
        raise ValueError("cout must be positive")
    shape = _image_shape(cin, cout)
    if image.dim() != 4 or tuple(image.shape) != shape or image.device != x.device or not image.is_contiguous():
        raise ValueError(f"the packed weight image must be a contiguous float16 tensor {shape} on {x.device} "
                         f"for {cin} -> {cout} channels, not {tuple(image.shape)}")
    if bias is not None:
        if (not torch.is_tensor(bias) or tuple(bias.shape) != (cout,) or bias.dtype != torch.float32
                or bias.device != x.device or not bias.is_contiguous()):
            raise ValueError(f"bias must be a contiguous float32 tensor [{cout}] on {x.device}")
        bias = bias.detach()
    out = _out(out, (b, cout, h, w), x)
    flags = (_lib.CONV_BIAS if bias is not None else 0) | (_lib.CONV_RELU if relu else 0)
    return x, image.detach(), bias, out, (b, cin, h, w, cout), flags


def _unpack_image(image, cin, cout):
    """The float32 weight [Cout, Cin, 3, 3] whose values are the image's (exact: binary16 values are fp32 values)."""
    w = image.float().permute(0, 1, 3, 2).reshape(image.shape[0], -1, 9)  # [Cout_p, 16 CB, 9]
    return w[:cout, :cin].reshape(cout, cin, 3, 3).contiguous()


def _weight_dtype_check(weight, precision):
    if precision == "f32" and _is_image(weight):
        raise ValueError('a packed float16 weight image needs precision="f16"')
    if precision == "f16" and torch.is_tensor(weight) and weight.dtype not in (torch.float32, torch.float16):
        raise ValueError("weight must be float32 [Cout, Cin, 3, 3] or a packed float16 image")


DILATIONS = (1, 2)


def _dilation(dilation, precision):
    if isinstance(dilation, bool) or not isinstance(dilation, int) or dilation not in DILATIONS:
        raise ValueError(f"dilation must be 1 or 2, not {dilation!r}")
    if dilation != 1 and precision != "f32":
        raise ValueError('the dilated convolution has no fp16 precision: dilation=2 needs precision="f32"')
    return dilation


def conv3x3(x, weight, bias=None, relu=False, out=None, stream=None, precision="f32", cout=None, dilation=1):
    """The 3x3 / stride 1 / zero padding 1 convolution of torch.nn.Conv2d on float32 CUDA tensors: x [B, Cin, H, W],
    weight [Cout, Cin, 3, 3], bias [Cout] or None -> [B, Cout, H, W]; relu: the ReLU fused into the same launch.
    All contiguous.  out: a tensor of that shape to write into.  Asynchronous on `stream` (a torch.cuda.Stream;
    default: the current stream).  Weights and biases must be finite.
    precision: "f32" (default) is the exact-fp32 kernel.  "f16" (opt-in) uses every input and weight rounded to
    binary16 on the fp16 matrix cores, with fp32 accumulation (include/fmpnp.h states the order and the bound against
    conv3x3_cpu(precision="f16")); weights must be below 65520 in magnitude.  Then `weight` is the float32 weight,
    packed on this call, or the image conv3x3_f16_weights(weight) built once (cout: its Cout, when the image does
    not carry it).
    dilation: 1 (default: the entry point as it always was), or 2 for Conv2d(dilation=2, padding=2): the same chain,
    tap (ky, kx) at ((ky - 1) * 2, (kx - 1) * 2) (fmpnp_conv3x3_dilated).  Anything else is a ValueError.  The fp16
    precision of the dilated form is not built: dilation=2 with precision="f16" is a ValueError."""
    precision = _precision(precision)
    dilation = _dilation(dilation, precision)
    _weight_dtype_check(weight, precision)
    if precision == "f16":
        if not _is_image(weight):
            _conv_args(x, weight, bias, relu, out, "cuda")  # (the fp32 weight's own checks)
            weight = conv3x3_f16_weights(weight, stream=stream)
        x, image, bias, out, (b, cin, h, w, cout), flags = _image_args(x, weight, bias, relu, out, cout, "cuda")
        rc = _launch(x.device, stream, (x, image, bias, out), lambda s: _lib.load().fmpnp_conv3x3_f16_async(
            _vp(x), b, cin, h, w, _vp(image), _vp(bias), cout, flags, _vp(out), s))
        _lib.check(rc, "fmpnp_conv3x3_f16_async")
        return out
    x, weight, bias, out, (b, cin, h, w, cout), flags = _conv_args(x, weight, bias, relu, out, "cuda")
    if dilation != 1:
        rc = _launch(x.device, stream, (x, weight, bias, out), lambda s: _lib.load().fmpnp_conv3x3_dilated_async(
            _vp(x), b, cin, h, w, _vp(weight), _vp(bias), cout, flags, _vp(out), dilation, s))
        _lib.check(rc, "fmpnp_conv3x3_dilated_async")
        return out
    rc = _launch(x.device, stream, (x, weight, bias, out), lambda s: _lib.load().fmpnp_conv3x3_async(
        _vp(x), b, cin, h, w, _vp(weight), _vp(bias), cout, flags, _vp(out), s))
    _lib.check(rc, "fmpnp_conv3x3_async")
    return out


def conv3x3_cpu(x, weight, bias=None, relu=False, out=None, n_threads=0, precision="f32", cout=None, dilation=1):
    """The CPU twin (fmpnp_conv3x3_cpu; fmpnp_conv3x3_dilated_cpu for dilation=2) on float32 CPU tensors: conv3x3's
    result bit for bit.  precision="f16": the
    REFERENCE of the fp16 precision (fmpnp_conv3x3_f16_cpu: binary16 operands, fp64 accumulation in the contract's
    order, one rounding), which bounds the kernel and is not its twin; a packed image is taken for the weights it
    holds.  dilation: as conv3x3 (no fp16 precision of the dilated form: a ValueError)."""
    precision = _precision(precision)
    dilation = _dilation(dilation, precision)
    _weight_dtype_check(weight, precision)
    if precision == "f16" and _is_image(weight):
        x, image, bias, out, (b, cin, h, w, cout), flags = _image_args(x, weight, bias, relu, out, cout, "cpu")
        weight = _unpack_image(image, cin, cout)
    else:
        x, weight, bias, out, (b, cin, h, w, cout), flags = _conv_args(x, weight, bias, relu, out, "cpu")
    if dilation != 1:
        rc = _lib.load().fmpnp_conv3x3_dilated_cpu(_vp(x), b, cin, h, w, _vp(weight), _vp(bias), cout, flags, _vp(out),
                                                   dilation, int(n_threads))
        _lib.check(rc, "fmpnp_conv3x3_dilated_cpu")
        return out
    fn = _lib.load().fmpnp_conv3x3_f16_cpu if precision == "f16" else _lib.load().fmpnp_conv3x3_cpu
    rc = fn(_vp(x), b, cin, h, w, _vp(weight), _vp(bias), cout, flags, _vp(out), int(n_threads))
    _lib.check(rc, "fmpnp_conv3x3_f16_cpu" if precision == "f16" else "fmpnp_conv3x3_cpu")
    return out


def conv1x1(x, weight, bias=None, relu=False, out=None, stream=None):
    """The 1x1 / stride 1 / padding 0 convolution of torch.nn.Conv2d on float32 CUDA tensors: x [B, Cin, H, W], weight
    [Cout, Cin, 1, 1] or [Cout, Cin], bias [Cout] or None -> [B, Cout, H, W]; relu: the ReLU fused into the same
    launch.  All contiguous.  out: a tensor of that shape to write into (not x).  One launch for any B, asynchronous
    on `stream` (a torch.cuda.Stream; default: the current stream).  Exact fp32: every output is one fmaf chain over
    the input channels ascending (include/fmpnp.h, "the 1x1 convolution"), the row of exhaustive_match's score map
    for sparse = weight and dense = x[b].  Weights and biases must be finite.  There is no fp16 precision."""
    x, weight, bias, out, (b, cin, h, w, cout), flags = _conv_args(x, weight, bias, relu, out, "cuda", ksize=1)
    rc = _launch(x.device, stream, (x, weight, bias, out), lambda s: _lib.load().fmpnp_conv1x1_async(
        _vp(x), b, cin, h, w, _vp(weight), _vp(bias), cout, flags, _vp(out), s))
    _lib.check(rc, "fmpnp_conv1x1_async")
    return out


def conv1x1_cpu(x, weight, bias=None, relu=False, out=None, n_threads=0):
    """The CPU twin (fmpnp_conv1x1_cpu) on float32 CPU tensors: conv1x1's result bit for bit, for any n_threads."""
    x, weight, bias, out, (b, cin, h, w, cout), flags = _conv_args(x, weight, bias, relu, out, "cpu", ksize=1)
    rc = _lib.load().fmpnp_conv1x1_cpu(_vp(x), b, cin, h, w, _vp(weight), _vp(bias), cout, flags, _vp(out), int(n_threads))
    _lib.check(rc, "fmpnp_conv1x1_cpu")
    return out


def _flat(x, name, kind):
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.device.type != kind:
        raise ValueError(f"{name} must be a float32 {kind} tensor")
    if not x.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return x.detach()


def relu(x, out=None, stream=None):
    """x > 0 ? x : (NaN stays, everything else +0) on a contiguous float32 CUDA tensor of any shape; out may be x
    itself.  Asynchronous on `stream` (default: the current stream)."""
    x = _flat(x, "x", "cuda")
    out = _out(out, x.shape, x)
    rc = _launch(x.device, stream, (x, out),
                 lambda s: _lib.load().fmpnp_relu_async(_vp(x), _vp(out), x.numel(), s))
    _lib.check(rc, "fmpnp_relu_async")
    return out


def relu_cpu(x, out=None, n_threads=0):
    """The CPU twin (fmpnp_relu_cpu): relu's result bit for bit."""
    x = _flat(x, "x", "cpu")
    out = _out(out, x.shape, x)
    _lib.check(_lib.load().fmpnp_relu_cpu(_vp(x), _vp(out), x.numel(), int(n_threads)), "fmpnp_relu_cpu")
    return out


def _pool_args(x, out, kind):
    x = _tensor4(x, "x", kind)
    b, c, h, w = (int(s) for s in x.shape)
    if h < 2 or w < 2:
        raise ValueError(f"maxpool2x2 of {h} x {w} would be empty")
    return x, _out(out, (b, c, h // 2, w // 2), x), (b, c, h, w)


def maxpool2x2(x, out=None, stream=None):
    """torch.nn.MaxPool2d(2, 2) (floor mode: an odd last row or column is dropped; a NaN wins) on a contiguous
    float32 CUDA tensor [B, C, H, W] -> [B, C, H // 2, W // 2].  Asynchronous on `stream` (default: the current
    stream)."""
    x, out, (b, c, h, w) = _pool_args(x, out, "cuda")
    rc = _launch(x.device, stream, (x, out),
                 lambda s: _lib.load().fmpnp_maxpool2x2_async(_vp(x), b, c, h, w, _vp(out), s))
    _lib.check(rc, "fmpnp_maxpool2x2_async")
    return out


def maxpool2x2_cpu(x, out=None, n_threads=0):
    """The CPU twin (fmpnp_maxpool2x2_cpu): maxpool2x2's result bit for bit."""
    x, out, (b, c, h, w) = _pool_args(x, out, "cpu")
    _lib.check(_lib.load().fmpnp_maxpool2x2_cpu(_vp(x), b, c, h, w, _vp(out), int(n_threads)), "fmpnp_maxpool2x2_cpu")
    return out


def _avgpool_args(x, out, kind):
    x = _tensor4(x, "x", kind)
    b, c, h, w = (int(s) for s in x.shape)
    if h < 2 or w < 2:
        raise ValueError(f"avgpool2x2s1 of {h} x {w} would be empty")
    return x, _out(out, (b, c, h - 1, w - 1), x), (b, c, h, w)


def avgpool2x2s1(x, out=None, stream=None):
    """torch.nn.AvgPool2d(2, stride=1) (no padding) on a contiguous float32 CUDA tensor [B, C, H, W] ->
    [B, C, H - 1, W - 1]: (((v00 + v01) + v10) + v11) * 0.25 in float32, in that order (include/fmpnp.h, "dense
    features").  out must not be x.  Asynchronous on `stream` (default: the current stream)."""
    x, out, (b, c, h, w) = _avgpool_args(x, out, "cuda")
    rc = _launch(x.device, stream, (x, out),
                 lambda s: _lib.load().fmpnp_avgpool2x2s1_async(_vp(x), b, c, h, w, _vp(out), s))
    _lib.check(rc, "fmpnp_avgpool2x2s1_async")
    return out


def avgpool2x2s1_cpu(x, out=None, n_threads=0):
    """The CPU twin (fmpnp_avgpool2x2s1_cpu): avgpool2x2s1's result bit for bit."""
    x, out, (b, c, h, w) = _avgpool_args(x, out, "cpu")
    _lib.check(_lib.load().fmpnp_avgpool2x2s1_cpu(_vp(x), b, c, h, w, _vp(out), int(n_threads)), "fmpnp_avgpool2x2s1_cpu")
    return out


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _check_child(i, m, precision="f32", owner="HipEncoder", what="child", ksize=3, dilations=(1,)):
    """"conv" / "relu" / "pool" / "avgpool" for a supported child; TypeError naming it otherwise.  owner, what: how the
    messages name the plan and the child (HipSuperPointNet: its attributes); ksize: 3, or 1 for a 1x1 / padding 0
    convolution (HipSuperPointNet's heads only); dilations: the dilations a 3x3 Conv2d may have, its padding being
    equal to it ((1,) unless the plan asks: HipEncoder takes DILATIONS and AvgPool2d(2, stride=1))."""
    def bad(why):
        return TypeError(f"{owner}: {what} {i} ({m!r}) is not supported: {why}")
    if isinstance(m, nn.Conv2d):
        pad = ksize // 2
        dil = _pair(m.dilation)
        if ksize == 3 and dil[0] == dil[1] and dil[0] != 1 and dil[0] in dilations:
            if precision == "f16":
                raise bad('the dilated convolution has no fp16 precision (precision="f16" takes dilation 1 only)')
            pad = dil[0]  # (padding = dilation: the output keeps the input's size)
        elif dil != (1, 1):
            dil = None
        if (_pair(m.kernel_size) != (ksize, ksize) or _pair(m.stride) != (1, 1) or _pair(m.padding) != (pad, pad)
                or dil is None or m.groups != 1 or m.padding_mode != "zeros"):
            if len(dilations) > 1:
                raise bad(f"a Conv2d must be {ksize}x{ksize}, stride 1, dilation 1 or 2 with padding equal to it, "
                          f"groups 1, zeros padding")
            raise bad(f"a Conv2d must be {ksize}x{ksize}, stride 1, padding {pad}, dilation 1, groups 1, zeros padding")
        params = [m.weight] + ([m.bias] if m.bias is not None else [])
        if any(p.dtype != torch.float32 for p in params):
            raise bad("float32 parameters only")
        if not all(bool(torch.isfinite(p.detach().cpu()).all()) for p in params):
            raise ValueError(f"{owner}: {what} {i} ({m!r}) has non-finite weights or biases")
        if precision == "f16" and ksize == 3 and float(m.weight.detach().abs().max()) >= F16_LIMIT:
            raise ValueError(f"{owner}: {what} {i} ({m!r}) has a weight of magnitude >= 65520, which binary16 "
                             f'does not hold (precision="f16")')
        return "conv"
    if isinstance(m, nn.ReLU):
        return "relu"
    if isinstance(m, nn.MaxPool2d):
        stride = m.kernel_size if m.stride is None else m.stride
        if (_pair(m.kernel_size) != (2, 2) or _pair(stride) != (2, 2) or _pair(m.padding) != (0, 0)
                or _pair(m.dilation) != (1, 1) or m.ceil_mode or m.return_indices):
            raise bad("a MaxPool2d must be 2x2, stride 2, no padding, no dilation, floor mode, no indices")
        return "pool"
    if isinstance(m, nn.AvgPool2d) and len(dilations) > 1:
        stride = m.kernel_size if m.stride is None else m.stride
        if (_pair(m.kernel_size) != (2, 2) or _pair(stride) != (1, 1) or _pair(m.padding) != (0, 0) or m.ceil_mode
                or m.divisor_override is not None):
            raise bad("an AvgPool2d must be 2x2, stride 1, no padding, floor mode, no divisor override")
        return "avgpool"  # (count_include_pad: there is no padding to count)
    raise bad("only Conv2d, ReLU, MaxPool2d and AvgPool2d children" if len(dilations) > 1
              else "only Conv2d, ReLU and MaxPool2d children")


def _cached_image(images, i, w):
    """The packed fp16 image of convolution i's weight w, built on first use and kept in `images`, keyed on the weight's
    device, data_ptr and version, so .to() and in-place updates rebuild it."""
    key = (w.device, w.data_ptr(), w._version)
    hit = images.get(i)
    if hit is None or hit[0] != key:
        hit = images[i] = (key, conv3x3_f16_weights(w))
    return hit[1]


class HipEncoder(nn.Module):
    """An nn.Sequential of Conv2d (3x3, stride 1, padding 1), ReLU and MaxPool2d(2, 2) children -- a stock VGG-16's
    features, for instance -- run through libfmpnp's operators instead of the framework's.  A D2-Net style trunk's
    two other children are taken too: a 3x3 Conv2d of dilation 2 with padding 2 (conv3x3(dilation=2)) and
    AvgPool2d(2, stride=1) without padding (avgpool2x2s1).

    The plan is built once: every child is checked (anything else raises TypeError naming the child) and the
    weights and biases are checked finite on the host.  The parameters stay the encoder's own (it is a submodule:
    .to() and state_dict() work as before; the finite check is not repeated when they change).  A convolution and
    the ReLU that follows it run as one launch.  Where the encoder lives decides what runs: the kernels on a CUDA
    device, the CPU twins on the CPU (bit-identical).  Inference only: nothing here is differentiable.

    precision="f16" (opt-in) runs every convolution in the fp16 precision: conv3x3(precision="f16") on a CUDA device,
    its reference on the CPU (not bit-identical to the device).  The plan then also rejects weights of magnitude
    >= 65520.  The packed weight images are built on first use and kept per convolution, keyed on the weight's
    device, data_ptr and version, so .to() and in-place updates rebuild them.  Activations stay float32; the ReLU
    and the pools are the same.  The dilated convolution has no fp16 precision: with precision="f16" a dilated child
    is a TypeError naming it."""

    def __init__(self, encoder, precision="f32"):
        super().__init__()
        if not isinstance(encoder, nn.Sequential):
            raise TypeError("HipEncoder takes an nn.Sequential")
        self.precision = _precision(precision)
        self.encoder = encoder
        self._kinds = [_check_child(i, m, self.precision, dilations=DILATIONS) for i, m in enumerate(encoder.children())]
        self._images = {}  # child index -> ((device, data_ptr, version), packed image)

    def _image(self, i, w):
        return _cached_image(self._images, i, w)

    def _ops(self, x):
        if x.is_cuda:
            return conv3x3, relu, maxpool2x2, avgpool2x2s1
        return conv3x3_cpu, relu_cpu, maxpool2x2_cpu, avgpool2x2s1_cpu

    def _input(self, x):
        if not torch.is_tensor(x) or x.dim() != 4:
            raise ValueError("HipEncoder takes a [B, C, H, W] tensor")
        p = next(self.encoder.parameters(), None)
        if p is not None and p.device != x.device:
            raise ValueError(f"the batch is on {x.device}, the encoder on {p.device}")
        return x.detach().to(torch.float32).contiguous()

    def _walk(self, x, end, taps=(), relu_last=False):
        """Children 0 .. end - 1 on x -> (the last output, {tapped child: its recorded input}).  relu_last: a ReLU
        behind the walk that is no child (DenseFeatureExtractor's use_relu): it joins the last convolution's launch
        when that is the last child run, and is its own launch otherwise."""
        conv, act, pool, avgpool = self._ops(x)
        children = list(self.encoder.children())
        maps, i = {}, 0
        while i < end:
            m, kind = children[i], self._kinds[i]
            if i in taps:
                maps[i] = x
            if kind == "conv":
                # the ReLU behind it joins the launch, unless the walk records the raw output: a tap on a ReLU
                # that is not in-place (an in-place one overwrites what torch's walk recorded)
                nxt = children[i + 1] if i + 1 < end and self._kinds[i + 1] == "relu" else None
                fuse = nxt is not None and not (i + 1 in taps and not nxt.inplace)
                tail = relu_last and i + 1 == end  # (the caller's ReLU behind the last child)
                d = _pair(m.dilation)[0]
                w = m.weight.detach().contiguous()
                b = m.bias.detach().contiguous() if m.bias is not None else None
                if self.precision == "f16":  # (the reference rounds the float32 weights itself)
                    x = conv(x, self._image(i, m.weight) if x.is_cuda and m.weight.is_contiguous() else w, b,
                             relu=fuse or tail, precision="f16")
                elif d != 1:
                    x = conv(x, w, b, relu=fuse or tail, dilation=d)
                else:
                    x = conv(x, w, b, relu=fuse or tail)
                if tail:
                    relu_last = False
                if fuse:
                    if i + 1 in taps:
                        maps[i + 1] = x
                    i += 2
                    continue
            elif kind == "relu":
                x = act(x)
                if m.inplace and i in taps:
                    maps[i] = x
            elif kind == "avgpool":
                x = avgpool(x)
            else:
                x = pool(x)
            i += 1
        if relu_last:
            x = act(x)
        return x, maps

    def forward(self, x, relu=False):
        """The last child's output, as the nn.Sequential itself returns it.  relu: a ReLU behind the last child (a
        D2-Net trunk's use_relu), one launch with the last convolution when that is the last child."""
        x = self._input(x)
        with torch.no_grad():
            return self._walk(x, len(self._kinds), relu_last=bool(relu))[0]

    def feature_maps(self, batch, hypercolumn_layers):
        """The layer walk of network.py:134-147: the input of every listed child (ascending, distinct indices), in
        order; nothing behind the last one runs.  A tap on a ReLU child returns what torch's walk returns: the
        values after the ReLU when it is in-place (torch's recorded tensor is overwritten), before it otherwise."""
        taps = [int(i) for i in hypercolumn_layers]
        if not taps or sorted(set(taps)) != taps or taps[0] < 0 or taps[-1] >= len(self._kinds):
            raise ValueError("hypercolumn_layers must be ascending, distinct indices of the encoder's children")
        x = self._input(batch)
        last = taps[-1]
        # (torch's walk runs the last listed child too; its output is dropped, but an in-place ReLU has by then
        # rewritten the recorded map)
        end = last + 1 if self._kinds[last] == "relu" and list(self.encoder.children())[last].inplace else last
        with torch.no_grad():
            x, maps = self._walk(x, end, set(taps))
        if last not in maps:
            maps[last] = x
        return [maps[i] for i in taps]
