"""The image front end: decoded uint8 pixels in, the tensor the networks take out.

The reference does this stage on the host in three places -- ImagesFromList (s2dhm/network/images_from_list.py:57-103:
PIL thumbnail / resize with Image.ANTIALIAS, then ToTensor + Normalize), the d2-net loader
(s2dhm/d2net_utils/extract_dense_features.py:27-45: the same resize, then the "caffe" / "torch" preprocessing) and
SuperPoint's (s2dhm/superpoint/detect_and_compute_superpoint.py:6-10: gray / 255).  Here the bytes are uploaded once
(3 bytes per pixel) and libfmpnp's kernels resize and transform them.  Pillow's 8-bit Lanczos resampling is fixed-point
integer arithmetic, so resize_lanczos equals Image.resize(size, Image.LANCZOS) bit for bit (include/fmpnp.h, "image
front end", states the contract; tests/golden/image_lanczos.npz records Pillow 12.2.0's results); the *_cpu functions are
the CPU twins (bit-identical; explicit entry points, never a fallback).

Sizes of tensors are (height, width), as the tensors have them; thumbnail_size speaks Pillow's (width, height).

Out of scope: JPEG / PNG decoding stays on the host, in PIL.  Pillow's reducing_gap is not reproduced: from a 4x shrink
on, Image.thumbnail first box-reduces by an integer (and a JPEG may be decoded at a reduced size by draft), so for
those shrinks load_images gives the fair resampling, Image.resize(..., reducing_gap=None), not thumbnail's pixels; below
4x the two are equal.  (The reference's datasets do not shrink at all: 1024 x 1024 and 1024 x 768 at image_size 1024.)
No other filter than Lanczos, no alpha channel, no 16-bit images.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .encoder import _launch, _vp

PREPROCESSINGS = {"torch": _lib.IMAGE_TORCH, "caffe": _lib.IMAGE_CAFFE, None: _lib.IMAGE_RAW, "gray": _lib.IMAGE_GRAY}


def thumbnail_size(width, height, image_size):
    """The (width, height) Image.thumbnail((image_size, image_size)) leaves an image of width x height with: the image's
    own size when it already fits, otherwise the aspect-preserving size by the round_aspect rule of Pillow 12.2.0
    (Image.py, thumbnail: of floor and ceil of the exact size the one whose aspect is nearer, floor on a tie, at least
    1).  The reference pins Pillow 7.1.2, whose rule is believed identical; that is NOT pinned by any test here."""
    width, height, image_size = int(width), int(height), int(math.floor(image_size))
    if width < 1 or height < 1 or image_size < 1:
        raise ValueError("thumbnail_size takes positive sizes")
    x = y = image_size
    if x >= width and y >= height:
        return width, height

    def round_aspect(number, key):
        return max(min(math.floor(number), math.ceil(number), key=key), 1)

    aspect = width / height
    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    return x, y


def _source(image, kind):
    """A uint8 [H, W, 3] or [B, H, W, 3] tensor on a `kind` device whose pixels are 3 consecutive bytes (rows and images
    may be strided: a crop view works) -> (tensor as 4-D, was_3d, image_stride, row_stride, B, H, W)."""
    if isinstance(image, np.ndarray) and kind == "cpu":
        image = torch.from_numpy(image)
    if not torch.is_tensor(image) or image.dtype != torch.uint8 or image.dim() not in (3, 4) or image.shape[-1] != 3:
        raise ValueError("the image must be a uint8 tensor [H, W, 3] or [B, H, W, 3]")
    if image.device.type != kind:
        raise ValueError(f"the image must be a {kind} tensor, not on {image.device}")
    squeeze = image.dim() == 3
    x = image.detach()
    if squeeze:
        x = x[None]
    b, h, w = (int(s) for s in x.shape[:3])
    if min(b, h, w) < 1:
        raise ValueError(f"empty image {tuple(image.shape)}")
    sb, sy, sx, sc = (int(s) for s in x.stride())
    if (sc != 1 or sx != 3 or sy < 3 * w or (b > 1 and sb < (h - 1) * sy + 3 * w)) and not x.is_contiguous():
        x = x.contiguous()  # (a view whose pixels are not 3 consecutive bytes, or whose rows overlap)
        sb, sy = 3 * w * h, 3 * w
    return x, squeeze, sb, sy, b, h, w


def _size(size, h, w):
    if size is None:
        return h, w
    if not isinstance(size, (tuple, list)) or len(size) != 2:
        raise ValueError("size is (height, width)")
    oh, ow = int(size[0]), int(size[1])
    if oh < 1 or ow < 1:
        raise ValueError("size must be positive")
    return oh, ow


def _dst(out, shape, dtype, like):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    if (not torch.is_tensor(out) or tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != like.device
            or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous {dtype} tensor {tuple(shape)} on {like.device}")
    return out


def _floats3(values, name):
    if values is None:
        return None
    v = [float(t) for t in values]
    if len(v) != 3 or not all(math.isfinite(t) for t in v):
        raise ValueError(f"{name} takes three finite numbers")
    return (ctypes.c_float * 3)(*v)


def _transform(preprocessing, mean, std, swap_rb):
    if preprocessing not in PREPROCESSINGS:
        raise ValueError('preprocessing must be "torch", "caffe", None or "gray"')
    mode = PREPROCESSINGS[preprocessing]
    if std is not None and mode != _lib.IMAGE_TORCH:
        raise ValueError('std goes with preprocessing="torch" only')
    if mean is not None and mode not in (_lib.IMAGE_TORCH, _lib.IMAGE_CAFFE):
        raise ValueError('mean goes with preprocessing="torch" or "caffe" only')
    std = _floats3(std, "std")
    if std is not None and any(t == 0 for t in std):
        raise ValueError("std must not be zero")
    flags = _lib.IMAGE_SWAP_RB if (mode == _lib.IMAGE_GRAY and swap_rb) else 0
    return mode, flags, _floats3(mean, "mean"), std, (1 if mode == _lib.IMAGE_GRAY else 3)


def _resize(image_u8, size, out, kind, run):
    x, squeeze, sb, sy, b, h, w = _source(image_u8, kind)
    oh, ow = _size(size, h, w)
    out4 = _dst(out[None] if (out is not None and squeeze and torch.is_tensor(out) and out.dim() == 3) else out,
                (b, oh, ow, 3), torch.uint8, x)
    run(x, out4, (_vp(x), sb, sy, b, h, w, oh, ow, _vp(out4)))
    return out4[0] if squeeze else out4


def resize_lanczos(image_u8, size, out=None, stream=None):
    """A uint8 CUDA tensor [H, W, 3] or [B, H, W, 3] -> the uint8 tensor [h, w, 3] or [B, h, w, 3] that
    PIL.Image.resize((w, h), Image.LANCZOS) gives for each image, bit for bit.  size = (h, w).  The source may be a
    strided view (a crop) as long as a pixel's 3 bytes are consecutive; out: a contiguous tensor to write into, which
    must not overlap the source.  At most two launches, asynchronous on `stream` (a torch.cuda.Stream; default: the
    current stream)."""
    def run(x, out4, args):
        rc = _launch(x.device, stream, (x, out4), lambda s: _lib.load().fmpnp_image_resize_u8_async(*args, s))
        _lib.check(rc, "fmpnp_image_resize_u8_async")
    return _resize(image_u8, size, out, "cuda", run)


def resize_lanczos_cpu(image_u8, size, out=None, n_threads=0):
    """The CPU twin (fmpnp_image_resize_u8_cpu) on a uint8 CPU tensor or numpy array: resize_lanczos's result bit for
    bit, for any n_threads."""
    def run(x, out4, args):
        _lib.check(_lib.load().fmpnp_image_resize_u8_cpu(*args, int(n_threads)), "fmpnp_image_resize_u8_cpu")
    return _resize(image_u8, size, out, "cpu", run)


def _to_tensor(image_u8, size, preprocessing, mean, std, swap_rb, out, kind, run):
    x, _, sb, sy, b, h, w = _source(image_u8, kind)
    oh, ow = _size(size, h, w)
    mode, flags, mean_c, std_c, channels = _transform(preprocessing, mean, std, swap_rb)
    out = _dst(out, (b, channels, oh, ow), torch.float32, x)
    run(x, out, (_vp(x), sb, sy, b, h, w, oh, ow, mode, flags, mean_c, std_c, _vp(out)))
    return out


def image_to_tensor(image_u8, size=None, preprocessing="torch", mean=None, std=None, swap_rb=True, out=None, stream=None):
    """A uint8 CUDA tensor [H, W, 3] or [B, H, W, 3] -> the float32 tensor [B, C, h, w] a network takes: the Lanczos
    resize to size = (h, w) (None: no resize), then the value transform as the last pass's epilogue.
    preprocessing: "torch" -- ((float)p / 255 - mean) / std with true float32 divisions, torchvision's ToTensor +
    Normalize bit for bit; mean / std default to ImageNet's; "caffe" -- channels reversed to BGR, (float)p - mean, mean
    defaulting to (103.939, 116.779, 123.68) per OUTPUT channel; None -- (float)p; "gray" -- one channel,
    (float)y / 255 with y = (9798 a + 19235 g + 3735 b + 16384) >> 15, where with swap_rb (default, the reference's
    cv2.imread + COLOR_RGB2GRAY on an RGB source) a is the source's channel 2 and b its channel 0, and without it the
    conventional weighting (a is channel 0).  One launch without a resize, at most two with one; asynchronous on
    `stream`."""
    def run(x, o, args):
        rc = _launch(x.device, stream, (x, o), lambda s: _lib.load().fmpnp_image_to_tensor_async(*args, s))
        _lib.check(rc, "fmpnp_image_to_tensor_async")
    return _to_tensor(image_u8, size, preprocessing, mean, std, swap_rb, out, "cuda", run)


def image_to_tensor_cpu(image_u8, size=None, preprocessing="torch", mean=None, std=None, swap_rb=True, out=None,
                        n_threads=0):
    """The CPU twin (fmpnp_image_to_tensor_cpu) on a uint8 CPU tensor or numpy array: image_to_tensor's result bit for
    bit, for any n_threads."""
    def run(x, o, args):
        _lib.check(_lib.load().fmpnp_image_to_tensor_cpu(*args, int(n_threads)), "fmpnp_image_to_tensor_cpu")
    return _to_tensor(image_u8, size, preprocessing, mean, std, swap_rb, out, "cpu", run)


def _decode(item):
    """A path -> the uint8 [H, W, 3] RGB array PIL decodes; a uint8 array or tensor [H, W, 3] passes through."""
    if torch.is_tensor(item):
        item = item.detach().cpu().numpy()
    if isinstance(item, np.ndarray):
        if item.dtype != np.uint8 or item.ndim != 3 or item.shape[2] != 3:
            raise ValueError("an image array must be uint8 [H, W, 3]")
        return np.ascontiguousarray(item)
    try:
        from PIL import Image
    except ImportError as e:  # (decoding is PIL's; arrays need none)
        raise ImportError("fmpnp.load_images decodes image files with Pillow, which is not installed; "
                          "pass decoded uint8 [H, W, 3] arrays instead") from e
    with Image.open(item) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def load_images(paths_or_arrays, image_size=None, resize=False, device="cuda", preserve_ratio=True, preprocessing="torch"):
    """ImagesFromList.image_path_to_tensor on the library's kernels: a list of image paths (decoded on the host by PIL,
    convert("RGB")) and / or uint8 [H, W, 3] arrays or tensors -> the float32 tensor [B, C, h, w] on `device`.
    resize: every image goes to thumbnail_size(W, H, image_size) (preserve_ratio, the reference's thumbnail) or to
    image_size x image_size; the outputs must share one size.  The bytes are uploaded as they are and resized and
    transformed by image_to_tensor; on a CPU device the twins run.  For shrinks of 4x or more the result is the fair
    resampling, not Image.thumbnail's box-reduced one (see the module's text)."""
    items = list(paths_or_arrays) if isinstance(paths_or_arrays, (list, tuple)) else [paths_or_arrays]
    if not items:
        raise ValueError("no images")
    if resize and (image_size is None or int(image_size) < 1):
        raise ValueError("resize needs a positive image_size")
    device = torch.device(device)
    arrays = [_decode(item) for item in items]

    def target(a):
        h, w = a.shape[:2]
        if not resize:
            return h, w
        if not preserve_ratio:
            return int(image_size), int(image_size)
        tw, th = thumbnail_size(w, h, image_size)
        return th, tw

    sizes = {target(a) for a in arrays}
    if len(sizes) != 1:
        raise ValueError(f"the images of a batch must come out at one size, not {sorted(sizes)}")
    size = sizes.pop()
    to_tensor = image_to_tensor_cpu if device.type == "cpu" else image_to_tensor
    if len({a.shape for a in arrays}) == 1:  # (one upload, one batched call)
        groups = [np.stack(arrays)]
    else:
        groups = [a[None] for a in arrays]
    outs = [to_tensor(torch.from_numpy(g).to(device), size, preprocessing) for g in groups]
    return outs[0] if len(outs) == 1 else torch.cat(outs)


def image_loader(preprocessing="torch", preserve_ratio=True):
    """The (paths, image_size, resize, device) callable HypercolumnExtractor and DenseFeatureExtractor accept as
    image_loader: load_images with this preprocessing."""
    if preprocessing not in PREPROCESSINGS:
        raise ValueError('preprocessing must be "torch", "caffe", None or "gray"')

    def loader(paths, image_size, resize, device):
        return load_images(paths, image_size, resize, device, preserve_ratio=preserve_ratio, preprocessing=preprocessing)
    return loader


def superpoint_image(path_or_array, device="cuda"):
    """superpoint_preprocess (s2dhm/superpoint/detect_and_compute_superpoint.py:6-10) -> the float32 [1, 1, H, W] gray
    tensor in [0, 1] on `device` (squeeze it to [H, W] for SuperPointFrontend.run).  A path is decoded by PIL as RGB; the
    reference's weighting -- cv2.imread's BGR pixels handed to COLOR_RGB2GRAY -- is swap_rb=True for such a source.
    Parity of the integer weights with OpenCV 4.2 is NOT pinned by any test here (cv2 is not available to them)."""
    return load_images([path_or_array], None, False, device, preprocessing="gray")
