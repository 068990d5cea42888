"""d2-net dense features: the reference's second dense feature source (SparseToDensePredictor.features and
optimize_feature_pnp(features=...) take 's2dhm' or 'd2-net') through libfmpnp's operators.

A D2-Net trunk is VGG-16 to conv4_3 with pool3 an AvgPool2d(2, stride=1), the three conv4 layers dilated by 2 with
padding 2, and a ReLU behind them; fmpnp.encoder.HipEncoder walks it (conv3x3(dilation=2), avgpool2x2s1).  The scale
pyramid (s2dhm/d2net_utils/dense_pyramid.py:5-42) runs the trunk on the image at every scale, adds the previous
scale's map resized with align_corners=True and L2-normalises over the channels: dense_pyramid_step is that
resize-add-normalise in one kernel (include/fmpnp.h, "dense features", states the numeric contract),
dense_pyramid_step_cpu its CPU twin (bit-identical; an explicit entry point, never a fallback).
DenseFeatureExtractor is extract_dense_features (s2dhm/d2net_utils/extract_dense_features.py:46-82) around the
caller's trunk; it offers compute_hypercolumn, so an instance can be passed as `net` to
fmpnp.optimize_feature_pnp(features="d2-net").
"""
import math

import numpy as np
import torch
from torch import nn

from . import _lib
from .encoder import HipEncoder, _launch, _out, _tensor4, _vp
from .hypercolumn import assemble_hypercolumn, assemble_hypercolumn_cpu


def _step_args(cur, prev, out, kind):
    cur = _tensor4(cur, "cur", kind)
    if prev is not None:
        prev = _tensor4(prev, "prev", kind)
        if prev.device != cur.device or tuple(prev.shape[:2]) != tuple(cur.shape[:2]):
            raise ValueError(f"prev must be [B, C, hp, wp] with cur's B and C on {cur.device}, not {tuple(prev.shape)}")
    out = _out(out, cur.shape, cur)
    if prev is not None and out.data_ptr() == prev.data_ptr():
        raise ValueError("out must not be prev (it may be cur)")
    b, c, h, w = (int(s) for s in cur.shape)
    hp, wp = (int(s) for s in prev.shape[2:]) if prev is not None else (0, 0)
    return cur, prev, out, (b, c, h, w, hp, wp)


def dense_pyramid_step(cur, prev=None, normalize=True, out=None, stream=None):
    """One step of the scale pyramid on contiguous float32 CUDA tensors: cur [B, C, h, w], prev [B, C, hp, wp] or None
    -> [B, C, h, w]: cur + prev resized to h x w (bilinear, align_corners=True: assemble_hypercolumn's resize; one
    float32 add; nothing is added without a prev), then, with normalize, every texel divided by max(n, 1e-12), n its L2
    norm over the channels (assemble_hypercolumn's norm with torch.nn.functional.normalize's clamp: an all-zero
    column gives 0; a NaN makes its own column NaN and no other).  out: a tensor of that shape to write into; it MAY
    BE cur itself (the reference's in-place +=), and must not overlap prev.  One launch, asynchronous on `stream`
    (a torch.cuda.Stream; default: the current stream)."""
    cur, prev, out, (b, c, h, w, hp, wp) = _step_args(cur, prev, out, "cuda")
    flags = _lib.PYR_NORMALIZE if normalize else 0
    rc = _launch(cur.device, stream, (cur, prev, out), lambda s: _lib.load().fmpnp_dense_pyramid_step_async(
        _vp(cur), _vp(prev), b, c, h, w, hp, wp, _vp(out), flags, s))
    _lib.check(rc, "fmpnp_dense_pyramid_step_async")
    return out


def dense_pyramid_step_cpu(cur, prev=None, normalize=True, out=None, n_threads=0):
    """The CPU twin (fmpnp_dense_pyramid_step_cpu) on float32 CPU tensors: dense_pyramid_step's result bit for bit, for
    any n_threads; out may be cur."""
    cur, prev, out, (b, c, h, w, hp, wp) = _step_args(cur, prev, out, "cpu")
    rc = _lib.load().fmpnp_dense_pyramid_step_cpu(_vp(cur), _vp(prev), b, c, h, w, hp, wp, _vp(out),
                                                  _lib.PYR_NORMALIZE if normalize else 0, int(n_threads))
    _lib.check(rc, "fmpnp_dense_pyramid_step_cpu")
    return out


D2NET_WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512)


def d2net_trunk(widths=D2NET_WIDTHS):
    """The untrained nn.Sequential of a D2-Net trunk's shape: 3-64-64, max-pool; 128-128, max-pool; 256-256-256,
    AvgPool2d(2, stride=1); 512-512-512 dilated by 2 with padding 2; a ReLU after every convolution but the last (the
    extractor's use_relu is the one behind it).  widths: the ten convolutions' output channels (narrower trunks of
    the same shape, for tests).  The d2-net sources are not part of this repository: that a checkpoint of theirs loads
    into this module's state_dict key for key is NOT pinned by any test here."""
    widths = tuple(int(c) for c in widths)
    if len(widths) != 10 or min(widths) < 1:
        raise ValueError("widths names the ten convolutions' output channels")
    layers, cin = [], 3
    for k, cout in enumerate(widths):
        d = 2 if k >= 7 else 1
        layers.append(nn.Conv2d(cin, cout, 3, padding=d, dilation=d))
        if k < 9:
            layers.append(nn.ReLU(inplace=True))
        if k in (1, 3):
            layers.append(nn.MaxPool2d(2, stride=2))
        elif k == 6:
            layers.append(nn.AvgPool2d(2, stride=1))
        cin = cout
    return nn.Sequential(*layers).eval()


def d2net_preprocess(image_hwc_uint8, preprocessing="caffe"):
    """An RGB image [H, W, 3] (uint8 or anything numeric) -> the float32 [3, H, W] array a D2-Net trunk takes, on the
    host with numpy.  "torch": / 255, then ImageNet's mean (0.485, 0.456, 0.406) and std (0.229, 0.224, 0.225) per
    channel; "caffe": RGB to BGR, minus (103.939, 116.779, 123.68); None: the values as they are.  The d2-net sources
    are not part of this repository: parity with their preprocess_image is NOT pinned by any test here."""
    image = np.asarray(image_hwc_uint8)
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("d2net_preprocess takes an [H, W, 3] image")
    image = image.astype(np.float32).transpose(2, 0, 1)
    if preprocessing is None:
        return np.ascontiguousarray(image)
    if preprocessing == "caffe":
        mean = np.array([103.939, 116.779, 123.68], dtype=np.float32)
        return np.ascontiguousarray(image[::-1] - mean.reshape(3, 1, 1))
    if preprocessing == "torch":
        mean = np.array([0.485, 0.456, 0.406], dtype=np.float32).reshape(3, 1, 1)
        std = np.array([0.229, 0.224, 0.225], dtype=np.float32).reshape(3, 1, 1)
        return np.ascontiguousarray((image / np.float32(255.0) - mean) / std)
    raise ValueError('preprocessing must be "caffe", "torch" or None')


MULTISCALE = (0.5, 1, 2)


class DenseFeatureExtractor:
    """extract_dense_features plus process_multiscale (s2dhm/d2net_utils/extract_dense_features.py:46-82,
    dense_pyramid.py:5-42) around the caller's trunk, as HypercolumnExtractor is around the caller's encoder.

    trunk: an nn.Sequential of a D2-Net trunk's children (d2net_trunk() builds an untrained one); use_relu: a ReLU
    behind it.  scales: the pyramid's image scales in order (multiscale=True: (.5, 1, 2), the reference's).
    image_loader(paths, image_size, resize, device) -> a [1, 3, H, W] tensor or a list of one [3, H, W] tensor;
    without one, compute_hypercolumn takes tensors only (no image decoding here; d2net_preprocess is the host-side
    value transform).  One image at a time, as the reference asserts.
    backend: "hip" (default) walks the trunk through fmpnp.encoder.HipEncoder -- the kernels where the trunk lives on a
    CUDA device, the CPU twins on the CPU, bit-identical -- resizes the image with assemble_hypercolumn and steps the
    pyramid with dense_pyramid_step: every value is exact-fp32 with a stated order, so the map does not depend on the
    machine's choice of algorithm.  The dilated convolution has no fp16 precision, so there is no precision
    argument.  "torch" runs the framework's children, F.interpolate and F.normalize in the trunk's dtype: the
    restatement the tests compare against."""

    def __init__(self, trunk, use_relu=True, scales=(1,), image_loader=None, device=None, backend="hip", multiscale=False):
        if backend not in ("torch", "hip"):
            raise ValueError('backend must be "torch" or "hip"')
        if not isinstance(trunk, nn.Sequential):
            raise TypeError("DenseFeatureExtractor takes an nn.Sequential")
        self.trunk = trunk
        self.use_relu = bool(use_relu)
        self.scales = tuple(MULTISCALE if multiscale else scales)
        if not self.scales or not all(isinstance(s, (int, float)) and math.isfinite(s) and s > 0 for s in self.scales):
            raise ValueError("scales must be positive numbers")
        self.backend = backend
        self._hip = HipEncoder(trunk) if backend == "hip" else None
        self.image_loader = image_loader
        p = next(trunk.parameters(), None)
        if device is None:
            device = p.device if p is not None else torch.device("cuda")
        self.device = torch.device(device)
        self.dtype = p.dtype if p is not None and backend == "torch" else torch.float32

    def _image(self, image, image_size, resize):
        items = list(image) if isinstance(image, (list, tuple)) else [image]
        if items and all(torch.is_tensor(t) for t in items):
            batch = items[0] if len(items) == 1 and items[0].dim() == 4 else torch.stack(
                [t if t.dim() == 3 else t.squeeze(0) for t in items])
        elif self.image_loader is None:
            raise TypeError("compute_hypercolumn takes image tensors; paths need an image_loader")
        else:
            batch = self.image_loader(items, image_size, resize, self.device)
            if not torch.is_tensor(batch):
                batch = torch.stack(list(batch))
        if batch.dim() != 4 or batch.shape[0] != 1:
            raise ValueError(f"one image at a time ([1, 3, H, W]), not {tuple(batch.shape)}")
        return batch.detach().to(device=self.device, dtype=self.dtype).contiguous()

    def _scaled(self, image, size):
        if tuple(image.shape[2:]) == size:
            return image
        if min(size) < 1:
            raise ValueError(f"a scale leaves no image ({size[0]} x {size[1]})")
        if self.backend == "torch":
            return torch.nn.functional.interpolate(image, size=size, mode="bilinear", align_corners=True)
        resize = assemble_hypercolumn if image.is_cuda else assemble_hypercolumn_cpu
        return resize([image], size, normalize=False)

    def extract(self, image):
        """image: a [1, 3, H, W] (or [3, H, W]) tensor -> the [1, C, h, w] dense map: for every scale s in order, the
        image resized to floor(H s) x floor(W s) (align_corners=True; scale 1 is the image itself), the trunk, the ReLU
        (use_relu; one launch with the last convolution), then the pyramid's step with the previous scale's map."""
        image = self._image(image, None, False)
        height, width = (int(s) for s in image.shape[2:])
        prev = None
        with torch.no_grad():
            for s in self.scales:
                scaled = self._scaled(image, (int(math.floor(height * s)), int(math.floor(width * s))))
                if self.backend == "torch":
                    cur = self.trunk(scaled)
                    if self.use_relu:
                        cur = torch.relu(cur)
                    if prev is not None:
                        cur = cur + torch.nn.functional.interpolate(prev, size=cur.shape[2:], mode="bilinear",
                                                                    align_corners=True)
                    prev = torch.nn.functional.normalize(cur, dim=1)
                else:
                    cur = self._hip(scaled, relu=self.use_relu)
                    step = dense_pyramid_step if cur.is_cuda else dense_pyramid_step_cpu
                    # (in place, as the reference's +=, unless an empty trunk handed the image itself back)
                    prev = step(cur, prev, out=cur if cur.data_ptr() != scaled.data_ptr() else None)
        return prev

    def compute_hypercolumn(self, image, image_size=None, resize=True, to_cpu=False):
        """HypercolumnExtractor.compute_hypercolumn's signature, so the object can stand wherever a `net` stands: image
        (one [1, 3, H, W] or [3, H, W] tensor, a list of one, or with an image_loader a list of one path) ->
        (the dense map [1, C, h, w], image_resolution (H, W)); to_cpu: a numpy array, as the reference returns."""
        batch = self._image(image, image_size, resize)
        dense = self.extract(batch)
        if to_cpu:
            dense = dense.cpu().numpy()
        return dense, batch.shape[2:]
