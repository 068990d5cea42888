"""Hypercolumn assembly on the GPU: the second half of ImageRetrievalModel.compute_hypercolumn
(s2dhm/network/network.py:149-173) -- every recorded layer resized to the first layer's size (bilinear,
align_corners=True), concatenated along the channels and L2-normalised per texel -- in one kernel
(libfmpnp's fmpnp_hypercolumn_assemble; include/fmpnp.h states the numeric contract).

assemble_hypercolumn runs it on CUDA tensors, assemble_hypercolumn_cpu runs the CPU twin (bit-identical
results; an explicit entry point, never a fallback).  sparse_hypercolumn / sparse_hypercolumn_cpu form the
hypercolumn's descriptors at single points straight from the layers (fmpnp_hypercolumn_sparse): the rows of
"assemble, then gather", bit for bit, without the dense map.  HypercolumnExtractor walks the caller's encoder (a
stock nn.Sequential: the convolutions stay PyTorch's unless backend="hip" asks for fmpnp.encoder's) as
network.py:134-147 does and assembles the recorded maps; it offers compute_hypercolumn, so an instance can be
passed as `net` to fmpnp.optimize_feature_pnp.
"""
import ctypes

import numpy as np
import torch

from . import _lib


def _layers(feature_maps, device_kind):
    """The fmpnp_hc_layer array of the maps and the tensors it points into (the caller keeps them alive)."""
    maps = list(feature_maps)
    if not 1 <= len(maps) <= 8:
        raise ValueError(f"1 to 8 feature maps, got {len(maps)}")
    keep = []
    for m in maps:
        if not torch.is_tensor(m) or m.dim() != 4 or m.dtype != torch.float32 or m.device.type != device_kind:
            raise ValueError(f"every feature map must be a float32 {device_kind} tensor [B, C, H, W]")
        if m.device != maps[0].device or m.shape[0] != maps[0].shape[0]:
            raise ValueError("the feature maps must share one device and one batch size")
        if min(m.shape) < 1:
            raise ValueError(f"empty feature map {tuple(m.shape)}")
        if m.stride(3) != 1 or m.stride(2) < m.shape[3] or min(m.stride()) < 0:
            m = m.contiguous()  # (rows must be dense; batch, channel and row strides are free)
        keep.append(m.detach())
    layers = (_lib.HcLayer * len(keep))()
    for d, m in zip(layers, keep):
        d.data = m.data_ptr()
        d.C, d.H, d.W = (int(s) for s in m.shape[1:])
        d.stride_b, d.stride_c, d.stride_y = (int(s) for s in m.stride()[:3])
    return layers, keep


def _plane_layers(feature_maps, device_kind):
    """_layers for layered matching (fmpnp_exhaustive_match_layers), which reads layer l as [C_l][H_l * W_l] with
    ld = the channel stride: every plane contiguous (stride_y == W_l, stride_c >= H_l * W_l).  A map that is not
    is copied; the strides of one-element dimensions, which the framework leaves arbitrary, are written as a
    contiguous tensor's."""
    layers, keep = _layers(feature_maps, device_kind)
    for k, (d, m) in enumerate(zip(layers, keep)):
        b, c, h, w = (int(s) for s in m.shape)
        ok = ((w == 1 or m.stride(3) == 1) and (h == 1 or m.stride(2) == w) and (c == 1 or m.stride(1) >= h * w)
              and (b == 1 or m.stride(0) >= 0))
        if not ok:
            keep[k] = m = m.contiguous()
            d.data = m.data_ptr()
        d.stride_y = w
        d.stride_c = h * w if c == 1 else int(m.stride(1))
        d.stride_b = 0 if b == 1 else int(m.stride(0))
    return layers, keep


def _describe(feature_maps, size, out, device_kind):
    """The fmpnp_hc_layer array of the maps (kept alive by the returned list), the output and its size."""
    layers, keep = _layers(feature_maps, device_kind)
    batch = int(keep[0].shape[0])
    height, width = (int(s) for s in (keep[0].shape[2:] if size is None else size))
    channels = sum(int(m.shape[1]) for m in keep)
    shape = (batch, channels, height, width)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=keep[0].device)
    elif (not torch.is_tensor(out) or tuple(out.shape) != shape or out.dtype != torch.float32
          or out.device != keep[0].device or out.stride(3) != 1 or out.stride(2) < width or min(out.stride()) < 0):
        raise ValueError(f"out must be a float32 tensor {shape} on {keep[0].device} with dense rows")
    return layers, keep, out, shape


def _flags(normalize, stores=None):
    if stores not in (None, "dword", "vector"):
        raise ValueError('stores must be None, "dword" or "vector"')
    knob = {None: 0, "dword": _lib.HC_DWORD_STORES, "vector": _lib.HC_VECTOR_STORES}[stores]
    return (_lib.HC_NORMALIZE if normalize else 0) | knob


def assemble_hypercolumn(feature_maps, size=None, normalize=True, out=None, stream=None, stores=None):
    """feature_maps: 1 to 8 float32 CUDA tensors [B, C_l, H_l, W_l] (any batch, channel and row strides) ->
    the [B, sum C_l, H, W] float32 CUDA hypercolumn: each map resized to size (default: the first map's
    (H, W), as the reference) and its channels appended, then every texel divided by its L2 norm over the
    channels (normalize).  out: a tensor of that shape to write into (it may be a view with dense rows).
    Asynchronous on `stream` (a torch.cuda.Stream; default: the device's current stream).  stores
    ("dword" / "vector": 4- or 16-byte stores; None: the library's choice) is a launch knob for measurements:
    the results do not depend on it."""
    layers, keep, out, (batch, _, height, width) = _describe(feature_maps, size, out, "cuda")
    device = out.device
    _lib.require_device(device)
    s = torch.cuda.current_stream(device) if stream is None else stream
    with torch.cuda.device(device):
        rc = _lib.load().fmpnp_hypercolumn_assemble_async(
            layers, len(keep), batch, out.data_ptr(), height, width, out.stride(0), out.stride(1), out.stride(2),
            _flags(normalize, stores), ctypes.c_void_p(s.cuda_stream))
    _lib.check(rc, "fmpnp_hypercolumn_assemble_async")
    for m in keep + [out]:
        m.record_stream(s)  # (the caching allocator must not hand the memory on before the kernel has run)
    return out


def assemble_hypercolumn_cpu(feature_maps, size=None, normalize=True, out=None, n_threads=0):
    """The CPU twin (fmpnp_hypercolumn_assemble_cpu) on float32 CPU tensors: assemble_hypercolumn's result
    bit for bit."""
    layers, keep, out, (batch, _, height, width) = _describe(feature_maps, size, out, "cpu")
    rc = _lib.load().fmpnp_hypercolumn_assemble_cpu(
        layers, len(keep), batch, out.data_ptr(), height, width, out.stride(0), out.stride(1), out.stride(2),
        _flags(normalize), int(n_threads))
    _lib.check(rc, "fmpnp_hypercolumn_assemble_cpu")
    return out


_AT = {"texel": _lib.HC_AT_TEXEL, "reference": _lib.HC_AT_REFERENCE, "cell": _lib.HC_AT_CELL}
_OUT_DTYPES = {torch.float32: _lib.F32, torch.float64: _lib.F64}


def _sparse_args(feature_maps, points, at, image_shape, cell_size, item, size, dtype, out, device_kind):
    """The arguments of fmpnp_hypercolumn_sparse* on the maps' device: (layers, keep, B, H, W, points tensor, item
    tensor or None, N, at code, p0, p1, out, ld_out, C)."""
    if at not in _AT:
        raise ValueError('at must be "reference", "cell" or "texel"')
    if dtype not in _OUT_DTYPES:
        raise ValueError("dtype must be torch.float32 or torch.float64")
    layers, keep = _layers(feature_maps, device_kind)
    device = keep[0].device
    batch = int(keep[0].shape[0])
    height, width = (int(s) for s in (keep[0].shape[2:] if size is None else size))
    channels = sum(int(m.shape[1]) for m in keep)
    p0 = p1 = 0.0
    if at == "reference":
        if image_shape is None:
            raise ValueError('at="reference" needs image_shape = (img0, img1)')
        p0, p1 = float(image_shape[0]), float(image_shape[1])
    elif at == "cell":
        if cell_size is None:
            raise ValueError('at="cell" needs cell_size, as generate_dense_keypoints returns it')
        p0, p1 = float(cell_size[0]), float(cell_size[1])
    want = torch.int32 if at == "texel" else torch.float64
    pts = points if torch.is_tensor(points) else torch.as_tensor(np.asarray(points))
    pts = pts.detach().reshape(-1, 2).to(device=device, dtype=want).contiguous()
    n = int(pts.shape[0])
    if item is not None:
        item = item if torch.is_tensor(item) else torch.as_tensor(np.asarray(item))
        item = item.detach().reshape(-1).to(device=device, dtype=torch.int32).contiguous()
        if int(item.shape[0]) != n:
            raise ValueError("item must name one batch item per point")
    if out is None:
        out = torch.empty((n, channels), dtype=dtype, device=device)
    elif (not torch.is_tensor(out) or tuple(out.shape) != (n, channels) or out.dtype != dtype or out.device != device
          or (channels > 1 and out.stride(1) != 1) or (n > 1 and out.stride(0) < channels)):
        raise ValueError(f"out must be a {dtype} tensor {(n, channels)} on {device} with dense rows")
    ld = int(out.stride(0)) if n > 1 else channels
    return layers, keep, batch, height, width, pts, item, n, _AT[at], p0, p1, out, ld, channels


_OUT_OF_MAP = ("a point maps outside the hypercolumn, or names a batch item the maps do not have "
               "(optimize_feature_pnp.py:56 raises IndexError)")


def sparse_hypercolumn(feature_maps, points, at="reference", image_shape=None, cell_size=None, item=None, size=None,
                       normalize=True, dtype=torch.float32, out=None, stream=None):
    """The hypercolumn's descriptors at N points, formed straight from the layers: [N, sum C_l] on the maps'
    device, bit for bit the rows that assemble_hypercolumn followed by a gather gives, without the dense map
    (libfmpnp's fmpnp_hypercolumn_sparse; include/fmpnp.h states the contract).

    feature_maps, size, normalize: as assemble_hypercolumn.  points: [N, 2], numpy or a tensor --
    at="reference": (x, y) image coordinates with image_shape = (img0, img1), gather_reference's index;
    at="cell": (x, y) with cell_size as generate_dense_keypoints returns it, fast_sparse_keypoint_descriptor's
    index (never out of the map); at="texel": integer (row, col) of the hypercolumn.  item: the batch item of
    each point (default 0).  dtype: float32, or float64 (the float32 value widened).  out: a [N, C] tensor to
    write into (it may be a view with a longer row stride; nothing else is written).  Raises IndexError when a
    point lies outside the map (the other rows are valid in `out`), as feature_pnp does; at="cell" cannot, and
    is asynchronous on `stream` (default: the current stream), the other two wait for it."""
    (layers, keep, batch, height, width, pts, item, n, code, p0, p1, out, ld,
     _) = _sparse_args(feature_maps, points, at, image_shape, cell_size, item, size, dtype, out, "cuda")
    device = out.device
    _lib.require_device(device)
    s = torch.cuda.current_stream(device) if stream is None else stream
    if stream is not None:
        s.wait_stream(torch.cuda.current_stream(device))  # (the points were uploaded on the current stream)
    args = (layers, len(keep), batch, height, width, pts.data_ptr(), item.data_ptr() if item is not None else None, n,
            code, p0, p1, out.data_ptr(), _OUT_DTYPES[dtype], ld, _lib.HC_NORMALIZE if normalize else 0)
    with torch.cuda.device(device):
        if at == "cell":
            rc = _lib.load().fmpnp_hypercolumn_sparse_async(*args, None, ctypes.c_void_p(s.cuda_stream))
        else:
            rc = _lib.load().fmpnp_hypercolumn_sparse(*args, None, ctypes.c_void_p(s.cuda_stream))
    for m in keep + [pts, out] + ([item] if item is not None else []):
        m.record_stream(s)
    if rc == _lib.ERANGE:
        raise IndexError(_OUT_OF_MAP)
    _lib.check(rc, "fmpnp_hypercolumn_sparse")
    return out


def sparse_hypercolumn_cpu(feature_maps, points, at="reference", image_shape=None, cell_size=None, item=None,
                           size=None, normalize=True, dtype=torch.float32, out=None, n_threads=0):
    """The CPU twin (fmpnp_hypercolumn_sparse_cpu) on float32 CPU tensors: sparse_hypercolumn's result bit for
    bit, IndexError included."""
    (layers, keep, batch, height, width, pts, item, n, code, p0, p1, out, ld,
     _) = _sparse_args(feature_maps, points, at, image_shape, cell_size, item, size, dtype, out, "cpu")
    rc = _lib.load().fmpnp_hypercolumn_sparse_cpu(
        layers, len(keep), batch, height, width, pts.data_ptr(), item.data_ptr() if item is not None else None, n,
        code, p0, p1, out.data_ptr(), _OUT_DTYPES[dtype], ld, _lib.HC_NORMALIZE if normalize else 0, None,
        int(n_threads))
    if rc == _lib.ERANGE:
        raise IndexError(_OUT_OF_MAP)
    _lib.check(rc, "fmpnp_hypercolumn_sparse_cpu")
    return out


def _pack_args(feature_maps, size, item, storage, layout, channels, device_kind):
    """The checked arguments both pack_hypercolumn forms share: (layers, keep, batch, item, H, W, C, cstride,
    (c_begin, c_end), storage dtype, output shape)."""
    if layout not in ("fgrad", "f"):
        raise ValueError("layout must be 'fgrad' or 'f'")
    storage = torch.float32 if storage is None else storage
    if storage not in _OUT_DTYPES or (layout == "f" and storage != torch.float32):
        raise ValueError("storage must be torch.float32, or torch.float64 for layout 'fgrad'")
    layers, keep = _layers(feature_maps, device_kind)
    batch = int(keep[0].shape[0])
    item = int(item)
    if not 0 <= item < batch:
        raise ValueError(f"item {item} of a batch of {batch}")
    height, width = (int(s) for s in (keep[0].shape[2:] if size is None else size))
    total = sum(int(m.shape[1]) for m in keep)
    c_begin, c_end = (0, total) if channels is None else (int(channels[0]), int(channels[1]))
    if not 0 <= c_begin < c_end <= total:
        raise ValueError(f"channels {(c_begin, c_end)} is no range of the {total} concatenated channels")
    cs = (total + 3) // 4 * 4
    shape = (height, width, 3, cs) if layout == "fgrad" else (height, width, cs)
    return layers, keep, batch, item, height, width, total, cs, (c_begin, c_end), storage, shape


def pack_hypercolumn(feature_maps, size=None, normalize=True, item=0, storage=None, layout="fgrad",
                     sobel_normalized=False, sobel_replicate_pad=False, channels=None, marks=None, out=None,
                     stream=None):
    """The encoder's layers straight into the refiner's packed layout -> PackedFeatures, bit for bit what
    pack_features(assemble_hypercolumn(feature_maps, size, normalize)[item], ...) gives, without the dense
    [C, H, W] map (libfmpnp's fmpnp_hypercolumn_pack; include/fmpnp.h states the contract).

    feature_maps, size, normalize: as assemble_hypercolumn.  item: the batch item to pack.  storage: float32
    (default), or float64 for layout "fgrad".  layout, sobel_normalized, sobel_replicate_pad: as pack_features.
    channels: (c_begin, c_end) of the concatenated channels to write (default: all).  marks: a uint8 / bool CUDA
    tensor [H, W]; only texels with a non-zero mark are written (default: all).  out: a contiguous CUDA tensor
    [H, W, 3, cstride] ([H, W, cstride] for layout "f"; cstride = C rounded up to 4) of the storage dtype to write
    into -- only the channels and texels named above are written, everything else in it stays as it is; without
    it the buffer is allocated as pack_features does (padding channels zero; with channels or marks the rest is
    zero too).  Asynchronous on `stream` (a torch.cuda.Stream; default: the current stream)."""
    from .refine import PackedFeatures
    (layers, keep, batch, item, height, width, total, cs, (c_begin, c_end), storage,
     shape) = _pack_args(feature_maps, size, item, storage, layout, channels, "cuda")
    device = keep[0].device
    _lib.require_device(device)
    s = torch.cuda.current_stream(device) if stream is None else stream
    with torch.cuda.device(device), torch.cuda.stream(s):
        if marks is not None:
            if (not torch.is_tensor(marks) or tuple(marks.shape) != (height, width) or marks.device != device
                    or marks.dtype not in (torch.uint8, torch.bool)):
                raise ValueError(f"marks must be a uint8 or bool tensor {(height, width)} on {device}")
            marks = marks.contiguous()
        if out is None:
            whole = cs == total and marks is None and (c_begin, c_end) == (0, total)
            out = (torch.empty if whole else torch.zeros)(shape, dtype=storage, device=device)
        elif (not torch.is_tensor(out) or tuple(out.shape) != shape or out.dtype != storage or out.device != device
              or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous {storage} tensor {list(shape)} on {device}")
        lib = _lib.load()
        work = None
        if normalize:
            work = torch.empty(int(lib.fmpnp_hypercolumn_pack_workspace_size(height, width)), dtype=torch.uint8,
                               device=device)
        rc = lib.fmpnp_hypercolumn_pack_async(
            layers, len(keep), batch, item, height, width, _lib.HC_NORMALIZE if normalize else 0, c_begin, c_end,
            _lib.LAYOUT_FGRAD if layout == "fgrad" else _lib.LAYOUT_F, _OUT_DTYPES[storage], cs,
            int(bool(sobel_normalized)), int(bool(sobel_replicate_pad)),
            marks.data_ptr() if marks is not None else None, out.data_ptr(),
            work.data_ptr() if work is not None else None, work.numel() if work is not None else 0,
            ctypes.c_void_p(s.cuda_stream))
    _lib.check(rc, "fmpnp_hypercolumn_pack_async")
    for m in keep + [out] + [t for t in (marks, work) if t is not None]:
        m.record_stream(s)  # (the caching allocator must not hand the memory on before the kernels have run)
    flags = int(bool(sobel_normalized)) | (int(bool(sobel_replicate_pad)) << 1)
    return PackedFeatures(out, total, height, width, cs, layout, flags if layout == "f" else 0)


def pack_hypercolumn_cpu(feature_maps, size=None, normalize=True, item=0, storage=None, layout="fgrad",
                         sobel_normalized=False, sobel_replicate_pad=False, channels=None, marks=None, out=None,
                         n_threads=0):
    """The CPU twin (fmpnp_hypercolumn_pack_cpu) on float32 CPU tensors: pack_hypercolumn's buffer bit for bit, as
    a numpy array in fmpnp.cpu.pack_host's layout ([H][W][3][cstride] or [H][W][cstride]).  marks: a uint8 / bool
    array or tensor [H, W]; out: a C-contiguous numpy array of that layout to write into (the rest of it stays as
    it is); without it the array starts as zeros."""
    (layers, keep, batch, item, height, width, total, cs, (c_begin, c_end), storage,
     shape) = _pack_args(feature_maps, size, item, storage, layout, channels, "cpu")
    np_dtype = np.float32 if storage == torch.float32 else np.float64
    if marks is not None:
        marks = np.ascontiguousarray(marks.numpy() if torch.is_tensor(marks) else marks)
        if marks.shape != (height, width) or marks.dtype not in (np.uint8, np.bool_):
            raise ValueError(f"marks must be a uint8 or bool array {(height, width)}")
    if out is None:
        out = np.zeros(shape, dtype=np_dtype)
    elif (not isinstance(out, np.ndarray) or out.shape != shape or out.dtype != np_dtype
          or not out.flags.c_contiguous or not out.flags.writeable):
        raise ValueError(f"out must be a C-contiguous {np_dtype.__name__} array {list(shape)}")
    rc = _lib.load().fmpnp_hypercolumn_pack_cpu(
        layers, len(keep), batch, item, height, width, _lib.HC_NORMALIZE if normalize else 0, c_begin, c_end,
        _lib.LAYOUT_FGRAD if layout == "fgrad" else _lib.LAYOUT_F, _OUT_DTYPES[storage], cs,
        int(bool(sobel_normalized)), int(bool(sobel_replicate_pad)),
        marks.ctypes.data if marks is not None else None, out.ctypes.data, int(n_threads))
    _lib.check(rc, "fmpnp_hypercolumn_pack_cpu")
    return out


class HypercolumnExtractor:
    """compute_hypercolumn (network.py:111-176) around the caller's encoder.

    encoder: an nn.Sequential (for instance a stock VGG16's features); hypercolumn_layers: ascending child
    indices -- the INPUT of child i is recorded for each listed i, and the walk stops after the last
    (network.py:134-147).  image_loader(paths, image_size, resize, device) -> a [B, 3, H, W] tensor or a list
    of [3, H, W] tensors; without one, compute_hypercolumn takes tensors only (no image decoding here).
    The maps are assembled where the encoder lives: on its CUDA device by the kernel; an encoder on the CPU
    is the caller's explicit choice of the CPU twin.
    backend: "torch" (default) runs the encoder's children as the framework does; "hip" (opt-in) runs them through
    fmpnp.encoder.HipEncoder -- libfmpnp's exact-fp32 convolution, ReLU and max-pool, whose bits do not depend on
    the batch or the machine's choice of algorithm (3x3 / stride 1 / padding 1 Conv2d, ReLU and MaxPool2d(2, 2)
    children only; TypeError otherwise).  Everything downstream of the walk is the same.
    precision: "f32" (default), or with backend="hip" the opt-in "f16": HipEncoder's fp16 matrix-core convolutions
    (binary16 operands, fp32 accumulation, float32 maps as before); with backend="torch" anything but "f32" is a
    ValueError."""

    def __init__(self, encoder, hypercolumn_layers, image_loader=None, device=None, backend="torch", precision="f32"):
        if backend not in ("torch", "hip"):
            raise ValueError('backend must be "torch" or "hip"')
        if precision not in ("f32", "f16"):
            raise ValueError(f'precision must be "f32" or "f16", not {precision!r}')
        if precision != "f32" and backend != "hip":
            raise ValueError('precision="f16" needs backend="hip"')
        self.encoder = encoder
        self.backend = backend
        self.precision = precision
        self._hip = None
        if backend == "hip":
            from .encoder import HipEncoder
            self._hip = HipEncoder(encoder, precision=precision)
        self.hypercolumn_layers = [int(i) for i in hypercolumn_layers]
        if not self.hypercolumn_layers or sorted(set(self.hypercolumn_layers)) != self.hypercolumn_layers:
            raise ValueError("hypercolumn_layers must be ascending, distinct child indices")
        if not 1 <= len(self.hypercolumn_layers) <= 8:
            raise ValueError("1 to 8 hypercolumn layers")
        if self.hypercolumn_layers[0] < 0 or self.hypercolumn_layers[-1] >= len(list(encoder.children())):
            raise ValueError("hypercolumn_layers name children the encoder does not have")
        self.image_loader = image_loader
        if device is None:
            p = next(encoder.parameters(), None)
            device = p.device if p is not None else torch.device("cuda")
        self.device = torch.device(device)

    def _images(self, image, image_size, resize):
        items = list(image) if isinstance(image, (list, tuple)) else [image]
        if items and all(torch.is_tensor(t) for t in items):
            if len(items) == 1 and items[0].dim() == 4:
                batch = items[0]
            else:
                batch = torch.stack([t if t.dim() == 3 else t.squeeze(0) for t in items])
            return batch.to(device=self.device, dtype=torch.float32)
        if self.image_loader is None:
            raise TypeError("compute_hypercolumn takes image tensors; paths need an image_loader")
        loaded = self.image_loader(items, image_size, resize, self.device)
        if not torch.is_tensor(loaded):
            loaded = torch.stack(list(loaded))
        return loaded.to(device=self.device, dtype=torch.float32)

    def feature_maps(self, batch):
        """The layer walk of network.py:134-147: the input of every listed child, in order."""
        if self._hip is not None:
            return self._hip.feature_maps(batch, self.hypercolumn_layers)
        maps, j = [], 0
        feature_map = batch
        with torch.no_grad():
            for i, layer in enumerate(self.encoder.children()):
                if j == len(self.hypercolumn_layers):
                    break
                if i == self.hypercolumn_layers[j]:
                    maps.append(feature_map)
                    j += 1
                feature_map = layer(feature_map)
        return maps

    def compute_feature_maps(self, image, image_size=None, resize=True):
        """The first half of compute_hypercolumn: image (as compute_hypercolumn takes it) -> (the recorded
        layers, image_resolution (H, W)).  assemble_hypercolumn of the layers is compute_hypercolumn's map;
        sparse_hypercolumn of them is its descriptors at points."""
        batch = self._images(image, image_size, resize)
        return self.feature_maps(batch), batch.shape[2:]

    def compute_sparse_hypercolumn(self, image, points, at="reference", image_size=None, resize=True, **kwargs):
        """compute_hypercolumn's descriptors at `points` without the dense map -> ([N, C], image_resolution);
        at and the keyword arguments are sparse_hypercolumn's."""
        maps, image_resolution = self.compute_feature_maps(image, image_size, resize)
        if self.device.type == "cuda":
            rows = sparse_hypercolumn(maps, points, at=at, **kwargs)
        else:
            rows = sparse_hypercolumn_cpu(maps, points, at=at, **kwargs)
        return rows, image_resolution

    def match(self, image, sparse_descriptor_maps, image_shape, cell_size, factor=None, image_size=None, resize=True):
        """exhaustive_search_multi of the image against the references' sparse descriptor maps without the image's
        dense hypercolumn: compute_feature_maps, then fmpnp.match.exhaustive_search_layers_multi on the layers
        (layered matching; the encoder must live on a CUDA device).  Returns ([(points, mask), ...],
        image_resolution)."""
        from .match import exhaustive_search_layers_multi
        maps, image_resolution = self.compute_feature_maps(image, image_size, resize)
        return exhaustive_search_layers_multi(maps, sparse_descriptor_maps, image_shape, cell_size, factor), image_resolution

    def compute_hypercolumn(self, image, image_size=None, resize=True, to_cpu=False):
        """image: a [B, 3, H, W] or [3, H, W] tensor, a list of [3, H, W] tensors, or (with an image_loader)
        a list of paths -> (hypercolumn [B, C, h, w], image_resolution (H, W)); to_cpu: a numpy array, as
        the reference returns."""
        maps, image_resolution = self.compute_feature_maps(image, image_size, resize)
        if self.device.type == "cuda":
            hypercolumn = assemble_hypercolumn(maps)
        else:
            hypercolumn = assemble_hypercolumn_cpu(maps)
        if to_cpu:
            hypercolumn = hypercolumn.cpu().numpy()
        return hypercolumn, image_resolution
