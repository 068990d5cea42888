"""Hypercolumn assembly on the GPU: the second half of ImageRetrievalModel.compute_hypercolumn
(s2dhm/network/network.py:149-173) -- every recorded layer resized to the first layer's size (bilinear,
align_corners=True), concatenated along the channels and L2-normalised per texel -- in one kernel
(libfmpnp's fmpnp_hypercolumn_assemble; include/fmpnp.h states the numeric contract).

assemble_hypercolumn runs it on CUDA tensors, assemble_hypercolumn_cpu runs the CPU twin (bit-identical
results; an explicit entry point, never a fallback).  HypercolumnExtractor walks the caller's encoder (a
stock nn.Sequential: the convolutions stay PyTorch's) as network.py:134-147 does and assembles the recorded
maps; it offers compute_hypercolumn, so an instance can be passed as `net` to fmpnp.optimize_feature_pnp.
"""
import ctypes

import torch

from . import _lib


def _describe(feature_maps, size, out, device_kind):
    """The fmpnp_hc_layer array of the maps (kept alive by the returned list), the output and its size."""
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
    batch = int(keep[0].shape[0])
    height, width = (int(s) for s in (keep[0].shape[2:] if size is None else size))
    channels = sum(int(m.shape[1]) for m in keep)
    shape = (batch, channels, height, width)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=keep[0].device)
    elif (not torch.is_tensor(out) or tuple(out.shape) != shape or out.dtype != torch.float32
          or out.device != keep[0].device or out.stride(3) != 1 or out.stride(2) < width or min(out.stride()) < 0):
        raise ValueError(f"out must be a float32 tensor {shape} on {keep[0].device} with dense rows")
    layers = (_lib.HcLayer * len(keep))()
    for d, m in zip(layers, keep):
        d.data = m.data_ptr()
        d.C, d.H, d.W = (int(s) for s in m.shape[1:])
        d.stride_b, d.stride_c, d.stride_y = (int(s) for s in m.stride()[:3])
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


class HypercolumnExtractor:
    """compute_hypercolumn (network.py:111-176) around the caller's encoder.

    encoder: an nn.Sequential (for instance a stock VGG16's features); hypercolumn_layers: ascending child
    indices -- the INPUT of child i is recorded for each listed i, and the walk stops after the last
    (network.py:134-147).  image_loader(paths, image_size, resize, device) -> a [B, 3, H, W] tensor or a list
    of [3, H, W] tensors; without one, compute_hypercolumn takes tensors only (no image decoding here).
    The maps are assembled where the encoder lives: on its CUDA device by the kernel; an encoder on the CPU
    is the caller's explicit choice of the CPU twin."""

    def __init__(self, encoder, hypercolumn_layers, image_loader=None, device=None):
        self.encoder = encoder
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

    def compute_hypercolumn(self, image, image_size=None, resize=True, to_cpu=False):
        """image: a [B, 3, H, W] or [3, H, W] tensor, a list of [3, H, W] tensors, or (with an image_loader)
        a list of paths -> (hypercolumn [B, C, h, w], image_resolution (H, W)); to_cpu: a numpy array, as
        the reference returns."""
        batch = self._images(image, image_size, resize)
        image_resolution = batch.shape[2:]
        maps = self.feature_maps(batch)
        if self.device.type == "cuda":
            hypercolumn = assemble_hypercolumn(maps)
        else:
            hypercolumn = assemble_hypercolumn_cpu(maps)
        if to_cpu:
            hypercolumn = hypercolumn.cpu().numpy()
        return hypercolumn, image_resolution
