"""Dense exhaustive matching on the GPU: the stage that produces the 2D-3D matches the refiner
consumes (s2dhm/pose_prediction/exhaustive_search.py, keypoint_association.py; called per retrieved
reference image by sparse_to_dense_predictor.py:140-191).

exhaustive_search / exhaustive_search_multi keep the reference's signature and return values and run
libfmpnp's exact-fp32 MFMA correlation with its fused row reduction (fmpnp_exhaustive_match);
fast_sparse_keypoint_descriptor runs the closed-form nearest-cell gather
(fmpnp_gather_sparse_descriptors).  exhaustive_match_cpu is the CPU twin (bit-identical results), an
explicit entry point and never a fallback.

precision="f16" (opt-in; the default "f32" is the exact contract) runs the correlation on the fp16 matrix
cores: both operands rounded to binary16, fp32 accumulation (include/fmpnp.h, "fp16 precision").  It has no
bit-identical CPU twin; exhaustive_match_cpu(precision="f16") is its fp64-accumulated reference.

exhaustive_match_layers / exhaustive_search_layers(_multi) (opt-in) take the query as its encoder layers instead of
the dense map: the correlation runs on each layer at the layer's own resolution and the small score maps are
resized and summed (include/fmpnp.h, "layered matching"), exact fp32 in its own rounding order, with
exhaustive_match_layers_cpu as the bit-identical twin.
"""
import ctypes

import numpy as np
import torch

from . import _lib, config

RATIO = 0.9  # retrieve_argmax's default (exhaustive_search.py:8)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _rows(t, name):
    """An fp32 2-D CUDA tensor with unit column stride (rows may be padded: ld = stride(0))."""
    if t.dim() != 2:
        raise ValueError(f"{name} must be 2-D")
    if t.dtype != torch.float32 or not t.is_cuda:
        raise ValueError(f"{name} must be a float32 CUDA tensor")
    if t.shape[1] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    ld = t.stride(0) if t.shape[0] > 1 else t.shape[1]
    if ld < t.shape[1]:
        t, ld = t.contiguous(), t.shape[1]
    return t, ld


def exhaustive_match(sparse, dense, top_k, ratio=RATIO, scores=False, precision="f32"):
    """fmpnp_exhaustive_match on CUDA tensors: sparse [N, C], dense [C, WH] (fp32, rows may be padded
    views).  Returns dict(argmax int32 [N], top, kth float32 [N], mask bool [N]) as numpy arrays, plus
    scores (a CUDA tensor [N, WH]) when asked.  Waits on the current stream.  precision: "f32" (exact) or
    "f16" (fmpnp_exhaustive_match_ex with FMPNP_MATCH_F16)."""
    prec = _lib.match_precision(precision)
    sparse, ld_s = _rows(sparse, "sparse")
    dense, ld_d = _rows(dense, "dense")
    n, c = sparse.shape
    if dense.shape[0] != c:
        raise ValueError(f"sparse has {c} channels, dense {dense.shape[0]}")
    wh = dense.shape[1]
    _lib.require_device(sparse.device)
    argmax, top, kth = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    mask = np.zeros(n, np.uint8)
    out = torch.empty((n, wh), dtype=torch.float32, device=sparse.device) if scores else None
    with torch.cuda.device(sparse.device):
        if prec == _lib.MATCH_F32:
            rc = _lib.load().fmpnp_exhaustive_match(
                _vp(sparse), n, ld_s, _vp(dense), c, wh, ld_d, int(top_k), float(ratio), argmax.ctypes.data,
                top.ctypes.data, kth.ctypes.data, mask.ctypes.data, _vp(out) if scores else None,
                _lib.stream_ptr(sparse.device))
        else:
            rc = _lib.load().fmpnp_exhaustive_match_ex(
                _vp(sparse), n, ld_s, _vp(dense), c, wh, ld_d, int(top_k), float(ratio), argmax.ctypes.data,
                top.ctypes.data, kth.ctypes.data, mask.ctypes.data, _vp(out) if scores else None, prec,
                _lib.stream_ptr(sparse.device))
    _lib.check(rc, "fmpnp_exhaustive_match")
    res = dict(argmax=argmax, top=top, kth=kth, mask=mask.astype(bool))
    if scores:
        res["scores"] = out
    return res


def _host_rows(a):
    a = np.asarray(a)
    if a.dtype != np.float32 or a.ndim != 2:
        raise ValueError("expected a 2-D float32 array")
    if a.shape[1] > 1 and a.strides[1] != 4:
        a = np.ascontiguousarray(a)
    ld = a.strides[0] // 4 if a.shape[0] > 1 else a.shape[1]
    if ld < a.shape[1] or a.strides[0] % 4:
        a = np.ascontiguousarray(a)
        ld = a.shape[1]
    return a, ld


def exhaustive_match_cpu(sparse, dense, top_k, ratio=RATIO, scores=False, n_threads=0, precision="f32"):
    """fmpnp_exhaustive_match_cpu on numpy arrays (the CPU twin: the GPU's results bit for bit).
    precision="f16": the reference of the f16 precision (operands rounded to binary16, fp64 accumulation,
    one rounding to fp32), not a twin: the GPU's f16 scores lie within a bound of it, not on it."""
    prec = _lib.match_precision(precision)
    sparse, ld_s = _host_rows(sparse)
    dense, ld_d = _host_rows(dense)
    n, c = sparse.shape
    if dense.shape[0] != c:
        raise ValueError(f"sparse has {c} channels, dense {dense.shape[0]}")
    wh = dense.shape[1]
    argmax, top, kth = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    mask = np.zeros(n, np.uint8)
    out = np.zeros((n, wh), np.float32) if scores else None
    if prec == _lib.MATCH_F32:
        rc = _lib.load().fmpnp_exhaustive_match_cpu(
            sparse.ctypes.data, n, ld_s, dense.ctypes.data, c, wh, ld_d, int(top_k), float(ratio), argmax.ctypes.data,
            top.ctypes.data, kth.ctypes.data, mask.ctypes.data, out.ctypes.data if scores else None, int(n_threads))
    else:
        rc = _lib.load().fmpnp_exhaustive_match_ex_cpu(
            sparse.ctypes.data, n, ld_s, dense.ctypes.data, c, wh, ld_d, int(top_k), float(ratio), argmax.ctypes.data,
            top.ctypes.data, kth.ctypes.data, mask.ctypes.data, out.ctypes.data if scores else None, int(n_threads),
            prec)
    _lib.check(rc, "fmpnp_exhaustive_match_cpu")
    res = dict(argmax=argmax, top=top, kth=kth, mask=mask.astype(bool))
    if scores:
        res["scores"] = out
    return res


def _layer_args(layers, size, item, device_kind):
    """(fmpnp_hc_layer array, the tensors it points into, B, item, H, W, C) of a layered query."""
    from .hypercolumn import _plane_layers
    desc, keep = _plane_layers(layers, device_kind)
    batch, item = int(keep[0].shape[0]), int(item)
    if not 0 <= item < batch:
        raise ValueError(f"item {item} of a batch of {batch}")
    height, width = (int(s) for s in (keep[0].shape[2:] if size is None else size))
    return desc, keep, batch, item, height, width, sum(int(m.shape[1]) for m in keep)


def exhaustive_match_layers(sparse, layers, top_k, ratio=RATIO, size=None, item=0, normalize=True, scores=False):
    """fmpnp_exhaustive_match_layers on CUDA tensors: exhaustive_match(sparse, assemble_hypercolumn(layers, size,
    normalize)[item].view(C, -1), ...) without the dense map -- the correlation runs on each layer at the layer's
    own resolution and the small score maps are resized and summed (include/fmpnp.h, "layered matching": exact
    fp32, its own rounding order, so within a stated bound of the dense path and not on its bits).
    sparse [N, C] (rows may be padded), layers: 1 to 8 float32 CUDA tensors [B, C_l, H_l, W_l] with sum C_l = C
    (a layer whose planes are not contiguous is copied).  Returns exhaustive_match's dict; scores: [N, H * W].
    Waits on the current stream."""
    sparse, ld_s = _rows(sparse, "sparse")
    desc, keep, batch, item, height, width, c = _layer_args(layers, size, item, "cuda")
    n = sparse.shape[0]
    if sparse.shape[1] != c:
        raise ValueError(f"sparse has {sparse.shape[1]} channels, the layers {c}")
    if keep[0].device != sparse.device:
        raise ValueError("sparse and the layers must share one device")
    _lib.require_device(sparse.device)
    argmax, top, kth = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    mask = np.zeros(n, np.uint8)
    out = torch.empty((n, height * width), dtype=torch.float32, device=sparse.device) if scores else None
    with torch.cuda.device(sparse.device):
        rc = _lib.load().fmpnp_exhaustive_match_layers(
            _vp(sparse), n, ld_s, desc, len(keep), batch, item, height, width, _lib.HC_NORMALIZE if normalize else 0,
            int(top_k), float(ratio), argmax.ctypes.data, top.ctypes.data, kth.ctypes.data, mask.ctypes.data,
            _vp(out) if scores else None, _lib.stream_ptr(sparse.device))
    _lib.check(rc, "fmpnp_exhaustive_match_layers")
    res = dict(argmax=argmax, top=top, kth=kth, mask=mask.astype(bool))
    if scores:
        res["scores"] = out
    return res


def exhaustive_match_layers_cpu(sparse, layers, top_k, ratio=RATIO, size=None, item=0, normalize=True, scores=False,
                                n_threads=0):
    """fmpnp_exhaustive_match_layers_cpu (the CPU twin: exhaustive_match_layers' results bit for bit): sparse a
    float32 numpy array [N, C], layers float32 CPU tensors."""
    sparse, ld_s = _host_rows(sparse)
    desc, keep, batch, item, height, width, c = _layer_args(layers, size, item, "cpu")
    n = sparse.shape[0]
    if sparse.shape[1] != c:
        raise ValueError(f"sparse has {sparse.shape[1]} channels, the layers {c}")
    argmax, top, kth = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    mask = np.zeros(n, np.uint8)
    out = np.zeros((n, height * width), np.float32) if scores else None
    rc = _lib.load().fmpnp_exhaustive_match_layers_cpu(
        sparse.ctypes.data, n, ld_s, desc, len(keep), batch, item, height, width, _lib.HC_NORMALIZE if normalize else 0,
        int(top_k), float(ratio), argmax.ctypes.data, top.ctypes.data, kth.ctypes.data, mask.ctypes.data,
        out.ctypes.data if scores else None, int(n_threads))
    _lib.check(rc, "fmpnp_exhaustive_match_layers_cpu")
    res = dict(argmax=argmax, top=top, kth=kth, mask=mask.astype(bool))
    if scores:
        res["scores"] = out
    return res


def _factor(factor):
    if factor is None:
        factor = config.exhaustive_search_kwargs()["factor"]
    if factor is None:
        raise TypeError("exhaustive_search: factor is not bound (pass it, or "
                        "fmpnp.config.configure(exhaustive_search_factor=...))")
    return factor


def _top_k(factor, width, height):
    top_k = int(factor * width * height)  # exhaustive_search.py:13
    if top_k < 1 or top_k > width * height:
        raise IndexError(f"exhaustive_search: top_k = int(factor * W * H) = {top_k} is outside 1..{width * height}")
    return top_k


def points_in_query_space(argmax, image_shape, width, height):
    """exhaustive_search.py:18-19,51-54: the argmax cell's centre in image space, formed in fp32."""
    idx = np.asarray(argmax).astype(np.int64)
    indices = torch.from_numpy(np.stack([idx % height, idx // height], axis=1).astype(np.float32))  # (a_x, a_y)
    query_cell_sizes = torch.FloatTensor(list(image_shape)) / torch.FloatTensor([width, height])
    return (indices * query_cell_sizes) + (query_cell_sizes / 2)


def _device_f32(t, device=None):
    t = torch.as_tensor(t)
    if not t.is_cuda:
        t = t.to(device or "cuda")
    return t.float()


def exhaustive_search(dense_descriptor_map, sparse_descriptor_map, image_shape, map_size, cell_size, factor=None,
                      precision="f32"):
    """exhaustive_search (exhaustive_search.py:24-55): dense [C, W*H], sparse [N, C] ->
    (argmax_in_query_space, a CPU FloatTensor [N, 2]; mask, a numpy bool array [N]).
    factor=None reads fmpnp.config (configure(exhaustive_search_factor=...)).  precision: as exhaustive_match's."""
    (points, mask), = exhaustive_search_multi(dense_descriptor_map, [sparse_descriptor_map], image_shape, map_size,
                                              cell_size, factor, precision)
    return points, mask


def exhaustive_search_multi(dense_descriptor_map, sparse_descriptor_maps, image_shape, map_size, cell_size,
                            factor=None, precision="f32"):
    """The top_N reference images of one query (sparse_to_dense_predictor.py:140-191) in one call:
    the rows are independent and the dense operand is shared, so the sparse maps are concatenated,
    matched in one launch sequence and the results split.  Returns [(points, mask), ...], each equal
    to exhaustive_search's on that reference bit for bit (under either precision; with "f16" the dense map is
    converted once for all the references)."""
    _lib.match_precision(precision)
    width, height = list(map(int, map_size))
    top_k = _top_k(_factor(factor), width, height)
    dense = _device_f32(dense_descriptor_map)
    if dense.dim() != 2 or dense.shape[1] != width * height:
        raise ValueError(f"dense_descriptor_map must be [C, {width * height}]")
    sparse = [_device_f32(s, dense.device) for s in sparse_descriptor_maps]
    counts = [int(s.shape[0]) for s in sparse]
    rows = sparse[0] if len(sparse) == 1 else torch.cat(sparse, dim=0)
    res = exhaustive_match(rows, dense, top_k, RATIO, precision=precision)
    out, at = [], 0
    for n in counts:
        out.append((points_in_query_space(res["argmax"][at:at + n], image_shape, width, height),
                    res["mask"][at:at + n].copy()))
        at += n
    return out


def exhaustive_search_layers(query_layers, sparse_descriptor_map, image_shape, cell_size, factor=None, item=0):
    """exhaustive_search with the query given as its encoder layers (a list of float32 CUDA tensors
    [B, C_l, H_l, W_l]; item: the query's batch item): what exhaustive_search returns on
    assemble_hypercolumn(query_layers)[item].view(C, -1), formed by layered matching without that map.
    map_size is read off the layers: the assembled map's two trailing dimensions."""
    (points, mask), = exhaustive_search_layers_multi(query_layers, [sparse_descriptor_map], image_shape, cell_size,
                                                     factor, item)
    return points, mask


def exhaustive_search_layers_multi(query_layers, sparse_descriptor_maps, image_shape, cell_size, factor=None, item=0):
    """exhaustive_search_multi with a layered query: the references' rows concatenated and matched in one call (the
    query's norm plane is formed once), the results split.  Each (points, mask) equals exhaustive_search_layers' on
    that reference bit for bit."""
    query_layers = list(query_layers)
    width, height = (int(s) for s in query_layers[0].shape[2:])  # (exhaustive_search's names: map_size = shape[1:])
    top_k = _top_k(_factor(factor), width, height)
    sparse = [_device_f32(s, query_layers[0].device) for s in sparse_descriptor_maps]
    counts = [int(s.shape[0]) for s in sparse]
    rows = sparse[0] if len(sparse) == 1 else torch.cat(sparse, dim=0)
    res = exhaustive_match_layers(rows, query_layers, top_k, RATIO, item=item)
    out, at = [], 0
    for n in counts:
        out.append((points_in_query_space(res["argmax"][at:at + n], image_shape, width, height),
                    res["mask"][at:at + n].copy()))
        at += n
    return out


def generate_dense_keypoints(feature_map_resolution, image_resolution, to_numpy=True):
    """generate_dense_keypoints (keypoint_association.py:7-38) in plain numpy: the cell centres of the
    regular grid as [M, 2] (the first resolution axis is the slow one, and each row is (centre along
    axis 1, centre along axis 0)), and (cell_size_x, cell_size_y).  to_numpy=False needs cv2."""
    cell_size_x = image_resolution[0] / feature_map_resolution[0]
    cell_size_y = image_resolution[1] / feature_map_resolution[1]
    arange_x = np.arange(0, image_resolution[0], cell_size_x) + cell_size_x / 2
    arange_y = np.arange(0, image_resolution[1], cell_size_y) + cell_size_y / 2
    jj, ii = np.meshgrid(arange_y, arange_x)  # ii: the slow axis (x), jj: the fast axis (y)
    keypoints = np.stack([jj.reshape(-1), ii.reshape(-1)], axis=1).astype(np.float64)
    if not to_numpy:
        import cv2
        cell_size = (cell_size_x + cell_size_y) / 2
        keypoints = [cv2.KeyPoint(float(j), float(i), cell_size) for j, i in keypoints]
    return keypoints, (cell_size_x, cell_size_y)


def nearest_cells(points, d1, d2, cell0, cell1):
    """The flat cell fmpnp_gather_sparse_descriptors picks for each point ([N, 2] fp64), in numpy: per
    axis clip(ceil(p / cell - 1), 0, n - 1); coordinate 0 runs along the map's last dimension (d2,
    cell1), coordinate 1 along the first (d1, cell0); a point exactly between two centres takes the
    lower cell, as fast_closest_points' argmin does (keypoint_association.py:77-86)."""
    p = np.asarray(points, np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        i0 = np.nan_to_num(np.ceil(p[:, 0] / cell1 - 1.0), nan=0.0, posinf=d2 - 1, neginf=0.0)
        i1 = np.nan_to_num(np.ceil(p[:, 1] / cell0 - 1.0), nan=0.0, posinf=d1 - 1, neginf=0.0)
    i0 = np.clip(i0, 0, d2 - 1).astype(np.int64)
    i1 = np.clip(i1, 0, d1 - 1).astype(np.int64)
    return i1 * d2 + i0


def gather_sparse_descriptors(dense_chw, points2d, cell0, cell1, out=None):
    """fmpnp_gather_sparse_descriptors: dense_chw [C, D1, D2] (fp32 CUDA), points2d [N, 2] ->
    [N, C] fp32 CUDA tensor of each point's nearest cell's descriptor.  Asynchronous on the current
    stream."""
    if dense_chw.dim() != 3 or dense_chw.dtype != torch.float32 or not dense_chw.is_cuda:
        raise ValueError("dense_chw must be a float32 CUDA tensor [C, D1, D2]")
    dense_chw = dense_chw.contiguous()
    c, d1, d2 = dense_chw.shape
    pts = torch.as_tensor(points2d).to(device=dense_chw.device, dtype=torch.float64).reshape(-1, 2).contiguous()
    n = pts.shape[0]
    if out is None:
        out = torch.empty((n, c), dtype=torch.float32, device=dense_chw.device)
    _lib.require_device(dense_chw.device)
    with torch.cuda.device(dense_chw.device):
        rc = _lib.load().fmpnp_gather_sparse_descriptors(_vp(dense_chw), c, d1, d2, _vp(pts), n, float(cell0),
                                                         float(cell1), _vp(out), out.stride(0) if n > 1 else c,
                                                         _lib.stream_ptr(dense_chw.device))
    _lib.check(rc, "fmpnp_gather_sparse_descriptors")
    return out


def fast_sparse_keypoint_descriptor(keypoints, dense_keypoints, dense_descriptors):
    """fast_sparse_keypoint_descriptor (keypoint_association.py:40-75): keypoints, a list of B arrays
    [>= 2, N_i] (rows 0 and 1 are the coordinates); dense_keypoints [M, 2], the grid of
    generate_dense_keypoints; dense_descriptors [B, C, W, H].  Returns the list of B tensors
    [N_i, C] on the descriptors' device.  The grid's cell sizes are read off its first centre
    (cell / 2 per axis); the [M x N] distance matrix is never formed."""
    dense_descriptors = _device_f32(dense_descriptors)
    batch, channels, width, height = dense_descriptors.shape
    grid = np.asarray(dense_keypoints.cpu() if torch.is_tensor(dense_keypoints) else dense_keypoints, np.float64)
    if grid.shape != (width * height, 2):
        raise ValueError(f"dense_keypoints must be [{width * height}, 2]")
    cell1, cell0 = 2.0 * grid[0, 0], 2.0 * grid[0, 1]  # coordinate 0 runs along the last dimension
    out = []
    for i, kp in enumerate(keypoints):
        pts = np.ascontiguousarray(np.asarray(kp, np.float64)[:2, :].T)
        out.append(gather_sparse_descriptors(dense_descriptors[i], pts, cell0, cell1))
    return out
