"""The localisation chain of one query on the GPU: match every retrieved reference, solve PnP for each,
pick the best prediction and refine it (SparseToDensePredictor.run,
s2dhm/pose_prediction/sparse_to_dense_predictor.py:114-259, with _choose_best_prediction and
_nearest_neighbor_prediction, predictor.py:48-73).

Between the stages nothing passes through the host: the match stage's argmax / mask stay on the device, a
glue kernel compacts the rows that passed the ratio test into the PnP stage's problems, the PnP stage reads
its sizes from those device descriptors, and a second glue kernel picks the best pair and assembles the
refiner's inputs (include/fmpnp.h, "localisation chain").  localize / localize_multi call the synchronous
fmpnp_localize: one upload, one pinned download and one host wait end the chain; the refinement
(fmpnp.feature_pnp) costs the second wait.

    localize(query_hypercolumn, references, image_shape, ...)   one query
    localize_multi(queries, ...)                                 B queries, one PnP launch over all pairs
    localize_cpu(...)                                            the same chain through the CPU twins, up to
                                                                 the best prediction (never a fallback)
    LocalizeLaunch                                               the asynchronous form (fmpnp_localize_async on
                                                                 device tensors): queue, then read()

A reference is a mapping with points_2D [n, 2], points_3D [n, 3], intrinsics, distortion_coefficients,
image_resolution, filename, and hypercolumn (the dense map [C, W, H] on the device) and / or
sparse_descriptors ([n, C], precomputed); optionally fallback_pose = (quaternion, matrix), the
reference's own pose (_nearest_neighbor_prediction).  The refinement reads the best reference's hypercolumn.
Instead of hypercolumn a reference may carry feature_maps, the encoder's layers of the reference image (a list
of float32 CUDA tensors [B, C_l, H_l, W_l], with feature_item naming its item when the maps are one batched
encoder pass over several references; default 0): its rows are then formed straight from the layers
(fmpnp.sparse_hypercolumn(at="cell") at points_2D -- all the references of a call that share one batched pass
in one launch) and handed on as sparse_descriptors are, and the refinement takes the layers too
(feature_pnp(reference_layers=...)), so the reference's dense map is never assembled.  The results are the
same bits.

One quirk of the reference is kept: the K handed to the refinement is the intrinsics of the LAST reference
of the loop (sparse_to_dense_predictor.py:143,167,244), not the best one's; refine_intrinsics="best" uses
the best one's.
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .match import RATIO, _factor, _top_k, nearest_cells
from .matrix_utils import matrix_quaternion
from .pnp import Prediction, _bound, _distortion, _no_prediction

Localization = namedtuple("Localization", "export prediction refined kind best predictions cached_matches")
Localization.__doc__ = """export: [*quaternion, *t] of the best prediction before refinement (predictor.py:52-54), or None;
prediction: the best Prediction, or None when no reference was eligible; refined: (t, quaternion, model) as
optimize_feature_pnp returns them, or None; kind: "solved" / "fallback" / "none"; best: the best reference's
index; predictions / cached_matches: with return_all, every reference's Prediction and its dict in the
cached_matches layout (sparse_to_dense_predictor.py:193-204), else None."""

KINDS = {_lib.LOC_NONE: "none", _lib.LOC_SOLVED: "solved", _lib.LOC_FALLBACK: "fallback"}


def _up(x, a=256):
    return (x + a - 1) // a * a


def _ref_get(ref, name, default=None):
    if isinstance(ref, dict):
        return ref.get(name, default)
    return getattr(ref, name, default)


class _RowsRef:
    """A reference whose sparse rows were formed from its feature_maps: sparse_descriptors, and every other
    field read through to the reference."""

    def __init__(self, ref, rows):
        self._ref, self.sparse_descriptors = ref, rows

    def __getattr__(self, name):  # (only for what the instance itself lacks)
        if name.startswith("__"):
            raise AttributeError(name)
        return _ref_get(self._ref, name)


def _layers_of(ref):
    """The reference's own layers [1, C_l, H_l, W_l] (its item of a batched pass), or None."""
    maps = _ref_get(ref, "feature_maps")
    if maps is None:
        return None
    item = int(_ref_get(ref, "feature_item") or 0)
    return [m[item:item + 1] for m in maps]


def _rows_from_layers(queries):
    """queries with every reference that carries feature_maps (and neither sparse_descriptors nor hypercolumn)
    replaced by one carrying the rows sparse_hypercolumn(at="cell") forms at its points_2D.  The references
    that share one set of maps (one batched encoder pass, told apart by feature_item) go in one launch."""
    from .hypercolumn import sparse_hypercolumn
    groups, order = {}, []
    for qi, (_, refs) in enumerate(queries):
        for ri, ref in enumerate(refs):
            maps = _ref_get(ref, "feature_maps")
            if (maps is None or _ref_get(ref, "sparse_descriptors") is not None
                    or _ref_get(ref, "hypercolumn") is not None):
                continue
            maps = list(maps)
            res = _ref_get(ref, "image_resolution")
            height, width = int(maps[0].shape[2]), int(maps[0].shape[3])
            cell = (float(res[0] / height), float(res[1] / width))
            key = (tuple((m.data_ptr(), tuple(m.shape), tuple(m.stride())) for m in maps), cell)
            if key not in groups:
                groups[key] = (maps, cell, [])
                order.append(key)
            groups[key][2].append((qi, ri, ref))
    if not order:
        return queries
    queries = [(q, list(refs)) for q, refs in queries]
    for key in order:
        maps, cell, members = groups[key]
        pts = [np.asarray(_ref_get(ref, "points_2D"), np.float64).reshape(-1, 2) for _, _, ref in members]
        item = np.concatenate([np.full(len(p), int(_ref_get(ref, "feature_item") or 0), np.int32)
                               for p, (_, _, ref) in zip(pts, members)])
        rows = sparse_hypercolumn(maps, np.concatenate(pts), at="cell", cell_size=cell, item=item)
        at = 0
        for p, (qi, ri, ref) in zip(pts, members):
            queries[qi][1][ri] = _RowsRef(ref, rows[at:at + len(p)])
            at += len(p)
    return queries


def _pnp_params(reprojection_threshold, minimum_matches, minimum_inliers, return_masked, iters, seed):
    p = _lib.LocParams()
    p.threshold = float(_bound("reprojection_threshold", reprojection_threshold))
    p.minimum_matches = int(_bound("minimum_matches", minimum_matches))
    p.minimum_inliers = int(_bound("minimum_inliers", minimum_inliers))
    p.return_masked = 1 if _bound("return_masked", return_masked) else 0
    p.iters, p.seed = int(_bound("iters", iters)), int(_bound("seed", seed))
    return p


class _Plan:
    """The descriptors of B queries' pairs in host memory, and the layout of every buffer of the chain.
    queries: [(query map [C, W, H], references)]."""

    def __init__(self, queries, image_shape, factor, params):
        self.params = params
        self.queries = queries
        self.image_shape = image_shape
        self.n_queries = len(queries)
        self.refs = [list(refs) for _, refs in queries]
        self.n_pairs = sum(len(r) for r in self.refs)
        if self.n_pairs > 65535:
            _lib.check(_lib.ETOOBIG, "fmpnp.localize: more than 65535 (query, reference) pairs")
        self.pairs = (_lib.LocPair * max(self.n_pairs, 1))()
        self.qdesc = (_lib.LocQuery * max(self.n_queries, 1))()
        self.dims, self.top_k = [], []
        self.p3, self.p2 = [], []  # per pair: points_3D [n, 3], points_2D [n, 2] (fp64, contiguous)
        factor = _factor(factor)
        rows, out, g = 0, 0, 0
        for qi, (qmap, refs) in enumerate(queries):
            if qmap.dim() == 4:
                qmap = qmap[0]
            c, width, height = qmap.shape
            self.dims.append((int(c), int(width), int(height)))
            self.top_k.append(_top_k(factor, width, height))
            q = self.qdesc[qi]
            q.pair_begin, q.pair_count, q.out_offset, cap = g, len(self.refs[qi]), out, 0
            for ref in self.refs[qi]:
                x3 = np.ascontiguousarray(np.asarray(_ref_get(ref, "points_3D"), np.float64).reshape(-1, 3))
                x2 = np.ascontiguousarray(np.asarray(_ref_get(ref, "points_2D"), np.float64).reshape(-1, 2))
                if x3.shape[0] != x2.shape[0]:
                    raise ValueError(f"{x3.shape[0]} 3D points for {x2.shape[0]} 2D points")
                K = np.asarray(_ref_get(ref, "intrinsics"), np.float64)
                if K.shape != (3, 3):
                    raise ValueError("intrinsics must be 3x3")
                p = self.pairs[g]
                p.K[:] = K.reshape(-1).tolist()
                p.dist[:] = _distortion(_ref_get(ref, "distortion_coefficients")).tolist()
                fb = _ref_get(ref, "fallback_pose")
                p.has_fallback = 0 if fb is None else 1
                if fb is not None:
                    m = np.asarray(fb[1], np.float64)
                    p.fallback_R[:] = m[:3, :3].reshape(-1).tolist()
                    p.fallback_t[:] = m[:3, 3].tolist()
                p.row_offset, p.n_rows = rows, x3.shape[0]
                p.image_shape[:] = [float(np.float32(image_shape[0])), float(np.float32(image_shape[1]))]
                p.dim[:] = [int(width), int(height)]
                self.p3.append(x3)
                self.p2.append(x2)
                rows += x3.shape[0]
                cap = max(cap, x3.shape[0])
                g += 1
            q.out_cap = cap
            out += cap
        self.total_rows, self.out_rows = rows, out

    def sections(self, return_all):
        """(name, dtype, elements) of the output buffers in download order: the records and the best pairs'
        arrays, then (return_all) every pair's; the rest stays on the device."""
        T, O, P = max(self.total_rows, 1), max(self.out_rows, 1), max(self.n_pairs, 1)
        head = [("records", np.uint8, max(self.n_queries, 1) * ctypes.sizeof(_lib.LocRecord)),
                ("b_pts3d", np.float64, 3 * O), ("b_ref2d", np.float64, 2 * O), ("b_q32", np.float32, 2 * O),
                ("b_idx", np.int32, O)]
        every = [("counts", np.int32, P), ("results", np.uint8, P * ctypes.sizeof(_lib.PnpResult)),
                 ("pnp_mask", np.uint8, T), ("m_q32", np.float32, 2 * T), ("m_x3", np.float64, 3 * T),
                 ("m_r2", np.float64, 2 * T), ("m_src", np.int32, T)]
        tail = [("m_q64", np.float64, 2 * T)]
        return head, every, tail


def _layout(sections):
    """{name: (byte offset, dtype, elements)} and the total size, every section 256-byte aligned."""
    at, out = 0, {}
    for name, dtype, n in sections:
        out[name] = (at, dtype, n)
        at += _up(n * np.dtype(dtype).itemsize)
    return out, at


def _views(buf, lay):
    """numpy views of a host byte array's sections."""
    return {k: buf[o:o + n * np.dtype(d).itemsize].view(d) for k, (o, d, n) in lay.items()}


def _pinned(nbytes):
    """A pinned host byte tensor (torch's caching host allocator: reused once the copies that use it are done)."""
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, pin_memory=True)


def _dense_map(ref, device):
    hc = _ref_get(ref, "hypercolumn")
    if hc is None:
        return None
    hc = hc[0] if hc.dim() == 4 else hc
    if not hc.is_cuda or hc.dtype != torch.float32:
        hc = hc.to(device=device, dtype=torch.float32)
    return hc.contiguous()


class LocalizeLaunch:
    """The asynchronous form: queues the sparse-descriptor gathers, the match launches of every query,
    fmpnp_localize_async (build, one PnP launch over all the pairs, pick) and the one pinned download on
    the current stream of the queries' device, and returns without waiting.  read() waits once and parses.
    fill: the byte every output buffer (results, masks, compacted arrays, records) holds before the
    launches; no output depends on it.  match_precision: the match stage's ("f32", the exact default, or "f16")."""

    def __init__(self, queries, image_shape, factor, params, return_all=False, fill=0, match_precision="f32"):
        prec = _lib.match_precision(match_precision)
        queries = _rows_from_layers([(q, list(refs)) for q, refs in queries])
        self.plan = plan = _Plan(queries, image_shape, factor, params)
        self.return_all = bool(return_all)
        L = _lib.load()
        qmaps = []
        for qmap, _ in queries:
            qmap = qmap[0] if qmap.dim() == 4 else qmap
            if not qmap.is_cuda or qmap.dtype != torch.float32:
                raise ValueError("query_hypercolumn must be a float32 CUDA tensor [C, W, H]")
            qmaps.append(qmap.contiguous())
        self.device = dev = qmaps[0].device if qmaps else torch.device("cuda", torch.cuda.current_device())
        _lib.require_device(dev)
        self.stream = stream = torch.cuda.current_stream(dev)
        T, P, Q = plan.total_rows, plan.n_pairs, plan.n_queries
        # one upload: the pair and query descriptors, then every pair's points
        b_pairs, b_q = _up(ctypes.sizeof(plan.pairs)), _up(ctypes.sizeof(plan.qdesc))
        o_p3 = b_pairs + b_q
        o_p2 = o_p3 + _up(24 * max(T, 1))
        n_up = o_p2 + _up(16 * max(T, 1))
        head, every, tail = plan.sections(self.return_all)
        self.lay, n_out = _layout(head + every + tail)
        self.n_down = _layout(head + (every if self.return_all else []))[1]
        with torch.cuda.device(dev):
            self.up_dev = torch.empty(n_up, dtype=torch.uint8, device=dev)
            self.out_dev = torch.full((n_out,), int(fill), dtype=torch.uint8, device=dev)
            self.sel_dev = torch.full((_up(4 * max(T, 1)) * 3 + _up(max(T, 1)),), int(fill), dtype=torch.uint8, device=dev)
            ws_loc = max(int(L.fmpnp_localize_workspace_size(P)), 8)
            self.ws_loc = torch.empty(ws_loc // 8 + 1, dtype=torch.int64, device=dev)
            base_up, base_out, base_sel = self.up_dev.data_ptr(), self.out_dev.data_ptr(), self.sel_dev.data_ptr()
            dev_pairs = (_lib.LocPair * max(P, 1)).from_buffer_copy(plan.pairs)
            host = _pinned(n_up)
            hb = host.numpy()
            for g in range(P):
                off, n = plan.pairs[g].row_offset, plan.pairs[g].n_rows
                dev_pairs[g].points3d = base_up + o_p3 + 24 * off
                dev_pairs[g].points2d = base_up + o_p2 + 16 * off
                hb[o_p3 + 24 * off:o_p3 + 24 * (off + n)] = plan.p3[g].reshape(-1).view(np.uint8)
                hb[o_p2 + 16 * off:o_p2 + 16 * (off + n)] = plan.p2[g].reshape(-1).view(np.uint8)
            hb[:ctypes.sizeof(dev_pairs)] = np.frombuffer(dev_pairs, np.uint8)
            hb[b_pairs:b_pairs + ctypes.sizeof(plan.qdesc)] = np.frombuffer(plan.qdesc, np.uint8)
            self.host_pairs = dev_pairs  # (the host descriptors: validation and sizes; its point pointers are not read)
            self.up_dev.copy_(host[:n_up], non_blocking=True)
            sp = _lib.stream_ptr(dev)
            # the sparse descriptors of every pair, gathered (or copied) straight into the concatenated rows
            o_arg, o_top, o_kth, o_mask = 0, _up(4 * max(T, 1)), 2 * _up(4 * max(T, 1)), 3 * _up(4 * max(T, 1))
            g = 0
            self.keep = []
            for qi, qmap in enumerate(qmaps):
                c, width, height = plan.dims[qi]
                n_q = sum(plan.pairs[g + j].n_rows for j in range(len(plan.refs[qi])))
                rows = torch.empty((max(n_q, 1), c), dtype=torch.float32, device=dev)
                at, row0 = 0, plan.pairs[g].row_offset if plan.refs[qi] else 0
                for ref in plan.refs[qi]:
                    n = plan.pairs[g].n_rows
                    sparse = _ref_get(ref, "sparse_descriptors")
                    if sparse is not None:
                        sparse = torch.as_tensor(sparse)
                        if tuple(sparse.shape) != (n, c):
                            raise ValueError(f"sparse_descriptors must be [{n}, {c}]")
                        rows[at:at + n].copy_(sparse.to(device=dev, dtype=torch.float32), non_blocking=True)
                    elif n:
                        hc = _dense_map(ref, dev)
                        if hc is None:
                            raise ValueError("a reference needs hypercolumn or sparse_descriptors")
                        if hc.shape[0] != c:
                            raise ValueError(f"the reference map has {hc.shape[0]} channels, the query {c}")
                        res = _ref_get(ref, "image_resolution")
                        self.keep.append(hc)
                        rc = L.fmpnp_gather_sparse_descriptors(
                            hc.data_ptr(), c, hc.shape[1], hc.shape[2], dev_pairs[g].points2d, n,
                            float(res[0] / hc.shape[1]), float(res[1] / hc.shape[2]),
                            rows.data_ptr() + 4 * c * at, c, sp)
                        _lib.check(rc, "fmpnp_gather_sparse_descriptors")
                    at += n
                    g += 1
                if n_q:
                    wh = width * height
                    if prec == _lib.MATCH_F32:
                        ws_bytes = int(L.fmpnp_match_workspace_size(n_q, wh))
                    else:
                        ws_bytes = int(L.fmpnp_match_workspace_size_ex(n_q, c, wh, prec))
                    ws = torch.empty(max(ws_bytes, 8) // 4 + 1, dtype=torch.float32, device=dev)
                    self.keep += [rows, ws]
                    if prec == _lib.MATCH_F32:
                        rc = L.fmpnp_exhaustive_match_async(
                            rows.data_ptr(), n_q, c, qmap.data_ptr(), c, wh, wh, plan.top_k[qi], float(RATIO),
                            base_sel + o_arg + 4 * row0, base_sel + o_top + 4 * row0, base_sel + o_kth + 4 * row0,
                            base_sel + o_mask + row0, None, ws.data_ptr(), ws.numel() * 4, sp)
                    else:
                        rc = L.fmpnp_exhaustive_match_ex_async(
                            rows.data_ptr(), n_q, c, qmap.data_ptr(), c, wh, wh, plan.top_k[qi], float(RATIO),
                            base_sel + o_arg + 4 * row0, base_sel + o_top + 4 * row0, base_sel + o_kth + 4 * row0,
                            base_sel + o_mask + row0, None, ws.data_ptr(), ws.numel() * 4, prec, sp)
                    _lib.check(rc, "fmpnp_exhaustive_match_async")
            lay = self.lay
            m = _lib.LocMatches(base_out + lay["m_q32"][0], base_out + lay["m_q64"][0], base_out + lay["m_x3"][0],
                                base_out + lay["m_r2"][0], base_out + lay["m_src"][0], base_out + lay["counts"][0])
            b = _lib.LocBest(base_out + lay["b_pts3d"][0], base_out + lay["b_ref2d"][0], base_out + lay["b_q32"][0],
                             base_out + lay["b_idx"][0], base_out + lay["records"][0])
            rc = L.fmpnp_localize_async(
                base_up, dev_pairs, P, base_up + b_pairs, plan.qdesc, Q, ctypes.byref(plan.params), base_sel + o_arg,
                base_sel + o_mask, T, ctypes.byref(m), ctypes.byref(b), base_out + lay["results"][0],
                base_out + lay["pnp_mask"][0], self.ws_loc.data_ptr(), ws_loc, sp)
            _lib.check(rc, "fmpnp_localize_async")
            self.down = _pinned(self.n_down)
            self.down[:self.n_down].copy_(self.out_dev[:self.n_down], non_blocking=True)

    def read(self):
        """Wait for the stream (the chain's one host wait) and return one Localization per query, unrefined."""
        self.stream.synchronize()
        host = self.down[:self.n_down].numpy().copy()
        head, every, _ = self.plan.sections(self.return_all)
        lay, _ = _layout(head + (every if self.return_all else []))
        return _parse(self.plan, _views(host, lay), self.return_all)


def _run_sync(queries, image_shape, factor, params, return_all, fill=0, match_precision="f32"):
    """fmpnp_localize: the chain in one call with one upload, one pinned download and one host wait on the
    current stream of the queries' device.  Returns one (unrefined) Localization per query.  fill: the byte
    the host arrays hold before the call; no output depends on it.  match_precision "f16": fmpnp_localize_ex."""
    prec = _lib.match_precision(match_precision)
    plan = _Plan(queries, image_shape, factor, params)
    L = _lib.load()
    qmaps = []
    for qmap, _ in queries:
        qmap = qmap[0] if qmap.dim() == 4 else qmap
        if not qmap.is_cuda or qmap.dtype != torch.float32:
            raise ValueError("query_hypercolumn must be a float32 CUDA tensor [C, W, H]")
        qmaps.append(qmap.contiguous())
    dev = qmaps[0].device if qmaps else torch.device("cuda", torch.cuda.current_device())
    _lib.require_device(dev)
    P, Q = plan.n_pairs, plan.n_queries
    c = plan.dims[0][0] if Q else 1
    if any(d[0] != c for d in plan.dims):
        raise ValueError("the queries' maps must have the same number of channels")
    sources, keep, g = (_lib.LocSource * max(P, 1))(), [], 0
    for qi in range(Q):
        for ref in plan.refs[qi]:
            n = plan.pairs[g].n_rows
            plan.pairs[g].points3d, plan.pairs[g].points2d = plan.p3[g].ctypes.data or None, plan.p2[g].ctypes.data or None
            sparse = _ref_get(ref, "sparse_descriptors")
            if sparse is not None:
                sparse = torch.as_tensor(sparse)
                if tuple(sparse.shape) != (n, c):
                    raise ValueError(f"sparse_descriptors must be [{n}, {c}]")
                sparse = sparse.to(device=dev, dtype=torch.float32).contiguous()
                keep.append(sparse)
                sources[g].sparse, sources[g].ld_sparse = sparse.data_ptr() or None, c
            elif n:
                hc = _dense_map(ref, dev)
                if hc is None:
                    raise ValueError("a reference needs hypercolumn or sparse_descriptors")
                if hc.shape[0] != c:
                    raise ValueError(f"the reference map has {hc.shape[0]} channels, the query {c}")
                res = _ref_get(ref, "image_resolution")
                keep.append(hc)
                s = sources[g]
                s.dense_chw, s.D1, s.D2 = hc.data_ptr(), hc.shape[1], hc.shape[2]
                s.cell0, s.cell1 = float(res[0] / hc.shape[1]), float(res[1] / hc.shape[2])
            g += 1
    head, every, tail = plan.sections(True)
    lay, n_out = _layout(head + every + tail)
    bufs = _views(np.full(n_out, int(fill), np.uint8), lay)
    m = _lib.LocMatches(*[bufs[k].ctypes.data for k in ("m_q32", "m_q64", "m_x3", "m_r2", "m_src", "counts")])
    b = _lib.LocBest(*[bufs[k].ctypes.data for k in ("b_pts3d", "b_ref2d", "b_q32", "b_idx", "records")])
    dense = (ctypes.c_void_p * max(Q, 1))(*[q.data_ptr() for q in qmaps])
    top_k = (ctypes.c_int * max(Q, 1))(*plan.top_k)
    with torch.cuda.device(dev):
        args = (plan.pairs, sources, P, plan.qdesc, dense, top_k, Q, c, float(RATIO), ctypes.byref(plan.params),
                plan.total_rows, ctypes.byref(b), ctypes.byref(m) if return_all else None,
                bufs["results"].ctypes.data if return_all else None,
                bufs["pnp_mask"].ctypes.data if return_all else None)
        if prec == _lib.MATCH_F32:
            rc = L.fmpnp_localize(*args, _lib.stream_ptr(dev))
        else:
            rc = L.fmpnp_localize_ex(*args, prec, _lib.stream_ptr(dev))
    _lib.check(rc, "fmpnp_localize")
    return _parse(plan, bufs, bool(return_all))


def _matrix(R, t):
    matrix = np.eye(4)  # matrix_from_se3 (matrix_utils.py:76-81)
    matrix[:3, 3] = t
    matrix[:3, :3] = np.asarray(R).reshape(3, 3)
    return matrix


def _fallback(ref, num_matches, ref2d, q32, x3):
    """sparse_to_dense_predictor.py:179-189 on _nearest_neighbor_prediction (predictor.py:56-73)."""
    quaternion, matrix = _ref_get(ref, "fallback_pose")
    return Prediction(success=True, num_matches=num_matches, num_inliers=0, reference_inliers=ref2d,
                      query_inliers=np.squeeze(q32.reshape(-1, 1, 2)), points_3d=x3.reshape(-1, 1, 3),
                      quaternion=quaternion, matrix=matrix, reference_filename=_ref_get(ref, "filename"),
                      reference_keypoints=None, inlier_mask=None)


def _parse(plan, v, return_all):
    """The downloaded sections -> one (unrefined) Localization per query."""
    prm = plan.params
    recs = (_lib.LocRecord * max(plan.n_queries, 1)).from_buffer_copy(v["records"].tobytes())
    res = (_lib.PnpResult * max(plan.n_pairs, 1)).from_buffer_copy(v["results"].tobytes()) if return_all else None
    out = []
    for qi in range(plan.n_queries):
        rec, q, refs = recs[qi], plan.qdesc[qi], plan.refs[qi]
        o, n = q.out_offset, rec.N
        ref2d, q32 = v["b_ref2d"].reshape(-1, 2)[o:o + n].copy(), v["b_q32"].reshape(-1, 2)[o:o + n].copy()
        x3 = v["b_pts3d"].reshape(-1, 3)[o:o + n].copy()
        kind = KINDS[rec.kind]
        if kind == "none":
            best = None
        elif kind == "fallback":
            best = _fallback(refs[rec.best], rec.num_matches, ref2d, q32, x3)
        else:
            matrix = _matrix(rec.R0[:], rec.t0[:])
            best = Prediction(success=True, num_matches=rec.num_matches, num_inliers=rec.num_inliers,
                              reference_inliers=ref2d, query_inliers=np.squeeze(q32.reshape(-1, 1, 2)),
                              points_3d=x3.reshape(-1, 1, 3), quaternion=matrix_quaternion(matrix), matrix=matrix,
                              reference_filename=_ref_get(refs[rec.best], "filename"), reference_keypoints=None,
                              inlier_mask=v["b_idx"][o:o + rec.num_inliers].copy())
        export = None if best is None else [*best.quaternion, *list(np.asarray(best.matrix)[:3, 3])]
        preds = cached = None
        if return_all:
            preds, cached = [], []
            for j, ref in enumerate(refs):
                g = q.pair_begin + j
                off, cnt = plan.pairs[g].row_offset, int(v["counts"][g])
                m_q = v["m_q32"].reshape(-1, 2)[off:off + cnt].copy()
                m_r = v["m_r2"].reshape(-1, 2)[off:off + cnt].copy()
                m_x = v["m_x3"].reshape(-1, 3)[off:off + cnt].copy()
                r = res[g]
                if r.status == _lib.PNP_OK and r.num_inliers >= prm.minimum_inliers:
                    inl = np.flatnonzero(v["pnp_mask"][off:off + cnt]).astype(np.int32)
                    matrix = _matrix(r.R[:], r.t[:])
                    sel = inl if prm.return_masked else slice(None)
                    pred = Prediction(success=True, num_matches=cnt, num_inliers=len(inl), reference_inliers=m_r[sel],
                                      query_inliers=np.squeeze(m_q.reshape(-1, 1, 2)[sel]),
                                      points_3d=m_x.reshape(-1, 1, 3)[sel], quaternion=matrix_quaternion(matrix),
                                      matrix=matrix, reference_filename=_ref_get(ref, "filename"),
                                      reference_keypoints=None, inlier_mask=inl)
                elif _ref_get(ref, "fallback_pose") is not None:
                    pred = _fallback(ref, cnt, m_r, m_q, m_x)
                else:
                    pred = _no_prediction(cnt, _ref_get(ref, "filename"), None)
                preds.append(pred)
                cached.append({"reference_filename": pred.reference_filename, "success": pred.success,   # :193-204
                               "query_2D": m_q.reshape(-1, 1, 2), "reference_2D": m_r, "points_3D": m_x.reshape(-1, 1, 3),
                               "num_matches": pred.num_matches, "num_inliers": pred.num_inliers,
                               "inlier_mask": pred.inlier_mask, "quaternion": pred.quaternion, "matrix": pred.matrix})
        out.append(Localization(export=export, prediction=best, refined=None, kind=kind,
                                best=rec.best if best is not None else None, predictions=preds, cached_matches=cached))
    return out


def _refine(loc, qmap, refs, image_shape, refine_intrinsics, kw):
    """sparse_to_dense_predictor.py:238-255: the refinement of a successful best prediction, returned as
    optimize_feature_pnp returns it (optimize_feature_pnp.py:84-91)."""
    from .optimize_feature_pnp import feature_pnp
    if loc.prediction is None or not loc.prediction.success:
        return loc
    if refine_intrinsics not in ("last", "best"):
        raise ValueError('refine_intrinsics must be "last" or "best"')
    K = _ref_get(refs[-1] if refine_intrinsics == "last" else refs[loc.best], "intrinsics")  # :143,167,244
    ref_hc = _ref_get(refs[loc.best], "hypercolumn")
    layers = _layers_of(refs[loc.best]) if ref_hc is None else None
    if ref_hc is None and layers is None:
        raise ValueError("the refinement needs the best reference's hypercolumn or feature_maps")
    q = qmap if qmap.dim() == 4 else qmap[None]
    R, t, model = feature_pnp(q, ref_hc, loc.prediction, torch.from_numpy(np.asarray(K, dtype=np.float64)),
                              image_shape, reference_layers=layers, **kw)
    T = np.eye(4)
    T[:3, :3], T[3, :3] = R.numpy(), t.numpy()  # the reference writes t into the bottom row (:87)
    return loc._replace(refined=(list(t.numpy()), list(matrix_quaternion(T)), model))


def localize_multi(queries, image_shape, factor=None, reprojection_threshold=None, minimum_matches=None,
                   minimum_inliers=None, return_masked=None, iters=None, seed=None, track=False, feature_pyramid=None,
                   model=None, storage=None, layout=None, window=None, refine=True, return_all=False,
                   refine_intrinsics="last", match_precision="f32"):
    """B queries in one chain: queries = [(query_hypercolumn, references), ...].  The match launches of all
    the queries, one PnP launch over all B x top_N pairs (at most 65535), one pick launch and one host wait;
    then the refinements, query by query.  Each query's Localization equals localize's bit for bit.
    match_precision: "f32" (the exact default) or "f16" (the match stage on the fp16 matrix cores)."""
    queries = [(q, list(refs)) for q, refs in queries]
    params = _pnp_params(reprojection_threshold, minimum_matches, minimum_inliers, return_masked, iters, seed)
    queries = _rows_from_layers(queries)
    out = _run_sync(queries, image_shape, factor, params, return_all, match_precision=match_precision)
    if refine:
        kw = dict(track=track, feature_pyramid=feature_pyramid, model=model, storage=storage, layout=layout, window=window)
        out = [_refine(loc, q, refs, image_shape, refine_intrinsics, kw) for loc, (q, refs) in zip(out, queries)]
    return out


def localize(query_hypercolumn, references, image_shape, factor=None, reprojection_threshold=None,
             minimum_matches=None, minimum_inliers=None, return_masked=None, iters=None, seed=None, track=False,
             feature_pyramid=None, model=None, storage=None, layout=None, window=None, refine=True, return_all=False,
             refine_intrinsics="last", match_precision="f32"):
    """One query against its retrieved references, in rank order (sparse_to_dense_predictor.py:114-259):
    match, PnP, best pick and (refine=True) feature_pnp.  factor and the solve_pnp arguments left None come
    from fmpnp.config, as exhaustive_search and solve_pnp read them; track .. window are feature_pnp's.
    Two host waits: one after the pick kernel and one after the refiner.  Returns a Localization.
    match_precision: "f32" (the exact default) or "f16"."""
    return localize_multi([(query_hypercolumn, references)], image_shape, factor, reprojection_threshold,
                          minimum_matches, minimum_inliers, return_masked, iters, seed, track, feature_pyramid, model,
                          storage, layout, window, refine, return_all, refine_intrinsics, match_precision)[0]


def _host_map(t):
    t = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(t[0] if t.ndim == 4 else t, dtype=np.float32)


def glue_build_cpu(plan, argmax, mask, bufs):
    """fmpnp_localize_build_cpu on a plan whose pairs carry HOST point pointers; bufs: the sections' numpy
    arrays (written in place).  Returns the fmpnp_pnp_problem array."""
    m = _lib.LocMatches(bufs["m_q32"].ctypes.data, bufs["m_q64"].ctypes.data, bufs["m_x3"].ctypes.data,
                        bufs["m_r2"].ctypes.data, bufs["m_src"].ctypes.data, bufs["counts"].ctypes.data)
    probs = (_lib.PnpProblem * max(plan.n_pairs, 1))()
    rc = _lib.load().fmpnp_localize_build_cpu(plan.pairs, plan.n_pairs, ctypes.byref(plan.params), argmax.ctypes.data,
                                              mask.ctypes.data, plan.total_rows, ctypes.byref(m), probs)
    _lib.check(rc, "fmpnp_localize_build_cpu")
    return probs


def glue_pick_cpu(plan, results, pnp_mask, bufs):
    """fmpnp_localize_pick_cpu: results an fmpnp_pnp_result array, bufs as glue_build_cpu's (written in place)."""
    m = _lib.LocMatches(bufs["m_q32"].ctypes.data, bufs["m_q64"].ctypes.data, bufs["m_x3"].ctypes.data,
                        bufs["m_r2"].ctypes.data, bufs["m_src"].ctypes.data, bufs["counts"].ctypes.data)
    b = _lib.LocBest(bufs["b_pts3d"].ctypes.data, bufs["b_ref2d"].ctypes.data, bufs["b_q32"].ctypes.data,
                     bufs["b_idx"].ctypes.data, bufs["records"].ctypes.data)
    rc = _lib.load().fmpnp_localize_pick_cpu(plan.pairs, plan.n_pairs, plan.qdesc, plan.n_queries,
                                             ctypes.byref(plan.params), results, pnp_mask.ctypes.data, plan.total_rows,
                                             ctypes.byref(m), ctypes.byref(b))
    _lib.check(rc, "fmpnp_localize_pick_cpu")


def localize_cpu(query_hypercolumn, references, image_shape, factor=None, reprojection_threshold=None,
                 minimum_matches=None, minimum_inliers=None, return_masked=None, iters=None, seed=None, refine=False,
                 return_all=False, n_threads=0, fill=0, match_precision="f32"):
    """The same chain through the CPU twins (fmpnp_exhaustive_match_cpu, fmpnp_localize_build_cpu,
    fmpnp_pnp_ransac_cpu, fmpnp_localize_pick_cpu), up to the best prediction: localize(refine=False)'s
    result bit for bit.  Host arrays (or tensors, copied to the host).  An explicit entry point, never a
    fallback; the refinement has no place here (refine must be False).  match_precision="f16" composes the
    f16 precision's CPU reference (not a twin: the GPU chain's f16 decisions may differ on near-ties)."""
    _lib.match_precision(match_precision)
    if refine:
        raise ValueError("localize_cpu stops at the best prediction: refine must be False")
    from .match import exhaustive_match_cpu
    params = _pnp_params(reprojection_threshold, minimum_matches, minimum_inliers, return_masked, iters, seed)
    qmap = _host_map(query_hypercolumn)
    references = list(references)
    plan = _Plan([(torch.from_numpy(qmap), references)], image_shape, factor, params)
    c, width, height = plan.dims[0]
    for g in range(plan.n_pairs):
        plan.pairs[g].points3d, plan.pairs[g].points2d = plan.p3[g].ctypes.data or None, plan.p2[g].ctypes.data or None
    T = plan.total_rows
    rows = np.zeros((max(T, 1), c), np.float32)
    for g, ref in enumerate(references):
        off, n = plan.pairs[g].row_offset, plan.pairs[g].n_rows
        sparse = _ref_get(ref, "sparse_descriptors")
        if sparse is not None:
            rows[off:off + n] = _host_rows32(sparse, n, c)
        elif n:
            hc = _host_map(_ref_get(ref, "hypercolumn"))
            res = _ref_get(ref, "image_resolution")
            cells = nearest_cells(plan.p2[g], hc.shape[1], hc.shape[2], res[0] / hc.shape[1], res[1] / hc.shape[2])
            rows[off:off + n] = hc.reshape(c, -1)[:, cells].T
    if T:
        sel = exhaustive_match_cpu(rows[:T], qmap.reshape(c, -1), plan.top_k[0], RATIO, n_threads=n_threads,
                                   precision=match_precision)
        argmax, mask = sel["argmax"], sel["mask"].astype(np.uint8)
    else:
        argmax, mask = np.zeros(1, np.int32), np.zeros(1, np.uint8)
    head, every, tail = plan.sections(True)
    lay, n_out = _layout(head + every + tail)
    bufs = _views(np.full(n_out, int(fill), np.uint8), lay)
    probs = glue_build_cpu(plan, argmax, mask, bufs)
    results = (_lib.PnpResult * max(plan.n_pairs, 1)).from_buffer(bufs["results"])
    rc = _lib.load().fmpnp_pnp_ransac_cpu(probs, plan.n_pairs, results, bufs["pnp_mask"].ctypes.data, max(T, 0),
                                          int(n_threads))
    _lib.check(rc, "fmpnp_pnp_ransac_cpu")
    glue_pick_cpu(plan, results, bufs["pnp_mask"], bufs)
    return _parse(plan, bufs, bool(return_all))[0]


def _host_rows32(sparse, n, c):
    a = sparse.detach().cpu().numpy() if torch.is_tensor(sparse) else np.asarray(sparse)
    if a.shape != (n, c):
        raise ValueError(f"sparse_descriptors must be [{n}, {c}]")
    return a.astype(np.float32)
