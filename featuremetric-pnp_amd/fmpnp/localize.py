"""The localisation chain of one query on the GPU: match every retrieved reference, solve PnP for each,
pick the best prediction and refine it (SparseToDensePredictor.run,
s2dhm/pose_prediction/sparse_to_dense_predictor.py:114-259, with _choose_best_prediction and
_nearest_neighbor_prediction, predictor.py:48-73).

Between the stages nothing passes through the host: the match stage's argmax / mask stay on the device, a
glue kernel compacts the rows that passed the ratio test into the PnP stage's problems, the PnP stage reads
its sizes from those device descriptors, and a second glue kernel picks the best pair and assembles the
refiner's inputs (include/fmpnp.h, "localisation chain").  localize / localize_multi call the synchronous
fmpnp_localize: one upload, one pinned download and one host wait end the chain; the refinement
(fmpnp.feature_pnp) costs the second wait.  With refine="batched" (opt-in) the refinement is queued behind the
pick as well -- fmpnp_localize_refined: every query's refiner problem assembled on the device, one gather and one
launch per level over all the queries -- and the call keeps its one wait.

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

The query too may be given as its layers (opt-in): a list of float32 CUDA tensors [B, C_l, H_l, W_l], or a mapping
with feature_maps / feature_item, in place of query_hypercolumn.  The match then runs through layered matching
(fmpnp_localize_layers: the correlation per layer at the layer's own resolution, include/fmpnp.h "layered matching"
-- exact fp32 in its own rounding order, so within a stated bound of the dense query's scores, not on their bits),
and refine=True hands the layers to feature_pnp(query_layers=...): with references that carry feature_maps no dense
hypercolumn exists anywhere in the call.  match_precision="f16" and refine="batched" read dense maps and raise
ValueError with a layered query.

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


class _QueryLayers:
    """A query given as its encoder layers (float32 CUDA tensors [B, C_l, H_l, W_l]; item: its batch item): the
    match runs through layered matching (fmpnp_localize_layers) and the refinement takes the layers too, so the
    query's dense hypercolumn is never assembled.  shape / dim() read as the assembled [C, W, H] map's."""

    def __init__(self, maps, item=0):
        self.maps, self.item = list(maps), int(item or 0)
        if not self.maps or not all(torch.is_tensor(m) and m.dim() == 4 for m in self.maps):
            raise ValueError("a layered query is a list of [B, C_l, H_l, W_l] tensors")
        self.shape = (sum(int(m.shape[1]) for m in self.maps), int(self.maps[0].shape[2]), int(self.maps[0].shape[3]))

    def dim(self):
        return 3

    def one(self):
        """The query's own layers [1, C_l, H_l, W_l]."""
        return [m[self.item:self.item + 1] for m in self.maps]


def _as_query(q):
    """A query as localize takes it: a dense map (returned as it is), a list of layers, or a mapping with
    feature_maps / feature_item as references carry them."""
    if isinstance(q, _QueryLayers) or torch.is_tensor(q):
        return q
    if isinstance(q, (list, tuple)):
        return _QueryLayers(q)
    maps = _ref_get(q, "feature_maps")
    if maps is not None:
        return _QueryLayers(maps, _ref_get(q, "feature_item"))
    return q


def _layered(queries, match_precision, refine):
    """Whether the call's queries are layered (all of them or none); what a layered query cannot be combined with
    is a ValueError that names the argument."""
    flags = [isinstance(q, _QueryLayers) for q, _ in queries]
    if not any(flags):
        return False
    if not all(flags):
        raise ValueError("give every query of a call as layers, or every one as a dense map")
    if _lib.match_precision(match_precision) != _lib.MATCH_F32:
        raise ValueError('match_precision="f16" reads a dense query map: a layered query takes match_precision="f32"')
    if isinstance(refine, str):
        raise ValueError('refine="batched" reads dense query maps: a layered query takes refine=True or False')
    return True


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

    def __init__(self, queries, image_shape, factor, params, return_all=False, fill=0, match_precision="f32",
                 refine=None):
        """refine: a _RefineSpec -- the queries' packs are queued ahead of the match and
        fmpnp_localize_refine_async behind the pick, on caller-owned (torch) buffers; read() then returns the
        refined Localizations, after the same single wait."""
        prec = _lib.match_precision(match_precision)
        self.refine = refine
        if any(not torch.is_tensor(q) for q, _ in queries):
            raise ValueError("LocalizeLaunch takes dense query maps; a layered query goes through localize / localize_multi")
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
            if refine is not None:
                self._queue_packs(L, qmaps, int(fill), sp)
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
            if refine is not None:
                self._queue_refine(L, base_up, b_pairs, b, int(fill), sp)
            self.down = _pinned(self.n_down)
            self.down[:self.n_down].copy_(self.out_dev[:self.n_down], non_blocking=True)

    def _queue_packs(self, L, qmaps, fill, sp):
        """The queries' packed maps (fmpnp_pack_features' kernel, one launch per query) into this launch's slabs:
        they do not depend on the chain, so they are queued ahead of the match."""
        spec, dev = self.refine, self.device
        cs, C = spec.params.cstride, spec.params.C
        self.feats = []
        for qmap in qmaps:
            _, hf, wf = qmap.shape
            feat = torch.full((hf * wf * 3 * cs * spec.elem,), fill, dtype=torch.uint8, device=dev)
            if cs != C:
                feat.zero_()  # (the Sobel pack writes channels < C)
            rc = L.fmpnp_pack_features(qmap.data_ptr(), None, None, _lib.F32, C, hf, wf, feat.data_ptr(),
                                       spec.opts.dtype, cs, 0, 0, sp)
            _lib.check(rc, "fmpnp_pack_features")
            self.feats.append(feat)

    def _queue_refine(self, L, base_up, b_pairs, best, fill, sp):
        spec, plan, dev = self.refine, self.plan, self.device
        Q, P, O = max(plan.n_queries, 1), max(plan.n_pairs, 1), max(plan.out_rows, 1)
        maps = (_lib.LocRefineMap * Q)()
        for qi, feat in enumerate(self.feats):
            maps[qi].feat, maps[qi].Hf, maps[qi].Wf = feat.data_ptr(), plan.dims[qi][1], plan.dims[qi][2]
        rsrc = spec.sources(plan, dev, self.keep)
        tables = np.concatenate([np.frombuffer(rsrc, np.uint8), np.frombuffer(maps, np.uint8)])
        host = _pinned(len(tables))
        host.numpy()[:len(tables)] = tables
        self.tab_dev = torch.empty(len(tables), dtype=torch.uint8, device=dev)
        self.tab_dev.copy_(host[:len(tables)], non_blocking=True)
        ws = int(L.fmpnp_localize_refine_workspace_size(plan.qdesc, plan.n_queries, maps, ctypes.byref(spec.params),
                                                        ctypes.byref(spec.opts)))
        if plan.n_queries and not ws:
            _lib.check(_lib.ETOOBIG, "fmpnp_localize_refine_workspace_size")
        mk = lambda n: torch.full((max(n, 1),), fill, dtype=torch.uint8, device=dev)  # noqa: E731
        self.r_probs = mk(ctypes.sizeof(_lib.Problem) * Q * spec.n_res)
        self.r_fref = mk(O * spec.params.cstride * spec.elem)
        self.r_cost, self.r_sup = mk(8 * O), mk(4 * O)
        self.r_out = mk(_up(ctypes.sizeof(_lib.Result) * Q * spec.n_res) + 4 * Q)
        self.r_ws = mk(ws + 256)
        o_flags = _up(ctypes.sizeof(_lib.Result) * Q * spec.n_res)
        bufs = _lib.LocRefineBuffers(self.r_probs.data_ptr(), self.r_fref.data_ptr(), self.r_cost.data_ptr(),
                                     self.r_sup.data_ptr(), self.r_out.data_ptr(), self.r_out.data_ptr() + o_flags)
        ws_ptr = _up(self.r_ws.data_ptr())
        rc = L.fmpnp_localize_refine_async(base_up, plan.n_pairs, base_up + b_pairs, plan.qdesc, plan.n_queries,
                                           self.tab_dev.data_ptr(), self.tab_dev.data_ptr() + ctypes.sizeof(rsrc), maps,
                                           ctypes.byref(spec.params), ctypes.byref(spec.opts), ctypes.byref(best),
                                           ctypes.byref(bufs), ws_ptr, ws, sp)
        _lib.check(rc, "fmpnp_localize_refine_async")
        self.r_down = _pinned(self.r_out.numel())
        self.r_down[:self.r_out.numel()].copy_(self.r_out, non_blocking=True)
        self.r_flags_at = o_flags

    def read(self):
        """Wait for the stream (the chain's one host wait) and return one Localization per query: unrefined, or
        with a _RefineSpec refined."""
        self.stream.synchronize()
        host = self.down[:self.n_down].numpy().copy()
        head, every, _ = self.plan.sections(self.return_all)
        lay, _ = _layout(head + (every if self.return_all else []))
        locs = _parse(self.plan, _views(host, lay), self.return_all)
        if self.refine is None:
            return locs
        from .refine import RESULT_DTYPE
        Q, n_res = max(self.plan.n_queries, 1), self.refine.n_res
        got = self.r_down[:self.r_out.numel()].numpy().copy()
        res = got[:ctypes.sizeof(_lib.Result) * Q * n_res].view(RESULT_DTYPE).reshape(Q, n_res)
        flags = got[self.r_flags_at:self.r_flags_at + 4 * Q].view(np.int32)
        return self.refine.apply(locs, self.plan, res, flags)


class _RefineSpec:
    """What refine="batched" hands to the chain: the refiner's options, the channel levels and the choice of K,
    resolved as feature_pnp's one-call path resolves them for every query (optimize_feature_pnp.py:50-71)."""

    def __init__(self, C, image_shape, feature_pyramid, model, storage, refine_intrinsics):
        from . import refine as _rf
        from .optimize_feature_pnp import _channel_levels, _new_model
        if refine_intrinsics not in ("last", "best"):
            raise ValueError('refine_intrinsics must be "last" or "best"')
        self.model, self.image_shape, self.refine_intrinsics = model, image_shape, refine_intrinsics
        m = _new_model(model)
        self.storage = storage or m.storage or torch.float32  # (the queries' maps are float32)
        if self.storage not in (torch.float32, torch.float64):
            raise ValueError('refine="batched" stores float32 or float64; use refine=True')
        levels = _channel_levels(feature_pyramid, C)
        if feature_pyramid is not None and (not levels or not all(0 <= a < b for a, b in levels)
                                            or len(levels) > _lib.LOC_REFINE_MAX_LEVELS):
            raise ValueError('refine="batched" takes a feature_pyramid of channel levels only; use refine=True')
        self.levels = levels or []
        self.n_res = len(self.levels) + 1 if self.levels else 1
        self.opts = m._options(_rf._dtype_code(self.storage))
        self.opts.layout, self.opts.sobel_flags = _lib.LAYOUT_FGRAD, 0
        self.lv = (_lib.Level * max(len(self.levels), 1))(*[_lib.Level(a, b) for a, b in self.levels])
        self.params = _lib.LocRefineParams(C, _rf._round4(C), int(image_shape[0]), int(image_shape[1]),
                                           _lib.LOC_K_BEST if refine_intrinsics == "best" else _lib.LOC_K_LAST,
                                           len(self.levels), self.lv)
        self.elem = 8 if self.storage == torch.float64 else 4

    def source(self, ref, dev, keep):
        """The pair's fmpnp_loc_refine_source fields: the reference's dense map as it is (float32 or float64)."""
        hc = _ref_get(ref, "hypercolumn")
        if hc is None:
            return None
        hc = torch.as_tensor(hc)
        hc = hc[0] if hc.dim() == 4 else hc
        if hc.dtype not in (torch.float32, torch.float64):
            hc = hc.to(torch.float32)
        hc = hc.to(dev).contiguous()
        if hc.dim() != 3 or hc.shape[0] != self.params.C:
            raise ValueError(f"the reference map has {tuple(hc.shape)[0]} channels, the query {self.params.C}")
        keep.append(hc)
        return hc.data_ptr(), _lib.F64 if hc.dtype == torch.float64 else _lib.F32, int(hc.shape[1]), int(hc.shape[2])

    def sources(self, plan, dev, keep):
        out, g = (_lib.LocRefineSource * max(plan.n_pairs, 1))(), 0
        for refs in plan.refs:
            for ref in refs:
                src = self.source(ref, dev, keep)
                if src is not None:
                    out[g].ref_chw, out[g].dtype, out[g].H_ref, out[g].W_ref = src
                g += 1
        return out

    def apply(self, locs, plan, res, flags, first=0):
        """The stage's results -> every Localization's refined, as _refine builds it from feature_pnp's."""
        from . import refine as _rf
        from .optimize_feature_pnp import _apply_one_call_results, _new_model
        out = []
        for qi, loc in enumerate(locs):
            if loc.prediction is None or not loc.prediction.success:
                out.append(loc)
                continue
            refs = plan.refs[qi]
            if _ref_get(refs[loc.best], "hypercolumn") is None:
                raise ValueError("the refinement needs the best reference's hypercolumn (refine=\"batched\" reads dense "
                                 "reference maps; use refine=True for feature_maps)")
            if flags[qi]:
                raise IndexError(f"query {first + qi}: a reference inlier maps outside the reference hypercolumn "
                                 "(optimize_feature_pnp.py:56 raises IndexError)")
            rows = _rf.results_from_array(res[qi])
            if any(x["status"] & _lib.STATUS_SYNC_TIMEOUT for x in rows):
                raise _lib.FmpnpError("cross-workgroup exchange timed out (device oversubscribed?)")
            K = _ref_get(refs[-1] if self.refine_intrinsics == "last" else refs[loc.best], "intrinsics")
            Kn = np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(3, 3))
            T = np.asarray(loc.prediction.matrix, dtype=np.float64)
            R0, t0 = np.ascontiguousarray(T[:3, :3]), np.ascontiguousarray(T[:3, 3])
            pts = np.ascontiguousarray(np.asarray(loc.prediction.points_3d, dtype=np.float64).reshape(-1, 3))
            R, t, model = _apply_one_call_results(_new_model(self.model), rows, len(self.levels), R0, t0, pts, Kn,
                                                  self.image_shape, False, lambda i, n_evals: None)
            M = np.eye(4)
            M[:3, :3], M[3, :3] = R.numpy(), t.numpy()  # the reference writes t into the bottom row (:87)
            out.append(loc._replace(refined=(list(t.numpy()), list(matrix_quaternion(M)), model)))
        return out


def _run_sync(queries, image_shape, factor, params, return_all, fill=0, match_precision="f32", refine=None, first=0):
    """fmpnp_localize: the chain in one call with one upload, one pinned download and one host wait on the
    current stream of the queries' device.  Returns one (unrefined) Localization per query.  fill: the byte
    the host arrays hold before the call; no output depends on it.  match_precision "f16": fmpnp_localize_ex.
    refine: a _RefineSpec -- fmpnp_localize_refined, the batched refinement stage behind the pick in the same call
    (still one wait); the Localizations then come back refined.  first: the index of the call's first query
    among the caller's (error messages)."""
    prec = _lib.match_precision(match_precision)
    plan = _Plan(queries, image_shape, factor, params)
    L = _lib.load()
    layered = bool(queries) and isinstance(queries[0][0], _QueryLayers)  # (all or none: localize_multi checked)
    qmaps, qlayers = [], (_lib.LocQueryLayers * max(len(queries), 1))()
    for qi, (qmap, _) in enumerate(queries):
        if layered:  # fmpnp_loc_query_layers: the descriptors (and the tensors they point into) live until the call ends
            from .hypercolumn import _plane_layers
            desc, held = _plane_layers(qmap.maps, "cuda")
            if not 0 <= qmap.item < int(held[0].shape[0]):
                raise ValueError(f"feature_item {qmap.item} of a batch of {int(held[0].shape[0])}")
            ql = qlayers[qi]
            ql.layers, ql.L, ql.B, ql.item = desc, len(held), int(held[0].shape[0]), qmap.item
            ql.H, ql.W, ql.flags = qmap.shape[1], qmap.shape[2], _lib.HC_NORMALIZE
            qmaps.append((desc, held))
            continue
        qmap = qmap[0] if qmap.dim() == 4 else qmap
        if not qmap.is_cuda or qmap.dtype != torch.float32:
            raise ValueError("query_hypercolumn must be a float32 CUDA tensor [C, W, H]")
        qmaps.append(qmap.contiguous())
    if layered:
        dev = qmaps[0][1][0].device
    else:
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
    dense = qlayers if layered else (ctypes.c_void_p * max(Q, 1))(*[q.data_ptr() for q in qmaps])
    top_k = (ctypes.c_int * max(Q, 1))(*plan.top_k)
    with torch.cuda.device(dev):
        args = (plan.pairs, sources, P, plan.qdesc, dense, top_k, Q, c, float(RATIO), ctypes.byref(plan.params),
                plan.total_rows, ctypes.byref(b), ctypes.byref(m) if return_all else None,
                bufs["results"].ctypes.data if return_all else None,
                bufs["pnp_mask"].ctypes.data if return_all else None)
        if refine is not None:
            hw = (ctypes.c_int * max(2 * Q, 1))(*[v for d in plan.dims for v in (d[1], d[2])])  # (Hf, Wf) = shape[1:]
            res = np.full(max(Q, 1) * refine.n_res * ctypes.sizeof(_lib.Result), int(fill), np.uint8)
            flags = np.full(max(Q, 1), int(fill) * 0x01010101, np.uint32).view(np.int32)
            rsrc = refine.sources(plan, dev, keep)
            rc = L.fmpnp_localize_refined(*args, prec, rsrc, hw, ctypes.byref(refine.params), ctypes.byref(refine.opts),
                                          res.ctypes.data, flags.ctypes.data, _lib.stream_ptr(dev))
        elif layered:
            rc = L.fmpnp_localize_layers(*args, _lib.stream_ptr(dev))
        elif prec == _lib.MATCH_F32:
            rc = L.fmpnp_localize(*args, _lib.stream_ptr(dev))
        else:
            rc = L.fmpnp_localize_ex(*args, prec, _lib.stream_ptr(dev))
    _lib.check(rc, "fmpnp_localize_refined" if refine is not None else "fmpnp_localize")
    locs = _parse(plan, bufs, bool(return_all))
    if refine is None:
        return locs
    from .refine import RESULT_DTYPE
    return refine.apply(locs, plan, res.view(RESULT_DTYPE).reshape(max(Q, 1), refine.n_res), flags, first)


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
    if isinstance(qmap, _QueryLayers):  # the fused pack: the query's dense map is not assembled here either
        q, q_layers = None, qmap.one()
    else:
        q, q_layers = (qmap if qmap.dim() == 4 else qmap[None]), None
    R, t, model = feature_pnp(q, ref_hc, loc.prediction, torch.from_numpy(np.asarray(K, dtype=np.float64)),
                              image_shape, reference_layers=layers, query_layers=q_layers, **kw)
    T = np.eye(4)
    T[:3, :3], T[3, :3] = R.numpy(), t.numpy()  # the reference writes t into the bottom row (:87)
    return loc._replace(refined=(list(t.numpy()), list(matrix_quaternion(T)), model))


def localize_multi(queries, image_shape, factor=None, reprojection_threshold=None, minimum_matches=None,
                   minimum_inliers=None, return_masked=None, iters=None, seed=None, track=False, feature_pyramid=None,
                   model=None, storage=None, layout=None, window=None, refine=True, return_all=False,
                   refine_intrinsics="last", match_precision="f32", refine_group=None):
    """B queries in one chain: queries = [(query_hypercolumn, references), ...].  The match launches of all
    the queries, one PnP launch over all B x top_N pairs (at most 65535), one pick launch and one host wait;
    then the refinements, query by query.  Each query's Localization equals localize's bit for bit.
    match_precision: "f32" (the exact default) or "f16" (the match stage on the fp16 matrix cores).

    refine="batched" (opt-in; True stays the per-query path): the refinement runs behind the pick in the same
    call, on the device -- every query's problem assembled there, the reference descriptors of all the queries
    gathered in one launch, compute_cost and each channel level as one launch over the B queries -- and comes
    back in the chain's one download after its one wait.  The Localizations equal refine=True's bit for bit.
    It takes dense query maps and dense reference hypercolumns, feature_pyramid of channel levels (or None), model,
    storage (float32 / float64), refine_intrinsics, match_precision and return_all; track=True, an explicit window,
    layout="f" and references given as feature_maps raise ValueError (use refine=True).  An inlier outside its
    reference map raises IndexError, as refine=True does, naming the query's index.  B packed maps are resident
    at once (12 C H W bytes each in float32): refine_group = the queries per chain call, None = as many as fit
    half of the free device memory; the groups are independent calls and a result does not depend on them."""
    queries = [(_as_query(q), list(refs)) for q, refs in queries]
    _layered(queries, match_precision, refine)
    params = _pnp_params(reprojection_threshold, minimum_matches, minimum_inliers, return_masked, iters, seed)
    if isinstance(refine, str):
        if refine != "batched":
            raise ValueError('refine must be True, False or "batched"')
        return _localize_batched(queries, image_shape, factor, params, return_all, match_precision, track, feature_pyramid,
                                 model, storage, layout, window, refine_intrinsics, refine_group)
    queries = _rows_from_layers(queries)
    out = _run_sync(queries, image_shape, factor, params, return_all, match_precision=match_precision)
    if refine:
        kw = dict(track=track, feature_pyramid=feature_pyramid, model=model, storage=storage, layout=layout, window=window)
        out = [_refine(loc, q, refs, image_shape, refine_intrinsics, kw) for loc, (q, refs) in zip(out, queries)]
    return out


def _batched_args(queries, track, layout, window):
    """refine="batched" takes less than refine=True: every other input is a ValueError that names it."""
    if track:
        raise ValueError('refine="batched" records no track_; use refine=True with track=True')
    if window is not None:
        raise ValueError('refine="batched" packs the queries\' maps in full; use refine=True with a window')
    if layout not in (None, "fgrad"):
        raise ValueError('refine="batched" packs the f, gx, gy planes; use refine=True with layout="f"')
    for _, refs in queries:
        for ref in refs:
            if _ref_get(ref, "feature_maps") is not None and _ref_get(ref, "hypercolumn") is None:
                raise ValueError('refine="batched" reads dense reference hypercolumns; use refine=True with feature_maps')


def _group_size(queries, spec, refine_group):
    """The queries per chain call: refine_group, or what fits half of the free device memory (a query's packed
    map, 3 cstride Hf Wf elements, dominates what it keeps resident)."""
    if refine_group is not None:
        if int(refine_group) < 1:
            raise ValueError("refine_group must be at least 1")
        return int(refine_group)
    if not queries:
        return 1
    q = queries[0][0]
    dev = q.device if q.is_cuda else torch.device("cuda", torch.cuda.current_device())
    free, _ = torch.cuda.mem_get_info(dev)
    per = max(q[0].numel() if q.dim() == 4 else q.numel(), 1) // max(spec.params.C, 1) * 3 * spec.params.cstride * spec.elem
    return max(1, int(free // 2 // max(per, 1)))


def _localize_batched(queries, image_shape, factor, params, return_all, match_precision, track, feature_pyramid, model,
                      storage, layout, window, refine_intrinsics, refine_group):
    _batched_args(queries, track, layout, window)
    if not queries:
        return []
    q0 = queries[0][0]
    spec = _RefineSpec(int((q0[0] if q0.dim() == 4 else q0).shape[0]), image_shape, feature_pyramid, model, storage,
                       refine_intrinsics)
    n, out = _group_size(queries, spec, refine_group), []
    for at in range(0, len(queries), n):
        out += _run_sync(queries[at:at + n], image_shape, factor, params, return_all, match_precision=match_precision,
                         refine=spec, first=at)
    return out


def localize(query_hypercolumn, references, image_shape, factor=None, reprojection_threshold=None,
             minimum_matches=None, minimum_inliers=None, return_masked=None, iters=None, seed=None, track=False,
             feature_pyramid=None, model=None, storage=None, layout=None, window=None, refine=True, return_all=False,
             refine_intrinsics="last", match_precision="f32", refine_group=None):
    """One query against its retrieved references, in rank order (sparse_to_dense_predictor.py:114-259):
    match, PnP, best pick and (refine=True) feature_pnp.  factor and the solve_pnp arguments left None come
    from fmpnp.config, as exhaustive_search and solve_pnp read them; track .. window are feature_pnp's.
    Two host waits: one after the pick kernel and one after the refiner.  Returns a Localization.
    match_precision: "f32" (the exact default) or "f16".  refine="batched": the refinement behind the pick in
    the same call, one host wait (localize_multi says what it takes)."""
    return localize_multi([(query_hypercolumn, references)], image_shape, factor, reprojection_threshold,
                          minimum_matches, minimum_inliers, return_masked, iters, seed, track, feature_pyramid, model,
                          storage, layout, window, refine, return_all, refine_intrinsics, match_precision, refine_group)[0]


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


def glue_refine_prep_cpu(plan, bufs, sources, maps, rparams, dtype, fref, flags):
    """fmpnp_localize_refine_prep_cpu: the refinement stage's descriptors, reference rows and flags from the pick
    step's outputs in bufs (HOST arrays; sources: a LocRefineSource array over HOST maps; maps: a LocRefineMap
    array; fref / flags: numpy arrays written in place).  Returns the fmpnp_problem array [n_res][n_queries]."""
    b = _lib.LocBest(bufs["b_pts3d"].ctypes.data, bufs["b_ref2d"].ctypes.data, bufs["b_q32"].ctypes.data,
                     bufs["b_idx"].ctypes.data, bufs["records"].ctypes.data)
    n_res = rparams.n_levels + 1 if rparams.n_levels else 1
    probs = (_lib.Problem * max(plan.n_queries * n_res, 1))()
    rc = _lib.load().fmpnp_localize_refine_prep_cpu(plan.pairs, plan.n_pairs, plan.qdesc, plan.n_queries, sources, maps,
                                                    ctypes.byref(rparams), int(dtype), ctypes.byref(b), probs,
                                                    fref.ctypes.data, flags.ctypes.data)
    _lib.check(rc, "fmpnp_localize_refine_prep_cpu")
    return probs


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
    from .match import exhaustive_match_cpu, exhaustive_match_layers_cpu
    params = _pnp_params(reprojection_threshold, minimum_matches, minimum_inliers, return_masked, iters, seed)
    query = _as_query(query_hypercolumn)
    references = list(references)
    if isinstance(query, _QueryLayers):  # the layered twin on host copies of the layers
        _layered([(query, references)], match_precision, False)
        query = _QueryLayers([m.detach().to(device="cpu", dtype=torch.float32) for m in query.maps], query.item)
        plan = _Plan([(query, references)], image_shape, factor, params)
    else:
        qmap = _host_map(query_hypercolumn)
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
    if T and isinstance(query, _QueryLayers):
        sel = exhaustive_match_layers_cpu(rows[:T], query.maps, plan.top_k[0], RATIO, item=query.item, n_threads=n_threads)
        argmax, mask = sel["argmax"], sel["mask"].astype(np.uint8)
    elif T:
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
