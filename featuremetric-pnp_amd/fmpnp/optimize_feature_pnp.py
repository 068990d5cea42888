"""Adapter: feature_pnp / optimize_feature_pnp (s2dhm/pose_prediction/optimize_feature_pnp.py:50-91)
and the DirectPoseModel call surface named by the build's north star.

The reference copies the GPU hypercolumn to host fp64, gathers the reference
descriptors with a per-point python loop, runs the Sobel on the CPU and then the
LM loop on the CPU (optimize_feature_pnp.py:51-69).  Here the query hypercolumn
stays on the device: one fused Sobel + channels-last pack kernel, one gather
kernel for the reference descriptors, one LM launch.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib, config
from . import refine as _rf
from .matrix_utils import matrix_quaternion
from .model import _find_inliers_packed, sparseFeaturePnP


def _new_model(model):
    if model is not None:
        return model
    return sparseFeaturePnP(**config.model_kwargs())  # "Parameters from gin!" (optimize_feature_pnp.py:63)


def feature_pnp_multi(query_hypercolumns, reference_hypercolumns, prediction, K, image_shape, track=False,
                      model=None, storage=None, rounds=3):
    """optimize_feature_pnp.py:20-47: refine on the current inliers, re-select the inliers
    with find_inliers at the new pose, three times.  The initial inliers are
    prediction.inlier_mask, or find_inliers at the initial pose when it is None.  The query
    map is packed once (f, gx, gy planes); every round reuses it and the
    device fref.  Returns (R, t, model) like feature_pnp."""
    model = _new_model(model)
    q = query_hypercolumns[0] if query_hypercolumns.dim() == 4 else query_hypercolumns
    dev = q.device if q.is_cuda else torch.device("cuda", torch.cuda.current_device())
    storage = storage or model.storage or (torch.float64 if q.dtype == torch.float64 else torch.float32)
    # (three LM launches and four point-cost launches on one map: the packed f/gx/gy planes, as
    # feature_pnp -- the LM reads 16C bytes per gathered texel from them against 40C from "f")
    feats = _rf.pack_features(q, storage=storage, device=dev, layout="fgrad")              # :28,31
    fref = _rf.gather_reference(reference_hypercolumns, prediction.reference_inliers, image_shape,
                                cstride=feats.cstride, storage=storage, device=dev)          # :21-26
    pts3D = np.asarray(prediction.points_3d, dtype=np.float64).reshape(-1, 3)               # :22
    T = np.asarray(prediction.matrix, dtype=np.float64)
    R, t = torch.from_numpy(T[:3, :3].copy()), torch.from_numpy(T[:3, 3].copy())             # :30-31
    Kt = K if isinstance(K, torch.Tensor) else torch.from_numpy(np.asarray(K, dtype=np.float64))
    W, H = image_shape[0], image_shape[1]
    if prediction.inlier_mask is not None:                                                  # :35-39
        inliers = torch.zeros(pts3D.shape[0], dtype=torch.bool)
        inliers[torch.as_tensor(np.asarray(prediction.inlier_mask))] = True
    else:
        print("No initial inliers found.")
        inliers = _find_inliers_packed(feats, pts3D, R, t, fref, Kt, W, H)
    for _ in range(rounds):                                                                 # :43-46
        idx = inliers.numpy()
        R, t = model._forward_packed(feats, pts3D[idx], fref[inliers.to(dev)], Kt, W, H, R, t, track)
        inliers = _find_inliers_packed(feats, pts3D, R, t, fref, Kt, W, H)
    return R, t, model


def _reference_layers(reference_layers, normalize=True):
    """reference_layers (the encoder's [1, C_l, H_l, W_l] CUDA maps of the reference image) as the sparse
    hypercolumn's source: (fmpnp_hc_layer array, the tensors it points into, C, H, W, flags)."""
    from .hypercolumn import _layers
    layers, keep = _layers(reference_layers, "cuda")
    if keep[0].shape[0] != 1:
        raise ValueError("reference_layers must be the maps of one image: [1, C_l, H_l, W_l]")
    return (layers, keep, sum(int(m.shape[1]) for m in keep), int(keep[0].shape[2]), int(keep[0].shape[3]),
            _lib.HC_NORMALIZE if normalize else 0)


def _gather_reference_rows(reference_hypercolumns, reference_layers, inliers, image_shape, cstride, storage, dev):
    """The reference descriptors [N, cstride] of the step-by-step paths: gathered from the dense map, or (with
    reference_layers) formed by the sparse hypercolumn kernel without one -- the same bits."""
    if reference_layers is None:
        return _rf.gather_reference(reference_hypercolumns, inliers, image_shape, cstride=cstride, storage=storage,
                                    device=dev)
    from .hypercolumn import sparse_hypercolumn
    n = np.asarray(inliers).reshape(-1, 2).shape[0] if not torch.is_tensor(inliers) else inliers.reshape(-1, 2).shape[0]
    channels = sum(int(m.shape[1]) for m in reference_layers)
    out = torch.zeros((n, cstride or _rf._round4(channels)), dtype=storage, device=dev)
    sparse_hypercolumn(reference_layers, inliers, at="reference", image_shape=image_shape, dtype=storage,
                       out=out[:, :channels])
    return out


def feature_pnp(query_hypercolumns, reference_hypercolumns, prediction, K, image_shape, track=False,
                feature_pyramid=None, model=None, storage=None, layout=None, window=None, reference_layers=None,
                query_layers=None):
    """optimize_feature_pnp.py:50-71.  Returns (R, t, model) with R, t fp64 CPU tensors.

    layout: None (default) packs the f/gx/gy planes ("fgrad": the fused Sobel + channels-last
    pack); "f" packs f only (FMPNP_LAYOUT_F: a third of the pack's bytes, the LM kernel forms
    the fp64 Sobel gradients of every texel it gathers).  One query per call is LM-bound, and
    the LM reads 16C bytes per gathered texel from "fgrad" against 40C from "f": cfg2, one
    call, pack + LM 66 + 259 us against 33 + 559 us (rocprofv3, profiles/r05_facade_*).

    window: the one-call path packs only the texels within `window` texels of each point's texel
    at the initial pose (fmpnp_feature_pnp; a point that leaves its window re-runs the call fully
    packed, so results are the full pack's bit for bit); None = window_radius(C, H, W, N), 0 = off.

    reference_layers: the reference image's encoder maps (a list of [1, C_l, H_l, W_l] CUDA tensors, as
    HypercolumnExtractor.compute_feature_maps returns) in place of its dense hypercolumn --
    reference_hypercolumns may then be None.  The reference descriptors are formed straight from the layers
    (fmpnp_feature_pnp_layers / sparse_hypercolumn), so the dense reference map is never assembled; the
    results are those of the assembled map, bit for bit.

    query_layers: the query image's encoder maps (the same kind of list) in place of its dense hypercolumn --
    query_hypercolumns must then be None (both given is a ValueError).  The packed map is formed straight from the
    layers (fmpnp_feature_pnp_query_layers under the one-call path's conditions, pack_hypercolumn on the
    step-by-step path), so the dense query map is never assembled -- except for a pyramid with a resized or
    blurred level (target_size / kernel_size), which is cut from the dense map: that path assembles it.  The
    results are those of assemble_hypercolumn's map, bit for bit, either way.

    storage: torch.float32 / torch.float64 (default: by the query's dtype), or torch.float16 -- opt-in binary16
    storage of the packed map and the descriptors (include/fmpnp.h, FMPNP_F16): dense maps, layout "fgrad" and
    nearest sampling only (anything else is a ValueError)."""
    model = _new_model(model)
    if layout is None:
        layout = "fgrad"
    if (storage or model.storage) == torch.float16:
        # binary16 storage (include/fmpnp.h, FMPNP_F16): the dense maps' packed f, gx, gy planes only
        if reference_layers is not None or query_layers is not None:
            raise ValueError("binary16 storage takes dense hypercolumns: reference_layers / query_layers are not "
                             "supported (the sparse and fused-pack hypercolumn kernels do not write float16)")
        if layout == "f":
            raise ValueError("binary16 storage has no layout 'f' (the f-only layout is fp32)")
    if query_layers is not None:
        if query_hypercolumns is not None:
            raise ValueError("feature_pnp takes the query as query_hypercolumns or as query_layers, not both")
        from .hypercolumn import _layers, assemble_hypercolumn, pack_hypercolumn
        query_layers = list(query_layers)
        _, keep = _layers(query_layers, "cuda")
        if keep[0].shape[0] != 1:
            raise ValueError("query_layers must be the maps of one image: [1, C_l, H_l, W_l]")
        # an empty tensor stands for the map the layers would assemble to (its device, dtype and channel count are
        # all the path choice below asks of q); the map itself is never formed
        q = keep[0].new_empty((sum(int(m.shape[1]) for m in keep), 0, 0))
    else:
        q = query_hypercolumns[0] if query_hypercolumns.dim() == 4 else query_hypercolumns
    dev = q.device if q.is_cuda else torch.device("cuda", torch.cuda.current_device())
    storage = storage or model.storage or (torch.float64 if q.dtype == torch.float64 else torch.float32)
    levels = _channel_levels(feature_pyramid, q.shape[0])
    if reference_layers is not None:
        reference_layers = list(reference_layers)
    elif reference_hypercolumns is None:
        raise ValueError("feature_pnp needs reference_hypercolumns or reference_layers")
    if _one_call_ok(model, q, reference_hypercolumns, feature_pyramid, levels, track, storage, layout,
                    reference_layers):
        return _feature_pnp_one_call(model, q, reference_hypercolumns, prediction, K, image_shape, track, levels,
                                     storage, layout, window, reference_layers, query_layers)
    if query_layers is None:
        feats = _rf.pack_features(q, storage=storage, device=dev, layout=layout)           # :57, :61
    else:
        with torch.cuda.device(dev):
            feats = pack_hypercolumn(query_layers, storage=storage, layout=layout)
        # a resized or blurred level is cut from the dense map itself: only then is it assembled
        dense = any(ts is not None or ks is not None for _, _, ts, ks in feature_pyramid or ())
        q = assemble_hypercolumn(query_layers)[0] if dense else None
    fref = _gather_reference_rows(reference_hypercolumns, reference_layers, prediction.reference_inliers, image_shape,
                                  feats.cstride, storage, dev)                               # :51-56
    pts3D = np.asarray(prediction.points_3d, dtype=np.float64).reshape(-1, 3)               # :52
    T = np.asarray(prediction.matrix, dtype=np.float64)
    R, t = torch.from_numpy(T[:3, :3].copy()), torch.from_numpy(T[:3, 3].copy())             # :59-60
    Kt = K if isinstance(K, torch.Tensor) else torch.from_numpy(np.asarray(K, dtype=np.float64))
    if feature_pyramid is None:                                                             # :64-69
        R, t = model._forward_packed(feats, pts3D, fref, Kt, image_shape[0], image_shape[1], R, t, track)
    else:
        R, t = model._multilevel_packed(feature_pyramid, feats, q, pts3D, fref, Kt, image_shape[0], image_shape[1],
                                        R, t, track)
    return R, t, model


def _channel_levels(feature_pyramid, C):
    """multilevel_optimization's levels (model.py:193-194) as channel ranges [start, min(end, C))
    when every level is a plain channel slice (no resize, no blur); None otherwise."""
    if feature_pyramid is None:
        return None
    out = []
    for start, end, target_size, kernel_size in feature_pyramid:
        if target_size is not None or kernel_size is not None:
            return None
        out.append((int(start), min(int(end), C)))  # python slicing clamps (model.py:194)
    return out


def _one_call_ok(model, q, r, feature_pyramid, levels, track, storage, layout, reference_layers=None):
    """fmpnp_feature_pnp runs the whole call (pack, gather, compute_cost, every level) with one
    host wait when both maps are device tensors of the same device and channel count and the
    pyramid is channel slices only; track_ with the ratio test needs the packed map for its
    threshold masks (fmpnp_point_costs), so that case takes the step-by-step path."""
    if reference_layers is not None:
        # (the layers stand for the dense map: float32 CUDA maps of one image on the query's device whose
        # channels add up to the query's)
        ref_ok = (all(torch.is_tensor(m) and m.is_cuda and m.device == q.device and m.dim() == 4
                      and m.dtype == torch.float32 and m.shape[0] == 1 for m in reference_layers)
                  and sum(int(m.shape[1]) for m in reference_layers) == q.shape[0])
    else:
        r = r[0] if r.dim() == 4 else r
        ref_ok = (r.is_cuda and q.device == r.device and r.dim() == 3
                  and r.dtype in (torch.float32, torch.float64) and r.shape[0] == q.shape[0])
    ok = (q.is_cuda and ref_ok and q.dim() == 3
          and q.dtype in (torch.float32, torch.float64)
          and storage in (torch.float32, torch.float64, torch.float16)
          and not (track and model.use_ratio_test_) and (layout == "fgrad" or storage == torch.float32))
    if feature_pyramid is not None:
        ok = ok and levels is not None and len(levels) > 0 and all(0 <= a < b for a, b in levels)
    return ok


def window_radius(C, H, W, N):
    """The one-call path's default pack window (texels): FMPNP_FACADE_WINDOW overrides."""
    env = os.environ.get("FMPNP_FACADE_WINDOW")
    if env is not None:
        return int(env)
    # wide maps only: the windowed pack saves the writes of the unmarked texels (RobotCar C = 1664 at
    # 256x256, 295 / 866 points: 1.57 -> 1.42 / 1.97 -> 1.88 ms per call), but a window turns the
    # speculative gathers off (cfg2, C = 256: 0.450 -> 0.465 ms); radius 6: no re-run over the
    # synthetic starts at radii >= 5 (profiles/r05_facade_window_sweep.txt)
    return 6 if C > 256 else 0


_DP = ctypes.POINTER(ctypes.c_double)


def _feature_pnp_one_call(model, q, r, prediction, K, image_shape, track, levels, storage, layout, window=None,
                          reference_layers=None, query_layers=None):
    """feature_pnp through fmpnp_feature_pnp (or, with reference_layers, fmpnp_feature_pnp_layers; with
    query_layers, fmpnp_feature_pnp_query_layers): one host call, one host wait (optimize_feature_pnp.py:50-71)."""
    if reference_layers is None:
        r = r[0] if r.dim() == 4 else r
        r = r.contiguous()
    if query_layers is None:
        q = q.contiguous()
        dev = q.device
        C, H, W = q.shape
        query_args = (q.data_ptr(), _rf._dtype_code(q.dtype), C, H, W)
    else:
        q_layers, q_keep, C, H, W, q_flags = _reference_layers(query_layers)  # (q_keep: alive until the wait)
        dev = q_keep[0].device
        query_args = (q_layers, len(q_keep), H, W, q_flags)
    opts = model._options(_rf._dtype_code(storage))
    opts.layout = _lib.LAYOUT_F if layout == "f" else _lib.LAYOUT_FGRAD
    opts.sobel_flags = 0
    inl = np.ascontiguousarray(np.asarray(prediction.reference_inliers, dtype=np.float64).reshape(-1, 2))  # :53
    pts = np.ascontiguousarray(np.asarray(prediction.points_3d, dtype=np.float64).reshape(-1, 3))          # :52
    if inl.shape[0] != pts.shape[0]:
        raise ValueError("reference_inliers and points_3d must have one row per match")
    T = np.asarray(prediction.matrix, dtype=np.float64)
    R0, t0 = np.ascontiguousarray(T[:3, :3]), np.ascontiguousarray(T[:3, 3])                            # :59-60
    Kn = np.ascontiguousarray((K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else np.asarray(K))
                              .astype(np.float64).reshape(3, 3))
    n_lv = len(levels) if levels else 0
    if window is None:
        window = window_radius(C, H, W, pts.shape[0])
    if layout != "fgrad" or getattr(model, "sampling", "nearest") != "nearest":
        window = 0
    lv = (_lib.Level * n_lv)(*[_lib.Level(a, b) for a, b in levels]) if n_lv else None
    res = np.zeros(n_lv + 1 if n_lv else 1, dtype=_rf.RESULT_DTYPE)
    want_trace = bool(track) or bool(model.verbose)
    stride = model.iterations + 1
    tr = (_lib.TraceEntry * (max(n_lv, 1) * stride))() if want_trace else None
    # (c_void_p arguments take plain addresses; the device switch only when the map is not on the current one)
    lib = _lib.load()
    if reference_layers is None:
        ref_map = (r.data_ptr(), _rf._dtype_code(r.dtype))
    else:
        hc_layers, keep, _, H_ref, W_ref, ref_flags = _reference_layers(reference_layers)  # (keep: alive until the wait)
    if query_layers is not None:  # (this entry takes both forms of the reference; exactly one is non-null)
        entry = lib.fmpnp_feature_pnp_query_layers
        ref_args = ((*ref_map, None, 0, r.shape[1], r.shape[2], 0) if reference_layers is None
                    else (None, 0, hc_layers, len(keep), H_ref, W_ref, ref_flags))
    elif reference_layers is None:
        entry, ref_args = lib.fmpnp_feature_pnp, (*ref_map, r.shape[0], r.shape[1], r.shape[2])
    else:
        entry, ref_args = lib.fmpnp_feature_pnp_layers, (hc_layers, len(keep), H_ref, W_ref, ref_flags)
    args = (*query_args, *ref_args, inl.ctypes.data, pts.ctypes.data, pts.shape[0],
            Kn.ctypes.data_as(_DP), R0.ctypes.data_as(_DP), t0.ctypes.data_as(_DP), int(image_shape[0]),
            int(image_shape[1]), lv, n_lv, ctypes.byref(opts), int(window), res.ctypes.data, tr,
            stride if want_trace else 0)
    if dev.index == torch.cuda.current_device():
        rc = entry(*args, _lib.stream_ptr(dev))
    else:
        with torch.cuda.device(dev):
            rc = entry(*args, _lib.stream_ptr(dev))
    if rc == _lib.ERANGE:
        raise IndexError("a reference inlier maps outside the reference hypercolumn "
                         "(optimize_feature_pnp.py:56 raises IndexError)")
    _lib.check(rc, "fmpnp_feature_pnp")
    out = _rf.results_from_array(res)
    if any(x["status"] & _lib.STATUS_SYNC_TIMEOUT for x in out):
        raise _lib.FmpnpError("cross-workgroup exchange timed out (device oversubscribed?)")

    def trace_of(i, n_evals):
        return _rf._trace_dict(tr[i * stride:(i + 1) * stride], n_evals) if want_trace else None
    return _apply_one_call_results(model, out, n_lv, R0, t0, pts, Kn, image_shape, track, trace_of)


def _apply_one_call_results(model, out, n_lv, R0, t0, pts, Kn, image_shape, track, trace_of):
    """The result records of one query's one-call refinement (fmpnp_feature_pnp's layout: [forward], or
    [compute_cost, forward per level]) -> (R, t, model), the model's attributes set as the reference sets them.
    trace_of(i, n_evals): forward i's trace dict, or None."""
    W_img, H_img = image_shape[0], image_shape[1]
    if not n_lv:                                                                            # :64-65
        R, t = model._apply_result(out[0], trace_of(0, out[0]["n_evals"]), pts, Kn, W_img, H_img, track)
        return R, t, model
    # multilevel_optimization (model.py:178-213): initial_cost_ from compute_cost; no support -> the
    # initial pose, unrefined (:183-187); else each level's forward from the previous level's pose
    cost = out[0]
    if cost["status"] & _lib.STATUS_NO_SUPPORT:
        model.initial_cost_ = None
        return torch.from_numpy(R0.copy()), torch.from_numpy(t0.copy()), model
    model.initial_cost_ = torch.tensor(cost["initial_cost"], dtype=torch.float64)
    for li in range(n_lv):
        R, t = model._apply_result(out[1 + li], trace_of(li, out[1 + li]["n_evals"]), pts, Kn, W_img, H_img, track)
    return R, t, model


def optimize_feature_pnp(query_hypercolumns, net, prediction, K, image_shape=None, track=False, feature_pyramid=None,
                         features="s2dhm", model=None, verbose=True, sparse_reference=False, query_layers=None):
    """optimize_feature_pnp.py:73-91.  Returns (list t, list quaternion, model).  Prints the reference's
    "Initial : ..." / "Final : ..." lines (:76, :90) unless verbose=False (the reference always prints
    them; a consumer that scrapes stdout sees the same lines).

    sparse_reference=True: net.compute_feature_maps (HypercolumnExtractor's; a net without it is a TypeError)
    gives the reference image's layers and feature_pnp forms the reference descriptors straight from them
    (reference_layers): the reference's dense hypercolumn is never assembled, the results are the same bits.

    query_layers: the query image's encoder maps (net.compute_feature_maps' list) in place of
    query_hypercolumns, which must then be None: feature_pnp packs them without assembling the dense query map.
    With sparse_reference=True no dense hypercolumn exists on either side.

    features="d2-net": `net` is a fmpnp.DenseFeatureExtractor (anything that offers compute_hypercolumn with
    HypercolumnExtractor's signature; a TypeError otherwise), whose dense map of the reference image takes the
    hypercolumn's place, as the reference's extract_dense_features does (:78-80); everything behind it is the
    's2dhm' branch.  query_hypercolumns is then the query's d2-net map.  sparse_reference=True and query_layers are
    ValueErrors with it: a d2-net map has no layers to take descriptors from."""
    cfg = config.adapter_kwargs()
    image_shape = image_shape if image_shape is not None else cfg.get("image_shape", (1024, 1024))
    if feature_pyramid is None:
        feature_pyramid = cfg.get("feature_pyramid")
    K = torch.from_numpy(np.asarray(K, dtype=np.float64))
    if verbose:
        print("Initial : {}".format(list(prediction.quaternion) + list(prediction.matrix[:3, 3])))
    if features == "d2-net":
        # (optimize_feature_pnp.py:78-84: the reference map from extract_dense_features, then the same feature_pnp)
        if sparse_reference or query_layers is not None:
            raise ValueError('features="d2-net" has one dense map and no layers to take descriptors from: '
                             "sparse_reference and query_layers need features=\"s2dhm\"")
        if not callable(getattr(net, "compute_hypercolumn", None)):
            raise TypeError('features="d2-net" needs a net with compute_hypercolumn (fmpnp.DenseFeatureExtractor)')
    if sparse_reference:
        if not callable(getattr(net, "compute_feature_maps", None)):
            raise TypeError("sparse_reference=True needs a net with compute_feature_maps (HypercolumnExtractor)")
        reference_layers, _ = net.compute_feature_maps([prediction.reference_filename], resize=True)
        R, t, model = feature_pnp(query_hypercolumns, None, prediction, K, image_shape, track=track,
                                  feature_pyramid=feature_pyramid, model=model, reference_layers=reference_layers,
                                  query_layers=query_layers)
    else:
        reference_hypercolumns, _ = net.compute_hypercolumn([prediction.reference_filename], to_cpu=False,
                                                            resize=True)
        R, t, model = feature_pnp(query_hypercolumns, reference_hypercolumns, prediction, K, image_shape,
                                  track=track, feature_pyramid=feature_pyramid, model=model, query_layers=query_layers)
    T = np.eye(4)
    T[:3, :3], T[3, :3] = R.numpy(), t.numpy()  # the reference writes t into the bottom row (:87)
    quaternion = matrix_quaternion(T)
    if verbose:
        print("Final : {}".format(list(quaternion) + list(t.numpy())))
    return list(t.numpy()), list(quaternion), model


class DirectPoseModel:
    """The call surface named by the build's north star: `.optimize_feature_pnp()` with the
    reference adapter's arguments, backed by the HIP refiner."""

    def __init__(self, **model_kwargs):
        self.model_kwargs = model_kwargs

    def make_model(self):
        kw = dict(config.model_kwargs())
        kw.update(self.model_kwargs)
        return sparseFeaturePnP(**kw)

    def feature_pnp_multi(self, query_hypercolumns, reference_hypercolumns, prediction, K, image_shape,
                          track=False):
        return feature_pnp_multi(query_hypercolumns, reference_hypercolumns, prediction, K, image_shape, track,
                                 model=self.make_model())

    def feature_pnp(self, query_hypercolumns, reference_hypercolumns, prediction, K, image_shape, track=False,
                    feature_pyramid=None):
        return feature_pnp(query_hypercolumns, reference_hypercolumns, prediction, K, image_shape, track,
                           feature_pyramid, model=self.make_model())

    def optimize_feature_pnp(self, query_hypercolumns, net, prediction, K, image_shape=None, track=False,
                             feature_pyramid=None, features="s2dhm"):
        return optimize_feature_pnp(query_hypercolumns, net, prediction, K, image_shape, track, feature_pyramid,
                                    features, model=self.make_model())
