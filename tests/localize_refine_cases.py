"""Shared pieces of the batched refinement stage's tests (test_localize_refine_cpu.py, test_gpu_localize_refine.py):
the pick step's outputs of several scenes in one plan, built from fmpnp.localize_cpu's results, and the numpy
restatement of the stage's prep and gather steps (include/fmpnp.h, "batched refinement of the chain's winners").
Scenes: tests/localize_cases.py."""
import ctypes
import functools

import numpy as np
import torch

import localize_cases as lc
import fmpnp
from fmpnp import _lib
from fmpnp import _localize as loc

FILL = 0xA5
NAMES = ("mixed", "tie", "fallback_loses", "fallback_wins", "none")
LEVELS = [(16, 32, None, None), (0, 16, None, None)]
KIND = {"none": _lib.LOC_NONE, "solved": _lib.LOC_SOLVED, "fallback": _lib.LOC_FALLBACK}


@functools.lru_cache(maxsize=None)
def cpu_localization(name, return_masked=True):
    sc = lc.scene(name)
    return fmpnp.localize_cpu(sc["query"], [lc.public(r) for r in sc["references"]], lc.IMAGE, factor=lc.FACTOR,
                              return_masked=return_masked, **lc.PNP)


def picked(names=NAMES, return_masked=True):
    """(plan, bufs, localizations): one plan over the scenes, its output sections filled with FILL and then with
    what the pick step leaves for each query -- the record and the N compacted rows -- taken from localize_cpu."""
    scenes = [lc.scene(n) for n in names]
    params = loc._pnp_params(return_masked=return_masked, **lc.PNP)
    plan = loc._Plan([(torch.from_numpy(s["query"]), [lc.public(r) for r in s["references"]]) for s in scenes], lc.IMAGE,
                     lc.FACTOR, params)
    for g in range(plan.n_pairs):
        plan.pairs[g].points3d, plan.pairs[g].points2d = plan.p3[g].ctypes.data or None, plan.p2[g].ctypes.data or None
    lay, n_out = loc._layout(sum(plan.sections(True), []))
    bufs = loc._views(np.full(n_out, FILL, np.uint8), lay)
    recs = (_lib.LocRecord * plan.n_queries).from_buffer(bufs["records"])
    locs = [cpu_localization(n, return_masked) for n in names]
    for qi, got in enumerate(locs):
        rec, o = recs[qi], plan.qdesc[qi].out_offset
        ctypes.memset(ctypes.addressof(rec), 0, ctypes.sizeof(rec))
        rec.kind, rec.best = KIND[got.kind], -1 if got.best is None else got.best
        if got.prediction is None:
            continue
        p = got.prediction
        m = np.asarray(p.matrix, np.float64)
        rec.R0[:], rec.t0[:] = m[:3, :3].reshape(-1).tolist(), m[:3, 3].tolist()
        x3 = np.asarray(p.points_3d, np.float64).reshape(-1, 3)
        r2 = np.asarray(p.reference_inliers, np.float64).reshape(-1, 2)
        rec.N, rec.num_matches, rec.num_inliers = len(x3), p.num_matches, p.num_inliers
        bufs["b_pts3d"].reshape(-1, 3)[o:o + len(x3)] = x3
        bufs["b_ref2d"].reshape(-1, 2)[o:o + len(r2)] = r2
    return plan, bufs, locs


def host_sources(plan, dtype=np.float32, drop=()):
    """(LocRefineSource array over the references' HOST maps, the maps): pairs in drop get a NULL source."""
    src, maps, g = (_lib.LocRefineSource * max(plan.n_pairs, 1))(), [], 0
    for refs in plan.refs:
        for ref in refs:
            m = ref["hypercolumn"]
            m = np.ascontiguousarray(m.cpu().numpy() if torch.is_tensor(m) else m, dtype=dtype)
            maps.append(m)
            if g not in drop:
                src[g].ref_chw, src[g].dtype = m.ctypes.data, _lib.F64 if dtype == np.float64 else _lib.F32
                src[g].H_ref, src[g].W_ref = m.shape[1], m.shape[2]
            g += 1
    return src, maps


def refine_params(cstride=None, levels=(), intrinsics=_lib.LOC_K_LAST):
    lv = (_lib.Level * max(len(levels), 1))(*[_lib.Level(a, b) for a, b in levels])
    p = _lib.LocRefineParams(lc.C, cstride or lc.C, lc.IMAGE[0], lc.IMAGE[1], intrinsics, len(levels), lv)
    p._keep = lv
    return p


def query_maps(plan, feat=0x1000):
    maps = (_lib.LocRefineMap * max(plan.n_queries, 1))()
    for qi in range(plan.n_queries):
        maps[qi].feat, maps[qi].Hf, maps[qi].Wf = feat + 0x100000 * qi, plan.dims[qi][1], plan.dims[qi][2]
    return maps


def reference_rows(ref_map, ref2d):
    """The numpy restatement of the gather: (rows [n, C] as float64, bad [n]) under fmpnp_gather_reference's
    convention -- col = trunc(x H_ref / img0), row = trunc(y W_ref / img1), python's negative wrap."""
    C, H, W = ref_map.shape
    colf, rowf = (H / lc.IMAGE[0]) * ref2d[:, 0], (W / lc.IMAGE[1]) * ref2d[:, 1]
    finite = np.isfinite(colf) & np.isfinite(rowf)
    col, row = np.trunc(np.where(finite, colf, 0)).astype(np.int64), np.trunc(np.where(finite, rowf, 0)).astype(np.int64)
    row, col = np.where((row < 0) & (row >= -H), row + H, row), np.where((col < 0) & (col >= -W), col + W, col)
    bad = ~finite | (row < 0) | (row >= H) | (col < 0) | (col >= W)
    rows = ref_map[:, np.where(bad, 0, row), np.where(bad, 0, col)].T.astype(np.float64)
    rows[bad] = 0.0
    return rows, bad
