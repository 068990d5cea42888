"""The localisation chain without a GPU: fmpnp.localize_cpu against the staged yardstick built from the CPU
twins that existed before it (exhaustive_match_cpu, solve_pnp_cpu), the two glue twins called directly on
hand-made arrays against a numpy restatement, and the host validation of the C entry points.
Scenes and yardstick: tests/localize_cases.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import localize_cases as lc
import fmpnp
from fmpnp import _lib
from fmpnp import _localize as loc  # (the module: fmpnp.localize is the function)
from fmpnp.match import exhaustive_match_cpu, nearest_cells, points_in_query_space
from fmpnp.pnp import solve_pnp_cpu

FILL = 0xA5


def host_sparse(ref):
    if "sparse_descriptors" in ref:
        return ref["sparse_descriptors"]
    hc = ref["hypercolumn"]
    cells = nearest_cells(ref["points_2D"], lc.W, lc.H, lc.IMAGE[0] / lc.W, lc.IMAGE[1] / lc.H)
    return np.ascontiguousarray(hc.reshape(lc.C, -1)[:, cells].T)


@functools.lru_cache(maxsize=None)
def cpu_yardstick(name, return_masked=True):
    sc = lc.scene(name)
    refs = sc["references"]
    rows = np.concatenate([host_sparse(r) for r in refs], 0)
    res = exhaustive_match_cpu(rows, sc["query"].reshape(lc.C, -1), int(lc.FACTOR * lc.W * lc.H))
    matches, at = [], 0
    for r in refs:
        n = r["points_2D"].shape[0]
        pts = points_in_query_space(res["argmax"][at:at + n], lc.IMAGE, lc.W, lc.H)
        matches.append((pts.cpu().numpy(), res["mask"][at:at + n]))
        at += n

    def solve(points_2D, points_3D, ref, ref_2D):
        return solve_pnp_cpu(points_2D, points_3D, ref["intrinsics"], ref["distortion_coefficients"],
                             reference_filename=ref["filename"], reference_2D_points=ref_2D, reference_keypoints=None,
                             return_masked=return_masked, **lc.PNP)
    return lc.staged(refs, matches, solve)


@functools.lru_cache(maxsize=None)
def chain_cpu(name, return_masked=True):
    sc = lc.scene(name)
    return fmpnp.localize_cpu(sc["query"], [lc.public(r) for r in sc["references"]], lc.IMAGE, factor=lc.FACTOR,
                              return_masked=return_masked, return_all=True, fill=FILL, **lc.PNP)


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("name", sorted(lc.SCENES))
def test_localize_cpu_equals_the_staged_twins(name, masked):
    every, eligible, arrays = cpu_yardstick(name, masked)
    got = chain_cpu(name, masked)
    export, best = lc.choose([p for _, p in eligible])
    lc.equal(got.export, export, "export")
    lc.equal_prediction(got.prediction, best, "best")
    assert got.kind == ("none" if best is None else "fallback" if best.inlier_mask is None else "solved")
    if best is not None:
        assert got.best == [j for j, p in eligible if p is best][0]
        assert got.prediction.query_inliers.dtype == np.float32 and got.prediction.points_3d.shape[1:] == (1, 3)
        if got.kind == "solved":
            assert got.prediction.inlier_mask.dtype == np.int32
    for j, (pred, (p2, r2, p3)) in enumerate(zip(every, arrays)):
        lc.equal_prediction(got.predictions[j], pred, f"pair {j}")
        e = got.cached_matches[j]
        lc.equal(e["query_2D"], p2, "query_2D")
        lc.equal(e["reference_2D"], r2, "reference_2D")
        lc.equal(e["points_3D"], p3, "points_3D")


def test_the_scenes_reach_every_branch():
    """Asserted on the yardstick's outputs: a scene that drifts off its branch fails here."""
    mm = lc.PNP["minimum_matches"]
    reached = {name: lc.branches(lc.scene(name)["references"], *cpu_yardstick(name), mm) for name in lc.SCENES}
    assert {"mask_all_zero", "count_le_minimum_matches", "too_few_inliers_absent", "solved"} <= reached["mixed"]
    assert "tie_earlier_wins" in reached["tie"]
    assert {"too_few_inliers_with_fallback", "solved"} <= reached["fallback_loses"]
    assert "fallback_wins" in reached["fallback_wins"]
    assert "none" in reached["none"]
    # the tie: both equal pairs solve with the same count and the earlier is the best
    got = chain_cpu("tie")
    assert got.best == 1 and got.predictions[1].num_inliers == got.predictions[2].num_inliers > 256
    # the row counts of the compaction
    assert tuple(r["points_2D"].shape[0] for r in lc.scene("mixed")["references"][:6]) == lc.ROW_COUNTS
    # the last reference's intrinsics differ from the best one's (refine_intrinsics "last" against "best")
    refs = lc.scene("fallback_loses")["references"]
    best = chain_cpu("fallback_loses").best
    assert not np.array_equal(refs[-1]["intrinsics"], refs[best]["intrinsics"])


# ---- the glue twins alone, on hand-made arrays ---------------------------------------------------------

def hand_made(seed=7, fallback=(False,) * 6):
    """One query of six pairs with the row counts of the compaction; random argmax / mask / points."""
    rng = np.random.Generator(np.random.PCG64(seed))
    refs = []
    for j, n in enumerate(lc.ROW_COUNTS):
        ref = dict(points_2D=rng.uniform(0, 64, (n, 2)), points_3D=rng.normal(0, 1, (n, 3)), intrinsics=lc.K0 + j,
                   distortion_coefficients=np.array([0.1, 0.2, 0.3, 0.4]) * (j + 1), image_resolution=lc.IMAGE,
                   filename=f"r{j}")
        if fallback[j]:
            m = np.eye(4)
            m[:3, :] = rng.normal(0, 1, (3, 4))
            ref["fallback_pose"] = (np.arange(4.0), m)
        refs.append(ref)
    params = loc._pnp_params(12.0, 70, 5, True, 256, 99)
    plan = loc._Plan([(torch.zeros(lc.C, lc.W, lc.H), refs)], lc.IMAGE, lc.FACTOR, params)
    for g in range(plan.n_pairs):
        plan.pairs[g].points3d, plan.pairs[g].points2d = plan.p3[g].ctypes.data, plan.p2[g].ctypes.data
    T = plan.total_rows
    argmax = rng.integers(0, lc.W * lc.H, T).astype(np.int32)
    mask = (rng.uniform(0, 1, T) < 0.6).astype(np.uint8) * rng.integers(1, 256, T).astype(np.uint8)  # any non-zero byte
    lay, n_out = loc._layout(sum(plan.sections(True), []))
    bufs = loc._views(np.full(n_out, FILL, np.uint8), lay)
    return plan, refs, argmax, mask, bufs


def test_build_twin_against_numpy():
    plan, refs, argmax, mask, bufs = hand_made()
    probs = loc.glue_build_cpu(plan, argmax, mask, bufs)
    for g, ref in enumerate(refs):
        off, n = plan.pairs[g].row_offset, plan.pairs[g].n_rows
        sel = np.flatnonzero(mask[off:off + n])                                            # the restatement:
        q = points_in_query_space(argmax[off:off + n][sel], lc.IMAGE, lc.W, lc.H).numpy()  # three lines of numpy
        want = dict(m_q32=q, m_q64=q.astype(np.float64), m_x3=ref["points_3D"][sel], m_r2=ref["points_2D"][sel],
                    m_src=sel.astype(np.int32))
        cnt = len(sel)
        assert bufs["counts"][g] == cnt
        for k, w in want.items():
            width = w.shape[1] if w.ndim == 2 else 1
            got = bufs[k].reshape(-1, width)[off:off + n]
            assert got.dtype == w.dtype and got[:cnt].tobytes() == np.ascontiguousarray(w).tobytes(), (g, k)
            assert (got[cnt:].view(np.uint8) == FILL).all(), (g, k)   # rows past the count are not written
        p = probs[g]
        assert p.M == (cnt if cnt > 70 else 0) and p.iters == 256 and p.n_dist == 4 and p.seed == 99
        assert p.threshold == 12.0 and p.mask_offset == off and p.reserved == 0
        assert p.points3d == bufs["m_x3"].ctypes.data + 24 * off and p.points2d == bufs["m_q64"].ctypes.data + 16 * off
        assert list(p.K) == list((lc.K0 + g).reshape(-1)) and list(p.dist) == list(np.array([0.1, 0.2, 0.3, 0.4]) * (g + 1))
    assert {int(probs[g].M > 0) for g in range(6)} == {0, 1}  # both sides of minimum_matches


@pytest.mark.parametrize("mode", ["solved_masked", "solved_all", "fallback", "none", "tie"])
def test_pick_twin_against_numpy(mode):
    fb = (False, True, True, False, False, False) if mode == "fallback" else (False,) * 6
    plan, refs, argmax, mask, bufs = hand_made(8, fb)
    plan.params.return_masked = 0 if mode == "solved_all" else 1
    loc.glue_build_cpu(plan, argmax, mask, bufs)
    rng = np.random.Generator(np.random.PCG64(9))
    results = (_lib.PnpResult * 6).from_buffer(bufs["results"])
    pm = bufs["pnp_mask"]
    # hand-made PnP results: pair 5 (1000 rows) solves with many inliers, pair 4 with fewer, pair 3 below minimum_inliers
    inliers = {5: 300, 4: 100, 3: 4} if mode != "tie" else {5: 100, 4: 100, 3: 4}
    for g in range(6):
        off, cnt = plan.pairs[g].row_offset, int(bufs["counts"][g])
        if mode in ("fallback", "none") or g not in inliers:
            results[g].status = _lib.PNP_TOO_FEW if g < 3 else _lib.PNP_NO_MODEL  # (the other fields keep the fill)
            continue
        chosen = np.sort(rng.permutation(cnt)[:inliers[g]])
        pm[off:off + cnt] = 0
        pm[off + chosen] = 1
        r = results[g]
        r.status, r.num_inliers = _lib.PNP_OK, inliers[g]
        r.R[:], r.t[:] = rng.normal(0, 1, 9).tolist(), rng.normal(0, 1, 3).tolist()
    loc.glue_pick_cpu(plan, results, pm, bufs)
    rec = _lib.LocRecord.from_buffer_copy(bufs["records"].tobytes())
    want_best = {"solved_masked": 5, "solved_all": 5, "fallback": 1, "none": -1, "tie": 4}[mode]
    assert rec.best == want_best and rec.reserved == 0
    out = {k: bufs[k].reshape(-1, w) for k, w in (("b_pts3d", 3), ("b_ref2d", 2), ("b_q32", 2), ("b_idx", 1))}
    if mode == "none":
        assert rec.kind == _lib.LOC_NONE and rec.N == rec.num_matches == rec.num_inliers == 0
        assert not any(rec.R0) and not any(rec.t0)
        assert all((v.view(np.uint8) == FILL).all() for v in out.values())  # nothing else is written
        return
    off, cnt = plan.pairs[want_best].row_offset, int(bufs["counts"][want_best])
    if mode == "fallback":
        rows, inl = np.arange(cnt), np.arange(0)
        assert rec.kind == _lib.LOC_FALLBACK and rec.num_inliers == 0
        m = refs[1]["fallback_pose"][1]
        assert list(rec.R0) == list(m[:3, :3].reshape(-1)) and list(rec.t0) == list(m[:3, 3])
    else:
        inl = np.flatnonzero(pm[off:off + cnt])                                       # the restatement:
        rows = inl if plan.params.return_masked else np.arange(cnt)                   # three lines of numpy
        assert rec.kind == _lib.LOC_SOLVED and rec.num_inliers == len(inl) == inliers[want_best]
        assert list(rec.R0) == list(results[want_best].R) and list(rec.t0) == list(results[want_best].t)
    assert rec.N == len(rows) and rec.num_matches == cnt
    want = dict(b_pts3d=bufs["m_x3"].reshape(-1, 3)[off:off + cnt][rows], b_ref2d=bufs["m_r2"].reshape(-1, 2)[off:off + cnt][rows],
                b_q32=bufs["m_q32"].reshape(-1, 2)[off:off + cnt][rows], b_idx=inl.astype(np.int32).reshape(-1, 1))
    for k, w in want.items():
        assert out[k].dtype == w.dtype and out[k][:len(w)].tobytes() == np.ascontiguousarray(w).tobytes(), k
        assert (out[k][len(w):].view(np.uint8) == FILL).all(), k


def test_result_does_not_depend_on_the_fill():
    sc = lc.scene("fallback_loses")
    refs = [lc.public(r) for r in sc["references"]]
    a = fmpnp.localize_cpu(sc["query"], refs, lc.IMAGE, factor=lc.FACTOR, return_masked=True, return_all=True, fill=0,
                           **lc.PNP)
    b = chain_cpu("fallback_loses")
    lc.equal_prediction(a.prediction, b.prediction)
    for x, y in zip(a.predictions, b.predictions):
        lc.equal_prediction(x, y)


# ---- host validation -------------------------------------------------------------------------------

def test_host_validation():
    L = _lib.load()
    plan, refs, argmax, mask, bufs = hand_made()
    m = _lib.LocMatches(*[bufs[k].ctypes.data for k in ("m_q32", "m_q64", "m_x3", "m_r2", "m_src", "counts")])
    b = _lib.LocBest(*[bufs[k].ctypes.data for k in ("b_pts3d", "b_ref2d", "b_q32", "b_idx", "records")])
    probs = (_lib.PnpProblem * 6)()
    prm, T = ctypes.byref(plan.params), plan.total_rows
    build = lambda pairs=plan.pairs, n=6, p=prm, a=argmax.ctypes.data, k=mask.ctypes.data, t=T, mm=ctypes.byref(m), \
        pr=probs: L.fmpnp_localize_build_cpu(pairs, n, p, a, k, t, mm, pr)  # noqa: E731
    assert build() == 0
    assert build(pairs=None) == _lib.EINVAL and build(p=None) == _lib.EINVAL and build(a=None) == _lib.EINVAL
    assert build(k=None) == _lib.EINVAL and build(mm=None) == _lib.EINVAL and build(pr=None) == _lib.EINVAL
    assert build(n=-1) == _lib.EINVAL and build(t=-1) == _lib.EINVAL and build(t=T - 1) == _lib.EINVAL
    assert build(n=65536) == _lib.ETOOBIG
    m_bad = _lib.LocMatches.from_buffer_copy(m)
    m_bad.src_row = None
    assert build(mm=ctypes.byref(m_bad)) == _lib.EINVAL
    results, pm = (_lib.PnpResult * 6)(), np.zeros(T, np.uint8)
    pick = lambda q=plan.qdesc, nq=1, r=results, k=pm.ctypes.data, bb=ctypes.byref(b), n=6: \
        L.fmpnp_localize_pick_cpu(plan.pairs, n, q, nq, prm, r, k, T, ctypes.byref(m), bb)  # noqa: E731
    assert pick() == 0
    assert pick(q=None) == _lib.EINVAL and pick(r=None) == _lib.EINVAL and pick(k=None) == _lib.EINVAL
    assert pick(bb=None) == _lib.EINVAL and pick(nq=-1) == _lib.EINVAL and pick(n=65536) == _lib.ETOOBIG
    small = (_lib.LocQuery * 1).from_buffer_copy(plan.qdesc)
    small[0].out_cap = 999  # below the largest n_rows
    assert pick(q=small) == _lib.EINVAL
    # the HIP entry point validates on the host before it touches the device: fake device addresses suffice
    dev, ws_bytes = 0x10000, L.fmpnp_localize_workspace_size(6)
    assert ws_bytes >= 6 * ctypes.sizeof(_lib.PnpProblem) + L.fmpnp_pnp_workspace_size(6)
    call = lambda pairs=plan.pairs, n=6, ws=dev, wsb=ws_bytes, pd=dev, res=dev, a=dev, t=T: L.fmpnp_localize_async(  # noqa: E731
        pd, pairs, n, dev, plan.qdesc, 1, prm, a, dev, t, ctypes.byref(m), ctypes.byref(b), res, dev, ws, wsb, None)
    assert call(ws=dev + 4) == _lib.EINVAL and call(ws=None) == _lib.EINVAL and call(wsb=ws_bytes - 1) == _lib.EINVAL
    assert call(pairs=None) == _lib.EINVAL and call(pd=None) == _lib.EINVAL and call(res=None) == _lib.EINVAL
    assert call(a=None) == _lib.EINVAL and call(n=-1) == _lib.EINVAL and call(t=-5) == _lib.EINVAL
    assert call(n=65536) == _lib.ETOOBIG
    # ... and so does the synchronous form
    src = (_lib.LocSource * 6)()
    for g in range(6):
        src[g].sparse, src[g].ld_sparse = dev, lc.C
    dense, top_k = (ctypes.c_void_p * 1)(dev), (ctypes.c_int * 1)(2)
    sync = lambda pairs=plan.pairs, sources=src, n=6, c=lc.C, bb=ctypes.byref(b), qd=dense, tk=top_k, t=T: \
        L.fmpnp_localize(pairs, sources, n, plan.qdesc, qd, tk, 1, c, 0.9, prm, t, bb, None, None, None, None)  # noqa: E731
    assert sync(pairs=None) == _lib.EINVAL and sync(sources=None) == _lib.EINVAL and sync(c=0) == _lib.EINVAL
    assert sync(bb=None) == _lib.EINVAL and sync(qd=None) == _lib.EINVAL and sync(tk=None) == _lib.EINVAL
    assert sync(n=-1) == _lib.EINVAL and sync(t=-1) == _lib.EINVAL and sync(n=65536) == _lib.ETOOBIG
    narrow = (_lib.LocSource * 6).from_buffer_copy(src)
    narrow[3].ld_sparse = lc.C - 1
    assert sync(sources=narrow) == _lib.EINVAL
    narrow[3].ld_sparse, narrow[3].sparse = lc.C, None
    assert sync(sources=narrow) == _lib.EINVAL
    with pytest.raises(_lib.FmpnpError, match="ETOOBIG"):
        loc._Plan([(torch.zeros(lc.C, lc.W, lc.H), [refs[0]] * 65536)], lc.IMAGE, lc.FACTOR, plan.params)


def test_exports_and_abi():
    assert {"fmpnp_localize_workspace_size", "fmpnp_localize_async", "fmpnp_localize", "fmpnp_localize_build_cpu",
            "fmpnp_localize_pick_cpu"} <= set(_lib.EXPORTS)
    assert _lib.load().fmpnp_abi_version() == 4
    with pytest.raises(ValueError):
        fmpnp.localize_cpu(lc.scene("none")["query"], [], lc.IMAGE, factor=lc.FACTOR, refine=True, return_masked=True,
                           **lc.PNP)
