"""The SuperPoint baseline's CPU twins (fmpnp_sp_*_cpu through fmpnp.superpoint with cpu=True) against the
goldens recorded from the reference's own SuperPointFrontend.run, fast_keypoint_matching, fast_closest_points
and _assemble_matches (tests/golden/gen_golden_superpoint.py).  The generator chose seeds at which the
reference's sorts and fp32 exp cannot break a tie either way, so keypoints, matches, argmins and assembled
arrays are compared exactly; the heatmap and the descriptors are held to 4 x the reference's own fp32 error
against the fp64 restatement."""
import ctypes

import numpy as np
import pytest
import torch

import superpoint_cases as sc
import fmpnp
from fmpnp import _lib
from fmpnp import superpoint as sp

DET = ("main", "dense", "border")
FILL = 0xA5


def detect(name, align_corners=False):
    g = sc.golden(f"det_{name}")
    H, W, _, d, conf, _, _ = sc.DETECTOR[name]
    return g, sp.superpoint_postprocess(g["semi"], g["coarse"], (H, W), d, conf, align_corners, cpu=True)


def test_golden_inputs_are_the_seeded_ones():
    for name in sc.DETECTOR:
        g = sc.golden(f"det_{name}")
        semi, coarse = sc.detector_inputs(name, int(g["seed"]))
        assert np.array_equal(semi, g["semi"]) and np.array_equal(coarse, g["coarse"])


@pytest.mark.parametrize("name", DET)
def test_keypoints_equal_the_reference(name):
    g, (pts, desc, heat) = detect(name)
    assert pts.dtype == np.float64 and pts.shape == g["pts"].shape, (pts.shape, g["pts"].shape)
    assert np.array_equal(pts[:2], g["pts"][:2])  # x, y, order and count
    assert np.all(np.diff(pts[2]) < 0)
    # the confidence is the twin's own heat value at that pixel
    assert np.array_equal(pts[2], heat[pts[1].astype(int), pts[0].astype(int)].astype(np.float64))


@pytest.mark.parametrize("name", DET)
def test_heatmap_and_descriptors_within_the_reference_error(name):
    g, (pts, desc, heat) = detect(name)
    assert heat.dtype == np.float32 and desc.dtype == np.float32 and desc.shape == g["desc"].shape
    e_heat, e_desc = np.abs(heat - g["heat64"]).max(), np.abs(desc - g["desc64"]).max()
    print(f"{name}: heat error {e_heat:.3e} (e_ref {float(g['e_ref_heat']):.3e}), descriptor error {e_desc:.3e} "
          f"(e_ref {float(g['e_ref_desc']):.3e})")
    assert e_heat <= 4 * float(g["e_ref_heat"])
    assert e_desc <= 4 * float(g["e_ref_desc"])


def test_no_candidate():
    g, (pts, desc, heat) = detect("none")
    assert pts.shape == (3, 0) and pts.dtype == np.float64 and desc is None and heat is None


def test_border_point_suppresses_then_leaves():
    g, (pts, _, heat) = detect("border")
    got = {(int(x), int(y)) for x, y in pts[:2].T}
    assert heat[20, 2] > heat[22, 5] >= np.float32(0.015)  # both are candidates, the border one the stronger
    assert (2, 20) not in got and (5, 22) not in got and (30, 30) in got
    assert pts[0].min() >= 4 and pts[0].max() < 64 - 4 and pts[1].min() >= 4 and pts[1].max() < 48 - 4


def test_chains_longer_than_a_window():
    for name in ("main", "dense"):
        g, (pts, _, _) = detect(name)
        got = {(int(x), int(y)) for x, y in pts[:2].T}
        chain = [(x, y) for x, y, _ in sc.DETECTOR[name][6][:9]]
        kept = [p in got for p in chain]
        # each kept peak frees the one after the peak it suppresses: six links span more than one window
        assert kept[:6] == [True, False] * 3, kept
        want = {(int(x), int(y)) for x, y in g["pts"][:2].T}
        assert kept == [p in want for p in chain]


@pytest.mark.parametrize("name", DET)
@pytest.mark.parametrize("align_corners", (False, True))
def test_sampling_against_grid_sample(name, align_corners):
    """The un-normalised samples against torch.nn.functional.grid_sample on the CPU.  Both form four products of
    a weight (two fp32 differences and a product: relative error <= 3 u, u = 2^-24) with a tap and add them:
    |error| <= (4 * (3 + 1) + 3) u * max |tap| per implementation, twice that between the two; the unit
    descriptors' taps are below 1 and the division by the norm (>= 0.3 here) amplifies by its inverse."""
    g, (pts, desc, _) = detect(name, align_corners)
    H, W = sc.DETECTOR[name][:2]
    grid = torch.from_numpy(pts[:2].copy())
    grid[0] = grid[0] / (float(W) / 2.) - 1.
    grid[1] = grid[1] / (float(H) / 2.) - 1.
    grid = grid.transpose(0, 1).contiguous().view(1, 1, -1, 2).float()
    ref = torch.nn.functional.grid_sample(torch.from_numpy(g["coarse"].copy())[None], grid, align_corners=align_corners)
    ref = ref.numpy().reshape(g["coarse"].shape[0], -1)
    norm = np.linalg.norm(ref, axis=0)
    assert norm.min() >= 0.3
    ref = ref / norm[None]
    bound = 2 * 19 * 2.0 ** -24 / 0.3 * 2  # (the factor 2: the norm's own error, relative, on values below 1)
    assert np.abs(desc - ref).max() <= bound, (np.abs(desc - ref).max(), bound)
    if not align_corners:
        assert np.abs(desc - g["desc"]).max() <= bound


@pytest.mark.parametrize("name", tuple(sc.MATCHING))
def test_matching_and_assembly_equal_the_reference(name):
    g = sc.golden("matching")
    seed = int(g[f"{name}.seed"])
    desc1, desc2 = sc.matching_inputs(name, seed)
    ratio = sc.MATCHING[name][3]
    out = sp.two_nearest(desc1, desc2, ratio, cpu=True)
    assert np.array_equal(out["idx"], g[f"{name}.nn_idx"])
    assert np.array_equal(out["ok"], g[f"{name}.ok"])
    assert out["matches"].dtype == np.int64 and np.array_equal(out["matches"], g[f"{name}.matches"])
    if sc.MATCHING[name][0] >= 63:
        assert out["ok"].any() and not out["ok"].all()
    assert np.array_equal(fmpnp.fast_keypoint_matching(desc1, desc2, ratio, cpu=True), g[f"{name}.matches"])
    # the distances are the fp32 chain's: within its summation error of the fp64 ones
    d64 = 2 * (1 - desc1.astype(np.float64) @ desc2.astype(np.float64).T)
    assert np.abs(out["dist"] - np.take_along_axis(d64, out["idx"].astype(np.int64), 1)).max() < 1e-5
    q_kp, r_kp, p2, p3 = sc.assembly_inputs(name, seed)
    argmins = fmpnp.fast_closest_points(r_kp[:2], p2, cpu=True)
    assert argmins.dtype == np.int64 and np.array_equal(argmins, g[f"{name}.argmins"])
    x2, r2, x3 = fmpnp.assemble_matches(q_kp, r_kp, p2, p3, out["matches"], cpu=True)
    for got, key in ((x2, "x2D"), (r2, "x2D_reference"), (x3, "x3D")):
        want = g[f"{name}.{key}"]
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), key
    if sc.MATCHING[name][0] >= 63:
        counts = np.bincount(out["matches"][:, 1], minlength=sc.MATCHING[name][1])
        assert counts.max() >= 2 and (counts == 0).any()  # a keypoint matched by several rows, one by none


def test_too_few_references_and_empty_queries():
    rng = np.random.default_rng(5)
    d1, d2 = rng.standard_normal((4, 16)).astype(np.float32), rng.standard_normal((1, 16)).astype(np.float32)
    with pytest.raises(_lib.FmpnpError, match="EINVAL"):
        sp.two_nearest(d1, d2, 0.9, cpu=True)  # topk(2) of one column raises in the reference
    out = sp.two_nearest(d1[:0], rng.standard_normal((5, 16)).astype(np.float32), 0.9, cpu=True)
    assert out["matches"].shape == (0, 2) and out["matches"].dtype == np.int64 and out["idx"].shape == (0, 2)
    x2, r2, x3 = fmpnp.assemble_matches(np.zeros((3, 0)), np.zeros((3, 7)), np.zeros((3, 2)), np.zeros((3, 3)),
                                        np.zeros((0, 2), np.int64), cpu=True)
    assert x2.shape == (0, 1, 2) and r2.shape == (0, 1, 2) and x3.shape == (0, 1, 3)


def test_outputs_untouched_past_the_counts():
    L = _lib.load()
    g = sc.golden("det_main")
    H, W, _, d, conf, _, _ = sc.DETECTOR["main"]
    heat = sp.heatmap(g["semi"], cpu=True)
    cap = int(L.fmpnp_sp_nms_capacity(H, W, d))
    assert cap == -(-H // (d + 1)) * -(-W // (d + 1))
    pts = np.full((3, cap + 3), np.nan)
    pts.view(np.uint8)[:] = FILL
    n = ctypes.c_int(-1)
    assert L.fmpnp_sp_nms_cpu(heat.ctypes.data, H, W, conf, d, 4, pts.ctypes.data, cap + 3, ctypes.byref(n)) == 0
    assert n.value == g["pts"].shape[1] and np.array_equal(pts[:2, :n.value], g["pts"][:2])
    assert (pts[:, n.value:].view(np.uint8) == FILL).all()


def test_argument_errors():
    L = _lib.load()
    a = 0x10000  # validation happens before any pointer is read
    n = ctypes.c_int(0)
    assert L.fmpnp_sp_heatmap_cpu(None, 2, 2, a) == _lib.EINVAL and L.fmpnp_sp_heatmap_cpu(a, -1, 2, a) == _lib.EINVAL
    assert L.fmpnp_sp_nms_cpu(a, 64, 96, 0.015, 17, 4, a, 10 ** 6, ctypes.byref(n)) == _lib.ETOOBIG
    assert L.fmpnp_sp_nms_cpu(a, 64, 96, 0.015, 4, 4, a, 5, ctypes.byref(n)) == _lib.EINVAL  # ld_pts below the capacity
    assert L.fmpnp_sp_nms_cpu(a, 64, 96, float("nan"), 4, 4, a, 10 ** 6, ctypes.byref(n)) == _lib.EINVAL
    assert L.fmpnp_sp_describe_cpu(a, 8, 4, 4, a, 3, 3, 32, 32, 2, a, 3) == _lib.EINVAL
    assert L.fmpnp_sp_match_cpu(a, 4, 8, a, 8, 1, 1, 0.9, a, a, a, a, ctypes.byref(n)) == _lib.EINVAL
    assert L.fmpnp_sp_assemble_cpu(a, 2, 2, a, 2, 2, a, a, 0, a, 0, a, a, a, a, ctypes.byref(n)) == _lib.EINVAL
    # the HIP entry points validate on the host before they touch the device
    assert L.fmpnp_sp_heatmap_async(None, 2, 2, a, None) == _lib.EINVAL
    assert L.fmpnp_sp_match_async(a, 4, 8, a, 8, 1, 1, 0.9, a, a, a, a, a, a, 1 << 20, None) == _lib.EINVAL
    assert L.fmpnp_sp_match(a, 4, 8, a, 8, 1, 1, 0.9, a, a, a, a, ctypes.byref(n), None) == _lib.EINVAL
    assert L.fmpnp_sp_nms_async(a, 64, 96, 0.015, 4, 4, a, 10 ** 6, None, 0, ctypes.byref(n), None, a, 1 << 30,
                                None) == _lib.EINVAL  # group 0
    assert L.fmpnp_sp_nms_async(a, 64, 96, 0.015, 4, 4, a, 10 ** 6, None, 4, ctypes.byref(n), None, a, 16, None) == _lib.EINVAL
    assert L.fmpnp_sp_nms_workspace_size(64, 96, 4) > 64 * 96 and L.fmpnp_sp_nms_workspace_size(64, 96, 17) == 0


def test_net_names_and_shapes():
    g = sc.golden("net")
    sd = fmpnp.SuperPointNet().state_dict()
    assert list(sd.keys()) == [str(n) for n in g["names"]]
    for (name, v), shape, nd in zip(sd.items(), g["shapes"], g["ndims"]):
        assert list(v.shape) == list(shape[:nd]), name
    semi, desc = fmpnp.SuperPointNet().eval()(torch.zeros(1, 1, 16, 24))
    assert semi.shape == (1, 65, 2, 3) and desc.shape == (1, 256, 2, 3)


def staged_cpu(query, refs, top_N, ratio):
    """SuperPointPredictor.run composed from the public stages, with the pick of predictor.py:48-54."""
    q_pts, q_desc = query
    finals = []
    for ref in refs[:top_N]:
        matches = fmpnp.fast_keypoint_matching(q_desc.T, ref["descriptors"].T, ratio, cpu=True)
        x2, r2, x3 = fmpnp.assemble_matches(q_pts, ref["keypoints"], ref["points_2D"], ref["points_3D"], matches, cpu=True)
        p = fmpnp.pnp.solve_pnp_cpu(x2, x3, ref["intrinsics"], ref["distortion_coefficients"], reference_filename=ref["filename"],
                                    reference_2D_points=r2, reference_keypoints=ref["keypoints"], return_masked=True, **sc.PNP)
        if not p.success and "fallback_pose" in ref:
            q, m = ref["fallback_pose"]
            p = fmpnp.Prediction(success=True, num_matches=x2.shape[0], num_inliers=0, reference_inliers=r2,
                                 query_inliers=np.squeeze(x2.reshape(-1, 1, 2)), points_3d=x3.reshape(-1, 1, 3), quaternion=q,
                                 matrix=m, reference_filename=ref["filename"], reference_keypoints=None, inlier_mask=None)
        finals.append(p)
    eligible = [(j, p) for j, p in enumerate(finals) if p.success]
    if not eligible:
        return None, None, finals
    j, best = eligible[int(np.argmax([p.num_inliers for _, p in eligible]))]
    return j, best, finals


def test_localize_equals_the_staged_composition():
    import localize_cases as lc
    query, refs = sc.localize_scene()
    loc = fmpnp.superpoint_localize(query, refs, top_N=4, ratio=0.9, return_masked=True, return_all=True, cpu=True, **sc.PNP)
    j, best, finals = staged_cpu(query, refs, 4, 0.9)
    assert j == 1 and loc.best == 1 and loc.kind == "solved" and best.num_inliers >= 60
    lc.equal_prediction(loc.prediction, best, "best")
    lc.equal(loc.export, [*best.quaternion, *list(np.asarray(best.matrix)[:3, 3])], "export")
    for k, (a, b) in enumerate(zip(loc.predictions, finals)):
        lc.equal_prediction(a, b, f"reference {k}")
    assert [p.success for p in finals] == [True, True, True, False] and finals[2].num_inliers == 0
    # the rank order decides what is tried: without the two good references the fallback is the best
    loc2 = fmpnp.superpoint_localize(query, refs[2:], top_N=2, ratio=0.9, return_masked=True, cpu=True, **sc.PNP)
    assert loc2.kind == "fallback" and loc2.best == 0 and loc2.prediction.matrix is refs[2]["fallback_pose"][1]
    loc3 = fmpnp.superpoint_localize(query, refs[3:], top_N=1, ratio=0.9, return_masked=True, cpu=True, **sc.PNP)
    assert loc3.kind == "none" and loc3.prediction is None and loc3.export is None
    # top_N cuts the list; top_N and ratio come from fmpnp.config when left None
    with pytest.raises(TypeError):
        fmpnp.superpoint_localize(query, refs, return_masked=True, cpu=True, **sc.PNP)
    fmpnp.config.configure(superpoint_top_N=1, superpoint_ratio=0.9)
    try:
        loc4 = fmpnp.superpoint_localize(query, refs, return_masked=True, return_all=True, cpu=True, **sc.PNP)
    finally:
        fmpnp.config.configure(superpoint_top_N=None, superpoint_ratio=None)
    assert loc4.best == 0 and len(loc4.predictions) == 1
    lc.equal_prediction(loc4.prediction, finals[0], "top_N = 1")


def test_exports():
    names = {f"fmpnp_sp_{s}{f}" for s in ("heatmap", "nms", "describe", "match", "assemble") for f in ("", "_async", "_cpu")}
    assert names <= set(_lib.EXPORTS)
    L = _lib.load()
    assert all(hasattr(L, n) for n in names) and L.fmpnp_abi_version() == 4
