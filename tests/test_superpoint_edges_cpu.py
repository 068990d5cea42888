"""The SuperPoint baseline's CPU twins on the inputs its goldens were chosen to avoid (superpoint_edge_cases.py):
plateaus of bit-equal heat, -0, NaN and +Inf heat, every nms_dist and conf_thresh <= 0, a keep capacity that is
reached exactly, keypoints whose taps leave the coarse map, duplicated descriptors and equal distances, NaN and
Inf scores, equidistant and NaN landmarks, an unordered match list with duplicates and entries out of range.
Each twin is held to a plain numpy reference written from the contract text.  What a case is meant to contain is
asserted from the reference alone before the twin is called, so a seed that stops providing it fails as a
condition and not as a parity error."""
import ctypes

import numpy as np
import pytest
import torch

import superpoint_cases as sc
import superpoint_edge_cases as ec
import fmpnp
from fmpnp import _lib
from fmpnp import superpoint as sp

FILL = 0xA5
GUARD = 16  # doubles behind an exactly-sized pts buffer


def filled(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == FILL).all())


def twin_nms(heat, conf, d, border, extra):
    """fmpnp_sp_nms_cpu into a FILLed buffer of ld_pts = capacity + extra columns with GUARD doubles behind it:
    (the buffer as [3, ld_pts], the guard, n)."""
    L = _lib.load()
    H, W = heat.shape
    cap = int(L.fmpnp_sp_nms_capacity(H, W, d))
    assert cap == ec.capacity(H, W, d)
    buf = filled(3 * (cap + extra) + GUARD, np.float64)
    n = ctypes.c_int(-1)
    heat = np.ascontiguousarray(heat, np.float32)
    rc = L.fmpnp_sp_nms_cpu(heat.ctypes.data, H, W, float(conf), d, border, buf.ctypes.data, cap + extra, ctypes.byref(n))
    assert rc == 0, rc
    return buf[:3 * (cap + extra)].reshape(3, cap + extra), buf[3 * (cap + extra):], n.value


def check_nms(heat, conf, d, border, want, extra):
    pts, guard, n = twin_nms(heat, conf, d, border, extra)
    assert n == want.shape[1], (n, want.shape[1])
    assert pts[:, :n].tobytes() == want.tobytes(), (pts[:, :n], want)
    assert untouched(pts[:, n:]) and untouched(guard)


# ---- NMS ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", ec.PLATEAU_BORDERS)
@pytest.mark.parametrize("d", ec.PLATEAU_DISTS)
@pytest.mark.parametrize("shape", ec.PLATEAU_SHAPES)
def test_nms_plateau_keeps_the_lattice(shape, d, border):
    H, W = shape
    heat = ec.plateau(H, W)
    want, kept = ec.plateau_ref(H, W, d, border)
    # the conditions: equal heats walk in pixel order, so the kept set is the lattice of multiples of d + 1 and
    # the capacity is reached exactly
    cap = ec.capacity(H, W, d)
    assert kept == cap
    lattice = [(x, y) for y in range(0, H, d + 1) for x in range(0, W, d + 1)
               if border <= x < W - border and border <= y < H - border]
    assert [tuple(c) for c in want[:2].T.astype(int)] == lattice and np.all(want[2] == 0.5)
    if border == 0:
        assert want.shape[1] == cap
    elif shape != (20, 37) or d == 16:
        assert want.shape[1] == 0 and kept > 0  # a kept set that empties after the drop
    else:
        assert 0 < want.shape[1] < cap
    check_nms(heat, ec.PLATEAU_CONF, d, border, want, extra=0)  # ld_pts == capacity: no slack column


def test_nms_plateau_capacities():
    assert [ec.capacity(20, 37, d) for d in ec.PLATEAU_DISTS] == [740, 190, 32, 6]
    (H, W), d = ec.CHAIN
    assert ec.plateau_ref(H, W, d, 0)[1] == 100  # every other pixel of the row


@pytest.mark.parametrize("d", ec.LEVEL_DISTS)
@pytest.mark.parametrize("conf", ec.LEVEL_CONFS)
@pytest.mark.parametrize("shape", ec.LEVEL_SHAPES)
def test_nms_levels_with_nan_negative_zero_and_inf(shape, conf, d):
    H, W = shape
    heat = ec.levels(H, W, d)
    assert np.isnan(heat).any() and np.isposinf(heat).any() and (np.signbit(heat) & (heat == 0)).sum() > 10
    want, kept = ec.levels_ref(H, W, conf, d)
    assert 0 < want.shape[1] <= kept and (kept > want.shape[1] or d == 16) and not np.isnan(want).any()
    assert np.isposinf(want[2, 0]) and np.all(want[2, :-1] >= want[2, 1:])
    if want.shape[1] > 2:
        assert np.any(want[2, :-1] == want[2, 1:])  # equal heats among the kept points
    if conf <= 0:
        y, x, _ = ec.level_plant(H, W, d)
        negzero = np.signbit(want[2])
        assert negzero.any() and (x, y) in [tuple(c) for c in want[:2, negzero].T.astype(int)]  # a -0 is a candidate
        if d == 0:
            assert ((want[2] == 0) & ~negzero).sum() > 10 < negzero.sum()  # ... among +0 ones of the same rank
    else:
        assert want[2].min() >= 0.25
    check_nms(heat, conf, d, ec.LEVEL_BORDER, want, extra=3)


def test_postprocess_on_a_plateau_and_on_the_heat_extremes():
    rng = np.random.default_rng(3)
    semi = np.full((65, 3, 5), 0.3, np.float32)  # 65 equal logits per cell: one plateau over the image
    coarse = rng.standard_normal((16, 3, 5)).astype(np.float32)
    pts, desc, heat = sp.superpoint_postprocess(semi, coarse, (24, 40), 4, 0.01, cpu=True)
    assert np.all(heat == heat[0, 0]) and 0.015 < heat[0, 0] < 0.016
    want, _ = ec.greedy_nms(heat, 0.01, 4, 4)
    assert want.shape[1] == 3 * 7 and pts.tobytes() == want.tobytes() and desc.shape == (16, 21)
    semi = ec.heat_extremes()
    coarse = rng.standard_normal((16, ec.HEAT_HC, ec.HEAT_WC)).astype(np.float32)
    pts, desc, heat = sp.superpoint_postprocess(semi, coarse, (8 * ec.HEAT_HC, 8 * ec.HEAT_WC), 1, 0.015, cpu=True)
    want, _ = ec.greedy_nms(heat, 0.015, 1, 4)
    assert want.shape[1] > 4 and pts.tobytes() == want.tobytes() and not np.isnan(desc).any()


# ---- the detector head -------------------------------------------------------------------------------------------
def test_heat_extremes():
    semi = ec.heat_extremes()
    heat = sp.heatmap(semi, cpu=True)
    with np.errstate(all="ignore"):
        heat64 = sc.heat64(semi)
    # NaN exactly where the fp32 exponential overflows (Inf / Inf) and over the cell with the NaN logit
    want_nan = np.zeros(heat.shape, bool)
    want_nan[ec.cell_pixels(ec.CELL_NAN)] = True
    want_nan[8 * ec.CELL_OVERFLOW[0] + ec.OVERFLOW_CHANNEL // 8, 8 * ec.CELL_OVERFLOW[1] + ec.OVERFLOW_CHANNEL % 8] = True
    assert np.array_equal(np.isnan(heat), want_nan)
    rest = heat[ec.cell_pixels(ec.CELL_OVERFLOW)].ravel()
    rest = np.delete(rest, ec.OVERFLOW_CHANNEL)
    assert np.all(rest == 0) and not np.signbit(rest).any()  # finite / Inf
    assert heat[8 * ec.CELL_LARGE[0] + ec.LARGE_CHANNEL // 8, 8 * ec.CELL_LARGE[1] + ec.LARGE_CHANNEL % 8] >= 1 - 2.0 ** -22
    assert heat[8 * ec.CELL_TINY[0] + ec.TINY_CHANNEL // 8, 8 * ec.CELL_TINY[1] + ec.TINY_CHANNEL % 8] == 0.0
    equal = heat[ec.cell_pixels(ec.CELL_EQUAL)]
    assert len({v.tobytes() for v in equal.ravel()}) == 1 and equal[0, 0] > 0  # 64 bit-equal values
    assert 0 < heat[ec.cell_pixels(ec.CELL_DUST)].max() < 1e-24
    # elsewhere the fp64 restatement, within the tolerance of test_heatmap_and_descriptors_within_the_reference_error
    # (4 x the reference's own fp32 error; the smallest of the golden cases')
    tol = 4 * min(float(sc.golden(f"det_{name}")["e_ref_heat"]) for name in ("main", "dense", "border"))
    ok = ~want_nan
    ok[ec.cell_pixels(ec.CELL_OVERFLOW)] = False  # (exp(89) is finite in fp64: there the fp64 heat is not the contract's)
    assert np.isfinite(heat64[ok]).all()
    err = np.abs(heat[ok] - heat64[ok]).max()
    print(f"heat extremes: error {err:.3e} against fp64 (tolerance {tol:.3e})")
    assert err <= tol


# ---- descriptors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align_corners", (False, True))
def test_descriptors_at_points_off_the_map(align_corners):
    buf, coarse = ec.desc_coarse()
    pts = ec.desc_points()
    H, W, N = ec.DESC_H, ec.DESC_W, pts.shape[1]
    raw, norm, taps = ec.desc64_padded(coarse, pts, H, W, align_corners)
    # the conditions, from the fp64 restatement alone
    some = taps > 0
    assert (~some).sum() == (5 if align_corners else 9) and (norm[~some] == 0).all()
    assert norm[some].min() >= 0.05, norm
    assert {1, 4} <= set(taps.tolist())  # one tap of a corner cell left, and all four
    desc = filled((ec.DESC_D, N + 2), np.float32)
    rc = _lib.load().fmpnp_sp_describe_cpu(coarse.ctypes.data, ec.DESC_D, ec.DESC_HC, ec.DESC_WC, pts.ctypes.data, N, N, H, W,
                                           int(align_corners), desc.ctypes.data, N + 2)
    assert rc == 0 and untouched(desc[:, N:])
    desc = desc[:, :N]
    assert np.array_equal(np.isnan(desc).all(axis=0), norm == 0)  # 0 / 0: a column is NaN iff it has no sample
    assert not np.isnan(desc[:, some]).any()  # (a NaN here would be a read outside the map)
    # the bound test_sampling_against_grid_sample derives, with this case's smallest norm
    bound = 2 * 19 * 2.0 ** -24 / norm[some].min() * 2
    e64 = np.abs(desc[:, some] - raw[:, some] / norm[some]).max()
    with np.errstate(invalid="ignore", over="ignore"):
        grid = torch.from_numpy(np.stack([pts[0] / (float(W) / 2.) - 1., pts[1] / (float(H) / 2.) - 1.], 1)).float()
    ref = torch.nn.functional.grid_sample(torch.from_numpy(coarse.copy())[None], grid.view(1, 1, -1, 2), mode="bilinear",
                                          padding_mode="zeros", align_corners=align_corners)
    ref = ref.numpy().reshape(ec.DESC_D, N).astype(np.float64)
    ref_norm = np.linalg.norm(ref, axis=0)
    # grid_sample agrees on which columns have no descriptor (zero, or NaN where a coordinate is not finite)
    assert np.array_equal((ref_norm == 0) | np.isnan(ref_norm), norm == 0)
    e_gs = np.abs(desc[:, some] - ref[:, some] / ref_norm[some]).max()
    print(f"align_corners={align_corners}: descriptor error {e64:.3e} against fp64, {e_gs:.3e} against grid_sample "
          f"(bound {bound:.3e}, smallest norm {norm[some].min():.4f})")
    assert e64 <= bound and e_gs <= bound


# ---- two nearest -------------------------------------------------------------------------------------------------
def test_two_nearest_case_conditions():
    ref = ec.nn_ref(ec.NN_RATIOS[0])
    for row, want in ec.NN_EXPECT.items():
        assert tuple(ref["idx"][row]) == want, (row, ref["idx"][row])
    assert ref["all"][ec.NN_ROW_DUP, list(ec.NN_DUPLICATES)].tolist() == [-22.0] * 4
    assert ref["all"][ec.NN_ROW_SECONDS, [500, 64, 257]].tolist() == [-22.0, -20.0, -20.0]
    assert np.all(ref["all"][ec.NN_ROW_ZERO, :2] == 2.0) and np.isnan(ref["all"][ec.NN_ROW_NAN]).all()
    assert (ref["dist"][:, 0] == ref["dist"][:, 1]).sum() >= 10
    assert np.isnan(ref["all"]).all(axis=1).sum() >= 1 and np.isnan(ref["all"][:, ec.NN_NAN_COLUMN]).all()
    assert not (ref["idx"] == ec.NN_NAN_COLUMN).any()
    column = ref["all"][:, ec.NN_INF_COLUMN]
    assert np.isneginf(column).any() and np.isposinf(column).any() and np.isnan(column).any()
    assert (ref["idx"][np.isneginf(column), 0] == ec.NN_INF_COLUMN).all()  # a distance of -Inf is the nearest
    assert (ref["dist"] < 0).sum() > 50  # the ratio test on negative numbers
    for ratio in ec.NN_RATIOS:
        ok = ec.nn_ref(ratio)["ok"]
        assert ok.any() and not ok.all() and not ok[ec.NN_ROW_NAN]


@pytest.mark.parametrize("ratio", ec.NN_RATIOS)
def test_two_nearest_with_equal_distances_nan_and_inf(ratio):
    d1, d2 = ec.nn_inputs()
    want = ec.nn_ref(ratio)
    got = sp.two_nearest(d1, d2, ratio, cpu=True)
    assert np.array_equal(got["idx"], want["idx"]), np.flatnonzero((got["idx"] != want["idx"]).any(axis=1))
    assert got["dist"].dtype == np.float32 and np.array_equal(got["dist"], want["dist"], equal_nan=True)
    assert np.array_equal(np.signbit(got["dist"]), np.signbit(want["dist"]))
    assert np.array_equal(got["ok"], want["ok"]) and np.array_equal(got["matches"], want["matches"])


# ---- association and assembly ------------------------------------------------------------------------------------
def test_assembly_case_conditions():
    q, _, _, _, m = ec.asm_inputs()
    argmin, x2d, x2d_ref, x3d = ec.asm_ref("all", True)
    assert argmin[ec.ASM_ON] == argmin[ec.ASM_NEAR] == ec.ASM_SAME[0] and argmin[ec.ASM_NAN_KEYPOINT] == 0
    assert not np.isin(argmin[np.arange(ec.ASM_N2) != ec.ASM_NAN_KEYPOINT], ec.ASM_NAN_LANDMARKS).any()
    rows = m[(m[:, 0] >= 0) & (m[:, 0] < ec.ASM_N1) & (m[:, 1] >= 0) & (m[:, 1] < ec.ASM_N2)]
    assert len(m) - len(rows) == 6 and len(np.unique(rows[:, 1])) == x2d.shape[0] < len(rows)
    assert not np.all(np.diff(rows[:, 1]) >= 0)  # unordered
    keys = np.unique(rows[:, 1])
    for j, named in ec.ASM_NAMED.items():
        mine = m[m[:, 1] == j, 0]
        assert sorted(mine[:len(named)].tolist()) == sorted(named) and len(mine) >= 3
        assert mine[len(named) - 1] == named[-1] == min(mine)  # the lowest row comes behind the others
        assert np.array_equal(x2d[np.searchsorted(keys, j)], q[:2, min(mine)])
    # the ignored entries name no keypoint (14 and 15 are what 2^40 + 14 and 2^40 + 15 would be as 32-bit numbers)
    assert 11 in keys and not np.isin([12, 13, 14, 15], keys).any()
    for which in ec.ASM_LANDMARK_SETS[1:]:
        assert not ec.asm_ref(which, True)[0].any()  # one landmark, or none that is a number


@pytest.mark.parametrize("matches", ("list", "empty"))
@pytest.mark.parametrize("which", ec.ASM_LANDMARK_SETS)
def test_assembly_with_equidistant_and_nan_landmarks(which, matches):
    q, r, _, _, m = ec.asm_inputs()
    p2, p3 = ec.asm_landmarks(which)
    m = m if matches == "list" else m[:0]
    argmin, x2d, x2d_ref, x3d = ec.asm_ref(which, matches == "list")
    got2, gotr, got3, got_argmin = fmpnp.assemble_matches(q, r, p2, p3, m, cpu=True, return_argmins=True)
    assert got_argmin.dtype == np.int32 and np.array_equal(got_argmin, argmin)
    assert got2.shape[0] == x2d.shape[0] == (0 if matches == "empty" else x2d.shape[0])
    assert got2.reshape(-1, 2).tobytes() == x2d.tobytes() and gotr.reshape(-1, 2).tobytes() == x2d_ref.tobytes()
    assert got3.reshape(-1, 3).tobytes() == x3d.tobytes()
