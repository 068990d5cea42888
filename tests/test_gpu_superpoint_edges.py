"""The SuperPoint baseline's kernels on the inputs of superpoint_edge_cases.py: plateaus of bit-equal heat, -0, NaN
and +Inf, a keep capacity reached exactly, more rounds than one group, keypoints whose taps leave the coarse map,
equal distances across lanes, waves and a thread's own stride, NaN and Inf scores, equidistant and NaN landmarks,
an unordered match list with duplicates and entries out of range.  Every case runs through the asynchronous
entry points into 0xA5-filled outputs and must equal the CPU twin bit for bit, a NaN standing for a NaN; the
twin's result is in turn compared with the numpy reference of the case, so a mistake the kernels and the twins
share (both are built from one header) fails here too.  Outputs past each count stay untouched and two runs are
identical."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import superpoint_edge_cases as ec
import fmpnp
from fmpnp import _lib
from fmpnp import superpoint as sp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5
GUARD = 16  # doubles behind an exactly-sized pts buffer
GROUPS = (1, 4, 64, 4)  # rounds per host read (two runs with 4 among them)


def filled(shape, dtype):
    """A device tensor whose every byte is FILL."""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(FILL)
    return t


def untouched(t):
    return bool((t.contiguous().view(torch.uint8) == FILL).all())


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def same(got, want, what=""):
    """Bit for bit, a NaN standing for a NaN (its sign and payload are the hardware's)."""
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (what, np.argwhere(np.isnan(got) != nan)[:8])
        got, want = np.where(nan, 0, got), np.where(nan, 0, want)
    assert got.tobytes() == want.tobytes(), (what, got.tobytes(), want.tobytes())


def gpu_nms(heat_dev, H, W, conf, d, border, group, extra):
    """fmpnp_sp_nms_async into a FILLed pts buffer of ld_pts = capacity + extra with GUARD doubles behind it:
    (the whole buffer, ld_pts, n, rounds)."""
    L = _lib.load()
    ld = int(L.fmpnp_sp_nms_capacity(H, W, d)) + extra
    buf, count = filled((3 * ld + GUARD,), torch.float64), filled((1,), torch.int32)
    ws = torch.empty(int(L.fmpnp_sp_nms_workspace_size(H, W, d)) // 8 + 1, dtype=torch.int64, device=DEV)
    n, rounds = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = L.fmpnp_sp_nms_async(heat_dev.data_ptr(), H, W, float(conf), d, border, buf.data_ptr(), ld, count.data_ptr(), group,
                              ctypes.byref(n), ctypes.byref(rounds), ws.data_ptr(), ws.numel() * 8, _lib.stream_ptr(DEV))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert int(count.item()) == n.value
    return buf, ld, n.value, rounds.value


def check_nms(heat, conf, d, border, extra, ref):
    """Every group size against the twin, and the twin against the reference; returns (n, rounds)."""
    H, W = heat.shape
    want = sp.nms(heat, conf, d, border, cpu=True)
    assert want.tobytes() == ref.tobytes()
    heat_dev = dev(heat)
    runs = [gpu_nms(heat_dev, H, W, conf, d, border, g, extra) for g in GROUPS]
    buf, ld, n, rounds = runs[0]
    assert n == want.shape[1], (n, want.shape[1])
    pts = buf[:3 * ld].view(3, ld)
    got = pts[:, :n].cpu().numpy()
    assert got.tobytes() == want.tobytes(), (got.tobytes(), want.tobytes())
    assert untouched(pts[:, n:]) and untouched(buf[3 * ld:])
    for other in runs[1:]:
        assert other[2] == n and other[3] == rounds, (other[2:], n, rounds)
        assert torch.equal(other[0].view(torch.uint8), buf.view(torch.uint8))
    return n, rounds


# ---- NMS ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", ec.PLATEAU_BORDERS)
@pytest.mark.parametrize("d", ec.PLATEAU_DISTS)
@pytest.mark.parametrize("shape", ec.PLATEAU_SHAPES)
def test_nms_plateau(shape, d, border):
    H, W = shape
    # ld_pts == capacity: no slack column
    n, rounds = check_nms(ec.plateau(H, W), ec.PLATEAU_CONF, d, border, 0, ec.plateau_ref(H, W, d, border)[0])
    print(f"plateau {H} x {W}, nms_dist {d}, border {border}: {n} points in {rounds} rounds")
    if border == 0:
        assert n == ec.capacity(H, W, d)
    if (shape, d) == ec.CHAIN:
        assert 100 <= rounds <= 200  # point 2k waits for 2k - 2: more rounds than one group of 64


@pytest.mark.parametrize("d", ec.LEVEL_DISTS)
@pytest.mark.parametrize("conf", ec.LEVEL_CONFS)
@pytest.mark.parametrize("shape", ec.LEVEL_SHAPES)
def test_nms_levels_with_nan_negative_zero_and_inf(shape, conf, d):
    H, W = shape
    n, rounds = check_nms(ec.levels(H, W, d), conf, d, ec.LEVEL_BORDER, 3, ec.levels_ref(H, W, conf, d)[0])
    assert n > 0 and rounds >= 1


def test_synchronous_nms_on_a_side_stream_at_the_capacity():
    L = _lib.load()
    (H, W), d = (20, 37), 4
    heat = ec.plateau(H, W)
    want = ec.plateau_ref(H, W, d, 0)[0]
    cap = ec.capacity(H, W, d)
    # (a stream of torch's high-priority pool: taking one of the default pool would shift which two streams every
    # later test of the process gets, and test_refine_batch_two_streams_concurrent needs two that overlap)
    side = torch.cuda.Stream(device=DEV, priority=-1)
    heat_dev = dev(heat)
    torch.cuda.synchronize()
    buf = np.zeros(3 * cap + GUARD)
    buf.view(np.uint8)[:] = FILL
    n, rounds = ctypes.c_int(-1), ctypes.c_int(-1)
    with torch.cuda.stream(side):
        rc = L.fmpnp_sp_nms(heat_dev.data_ptr(), H, W, ec.PLATEAU_CONF, d, 0, buf.ctypes.data, cap, 2, ctypes.byref(n),
                            ctypes.byref(rounds), _lib.stream_ptr(DEV))
    side.synchronize()
    assert rc == 0 and n.value == cap == want.shape[1]
    assert buf[:3 * cap].tobytes() == want.tobytes() and (buf[3 * cap:].view(np.uint8) == FILL).all()


# ---- the detector head and the whole front end -------------------------------------------------------------------
def test_heat_extremes_and_postprocess():
    semi = ec.heat_extremes()
    heat = sp.heatmap(dev(semi)).cpu().numpy()
    want = sp.heatmap(semi, cpu=True)
    same(heat, want, "heat")
    nan = np.isnan(want)
    print(f"NaN heat: the twin's bits {sorted({hex(v) for v in want.view(np.uint32)[nan]})}, the kernel's "
          f"{sorted({hex(v) for v in heat.view(np.uint32)[nan]})}")
    rng = np.random.default_rng(3)
    coarse = rng.standard_normal((16, ec.HEAT_HC, ec.HEAT_WC)).astype(np.float32)
    plateau = np.full((65, 3, 5), 0.3, np.float32)
    for semi, coarse, hw, d, conf in ((semi, coarse, (8 * ec.HEAT_HC, 8 * ec.HEAT_WC), 1, 0.015),
                                      (plateau, rng.standard_normal((16, 3, 5)).astype(np.float32), (24, 40), 4, 0.01)):
        a = sp.superpoint_postprocess(dev(semi), dev(coarse), hw, d, conf)
        b = sp.superpoint_postprocess(semi, coarse, hw, d, conf, cpu=True)
        assert b[0].shape[1] > 4
        for x, y, what in zip(a, b, ("pts", "desc", "heat")):
            same(x, y, what)


# ---- descriptors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align_corners", (False, True))
def test_descriptors_at_points_off_the_map(align_corners):
    L = _lib.load()
    buf, coarse = ec.desc_coarse()
    pts = ec.desc_points()
    N, H, W = pts.shape[1], ec.DESC_H, ec.DESC_W
    want = sp.describe(coarse, pts, (H, W), align_corners, cpu=True)
    none = np.isnan(want).all(axis=0)
    assert none.sum() == (5 if align_corners else 9) and not np.isnan(want[:, ~none]).any()
    assert np.array_equal(none, ec.desc64_padded(coarse, pts, H, W, align_corners)[1] == 0)  # the columns without a tap
    buf_dev = dev(buf)  # the map in the middle of NaN: a read outside it would show
    wide = np.full((3, N + 3), np.nan)
    wide[:, :N] = pts
    pts_dev = dev(wide)
    runs = []
    for _ in range(2):
        desc = filled((ec.DESC_D, N + 5), torch.float32)
        rc = L.fmpnp_sp_describe_async(buf_dev.data_ptr() + 4 * ec.DESC_PAD, ec.DESC_D, ec.DESC_HC, ec.DESC_WC, pts_dev.data_ptr(),
                                       N + 3, N, H, W, int(align_corners), desc.data_ptr(), N + 5, _lib.stream_ptr(DEV))
        assert rc == 0
        torch.cuda.synchronize()
        same(desc[:, :N], want, "desc")  # (the columns without a tap are NaN in every channel, as the twin's)
        assert untouched(desc[:, N:])
        runs.append(desc)
    assert torch.equal(runs[0].view(torch.uint8), runs[1].view(torch.uint8))


# ---- two nearest -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cpu_two_nearest(ratio):
    return sp.two_nearest(*ec.nn_inputs(), ratio, cpu=True)


def gpu_match(a, b_t, rows, ratio):
    """fmpnp_sp_match_async over the query rows [rows[0], rows[1]) into FILLed outputs."""
    L = _lib.load()
    i0, n1 = rows[0], rows[1] - rows[0]
    idx, dist, ok = filled((n1, 2), torch.int32), filled((n1, 2), torch.float32), filled((n1,), torch.uint8)
    matches, count = filled((n1, 2), torch.int64), filled((1,), torch.int32)
    ws = torch.empty(int(L.fmpnp_match_workspace_size(n1, ec.NN_N2)) // 4 + 1, dtype=torch.float32, device=DEV)
    rc = L.fmpnp_sp_match_async(a.data_ptr() + 4 * ec.NN_D * i0, n1, ec.NN_D, b_t.data_ptr(), ec.NN_D, ec.NN_N2, ec.NN_N2,
                                float(ratio), idx.data_ptr(), dist.data_ptr(), ok.data_ptr(), matches.data_ptr(),
                                count.data_ptr(), ws.data_ptr(), ws.numel() * 4, _lib.stream_ptr(DEV))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return idx, dist, ok, matches, int(count.item())


@pytest.mark.parametrize("ratio", ec.NN_RATIOS)
def test_two_nearest_with_equal_distances_nan_and_inf(ratio):
    d1, d2 = ec.nn_inputs()
    want = cpu_two_nearest(ratio)
    ref = ec.nn_ref(ratio)
    for row, expect in ec.NN_EXPECT.items():
        assert tuple(want["idx"][row]) == expect
    assert np.array_equal(want["idx"], ref["idx"]) and np.array_equal(want["dist"], ref["dist"], equal_nan=True)
    assert np.array_equal(want["ok"], ref["ok"]) and np.array_equal(want["matches"], ref["matches"])
    a, b_t = dev(d1), dev(d2).t().contiguous()
    runs = [gpu_match(a, b_t, (0, ec.NN_N1), ratio) for _ in range(2)]
    idx, dist, ok, matches, n = runs[0]
    same(idx, want["idx"], "idx")
    same(dist, want["dist"], "dist")
    assert np.array_equal(ok.cpu().numpy().astype(bool), want["ok"])
    assert n == want["matches"].shape[0] and np.array_equal(matches[:n].cpu().numpy(), want["matches"]) and untouched(matches[n:])
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(runs[0][:4], runs[1][:4]))
    # the round size is the library's (a workspace below fmpnp_match_workspace_size is an error), so the rounds of
    # rows are reached from below, as test_rounds_of_rows_do_not_change_a_bit does: the rows in two calls
    cut = 33
    for i0, i1 in ((0, cut), (cut, ec.NN_N1)):
        idx, dist, ok, matches, n = gpu_match(a, b_t, (i0, i1), ratio)
        same(idx, want["idx"][i0:i1], "idx of a part")
        same(dist, want["dist"][i0:i1], "dist of a part")
        assert np.array_equal(ok.cpu().numpy().astype(bool), want["ok"][i0:i1])
        part = want["matches"][(want["matches"][:, 0] >= i0) & (want["matches"][:, 0] < i1)] - np.array([i0, 0])
        assert n == part.shape[0] and np.array_equal(matches[:n].cpu().numpy(), part) and untouched(matches[n:])
    # ... and the synchronous form with the library's own workspace
    got = sp.two_nearest(a, dev(d2), ratio)
    same(got["idx"], want["idx"], "idx, synchronous")
    same(got["dist"], want["dist"], "dist, synchronous")
    assert np.array_equal(got["ok"], want["ok"]) and np.array_equal(got["matches"], want["matches"])


# ---- association and assembly ------------------------------------------------------------------------------------
@pytest.mark.parametrize("matches", ("list", "empty"))
@pytest.mark.parametrize("which", ec.ASM_LANDMARK_SETS)
def test_assembly_with_equidistant_and_nan_landmarks(which, matches):
    L = _lib.load()
    q, r, _, _, m = ec.asm_inputs()
    p2, p3 = ec.asm_landmarks(which)
    m = m if matches == "list" else m[:0]
    x2_w, r2_w, x3_w, argmin_w = fmpnp.assemble_matches(q, r, p2, p3, m, cpu=True, return_argmins=True)
    ref = ec.asm_ref(which, matches == "list")
    for w, v in zip((argmin_w, x2_w.reshape(-1, 2), r2_w.reshape(-1, 2), x3_w.reshape(-1, 3)), ref):
        assert w.dtype == v.dtype and w.tobytes() == v.tobytes()
    if which == "all":
        assert argmin_w[ec.ASM_ON] == argmin_w[ec.ASM_NEAR] == ec.ASM_SAME[0] and argmin_w[ec.ASM_NAN_KEYPOINT] == 0
    N1, N2, M = ec.ASM_N1, ec.ASM_N2, p2.shape[0]
    dq, dr, d2, d3 = dev(q), dev(r), dev(p2), dev(p3)
    dm = dev(m) if len(m) else torch.zeros((1, 2), dtype=torch.int64, device=DEV)
    runs = []
    for _ in range(2):
        am, o2, or2, o3 = (filled((N2,), torch.int32), filled((N2, 2), torch.float64), filled((N2, 2), torch.float64),
                           filled((N2, 3), torch.float64))
        count, ws = filled((1,), torch.int32), torch.empty(N2 + 1, dtype=torch.int32, device=DEV)
        rc = L.fmpnp_sp_assemble_async(dq.data_ptr(), N1, N1, dr.data_ptr(), N2, N2, d2.data_ptr(), d3.data_ptr(), M,
                                       dm.data_ptr(), len(m), am.data_ptr(), o2.data_ptr(), or2.data_ptr(), o3.data_ptr(),
                                       count.data_ptr(), ws.data_ptr(), ws.numel() * 4, _lib.stream_ptr(DEV))
        assert rc == 0, rc
        torch.cuda.synchronize()
        n = int(count.item())
        assert n == x2_w.shape[0] and (n > 0) == (matches == "list")
        assert np.array_equal(am.cpu().numpy(), argmin_w)
        assert o2[:n].cpu().numpy().tobytes() == x2_w.tobytes() and or2[:n].cpu().numpy().tobytes() == r2_w.tobytes()
        assert o3[:n].cpu().numpy().tobytes() == x3_w.tobytes()
        assert untouched(o2[n:]) and untouched(or2[n:]) and untouched(o3[n:])
        runs.append((am, o2, or2, o3))
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(*runs))
    # the synchronous form through the package
    got = fmpnp.assemble_matches(q, r, p2, p3, m, return_argmins=True)
    for g, w in zip(got, (x2_w, r2_w, x3_w, argmin_w)):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
