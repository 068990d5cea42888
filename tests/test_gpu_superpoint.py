"""The SuperPoint baseline on the GPU (fmpnp.superpoint; fmpnp_sp_* of include/fmpnp.h): every stage equals its
CPU twin bit for bit on the shapes of tests/superpoint_cases.py, the outputs past each count keep the 0xA5 they
were filled with, two runs are identical, the asynchronous forms on a side stream equal the synchronous ones, the
NMS does not depend on the round-group size, and superpoint_localize equals its CPU form."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import localize_cases as lc
import superpoint_cases as sc
import fmpnp
from fmpnp import _lib
from fmpnp import superpoint as sp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5
DET = ("main", "dense", "border", "tiles")


def filled(shape, dtype):
    """A device tensor whose every byte is FILL."""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(FILL)
    return t


def untouched(t):
    return bool((t.contiguous().view(torch.uint8) == FILL).all())


@functools.lru_cache(maxsize=None)
def det_case(name):
    """(semi, coarse, H, W, nms_dist, conf_thresh): a golden case, or "tiles": 200 x 264 (no multiple of the NMS
    tile or the compaction chunk, thirteen chunks), random logits, several candidates per window."""
    if name == "tiles":
        rng = np.random.default_rng(77)
        semi = rng.standard_normal((65, 25, 33)).astype(np.float32) * 1.5
        semi[64] += 3.0
        coarse = rng.standard_normal((40, 25, 33)).astype(np.float32)
        return semi, coarse, 200, 264, 3, 0.02
    g = sc.golden(f"det_{name}")
    H, W, _, d, conf, _, _ = sc.DETECTOR[name]
    return g["semi"], g["coarse"], H, W, d, conf


@functools.lru_cache(maxsize=None)
def cpu_detect(name, align_corners=False):
    semi, coarse, H, W, d, conf = det_case(name)
    heat = sp.heatmap(semi, cpu=True)
    pts = sp.nms(heat, conf, d, cpu=True)
    return heat, pts, sp.describe(coarse, pts, (H, W), align_corners, cpu=True)


def gpu_nms(heat_dev, H, W, conf, d, group=4, extra=3):
    """fmpnp_sp_nms_async into a FILLed pts tensor: (pts tensor, n, rounds, device count)."""
    L = _lib.load()
    cap = int(L.fmpnp_sp_nms_capacity(H, W, d))
    pts, count = filled((3, cap + extra), torch.float64), filled((1,), torch.int32)
    ws = torch.empty(int(L.fmpnp_sp_nms_workspace_size(H, W, d)) // 8 + 1, dtype=torch.int64, device=DEV)
    n, rounds = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = L.fmpnp_sp_nms_async(heat_dev.data_ptr(), H, W, conf, d, 4, pts.data_ptr(), cap + extra, count.data_ptr(), group,
                              ctypes.byref(n), ctypes.byref(rounds), ws.data_ptr(), ws.numel() * 8, _lib.stream_ptr(DEV))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return pts, n.value, rounds.value, int(count.item())


@pytest.mark.parametrize("name", DET)
def test_detector_stages_equal_the_twins(name):
    semi, coarse, H, W, d, conf = det_case(name)
    heat_cpu, pts_cpu, desc_cpu = cpu_detect(name)
    heat = sp.heatmap(torch.from_numpy(semi.copy()).to(DEV))
    assert heat.cpu().numpy().tobytes() == heat_cpu.tobytes()
    pts, n, rounds, n_dev = gpu_nms(heat, H, W, conf, d)
    assert n == pts_cpu.shape[1] == n_dev and n > 0 and rounds >= 1
    assert pts[:, :n].cpu().numpy().tobytes() == pts_cpu.tobytes()  # x, y, confidence, order
    assert untouched(pts[:, n:])
    for align in (False, True):
        desc = filled((coarse.shape[0], n + 5), torch.float32)
        rc = _lib.load().fmpnp_sp_describe_async(torch.from_numpy(coarse.copy()).to(DEV).data_ptr(), coarse.shape[0], H // 8, W // 8,
                                                 pts.data_ptr(), pts.shape[1], n, H, W, int(align), desc.data_ptr(), n + 5,
                                                 _lib.stream_ptr(DEV))
        assert rc == 0
        torch.cuda.synchronize()
        assert desc[:, :n].cpu().numpy().tobytes() == cpu_detect(name, align)[2].tobytes()
        assert untouched(desc[:, n:])
    if name != "tiles":
        assert np.array_equal(pts[:2, :n].cpu().numpy(), sc.golden(f"det_{name}")["pts"][:2])  # the reference's


def test_postprocess_equals_the_twin_and_the_empty_case():
    for name in ("main", "none"):
        semi, coarse, H, W, d, conf = det_case(name)
        a = sp.superpoint_postprocess(torch.from_numpy(semi.copy()).to(DEV), torch.from_numpy(coarse.copy()).to(DEV), (H, W), d, conf)
        b = sp.superpoint_postprocess(semi, coarse, (H, W), d, conf, cpu=True)
        for x, y in zip(a, b):
            lc.equal(x, y, name)
    assert a[1] is None and a[2] is None and a[0].shape == (3, 0)


@pytest.mark.parametrize("name", ("main", "tiles"))
def test_nms_does_not_depend_on_the_group_size(name):
    semi, _, H, W, d, conf = det_case(name)
    heat = torch.from_numpy(cpu_detect(name)[0]).to(DEV)
    runs = [gpu_nms(heat, H, W, conf, d, group=g) for g in (1, 3, 4, 64, 4)]
    for pts, n, rounds, _ in runs[1:]:
        assert n == runs[0][1] and rounds == runs[0][2]
        assert torch.equal(pts.view(torch.uint8), runs[0][0].view(torch.uint8))  # (two runs with group 4 among them)
    assert 1 < runs[0][2] <= int((cpu_detect(name)[0] >= np.float32(conf)).sum())  # chains need more than a round


def test_synchronous_detector_forms_on_a_side_stream():
    L = _lib.load()
    semi, coarse, H, W, d, conf = det_case("main")
    heat_cpu, pts_cpu, desc_cpu = cpu_detect("main")
    side = torch.cuda.Stream(device=DEV)
    semi_d, coarse_d = torch.from_numpy(semi.copy()).to(DEV), torch.from_numpy(coarse.copy()).to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        s = _lib.stream_ptr(DEV)
        heat = np.zeros((H, W), np.float32)
        assert L.fmpnp_sp_heatmap(semi_d.data_ptr(), H // 8, W // 8, heat.ctypes.data, s) == 0
        assert heat.tobytes() == heat_cpu.tobytes()
        heat_d = torch.from_numpy(heat).to(DEV)
        cap = int(L.fmpnp_sp_nms_capacity(H, W, d))
        pts = np.zeros((3, cap + 2))
        pts.view(np.uint8)[:] = FILL
        n, rounds = ctypes.c_int(-1), ctypes.c_int(-1)
        assert L.fmpnp_sp_nms(heat_d.data_ptr(), H, W, conf, d, 4, pts.ctypes.data, cap + 2, 2, ctypes.byref(n),
                              ctypes.byref(rounds), s) == 0
        assert n.value == pts_cpu.shape[1] and pts[:, :n.value].tobytes() == pts_cpu.tobytes()
        assert (pts[:, n.value:].view(np.uint8) == FILL).all()
        pts_d = torch.from_numpy(pts_cpu).to(DEV)
        desc = np.zeros((coarse.shape[0], n.value + 1), np.float32)
        desc.view(np.uint8)[:] = FILL
        assert L.fmpnp_sp_describe(coarse_d.data_ptr(), coarse.shape[0], H // 8, W // 8, pts_d.data_ptr(), n.value, n.value,
                                   H, W, 0, desc.ctypes.data, n.value + 1, s) == 0
        assert desc[:, :n.value].tobytes() == desc_cpu.tobytes() and (desc[:, n.value:].view(np.uint8) == FILL).all()
    side.synchronize()


@functools.lru_cache(maxsize=None)
def cpu_match(name):
    seed = int(sc.golden("matching")[f"{name}.seed"])
    desc1, desc2 = sc.matching_inputs(name, seed)
    out = sp.two_nearest(desc1, desc2, sc.MATCHING[name][3], cpu=True)
    q_kp, r_kp, p2, p3 = sc.assembly_inputs(name, seed)
    asm = fmpnp.assemble_matches(q_kp, r_kp, p2, p3, out["matches"], cpu=True, return_argmins=True)
    return out, asm


@pytest.mark.parametrize("name", tuple(sc.MATCHING))
def test_matching_and_assembly_equal_the_twins(name):
    L = _lib.load()
    N1, N2, D, ratio = sc.MATCHING[name]
    seed = int(sc.golden("matching")[f"{name}.seed"])
    desc1, desc2 = sc.matching_inputs(name, seed)
    want, (x2_w, r2_w, x3_w, argmin_w) = cpu_match(name)
    # the synchronous form (host outputs) ...
    got = sp.two_nearest(torch.from_numpy(desc1.copy()).to(DEV), torch.from_numpy(desc2.copy()).to(DEV), ratio)
    for k in ("idx", "dist", "ok", "matches"):
        lc.equal(got[k], want[k], k)
    # ... and the asynchronous one on a side stream, into FILLed buffers, twice
    a, b = torch.from_numpy(desc1.copy()).to(DEV), torch.from_numpy(desc2.copy()).to(DEV).t().contiguous()
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    runs = []
    for _ in range(2):
        idx, dist, ok = filled((N1, 2), torch.int32), filled((N1, 2), torch.float32), filled((N1,), torch.uint8)
        matches, count = filled((N1, 2), torch.int64), filled((1,), torch.int32)
        ws = torch.empty(int(L.fmpnp_match_workspace_size(N1, N2)) // 4 + 1, dtype=torch.float32, device=DEV)
        with torch.cuda.stream(side):
            rc = L.fmpnp_sp_match_async(a.data_ptr(), N1, D, b.data_ptr(), D, N2, N2, ratio, idx.data_ptr(), dist.data_ptr(),
                                        ok.data_ptr(), matches.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel() * 4,
                                        _lib.stream_ptr(DEV))
        assert rc == 0
        side.synchronize()
        n = int(count.item())
        assert n == want["matches"].shape[0]
        assert idx.cpu().numpy().tobytes() == want["idx"].tobytes() and dist.cpu().numpy().tobytes() == want["dist"].tobytes()
        assert np.array_equal(ok.cpu().numpy().astype(bool), want["ok"])
        assert np.array_equal(matches[:n].cpu().numpy(), want["matches"]) and untouched(matches[n:])
        runs.append((idx, dist, ok, matches))
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(*runs))
    assert np.array_equal(want["matches"], sc.golden("matching")[f"{name}.matches"])  # the reference's
    # stage 5: the synchronous form through the package, the asynchronous one raw
    q_kp, r_kp, p2, p3 = sc.assembly_inputs(name, seed)
    x2, r2, x3, argmin = fmpnp.assemble_matches(q_kp, r_kp, p2, p3, want["matches"], return_argmins=True)
    for g_, w_ in ((x2, x2_w), (r2, r2_w), (x3, x3_w), (argmin, argmin_w)):
        lc.equal(g_, w_, "assembled")
    assert np.array_equal(fmpnp.fast_closest_points(r_kp[:2], p2), argmin_w.astype(np.int64))
    dq, dr, d2, d3 = (torch.from_numpy(np.array(v)).to(DEV) for v in (q_kp, r_kp, p2, p3))
    dm = torch.from_numpy(want["matches"]).to(DEV)
    am, o2, or2, o3 = (filled((N2,), torch.int32), filled((N2, 2), torch.float64), filled((N2, 2), torch.float64),
                       filled((N2, 3), torch.float64))
    count, ws = filled((1,), torch.int32), torch.empty(N2 + 1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        rc = L.fmpnp_sp_assemble_async(dq.data_ptr(), N1, N1, dr.data_ptr(), N2, N2, d2.data_ptr(), d3.data_ptr(), p2.shape[0],
                                       dm.data_ptr(), dm.shape[0], am.data_ptr(), o2.data_ptr(), or2.data_ptr(), o3.data_ptr(),
                                       count.data_ptr(), ws.data_ptr(), ws.numel() * 4, _lib.stream_ptr(DEV))
    assert rc == 0
    side.synchronize()
    n = int(count.item())
    assert n == x2_w.shape[0] and np.array_equal(am.cpu().numpy(), argmin_w)
    assert o2[:n].cpu().numpy().tobytes() == x2_w.tobytes() and or2[:n].cpu().numpy().tobytes() == r2_w.tobytes()
    assert o3[:n].cpu().numpy().tobytes() == x3_w.tobytes()
    assert untouched(o2[n:]) and untouched(or2[n:]) and untouched(o3[n:])


def test_rounds_of_rows_do_not_change_a_bit():
    """More rows than one round of the bounded score workspace holds would need gigabytes; the rounds are instead
    reached from below: the rows of a case in two calls equal the one call (each row is its own reduction)."""
    name = "n257_63"
    N1, N2, D, ratio = sc.MATCHING[name]
    desc1, desc2 = sc.matching_inputs(name, int(sc.golden("matching")[f"{name}.seed"]))
    whole = cpu_match(name)[0]
    d2 = torch.from_numpy(desc2.copy()).to(DEV)
    parts = [sp.two_nearest(torch.from_numpy(desc1[a:b].copy()).to(DEV), d2, ratio) for a, b in ((0, 130), (130, N1))]
    assert np.array_equal(np.vstack([p["idx"] for p in parts]), whole["idx"])
    assert np.vstack([p["dist"] for p in parts]).tobytes() == whole["dist"].tobytes()


def test_errors_and_empty_inputs():
    rng = np.random.default_rng(5)
    d1, d2 = rng.standard_normal((4, 16)).astype(np.float32), rng.standard_normal((1, 16)).astype(np.float32)
    with pytest.raises(_lib.FmpnpError, match="EINVAL"):
        sp.two_nearest(torch.from_numpy(d1).to(DEV), torch.from_numpy(d2).to(DEV), 0.9)
    out = sp.two_nearest(torch.from_numpy(d1[:0]).to(DEV), torch.from_numpy(np.repeat(d2, 3, 0)).to(DEV), 0.9)
    assert out["matches"].shape == (0, 2)
    x2, r2, x3 = fmpnp.assemble_matches(np.zeros((3, 0)), np.zeros((3, 7)), np.zeros((3, 2)), np.zeros((3, 3)),
                                        np.zeros((0, 2), np.int64))
    assert x2.shape == (0, 1, 2) and x3.shape == (0, 1, 3)


def test_localize_equals_its_cpu_form():
    query, refs = sc.localize_scene()
    kw = dict(top_N=4, ratio=0.9, return_masked=True, return_all=True, **sc.PNP)
    a, b = fmpnp.superpoint_localize(query, refs, **kw), fmpnp.superpoint_localize(query, refs, cpu=True, **kw)
    assert a.kind == b.kind == "solved" and a.best == b.best == 1
    lc.equal(a.export, b.export, "export")
    lc.equal_prediction(a.prediction, b.prediction, "best")
    for j, (x, y) in enumerate(zip(a.predictions, b.predictions)):
        lc.equal_prediction(x, y, f"reference {j}")


def test_frontend_runs_the_network_and_the_stages():
    torch.manual_seed(3)
    net = fmpnp.SuperPointNet().to(DEV).eval()
    fe = fmpnp.SuperPointFrontend(net, nms_dist=4, conf_thresh=0.015, nn_thresh=0.7)
    img = torch.rand(64, 96)
    pts, desc, heat = fe.run(img)
    with torch.no_grad():
        semi, coarse = net(img.to(DEV).view(1, 1, 64, 96))
    want = sp.superpoint_postprocess(semi.cpu(), coarse.cpu(), (64, 96), 4, 0.015, cpu=True)
    for x, y in zip((pts, desc, heat), want):
        lc.equal(x, y, "frontend")
