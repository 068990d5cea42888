"""P3P RANSAC + polish on the GPU (fmpnp_pnp_ransac / _async) against the CPU twin: every result field
and mask byte equal under ==.  This is also the repository's check that fp64 / and sqrt on gfx950 round
as the host's do.  Cases and generator: tests/pnp_cases.py."""
import ctypes
import functools
import threading

import numpy as np
import pytest
import torch

import pnp_cases as pc
import fmpnp
from fmpnp import _lib, pnp, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def case(name):
    return pc.make_case(name)


@functools.lru_cache(maxsize=None)
def shaped(M, iters, seed=None):
    """A planted problem of M points (30 % outliers, 0.5 px noise) with its own generator seed."""
    c = pc.generate(M, 0.3 if M > 5 else 0.0, 0.5 if M > 5 else 0.0, 400.0, (0.0, 0.0, 0.0, 0.0),
                    1000 + M if seed is None else seed, iters)
    return pc.problem(c)


def assert_equal(gpu, cpu):
    assert len(gpu) == len(cpu)
    for i, (g, c) in enumerate(zip(gpu, cpu)):
        for k in ("R", "t", "R_hyp", "t_hyp", "cost", "num_inliers", "best_h", "status", "polish_iters", "mask"):
            a, b = np.asarray(g[k]), np.asarray(c[k])
            assert a.tobytes() == b.tobytes(), (i, k, a, b)


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_gpu_equals_twin_on_the_cases(name):
    c = case(name)  # (robotcar866 is the one case with iters = 5000)
    p = pc.problem(c)
    gpu, cpu = pnp.ransac([p], DEV), pnp.ransac_cpu([p], 16)
    assert_equal(gpu, cpu)
    assert (gpu[0]["mask"].astype(bool) == c["planted"]).all() and gpu[0]["status"] == _lib.PNP_OK


RAGGED = {
    1: [(257, 256)],
    3: [(65, 257), (4100, 255), (13, 1)],
    10: [(4, 256), (5, 257), (13, 255), (64, 1), (65, 256), (257, 257), (866, 255), (4100, 256), (3, 64), (300, 257)],
}


@pytest.mark.parametrize("B", sorted(RAGGED))
def test_gpu_equals_twin_on_ragged_batches(B):
    probs = [shaped(M, iters) for M, iters in RAGGED[B]]
    gpu, cpu = pnp.ransac(probs, DEV), pnp.ransac_cpu(probs, 16)
    assert_equal(gpu, cpu)
    for (M, iters), g in zip(RAGGED[B], gpu):
        assert g["status"] == (_lib.PNP_TOO_FEW if M < 4 else g["status"])
        if M >= 13 and iters >= 255:
            assert g["status"] == _lib.PNP_OK and g["num_inliers"] >= M - int(round(0.3 * M))


def degenerate_problems():
    c = case("noisy300")
    inl = np.flatnonzero(c["planted"])
    X, x = c["points3d"].copy(), c["points2d"].copy()
    X[inl[3], 1] = np.nan
    x[inl[7], 0] = np.inf
    X[inl[11], 2] = -np.inf
    nonfinite = pc.problem(c, points3d=X, points2d=x)
    s = np.arange(40, dtype=np.float64)
    Xl = np.stack([1.0 + s, 2.0 + 2.0 * s, 30.0 + 4.0 * s], 1)
    K = c["K"]
    xl, _ = pc.project(K, (0, 0, 0, 0), np.eye(3), np.zeros(3), Xl)
    collinear = dict(points3d=Xl, points2d=xl, K=K, dist=np.zeros(4), threshold=12.0, iters=256, seed=0)
    rng = np.random.Generator(np.random.PCG64(77))
    outliers = pc.problem(c, points2d=rng.uniform(40.0, 984.0, (300, 2)), iters=256)
    all_nan = pc.problem(c, points3d=np.full((300, 3), np.nan), iters=64)
    same = pc.problem(c, points3d=np.repeat(c["points3d"][:1], 300, 0), iters=64)
    return [nonfinite, collinear, outliers, all_nan, same, shaped(3, 64)]


def test_non_finite_and_degenerate_problems_equal_the_twin():
    probs = degenerate_problems()
    gpu, cpu = pnp.ransac(probs, DEV), pnp.ransac_cpu(probs, 16)
    assert_equal(gpu, cpu)
    assert gpu[0]["status"] == _lib.PNP_OK and gpu[0]["num_inliers"] == case("noisy300")["planted"].sum() - 3
    assert gpu[1]["status"] == _lib.PNP_NO_MODEL and gpu[3]["status"] == _lib.PNP_NO_MODEL
    assert gpu[5]["status"] == _lib.PNP_TOO_FEW


def test_multi_call_equals_the_single_calls():
    names = ["tiny13", "noisy300", "exact64"]
    items = []
    for n in names:
        c = case(n)
        items.append((c["points2d"], c["points3d"], n + ".jpg", c["points2d"] + 5.0, None))
    items.append((case("tiny13")["points2d"][:6], case("tiny13")["points3d"][:6], "few.jpg", None, None))  # too few matches
    K = case("tiny13")["K"]
    kw = dict(reprojection_threshold=12.0, minimum_matches=10, minimum_inliers=8, return_masked=True, iters=1024)
    multi = fmpnp.solve_pnp_multi(items, K, np.zeros(4), **kw)
    assert multi[3].success is False and multi[3].num_matches == 6
    for it, m in zip(items, multi):
        s = fmpnp.solve_pnp(it[0], it[1], K, np.zeros(4), reference_filename=it[2], reference_2D_points=it[3],
                            reference_keypoints=it[4], use_ransac=True, **kw)
        assert s.success == m.success and s.num_matches == m.num_matches and s.reference_filename == m.reference_filename
        if s.success:
            for f in ("num_inliers", "reference_inliers", "query_inliers", "points_3d", "quaternion", "matrix",
                      "inlier_mask"):
                assert np.asarray(getattr(s, f)).tobytes() == np.asarray(getattr(m, f)).tobytes(), f
    assert multi[0].success and multi[1].success and multi[2].success
    assert (multi[1].inlier_mask == np.flatnonzero(case("noisy300")["planted"])).all()


def test_async_entry_on_a_side_stream():
    probs = [shaped(65, 257), shaped(3, 64), shaped(257, 256)]
    cpu = pnp.ransac_cpu(probs, 8)
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        call = pnp.AsyncRansac(probs, DEV, results_fill=0xAB, mask_fill=0xCD)
        raw = call.read()
        res_bytes = call.results.cpu().numpy()
        mask_bytes = call.mask.cpu().numpy()
    assert_equal([raw[0], raw[2]], [cpu[0], cpu[2]])
    # the problem with M < 4: only its status is written
    size = ctypes.sizeof(_lib.PnpResult)
    off = _lib.PnpResult.status.offset
    untouched = np.full(size, 0xAB, np.uint8)
    untouched[off:off + 4] = np.frombuffer(np.int32(_lib.PNP_TOO_FEW).tobytes(), np.uint8)
    assert (res_bytes[size:2 * size] == untouched).all()
    assert (mask_bytes[65:68] == 0xCD).all()


def test_two_threads_on_two_streams_equal_serial_calls():
    sets = [[shaped(257, 257), shaped(13, 255)], [shaped(866, 255), shaped(65, 256), shaped(5, 257)]]
    serial = [pnp.ransac(ps, DEV) for ps in sets]
    streams = [torch.cuda.Stream(device=DEV) for _ in sets]
    out, errors = [None, None], []

    def work(i):
        try:
            with torch.cuda.stream(streams[i]):
                for _ in range(3):
                    out[i] = pnp.ransac(sets[i], DEV)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for got, want in zip(out, serial):
        assert_equal(got, want)


def test_prediction_feeds_feature_pnp_unchanged():
    N, C, Hf, Wf = 64, 16, 60, 80
    (batch,), img = synth.pipeline_queries(1, 1, N, C, Hf, Wf, device=DEV, seed0=31)
    q, r, truth, K = batch[0]
    X, inl = np.asarray(truth.points_3d), np.asarray(truth.reference_inliers)
    obs, _ = pc.project(K, (0, 0, 0, 0), np.eye(3), np.zeros(3), X)   # the scene's true pose is the identity
    rng = np.random.Generator(np.random.PCG64(9))
    out = np.zeros(N, bool)
    out[rng.permutation(N)[:int(round(0.3 * N))]] = True
    ang, mag = rng.uniform(0, 2 * np.pi, N), rng.uniform(40.0, 100.0, N)
    obs = np.where(out[:, None], obs + np.stack([np.cos(ang), np.sin(ang)], 1) * mag[:, None], obs)
    pred = fmpnp.solve_pnp(obs, X, K, np.zeros(4), 12.0, 10, 12, "ref.jpg", inl, None, True, True, iters=512)
    assert pred.success and (pred.inlier_mask == np.flatnonzero(~out)).all()
    assert np.abs(pred.matrix - np.eye(4)).max() < 1e-6
    R, t, _ = fmpnp.feature_pnp(q, r, pred, K, img, model=fmpnp.sparseFeaturePnP(5))
    assert torch.isfinite(R).all() and torch.isfinite(t).all()
    assert R.shape == (3, 3) and t.numel() == 3
