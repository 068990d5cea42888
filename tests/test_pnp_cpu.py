"""P3P RANSAC + polish through the CPU twin (fmpnp_pnp_ransac_cpu, fmpnp_p3p_cpu): the numeric contract
of include/fmpnp.h on planted problems, against numpy's re-scoring and scipy's LM of the same objective.
Tolerances and their provenance: tests/pnp_cases.py."""
import ctypes
import functools

import numpy as np
import pytest

import pnp_cases as pc
from fmpnp import _lib, config, pnp

NAMES = sorted(pc.CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    return pc.make_case(name)


@functools.lru_cache(maxsize=None)
def twin(name):
    return pnp.ransac_cpu([pc.problem(case(name))], n_threads=16)[0]


@functools.lru_cache(maxsize=None)
def scipy_pair(name):
    c, r = case(name), twin(name)
    return pc.scipy_polish(c, c["R_true"], c["t_true"]), pc.scipy_polish(c, r["R_hyp"], r["t_hyp"])


# ---- mask and independent re-scoring ----------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_mask_is_the_planted_set(name):
    c, r = case(name), twin(name)
    assert r["status"] == _lib.PNP_OK
    assert (r["mask"].astype(bool) == c["planted"]).all()
    assert r["num_inliers"] == int(c["planted"].sum())
    assert 0 <= r["best_h"] < c["iters"]


@pytest.mark.parametrize("name", NAMES)
def test_numpy_rescoring_of_the_hypothesis_reproduces_the_mask(name):
    c, r = case(name), twin(name)
    mask, e2 = pc.rescore(c["K"], c["dist"], r["R_hyp"], r["t_hyp"], c["points3d"], c["points2d"])
    assert np.abs(np.sqrt(e2) - pc.THRESHOLD).min() > 1e-6  # no point sits on the threshold
    assert (mask == r["mask"].astype(bool)).all()


# ---- polish against scipy's LM ----------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_scipy_spread_is_within_the_recorded_constants(name):
    (ra, ta, _), (rb, tb, _) = scipy_pair(name)
    print(name, "scipy spread", np.abs(ra - rb).max(), np.abs(ta - tb).max())
    assert np.abs(ra - rb).max() <= pc.POLISH_SPREAD_RVEC
    assert np.abs(ta - tb).max() <= pc.POLISH_SPREAD_T


@pytest.mark.parametrize("name", NAMES)
def test_polish_matches_scipy(name):
    c, r = case(name), twin(name)
    (ra, ta, _), _ = scipy_pair(name)
    dr, dt = np.abs(pc.rotvec(r["R"]) - ra).max(), np.abs(r["t"] - ta).max()
    print(name, "polish vs scipy", dr, dt, "iters", r["polish_iters"])
    assert dr <= pc.POLISH_RVEC_TOL
    assert dt <= pc.POLISH_T_TOL
    assert np.abs(r["R"] @ r["R"].T - np.eye(3)).max() < 1e-12
    # cost: numpy's sum of squares at the returned pose
    px, _ = pc.project(c["K"], c["dist"], r["R"], r["t"], c["points3d"][c["planted"]])
    ref = float(((px - c["points2d"][c["planted"]]) ** 2).sum())
    print(name, "cost", r["cost"], ref)
    assert abs(r["cost"] - ref) <= pc.POLISH_RVEC_TOL * ref + pc.cost_atol(ref, int(c["planted"].sum()))
    # and the polish did not make the hypothesis worse
    px, _ = pc.project(c["K"], c["dist"], r["R_hyp"], r["t_hyp"], c["points3d"][c["planted"]])
    hyp = float(((px - c["points2d"][c["planted"]]) ** 2).sum())
    assert r["cost"] <= hyp + pc.cost_atol(hyp, int(c["planted"].sum()))


# ---- P3P alone --------------------------------------------------------------------------------------
def test_numpy_reprojection_noise_is_within_the_recorded_constant():
    c = case("exact64")
    px, _ = pc.project(c["K"], c["dist"], c["R_true"], c["t_true"], c["points3d"])
    err = float(np.abs(px - pc.project_extended(c["K"], c["R_true"], c["t_true"], c["points3d"])).max())
    print("numpy reprojection noise", err)
    assert err <= pc.P3P_REPROJ_NOISE_PX


def test_p3p_returns_the_true_pose():
    c = case("exact64")
    idx = np.flatnonzero(c["planted"])
    for k in range(0, len(idx) - 2, 3):
        tri = idx[k:k + 3]
        y = np.concatenate([(c["points2d"][tri] - 512.0) / 400.0, np.ones((3, 1))], 1)
        y *= np.array([[1.0], [2.5], [0.3]])  # any positive length
        R, t = pnp.p3p_cpu(y, c["points3d"][tri])
        assert 1 <= len(R) <= 4
        near = []
        for Ri, ti in zip(R, t):
            assert np.isfinite(Ri).all() and np.isfinite(ti).all()
            P = c["points3d"][tri] @ Ri.T + ti
            assert (P[:, 2] > 0).all()                                   # positive depth ...
            lam = np.linalg.norm(P, axis=1)
            yn = y / np.linalg.norm(y, axis=1, keepdims=True)
            assert np.abs(P - lam[:, None] * yn).max() <= 1e-9 * lam.max()   # ... on the bearings
            px, _ = pc.project(c["K"], c["dist"], Ri, ti, c["points3d"][tri])
            assert np.abs(px - c["points2d"][tri]).max() <= pc.P3P_TOL
            near.append(max(np.abs(Ri - c["R_true"]).max(), np.abs(ti - c["t_true"]).max()))
        print(k, len(R), min(near))
        assert min(near) <= pc.P3P_TOL


@pytest.mark.parametrize("kind", ["collinear", "two_equal"])
def test_p3p_degenerate_triples_give_no_nan_pose(kind):
    X = np.array([[0.0, 0.0, 10.0], [1.0, 2.0, 12.0], [2.0, 4.0, 14.0]])
    if kind == "two_equal":
        X = np.array([[0.0, 0.0, 10.0], [0.0, 0.0, 10.0], [2.0, -1.0, 14.0]])
    y = X / X[:, 2:3]
    R, t = pnp.p3p_cpu(y, X)
    assert np.isfinite(R).all() and np.isfinite(t).all()  # 0 solutions or finite ones


# ---- determinism and the twin's threading -----------------------------------------------------------
def test_thread_count_does_not_change_a_byte():
    p = pc.problem(case("noisy300"))
    ref = pc.result_bytes(pnp.ransac_cpu([p], 1)[0])
    for nt in (3, 16):
        assert pc.result_bytes(pnp.ransac_cpu([p], nt)[0]) == ref
    assert ref == pc.result_bytes(twin("noisy300"))


def test_batch_position_does_not_change_a_byte():
    a, b, t13 = pc.problem(case("noisy300")), pc.problem(case("distorted257")), pc.problem(case("tiny13"))
    out = pnp.ransac_cpu([a, t13, a, b], 4)
    assert pc.result_bytes(out[0]) == pc.result_bytes(out[2]) == pc.result_bytes(twin("noisy300"))
    assert pc.result_bytes(out[1]) == pc.result_bytes(twin("tiny13"))
    assert pc.result_bytes(out[3]) == pc.result_bytes(twin("distorted257"))


def test_another_seed_gives_another_best_hypothesis():
    c = case("noisy300")
    r = pnp.ransac_cpu([pc.problem(c, seed=12345)], 4)[0]
    assert r["best_h"] != twin("noisy300")["best_h"]
    assert (r["mask"].astype(bool) == c["planted"]).all()


# ---- edges ------------------------------------------------------------------------------------------
def exact_points(M, seed=5):
    c = pc.generate(M, 0.0, 0.0, 400.0, (0.0, 0.0, 0.0, 0.0), seed, iters=64)
    assert c["planted"].all()
    return c


def test_three_points_set_the_too_few_status():
    c = exact_points(3)
    r = pnp.ransac_cpu([pc.problem(c)], 1)[0]
    assert r["status"] == _lib.PNP_TOO_FEW and r["num_inliers"] == 0


@pytest.mark.parametrize("M", [4, 5])
def test_minimal_problems(M):
    c = exact_points(M)
    r = pnp.ransac_cpu([pc.problem(c)], 2)[0]
    assert r["status"] == _lib.PNP_OK and r["num_inliers"] == M and r["mask"].all()
    px, _ = pc.project(c["K"], c["dist"], r["R"], r["t"], c["points3d"])
    assert np.abs(px - c["points2d"]).max() < 1e-6


def test_one_iteration():
    c = case("noisy300")
    r = pnp.ransac_cpu([pc.problem(c, iters=1)], 4)[0]
    assert r["best_h"] in (0, -1)
    assert r["status"] in (_lib.PNP_OK, _lib.PNP_NO_MODEL, _lib.PNP_POLISH_FAILED)
    mask, _ = pc.rescore(c["K"], c["dist"], r["R_hyp"], r["t_hyp"], c["points3d"], c["points2d"])
    if r["best_h"] == 0:
        assert (mask == r["mask"].astype(bool)).all() and r["num_inliers"] == mask.sum()


def test_collinear_points_set_the_no_model_status():
    s = np.arange(40, dtype=np.float64)
    X = np.stack([1.0 + s, 2.0 + 2.0 * s, 30.0 + 4.0 * s], 1)  # (exactly representable: exact cross products)
    K = np.array([[400.0, 0.0, 512.0], [0.0, 400.0, 512.0], [0.0, 0.0, 1.0]])
    x, _ = pc.project(K, (0, 0, 0, 0), np.eye(3), np.zeros(3), X)
    r = pnp.ransac_cpu([dict(points3d=X, points2d=x, K=K, dist=np.zeros(4), threshold=12.0, iters=256, seed=0)], 2)[0]
    assert r["status"] == _lib.PNP_NO_MODEL and r["num_inliers"] == 0 and r["best_h"] == -1 and not r["mask"].any()


def test_non_finite_points_stay_outside_the_mask():
    c = case("noisy300")
    inl = np.flatnonzero(c["planted"])
    X, x = c["points3d"].copy(), c["points2d"].copy()
    X[inl[3], 1] = np.nan
    x[inl[7], 0] = np.inf
    r = pnp.ransac_cpu([pc.problem(c, points3d=X, points2d=x)], 8)[0]
    want = c["planted"].copy()
    want[[inl[3], inl[7]]] = False
    assert r["status"] == _lib.PNP_OK
    assert (r["mask"].astype(bool) == want).all() and r["num_inliers"] == want.sum()
    assert np.isfinite(r["R"]).all() and np.isfinite(r["t"]).all() and np.isfinite(r["cost"])


def all_outlier_problem():
    rng = np.random.Generator(np.random.PCG64(77))
    c = exact_points(60, seed=6)
    x = rng.uniform(40.0, 984.0, (60, 2))  # observations unrelated to the points
    return c, pc.problem(c, points2d=x, iters=256)


def test_all_outliers_fail_the_minimum_inliers():
    c, p = all_outlier_problem()
    r = pnp.ransac_cpu([p], 4)[0]
    assert r["num_inliers"] < 12
    pred = pnp.solve_pnp_cpu(p["points2d"], p["points3d"], p["K"], p["dist"], 12.0, 10, 12, "ref.jpg",
                             p["points2d"], None, True, True, iters=256)
    assert pred.success is False and pred.num_matches == 60 and pred.matrix is None


# ---- Python solve_pnp_cpu against solve_pnp.py's branches ------------------------------------------------
def call(c, minimum_matches=10, minimum_inliers=12, return_masked=True, dist=None, **kw):
    ref2d = c["points2d"][:, None, :] + 1000.0  # the reference's [M, 1, 2] reprojected points (any values)
    return pnp.solve_pnp_cpu(c["points2d"][:, None, :], c["points3d"], c["K"], c["dist"] if dist is None else dist,
                             12.0, minimum_matches, minimum_inliers, "ref.jpg", ref2d, "kp", True, return_masked,
                             iters=c["iters"], **kw), ref2d


def test_prediction_fields_masked():
    c, r = case("noisy300"), twin("noisy300")
    pred, ref2d = call(c)
    assert pred._fields == ("success", "num_matches", "num_inliers", "reference_inliers", "query_inliers", "points_3d",
                            "quaternion", "matrix", "reference_filename", "reference_keypoints", "inlier_mask")
    idx = np.flatnonzero(c["planted"])
    assert pred.success is True and pred.num_matches == 300 and pred.num_inliers == len(idx)
    assert pred.inlier_mask.dtype == np.int32 and (pred.inlier_mask == idx).all()  # ascending indices
    assert (pred.reference_inliers == ref2d[idx]).all()
    assert (pred.query_inliers == c["points2d"][idx]).all() and pred.query_inliers.shape == (len(idx), 2)
    assert (pred.points_3d == c["points3d"][idx]).all()
    assert pred.matrix.shape == (4, 4) and (pred.matrix[:3, :3] == r["R"]).all() and (pred.matrix[:3, 3] == r["t"]).all()
    assert (pred.matrix[3] == [0, 0, 0, 1]).all()
    from fmpnp.matrix_utils import matrix_quaternion
    assert (pred.quaternion == matrix_quaternion(pred.matrix)).all()
    assert pred.reference_filename == "ref.jpg" and pred.reference_keypoints == "kp"


def test_prediction_fields_unmasked():
    c = case("noisy300")
    pred, ref2d = call(c, return_masked=False)
    assert pred.success and pred.reference_inliers is ref2d and (pred.points_3d == c["points3d"]).all()
    assert pred.query_inliers.shape == (300, 2) and (pred.inlier_mask == np.flatnonzero(c["planted"])).all()


def test_minimum_matches_and_minimum_inliers():
    c = case("noisy300")
    pred, _ = call(c, minimum_matches=300)           # M <= minimum_matches: no launch
    assert pred.success is False and pred.num_matches == 300 and pred.num_inliers is None and pred.inlier_mask is None
    assert pred.reference_filename == "ref.jpg" and pred.reference_keypoints == "kp"
    n = int(c["planted"].sum())
    assert call(c, minimum_inliers=n)[0].success is True
    assert call(c, minimum_inliers=n + 1)[0].success is False


def test_configure_bindings():
    c = case("tiny13")
    saved = config.solve_pnp_kwargs()
    try:
        with pytest.raises(TypeError):
            pnp.solve_pnp_cpu(c["points2d"], c["points3d"], c["K"], c["dist"])
        config.configure(solve_pnp_reprojection_threshold=12.0, solve_pnp_minimum_matches=5, solve_pnp_minimum_inliers=5,
                         solve_pnp_return_masked=True, solve_pnp_iters=1024, solve_pnp_seed=0)
        pred = pnp.solve_pnp_cpu(c["points2d"], c["points3d"], c["K"], c["dist"], reference_2D_points=c["points2d"])
        assert pred.success and (pred.inlier_mask == np.flatnonzero(c["planted"])).all()
        assert (pred.matrix[:3, 3] == twin("tiny13")["t"]).all()
        with pytest.raises(KeyError):
            config.configure(solve_pnp_confidence=0.99)
    finally:
        config.configure(**{"solve_pnp_" + k: v for k, v in saved.items()})


def test_five_distortion_coefficients_raise():
    c = case("tiny13")
    with pytest.raises(ValueError):
        call(c, dist=np.zeros(5))
    with pytest.raises(ValueError):
        call(c, dist=np.zeros((2, 2, 1)))
    L = _lib.load()
    arr, keep, total = pnp.make_problems([pc.problem(c)])
    arr[0].n_dist = 5
    res, mask = (_lib.PnpResult * 1)(), np.zeros(total, np.uint8)
    assert L.fmpnp_pnp_ransac_cpu(arr, 1, res, mask.ctypes.data, total, 1) == -1
    assert L.fmpnp_pnp_ransac(arr, 1, 0, res, mask.ctypes.data, total, None) == -1  # (before any device call)


# ---- ABI ----------------------------------------------------------------------------------------------
def test_abi_has_the_pnp_symbols():
    L = _lib.load()
    for f in ("fmpnp_pnp_workspace_size", "fmpnp_pnp_ransac_async", "fmpnp_pnp_ransac", "fmpnp_pnp_ransac_cpu",
              "fmpnp_p3p_cpu"):
        assert hasattr(L, f), f
    assert L.fmpnp_abi_version() == 4
    assert L.fmpnp_pnp_workspace_size(10) == 80
    assert ctypes.sizeof(_lib.PnpProblem) == 160 and ctypes.sizeof(_lib.PnpResult) == 216


@pytest.mark.parametrize("name,cls", [("fmpnp_pnp_problem", _lib.PnpProblem), ("fmpnp_pnp_result", _lib.PnpResult)])
def test_pnp_struct_layout_matches_c(name, cls, tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = [f'printf("%zu\\n", sizeof({name}));'] + [f'printf("%zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fmpnp.h"\nint main(void){\n' + "\n".join(lines)
                   + "\nreturn 0;}\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(cls)
    for (f, _), off in zip(cls._fields_, vals[1:]):
        assert getattr(cls, f).offset == off, f
