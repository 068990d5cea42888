"""Shared generator and numpy reference for the P3P RANSAC + polish tests (test_pnp_cpu.py,
test_gpu_pnp.py): seeded synthetic problems with a planted inlier set, the forward camera model in
numpy, and scipy's Levenberg-Marquardt on the same objective as the polish's reference optimiser.

The tolerances below are measured against the references alone (never against the code under test):

POLISH_RVEC_TOL / POLISH_T_TOL   scipy.optimize.least_squares(method="lm", xtol=ftol=gtol=1e-15) on
    the planted inliers, started from the true pose and from the best hypothesis (R_hyp, t_hyp), differs
    from itself by at most 1.6e-9 in the rotation vector and 3.6e-8 in the translation over the five
    cases (both maxima on tiny13; the others stay below 4e-11 / 2e-9): its own reproducibility, which
    test_pnp_cpu.py re-measures at every run.  The tolerance is 10x that spread: one decimal order for a
    different but convergent iteration.  cost is compared with numpy's sum at the returned pose to
    POLISH_RVEC_TOL relative, plus the sum's own fp64 uncertainty (cost_atol) where the cost is rounding
    noise (exact64).
P3P_TOL   numpy's fp64 reprojection of the true pose on exact64's noise-free points differs from the
    same projection in extended precision by at most 1.8e-13 px over its 64 points (numpy's own error; re-measured at every
    run); x 1e3 for the solver's conditioning gives 1.8e-10, applied to the solution's reprojection of its
    three points (px) and to the entries of R and t of the solution nearest the true pose.
"""
import numpy as np

THRESHOLD = 12.0  # px: the production value (robotcar gin)

POLISH_SPREAD_RVEC, POLISH_SPREAD_T = 1.6e-9, 3.6e-8  # scipy against itself (see above)
POLISH_RVEC_TOL, POLISH_T_TOL = 10 * POLISH_SPREAD_RVEC, 10 * POLISH_SPREAD_T
P3P_REPROJ_NOISE_PX = 1.8e-13  # numpy's fp64 reprojection of the true pose against extended precision, exact64
P3P_TOL = 1e3 * P3P_REPROJ_NOISE_PX

# name: (M, outlier fraction, sigma px, f, distortion, generator seed, iters)
CASES = {
    "exact64": (64, 0.5, 0.0, 400.0, (0.0, 0.0, 0.0, 0.0), 11, 512),
    "tiny13": (13, 0.3, 0.5, 400.0, (0.0, 0.0, 0.0, 0.0), 12, 1024),
    "noisy300": (300, 0.4, 1.0, 400.0, (0.0, 0.0, 0.0, 0.0), 13, 1024),
    "distorted257": (257, 0.4, 1.0, 800.0, (-0.1, 0.02, 1e-3, -1e-3), 14, 1024),
    "robotcar866": (866, 0.6, 1.0, 400.0, (0.0, 0.0, 0.0, 0.0), 15, 5000),
}


def rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th < 1e-300:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def rotvec(R):
    """The rotation vector of a rotation matrix (angles below pi)."""
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2.0
    s = np.linalg.norm(w)
    c = (np.trace(R) - 1.0) / 2.0
    th = np.arctan2(s, c)
    return w * (th / s) if s > 1e-300 else w


def project(K, dist, R, t, X):
    """The forward model of include/fmpnp.h: pixels [M, 2] and depths [M]."""
    P = X @ np.asarray(R).T + np.asarray(t)
    with np.errstate(all="ignore"):
        x, y = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
        k1, k2, p1, p2 = dist
        r2 = x * x + y * y
        rad = 1 + k1 * r2 + k2 * r2 * r2
        xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        return np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], 1), P[:, 2]


def rescore(K, dist, R, t, X, x, threshold=THRESHOLD):
    """(mask, squared errors) of the score's definition in numpy; NaN compares false."""
    px, z = project(K, dist, R, t, X)
    with np.errstate(all="ignore"):
        e2 = ((px - x) ** 2).sum(1)
        return (z > 0) & (e2 <= threshold * threshold), e2


def project_extended(K, R, t, X):
    """The undistorted projection in numpy's extended precision (the measure of project()'s own error)."""
    L = np.longdouble
    P = X.astype(L) @ np.asarray(R).astype(L).T + np.asarray(t).astype(L)
    return np.stack([K[0, 0] * (P[:, 0] / P[:, 2]) + K[0, 2], K[1, 1] * (P[:, 1] / P[:, 2]) + K[1, 2]], 1)


def cost_atol(cost, n):
    """The fp64 uncertainty of a sum of 2 n squared residuals whose entries each carry up to
    2 P3P_REPROJ_NOISE_PX of reprojection rounding (numpy's and the library's):
    |sum (r + d)^2 - sum r^2| <= 2 |r|_1 e + 2 n e^2 <= 2 sqrt(2 n cost) e + 2 n e^2."""
    e = 2 * P3P_REPROJ_NOISE_PX
    return 2 * np.sqrt(2 * n * cost) * e + 2 * n * e * e


def make_case(name):
    """dict(points3d, points2d, K, dist, threshold, iters, seed=0, planted (bool [M]), R_true, t_true)."""
    M, fo, sigma, f, dist, seed, iters = CASES[name]
    return generate(M, fo, sigma, f, dist, seed, iters)


def generate(M, fo, sigma, f, dist, seed, iters=1024):
    rng = np.random.Generator(np.random.PCG64(seed))
    K = np.array([[f, 0.0, 512.0], [0.0, f, 512.0], [0.0, 0.0, 1.0]])
    R = rodrigues(rng.normal(0.0, 0.3, 3))
    t = rng.normal(0.0, 1.0, 3)
    xn = rng.uniform(-472.0 / f, 472.0 / f, (M, 2))
    z = rng.uniform(5.0, 50.0, M)
    Pc = np.concatenate([xn * z[:, None], z[:, None]], 1)
    X = (Pc - t) @ R                      # world = R^T (P - t)
    x0, _ = project(K, dist, R, t, X)
    noise = np.clip(rng.normal(0.0, sigma, (M, 2)), -3.0, 3.0) if sigma > 0 else np.zeros((M, 2))
    n_out = int(round(fo * M))
    out = np.zeros(M, bool)
    out[rng.permutation(M)[:n_out]] = True
    ang, mag = rng.uniform(0.0, 2 * np.pi, M), rng.uniform(40.0, 300.0, M)
    x = np.where(out[:, None], x0 + np.stack([np.cos(ang), np.sin(ang)], 1) * mag[:, None], x0 + noise)
    planted = ~out
    # the planted set under the true pose: inliers within 4.3 px (3 sqrt 2 of clipped noise), outliers at 40 px or more
    _, e2 = rescore(K, dist, R, t, X, x)
    assert (np.sqrt(e2[planted]) <= 4.3).all() and (np.sqrt(e2[out]) >= 40.0 - 1e-9).all()
    return dict(points3d=X, points2d=x, K=K, dist=np.array(dist), threshold=THRESHOLD, iters=iters, seed=0,
                planted=planted, R_true=R, t_true=t)


def problem(case, **over):
    """The fields fmpnp.pnp.ransac / ransac_cpu read, with overrides."""
    p = {k: case[k] for k in ("points3d", "points2d", "K", "dist", "threshold", "iters", "seed")}
    p.update(over)
    return p


def scipy_polish(case, R0, t0, inliers=None):
    """The reference optimiser: scipy's LM on the planted inliers with the forward model.  Returns
    (rotation vector, translation, cost = sum of squared residuals)."""
    from scipy.optimize import least_squares
    idx = case["planted"] if inliers is None else inliers
    X, x = case["points3d"][idx], case["points2d"][idx]

    def fun(p):
        px, _ = project(case["K"], case["dist"], rodrigues(p[:3]), p[3:], X)
        return (px - x).reshape(-1)

    r = least_squares(fun, np.concatenate([rotvec(np.asarray(R0)), np.asarray(t0)]), method="lm", xtol=1e-15,
                      ftol=1e-15, gtol=1e-15)
    return r.x[:3], r.x[3:], float((r.fun ** 2).sum())


def result_bytes(r):
    """Every result field and mask byte of one problem as bytes (for == between tiers)."""
    return b"".join([np.asarray(r[k], np.float64).tobytes() for k in ("R", "t", "R_hyp", "t_hyp", "cost")]
                    + [np.asarray([r[k] for k in ("num_inliers", "best_h", "status", "polish_iters")], np.int32).tobytes(),
                       np.asarray(r["mask"], np.uint8).tobytes()])
