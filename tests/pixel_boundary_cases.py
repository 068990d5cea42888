"""Points on the boundaries of the pixel rounding and of the texel rescale, shared by
tests/test_pixel_boundary_cpu.py, tests/test_gpu_pixel_boundary.py, tests/test_window_pack.py and
tests/golden/gen_golden.py (case pixel_boundary).  Numpy only: no device, no torch.  Seeded.

Every tier restates three steps of integer geometry (featurePnP/model.py:303-311, :88-89):
p = round_half_even(K (R X + t) / z) - 1, the support test 0 <= p < (W, H) and the texel
floor(p * (Hf, Wf) / (H, W)).  `pixel_model` below is the definition the tiers are compared with: elementwise
numpy in the expression order of transform_pt / project_px (fmpnp_device.h), sequential products, no FMA
(numpy runs one ufunc per operation; `@` and np.dot are never used on these inputs: a BLAS may fuse).

Boundary points.  A point is built from a pose, a K, a target quotient per axis and a class label; its X is
found by stepping coordinates in ulps until the model's quotient EQUALS the target.  Targets are half-integers
k + 0.5 (rint's boundary; k even and odd, ties go to even) moved by OFFSETS ulps, on the x axis, the y axis or
both; the same around the image's edges; z < 0 (not masked by the reference); |z| at EXTREME_DEPTHS; NaN / Inf
coordinates.  The image has the map's size (one pixel per texel), so every one-pixel flip changes the texel.

Maps and fref.  Map channels are small integers (a texel identifier, the column, the row, one), so every sum is
exact in fp64 from fp64, fp32 and (maps of at most 2048 texels) binary16 storage.  Two fref tables go with a
problem: `fref0` = 0, under which a point's cost 0.5 (id^2 + col^2 + row^2 + 1) names its texel (the per-point
checks), and `fref`, the contrast table of the mean-cost checks: a point's own texel (cost 0) and, for every 8th
point, its texel + (0, 2, 2, 0) (0.5 ||e||^2 = 4).  Under it one point on a neighbouring texel, or one support
bit toggled, moves the mean cost of a problem of up to 512 points by more than 1e-3 relative under the squared
and the Geman-McClure loss -- 1e3 times the fp32 tier's 1e-6 (`min_single_point_change` measures it; with
fref = 0 and the saturating Geman-McClure loss a flip would be invisible at any tolerance).

Rescale sweeps.  Points exactly at pixel centres (z = 1, focal length 1024, quotient k + 1 exactly), point i at
pixel (i mod W, i mod H), over the (image, map) sizes of SWEEP_SIZES per axis: d = 1, powers of two, 2^k +- 1,
maps larger than the image, and 65536 x 65535 (products just under 2^32) on a one-row map.
"""
import functools
import math

import numpy as np

SEED = 20261
OFFSETS = (0, 1, -1, 2, -2, 3, -3, 4, -4, 7, -7, 8, -8, 9, -9, 15, -15, 16, -16, 17, -17, 64, -64)
NEAR_OFFSETS = (0, 1, -1)                            # where a reciprocal's product and the division part
SHORT_OFFSETS = (0, 1, -1, 2, -2, 8, -8, 9, -9, 16, -16, 17, -17)   # the groups that claim fewer classes
EDGE_OFFSETS = (0, 1, -1, 2, -2, 9, -9, 17, -17)
EXTREME_DEPTHS = (-1030, -1010, -999, 999, 1010)     # |z| = 2^e * [1, 1.9)
PER_CLASS, PER_NEAR_CLASS = 10, 50   # points attempted per (offset, axis) class (NEAR_OFFSETS: half of all points)
LOUD_EVERY, LOUD = 8, (0.0, 2.0, 2.0, 0.0)           # the contrast fref (module comment)

K_STD = np.array([[400.0, 0.0, 640.0], [0.0, 400.0, 480.0], [0.0, 0.0, 1.0]])
K_OFF = np.array([[48.0, 0.0, 31.25], [0.0, 40.0, 22.75], [0.0, 0.0, 1.0]])      # fx != fy, off-centre
K_SKEW = np.array([[48.0, 0.375, 31.25], [0.0, 40.0, 22.75], [0.0, 0.0, 1.0]])   # project_pc's project_px branch
K_W2 = np.array([[96.0, 0.0, 62.5], [0.0, 80.0, 45.5], [0.0, 0.0, 2.0]])         # K[2][2] = 2: likewise
KS = {"std": K_STD, "off": K_OFF, "skew": K_SKEW, "w2": K_W2}


def _rot_xyz(dx, dy, dz):
    cx, sx, cy, sy, cz, sz = (f(math.radians(a)) for a in (dx, dy, dz) for f in (math.cos, math.sin))
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return np.array([[sum(rz[i, k] * sum(ry[k, l] * rx[l, j] for l in range(3)) for k in range(3))
                      for j in range(3)] for i in range(3)])


POSES = {
    "ident": (np.eye(3), np.zeros(3)),
    "shift": (np.eye(3), np.array([0.3125, -0.171875, 0.40625])),
    "perm": (np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]]), np.array([-0.21875, 0.140625, 0.53125])),
    "general": (_rot_xyz(10.0, -7.0, 20.0), np.array([0.2, -0.12, 0.35])),
}

# group name -> (pose, K, (W, H), axes of the half-integer classes, further classes); the first three claim every
# offset of OFFSETS, the others SHORT_OFFSETS
GROUPS = {
    "ident-std":   ("ident", "std", (64, 48), ("x", "y", "xy"), ("edge", "zneg")),
    "shift-off":   ("shift", "off", (64, 48), ("x", "y", "xy"), ("edge", "zneg")),
    "perm-std":    ("perm", "std", (64, 48), ("x", "y", "xy"), ("edge", "zneg")),
    "general-off": ("general", "off", (64, 48), ("x", "y"), ()),                 # hitting one axis is enough
    "ident-skew":  ("ident", "skew", (64, 48), ("x", "y", "xy"), ("edge",)),
    "shift-w2":    ("shift", "w2", (64, 48), ("x", "y", "xy"), ("edge",)),
    "ident-off-odd": ("ident", "off", (63, 47), ("xy",), ("edge",)),             # odd W and H
    "ident-std-f16": ("ident", "std", (64, 32), ("x", "y"), ()),                 # 2048 texels: binary16 storage
    "extreme":     ("ident", "std", (64, 48), (), ("extreme", "nonfinite")),     # cost mode only
}
FINITE_GROUPS = tuple(g for g in GROUPS if g != "extreme")


def group_offsets(name):
    return OFFSETS if name in ("ident-std", "shift-off", "perm-std") else SHORT_OFFSETS


# --- the model ----------------------------------------------------------------------------------------------
def quotients(R, t, K, X0, X1, X2):
    """The unrounded K (R X + t) / z per axis, as transform_pt / project_px form them."""
    with np.errstate(all="ignore"):
        P = [((R[i, 0] * X0 + R[i, 1] * X1) + R[i, 2] * X2) + t[i] for i in range(3)]
        u = [(K[i, 0] * P[0] + K[i, 1] * P[1]) + K[i, 2] * P[2] for i in range(3)]
        return u[0] / u[2], u[1] / u[2], u


def texels(px, py, sup, W, H, Hf, Wf):
    """indexing_'s (row, col) of supported integer pixels; -1 where unsupported."""
    x = np.where(sup, px, 0).astype(np.int64)
    y = np.where(sup, py, 0).astype(np.int64)
    return np.where(sup, (y * Hf) // H, -1), np.where(sup, (x * Wf) // W, -1)


def pixel_model(R, t, X, K, W, H, Hf, Wf):
    """The reference's pixel, support and texel of every point: dict(qx, qy, px, py (floats: rint(q) - 1, NaN
    kept), sup, row, col (-1 where unsupported), u (the three rows of K P))."""
    R, t, K = (np.asarray(a, dtype=np.float64) for a in (R, t, K))
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    qx, qy, u = quotients(R, t, K, X[:, 0], X[:, 1], X[:, 2])
    with np.errstate(all="ignore"):
        px, py = np.rint(qx) - 1.0, np.rint(qy) - 1.0
        sup = (px >= 0) & (px < W) & (py >= 0) & (py < H)
    row, col = texels(px, py, sup, W, H, Hf, Wf)
    return dict(qx=qx, qy=qy, px=px, py=py, sup=sup, row=row, col=col, u=u)


def fused_pixels(R, t, X, K):
    """(px, py) as pixel_model forms them, but with K P accumulated as a fused chain: c = K_i0 P_0,
    c = fma(K_i1, P_1, c), c = fma(K_i2, P_2, c) (each fma rounded once: exact rationals).  R X + t stays
    sequential.  What the reference's torch.mm(K, P.T) computes through some BLAS kernels ("The
    reference's own K P"); finite points only."""
    from fractions import Fraction
    R, t, K = (np.asarray(a, dtype=np.float64) for a in (R, t, K))
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    P = np.stack([((R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1]) + R[i, 2] * X[:, 2]) + t[i] for i in range(3)], 1)
    u = np.empty_like(P)
    for n in range(len(P)):
        for i in range(3):
            c = K[i, 0] * P[n, 0]
            c = float(Fraction(K[i, 1]) * Fraction(P[n, 1]) + Fraction(c))
            u[n, i] = float(Fraction(K[i, 2]) * Fraction(P[n, 2]) + Fraction(c))
    return np.rint(u[:, 0] / u[:, 2]) - 1.0, np.rint(u[:, 1] / u[:, 2]) - 1.0


def ulp_step(x, j):
    """x moved by j ulps in the direction of the value (x != 0)."""
    x = np.asarray(x, dtype=np.float64)
    v = x.view(np.int64)
    return np.where(x > 0, v + j, v - j).astype(np.int64).view(np.float64)


# --- one boundary point ---------------------------------------------------------------------------------------
_ZN, _XN, _TRIES = 1024, 12, 9


def _build_point(R, t, K, tx, ty, adv, zmag, ty_alt=None):
    """(X, ty) with the model's quotient equal to tx on the axes in `adv` ("x", "y", "xy") -- ty likewise -- or
    None.  ty_alt (both axes, no skew, a pose of 0 / +-1 entries: the axes do not interact): y may take any
    of these targets instead, whichever a depth that reaches tx also reaches.
    zmag: n -> n signed depths.  With a long focal length u = K P lies on a grid coarser than the quotient's
    ulps, so a given depth reaches a given target only with some probability: _ZN depths are tried at once, and
    for each the coordinate that feeds an adversarial axis is stepped +-_XN ulps around its computed value."""
    a, b = (int(np.argmax(np.abs(R[i]))) for i in range(2))
    xn = np.arange(-_XN, _XN + 1)[None, :]
    for attempt in range(_TRIES if adv else 1):
        z = zmag(min(_ZN, 32 * 4 ** attempt) if adv else 1)   # (a short focal length hits at once)
        p1 = (ty * K[2, 2] - K[1, 2]) * z / K[1, 1]
        p0 = ((tx * K[2, 2] - K[0, 2]) * z - K[0, 1] * p1) / K[0, 0]
        d = [p0 - t[0], p1 - t[1], z - t[2]]
        G = [((R[0, i] * d[0] + R[1, i] * d[1]) + R[2, i] * d[2])[:, None] for i in range(3)]
        if not adv:
            return np.array([G[i][0, 0] for i in range(3)]), ty
        with np.errstate(over="ignore"):
            rows = np.isfinite(G[0] * G[1] * G[2])[:, 0] & (G[a][:, 0] != 0) & (G[b][:, 0] != 0)
        if adv == "xy" and ty_alt is not None:
            Gx = list(G)
            Gx[a] = ulp_step(np.where(G[a] == 0, 1.0, G[a]) + 0.0 * xn, xn)
            hit = quotients(R, t, K, *Gx)[0] == tx
            sel = np.nonzero(rows & hit.any(1))[0][:64]
            if not len(sel):
                continue
            Xa = Gx[a][sel, np.argmax(hit[sel], 1)][:, None, None]
            d1 = (ty_alt[None, :] * K[2, 2] - K[1, 2]) * z[sel, None] / K[1, 1] - t[1]
            Xb = (R[0, b] * d[0][sel, None] + R[1, b] * d1) + R[2, b] * d[2][sel, None]
            Xb = ulp_step(np.where(Xb == 0, 1.0, Xb)[:, :, None] + 0.0 * xn[None], xn[None])
            Gy = [G[i][sel][:, :, None] for i in range(3)]
            Gy[a], Gy[b] = Xa, Xb
            qx, qy, _ = quotients(R, t, K, *Gy)
            hit = (qy == ty_alt[None, :, None]) & (qx == tx)
            if hit.any():
                s_, k_, n_ = (int(v[0]) for v in np.nonzero(hit))
                X = [float(G[i][sel[s_], 0]) for i in range(3)]
                X[a], X[b] = float(Xa[s_, 0, 0]), float(Xb[s_, k_, n_])
                return np.array(X), float(ty_alt[k_])
            continue
        if "y" in adv:  # first: with a skewed K the y coordinate feeds u0 too, the x coordinate never u1
            Gy = list(G)
            Gy[b] = ulp_step(np.where(G[b] == 0, 1.0, G[b]) + 0.0 * xn, xn)
            hit = quotients(R, t, K, *Gy)[1] == ty
            rows &= hit.any(1)
            G[b] = Gy[b][np.arange(len(z)), np.argmax(hit, 1)][:, None]
        if "x" in adv:
            Gx = list(G)
            Gx[a] = ulp_step(np.where(G[a] == 0, 1.0, G[a]) + 0.0 * xn, xn)
            qx, qy, _ = quotients(R, t, K, *Gx)
            hit = (qx == tx) & ((qy == ty) if "y" in adv else True)
            rows &= hit.any(1)
            G[a] = Gx[a][np.arange(len(z)), np.argmax(hit, 1)][:, None]
        if rows.any():
            r = int(np.argmax(rows))
            return np.array([float(G[i][r, 0]) for i in range(3)]), ty
    return None


def _half_targets(rng, n, lo, hi, off):
    """n half-integer targets k + 0.5 moved by `off` ulps, k alternating even and odd."""
    k = rng.integers(lo, hi, n)
    k = k - ((k + np.arange(n)) % 2)   # parity alternates with the index
    return ulp_step(k + 0.5, off)


@functools.lru_cache(maxsize=None)
def group(name):
    """The boundary points of GROUPS[name]: dict(name, pose, K_name, R0, t0, K, W, H, Hf, Wf, X [N, 3],
    cls [N] (labels "half:x:+1", "edge:x:W-0.5", "zneg", "extreme:-1010", "nonfinite", ...), off [N] (the
    target's ulp offset, 0 where it has none), tx, ty (targets; NaN where the axis is not adversarial))."""
    pose, kname, (W, H), axes, extra = GROUPS[name]
    R, t = POSES[pose]
    K = KS[kname]
    rng = np.random.Generator(np.random.PCG64([SEED, sorted(GROUPS).index(name)]))
    X, cls, off, txs, tys = [], [], [], [], []

    def zpos(n):
        return rng.uniform(0.5, 60.0, n)

    free_y = K[0, 1] == 0 and set(np.abs(R).ravel()) <= {0.0, 1.0}

    def add(label, o, tx, ty, adv, zmag=zpos):
        alt = ulp_step(np.arange(-3, H + 4) + 0.5, o) if (free_y and label.startswith("half:xy")) else None
        got = _build_point(R, t, K, float(tx), float(ty), adv, zmag, alt)
        if got is None:
            return
        x, ty = got
        X.append(x)
        cls.append(label)
        off.append(o)
        txs.append(tx if "x" in adv else np.nan)
        tys.append(ty if "y" in adv else np.nan)

    def plain(n, size):
        return rng.integers(1, size, n) + rng.choice([0.25, 0.3125, 0.75], n)   # inside, far from a boundary

    for ax in axes:
        for o in group_offsets(name):
            n = PER_NEAR_CLASS if o in NEAR_OFFSETS else PER_CLASS
            hx, hy = _half_targets(rng, n, -3, W + 4, o), _half_targets(rng, n, -3, H + 4, o)
            px_, py_ = plain(n, W), plain(n, H)
            for i in range(n):
                add(f"half:{ax}:{o:+d}", o, hx[i] if "x" in ax else px_[i], hy[i] if "y" in ax else py_[i], ax)
    if "edge" in extra:
        edges = [("x", "-0.5", -0.5), ("x", "0.5", 0.5), ("x", "1.5", 1.5), ("x", "W-0.5", W - 0.5),
                 ("x", "W+0.5", W + 0.5), ("y", "-0.5", -0.5), ("y", "0.5", 0.5), ("y", "1.5", 1.5),
                 ("y", "H-0.5", H - 0.5), ("y", "H+0.5", H + 0.5)]
        for ax, tag, base in edges:
            other = plain(len(EDGE_OFFSETS), H if ax == "x" else W)
            for i, o in enumerate(EDGE_OFFSETS):
                tgt = float(ulp_step(base, o))
                add(f"edge:{ax}:{tag}", o, tgt if ax == "x" else other[i], tgt if ax == "y" else other[i], ax)
    if "zneg" in extra:
        for i, o in enumerate((0, 1, -1, 2, -2, 8, -8, 9, -9, 17, -17)):
            ax = "xy"[i % 2]
            hx, hy = _half_targets(rng, 1, 1, W - 1, o)[0], _half_targets(rng, 1, 1, H - 1, o)[0]
            add("zneg", o, hx if ax == "x" else plain(1, W)[0], hy if ax == "y" else plain(1, H)[0], ax,
                lambda n: -rng.uniform(0.5, 60.0, n))
    if "extreme" in extra:
        for e in EXTREME_DEPTHS:
            def zext(n, e=e):
                return np.ldexp(rng.uniform(1.0, 1.9, n), e) * rng.choice([1.0, 1.0, -1.0], n)
            for i in range(10):     # an ordinary pixel, no nudging (always built)
                add(f"extreme:{e}", 0, plain(1, W)[0], plain(1, H)[0], "", zext)
            for o in (0, 1, -1, 0, 1, -1):   # ... and on the rounding boundary where one can be found
                add(f"extreme:{e}", o, _half_targets(rng, 1, 1, W - 1, o)[0], plain(1, H)[0], "x", zext)
    if "nonfinite" in extra:
        for i in range(24):   # ordinary points beside them, so that the cost is a number
            add("ordinary", 0, plain(1, W)[0], plain(1, H)[0], "")
        for v in (np.nan, np.inf, -np.inf):
            for j in range(3):
                add("ordinary", 0, plain(1, W)[0], plain(1, H)[0], "")
                X[-1][j] = v
                cls[-1] = "nonfinite"
    return dict(name=name, pose=pose, K_name=kname, R0=R, t0=t, K=K, W=W, H=H, Hf=H, Wf=W, X=np.array(X),
                cls=np.array(cls), off=np.array(off, dtype=np.int64), tx=np.array(txs), ty=np.array(tys))


# --- maps, fref, problems -------------------------------------------------------------------------------------
def id_map(Hf, Wf):
    """[4, Hf, Wf] fp64: texel identifier row * Wf + col, column, row, one."""
    row, col = np.meshgrid(np.arange(Hf, dtype=np.float64), np.arange(Wf, dtype=np.float64), indexing="ij")
    return np.stack([row * Wf + col, col, row, np.ones_like(row)])


def colrow_map(Hf, Wf):
    """[4, Hf, Wf] fp64 of the rescale sweeps: column, row, one, zero."""
    row, col = np.meshgrid(np.arange(Hf, dtype=np.float64), np.arange(Wf, dtype=np.float64), indexing="ij")
    return np.stack([col, row, np.ones_like(row), np.zeros_like(row)])


def contrast_fref(fmap, m, loud):
    """The contrast fref (module comment): every point's own texel (an unsupported point's: the texel of its
    pixel clamped into the image, what a wrongly set support bit would read), every LOUD_EVERY-th + loud."""
    C, Hf, Wf = fmap.shape
    n = len(m["sup"])
    with np.errstate(invalid="ignore"):
        cx = np.clip(np.nan_to_num(m["px"], nan=0.0, posinf=1e9, neginf=-1e9), 0, m["W"] - 1).astype(np.int64)
        cy = np.clip(np.nan_to_num(m["py"], nan=0.0, posinf=1e9, neginf=-1e9), 0, m["H"] - 1).astype(np.int64)
    row, col = (cy * Hf) // m["H"], (cx * Wf) // m["W"]
    fref = fmap[:, row, col].T.copy()
    fref[np.arange(n) % LOUD_EVERY == 3] += np.asarray(loud)
    return fref, row, col


def make_problem(name, R0, t0, K, W, H, fmap, X, loud=LOUD, **labels):
    """One problem dict: inputs, the model's answer (`model`), fref0 / fref and the labels."""
    Hf, Wf = fmap.shape[1:]
    m = pixel_model(R0, t0, X, K, W, H, Hf, Wf)
    m["W"], m["H"] = W, H
    fref, crow, ccol = contrast_fref(fmap, m, loud)
    m["clamped_row"], m["clamped_col"] = crow, ccol
    return dict(name=name, R0=np.asarray(R0, dtype=np.float64), t0=np.asarray(t0, dtype=np.float64),
                K=np.asarray(K, dtype=np.float64), im_width=W, im_height=H, fmap=fmap,
                pts3d=np.ascontiguousarray(X, dtype=np.float64), fref0=np.zeros((len(X), fmap.shape[0])), fref=fref,
                model=m, **labels)


def group_problems(name, n=480):
    """GROUPS[name]'s points as problems of exactly n points each (of all its points where it has fewer).  The
    points are taken in a strided order, so every problem holds every class; the last problem wraps round to
    the first points to fill up."""
    g = group(name)
    N = len(g["X"])
    n = min(n, N)
    nprob = -(-N // n)
    order = np.concatenate([np.arange(j, N, nprob) for j in range(nprob)])
    fmap = id_map(g["Hf"], g["Wf"])
    out = []
    for j in range(nprob):
        idx = order[(j * n + np.arange(n)) % N]
        out.append(make_problem(f"{name}[{j}/{nprob}]", g["R0"], g["t0"], g["K"], g["W"], g["H"], fmap, g["X"][idx],
                                group=name, pose=g["pose"], K_name=g["K_name"], cls=g["cls"][idx], off=g["off"][idx]))
    return out


def describe(p, i):
    """Class, pose and K of point i of a problem (failure messages)."""
    m = p["model"]
    return (f"{p['name']} point {i}: class {p['cls'][i]}, pose {p['pose']}, K {p['K_name']}, X {p['pts3d'][i]!r}, "
            f"model q ({m['qx'][i]!r}, {m['qy'][i]!r}) -> pixel ({m['px'][i]}, {m['py'][i]}) supported "
            f"{bool(m['sup'][i])} texel ({m['row'][i]}, {m['col'][i]})")


# --- rescale sweeps ---------------------------------------------------------------------------------------------
SWEEP_SIZES = [(1, 1), (2, 1), (3, 2), (37, 64), (100, 100), (1023, 256), (1024, 256), (1025, 256), (997, 250),
               (1280, 43), (641, 640)]   # (image, map) per axis
SWEEP_F = 1024.0
K_SWEEP = np.array([[SWEEP_F, 0.0, 0.0], [0.0, SWEEP_F, 0.0], [0.0, 0.0, 1.0]])


def _centre_points(px, py):
    """Points whose quotients are exactly (px + 1, py + 1): z = 1, a power-of-two focal length."""
    return np.stack([(px + 1.0) / SWEEP_F, (py + 1.0) / SWEEP_F, np.ones(len(px))], 1)


@functools.lru_cache(maxsize=None)
def sweep_problems():
    """The rescale sweeps as problems of at most 512 points: sweep j takes (W, Wf) = SWEEP_SIZES[j] and
    (H, Hf) = SWEEP_SIZES[(j + 4) % 11], so every size is swept on both axes; then 65536 x 65535."""
    out = []
    n = len(SWEEP_SIZES)
    for j, (W, Wf) in enumerate(SWEEP_SIZES):
        H, Hf = SWEEP_SIZES[(j + 4) % n]
        i = np.arange(max(W, H))
        X = _centre_points(i % W, i % H)
        fmap = colrow_map(Hf, Wf)
        for s, Xs in enumerate(np.array_split(X, -(-len(X) // 512))):   # (near-equal parts: none of one point)
            out.append(make_problem(f"sweep W{W}/{Wf} H{H}/{Hf} [{s}]", np.eye(3), np.zeros(3), K_SWEEP, W, H, fmap,
                                    Xs, loud=(2.0, 2.0, 0.0, 0.0), group="sweep", pose="ident", K_name="sweep",
                                    cls=np.full(len(Xs), "sweep"), off=np.zeros(len(Xs), dtype=np.int64)))
    W, Wf = 65536, 65535
    rng = np.random.Generator(np.random.PCG64([SEED, 99]))
    px = np.unique(np.concatenate([np.arange(512), np.arange(W - 512, W), np.arange(32768 - 256, 32768 + 256),
                                   rng.integers(512, W - 512, 600)]))[:2048]
    fmap = colrow_map(1, Wf)
    for s in range(0, len(px), 512):
        q = px[s:s + 512]
        out.append(make_problem(f"sweep W{W}/{Wf} H1/1 [{s}:]", np.eye(3), np.zeros(3), K_SWEEP, W, 1, fmap,
                                _centre_points(q, np.zeros(len(q))), loud=(2.0, 2.0, 0.0, 0.0), group="sweep",
                                pose="ident", K_name="sweep", cls=np.full(len(q), "sweep"),
                                off=np.zeros(len(q), dtype=np.int64)))
    return out


# --- what a single wrong point does to the mean cost ----------------------------------------------------------
def loss_rho(x, loss):
    """rho of 0.5 ||e||^2 = x (helpers/utils.py:15-38): the squared and the Geman-McClure loss."""
    return x if loss == "squared" else 4.0 * x / (x + 4.0)


def table_cost(p, loss, fref=None):
    """(mean cost over the supported points, per-point rho [N] at each point's (clamped) texel) from the model's
    texel table: what the oracle must return for evaluation 0."""
    m = p["model"]
    fref = p["fref"] if fref is None else fref
    e = p["fmap"][:, m["clamped_row"], m["clamped_col"]].T - fref
    rho = loss_rho(0.5 * (e * e).sum(1), loss)
    return rho[m["sup"]].mean() if m["sup"].any() else float("nan"), rho


def min_single_point_change(p, loss):
    """The smallest relative change of the mean cost when one point moves to one of its 8 neighbouring texels
    (inside the map) or one support bit is toggled."""
    m = p["model"]
    sup = m["sup"]
    base, rho = table_cost(p, loss)
    S, n = rho[sup].sum(), int(sup.sum())
    Hf, Wf = p["fmap"].shape[1:]
    worst = np.inf
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr == 0 and dc == 0:
                continue
            r, c = m["clamped_row"] + dr, m["clamped_col"] + dc
            ok = sup & (r >= 0) & (r < Hf) & (c >= 0) & (c < Wf)
            e = p["fmap"][:, np.clip(r, 0, Hf - 1), np.clip(c, 0, Wf - 1)].T - p["fref"]
            alt = loss_rho(0.5 * (e * e).sum(1), loss)
            if ok.any():
                worst = min(worst, np.abs((S - rho + alt)[ok] / n - base).min() / abs(base))
    if n > 1 and sup.any():
        worst = min(worst, np.abs((S - rho[sup]) / (n - 1) - base).min() / abs(base))
    if (~sup).any():
        worst = min(worst, np.abs((S + rho[~sup]) / (n + 1) - base).min() / abs(base))
    return worst
