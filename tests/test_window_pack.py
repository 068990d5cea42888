"""Windowed f-only packs (fmpnp_pack_features_f_window_batch, fmpnp.pipeline window=r).

The refinement reads only the 3x3 neighbourhoods of the texels its points visit
(featurePnP/model.py:303-311 projection, :74-97 indexing_), so the pipeline may pack only the
texels near each point's texel at the initial pose (optimize_feature_pnp.py:57-61 packs all of
them).  The LM kernel checks every gather against the window's plane 1 and stops a problem that
leaves it (FMPNP_STATUS_WINDOW); the pipeline packs such queries in full and refines them again.

Checked here: the packed texels equal the full pack's, plane 1 lies inside plane 0 and holds
every supported point's initial texel; the windowed pipeline's results equal the fully packed
pipeline's bit for bit on the easy and the hard start, including radii small enough that many
queries leave their window and take the refill.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import fmpnp  # noqa: E402
from fmpnp import _lib, refine as rf, synth  # noqa: E402  (no skip: a missing HIP library must fail)
from fmpnp.pipeline import RefinePipeline  # noqa: E402

import pixel_boundary_cases as pb  # noqa: E402

DEV = torch.device("cuda", 0)


def _initial_texels(X, K, R, t, W, H, Hf, Wf):
    """The texels of the supported points at (R, t): the sequential model of tests/pixel_boundary_cases.py
    (elementwise products in transform_pt / project_px's order; no `@`: a BLAS may fuse)."""
    m = pb.pixel_model(R, t, X, K, W, H, Hf, Wf)
    return m["row"][m["sup"]], m["col"][m["sup"]]


def _squares(row, col, r, Hf, Wf):
    """The union of the squares of radius r (clipped to the map) around the texels; r < 0: nothing."""
    w = np.zeros((Hf, Wf), dtype=bool)
    if r >= 0:
        for y, x in zip(row, col):
            w[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1] = True
    return w


def _boundary_queries(n_queries):
    """Queries on the boundary points of tests/pixel_boundary_cases.py at one pixel per texel (150 points each:
    more than 100 supported, a radius-2 window that leaves part of the 48 x 64 map unmarked)."""
    qs = []
    for name in ("ident-std", "perm-std", "ident-skew")[:n_queries]:
        p = pb.group_problems(name, 150)[0]
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = p["R0"], p["t0"]
        fmap = torch.from_numpy(p["fmap"]).float().to(DEV)
        qs.append((fmap, fmap[None], synth.QueryPrediction(p["pts3d"], None, T), p["K"]))
    return qs, (64, 48)


def _window_pack(qs, W, H, radius, dt):
    """fmpnp_pack_features_f_window_batch on the queries, over outputs of NaN and window maps of 7: (the full
    f-only packs, the windowed outputs, the window maps)."""
    n = len(qs)
    C, Hf, Wf = qs[0][0].shape
    cs = (C + 3) // 4 * 4
    full = [rf.pack_features(q[0], storage=torch.float32, device=DEV, layout="f").buf for q in qs]
    outs = [torch.full((Hf, Wf, cs), float("nan"), device=DEV) for _ in range(n)]
    wins = [torch.full((2, Hf, Wf), 7, dtype=torch.uint8, device=DEV) for _ in range(n)]
    pts = [torch.as_tensor(np.asarray(q[2].points_3d), dtype=torch.float64, device=DEV) for q in qs]
    desc = np.zeros(n, dtype=rf.PROBLEM_DTYPE)
    desc["feat"] = [o.data_ptr() for o in outs]
    desc["fref"] = desc["feat"]
    desc["pts3d"] = [p.data_ptr() for p in pts]
    desc["window"] = [w.data_ptr() for w in wins]
    desc["Hf"], desc["Wf"], desc["cstride"], desc["c_end"], desc["ld_ref"] = Hf, Wf, cs, C, cs
    desc["N"] = [p.shape[0] for p in pts]
    desc["im_width"], desc["im_height"] = W, H
    desc["K"] = np.stack([np.asarray(q[3], np.float64).reshape(9) for q in qs])
    desc["R0"] = np.stack([np.asarray(q[2].matrix)[:3, :3].reshape(9) for q in qs])
    desc["t0"] = np.stack([np.asarray(q[2].matrix)[:3, 3] for q in qs])
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(DEV)
    vp = ctypes.c_void_p
    rc = _lib.load().fmpnp_pack_features_f_window_batch(
        vp(d_desc.data_ptr()), vp(desc.ctypes.data), n, (vp * n)(*[q[0].data_ptr() for q in qs]),
        _lib.F64 if dt == "f64" else _lib.F32, radius,
        _lib.stream_ptr(DEV))
    _lib.check(rc, "window pack")
    torch.cuda.synchronize()
    return full, outs, wins


def _check_window_item(q, full, out, win, W, H, radius):
    """One query's window map and windowed pack against the model's texels and the full pack; returns (the
    supported points' rows, the window map)."""
    _, Hf, Wf = q[0].shape
    w = win.cpu().numpy()
    assert set(np.unique(w)) <= {0, 1}
    assert not (w[1] & ~w[0]).any()  # plane 1 (3x3 neighbourhood packed) inside plane 0
    T = np.asarray(q[2].matrix)
    row, col = _initial_texels(np.asarray(q[2].points_3d), np.asarray(q[3]), T[:3, :3], T[:3, 3], W, H, Hf, Wf)
    assert w[1][row, col].all()
    # exactly the squares around the model's texels (containment alone passes a one-texel flip)
    np.testing.assert_array_equal(w[0].astype(bool), _squares(row, col, radius, Hf, Wf))
    np.testing.assert_array_equal(w[1].astype(bool), _squares(row, col, radius - 1, Hf, Wf))
    # interior of plane 1: the whole 3x3 neighbourhood (clipped to the map) is in plane 0
    for y, x in zip(*np.nonzero(w[1])):
        assert w[0][max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].all()
    m = torch.from_numpy(w[0].astype(bool)).to(DEV)
    assert torch.equal(out[m], full[m])           # packed texels: the full pack's bits
    assert torch.isnan(out[~m]).all()             # nothing else written
    return row, w


# (Wf = 43: no 16-byte column quads, the per-texel loads and window reads; fp64 CHW input: the converting
# loads; Hf = 30: a last tile of two rows; C = 37: a partial channel tile and a zero-padded stride)
# (Wf_ = "boundary": the points of tests/pixel_boundary_cases.py on rint's boundaries, one pixel per texel -- a marker
# that rounds one pixel differently from the reference marks a neighbouring texel)
@pytest.mark.parametrize("radius,Wf_,dt", [(2, 44, "f32"), (5, 44, "f32"), (2, 43, "f32"), (5, 44, "f64"),
                                           (2, 43, "f64"), (2, "boundary", "f32")])
def test_window_pack_writes_exactly_the_marked_texels(radius, Wf_, dt):
    if Wf_ == "boundary":
        qs, (W, H) = _boundary_queries(3)
    else:
        batches, (W, H) = synth.pipeline_queries(1, 3, N=200, C=37, Hf=30, Wf=Wf_, device=DEV, seed0=70)
        qs = batches[0]
    if dt == "f64":
        qs = [(a.double(), b, p, k) for (a, b, p, k) in qs]
    full, outs, wins = _window_pack(qs, W, H, radius, dt)
    for i, q in enumerate(qs):
        row, w = _check_window_item(q, full[i], outs[i], wins[i], W, H, radius)
        assert len(row) > 100
        assert 0.05 < w[0].mean() < 1.0


def test_window_pack_over_more_than_one_item_table():
    """65 problems in one call: the item table of the pack's kernel holds 64, so the call makes two launches and
    the last problem is the second table's only item.  C = 5 (stride 8), 6 x 9 texels, 3 points each, radius 2.
    The poses are chosen here: point 0 is built to project inside the image at its problem's pose, the other
    two may fall outside it (unsupported: no square)."""
    n, C, Hf, Wf, W, H, radius = 65, 5, 6, 9, 36, 24, 2
    rng = np.random.default_rng(65)
    g = torch.Generator().manual_seed(65)
    K = np.array([[30.0, 0.0, 18.0], [0.0, 30.0, 12.0], [0.0, 0.0, 1.0]])
    qs = []
    for i in range(n):
        a = 0.02 * (i - 32)
        R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        t = np.array([0.01 * (i % 5), -0.01 * (i % 3), 0.1])
        # pixel targets (the model subtracts 1): point 0 well inside, the others up to 10 pixels outside
        u = np.concatenate([rng.uniform(3.0, W - 2.0, 1), rng.uniform(-10.0, W + 10.0, 2)])
        v = np.concatenate([rng.uniform(3.0, H - 2.0, 1), rng.uniform(-10.0, H + 10.0, 2)])
        z = rng.uniform(2.0, 6.0, 3)
        P = np.stack([(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z], 1)
        X = (P - t) @ R                                    # R^T (P - t), row-wise
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        fmap = torch.randn((C, Hf, Wf), generator=g).to(DEV)
        qs.append((fmap, fmap[None], synth.QueryPrediction(X, None, T), K))
    full, outs, wins = _window_pack(qs, W, H, radius, "f32")
    for i, q in enumerate(qs):
        row, _ = _check_window_item(q, full[i], outs[i], wins[i], W, H, radius)
        assert len(row) >= 1, i


def _queries(init, nb, qb, seed0):
    batches, img = synth.pipeline_queries(nb, qb, 512, 256, 240, 320, device=DEV, seed0=seed0)
    if init != "easy":
        R0, t0 = synth.INITS[init]
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R0, t0
        batches = [[(a, b, p._replace(matrix=T), k) for (a, b, p, k) in qs] for qs in batches]
    return batches, img


def _pipe(img, window):
    return RefinePipeline(img, storage=torch.float32, depth=2, window=window,
                          model_kwargs=dict(n_iters=50, loss_fn=fmpnp.geman_mcclure_loss, lambda_=0.01,
                                            ratio_threshold=None))


@pytest.mark.parametrize("init", ["easy", "hard"])
def test_windowed_pipeline_equals_full_pack(init):
    """window = 6 (the bench's radius) and window = 2 (most queries leave it and are refilled):
    every query's result equals the fully packed pipeline's bit for bit."""
    batches, img = _queries(init, 2, 12, 900)
    base = _pipe(img, None).run(batches)
    for radius in (6, 2):
        pipe = _pipe(img, radius)
        out = pipe.run(batches)
        for b0, b1 in zip(base, out):
            for r0, r1 in zip(b0, b1):
                assert np.array_equal(r0["R"], r1["R"]) and np.array_equal(r0["t"], r1["t"])
                for k in ("best_cost", "initial_cost", "n_evals", "n_steps", "best_num_inliers", "status",
                          "texel_gathers"):
                    assert r0[k] == r1[k] or (k.endswith("cost") and np.isnan(r0[k]) and np.isnan(r1[k])), k
                assert r1["status"] & _lib.STATUS_WINDOW == 0
        if radius == 2:
            assert pipe.refills > 0  # the refill path ran
        print(init, radius, "refills", pipe.refills)


def test_window_miss_stops_the_problem_with_its_status():
    """A radius-2 window around the easy start: the LM reports FMPNP_STATUS_WINDOW for a query
    whose points move more than one texel (the pipeline's refill input)."""
    batches, img = _queries("easy", 1, 8, 950)
    pipe = _pipe(img, 2)
    batch, keep, err = pipe._prepare(batches[0], 0)
    torch.cuda.synchronize()  # the prep stream's descriptor upload, packs and gathers are done
    batch.launch(_lib.stream_ptr(DEV))
    res = batch.results()
    flagged = [r for r in res if r["status"] & _lib.STATUS_WINDOW]
    assert flagged, [r["status"] for r in res]
    base = _pipe(img, None).run(batches)[0]
    # unflagged queries are already the full pack's results
    for r, b in zip(res, base):
        if not r["status"] & _lib.STATUS_WINDOW:
            assert np.array_equal(r["R"], b["R"]) and r["best_cost"] == b["best_cost"]


def test_pipeline_channel_levels_equal_level_by_level_runs():
    """RefinePipeline(levels=...) (multilevel_optimization's channel pyramid, model.py:178-213,
    poses chained on the device) equals running each level as its own pipeline pass, the next
    level's initial pose taken from the previous level's results on the host."""
    levels = [(32, 64), (8, 32), (0, 8)]
    batches, img = synth.pipeline_queries(2, 5, N=128, C=64, Hf=48, Wf=64, device=DEV, seed0=1300)
    kw = dict(n_iters=20, loss_fn=fmpnp.geman_mcclure_loss, lambda_=0.01, ratio_threshold=None)
    chained = RefinePipeline(img, storage=torch.float32, depth=2, levels=levels, model_kwargs=kw).run(batches)
    cur = batches
    for lv in levels:
        out = RefinePipeline(img, storage=torch.float32, depth=2, levels=[lv], model_kwargs=kw).run(cur)
        nxt = []
        for qs, rs in zip(cur, out):
            row = []
            for (a, b, p, k), r in zip(qs, rs):
                T = np.eye(4)
                T[:3, :3], T[:3, 3] = r["R"], r["t"]
                row.append((a, b, p._replace(matrix=T), k))
            nxt.append(row)
        cur = nxt
    for b0, b1 in zip(chained, out):
        for r0, r1 in zip(b0, b1):
            assert np.array_equal(r0["R"], r1["R"]) and np.array_equal(r0["t"], r1["t"])
            assert r0["best_cost"] == r1["best_cost"] and r0["n_evals"] == r1["n_evals"]
    with pytest.raises(ValueError):
        RefinePipeline(img, storage=torch.float32, levels=levels, window=5, model_kwargs=kw)
