"""NaN / Inf inputs through the HIP refiner: the reference's goldens (golden_io.NONFINITE_CASES),
every LM kernel specialisation with poisoned problems in its batch, and the state one workgroup
carries from one problem to the next.

The reference breaks out of its loop on a NaN step (featurePnP/model.py:411-413) and returns
R_best; a NaN trial cost is accepted on the way there and never becomes the best; an Inf texel
gives a rejected trial and the run goes on (tests/nonfinite_checks.py).  In the kernel these pass
through the accept / reject / bookkeeping tail, the memoised sums, the speculative gathers, the
ratio test's limit and the per-workgroup state (the `nan` word of the step scalars, the
linearisation cache, the memo columns) -- none of which a finite input enters.

Tolerances are the suite's: fp64 texels -- identical status and counts, NaN / Inf at the same
indices, finite costs within 1e-10 relative, poses within 1e-9; fp32 texels -- identical status,
counts, support and NaN / Inf positions, finite costs within 1e-6 relative, pose within
1e-4 rad / 1e-4 m (tests/test_variant_coverage.py).
"""
import warnings
from collections import namedtuple

import numpy as np
import pytest
import torch

import nonfinite_checks as nf
import oracle.oracle as orc
from golden_io import (NONFINITE_FORWARD_CASES, NONFINITE_PYRAMID_CASES, NONFINITE_RATIO_CASES, case, poisoned_maps)

pytestmark = pytest.mark.gpu

import fmpnp  # noqa: E402  (no skip: a missing HIP library must fail)
from fmpnp import _lib, refine as rf, synth  # noqa: E402
from fmpnp.pipeline import RefinePipeline  # noqa: E402
from variant_recipes import (C, HF, ITERS, LOSSES, M512, N_512, N_PTS, RECIPES, WF,  # noqa: E402
                             case_key, info_key)

DEV = "cuda:0"
LOSS = {"squared": _lib.SQUARED, "huber": _lib.HUBER, "cauchy": _lib.CAUCHY, "geman_mcclure": _lib.GEMAN_MCCLURE}
LOSS_FN = {"squared": fmpnp.squared_loss, "huber": fmpnp.huber_loss, "cauchy": fmpnp.cauchy_loss,
           "geman_mcclure": fmpnp.geman_mcclure_loss}
STORAGE = {"f32": torch.float32, "f64": torch.float64}
CODE = {"f32": _lib.F32, "f64": _lib.F64}
QUIET = _lib.STATUS_HELPER_WAIT  # informational and timing dependent: not part of a result


# --------------------------------------------------------------------------------------------
# 3. the reference's goldens
# --------------------------------------------------------------------------------------------
_GOLD = {}


def _golden_problem(name, dt, **slice_kw):
    """(problem, inputs, meta, golden) of a non-finite golden case packed with `dt` texels."""
    key = (name, dt)
    if key not in _GOLD:
        inp, meta, gold = case(name)
        f, gx, gy = poisoned_maps(inp, meta, orc.sobel)
        feats = rf.pack_features(torch.from_numpy(f), torch.from_numpy(gx), torch.from_numpy(gy), storage=STORAGE[dt],
                                 device=DEV)
        _GOLD[key] = (feats, inp, meta, gold)
    feats, inp, meta, gold = _GOLD[key]
    prob = rf.make_problem(feats, torch.from_numpy(inp["fref"]), inp["pts3d"], inp["K"], inp["im_width"],
                           inp["im_height"], slice_kw.pop("R0", inp["R0"]), slice_kw.pop("t0", inp["t0"]), **slice_kw)
    return prob, inp, meta, gold


def _golden_options(meta, dt, **kw):
    return rf.make_options(meta["n_iters"], meta["lambda0"], LOSS[meta["loss"]], 0.0, meta.get("ratio_threshold"),
                           dtype=CODE[dt], **kw)


def _oracle_of_golden(name):
    inp, meta, gold = case(name)
    f, gx, gy = poisoned_maps(inp, meta, orc.sobel)
    p = orc.make_problem(inp["pts3d"], inp["fref"], f, gx, gy, inp["K"], inp["im_width"], inp["im_height"],
                         inp["R0"], inp["t0"])
    return orc.forward(p, orc.make_options(meta["n_iters"], meta["lambda0"], meta["loss"],
                                           meta.get("ratio_threshold")), meta["n_iters"] + 1)


def check_against_oracle(res, tr, ores, otr, dt, what):
    """A device result against the oracle on the same (poisoned) inputs: the assertions of the
    golden comparison (nonfinite_checks.check_forward), the oracle in the golden's place."""
    st = res["status"] & ~QUIET
    assert st == {"nan": _lib.STATUS_NAN, "ok": 0}[ores["status"]], (what, res["status"], ores["status"])
    for k in ("n_evals", "n_steps", "n_accepted", "has_best", "best_num_inliers"):
        assert res[k] == ores[k], (what, k, res[k], ores[k])
    nf.assert_same_nonfinite(tr["cost"], otr["cost"], what)
    np.testing.assert_array_equal(tr["n_supported"], otr["n_supported"], err_msg=what)
    np.testing.assert_array_equal(tr["n_kept"], otr["n_kept"], err_msg=what)
    rtol = 1e-10 if dt == "f64" else 1e-6
    np.testing.assert_allclose(tr["cost"], otr["cost"], rtol=rtol, atol=0, equal_nan=True, err_msg=what)
    np.testing.assert_allclose(res["best_cost"], ores["best_cost"], rtol=rtol, atol=0, equal_nan=True, err_msg=what)
    if dt == "f64":
        np.testing.assert_allclose(res["R"], ores["R"], rtol=0, atol=1e-9, err_msg=what)
        np.testing.assert_allclose(res["t"], ores["t"], rtol=0, atol=1e-9, err_msg=what)
    else:
        assert nf.rot_angle(res["R"], ores["R"]) < 1e-4, what
        assert np.linalg.norm(res["t"] - ores["t"]) < 1e-4, what


GOLDEN_PARAMS = [(n, d) for n in NONFINITE_FORWARD_CASES + NONFINITE_RATIO_CASES for d in ("f64", "f32")]


@pytest.mark.parametrize("name,dt", GOLDEN_PARAMS, ids=[f"{n}-{d}" for n, d in GOLDEN_PARAMS])
def test_nonfinite_golden(name, dt):
    """Every forward NaN / Inf golden through pack_features / refine with a trace.  The ratio cases
    (the reference raises after recording a NaN cost with nothing kept) pin that prefix against the
    golden and the rest against the oracle, whose tail tests/test_cpu_twin.py defines."""
    prob, inp, meta, gold = _golden_problem(name, dt)
    (res,), (tr,) = rf.refine([prob], _golden_options(meta, dt), trace=True)
    print(name, dt, "status", res["status"], "evals", res["n_evals"], "steps", res["n_steps"], "costs", tr["cost"][:4],
          "best", res["best_cost"], res["best_num_inliers"])
    if name in NONFINITE_RATIO_CASES:
        if dt == "f64":
            nf.check_ratio_prefix(name, gold, dict(cost=tr["cost"], R=tr["R"], t=tr["t"], n_kept=tr["n_kept"]))
        check_against_oracle(res, tr, *_oracle_of_golden(name), dt, name)
        return
    nf.check_forward(name, gold, nf.from_fmpnp(res, tr, _lib.STATUS_NAN, ignore=QUIET), fp32=dt == "f32")
    assert list(tr["accepted"][1:]) == nf.accepts(list(gold["track_costs"]))


def test_nonfinite_facade():
    """sparseFeaturePnP.forward on the NaN-texel golden: the reference's warning, its attributes,
    its three tracked costs and R_best."""
    name = "nan_texel_gm"
    inp, meta, gold = case(name)
    f, gx, gy = poisoned_maps(inp, meta, orc.sobel)
    m = fmpnp.sparseFeaturePnP(meta["n_iters"], loss_fn=LOSS_FN[meta["loss"]], lambda_=meta["lambda0"])
    with pytest.warns(UserWarning, match="NaN detected"):
        R, t = m(torch.from_numpy(inp["pts3d"]), torch.from_numpy(inp["fref"]), torch.from_numpy(f),
                 torch.from_numpy(gx), torch.from_numpy(gy), torch.from_numpy(inp["K"]), int(inp["im_width"]),
                 int(inp["im_height"]), R_init=torch.from_numpy(inp["R0"]), t_init=torch.from_numpy(inp["t0"]),
                 track=True)
    assert m.status_ & _lib.STATUS_NAN
    assert float(m.best_cost_) == pytest.approx(float(gold["best_cost_"]), rel=1e-10)
    assert m.best_num_inliers_ == int(gold["best_num_inliers_"])
    costs = m.track_["costs"]
    assert len(costs) == 3 and np.isnan(costs[2]) and not np.isnan(costs[:2]).any()
    np.testing.assert_allclose(costs[:2], gold["track_costs"][:2], rtol=1e-10)
    np.testing.assert_allclose(R.numpy(), gold["out_R"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(t.numpy(), gold["out_t"], rtol=0, atol=1e-9)


Pred = namedtuple("Prediction", "points_3d reference_inliers matrix quaternion reference_filename")


def _as_query(inp, f):
    """The pyramid golden as a feature_pnp query: a reference hypercolumn and inliers whose gather
    (optimize_feature_pnp.py:51-56) returns the case's fref rows."""
    N, Cc = inp["fref"].shape
    S = int(np.ceil(np.sqrt(N)))
    ref = np.zeros((Cc, S, S))
    rows, cols = np.arange(N) // S, np.arange(N) % S
    ref[:, rows, cols] = inp["fref"].T
    W, H = int(inp["im_width"]), int(inp["im_height"])
    inl = np.stack([(cols + 0.5) * W / S, (rows + 0.5) * H / S], 1)
    assert np.array_equal(orc.gather_reference_features(ref, inl, (W, H)), inp["fref"])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = inp["R0"], inp["t0"]
    return (torch.from_numpy(f).to(DEV), torch.from_numpy(ref).to(DEV)[None],
            Pred(inp["pts3d"], inl, T, np.array([1.0, 0, 0, 0]), "ref.png"), inp["K"]), (W, H)


class _RecordingModel(fmpnp.sparseFeaturePnP):
    """Keeps every level's result record (the model itself keeps the last one)."""

    def _apply_result(self, res, *a, **k):
        self.__dict__.setdefault("results_", []).append(res)
        return super()._apply_result(res, *a, **k)


@pytest.mark.parametrize("name", NONFINITE_PYRAMID_CASES)
def test_nonfinite_pyramid(name):
    """The first level breaks on a NaN step and the two clean levels go on from its R_best:
    multilevel_optimization against the golden; the same query through the one-call facade
    (fmpnp_feature_pnp) and the pipeline's level chain, which form the gradients of the poisoned
    map themselves, against the oracle on those gradients -- the NaN bit at level 0 only."""
    inp, meta, gold = case(name)
    f, gx, gy = poisoned_maps(inp, meta, orc.sobel)
    pyr = [tuple(lv) for lv in meta["pyramid"]]
    kw = dict(loss_fn=LOSS_FN[meta["loss"]], lambda_=meta["lambda0"])
    m = fmpnp.sparseFeaturePnP(meta["n_iters"], **kw)
    with pytest.warns(UserWarning, match="NaN detected"):
        R, t = m.multilevel_optimization(pyr, torch.from_numpy(inp["pts3d"]), torch.from_numpy(inp["fref"]),
                                         torch.from_numpy(f), torch.from_numpy(gx), torch.from_numpy(gy),
                                         torch.from_numpy(inp["K"]), int(inp["im_width"]), int(inp["im_height"]),
                                         R_init=torch.from_numpy(inp["R0"]), t_init=torch.from_numpy(inp["t0"]),
                                         track=True)
    np.testing.assert_allclose(R.numpy(), gold["out_R"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(t.numpy(), gold["out_t"], rtol=0, atol=1e-9)
    nf.assert_same_nonfinite(m.track_["costs"], gold["track_costs"], name)
    np.testing.assert_allclose(m.track_["costs"], gold["track_costs"], rtol=1e-10, equal_nan=True)
    assert float(m.best_cost_) == pytest.approx(float(gold["best_cost_"]), rel=1e-10)
    assert m.best_num_inliers_ == int(gold["best_num_inliers_"])
    assert m.status_ == 0  # the last level's

    # the oracle with the Sobel of the poisoned map (what the device forms from the query map)
    pgx, pgy = orc.sobel(f)
    oR, ot, oattrs, otraces = orc.multilevel(meta["pyramid"], inp["pts3d"], inp["fref"], f, pgx, pgy, inp["K"],
                                             inp["im_width"], inp["im_height"], inp["R0"], inp["t0"],
                                             meta["n_iters"], meta["lambda0"], meta["loss"], trace_cap=64)
    assert [o["status"] for o, _ in otraces] == ["nan", "ok", "ok"]
    query, img = _as_query(inp, f)
    rec = _RecordingModel(meta["n_iters"], storage=torch.float64, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        R1, t1, _ = fmpnp.feature_pnp(query[0][None], query[1], query[2], query[3], img, feature_pyramid=pyr,
                                      model=rec)
    status = [r["status"] & ~QUIET for r in rec.results_]
    assert status == [_lib.STATUS_NAN, 0, 0], status
    assert [r["n_evals"] for r in rec.results_] == [o["n_evals"] for o, _ in otraces]
    np.testing.assert_allclose(R1.numpy(), oR, rtol=0, atol=1e-9)
    np.testing.assert_allclose(t1.numpy(), ot, rtol=0, atol=1e-9)

    pipe = RefinePipeline(img, storage=torch.float64, levels=[lv[:2] for lv in pyr],
                          model_kwargs=dict(n_iters=meta["n_iters"], ratio_threshold=None, **kw))
    ((r,),) = pipe.run([[query]])
    assert r["status"] & _lib.STATUS_NAN
    assert [s & ~QUIET for s in r["level_status"]] == [_lib.STATUS_NAN, 0, 0], r["level_status"]
    np.testing.assert_allclose(r["R"], oR, rtol=0, atol=1e-9)
    np.testing.assert_allclose(r["t"], ot, rtol=0, atol=1e-9)


# --------------------------------------------------------------------------------------------
# 4. every kernel specialisation, with poisoned problems in its batch
# --------------------------------------------------------------------------------------------
_INPUTS = {}
# query q is synthetic scene SEED0 + q; the base is chosen so that every case meets its condition on the
# inputs (min_k below: found with the oracle on the CPU, asserted in the test)
SEED0 = 2000


def _inputs(q, n_pts=N_PTS):
    """Host inputs of synthetic query q (generated on the CPU: the same on every machine, so the
    poison's condition below can be checked without a device).  Every query starts from the harder
    initial pose: several texels of image motion, so points keep entering new texels."""
    if (q, n_pts) not in _INPUTS:
        inp = synth.problem_inputs(n_pts, C, HF, WF, seed=SEED0 + q, device="cpu", init="hard")
        fm = inp["fmap"].double().numpy()
        gx, gy = orc.sobel(fm)
        _INPUTS[(q, n_pts)] = dict(inp, fmap=fm, fref=inp["fref"].double().numpy(), gx=gx, gy=gy)
    return _INPUTS[(q, n_pts)]


def _oracle(inp, f, gx, gy, loss_name, ratio, sampling):
    p = orc.make_problem(inp["pts3d"], inp["fref"], f, gx, gy, inp["K"], inp["im_width"], inp["im_height"],
                         inp["R0"], inp["t0"])
    return orc.forward(p, orc.make_options(ITERS, 0.01, loss_name, ratio, sampling=sampling), trace_cap=ITERS + 1)


def _footprints(inp, R, t, sampling, layout):
    """The texels (row * WF + col) each supported point's sample reads at pose (R, t): its texel
    (nearest, gradients supplied by the caller), the 2x2 cell of bilinear_taps (fmpnp_device.h), or
    the texel's 3x3 neighbourhood (FMPNP_LAYOUT_F: the gradients are formed from the map)."""
    W, H = inp["im_width"], inp["im_height"]
    X, K = inp["pts3d"], inp["K"]
    P = [((R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1]) + R[i, 2] * X[:, 2]) + t[i] for i in range(3)]
    u = [((K[i, 0] * P[0] + K[i, 1] * P[1]) + K[i, 2] * P[2]) for i in range(3)]
    qx, qy = u[0] / u[2], u[1] / u[2]
    px, py = np.rint(qx) - 1.0, np.rint(qy) - 1.0
    sup = (px >= 0) & (px < W) & (py >= 0) & (py < H)
    out = set()
    if sampling == "bilinear":
        x0 = np.floor(((qx - 0.5) * WF) / W - 0.5).astype(np.int64)
        y0 = np.floor(((qy - 0.5) * HF) / H - 0.5).astype(np.int64)
        for dy in (0, 1):
            for dx in (0, 1):
                rr, cc = np.clip(y0 + dy, 0, HF - 1), np.clip(x0 + dx, 0, WF - 1)
                out.update((rr[sup] * WF + cc[sup]).tolist())
        return out
    row = (py[sup].astype(np.int64) * HF) // H
    col = (px[sup].astype(np.int64) * WF) // W
    reach = (-1, 0, 1) if layout == "f" else (0,)
    for dy in reach:
        for dx in reach:
            rr, cc = row + dy, col + dx
            ok = (rr >= 0) & (rr < HF) & (cc >= 0) & (cc < WF)
            out.update((rr[ok] * WF + cc[ok]).tolist())
    return out


def choose_poison(inp, otr, sampling, layout):
    """(k, row, col): the texel some point's sample first reads at the latest accepted evaluation k
    of the clean run (oracle trace `otr`) that a linearisation still follows (k < n_iters), no
    sample having read it at any earlier evaluation, accepted or not.  Poisoning it leaves
    evaluations 0 .. k-1 as they were and makes evaluation k's cost or its linearisation non-finite."""
    acc = [True] + nf.accepts(list(otr["cost"]))
    seen, new_at = set(), []
    for k in range(len(otr["cost"])):
        fp = _footprints(inp, otr["R"][k], otr["t"][k], sampling, layout)
        # (LAYOUT_F: a texel a point sits on before one that is only a neighbour of its texel)
        own = _footprints(inp, otr["R"][k], otr["t"][k], sampling, "fgrad")
        new_at.append(sorted(fp - seen, key=lambda tex: (tex not in own, tex)))
        seen |= fp
    for k in range(min(len(new_at) - 1, ITERS - 1), 0, -1):
        if acc[k] and new_at[k]:
            tex = new_at[k][0]
            return k, tex // WF, tex % WF
    return 0, None, None


_POISONED = {}


def poisoned_problem(q, n_pts, loss_name, ratio, sampling, layout):
    """Query q with one NaN channel at the texel choose_poison picks: (k, f, gx, gy, oracle result,
    oracle trace).  FGRAD keeps the clean map's gradients (the caller supplies them); LAYOUT_F forms
    them from the poisoned map, as the device does."""
    key = (q, n_pts, loss_name, ratio, sampling, layout)
    if key not in _POISONED:
        inp = _inputs(q, n_pts)
        _, otr = _oracle(inp, inp["fmap"], inp["gx"], inp["gy"], loss_name, ratio, sampling)
        k, row, col = choose_poison(inp, otr, sampling, layout)
        f = inp["fmap"].copy()
        if row is not None:
            f[(3 + 5 * q) % C, row, col] = np.nan
        gx, gy = orc.sobel(f) if layout == "f" else (inp["gx"], inp["gy"])
        ores, ptr = _oracle(inp, f, gx, gy, loss_name, ratio, sampling)
        _POISONED[key] = (k, f, gx, gy, ores, ptr)
    return _POISONED[key]


_PACKED = {}


def _pack(inp, f, gx, gy, dt, layout):
    st = STORAGE[dt]
    if layout == "f":
        feats = rf.pack_features(torch.from_numpy(f).to(st), storage=st, device=DEV, layout="f")
    else:
        feats = rf.pack_features(torch.from_numpy(f).to(st), torch.from_numpy(gx).to(st), torch.from_numpy(gy).to(st),
                                 storage=st, device=DEV)
    return rf.make_problem(feats, torch.from_numpy(inp["fref"]).to(st), inp["pts3d"], inp["K"], inp["im_width"],
                           inp["im_height"], inp["R0"], inp["t0"])


def _clean_problem(q, dt, layout, n_pts=N_PTS):
    key = (q, dt, layout, n_pts)
    if key not in _PACKED:
        inp = _inputs(q, n_pts)
        _PACKED[key] = _pack(inp, inp["fmap"], inp["gx"], inp["gy"], dt, layout)
    return _PACKED[key]


def min_k(sampling, layout):
    """The least evaluation at which the poison may first be read for a case to count (a condition
    on the inputs, so that a case cannot degrade into the first-step one): evaluation 2 where the
    gradients are the caller's clean ones, evaluation 1 for FMPNP_LAYOUT_F, whose 3x3 footprint
    leaves few texels unread."""
    return 1 if layout == "f" else 2


def _forward_cases():
    out = []
    for name, r in RECIPES.items():
        if r[2] != "fwd":
            continue
        for dt in ("f32", "f64"):
            if (r[4] == "f" or name in M512) and dt == "f64":
                continue
            for ratio in (None, 0.8):
                out.append((name, dt, ratio))
    return out


FORWARD = _forward_cases()


def _same_bits(a, b, what):
    assert np.array_equal(a["R"], b["R"], equal_nan=True) and np.array_equal(a["t"], b["t"], equal_nan=True), what
    for k in ("best_cost", "initial_cost"):
        assert a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])), (what, k, a[k], b[k])
    for k in ("n_evals", "n_steps", "n_accepted", "best_num_inliers", "has_best"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert a["status"] & ~QUIET == b["status"] & ~QUIET, (what, a["status"], b["status"])


def _same_trace(a, b, what):
    for k in ("R", "t", "cost", "lam", "lr", "n_supported", "n_kept", "accepted"):
        assert np.array_equal(a[k], b[k], equal_nan=k in ("R", "t", "cost", "lam", "lr")), (what, k)


@pytest.mark.parametrize("name,dt,ratio", FORWARD, ids=[f"{n}-{d}-{'r08' if r else 'nor'}" for n, d, r in FORWARD])
def test_specialisation_with_poisoned_problem(name, dt, ratio):
    """The recipe's batch with problems 0, B//2 and B-1 poisoned (one NaN channel of one texel, first
    read at a late accepted evaluation): the poisoned problems against the oracle on the same inputs,
    every other problem bit-identical to the batch launched clean."""
    B, loss, mode, sampling, layout, memo, spec, wgs, *_ = RECIPES[name]
    code, loss_name = LOSSES[loss]
    n_pts = N_512 if name in M512 else N_PTS
    clean = [_clean_problem(q, dt, layout, n_pts) for q in range(B)]
    opts = rf.make_options(ITERS, 0.01, code, ratio_threshold=ratio, dtype=CODE[dt], wgs_per_problem=wgs,
                           memoize=memo, sampling=sampling, speculate=spec)
    base, _ = rf.refine(clean, opts)
    assert info_key(_lib.last_launch()) == case_key(name, dt, ratio), _lib.last_launch()
    subset = sorted({0, B // 2, B - 1})
    probs, expect = list(clean), {}
    for q in subset:
        k, f, gx, gy, ores, otr = poisoned_problem(q, n_pts, loss_name, ratio, sampling, layout)
        assert k >= min_k(sampling, layout), (name, q, k)
        probs[q] = _pack(_inputs(q, n_pts), f, gx, gy, dt, layout)
        expect[q] = (k, ores, otr)
    res, trs = rf.refine(probs, opts, trace=True)
    assert info_key(_lib.last_launch()) == case_key(name, dt, ratio), _lib.last_launch()
    for q in range(B):
        what = f"{name} {dt} ratio={ratio} query {q}"
        if q not in expect:
            _same_bits(res[q], base[q], what)
            continue
        k, ores, otr = expect[q]
        print(what, "first read at evaluation", k, "oracle", ores["status"], ores["n_evals"], "device",
              res[q]["status"], res[q]["n_evals"], res[q]["n_steps"])
        # the poison took effect at evaluation k: the loop broke on the step that follows it, or (ratio
        # test: the limit is NaN and nothing is kept, tests/test_cpu_twin.py) its cost is NaN
        broke = ores["status"] == "nan" and ores["n_evals"] == ores["n_steps"] == k + 1
        assert broke if ratio is None else (broke or (otr["n_kept"][k] == 0 and np.isnan(otr["cost"][k]))), (what, ores)
        check_against_oracle(res[q], trs[q], ores, otr, dt, what)


LEAK = [("nearest", "fgrad", True, "f64"), ("nearest", "fgrad", True, "f32"), ("nearest", "f", True, "f32"),
        ("bilinear", "fgrad", True, "f64"), ("bilinear", "fgrad", True, "f32")]


@pytest.mark.parametrize("sampling,layout,memo,dt", LEAK, ids=[f"{s}-{l}-{d}" for s, l, _, d in LEAK])
def test_poison_does_not_leak_to_the_next_problem(sampling, layout, memo, dt):
    """One team walks [clean, poisoned, clean, poisoned at its first step, clean]: every result is
    its single launch's, bit for bit, and the clean ones end with status 0 -- the NaN word of the
    step scalars, the linearisation cache and the memo columns are reset between problems."""
    loss_name = "geman_mcclure"
    opts = rf.make_options(ITERS, 0.01, _lib.GEMAN_MCCLURE, dtype=CODE[dt], wgs_per_problem=1, max_teams=1,
                           memoize=memo, sampling=sampling)
    k, f, gx, gy, ores, _ = poisoned_problem(1, N_PTS, loss_name, None, sampling, layout)
    assert k >= min_k(sampling, layout)
    late = _pack(_inputs(1), f, gx, gy, dt, layout)
    inp = _inputs(3)
    tex = sorted(_footprints(inp, inp["R0"], inp["t0"], sampling, layout))[0]
    f0 = inp["fmap"].copy()
    f0[5, tex // WF, tex % WF] = np.nan
    g0 = orc.sobel(f0) if layout == "f" else (inp["gx"], inp["gy"])
    first = _pack(inp, f0, g0[0], g0[1], dt, layout)
    walk = [_clean_problem(0, dt, layout), late, _clean_problem(2, dt, layout), first, _clean_problem(4, dt, layout)]
    res, trs = rf.refine(walk, opts, trace=True)
    info = _lib.last_launch()
    assert info["teams"] == 1 and info["wgs_per_problem"] == 1, info
    if sampling == "bilinear":
        assert info["variant_name"] == "BILINEAR", info   # the cell memo
    for i, p in enumerate(walk):
        (one,), (tr1,) = rf.refine([p], opts, trace=True)
        _same_bits(res[i], one, f"problem {i}")
        _same_trace(trs[i], tr1, f"problem {i}")
    assert [r["status"] & ~QUIET for r in res] == [0, _lib.STATUS_NAN, 0, _lib.STATUS_NAN, 0]
    assert res[1]["n_evals"] == k + 1 == res[1]["n_steps"]
    assert res[3]["n_evals"] == 1 and res[3]["n_steps"] == 1 and np.array_equal(res[3]["R"], inp["R0"])


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["nan_texel_gm", "inf_texel_squared"])
def test_poisoned_result_independent_of_memo_and_speculation(name, dt):
    """Memoised with speculative gathers, not memoised, memoised without speculation: the same bits,
    trace included.  The Inf case runs all its steps with an Inf sum cached in the memo."""
    prob, inp, meta, gold = _golden_problem(name, dt)
    runs = []
    for no_memo in (0, 1, 2):
        o = _golden_options(meta, dt)
        o.no_memo = no_memo
        (r,), (tr,) = rf.refine([prob], o, trace=True)
        runs.append((r, tr))
    assert runs[0][0]["n_evals"] == len(gold["track_costs"])
    for no_memo, (r, tr) in zip((1, 2), runs[1:]):
        _same_bits(r, runs[0][0], f"{name} {dt} no_memo={no_memo}")
        _same_trace(tr, runs[0][1], f"{name} {dt} no_memo={no_memo}")


SYNTH_480 = "synthetic_480_points"


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["nan_texel_gm", "nan_fref_gm", "nan_texel_ratio08_gm", SYNTH_480])
def test_poisoned_result_independent_of_team_size(name, dt):
    """1, 2, 3 and 8 workgroups per problem: the same bits, and every member sees the break -- no
    cross-workgroup exchange times out (refine raises on FMPNP_STATUS_SYNC_TIMEOUT; asserted too).
    The goldens' 128 points are two 64-point blocks, so their teams stop at two workgroups; the
    480-point synthetic query (poisoned as in test_specialisation_with_poisoned_problem) forms the
    teams of three and eight."""
    if name == SYNTH_480:
        k, f, gx, gy, ores, _ = poisoned_problem(0, N_512, "geman_mcclure", None, "nearest", "fgrad")
        assert k >= 2 and ores["status"] == "nan"
        prob = _pack(_inputs(0, N_512), f, gx, gy, dt, "fgrad")
        options = lambda g: rf.make_options(ITERS, 0.01, _lib.GEMAN_MCCLURE, dtype=CODE[dt], wgs_per_problem=g)  # noqa: E731
        n_evals, widest = k + 1, 8
    else:
        prob, inp, meta, gold = _golden_problem(name, dt)
        options = lambda g: _golden_options(meta, dt, wgs_per_problem=g)  # noqa: E731
        n_evals, widest = (meta["n_iters"] + 1 if name in NONFINITE_RATIO_CASES else len(gold["track_costs"])), 2
    runs = []
    for g in (1, 2, 3, 8):
        (r,), (tr,) = rf.refine([prob], options(g), trace=True)
        assert r["status"] & _lib.STATUS_SYNC_TIMEOUT == 0, (name, dt, g, r["status"])
        runs.append((g, r, tr, _lib.last_launch()["wgs_per_problem"]))
    assert max(w for *_, w in runs) == widest, [w for *_, w in runs]   # the teams did form
    assert runs[0][1]["n_evals"] == n_evals
    for g, r, tr, _ in runs[1:]:
        _same_bits(r, runs[0][1], f"{name} {dt} wgs={g}")
        _same_trace(tr, runs[0][2], f"{name} {dt} wgs={g}")
