"""Opt-in binary16 storage of the packed map and fref (FMPNP_F16, include/fmpnp.h) on the device.

The pack and the reference gather are the fp32 ones narrowed, bit for bit.  Everything that reads binary16 --
the LM kernel's specialisations, fmpnp_point_costs, fmpnp_compute_cost_async, fmpnp_feature_pnp -- is compared
with the oracle on the rounded values (tests/f16_storage_cases.py): both sides read identical numbers, so the
tolerance is the project's identical-inputs tier and no new one is introduced.  Launch shape, helpers,
speculation and windows change nothing, bit for bit."""
import ctypes
import itertools
import threading
from collections import namedtuple

import numpy as np
import pytest
import torch

import oracle.oracle as orc

pytestmark = pytest.mark.gpu

import fmpnp  # noqa: E402  (no skip: a missing HIP library must fail)
from fmpnp import _lib, refine as rf, synth  # noqa: E402

from f16_storage_cases import (C, CALL_C, CALL_HF, CALL_LEVELS, CALL_N, CALL_WF, CASES, HF, ITERS,  # noqa: E402
                               LOSSES, N_PTS, PACK_SHAPES, PATH_CHANNELS, PATH_HF, PATH_N, PATH_WF, RECIPES, WF,
                               case_key, check_identical_inputs, oracle_cost, oracle_forward, round16, rounded_maps)
from variant_recipes import info_key  # noqa: E402

DEV = "cuda:0"
CODE = {"gm": _lib.GEMAN_MCCLURE, "cauchy": _lib.CAUCHY}
Pred = namedtuple("Prediction", "points_3d reference_inliers matrix quaternion reference_filename")


def _bits(t):
    return t.contiguous().view(torch.int16)


# --- pack -------------------------------------------------------------------------------------------------------------
def _pack_map(shape, kind):
    Cc, H, W = shape
    g = torch.Generator().manual_seed(11)
    fm = torch.randn((Cc, H, W), generator=g, dtype=torch.float32)
    if kind == "tiny":          # values into binary16's subnormals and to zero
        fm = fm * 1e-6
    elif kind == "overflow":    # one value above 65504
        fm[Cc // 2, H // 2, W // 2] = 7.0e4
    return fm


@pytest.mark.parametrize("kind", ["plain", "tiny", "overflow"])
@pytest.mark.parametrize("norm,rep", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["zero", "zero-norm", "replicate", "replicate-norm"])
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=["c20", "c16"])
def test_pack_is_the_fp32_pack_narrowed(shape, norm, rep, kind):
    Cc = shape[0]
    fm = _pack_map(shape, kind).to(DEV)
    p32 = rf.pack_features(fm, storage=torch.float32, device=DEV, sobel_normalized=norm, sobel_replicate_pad=rep)
    p16 = rf.pack_features(fm, storage=torch.float16, device=DEV, sobel_normalized=norm, sobel_replicate_pad=rep)
    assert p16.buf.dtype == torch.float16 and p16.cstride % 8 == 0 and Cc <= p16.cstride < Cc + 8
    assert torch.equal(_bits(p16.buf[..., :Cc]), _bits(p32.buf[..., :Cc].half()))
    assert not p16.buf[..., Cc:].any()
    if kind == "tiny":
        f = p16.buf[:, :, 0, :Cc].float().abs()
        assert ((f > 0) & (f < 6.1e-5)).any() and (f == 0).any()    # subnormals kept, smaller values to zero
    if kind == "overflow":
        assert torch.isposinf(p16.buf[shape[1] // 2, shape[2] // 2, 0, Cc // 2])


@pytest.mark.parametrize("in_dt", [torch.float32, torch.float64], ids=["in32", "in64"])
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=["c20", "c16"])
def test_pack_given_gradients(shape, in_dt):
    g = torch.Generator().manual_seed(12)
    fm, gx, gy = (torch.randn(shape, generator=g, dtype=torch.float64).to(in_dt).to(DEV) for _ in range(3))
    p32 = rf.pack_features(fm, gx, gy, storage=torch.float32, device=DEV)
    p16 = rf.pack_features(fm, gx, gy, storage=torch.float16, device=DEV)
    assert torch.equal(_bits(p16.buf[..., :shape[0]]), _bits(p32.buf[..., :shape[0]].half()))
    assert not p16.buf[..., shape[0]:].any()


def test_pack_and_point_costs_reject_bad_strides():
    fm = torch.zeros((12, 4, 4), device=DEV)
    out = torch.zeros((4, 4, 3, 12), dtype=torch.float16, device=DEV)
    rc = _lib.load().fmpnp_pack_features(ctypes.c_void_p(fm.data_ptr()), None, None, _lib.F32, 12, 4, 4,
                                         ctypes.c_void_p(out.data_ptr()), _lib.F16, 12, 0, 0, _lib.stream_ptr(DEV))
    assert rc == -2  # FMPNP_EALIGN
    rc = _lib.load().fmpnp_pack_features(ctypes.c_void_p(out.data_ptr()), None, None, _lib.F16, 12, 4, 4,
                                         ctypes.c_void_p(out.data_ptr()), _lib.F16, 16, 0, 0, _lib.stream_ptr(DEV))
    assert rc == -1  # FMPNP_EINVAL: maps never arrive as binary16
    torch.cuda.synchronize()


# --- reference gather ---------------------------------------------------------------------------------------------------
def _ref_case():
    g = torch.Generator().manual_seed(13)
    ref = torch.randn((20, 9, 9), generator=g, dtype=torch.float32).to(DEV)
    inl = np.random.default_rng(3).uniform(0.0, 1.0, (37, 2)) * 48.0
    return ref, inl, (48, 48)


def test_reference_gather_sync_and_async():
    ref, inl, img = _ref_case()
    r32 = rf.gather_reference(ref, inl, img, storage=torch.float32, device=DEV)
    r16 = rf.gather_reference(ref, inl, img, storage=torch.float16, device=DEV)
    assert r16.shape == (37, 24) and r32.shape == (37, 20)
    assert torch.equal(_bits(r16[:, :20]), _bits(r32.half())) and not r16[:, 20:].any()
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    a16 = rf.gather_reference(ref, inl, img, storage=torch.float16, device=DEV, err_flag=flag)
    assert torch.equal(_bits(a16), _bits(r16)) and int(flag.item()) == 0
    # an inlier outside the map: the same error / flag as fp32 storage, and a zeroed row
    bad = inl.copy()
    bad[5] = (1.0e4, 3.0)
    for st in (torch.float32, torch.float16):
        with pytest.raises(IndexError):
            rf.gather_reference(ref, bad, img, storage=st, device=DEV)
        flag.zero_()
        out = rf.gather_reference(ref, bad, img, storage=st, device=DEV, err_flag=flag)
        assert int(flag.item()) == 1 and not out[5].any() and out[4].any()


def test_reference_gather_batch():
    ref, inl, img = _ref_case()
    refs = [ref, (ref * 2.0).double()[:, :7, :7].contiguous()]
    inls = [torch.from_numpy(inl).to(DEV), torch.from_numpy(inl[:9].copy()).to(DEV)]
    inls[1][2] = torch.tensor([-1.0e3, 2.0], dtype=torch.float64)   # outside the second map
    L, vp = _lib.load(), ctypes.c_void_p
    outs = {}
    for dt_in, k in ((torch.float32, 0), (torch.float64, 1)):
        for st in (torch.float32, torch.float16):
            ld = 24 if st == torch.float16 else 20
            out = torch.zeros((inls[k].shape[0], ld), dtype=st, device=DEV)
            err = torch.zeros(1, dtype=torch.int32, device=DEV)
            rc = L.fmpnp_gather_reference_batch(
                1, (vp * 1)(refs[k].data_ptr()), (ctypes.c_int * 3)(*refs[k].shape), (vp * 1)(inls[k].data_ptr()),
                (ctypes.c_int * 1)(inls[k].shape[0]), img[0], img[1], (vp * 1)(out.data_ptr()), (ctypes.c_int * 1)(ld),
                rf._dtype_code(dt_in), rf._dtype_code(st), vp(err.data_ptr()), _lib.stream_ptr(DEV))
            assert rc == 0
            outs[(k, st)] = (out, int(err.item()))
    for k in (0, 1):
        o32, e32 = outs[(k, torch.float32)]
        o16, e16 = outs[(k, torch.float16)]
        assert e32 == e16 == k
        assert torch.equal(_bits(o16[:, :20]), _bits(o32.half())) and not o16[:, 20:].any()
    assert not outs[(1, torch.float16)][0][2].any()


# --- every specialisation the planner chooses ---------------------------------------------------------------------------
_INPUTS, _PACKED, _ROUNDED, _ORACLE = {}, {}, {}, {}


def _inputs(seed):
    if seed not in _INPUTS:
        init = "hard" if seed % 2 else "easy"
        _INPUTS[seed] = synth.problem_inputs(N_PTS, C, HF, WF, seed=1000 + seed, device=DEV, init=init)
    return _INPUTS[seed]


def _problem(seed):
    if seed not in _PACKED:
        inp = _inputs(seed)
        feats = rf.pack_features(inp["fmap"], storage=torch.float16, device=DEV)
        _PACKED[seed] = rf.make_problem(feats, inp["fref"], inp["pts3d"], inp["K"], inp["im_width"],
                                        inp["im_height"], inp["R0"], inp["t0"])
    return _PACKED[seed]


def _rounded(seed):
    if seed not in _ROUNDED:
        inp = _inputs(seed)
        _ROUNDED[seed] = rounded_maps(inp["fmap"].cpu().numpy(), inp["fref"].cpu().numpy())
    return _ROUNDED[seed]


def _oracle(seed, loss, ratio, mode="fwd"):
    key = (seed, loss, ratio, mode)
    if key not in _ORACLE:
        if mode == "cost":
            _ORACLE[key] = (oracle_cost(_inputs(seed), _rounded(seed), ratio), None)
        else:
            _ORACLE[key] = oracle_forward(_inputs(seed), _rounded(seed), LOSSES[loss], ratio)
    return _ORACLE[key]


def _options(loss, ratio, mode="fwd", **kw):
    return rf.make_options(ITERS, 0.01, CODE[loss], ratio_threshold=ratio, dtype=_lib.F16,
                           mode=_lib.MODE_COMPUTE_COST if mode == "cost" else _lib.MODE_FORWARD, **kw)


@pytest.mark.parametrize("name,ratio", CASES, ids=[f"{n}-{'r08' if r else 'nor'}" for n, r in CASES])
def test_specialisation_against_oracle_on_rounded_values(name, ratio):
    B, loss, mode, memo, spec, wgs, *_ = RECIPES[name]
    probs = [_problem(q) for q in range(B)]
    res, trs = rf.refine(probs, _options(loss, ratio, mode, wgs_per_problem=wgs, memoize=memo, speculate=spec),
                         trace=mode == "fwd")
    info = _lib.last_launch()
    assert info_key(info) == case_key(name, ratio), info
    for q in sorted({0, B // 2, B - 1}):
        ores, otr = _oracle(q, loss, ratio, mode)
        what = f"{name} ratio={ratio} query {q}"
        if mode == "cost":
            assert res[q]["initial_cost"] == pytest.approx(ores, rel=1e-10), what
            continue
        check_identical_inputs(res[q], trs[q], ores, otr, what, ignore_status=_lib.STATUS_HELPER_WAIT)


def test_every_planner_choice_has_an_oracle_case():
    """tests/test_variant_coverage.py's sweep with dtype = f16: every specialisation fmpnp_plan chooses has a case
    above, and every case is one the planner chooses."""
    seen = {}
    grid = itertools.product(("gm", "cauchy"), ("fwd", "cost"), (0, 1, 2), (None, 0.8), (1, 8, 128, 256, 512),
                             (64, 128, 480, 2048), (16, 512), (0, 2), (0, -1))
    for loss, mode, no_memo, ratio, B, N, Cc, wgs, helpers in grid:
        desc = np.zeros(B, dtype=rf.PROBLEM_DTYPE)
        desc["feat"], desc["fref"], desc["pts3d"] = 256, 256, 256  # never dereferenced by the planner
        desc["Hf"], desc["Wf"], desc["cstride"], desc["c_end"], desc["ld_ref"] = HF, WF, Cc, Cc, Cc
        desc["N"], desc["im_width"], desc["im_height"] = N, 4 * WF, 4 * HF
        o = _options(loss, ratio, mode, wgs_per_problem=wgs, helpers=helpers)
        o.no_memo = no_memo
        info = _lib.LaunchInfo()
        rc = _lib.load().fmpnp_plan(desc.ctypes.data_as(ctypes.POINTER(_lib.Problem)), B, ctypes.byref(o),
                                    ctypes.byref(info))
        assert rc == 0, (loss, mode, no_memo, ratio, B, N, Cc, wgs, helpers, rc)
        seen.setdefault(info_key(_lib._info_dict(info)), (loss, mode, no_memo, ratio, B, N, Cc, wgs, helpers))
    covered = {case_key(*c) for c in CASES}
    missing = {k: v for k, v in seen.items() if k not in covered}
    assert not missing, f"binary16 specialisations the planner chooses without an oracle-compared case: {missing}"
    assert not covered - set(seen), f"cases the sweep never chose: {sorted(covered - set(seen))}"
    # ... and the bilinear and f-only rows of that grid are refused for binary16
    desc = np.zeros(1, dtype=rf.PROBLEM_DTYPE)
    desc["feat"], desc["fref"], desc["pts3d"] = 256, 256, 256
    desc["Hf"], desc["Wf"], desc["cstride"], desc["c_end"], desc["ld_ref"] = HF, WF, 16, 16, 16
    desc["N"], desc["im_width"], desc["im_height"] = 64, 4 * WF, 4 * HF
    for bad in ("bilinear", "f"):
        o = _options("gm", None)
        o.sampling = _lib.BILINEAR if bad == "bilinear" else _lib.NEAREST
        o.layout = _lib.LAYOUT_F if bad == "f" else _lib.LAYOUT_FGRAD
        info = _lib.LaunchInfo()
        assert _lib.load().fmpnp_plan(desc.ctypes.data_as(ctypes.POINTER(_lib.Problem)), 1, ctypes.byref(o),
                                      ctypes.byref(info)) == -1


# --- the gather's channel paths -----------------------------------------------------------------------------------------
_PATH = {}


def _path_case(Cc):
    if Cc not in _PATH:
        inp = synth.problem_inputs(PATH_N, Cc, PATH_HF, PATH_WF, seed=77, device=DEV, init="hard")
        feats = rf.pack_features(inp["fmap"], storage=torch.float16, device=DEV)
        prob = rf.make_problem(feats, inp["fref"], inp["pts3d"], inp["K"], inp["im_width"], inp["im_height"],
                               inp["R0"], inp["t0"])
        maps = rounded_maps(inp["fmap"].cpu().numpy(), inp["fref"].cpu().numpy())
        _PATH[Cc] = (inp, prob, maps, oracle_forward(inp, maps, "geman_mcclure", None, n_iters=20))
    return _PATH[Cc]


@pytest.mark.parametrize("wgs", [0, 2], ids=["b1-helpers", "team2"])
@pytest.mark.parametrize("Cc", PATH_CHANNELS)
def test_gather_channel_paths(Cc, wgs):
    inp, prob, maps, (ores, otr) = _path_case(Cc)
    assert prob.feats.cstride == (Cc + 7) // 8 * 8
    opts = rf.make_options(20, 0.01, _lib.GEMAN_MCCLURE, dtype=_lib.F16, wgs_per_problem=wgs)
    (res,), (tr,) = rf.refine([prob], opts, trace=True)
    info = _lib.last_launch()
    assert info["dtype_name"] == "f16" and info["wgs_per_problem"] == (2 if wgs else 1), info
    assert (info["helpers"] > 0) == (wgs == 0) and info["speculate"] == (1 if wgs == 0 and Cc <= 512 else 0), info
    check_identical_inputs(res, tr, ores, otr, f"C={Cc} wgs={wgs}", ignore_status=_lib.STATUS_HELPER_WAIT)


@pytest.mark.parametrize("Cc", [20, 520])
def test_point_costs_and_compute_cost(Cc):
    inp, prob, maps, _ = _path_case(Cc)
    f, _, _, fref = maps
    cost, sup = rf.point_costs(prob)
    args = (inp["pts3d"], fref, f, inp["K"], inp["im_width"], inp["im_height"], inp["R0"], inp["t0"])
    mask, ocost, nsup = orc.find_inliers(*args, 1.0e30)
    # (orc.find_inliers: cost = 0.5 ||e||^2 per supported point; its mask under a huge threshold is the support)
    assert int(sup.sum()) == nsup
    np.testing.assert_array_equal(sup.cpu().numpy(), mask)
    np.testing.assert_allclose(cost.cpu().numpy()[mask], ocost[mask], rtol=1e-12, atol=0)
    for ratio in (None, 0.8):
        got = rf.compute_cost(prob, ratio is not None, ratio)
        assert got["initial_cost"] == pytest.approx(oracle_cost(inp, maps, ratio), rel=1e-12), ratio


# --- launch independence ------------------------------------------------------------------------------------------------
def _same(a, b, what):
    assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]), what
    for k in ("initial_cost", "best_cost", "best_num_inliers", "n_evals", "n_steps", "n_accepted"):
        assert a[k] == b[k], (what, k)
    assert (a["status"] ^ b["status"]) & ~_lib.STATUS_HELPER_WAIT == 0, what


@pytest.mark.parametrize("ratio", [None, 0.8], ids=["nor", "r08"])
def test_launch_shape_changes_nothing(ratio):
    """Helpers on / off, speculation on / off, no_memo 0 / 1 / 2, B = 1 against the same problem inside B = 128:
    bit for bit."""
    prob = _problem(1)
    (base,), _ = rf.refine([prob], _options("gm", ratio))
    assert _lib.last_launch()["variant_name"] == "GM_SPEC_H"
    runs = {"helpers off": _options("gm", ratio, helpers=-1), "speculation off": _options("gm", ratio, speculate=False),
            "no memo": _options("gm", ratio, memoize=False), "team of 2": _options("gm", ratio, wgs_per_problem=2)}
    variants = set()
    for what, o in runs.items():
        (r,), _ = rf.refine([prob], o)
        variants.add(_lib.last_launch()["variant_name"])
        _same(r, base, what)
    assert variants == {"GM_SPEC", "GM_H", "GM"}, variants
    batch, _ = rf.refine([_problem(q) for q in range(127)] + [prob], _options("gm", ratio))
    assert _lib.last_launch()["grid"] == 128
    _same(batch[127], base, "inside B = 128")
    _same(batch[1], base, "inside B = 128 (the same seed)")


# --- the consumer's call ------------------------------------------------------------------------------------------------
def _query(seed, init, N=CALL_N):
    (batch,), img = synth.pipeline_queries(1, 1, N, CALL_C, CALL_HF, CALL_WF, device=DEV, seed0=seed, init=init)
    q, r, p, K = batch[0]
    return q[None], r, Pred(p.points_3d, p.reference_inliers, p.matrix, np.array([1.0, 0, 0, 0]), "ref.png"), K, img


def _call(args, pyr, window=None, track=True):
    model = fmpnp.sparseFeaturePnP(ITERS, loss_fn=fmpnp.geman_mcclure_loss, lambda_=0.01)
    return fmpnp.feature_pnp(*args, track=track, feature_pyramid=pyr, model=model, window=window,
                             storage=torch.float16)


def _same_call(a, b, what):
    (Ra, ta, ma), (Rb, tb, mb) = a, b
    assert torch.equal(Ra, Rb) and torch.equal(ta, tb), what
    assert torch.equal(ma.best_cost_, mb.best_cost_) and ma.best_num_inliers_ == mb.best_num_inliers_, what
    assert torch.equal(ma.initial_cost_, mb.initial_cost_), what
    assert [float(c) for c in ma.track_["costs"]] == [float(c) for c in mb.track_["costs"]], what


@pytest.mark.parametrize("init", ["easy", "hard"])
def test_consumer_call(init):
    pyr = [(a, b, None, None) for a, b in CALL_LEVELS]
    args = _query(29, init)
    q, r, pred, K, img = args
    L = _lib.load()
    full = _call(args, pyr, window=0)
    assert _lib.last_launch()["dtype_name"] == "f16" and not _lib.last_launch()["variant_name"].endswith("_W")
    before = L.fmpnp_feature_pnp_reruns()
    _same_call(_call(args, pyr), full, "default window")
    _same_call(_call(args, pyr, window=6), full, "window 6")
    assert _lib.last_launch()["variant_name"] in ("GM_W", "GM_H_W"), _lib.last_launch()
    assert L.fmpnp_feature_pnp_reruns() == before
    _same_call(_call(args, pyr, window=2), full, "window 2")
    if init == "hard":
        # The re-run path: a window miss re-runs the call fully packed.  At this shape the windows of 70 points
        # (5 x 5 texels each, radius 2) cover two thirds of the 24 x 32 map between them, and the oracle's
        # trajectories from synth's hard start never visit a texel outside them (80 seeds): that start alone does
        # not force a re-run.  With its translation tripled this query's points visit unmarked texels at 135 of
        # their evaluations (the oracle's trajectory against the marks of the initial pose).
        T = np.array(pred.matrix, dtype=np.float64)
        T[:3, 3] *= 3.0
        harder = (q, r, pred._replace(matrix=T), K, img)
        full_h = _call(harder, pyr, window=0)
        before = L.fmpnp_feature_pnp_reruns()
        _same_call(_call(harder, pyr, window=2), full_h, "window 2, re-run")
        assert L.fmpnp_feature_pnp_reruns() == before + 1
    # the oracle on the rounded values: the reference's preamble and multilevel_optimization
    R, t, m = full
    fm = q[0].double().cpu().numpy()
    fref = orc.gather_reference_features(fm, pred.reference_inliers, img)
    f16, gx16, gy16, fref16 = rounded_maps(fm, fref)
    T = np.asarray(pred.matrix, dtype=np.float64)
    pts = np.asarray(pred.points_3d, dtype=np.float64).reshape(-1, 3)
    oR, ot, attrs, otr = orc.multilevel(pyr, pts, fref16, f16, gx16, gy16, np.asarray(K, dtype=np.float64), img[0],
                                        img[1], T[:3, :3], T[:3, 3], ITERS, loss="geman_mcclure", trace_cap=ITERS + 1)
    ocost = np.concatenate([tr["cost"] for _, tr in otr])
    onsup = np.concatenate([tr["n_supported"] for _, tr in otr])
    assert m.status_ == 0 and len(m.track_["costs"]) == len(ocost)
    np.testing.assert_array_equal(np.array([int(mk.sum()) for mk in m.track_["mask"]]), onsup)
    np.testing.assert_allclose(np.asarray(m.track_["costs"], dtype=np.float64), ocost, rtol=1e-10, atol=0)
    np.testing.assert_allclose(R.numpy(), oR, rtol=0, atol=1e-9)
    np.testing.assert_allclose(t.numpy(), ot, rtol=0, atol=1e-9)
    assert float(m.initial_cost_) == pytest.approx(attrs["initial_cost"], rel=1e-10)
    assert float(m.best_cost_) == pytest.approx(attrs["best_cost"], rel=1e-10)
    assert m.best_num_inliers_ == attrs["best_num_inliers"]


def test_consumer_call_refuses_layers_and_layout_f():
    q, r, pred, K, img = _query(31, "easy")
    with pytest.raises(ValueError, match="layout 'f'"):
        fmpnp.feature_pnp(q, r, pred, K, img, storage=torch.float16, layout="f")
    with pytest.raises(ValueError, match="reference_layers"):
        fmpnp.feature_pnp(q, None, pred, K, img, storage=torch.float16, reference_layers=[r])
    with pytest.raises(ValueError, match="query_layers"):
        fmpnp.feature_pnp(None, r, pred, K, img, storage=torch.float16, query_layers=[r])


def test_feature_pnp_two_streams_concurrent():
    """Two threads on two streams calling fmpnp_feature_pnp with binary16 storage (the scratch carve follows the
    element size): each thread's results equal its serial calls bit for bit."""
    pyr = [(a, b, None, None) for a, b in CALL_LEVELS]
    qa, qb = _query(41, "easy"), _query(42, "hard", N=130)
    sa, sb = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)

    def calls(args, stream, reps):
        def f():
            with torch.cuda.stream(stream):
                return [_call(args, pyr, track=False) for _ in range(reps)]
        return f
    ra, rb = calls(qa, sa, 1)()[0], calls(qb, sb, 1)()[0]
    out, errs = [None, None], []

    def run(i, fn):
        try:
            out[i] = fn()
        except BaseException as e:  # noqa: BLE001  (re-raised in the main thread)
            errs.append(e)
    ts = [threading.Thread(target=run, args=(0, calls(qa, sa, 6))), threading.Thread(target=run, args=(1, calls(qb, sb, 6)))]
    for th in ts:
        th.start()
    for th in ts:
        th.join(120)
    if errs:
        raise errs[0]
    for got, ref in ((out[0], ra), (out[1], rb)):
        for R, t, m in got:
            assert torch.equal(R, ref[0]) and torch.equal(t, ref[1])
            assert torch.equal(m.best_cost_, ref[2].best_cost_) and m.best_num_inliers_ == ref[2].best_num_inliers_
