"""Opt-in binary16 storage of the packed map and fref (FMPNP_F16, include/fmpnp.h) on the host: the host pack,
the CPU twin against the oracle on the rounded values (tests/f16_storage_cases.py: the identical-inputs tier, no
new tolerance), the planner's choices and the argument errors -- CPU only, no device."""
import ctypes

import numpy as np
import pytest
import torch

import nonfinite_checks as nf
import oracle.oracle as orc
from f16_storage_cases import (C, HF, ITERS, LOSSES, N_PTS, WF, check_identical_inputs, oracle_cost, oracle_forward,
                               round16, rounded_maps)
from golden_io import FORWARD_CASES, case

from fmpnp import _lib, cpu, refine as rf, synth

EINVAL, EALIGN = -1, -2
LOSS_CODE = {"squared": _lib.SQUARED, "huber": _lib.HUBER, "cauchy": _lib.CAUCHY, "geman_mcclure": _lib.GEMAN_MCCLURE,
             "barron": _lib.BARRON}
FP32_FORWARD_CASES = [n for n in FORWARD_CASES if "fmap32" in case(n)[0]]


def test_abi_and_code():
    assert _lib.load().fmpnp_abi_version() == 4 and _lib.F16 == 2
    assert rf._dtype_code(torch.float16) == _lib.F16


def _small(seed, init):
    inp = synth.problem_inputs(N_PTS, C, HF, WF, seed=1000 + seed, device="cpu", init=init)
    return dict(inp, fmap=inp["fmap"].numpy(), fref=inp["fref"].numpy())


def _host_problem(inp, c_begin=0, c_end=None):
    f = inp["fmap"].astype(np.float64)
    gx, gy = orc.sobel(f)
    feats = cpu.pack_host(f, gx, gy, dtype=np.float16)
    return cpu.problem_host(feats, inp["fref"], inp["pts3d"], inp["K"], inp["im_width"], inp["im_height"], inp["R0"],
                            inp["t0"], c_begin=c_begin, c_end=c_end)


@pytest.mark.parametrize("shape", [(20, 5, 7), (16, 48, 64)], ids=["c20", "c16"])
def test_host_pack_is_the_fp32_pack_narrowed(shape):
    Cc, H, W = shape
    rng = np.random.default_rng(5)
    f = rng.standard_normal((Cc, H, W)).astype(np.float32).astype(np.float64)
    f[0, 0, 0], f[1, 1, 1], f[2, 2, 2] = 7.0e4, 3.0e-6, 1.0e-9   # overflow, a subnormal, underflow to zero
    gx, gy = orc.sobel(f)
    p32 = cpu.pack_host(f, gx, gy, dtype=np.float32)
    p16 = cpu.pack_host(f, gx, gy, dtype=np.float16)
    cs = p16.shape[-1]
    assert p16.dtype == np.float16 and cs % 8 == 0 and Cc <= cs < Cc + 8 and p16.shape[:3] == (H, W, 3)
    with np.errstate(over="ignore"):
        want = p32[..., :Cc].astype(np.float16)
    assert np.array_equal(p16[..., :Cc].view(np.uint16), want.view(np.uint16))
    assert not p16[..., Cc:].any()
    assert np.isposinf(p16[0, 0, 0, 0]) and 0 < p16[1, 1, 0, 1] < 6.2e-5 and p16[2, 2, 0, 2] == 0


@pytest.mark.parametrize("ratio", [None, 0.8], ids=["nor", "r08"])
@pytest.mark.parametrize("loss", ["gm", "cauchy"])
@pytest.mark.parametrize("init", ["easy", "hard"])
def test_twin_against_oracle_on_rounded_values(init, loss, ratio):
    inp = _small(0 if init == "easy" else 1, init)
    maps = rounded_maps(inp["fmap"], inp["fref"])
    prob = _host_problem(inp)
    what = f"{init} {loss} ratio={ratio}"
    opts = rf.make_options(ITERS, 0.01, LOSS_CODE[LOSSES[loss]], ratio_threshold=ratio)
    (res,), (tr,) = cpu.refine_cpu([prob], opts, trace=True, n_threads=1)
    ores, otr = oracle_forward(inp, maps, LOSSES[loss], ratio)
    assert ores["n_evals"] > 3, what
    check_identical_inputs(res, tr, ores, otr, what)
    copts = rf.make_options(0, ratio_threshold=ratio, mode=_lib.MODE_COMPUTE_COST)
    (cres,), _ = cpu.refine_cpu([prob], copts)
    assert cres["initial_cost"] == pytest.approx(oracle_cost(inp, maps, ratio), rel=1e-10), what


@pytest.mark.parametrize("name", FP32_FORWARD_CASES)
def test_twin_golden_cases_on_rounded_inputs(name):
    """The fp32-input golden cases, the oracle run on their rounded inputs (the goldens themselves are the
    unrounded trajectories: binary16 is not expected to follow those)."""
    ginp, meta, _ = case(name)
    inp = dict(ginp, fmap=ginp["fmap32"])
    maps = rounded_maps(inp["fmap"], inp["fref"])
    prob = _host_problem(inp)
    opts = rf.make_options(meta["n_iters"], meta["lambda0"], LOSS_CODE[meta["loss"]], meta.get("barron_alpha") or 0.0,
                           meta.get("ratio_threshold"))
    (res,), (tr,) = cpu.refine_cpu([prob], opts, trace=True, n_threads=1)
    ores, otr = oracle_forward(inp, maps, meta["loss"], meta.get("ratio_threshold"), meta["n_iters"], meta["lambda0"],
                               barron_alpha=meta.get("barron_alpha") or 0.0)
    check_identical_inputs(res, tr, ores, otr, name)


def test_twin_channel_range_off_a_multiple_of_8():
    inp = _small(1, "hard")
    maps = rounded_maps(inp["fmap"], inp["fref"])
    prob = _host_problem(inp, c_begin=3, c_end=13)
    (res,), (tr,) = cpu.refine_cpu([prob], rf.make_options(ITERS, 0.01, _lib.GEMAN_MCCLURE), trace=True, n_threads=1)
    ores, otr = oracle_forward(inp, maps, "geman_mcclure", None, c_begin=3, c_end=13)
    check_identical_inputs(res, tr, ores, otr, "channels [3, 13)")


def test_twin_overflowed_texel_behaves_as_an_inf_texel():
    """A texel above 65504 packs to Inf; the twin's run on it has the status, counts and NaN / Inf positions of
    the fp32-storage twin on a map holding Inf there."""
    inp = _small(0, "easy")
    f = inp["fmap"].astype(np.float64)
    # (a texel under a point's initial pixel, so the run reads it)
    px = rf.project_pixels(inp["R0"], inp["t0"], inp["pts3d"][:1], inp["K"])[0]
    row, col = int(px[1]) * HF // inp["im_height"], int(px[0]) * WF // inp["im_width"]
    gx, gy = orc.sobel(f)                      # (the clean map's gradients: only the texel overflows)
    big, inf = f.copy(), f.copy()
    big[2, row, col], inf[2, row, col] = 7.0e4, np.inf
    p16 = cpu.pack_host(big, gx, gy, dtype=np.float16)
    assert np.isposinf(p16[row, col, 0, 2]) and np.isfinite(p16[..., 1:, :]).all()
    p32 = cpu.pack_host(inf, round16(gx), round16(gy), dtype=np.float32)
    p32[..., 0, :C] = round16(np.moveaxis(inf, 0, -1))
    args = (inp["pts3d"], inp["K"], inp["im_width"], inp["im_height"], inp["R0"], inp["t0"])
    for loss in (_lib.GEMAN_MCCLURE, _lib.SQUARED):
        opts = rf.make_options(12, 0.01, loss)
        (a,), (ta,) = cpu.refine_cpu([cpu.problem_host(p16, inp["fref"], *args)], opts, trace=True, n_threads=1)
        (b,), (tb,) = cpu.refine_cpu([cpu.problem_host(p32, round16(inp["fref"]), *args)], opts, trace=True, n_threads=1)
        assert (a["status"], a["n_evals"], a["n_steps"], a["n_accepted"], a["best_num_inliers"]) == \
            (b["status"], b["n_evals"], b["n_steps"], b["n_accepted"], b["best_num_inliers"])
        nf.assert_same_nonfinite(ta["cost"], tb["cost"], "overflowed texel")
        np.testing.assert_array_equal(ta["n_supported"], tb["n_supported"])
        np.testing.assert_array_equal(ta["cost"], tb["cost"])  # (the twin sums every storage type in one order)


# --- argument errors -----------------------------------------------------------------------------------------------
def _descs(n, N=512, Cc=256, cs=None, ld=None, Hf=240, Wf=320):
    arr = (_lib.Problem * n)()
    cs = (Cc + 7) // 8 * 8 if cs is None else cs
    for i in range(n):
        p = arr[i]
        p.feat, p.fref, p.pts3d = 0x1000, 0x2000, 0x3000  # never dereferenced by the planner
        p.Hf, p.Wf, p.cstride, p.c_begin, p.c_end, p.ld_ref, p.N = Hf, Wf, cs, 0, Cc, cs if ld is None else ld, N
        p.im_width, p.im_height = 4 * Wf, 4 * Hf
        p.K[:] = [1000.0, 0, 640.0, 0, 1000.0, 480.0, 0, 0, 1]
        p.R0[:] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    return arr


def _plan_rc(opts, n=1, **kw):
    info = _lib.LaunchInfo()
    return _lib.load().fmpnp_plan(_descs(n, **kw), n, ctypes.byref(opts), ctypes.byref(info)), info


@pytest.fixture()
def plan_cus(monkeypatch):
    # (as tests/test_planner_host.py: the library honours FMPNP_PLAN_CUS only without a device)
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the planner plans for the device present, which does not have 256 CUs")
    monkeypatch.setenv("FMPNP_PLAN_CUS", "256")


def test_c_abi_rejects_unsupported_combinations(plan_cus):
    L = _lib.load()
    bil = rf.make_options(5, dtype=_lib.F32, sampling="bilinear")
    bil.dtype = _lib.F16
    lay = rf.make_options(5, dtype=_lib.F16)
    lay.layout = _lib.LAYOUT_F
    res = (_lib.Result * 1)()
    for o in (bil, lay):
        assert _plan_rc(o)[0] == EINVAL
        assert L.fmpnp_workspace_size(_descs(1), 1, ctypes.byref(o)) == 0   # (its way of reporting an error)
        assert L.fmpnp_refine_batch_cpu(_descs(1, N=0), 1, ctypes.byref(o), res, None, 0, 1) == EINVAL
    ok = rf.make_options(5, dtype=_lib.F16)
    assert _plan_rc(ok)[0] == 0 and L.fmpnp_workspace_size(_descs(1), 1, ctypes.byref(ok)) > 0
    # strides: multiples of 8 channels
    assert _plan_rc(ok, Cc=12, cs=12)[0] == EALIGN
    assert _plan_rc(ok, Cc=12, cs=16, ld=12)[0] == EALIGN
    assert L.fmpnp_refine_batch_cpu(_descs(1, N=0, Cc=12, cs=12), 1, ctypes.byref(ok), res, None, 0, 1) == EALIGN
    assert _plan_rc(rf.make_options(5, dtype=_lib.F32), Cc=12, cs=12)[0] == 0   # (fp32 keeps its strides of 4)


def test_python_value_errors():
    f = np.zeros((8, 4, 4), np.float32)
    with pytest.raises(ValueError, match="layout 'f'"):
        cpu.pack_host(f, dtype=np.float16, layout="f")
    with pytest.raises(ValueError, match="bilinear"):
        rf.make_options(5, dtype=_lib.F16, sampling="bilinear")
    g = np.zeros_like(f)
    prob = cpu.problem_host(cpu.pack_host(f, g, g, dtype=np.float16), np.zeros((3, 8), np.float32), np.ones((3, 3)),
                            np.eye(3), 16, 16, np.eye(3), np.zeros(3))
    with pytest.raises(ValueError, match="nearest"):
        cpu.refine_cpu([prob], rf.make_options(5, sampling="bilinear"))
    from fmpnp import replay
    from fmpnp.pipeline import RefinePipeline
    from fmpnp.localize import _RefineSpec
    with pytest.raises(ValueError, match="binary16"):
        replay.replay({}, {}, {}, np.eye(3), storage=torch.float16)
    with pytest.raises(ValueError, match="binary16"):
        RefinePipeline(storage=torch.float16, device="cpu")
    with pytest.raises(ValueError, match="float32 or float64"):
        _RefineSpec(16, (64, 64), None, None, torch.float16, "last")


def test_feature_pnp_value_errors():
    """layout "f" and the layers entry points with binary16: refused before any device is asked for."""
    from fmpnp.optimize_feature_pnp import feature_pnp
    q = torch.zeros((8, 4, 4))
    layers = [torch.zeros((1, 8, 4, 4))]
    with pytest.raises(ValueError, match="layout 'f'"):
        feature_pnp(q, q, None, np.eye(3), (16, 16), storage=torch.float16, layout="f")
    with pytest.raises(ValueError, match="reference_layers"):
        feature_pnp(q, None, None, np.eye(3), (16, 16), storage=torch.float16, reference_layers=layers)


def test_planner_choices(plan_cus):
    """The speculation limit follows 64 * (16 / element size) = 512 channels; the _512 carve is never chosen."""
    gm = rf.make_options(50, 0.01, _lib.GEMAN_MCCLURE, dtype=_lib.F16)
    rc, info = _plan_rc(gm, n=128, Cc=512)
    i = _lib._info_dict(info)
    assert rc == 0 and i["dtype_name"] == "f16" and i["variant_name"] == "GM_SPEC" and i["speculate"] == 1, i
    rc, info = _plan_rc(gm, n=128, Cc=520)
    i = _lib._info_dict(info)
    assert rc == 0 and i["dtype_name"] == "f16" and "SPEC" not in i["variant_name"] and i["speculate"] == 0, i
    rc, info = _plan_rc(gm, n=1, Cc=256)     # (N = 512: fp32 would take the compile-time carve)
    i = _lib._info_dict(info)
    assert rc == 0 and i["variant_name"] == "GM_SPEC_H" and i["helpers"] >= 2, i
