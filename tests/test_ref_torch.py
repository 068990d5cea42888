"""The PyTorch-CPU restatement (oracle/ref_torch.py, bench.py's second CPU baseline) against
the reference's own golden vectors: same trajectory (tracked costs), same result.  CPU only."""
import numpy as np
import pytest
import torch

import nonfinite_checks as nf
from golden_io import (FORWARD_CASES, NONFINITE_FORWARD_CASES, NONFINITE_PYRAMID_CASES, NONFINITE_RATIO_CASES, case,
                       maps64, poisoned_maps)
from oracle import ref_torch

# every forward case except the early exits' attribute bookkeeping (checked in the C oracle)
CASES = [c for c in FORWARD_CASES]


@pytest.mark.parametrize("name", CASES)
def test_ref_torch_matches_reference(name):
    inp, meta, gold = case(name)
    f, gx, gy = maps64(inp, lambda x: tuple(a.numpy() for a in ref_torch.sobel(x)))
    R, t, info = ref_torch.forward(inp["pts3d"], inp["fref"], f, gx, gy, inp["K"], int(inp["im_width"]),
                                   int(inp["im_height"]), inp["R0"], inp["t0"], meta["n_iters"], meta["lambda0"],
                                   meta["loss"], meta.get("ratio_threshold"), meta.get("barron_alpha") or 0.0)
    np.testing.assert_allclose(R.numpy(), gold["out_R"], atol=1e-9)
    np.testing.assert_allclose(t.numpy(), gold["out_t"], atol=1e-9)
    if "track_costs" in gold:
        np.testing.assert_allclose(info["costs"], gold["track_costs"], rtol=1e-10)
    if bool(gold["has_best_cost_"]):
        assert float(info["best_cost"]) == pytest.approx(float(gold["best_cost_"]), rel=1e-10)
        assert info["best_num_inliers"] == int(gold["best_num_inliers_"])


def test_ref_torch_sobel_matches_oracle():
    import oracle.oracle as orc
    x = torch.randn((5, 17, 23), generator=torch.Generator().manual_seed(1), dtype=torch.float64).numpy()
    gx, gy = ref_torch.sobel(x)
    ogx, ogy = orc.sobel(x)
    np.testing.assert_allclose(gx.numpy(), ogx, atol=1e-13)
    np.testing.assert_allclose(gy.numpy(), ogy, atol=1e-13)


def _np_sobel(x):
    return tuple(a.numpy() for a in ref_torch.sobel(x))


def run_ref_torch_nonfinite(name):
    inp, meta, gold = case(name)
    f, gx, gy = poisoned_maps(inp, meta, _np_sobel)
    R, t, info = ref_torch.forward(inp["pts3d"], inp["fref"], f, gx, gy, inp["K"], int(inp["im_width"]),
                                   int(inp["im_height"]), inp["R0"], inp["t0"], meta["n_iters"], meta["lambda0"],
                                   meta["loss"], meta.get("ratio_threshold"))
    return gold, R.numpy(), t.numpy(), info


def _got(R, t, info):
    return dict(nan=info["status"] == "nan", ok=info["status"] == "ok", n_evals=len(info["costs"]),
                n_steps=info["n_steps"], n_accepted=info["n_accepted"], cost=np.array(info["costs"]), R=R, t=t,
                has_best=info["best_cost"] is not None, best_cost=float(info["best_cost"]),
                best_num_inliers=info["best_num_inliers"])


@pytest.mark.parametrize("name", NONFINITE_FORWARD_CASES)
def test_ref_torch_nonfinite_matches_golden(name):
    """NaN / Inf inputs (nonfinite_checks.check_forward).  ref_torch's Sobel is the reference's
    conv2d, so the poisoned-gradient case sees a NaN at all nine positions of both planes."""
    gold, R, t, info = run_ref_torch_nonfinite(name)
    nf.check_forward(name, gold, _got(R, t, info))
    assert [s[0] for s in info["steps"]] == list(gold["rec_lam"])
    assert [s[1] for s in info["steps"]] == list(gold["rec_lr"])
    nf.assert_same_nonfinite(np.stack([s[2].numpy() for s in info["steps"]]), gold["rec_delta"], name)


@pytest.mark.parametrize("name", NONFINITE_RATIO_CASES)
def test_ref_torch_nonfinite_ratio_prefix_matches_golden(name):
    """What the reference recorded before it raised on the empty ratio mask (see
    tests/test_oracle_golden.py test_oracle_nonfinite_ratio_prefix_matches_golden)."""
    gold, R, t, info = run_ref_torch_nonfinite(name)
    nf.check_ratio_prefix(name, gold, dict(cost=np.array(info["costs"]), R=np.stack([r.numpy() for r in info["Rs"]]),
                                           t=np.stack([x.numpy() for x in info["ts"]]), n_kept=info["n_kept"]))
    assert [s[0] for s in info["steps"][:2]] == list(gold["rec_lam"])
    assert [s[1] for s in info["steps"][:2]] == list(gold["rec_lr"])
    sd = np.abs(gold["rec_delta"]).max(axis=1, keepdims=True)
    np.testing.assert_allclose(np.stack([s[2].numpy() for s in info["steps"][:2]]) / sd, gold["rec_delta"] / sd,
                               rtol=0, atol=1e-9)


@pytest.mark.parametrize("name", NONFINITE_PYRAMID_CASES)
def test_ref_torch_nonfinite_multilevel_matches_golden(name):
    """multilevel_optimization (model.py:193-213) composed from forward over channel slices: the
    first level breaks on the NaN step and hands its R_best to the two clean levels."""
    inp, meta, gold = case(name)
    f, gx, gy = poisoned_maps(inp, meta, _np_sobel)
    R, t = inp["R0"], inp["t0"]
    costs, status = [], []
    for c0, c1 in nf.pyramid_levels(meta):
        R, t, info = ref_torch.forward(inp["pts3d"], inp["fref"][:, c0:c1], f[c0:c1], gx[c0:c1], gy[c0:c1], inp["K"],
                                       int(inp["im_width"]), int(inp["im_height"]), R, t, meta["n_iters"],
                                       meta["lambda0"], meta["loss"])
        costs += info["costs"]
        status.append(info["status"])
    assert status == ["nan", "ok", "ok"]
    nf.assert_same_nonfinite(costs, gold["track_costs"], name)
    np.testing.assert_allclose(costs, gold["track_costs"], rtol=1e-10, equal_nan=True)
    np.testing.assert_allclose(R.numpy(), gold["out_R"], atol=1e-9)
    np.testing.assert_allclose(t.numpy(), gold["out_t"], atol=1e-9)
    assert float(info["best_cost"]) == pytest.approx(float(gold["best_cost_"]), rel=1e-10)
    assert info["best_num_inliers"] == int(gold["best_num_inliers_"])
