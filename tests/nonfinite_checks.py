"""What every tier must reproduce on the NaN / Inf goldens (golden_io.NONFINITE_CASES), shared by
the oracle, ref_torch, CPU-twin and GPU tests.

The reference's NaN-step exit (featurePnP/model.py:411-413) and what rides on it:
  * a NaN trial cost is accepted (`new_cost > prev_cost` is False, model.py:472) but never
    becomes the best (`new_cost < best_cost_` is False, :479);
  * the step after it is NaN, the loop breaks and R_best -- not the current pose -- is returned;
  * the NaN step counts as a step: n_steps == n_evals where the run broke, n_evals - 1 otherwise;
  * a NaN first cost leaves best_cost_ set and NaN (:349).
An Inf texel gives an Inf (squared, Huber) or saturated (Cauchy: the 33e37 clamp; Geman-McClure:
rho -> 4) trial cost, which is rejected: the run goes on for all its iterations.
"""
import numpy as np

# where the reference breaks on a NaN step (the others run all their iterations, status OK)
BREAKS = {"nan_texel_gm": True, "nan_texel_gm_lambda0": True, "nan_grad_first_step_gm": True, "nan_fref_gm": True,
          "inf_texel_gm": False, "inf_texel_cauchy": False, "inf_texel_squared": False, "inf_texel_huber": False}


def accepts(costs):
    """accept/reject sequence from tracked costs (model.py:469-486); a NaN cost is accepted."""
    acc, prev = [], costs[0]
    for c in costs[1:]:
        a = not (c > prev)
        acc.append(a)
        if a:
            prev = c
    return acc


def rot_angle(Ra, Rb):
    c = (np.trace(np.asarray(Ra).T @ np.asarray(Rb)) - 1.0) / 2.0
    return float(np.arccos(np.clip(c, -1.0, 1.0)))


def assert_same_nonfinite(a, b, what=""):
    """NaN, +Inf and -Inf at the same indices."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=what)
    np.testing.assert_array_equal(np.isposinf(a), np.isposinf(b), err_msg=what)
    np.testing.assert_array_equal(np.isneginf(a), np.isneginf(b), err_msg=what)


def check_forward(name, gold, got, fp32=False):
    """`got`: nan (status is the NaN exit), ok (status is 0 otherwise), n_evals, n_steps,
    n_accepted, cost [n_evals], n_supported [n_evals] or None, R, t, has_best, best_cost,
    best_num_inliers -- against the reference's golden.  fp64 tolerances: costs 1e-10 relative,
    pose 1e-9; fp32 texels (fp32=True): costs 1e-6 relative, pose 1e-4 rad / 1e-4 m, counts,
    status and the NaN / Inf positions identical."""
    gc = gold["track_costs"]
    assert got["nan"] == BREAKS[name] and got["ok"] == (not BREAKS[name]), (name, got["nan"], got["ok"])
    assert got["n_evals"] == len(gc), name
    assert got["n_steps"] == int(gold["rec_n"]), name
    assert got["n_steps"] == got["n_evals"] - (0 if BREAKS[name] else 1), name
    assert got["n_accepted"] == sum(accepts(list(gc))), name
    assert_same_nonfinite(got["cost"], gc, name)
    np.testing.assert_allclose(got["cost"], gc, rtol=1e-6 if fp32 else 1e-10, atol=0, equal_nan=True, err_msg=name)
    if got.get("n_supported") is not None:
        np.testing.assert_array_equal(got["n_supported"], gold["track_npts"], err_msg=name)
    if fp32:
        assert rot_angle(got["R"], gold["out_R"]) < 1e-4, name
        assert np.linalg.norm(np.asarray(got["t"]) - gold["out_t"]) < 1e-4, name
    else:
        np.testing.assert_allclose(got["R"], gold["out_R"], rtol=0, atol=1e-9, err_msg=name)
        np.testing.assert_allclose(got["t"], gold["out_t"], rtol=0, atol=1e-9, err_msg=name)
    assert bool(got["has_best"]) == bool(gold["has_best_cost_"]), name
    np.testing.assert_allclose(got["best_cost"], float(gold["best_cost_"]), rtol=1e-6 if fp32 else 1e-10, atol=0,
                               equal_nan=True, err_msg=name)
    assert got["best_num_inliers"] == int(gold["best_num_inliers_"]), name


def check_ratio_prefix(name, gold, got):
    """The ratio cases: the reference raises in its third iteration (model.py:95, an empty
    torch.cat), so only what it recorded before is pinned: three tracked costs and poses, and
    nothing kept at evaluation 2.  `got`: cost, R, t (traces), n_kept."""
    assert len(gold["track_costs"]) == 3 and int(gold["rec_n"]) == 2, name
    assert_same_nonfinite(got["cost"][:3], gold["track_costs"], name)
    assert np.isnan(got["cost"][2]), name
    np.testing.assert_allclose(got["cost"][:3], gold["track_costs"], rtol=1e-10, atol=0, equal_nan=True,
                               err_msg=name)
    np.testing.assert_allclose(got["R"][:3], gold["track_R"], rtol=0, atol=1e-9, err_msg=name)
    np.testing.assert_allclose(got["t"][:3], gold["track_t"], rtol=0, atol=1e-9, err_msg=name)
    assert got["n_kept"][0] > 0 and got["n_kept"][1] > 0 and got["n_kept"][2] == 0, (name, got["n_kept"][:3])


def from_oracle(res, tr):
    return dict(nan=res["status"] == "nan", ok=res["status"] == "ok", n_evals=res["n_evals"], n_steps=res["n_steps"],
                n_accepted=res["n_accepted"], cost=tr["cost"], n_supported=tr["n_supported"], R=res["R"], t=res["t"],
                has_best=res["has_best"], best_cost=res["best_cost"], best_num_inliers=res["best_num_inliers"])


def from_fmpnp(res, tr, status_nan, ignore=0):
    """A result / trace of fmpnp.refine.refine or fmpnp.cpu.refine_cpu."""
    st = res["status"] & ~ignore
    return dict(nan=st == status_nan, ok=st == 0, n_evals=res["n_evals"], n_steps=res["n_steps"],
                n_accepted=res["n_accepted"], cost=tr["cost"], n_supported=tr["n_supported"], R=res["R"], t=res["t"],
                has_best=res["has_best"], best_cost=res["best_cost"], best_num_inliers=res["best_num_inliers"])


def pyramid_levels(meta):
    """(c_begin, c_end) of every level of a pyramid case whose levels only slice channels."""
    assert all(ts is None and ks is None for _, _, ts, ks in meta["pyramid"])
    return [(s, e) for s, e, _, _ in meta["pyramid"]]
