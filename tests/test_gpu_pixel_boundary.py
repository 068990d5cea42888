"""Pixel rounding, support test and texel rescale at their boundaries -- every GPU projection site.

The points are those of tests/pixel_boundary_cases.py (see tests/test_pixel_boundary_cpu.py for what they are
and for the generator's own conditions): quotients that are half-integers or lie a few ulps beside one, the
image's edges, z < 0, extreme depths, NaN / Inf, and pixel-centre sweeps over awkward (image, map) sizes.

Everything is compared with the oracle (oracle/fmpnp_oracle.c) on the same inputs at evaluation 0 only --
trace[0] and initial_cost with n_iters = 1: the integer-valued maps are not smooth, later evaluations prove
nothing.  Tolerances are the identical-inputs tier of tests/test_variant_coverage.py: n_supported equal, cost
1e-10 relative for fp64 (and binary16: exact widening) texels, 1e-6 for fp32 texels.  Per point
(fmpnp_point_costs) `supported` is the oracle's mask and the cost exactly the oracle's: the sums are exact.

Sites: project_px (fmpnp_point_costs, fmpnp_compute_cost_async, bilinear, non-pinhole K), project_pc's guarded
reciprocal in eval_pass (latency and throughput builds, teams, the 512-point carve, layout f, binary16) and in
the first-evaluation helpers (B = 1), cost mode through the LM launch (the only place the extreme-depth and
non-finite classes run), the multiplier rescale (udiv) against fmpnp_points.hip's plain division.

That it bites (measured on gfx950, a scratch build whose guard in project_pc is 2^-60 instead of 2^-49): 13 of the
44 tests here fail -- every LM evaluation-0 case and cost mode; as one-point problems 70 of 6466 boundary points
flip, all of them exact ties (offset 0; none at +-1 ulp or beyond, none through the non-pinhole K's project_px
branch).  The shipped guard sends neighbours 9, 15, 16, 17 and 64 ulps from a tie (1345 targets) to the
reciprocal's product, and every one agrees with the exact division.
"""
import numpy as np
import pytest
import torch

import oracle.oracle as orc
import pixel_boundary_cases as pb

pytestmark = pytest.mark.gpu

from fmpnp import _lib, refine as rf  # noqa: E402  (no skip: a missing HIP library must fail)

DEV = "cuda:0"
TIER = {"f64": 1e-10, "f16": 1e-10, "f32": 1e-6}
STORAGE = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16}
CODE = {"f64": _lib.F64, "f32": _lib.F32, "f16": _lib.F16}
# the groups that share the 64 x 48 image (one launch may mix them) and the odd-sized one
MAIN = ("ident-std", "shift-off", "perm-std", "general-off", "ident-skew", "shift-w2", "ident-off-odd")

_FEATS, _ORC = {}, {}


def _feats(p, dt, layout):
    key = (p["fmap"].shape, float(p["fmap"][0].sum()), dt, layout)
    if key not in _FEATS:
        fm = torch.from_numpy(p["fmap"]).to(torch.float64 if dt == "f64" else torch.float32)
        # (evaluation 0 reads no gradient: zeros are packed as given, the maps here go down to one row or column)
        g0 = torch.zeros_like(fm) if layout == "fgrad" else None
        _FEATS[key] = rf.pack_features(fm, g0, g0, storage=STORAGE[dt], device=DEV, layout=layout)
    return _FEATS[key]


def _dev(p, dt, layout="fgrad", fref="fref"):
    feats = _feats(p, dt, layout)
    return rf.make_problem(feats, torch.from_numpy(p[fref]).to(STORAGE[dt] if dt != "f16" else torch.float32),
                           p["pts3d"], p["K"], p["im_width"], p["im_height"], p["R0"], p["t0"])


def _oracle(p, ratio=None, sampling="nearest", mode="fwd"):
    """Evaluation 0 of the oracle: (n_supported, Geman-McClure cost), or the compute_cost value."""
    key = (p["name"], len(p["pts3d"]), ratio, sampling, mode)
    if key not in _ORC:
        if mode == "cost":
            _ORC[key] = orc.compute_cost(p["pts3d"], p["fref"], p["fmap"], p["K"], p["im_width"], p["im_height"],
                                         p["R0"], p["t0"], ratio)
        else:
            gx, gy = orc.sobel(p["fmap"])
            prob = orc.make_problem(p["pts3d"], p["fref"], p["fmap"], gx, gy, p["K"], p["im_width"], p["im_height"],
                                    p["R0"], p["t0"])
            _, tr = orc.forward(prob, orc.make_options(1, 0.01, "geman_mcclure", ratio, sampling=sampling), 2)
            _ORC[key] = (int(tr["n_supported"][0]), float(tr["cost"][0]))
    return _ORC[key]


def _what(case, p):
    return (f"{case}: {p['name']} (pose {p['pose']}, K {p['K_name']}, {len(p['pts3d'])} points, classes "
            f"{sorted(set(c.rsplit(':', 1)[0] for c in p['cls'].tolist()))})")


def _problems(groups, n):
    return [p for g in groups for p in pb.group_problems(g, n)]


# --- per point: project_px, the plain-division rescale ------------------------------------------------------------
@pytest.mark.parametrize("group,dt", [(g, dt) for g in pb.GROUPS for dt in ("f64", "f32")] + [("ident-std-f16", "f16")])
def test_point_costs_name_every_texel(group, dt):
    for p in pb.group_problems(group):
        omask, ocost, _ = orc.find_inliers(p["pts3d"], p["fref0"], p["fmap"], p["K"], p["im_width"], p["im_height"],
                                           p["R0"], p["t0"], np.inf)
        np.testing.assert_array_equal(omask, p["model"]["sup"])      # the oracle against the generator's model
        cost, sup = rf.point_costs(_dev(p, dt, fref="fref0"))
        cost, sup = cost.cpu().numpy(), sup.cpu().numpy()
        for i in np.nonzero((sup != omask) | (cost != ocost))[0][:5]:
            raise AssertionError(f"fmpnp_point_costs {dt}: supported {sup[i]} cost {cost[i]!r}, the oracle's "
                                 f"{omask[i]} {ocost[i]!r} at " + pb.describe(p, i))
        r = rf.compute_cost(_dev(p, dt))
        assert r["initial_cost"] == pytest.approx(_oracle(p, mode="cost"), rel=TIER[dt], abs=0), \
            _what(f"fmpnp_compute_cost_async {dt}", p)


# --- the LM kernel: every projection site and build -------------------------------------------------------------------
# name -> (dt, layout, B, N, wgs_per_problem, helpers, expected (build, team, variant), groups)
LM_CASES = {
    "eval_pass-f64-N128":  ("f64", "fgrad", 128, 128, 0, -1, ("latency", 0, "GM_SPEC"), MAIN),
    "eval_pass-f64-N130":  ("f64", "fgrad", 128, 130, 0, -1, ("latency", 0, "GM_SPEC"), MAIN),
    "eval_pass-f32-N480":  ("f32", "fgrad", 128, 480, 0, -1, ("latency", 0, "GM_SPEC_512"), MAIN),
    "helpers-f64-B1":      ("f64", "fgrad", 1, 128, 0, 0, ("latency", 0, "GM_SPEC_H"), MAIN),
    # (not the odd-sized group: 339 points, no 512-point carve)
    "helpers-f32-B1-N480": ("f32", "fgrad", 1, 480, 0, 0, ("latency", 0, "GM_SPEC_H_512"), MAIN[:-1]),
    "team-f64":            ("f64", "fgrad", 1, 128, 2, -1, ("latency", 1, "GM"), MAIN),
    "throughput-f32":      ("f32", "fgrad", 512, 128, 0, -1, ("throughput", 0, "GM"), MAIN),
    "layout_f-f32":        ("f32", "f", 1, 128, 1, -1, ("latency", 0, "F_GM"), MAIN),
    "binary16":            ("f16", "fgrad", 128, 128, 0, -1, ("latency", 0, "GM_SPEC"), ("ident-std-f16",)),
}
LM_RUNS = [(c, None) for c in LM_CASES] + [("eval_pass-f64-N128", 0.8), ("eval_pass-f32-N480", 0.8)]


@pytest.mark.parametrize("case,ratio", LM_RUNS, ids=[f"{c}-{'r08' if r else 'nor'}" for c, r in LM_RUNS])
def test_lm_evaluation_0_against_oracle(case, ratio):
    dt, layout, B, N, wgs, helpers, (build, team, variant), groups = LM_CASES[case]
    distinct = _problems(groups, N)
    opts = rf.make_options(1, 0.01, _lib.GEMAN_MCCLURE, ratio_threshold=ratio, dtype=CODE[dt], wgs_per_problem=wgs,
                           helpers=helpers)
    devs = [_dev(p, dt, layout) for p in distinct]
    # B = 1: one launch per problem (the helpers project exactly the initial pose); else one batch that repeats them
    launches = [[i] for i in range(len(distinct))] if B == 1 else [[i % len(distinct) for i in range(B)]]
    for idx in launches:
        res, trs = rf.refine([devs[i] for i in idx], opts, trace=True)
        info = _lib.last_launch()
        got = (info["dtype_name"], info["build_name"], int(info["team"]), int(info["ratio"]), info["variant_name"])
        assert got == (dt, build, team, int(ratio is not None), variant), (case, info)
        for q in sorted(set(list(range(min(len(idx), len(distinct)))) + [len(idx) - 1])):
            p = distinct[idx[q]]
            if ratio is not None and q != 0:    # (the ratio test: on the first item only)
                continue
            nsup, cost = _oracle(p, ratio)
            what = _what(f"{case} ratio={ratio} item {q}", p)
            assert trs[q]["n_supported"][0] == nsup, what
            assert trs[q]["cost"][0] == pytest.approx(cost, rel=TIER[dt], abs=0), what
            assert res[q]["initial_cost"] == pytest.approx(cost, rel=TIER[dt], abs=0), what


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_lm_cost_mode_with_extreme_depth_and_nonfinite_points(dt):
    """Cost mode through the LM launch: every group, and the only run of the extreme-depth and non-finite
    classes -- |z| outside [2^-1000, 2^1000], NaN / Inf coordinates (project_pc's exact-division fallback), for
    which the oracle is the definition (the reference's int cast of such quotients is undefined)."""
    probs = _problems(MAIN + ("extreme",), 480)
    for ratio in (None, 0.8):
        opts = rf.make_options(0, ratio_threshold=ratio, dtype=CODE[dt], mode=_lib.MODE_COMPUTE_COST)
        for batch in ([probs[-1]], probs):      # B = 1 (the team spread), and one batch
            res, _ = rf.refine([_dev(p, dt) for p in batch], opts)
            for p, r in zip(batch, res):
                assert r["initial_cost"] == pytest.approx(_oracle(p, ratio, mode="cost"), rel=TIER[dt], abs=0), \
                    _what(f"LM cost mode {dt} ratio={ratio} B={len(batch)}", p)


@pytest.mark.parametrize("memo", [False, True], ids=["direct", "memo"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_bilinear_support_edges(dt, memo):
    """Bilinear sampling is continuous across a cell edge, so only the mask is at stake: the support-edge
    classes against the oracle's bilinear."""
    probs = []
    for name in MAIN:
        g = pb.group(name)
        sel = np.char.startswith(g["cls"], "edge")
        if sel.any():
            probs.append(pb.make_problem(f"{name}[edges]", g["R0"], g["t0"], g["K"], g["W"], g["H"],
                                         pb.id_map(g["Hf"], g["Wf"]), g["X"][sel], group=name, pose=g["pose"],
                                         K_name=g["K_name"], cls=g["cls"][sel], off=g["off"][sel]))
    opts = rf.make_options(1, 0.01, _lib.GEMAN_MCCLURE, dtype=CODE[dt], sampling="bilinear", memoize=memo,
                           speculate=memo, wgs_per_problem=0 if memo else 1)
    batch = [probs[i % len(probs)] for i in range(128 if memo else len(probs))]
    res, trs = rf.refine([_dev(p, dt) for p in batch], opts, trace=True)
    info = _lib.last_launch()
    assert info["variant_name"] == ("BILINEAR" if memo else "BIL_DIRECT"), info
    for p, r, tr in zip(batch[:len(probs)], res, trs):
        nsup, cost = _oracle(p, sampling="bilinear")
        what = _what(f"bilinear {'memo' if memo else 'direct'} {dt}", p)
        assert nsup == int(p["model"]["sup"].sum()), what
        assert tr["n_supported"][0] == nsup, what
        assert tr["cost"][0] == pytest.approx(cost, rel=TIER[dt], abs=0), what


# --- the rescale sweeps -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_rescale_sweeps_per_point(dt):
    for p in pb.sweep_problems():
        omask, ocost, _ = orc.find_inliers(p["pts3d"], p["fref0"], p["fmap"], p["K"], p["im_width"], p["im_height"],
                                           p["R0"], p["t0"], np.inf)
        m = p["model"]
        assert omask.all() and np.array_equal(ocost, 0.5 * (m["col"] ** 2.0 + m["row"] ** 2.0 + 1.0)), p["name"]
        cost, sup = rf.point_costs(_dev(p, dt, fref="fref0"))
        cost, sup = cost.cpu().numpy(), sup.cpu().numpy()
        for i in np.nonzero(~sup | (cost != ocost))[0][:5]:
            raise AssertionError(f"fmpnp_point_costs {dt}: supported {sup[i]} cost {cost[i]!r}, the oracle's "
                                 f"{ocost[i]!r} at " + pb.describe(p, i))


@pytest.mark.parametrize("wgs", [1, 2])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_rescale_sweeps_through_the_lm_kernel(dt, wgs):
    """udiv_make / udiv (fmpnp_device.h) at d = 1, powers of two, 2^k +- 1, maps larger than the image and
    products just under 2^32: evaluation 0 against the oracle's plain division."""
    probs = list(pb.sweep_problems())
    opts = rf.make_options(1, 0.01, _lib.GEMAN_MCCLURE, dtype=CODE[dt], wgs_per_problem=wgs)
    res, trs = rf.refine([_dev(p, dt) for p in probs], opts, trace=True)
    assert int(_lib.last_launch()["team"]) == (wgs > 1)
    for p, r, tr in zip(probs, res, trs):
        nsup, cost = _oracle(p)
        what = _what(f"sweep {dt} wgs_per_problem={wgs}", p)
        assert tr["n_supported"][0] == nsup == len(p["pts3d"]), what
        assert tr["cost"][0] == pytest.approx(cost, rel=TIER[dt], abs=0), what


# --- launch independence ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 128])
def test_evaluation_0_is_independent_of_the_launch(B):
    """Helpers on or off, speculation on or off, no_memo 0 / 1 / 2: identical evaluation-0 trace entries
    (the project's bit-for-bit tier), whichever of eval_pass and helper_run projected the initial pose."""
    distinct = _problems(MAIN, 128)
    idx = [i % len(distinct) for i in range(B)] if B > 1 else None
    seen = {}
    for helpers in (0, -1):
        for no_memo in (0, 1, 2):
            opts = rf.make_options(1, 0.01, _lib.GEMAN_MCCLURE, dtype=_lib.F64, helpers=helpers)
            opts.no_memo = no_memo
            runs = [[i] for i in range(0, len(distinct), 7)] if B == 1 else [idx]
            out = []
            for run in runs:
                _, trs = rf.refine([_dev(distinct[i], "f64") for i in run], opts, trace=True)
                out += [(int(t["n_supported"][0]), float(t["cost"][0])) for t in trs]
            seen[(helpers, no_memo)] = out
    first = seen[(0, 0)]
    for k, v in seen.items():
        assert [a for a, _ in v] == [a for a, _ in first], k
        assert v == first, k
