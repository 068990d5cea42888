"""Pixel rounding, support test and texel rescale at their boundaries -- the CPU tiers (no device).

The points come from tests/pixel_boundary_cases.py: quotients that ARE half-integers (rint's boundary, ties to
even) or lie a few ulps beside one, on the image's edges, behind the camera, at extreme depths, non-finite; and
pixel-centre sweeps over the (image, map) sizes at which an invariant-multiplier division can go wrong.  Random
points never land there (a quotient falls within 2^-49 relative of a half-integer with probability ~2^-46).

Checked here
  1. the generator's conditions: enough points survive in every class, a naive u * (1 / z) rounds another pixel
     than u / z at 30 points or more, and on every problem one point on a neighbouring texel or one toggled
     support bit moves the evaluation-0 cost by at least 1e3 times the tolerance it is compared under;
  2. tests/golden/pixel_boundary.npz, recorded from the reference's own forward: the generator's model, the
     oracle, fmpnp.refine.project_pixels and oracle/ref_torch.py give the reference's pixel, mask and texel
     exactly; the oracle's evaluation 0 has the reference's support count, its cost within 1e-10 relative;
  3. the CPU twin (fmpnp.cpu.refine_cpu) on every boundary and sweep problem, fp64 and fp32 storage, layouts
     fgrad and f, forward (n_iters = 1) and cost mode: evaluation 0's support count is the oracle's, its cost
     within the twin's tier of tests/test_cpu_twin.py (1e-10 relative fp64, 1e-6 fp32).

The extreme-depth and non-finite classes are not in the fixture: the reference casts such quotients to int,
which is undefined; for them the oracle is the definition, and they run in cost mode only (the Jacobian's 1 / z
is not claimed to match there).

The fixture's fused/ entries: at these points the reference's torch.mm(K, P.T) -- a BLAS kernel that accumulates
with fused multiply-adds for this operand layout and N >= 2, and without them for N = 1 or a strided operand --
rounds ANOTHER pixel than the sequential products every tier of this project (and the reference's own R X)
uses.  They are excluded from the comparison for that reason ("The reference's own K P"); the test
asserts that the fused chain explains every one of them.
"""
import collections

import numpy as np
import pytest
import torch

import oracle.oracle as orc
import pixel_boundary_cases as pb
from golden_io import load_npz
from oracle import ref_torch

from fmpnp import _lib, cpu, refine as rf

TIER = {"f64": 1e-10, "f32": 1e-6}     # tests/test_cpu_twin.py, tests/test_variant_coverage.py
BITE = 1e3                              # a single wrong point must move the cost by BITE * tolerance


def _all_problems():
    out = []
    for name in pb.GROUPS:
        out += pb.group_problems(name)
    return out + list(pb.sweep_problems())


# --- 1. the generator ---------------------------------------------------------------------------------------------
def test_generator_conditions():
    total = near = flips = 0
    flip_offsets = collections.Counter()
    for name in pb.GROUPS:
        g = pb.group(name)
        counts = collections.Counter(g["cls"].tolist())
        print(f"{name} ({g['pose']}, K {g['K_name']}, {g['W']}x{g['H']}): {len(g['X'])} points; "
              + ", ".join(f"{k} {v}" for k, v in sorted(counts.items())))
        pose, kname, size, axes, extra = pb.GROUPS[name]
        claimed = [f"half:{ax}:{o:+d}" for ax in axes for o in pb.group_offsets(name)]
        if "edge" in extra:
            claimed += [f"edge:{ax}:{tag}" for ax in "xy" for tag in ("-0.5", "0.5", "1.5")]
            claimed += ["edge:x:W-0.5", "edge:x:W+0.5", "edge:y:H-0.5", "edge:y:H+0.5"]
        claimed += ["zneg"] * ("zneg" in extra) + [f"extreme:{e}" for e in pb.EXTREME_DEPTHS if "extreme" in extra]
        claimed += ["nonfinite"] * ("nonfinite" in extra)
        for c in claimed:
            assert counts[c] >= 8, (name, c, counts[c])
        m = pb.pixel_model(g["R0"], g["t0"], g["X"], g["K"], g["W"], g["H"], g["Hf"], g["Wf"])
        # every adversarial quotient IS its target
        assert np.all(np.isnan(g["tx"]) | (m["qx"] == g["tx"])) and np.all(np.isnan(g["ty"]) | (m["qy"] == g["ty"]))
        half = np.char.startswith(g["cls"], "half")
        total += int(half.sum())
        near += int((half & (np.abs(g["off"]) <= 1)).sum())
        # even and odd k on ties, z < 0 where claimed
        tie = half & (g["off"] == 0)
        for tq in (g["tx"][tie & ~np.isnan(g["tx"])], g["ty"][tie & ~np.isnan(g["ty"])]):
            if len(tq):
                assert set(np.floor(tq).astype(int) % 2) == {0, 1}, name
        if "zneg" in extra:
            assert (m["u"][2][g["cls"] == "zneg"] < 0).all()
        with np.errstate(all="ignore"):
            r = 1.0 / m["u"][2]
            fl = half & ((np.rint(m["u"][0] * r) != np.rint(m["qx"])) | (np.rint(m["u"][1] * r) != np.rint(m["qy"])))
        flips += int(fl.sum())
        flip_offsets.update(g["off"][fl].tolist())
    print(f"half-integer points: {total}, at offsets 0 and +-1: {near}; points where u * (1 / z) rounds another "
          f"pixel than u / z: {flips}, by offset {dict(sorted(flip_offsets.items()))}")
    assert total >= 600 and 2 * near >= total
    assert flips >= 30


def test_every_problem_shows_a_single_wrong_point():
    """One point on a neighbouring texel, or one support bit toggled, moves evaluation 0's cost by at least
    1e3 x 1e-6 (the fp32 tier; the fp64 tier's 1e-10 is covered a fortiori) -- from the model's texel table,
    which is the oracle's cost (checked)."""
    worst = np.inf
    for p in _all_problems():
        for loss in ("squared", "geman_mcclure"):
            base, _ = pb.table_cost(p, loss)
            assert base > 0, p["name"]
            o = orc.compute_cost(p["pts3d"], p["fref"], p["fmap"], p["K"], p["im_width"], p["im_height"], p["R0"],
                                 p["t0"]) if loss == "squared" else None
            if o is not None:
                assert o == base, (p["name"], o, base)   # (compute_cost: the plain 0.5 ||e||^2 mean, exact sums)
            w = pb.min_single_point_change(p, loss)
            worst = min(worst, w)
            assert w >= BITE * TIER["f32"], (p["name"], loss, w)
    print(f"smallest relative cost change of a single wrong point over all problems: {worst:.3e}")


# --- 2. the fixture ---------------------------------------------------------------------------------------------
def _fixture(name):
    z = load_npz("pixel_boundary")
    return {k[len(name) + 1:]: v for k, v in z.items() if k.startswith(name + "/")}


FIXTURE_GROUPS = [g for g in pb.FINITE_GROUPS if not g.endswith("f16")]


@pytest.mark.parametrize("name", FIXTURE_GROUPS)
def test_fixture_every_tier_gives_the_references_pixels(name):
    f = _fixture(name)
    W, H, Hf, Wf = (int(v) for v in f["size"])
    X, K, R0, t0 = f["pts3d"], f["K"], f["R0"], f["t0"]
    g = pb.group(name)
    np.testing.assert_array_equal(X, g["X"][f["index"]])        # the generator still builds these points
    p2d, mask = f["points2d"].astype(np.int64), f["mask"].astype(bool)
    # the reference's texel as indexing_ writes it (model.py:88-89)
    rrow = np.floor(p2d[:, 1].astype(np.float64) * Hf / H).astype(np.int64)
    rcol = np.floor(p2d[:, 0].astype(np.float64) * Wf / W).astype(np.int64)

    def msg(i, tier):
        return (f"{tier}: {name} point {i}: class {f['cls'][i]}, pose {g['pose']}, K {g['K_name']}, X {X[i]!r}, "
                f"reference pixel {p2d[i]} mask {mask[i]}")

    m = pb.pixel_model(R0, t0, X, K, W, H, Hf, Wf)
    fmap = pb.id_map(Hf, Wf)
    omask, ocost, onsup = orc.find_inliers(X, np.zeros((len(X), 4)), fmap, K, W, H, R0, t0, np.inf)
    pp = rf.project_pixels(R0, t0, X, K)
    _, tp2, tm = ref_torch._project(torch.from_numpy(R0), torch.from_numpy(t0), torch.from_numpy(X),
                                    torch.from_numpy(K), W, H)
    trow, tcol = ref_torch._texels(tp2[tm], Hf, Wf, W, H)
    for i in range(len(X)):
        assert m["sup"][i] == mask[i] and m["px"][i] == p2d[i, 0] and m["py"][i] == p2d[i, 1], msg(i, "model")
        assert omask[i] == mask[i], msg(i, "oracle find_inliers")
        assert tuple(pp[i]) == tuple(p2d[i]), msg(i, "project_pixels")
        assert bool(tm[i]) == mask[i] and tuple(tp2[i].tolist()) == tuple(p2d[i]), msg(i, "ref_torch")
        if mask[i]:
            assert (m["row"][i], m["col"][i]) == (rrow[i], rcol[i]), msg(i, "model texel")
            ident = rrow[i] * Wf + rcol[i]
            want = 0.5 * (ident ** 2 + rcol[i] ** 2 + rrow[i] ** 2 + 1.0)
            assert ocost[i] == want, msg(i, f"oracle texel (cost {ocost[i]!r}, the reference's texel gives {want!r})")
    assert onsup == int(mask.sum())
    np.testing.assert_array_equal(trow.numpy(), rrow[mask])
    np.testing.assert_array_equal(tcol.numpy(), rcol[mask])
    # evaluation 0 through the oracle
    gx, gy = orc.sobel(fmap)
    prob = orc.make_problem(X, f["fref"], fmap, gx, gy, K, W, H, R0, t0)
    ores, otr = orc.forward(prob, orc.make_options(1, 0.01, "squared"), trace_cap=2)
    assert otr["n_supported"][0] == int(mask.sum())
    assert otr["cost"][0] == pytest.approx(float(f["cost0"]), rel=1e-10, abs=0)
    cc = orc.compute_cost(X, f["fref"], fmap, K, W, H, R0, t0)
    assert cc == pytest.approx(float(f["initial_cost"]), rel=1e-10, abs=0)
    assert ores["initial_cost"] == pytest.approx(float(f["initial_cost"]), rel=1e-10, abs=0)


@pytest.mark.parametrize("name", FIXTURE_GROUPS)
def test_fixture_left_out_points_are_the_references_fused_product(name):
    """The points the fixture leaves out: the reference rounded another pixel than the sequential model, and
    the fused accumulation of K P reproduces the reference's pixel at every one (see the module comment)."""
    f = _fixture(name)
    W, H, Hf, Wf = (int(v) for v in f["size"])
    X = f["fused/pts3d"]
    if not len(X):
        return
    m = pb.pixel_model(f["R0"], f["t0"], X, f["K"], W, H, Hf, Wf)
    p2d = f["fused/points2d"]
    assert ((m["px"] != p2d[:, 0]) | (m["py"] != p2d[:, 1])).all()
    fx, fy = pb.fused_pixels(f["R0"], f["t0"], X, f["K"])
    np.testing.assert_array_equal(fx, p2d[:, 0])
    np.testing.assert_array_equal(fy, p2d[:, 1])
    print(f"{name}: {len(X)} of {int(f['fused/N'])} chosen points left out, classes "
          f"{dict(collections.Counter(f['fused/cls'].tolist()))}")


# --- 3. the CPU twin ----------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle_eval0(p):
    """(n_supported, Geman-McClure cost) of evaluation 0 -- from orc.forward where the problem may run forward."""
    if p["name"] not in _ORACLE:
        gx, gy = orc.sobel(p["fmap"])
        prob = orc.make_problem(p["pts3d"], p["fref"], p["fmap"], gx, gy, p["K"], p["im_width"], p["im_height"],
                                p["R0"], p["t0"])
        if p["group"] == "extreme":
            mask, _, nsup = orc.find_inliers(p["pts3d"], p["fref0"], p["fmap"], p["K"], p["im_width"],
                                             p["im_height"], p["R0"], p["t0"], np.inf)
            _ORACLE[p["name"]] = (nsup, None, gx, gy)
        else:
            _, otr = orc.forward(prob, orc.make_options(1, 0.01, "geman_mcclure"), trace_cap=2)
            _ORACLE[p["name"]] = (int(otr["n_supported"][0]), float(otr["cost"][0]), gx, gy)
        assert _ORACLE[p["name"]][0] == int(p["model"]["sup"].sum()), p["name"]   # the oracle against the model
    return _ORACLE[p["name"]]


@pytest.mark.parametrize("dt,layout", [("f64", "fgrad"), ("f32", "fgrad"), ("f32", "f")])
def test_twin_on_every_boundary_and_sweep_problem(dt, layout):
    dtype = np.float64 if dt == "f64" else np.float32
    for p in _all_problems():
        nsup, ocost, gx, gy = _oracle_eval0(p)
        feats = cpu.pack_host(p["fmap"], gx, gy, dtype) if layout == "fgrad" else \
            cpu.pack_host(p["fmap"], dtype=dtype, layout="f")
        prob = cpu.problem_host(feats, p["fref"], p["pts3d"], p["K"], p["im_width"], p["im_height"], p["R0"], p["t0"])
        what = f"twin {dt} {layout}: {p['name']} (pose {p['pose']}, K {p['K_name']})"
        ccost = orc.compute_cost(p["pts3d"], p["fref"], p["fmap"], p["K"], p["im_width"], p["im_height"], p["R0"],
                                 p["t0"])
        (res,), _ = cpu.refine_cpu([prob], rf.make_options(0, mode=_lib.MODE_COMPUTE_COST), n_threads=1)
        assert res["initial_cost"] == pytest.approx(ccost, rel=TIER[dt], abs=0), what + " cost mode"
        if p["group"] == "extreme":
            continue
        (res,), (tr,) = cpu.refine_cpu([prob], rf.make_options(1, 0.01, _lib.GEMAN_MCCLURE), trace=True, n_threads=1)
        assert tr["n_supported"][0] == nsup, what
        assert tr["cost"][0] == pytest.approx(ocost, rel=TIER[dt], abs=0), what
        assert res["initial_cost"] == pytest.approx(ocost, rel=TIER[dt], abs=0), what
