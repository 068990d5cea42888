"""The trimmed block partial of the speculating LM variants without the ratio test (fmpnp_lm_impl.h: reduce28_in64,
reduce28_index, contrib_geo<B28>).

In VAR_GM_SPEC, VAR_GM_SPEC_512, VAR_NEAREST_SPEC and their _H forms a block's partial is reduced over the wave
without its four spare slots: the 27 normal-equation sums and rho go through a 28-value tree, and the kept and
supported counts, one predicate there, are the popcount of a ballot.  That may not change a bit of a result, and
predictions only choose what is fetched early (the prediction formed behind barrier 1, measured with this change
and not adopted, was held to the same cases).  So every case runs the same problems through the planner's
choice (a trimmed _SPEC variant, one workgroup per problem, no team) and through speculate=False (a plain
variant: reduce32_in64, no predictions), and asserts
  * every field of bench.DUMP_FIELDS equal (np.array_equal, NaN for NaN);
  * the per-evaluation traces equal: pose, cost, damping, supported and kept counts and the decision at every
    evaluation, not only at the best one;
  * no FMPNP_STATUS_SYNC_TIMEOUT;
and checks the trimmed run against the oracle at tests/test_gpu_parity.py's tolerances for fp32 texels (pose
within 1e-4 rad / 1e-4 m; n_evals, n_steps, n_accepted, best_num_inliers and status identical; final_lambda and
final_lr to 1e-12 relative).  For binary16 storage the oracle reads the values as the pack rounds them.

Shapes: a 12 x 16 map (48 x 64 image), 50 iterations, lambda0 = 0.01, Geman-McClure and Cauchy (the GM and
NEAREST variants); a batch of three (hard, easy, hard start) without helpers and one query with the
first-evaluation helpers, whose records must be the batch's for the same query (the planner gives helpers to
problems of two blocks and more: N = 1 and N = 64 run that query alone without them).
  N = 64           one full block
  N = 70           a full block and a block of 6 points: the ballot's count skips the invalid lanes
  N = 1            a count of one, every partner lane invalid
  N = 96           a last block whose high half is empty: the bit-5 partners are all invalid
  N = 449, 480, 512   the 512-point carve at its lower bound (a last block of one point), with a half block, full
  C = 256 and C = 40 at fp32; fp64 (C = 128) and binary16 (C = 512) at N = 70: all three units compile the change.
"""
import numpy as np
import pytest
import torch

import nonfinite_checks as nf
import oracle.oracle as orc

pytestmark = pytest.mark.gpu

from bench import DUMP_FIELDS  # noqa: E402
from f16_storage_cases import rounded_maps  # noqa: E402
from fmpnp import _lib, refine as rf, synth  # noqa: E402  (no skip: a missing HIP library must fail)

DEV = "cuda:0"
ITERS, HF, WF = 50, 12, 16
LOSS = {"geman_mcclure": _lib.GEMAN_MCCLURE, "cauchy": _lib.CAUCHY}
QUIET = _lib.STATUS_HELPER_WAIT  # informational and timing dependent: not part of a result
STORAGE = {"f32": (torch.float32, _lib.F32), "f64": (torch.float64, _lib.F64), "f16": (torch.float16, _lib.F16)}
STARTS = [(1, "hard"), (2, "easy"), (3, "hard")]  # (synth seed, start) of the batch's three queries
ORC_STATUS = {"ok": _lib.STATUS_OK, "no_support": _lib.STATUS_NO_SUPPORT, "nan": _lib.STATUS_NAN,
              "no_support_trial": _lib.STATUS_NO_SUPPORT_TRIAL}
TRACE_FIELDS = ("R", "t", "cost", "lam", "lr", "n_supported", "n_kept", "accepted")

# id -> (storage, C, N)
SHAPES = {
    "f32-C256-N64": ("f32", 256, 64),
    "f32-C256-N70": ("f32", 256, 70),
    "f32-C256-N1": ("f32", 256, 1),
    "f32-C256-N96": ("f32", 256, 96),
    "f32-C256-N449": ("f32", 256, 449),
    "f32-C256-N480": ("f32", 256, 480),
    "f32-C256-N512": ("f32", 256, 512),
    "f32-C40-N70": ("f32", 40, 70),
    "f32-C40-N96": ("f32", 40, 96),
    "f64-C128-N70": ("f64", 128, 70),
    "f16-C512-N70": ("f16", 512, 70),
}

_INPUTS = {}
_ORACLE = {}


def _inputs(C, n_pts, seed, init):
    key = (C, n_pts, seed, init)
    if key not in _INPUTS:
        _INPUTS[key] = synth.problem_inputs(n_pts, C, HF, WF, seed=seed, device="cpu", init=init)
    return _INPUTS[key]


def _oracle(inp, storage, loss):
    """The oracle on the values the kernel reads: the fp32 map with the fp64 Sobel, or (binary16) every plane
    and the descriptors as the pack rounds them.  Returns (result, trace)."""
    f = inp["fmap"].double().cpu().numpy()
    fref = inp["fref"].double().cpu().numpy()
    if storage == "f16":
        f, gx, gy, fref = rounded_maps(inp["fmap"].cpu().numpy(), fref)
    else:
        gx, gy = orc.sobel(f)
    p = orc.make_problem(inp["pts3d"], fref, f, gx, gy, inp["K"], inp["im_width"], inp["im_height"], inp["R0"],
                         inp["t0"], 0, f.shape[0])
    return orc.forward(p, orc.make_options(ITERS, 0.01, loss), trace_cap=ITERS + 1)


def _oracle_of(C, n_pts, seed, init, storage, loss):
    key = (C, n_pts, seed, init, storage, loss)
    if key not in _ORACLE:
        _ORACLE[key] = _oracle(_inputs(C, n_pts, seed, init), storage, loss)
    return _ORACLE[key]


def _problem(inp, storage):
    feats = rf.pack_features(inp["fmap"], storage=STORAGE[storage][0], device=DEV)
    return rf.make_problem(feats, inp["fref"], inp["pts3d"], inp["K"], inp["im_width"], inp["im_height"], inp["R0"],
                           inp["t0"])


def _quiet(r):
    return dict(r, status=r["status"] & ~QUIET)


def _same_records(a, b, what):
    for k in DUMP_FIELDS:
        assert np.array_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64),
                              equal_nan=True), (what, k, a[k], b[k])


def _same_traces(a, b, what):
    for k in TRACE_FIELDS:
        assert np.array_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64),
                              equal_nan=True), (what, "trace", k, a[k], b[k])


def _both_ways(probs, dtype, loss, helpers, what):
    """The problems through the planner's choice, which must be a trimmed _SPEC variant with one workgroup per
    problem and no team, and through speculate=False (a plain variant): records and traces equal field by
    field, no timeout.  Returns the first run's results, traces and launch plan, and the plain run's results."""
    res, tr = rf.refine(probs, rf.make_options(ITERS, 0.01, LOSS[loss], dtype=dtype, helpers=helpers), trace=True)
    info = _lib.last_launch()
    assert "_SPEC" in info["variant_name"], (what, info)
    assert info["wgs_per_problem"] == 1 and not info["team"], (what, info)
    plain, ptr = rf.refine(probs, rf.make_options(ITERS, 0.01, LOSS[loss], dtype=dtype, helpers=helpers,
                                                  speculate=False), trace=True)
    assert "SPEC" not in _lib.last_launch()["variant_name"], (what, _lib.last_launch())
    for q, (r, p) in enumerate(zip(res, plain)):
        assert r["status"] & _lib.STATUS_SYNC_TIMEOUT == 0 and p["status"] & _lib.STATUS_SYNC_TIMEOUT == 0, (what, q)
        _same_records(_quiet(r), _quiet(p), f"{what} query {q}: trimmed vs plain variant")
        _same_traces(tr[q], ptr[q], f"{what} query {q}: trimmed vs plain variant")
    return res, tr, info, plain


def _check_oracle(res, ores, what):
    """tests/test_gpu_parity.py's fp32 tolerances on the pose; the schedule, the count and the status identical."""
    assert res["status"] & ~QUIET == ORC_STATUS[ores["status"]], (what, ores["status"], res["status"])
    assert nf.rot_angle(res["R"], ores["R"]) < 1e-4, what
    assert np.linalg.norm(res["t"] - ores["t"]) < 1e-4, what
    for k in ("n_evals", "n_steps", "n_accepted", "best_num_inliers"):
        assert res[k] == ores[k], (what, k, res[k], ores[k])
    assert res["final_lambda"] == pytest.approx(ores["final_lambda"], rel=1e-12), what
    assert res["final_lr"] == pytest.approx(ores["final_lr"], rel=1e-12), what


@pytest.mark.parametrize("loss", ["geman_mcclure", "cauchy"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_trimmed_equals_plain_and_oracle(shape, loss, monkeypatch):
    monkeypatch.delenv("FMPNP_SPEC_CAP", raising=False)
    storage, C, n_pts = SHAPES[shape]
    dtype = STORAGE[storage][1]
    inps = [_inputs(C, n_pts, seed, init) for seed, init in STARTS]
    probs = [_problem(inp, storage) for inp in inps]
    # B = 3, no helpers
    res, tr, info, _ = _both_ways(probs, dtype, loss, -1, f"{shape} {loss} B=3")
    assert info["helpers"] == 0, info
    if n_pts > 448 and storage == "f32" and loss == "geman_mcclure":
        assert "512" in info["variant_name"], info  # (the 512-point carve: the Geman-McClure variants have one)
    for q, (r, (seed, init)) in enumerate(zip(res, STARTS)):
        ores, otr = _oracle_of(C, n_pts, seed, init, storage, loss)
        _check_oracle(r, ores, f"{shape} {loss} B=3 query {q}")
        np.testing.assert_array_equal(tr[q]["n_supported"], otr["n_supported"], err_msg=f"{shape} {loss} query {q}")
    # B = 1 with the first-evaluation helpers: the helpers' sums are the main workgroup's
    # (the planner gives helpers to problems of two blocks and more: N = 1 and N = 64 run the same query alone)
    one, otr1, info, _ = _both_ways(probs[:1], dtype, loss, 0, f"{shape} {loss} B=1 helpers")
    assert (info["helpers"] > 0) == (n_pts > 64) and ("_H" in info["variant_name"]) == (n_pts > 64), info
    _same_records(_quiet(one[0]), _quiet(res[0]), f"{shape} {loss}: with helpers vs without")
    _same_traces(otr1[0], tr[0], f"{shape} {loss}: with helpers vs without")


# ---------------------------------------------------------------------------
# Points without support (N = 70, C = 40, fp32): the supported count is the ballot's, below N at every
# evaluation and changing over the run; an unsupported point keeps its last supported pixel as the motion's
# origin and gets no prediction.
# ---------------------------------------------------------------------------
FAR = [0, 1, 2, 64, 65, 69]                 # pushed 8 px and more left of the image, for good (both blocks)
EDGE = list(range(10, 18)) + [66, 67]       # put across the left / right border from where they start
EDGE_FRAC = 0.3                             # ... with this part of their start-to-identity motion inside


def _pixels(R, t, X, K):
    P = X @ np.asarray(R).T + np.asarray(t)
    return np.stack([K[0, 0] * P[:, 0] / P[:, 2] + K[0, 2], K[1, 1] * P[:, 1] / P[:, 2] + K[1, 2]], 1)


def _unsupported_inputs():
    """The hard-start synth problem with FAR moved out of the image and EDGE moved onto a vertical border, so
    that the start pose and the identity pose (where the run heads) see each on different sides of it.  The
    descriptors stay the original points'."""
    inp = _inputs(40, 70, 1, "hard")
    X = inp["pts3d"].copy()
    K, W = inp["K"], inp["im_width"]
    for k, j in enumerate(FAR):
        X[j, 0] = ((-8.0 - k) - K[0, 2]) * X[j, 2] / K[0, 0]
    du = (_pixels(inp["R0"], inp["t0"], X, K) - _pixels(np.eye(3), np.zeros(3), X, K))[:, 0]
    for k, j in enumerate(EDGE):
        border = -0.5 if k % 2 == 0 else W - 0.5
        X[j, 0] = (border - EDGE_FRAC * du[j] - K[0, 2]) * X[j, 2] / K[0, 0]
    return dict(inp, pts3d=X)


@pytest.mark.parametrize("loss", ["geman_mcclure", "cauchy"])
def test_unsupported_points(loss, monkeypatch):
    monkeypatch.delenv("FMPNP_SPEC_CAP", raising=False)
    inp = _unsupported_inputs()
    ores, otr = _oracle(inp, "f32", loss)
    ns = otr["n_supported"]
    # the condition, from the oracle alone (the moved points were chosen with it on the CPU)
    assert ores["status"] == "ok" and len(ns) == ITERS + 1
    assert ns.max() < 70 and ns.min() > 0, ns
    assert np.count_nonzero(np.diff(ns)) >= 2, ns
    res, tr, _, _ = _both_ways([_problem(inp, "f32")], _lib.F32, loss, -1, f"unsupported {loss}")
    _check_oracle(res[0], ores, f"unsupported {loss}")
    np.testing.assert_array_equal(tr[0]["n_supported"], ns)
    np.testing.assert_array_equal(tr[0]["n_kept"], otr["n_kept"])
    # ... in a batch beside an untouched query, and alone with the helpers
    two, tr2, _, _ = _both_ways([_problem(_inputs(40, 70, 2, "easy"), "f32"), _problem(inp, "f32")], _lib.F32, loss,
                                -1, f"unsupported {loss} B=2")
    _same_records(_quiet(two[1]), _quiet(res[0]), f"unsupported {loss}: in a batch vs alone")
    one, tr1, info, _ = _both_ways([_problem(inp, "f32")], _lib.F32, loss, 0, f"unsupported {loss} helpers")
    assert info["helpers"] > 0, info
    _same_records(_quiet(one[0]), _quiet(res[0]), f"unsupported {loss}: with helpers vs without")
    _same_traces(tr1[0], tr[0], f"unsupported {loss}: with helpers vs without")


# ---------------------------------------------------------------------------
# Non-finite texels (the same shape): a NaN and a +Inf texel on points' paths.  The trimmed and the plain
# variant agree field by field, NaN for NaN, and end with the same status.
# ---------------------------------------------------------------------------
def _texel(inp, R, t, j):
    p = rf.project_pixels(np.asarray(R), np.asarray(t), inp["pts3d"][j:j + 1], inp["K"])[0]
    return (int(p[1]) * HF) // inp["im_height"], (int(p[0]) * WF) // inp["im_width"]


@pytest.mark.parametrize("loss", ["geman_mcclure", "cauchy"])
def test_nonfinite_texels(loss, monkeypatch):
    monkeypatch.delenv("FMPNP_SPEC_CAP", raising=False)
    base = _inputs(40, 70, 1, "hard")
    fmap = base["fmap"].clone()
    # +Inf where point 5 starts, NaN where point 68 (the partial block) ends up at the identity pose
    ri, ci = _texel(base, base["R0"], base["t0"], 5)
    rn, cn = _texel(base, np.eye(3), np.zeros(3), 68)
    assert (ri, ci) != (rn, cn)
    fmap[:, ri, ci] = float("inf")
    fmap[:, rn, cn] = float("nan")
    inp = dict(base, fmap=fmap)
    # (records and traces compared inside, NaN for NaN)
    res, tr, _, plain = _both_ways([_problem(inp, "f32")], _lib.F32, loss, -1, f"non-finite {loss}")
    assert res[0]["status"] & ~QUIET == plain[0]["status"] & ~QUIET
    # the start's +Inf texel was read: Geman-McClure saturates it (rho -> 4), Cauchy's cost is not finite
    assert tr[0]["n_supported"][0] == 70
    one, tr1, info, _ = _both_ways([_problem(inp, "f32")], _lib.F32, loss, 0, f"non-finite {loss} helpers")
    assert info["helpers"] > 0, info
    _same_records(_quiet(one[0]), _quiet(res[0]), f"non-finite {loss}: with helpers vs without")
    _same_traces(tr1[0], tr[0], f"non-finite {loss}: with helpers vs without")


# ---------------------------------------------------------------------------
# Predictions withdrawn (FMPNP_SPEC_CAP = 0: every prediction is formed and none is gathered): the equality
# cannot rest on them.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["geman_mcclure", "cauchy"])
def test_no_predictions_gathered(loss, monkeypatch):
    inp = _inputs(256, 70, 1, "hard")
    monkeypatch.delenv("FMPNP_SPEC_CAP", raising=False)
    ref, rtr, _, _ = _both_ways([_problem(inp, "f32")], _lib.F32, loss, -1, f"default cap {loss}")
    monkeypatch.setenv("FMPNP_SPEC_CAP", "0")
    res, tr, _, _ = _both_ways([_problem(inp, "f32")], _lib.F32, loss, -1, f"FMPNP_SPEC_CAP=0 {loss}")
    _same_records(_quiet(res[0]), _quiet(ref[0]), f"{loss}: no predictions gathered vs the default")
    _same_traces(tr[0], rtr[0], f"{loss}: no predictions gathered vs the default")
    _check_oracle(res[0], _oracle_of(256, 70, 1, "hard", "f32", loss)[0], f"FMPNP_SPEC_CAP=0 {loss}")
