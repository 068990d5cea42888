"""The per-wave release of the speculating LM variants (fmpnp_lm_impl.h release_wait_burst /
tail_release; up to commit bc62f2e also the lane-0 release_wait of a build with -DFMPNP_TAIL_BURST=0).

With one workgroup per problem, speculation and no ratio test (VAR_GM_SPEC, VAR_GM_SPEC_512,
VAR_NEAREST_SPEC and their _H forms) the evaluation loop has no closing barrier: the three tail
waves count up a release word after their last LDS access and every wave enters the next
evaluation once the word has arrived.  What the barrier ordered -- the next pose and state complete
before they are read, the block partials read before they are overwritten, the state of one problem
not carried into the next -- is pinned here on small problems: every case runs the same problems with
speculate=False, which takes a plain variant that keeps the barrier, and asserts the result records
equal field by field (bench.py's DUMP_FIELDS, np.array_equal), and checks poses and costs against
the oracle with tests/test_gpu_headline.py's helpers and tolerances (fp32 texels: pose within
1e-4 rad / 1e-4 m, costs 1e-6 relative, support counts and the schedule identical).

Shapes: C = 16 channels on a 24 x 32 synthetic map (96 x 128 image), fp32 texels, packed f / gx / gy,
50 iterations unless stated; the early exits use the reference's goldens (128 points at C = 16, 24 at C = 4)
with their own loss, damping and iteration count.
No case may end with FMPNP_STATUS_SYNC_TIMEOUT, and none provokes it.
"""
import numpy as np
import pytest
import torch

import nonfinite_checks as nf
import oracle.oracle as orc
from golden_io import case, maps64, poisoned_maps

pytestmark = pytest.mark.gpu

from bench import DUMP_FIELDS  # noqa: E402
from fmpnp import _lib, refine as rf, synth  # noqa: E402  (no skip: a missing HIP library must fail)
from test_gpu_headline import check, host_copy, oracle_run  # noqa: E402  (the headline's helpers and tolerances)

DEV = "cuda:0"
ITERS, C, HF, WF = 50, 16, 24, 32
LOSS = {"geman_mcclure": _lib.GEMAN_MCCLURE, "cauchy": _lib.CAUCHY, "squared": _lib.SQUARED}
QUIET = _lib.STATUS_HELPER_WAIT  # informational and timing dependent: not part of a result

_CACHE = {}


def _query(n_pts, seed, init):
    """(packed problem, oracle inputs) of one synthetic query, shared among the cases.  Generated on
    the CPU: the same on every machine, so the conditions on the inputs hold wherever the test runs."""
    key = (n_pts, seed, init)
    if key not in _CACHE:
        inp = synth.problem_inputs(n_pts, C, HF, WF, seed=seed, device="cpu", init=init)
        feats = rf.pack_features(inp["fmap"], storage=torch.float32, device=DEV)
        prob = rf.make_problem(feats, inp["fref"], inp["pts3d"], inp["K"], inp["im_width"], inp["im_height"],
                               inp["R0"], inp["t0"])
        _CACHE[key] = (prob, host_copy(inp))
    return _CACHE[key]


_ORACLE = {}


def _oracle(n_pts, seed, init, n_iters=ITERS, loss="geman_mcclure"):
    key = (n_pts, seed, init, n_iters, loss)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_run(_query(n_pts, seed, init)[1], n_iters=n_iters, loss=loss)
    return _ORACLE[key]


def _options(n_iters=ITERS, loss="geman_mcclure", lambda0=0.01, **kw):
    return rf.make_options(n_iters, lambda0, LOSS[loss], dtype=_lib.F32, **kw)


def _same_records(a, b, what):
    for k in DUMP_FIELDS:
        assert np.array_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64),
                              equal_nan=True), (what, k, a[k], b[k])


def _released_and_barrier(probs, what, variants, n_iters=ITERS, loss="geman_mcclure", **kw):
    """The problems through a speculating variant (the per-wave release) and through the plain one
    (speculate=False: the closing barrier): the plans asserted, the records equal field by field, no
    timeout.  Returns the released run's (results, traces)."""
    res, trs = rf.refine(probs, _options(n_iters, loss, **kw), trace=True)
    info = _lib.last_launch()
    assert info["variant_name"] in variants and "_SPEC" in info["variant_name"], (what, info)
    assert info["wgs_per_problem"] == 1 and not info["team"] and not info["ratio"], (what, info)
    base, _ = rf.refine(probs, _options(n_iters, loss, speculate=False, **kw), trace=True)
    plain = _lib.last_launch()
    assert "SPEC" not in plain["variant_name"], (what, plain)
    for q, (r, b) in enumerate(zip(res, base)):
        assert r["status"] & _lib.STATUS_SYNC_TIMEOUT == 0 and b["status"] & _lib.STATUS_SYNC_TIMEOUT == 0, (what, q)
        assert r["status"] & ~QUIET == b["status"] & ~QUIET, (what, q, r["status"], b["status"])
        _same_records(dict(r, status=r["status"] & ~QUIET), dict(b, status=b["status"] & ~QUIET), f"{what} query {q}")
    return res, trs


# N = 512; 480 (the last block partial, the 512 carve); 449 (the carve's smallest); 448 and 130 (GM_SPEC:
# waves without a block, 130: two points in the last block); 64 (one block: waves 1 and 2 run their
# tail roles with no block); 1
POINTS = [(512, "GM_SPEC_512"), (480, "GM_SPEC_512"), (449, "GM_SPEC_512"), (448, "GM_SPEC"), (130, "GM_SPEC"),
          (64, "GM_SPEC"), (1, "GM_SPEC")]


@pytest.mark.parametrize("n_pts,variant", POINTS, ids=[f"N{n}" for n, _ in POINTS])
def test_point_counts(n_pts, variant):
    """Every block count a workgroup can hold, without the first-evaluation helpers (the plain _SPEC
    forms), two problems per launch: an easy and a hard start."""
    qs = [(n_pts, 100 + n_pts, "easy"), (n_pts, 200 + n_pts, "hard")]
    res, trs = _released_and_barrier([_query(*q)[0] for q in qs], f"N={n_pts}", (variant,), helpers=-1)
    assert _lib.last_launch()["helpers"] == 0
    for q, r, tr in zip(qs, res, trs):
        check(dict(r, status=r["status"] & ~QUIET), tr, *_oracle(*q), f"N={n_pts} {q[2]}")


def test_nearest_spec_cauchy():
    """VAR_NEAREST_SPEC (any loss but Geman-McClure) and its _H form."""
    qs = [(130, 330, "easy"), (130, 331, "hard")]
    probs = [_query(*q)[0] for q in qs]
    for helpers, variant in ((-1, "NEAREST_SPEC"), (0, "NEAREST_SPEC_H")):
        res, trs = _released_and_barrier(probs, f"cauchy helpers={helpers}", (variant,), loss="cauchy", helpers=helpers)
        for q, r, tr in zip(qs, res, trs):
            check(dict(r, status=r["status"] & ~QUIET), tr, *_oracle(*q, loss="cauchy"), f"cauchy {q}")


@pytest.mark.parametrize("B", [1, 3, 8])
def test_batch_sizes(B):
    """B = 1, 3 and 8 problems of 512 points with the first-evaluation helpers (the _H forms)."""
    qs = [(512, 400 + q, "hard" if q % 2 else "easy") for q in range(B)]
    res, trs = _released_and_barrier([_query(*q)[0] for q in qs], f"B={B}", ("GM_SPEC_H_512",))
    assert _lib.last_launch()["helpers"] > 0
    for q, r, tr in zip(qs, res, trs):
        check(dict(r, status=r["status"] & ~QUIET), tr, *_oracle(*q), f"B={B} query {q[1]}")


def test_five_launches_on_one_async_batch():
    """The same B = 3 batch launched five times on one AsyncBatch (one workspace, one result buffer):
    every launch returns the traced synchronous launch's records -- the release word, the abort words
    and the helpers' tags carry nothing from launch to launch."""
    qs = [(512, 400 + q, "hard" if q % 2 else "easy") for q in range(3)]
    probs = [_query(*q)[0] for q in qs]
    ref, _ = _released_and_barrier(probs, "async B=3", ("GM_SPEC_H_512",))
    ab = rf.AsyncBatch(probs, _options())
    for launch in range(5):
        ab.launch()
        got = ab.results()
        assert "_SPEC" in _lib.last_launch()["variant_name"]
        for q in range(3):
            assert got[q]["status"] & _lib.STATUS_SYNC_TIMEOUT == 0
            _same_records(dict(got[q], status=got[q]["status"] & ~QUIET), dict(ref[q], status=ref[q]["status"] & ~QUIET),
                          f"launch {launch} query {q}")


def test_one_workgroup_walks_several_problems():
    """max_teams = 1: one workgroup takes five problems of different sizes in turn, so the release
    word is reset between problems (problem_begin); each equals its own single launch."""
    qs = [(512, 400, "easy"), (130, 331, "hard"), (512, 401, "hard"), (1, 101, "easy"), (449, 649, "hard")]
    probs = [_query(*q)[0] for q in qs]
    res, trs = _released_and_barrier(probs, "walk", ("GM_SPEC", "GM_SPEC_512"), max_teams=1, helpers=-1)
    assert _lib.last_launch()["teams"] == 1
    for q, p, r, tr in zip(qs, probs, res, trs):
        (one,), _ = rf.refine([p], _options(helpers=-1), trace=True)
        _same_records(r, one, f"walk {q}")
        check(r, tr, *_oracle(*q), f"walk {q}")


@pytest.mark.parametrize("init,seed", [("hard", 331), ("easy", 401)])
def test_accept_sequences(init, seed):
    """The hard start of this query rejects steps, so the reject stepper publishes the next pose; the
    easy one takes every step (conditions on the inputs, asserted on the oracle's trace)."""
    n_pts = 130 if init == "hard" else 512
    ores, otr = _oracle(n_pts, seed, init)
    rejects = nf.accepts(list(otr["cost"])).count(False)
    assert rejects >= 3 if init == "hard" else rejects == 0, rejects
    for helpers in (-1, 0):
        (res,), (tr,) = _released_and_barrier([_query(n_pts, seed, init)[0]], f"{init} helpers={helpers}",
                                              ("GM_SPEC", "GM_SPEC_H", "GM_SPEC_512", "GM_SPEC_H_512"), helpers=helpers)
        check(dict(res, status=res["status"] & ~QUIET), tr, ores, otr, f"{init} helpers={helpers}")
        assert list(tr["accepted"][1:]) == nf.accepts(list(otr["cost"]))


@pytest.mark.parametrize("n_iters", [1, 2])
def test_few_iterations(n_iters):
    """n_iters = 1 and 2: the loop leaves through the books wave's `done` after two / three
    evaluations (the last one's tail takes no step)."""
    qs = [(512, 400, "easy"), (130, 331, "hard")]
    for q in qs:
        (res,), (tr,) = _released_and_barrier([_query(*q)[0]], f"n_iters={n_iters} {q}",
                                              ("GM_SPEC_H", "GM_SPEC_H_512"), n_iters=n_iters)
        assert res["n_evals"] == n_iters + 1 and res["n_steps"] == n_iters
        check(dict(res, status=res["status"] & ~QUIET), tr, *_oracle(*q, n_iters=n_iters), f"n_iters={n_iters} {q}")


def test_compute_cost_mode():
    """compute_cost stops after the first evaluation.  The planner speculates in forward runs only, so
    this mode takes the plain variant with the closing barrier (asserted): the cost against the oracle,
    and the first evaluation of a squared-loss forward run (compute_cost's loss, model.py:216-243) --
    through the released variant -- gives the same cost."""
    n_pts, seed, init = 512, 400, "easy"
    prob, host = _query(n_pts, seed, init)
    (res,), _ = rf.refine([prob], _options(mode=_lib.MODE_COMPUTE_COST, wgs_per_problem=1))
    info = _lib.last_launch()
    assert "SPEC" not in info["variant_name"], info
    assert res["status"] == 0 and res["n_evals"] == 1 and res["n_steps"] == 0
    want = orc.compute_cost(host["pts3d"], host["fref"], host["fmap"], host["K"], host["im_width"], host["im_height"],
                            host["R0"], host["t0"], None)
    assert res["initial_cost"] == pytest.approx(want, rel=1e-6)
    (fwd,), _ = _released_and_barrier([prob], "forward of compute_cost", ("NEAREST_SPEC_H",), loss="squared")
    assert fwd["initial_cost"] == pytest.approx(want, rel=1e-6)


def _golden_problem(name, poisoned=False, **kw):
    inp, meta, gold = case(name)
    f, gx, gy = poisoned_maps(inp, meta, orc.sobel) if poisoned else maps64(inp, orc.sobel)
    feats = rf.pack_features(torch.from_numpy(f), torch.from_numpy(gx), torch.from_numpy(gy), storage=torch.float32,
                             device=DEV)
    prob = rf.make_problem(feats, torch.from_numpy(inp["fref"]), inp["pts3d"], inp["K"], inp["im_width"],
                           inp["im_height"], kw.get("R0", inp["R0"]), kw.get("t0", inp["t0"]))
    return prob, inp, meta, gold, (f, gx, gy)


def _golden_oracle(inp, meta, maps, t0=None):
    p = orc.make_problem(inp["pts3d"], inp["fref"], *maps, inp["K"], inp["im_width"], inp["im_height"], inp["R0"],
                         inp["t0"] if t0 is None else t0)
    return orc.forward(p, orc.make_options(meta["n_iters"], meta["lambda0"], meta["loss"]), meta["n_iters"] + 1)


def _golden_run(prob, meta, what):
    """The golden's problem alone, with its own options (loss, lambda0, iterations)."""
    assert meta.get("ratio_threshold") is None
    variants = ("GM_SPEC", "GM_SPEC_H") if meta["loss"] == "geman_mcclure" else ("NEAREST_SPEC", "NEAREST_SPEC_H")
    (res,), (tr,) = _released_and_barrier([prob], what, variants, n_iters=meta["n_iters"], loss=meta["loss"],
                                          lambda0=meta["lambda0"])
    return res, tr


def test_no_support_at_the_start():
    """Every point projects outside the image at the initial pose (the reference's no_support_init
    golden): FMPNP_STATUS_NO_SUPPORT, the initial pose returned, no evaluation counted."""
    prob, inp, meta, gold, maps = _golden_problem("no_support_init")
    res, tr = _golden_run(prob, meta, "no_support_init")
    assert res["status"] & ~QUIET == _lib.STATUS_NO_SUPPORT and not res["has_best"] and res["n_evals"] == 0
    np.testing.assert_array_equal(res["R"], np.asarray(inp["R0"]).reshape(3, 3))
    np.testing.assert_array_equal(res["t"], np.asarray(inp["t0"]).reshape(3))


def test_no_support_after_a_step():
    """The no_support_trial golden: a step carries every point out of the image
    (FMPNP_STATUS_NO_SUPPORT_TRIAL) and the current pose is returned, as the oracle does."""
    prob, inp, meta, gold, maps = _golden_problem("no_support_trial")
    ores, otr = _golden_oracle(inp, meta, maps)
    assert ores["status"] == "no_support_trial" and ores["n_evals"] >= 1
    res, tr = _golden_run(prob, meta, "no_support_trial")
    assert res["status"] & ~QUIET == _lib.STATUS_NO_SUPPORT_TRIAL
    assert res["n_evals"] == ores["n_evals"] and res["n_steps"] == ores["n_steps"]
    assert nf.rot_angle(res["R"], ores["R"]) < 1e-4 and np.linalg.norm(res["t"] - ores["t"]) < 1e-4
    np.testing.assert_allclose(res["R"], gold["out_R"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(res["t"], gold["out_t"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(tr["cost"], otr["cost"][:len(tr["cost"])], rtol=1e-6)


def test_nan_step():
    """The NaN-step exit of the nan_texel_gm golden (model.py:411-413): status, pose and counters as
    tests/test_gpu_nonfinite.py expects them with fp32 texels; the stepping wave's `nan` word is part
    of what the release publishes."""
    name = "nan_texel_gm"
    prob, inp, meta, gold, maps = _golden_problem(name, poisoned=True)
    res, tr = _golden_run(prob, meta, name)
    nf.check_forward(name, gold, nf.from_fmpnp(res, tr, _lib.STATUS_NAN, ignore=QUIET), fp32=True)
    assert list(tr["accepted"][1:]) == nf.accepts(list(gold["track_costs"]))
