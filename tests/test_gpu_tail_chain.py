"""The shortened tail chain of the speculating LM variants (fmpnp_lm_impl.h: release_wait_burst,
tail_preload / tail_operands, the 16-byte pose store).

In the variants with the per-wave release (VAR_GM_SPEC, VAR_GM_SPEC_512, VAR_NEAREST_SPEC and their
_H forms) a wave now reads the release word, the next pose and done / nan in one burst of LDS reads,
the next pose is stored with 16-byte writes, and in the Geman-McClure ones the accept stepper takes
its 27 operands from the combine's registers and the steppers read the schedule's state ahead of
the combine.  Every step
moves data differently and none may change a bit of a result, so every case here runs the same
problems three ways and asserts the result records equal field by field (bench.py's DUMP_FIELDS,
np.array_equal):
  * the default launch (released waves, the new tail chain),
  * FMPNP_SPEC_W0=0 (the same variant with the loop's closing barrier kept),
  * speculate=False (a plain variant: the parent's tail, untouched by the change),
and checks the released run against the oracle at tests/test_gpu_parity.py's tolerances for fp32
texels (pose within 1e-4 rad / 1e-4 m; n_evals, n_steps, n_accepted, status identical; final_lambda
and final_lr, products of the same powers of ten in both, to 1e-12 relative).

Shapes: C = 64 channels, fp32 texels, a 24 x 32 map (96 x 128 image), packed f / gx / gy; N = 64 (one
block), 130 (a partial last block, VAR_GM_SPEC), 480 and 512 (the 512-point carve); B = 1 and 3; the
easy start (every step accepted: the accept stepper stores the pose) and the hard start (steps
rejected: the reject stepper stores it and the accept stepper returns early), both asserted on the
oracle's trace.  No case may end with FMPNP_STATUS_SYNC_TIMEOUT, and none provokes it.
"""
import numpy as np
import pytest
import torch

import nonfinite_checks as nf
import oracle.oracle as orc

pytestmark = pytest.mark.gpu

from bench import DUMP_FIELDS  # noqa: E402
from fmpnp import _lib, refine as rf, synth  # noqa: E402  (no skip: a missing HIP library must fail)
from test_gpu_headline import host_copy, oracle_run  # noqa: E402

DEV = "cuda:0"
ITERS, C, HF, WF = 50, 64, 24, 32
LOSS = {"geman_mcclure": _lib.GEMAN_MCCLURE, "cauchy": _lib.CAUCHY}
QUIET = _lib.STATUS_HELPER_WAIT  # informational and timing dependent: not part of a result

_QUERY, _ORACLE = {}, {}


def _query(n_pts, seed, init):
    """(packed problem, oracle inputs) of one synthetic query, generated on the CPU and shared."""
    key = (n_pts, seed, init)
    if key not in _QUERY:
        inp = synth.problem_inputs(n_pts, C, HF, WF, seed=seed, device="cpu", init=init)
        feats = rf.pack_features(inp["fmap"], storage=torch.float32, device=DEV)
        prob = rf.make_problem(feats, inp["fref"], inp["pts3d"], inp["K"], inp["im_width"], inp["im_height"],
                               inp["R0"], inp["t0"])
        _QUERY[key] = (prob, host_copy(inp))
    return _QUERY[key]


def _oracle(n_pts, seed, init, n_iters=ITERS, loss="geman_mcclure"):
    key = (n_pts, seed, init, n_iters, loss)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_run(_query(n_pts, seed, init)[1], n_iters=n_iters, loss=loss)
    return _ORACLE[key]


def _options(n_iters=ITERS, loss="geman_mcclure", **kw):
    return rf.make_options(n_iters, 0.01, LOSS[loss], dtype=_lib.F32, **kw)


def _quiet(r):
    return dict(r, status=r["status"] & ~QUIET)


def _same_records(a, b, what):
    for k in DUMP_FIELDS:
        assert np.array_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64),
                              equal_nan=True), (what, k, a[k], b[k])


def _three_ways(probs, what, variants, monkeypatch, n_iters=ITERS, loss="geman_mcclure", trace=True, **kw):
    """The problems through the released variant, the same variant with the closing barrier
    (FMPNP_SPEC_W0=0) and the plain one (speculate=False): plans asserted, records equal field by
    field, no timeout.  Returns the released run's (results, traces)."""
    monkeypatch.delenv("FMPNP_SPEC_W0", raising=False)
    res, trs = rf.refine(probs, _options(n_iters, loss, **kw), trace=trace)
    info = _lib.last_launch()
    assert info["variant_name"] in variants and "_SPEC" in info["variant_name"], (what, info)
    assert info["wgs_per_problem"] == 1 and not info["team"] and not info["ratio"], (what, info)
    monkeypatch.setenv("FMPNP_SPEC_W0", "0")
    barrier, _ = rf.refine(probs, _options(n_iters, loss, **kw), trace=trace)
    assert _lib.last_launch()["variant_name"] == info["variant_name"], what
    monkeypatch.delenv("FMPNP_SPEC_W0")
    plain, _ = rf.refine(probs, _options(n_iters, loss, speculate=False, **kw), trace=trace)
    assert "SPEC" not in _lib.last_launch()["variant_name"], (what, _lib.last_launch())
    for q, (r, b, p) in enumerate(zip(res, barrier, plain)):
        for x in (r, b, p):
            assert x["status"] & _lib.STATUS_SYNC_TIMEOUT == 0, (what, q)
        _same_records(_quiet(r), _quiet(b), f"{what} query {q}: released vs closing barrier")
        _same_records(_quiet(r), _quiet(p), f"{what} query {q}: released vs plain variant")
    return res, trs


def _check_oracle(res, tr, ores, otr, what):
    """tests/test_gpu_parity.py's fp32 tolerances on the pose; the schedule identical."""
    assert ores["status"] == "ok" and res["status"] & ~QUIET == 0, what
    assert nf.rot_angle(res["R"], ores["R"]) < 1e-4, what
    assert np.linalg.norm(res["t"] - ores["t"]) < 1e-4, what
    for k in ("n_evals", "n_steps", "n_accepted"):
        assert res[k] == ores[k], (what, k, res[k], ores[k])
    assert res["final_lambda"] == pytest.approx(ores["final_lambda"], rel=1e-12), what
    assert res["final_lr"] == pytest.approx(ores["final_lr"], rel=1e-12), what
    if tr is not None:
        assert list(tr["accepted"][1:]) == nf.accepts(list(otr["cost"])), what


def _rejects(n_pts, seed, init, **kw):
    return nf.accepts(list(_oracle(n_pts, seed, init, **kw)[1]["cost"])).count(False)


# (points, the variants the planner may pick: the plain _SPEC form and its _H form)
POINTS = [(64, ("GM_SPEC", "GM_SPEC_H")), (130, ("GM_SPEC", "GM_SPEC_H")),
          (480, ("GM_SPEC_512", "GM_SPEC_H_512")), (512, ("GM_SPEC_512", "GM_SPEC_H_512"))]
# synth seeds per point count, chosen on the oracle: two hard starts that reject steps (on this small map
# most hard starts of 480 or 512 points are accepted throughout) and an easy start that rejects none
SEEDS_HARD = {64: (1, 4), 130: (2, 4), 480: (15, 19), 512: (98, 66)}
SEED_EASY = {64: 3, 130: 1, 480: 1, 512: 1}


def _starts(n_pts, B):
    """B queries of n_pts points: hard, easy, hard."""
    return [(n_pts, SEEDS_HARD[n_pts][q // 2], "hard") if q % 2 == 0 else (n_pts, SEED_EASY[n_pts], "easy")
            for q in range(B)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n_pts,variants", POINTS, ids=[f"N{n}" for n, _ in POINTS])
def test_point_counts_and_batches(n_pts, variants, B, monkeypatch):
    """Every shape and batch, without (B = 1) and with (B = 3) the first-evaluation helpers; B = 1
    runs the hard and then the easy start.  The hard start rejects steps and the easy one none
    (conditions on the inputs, asserted on the oracle's trace)."""
    assert all(_rejects(n_pts, s, "hard") >= 1 for s in SEEDS_HARD[n_pts])
    assert _rejects(n_pts, SEED_EASY[n_pts], "easy") == 0
    batches = [_starts(n_pts, 3)] if B == 3 else [_starts(n_pts, 2)[:1], _starts(n_pts, 2)[1:]]
    for qs in batches:
        res, trs = _three_ways([_query(*q)[0] for q in qs], f"N={n_pts} B={B}", variants, monkeypatch,
                               helpers=-1 if B == 1 else 0)
        for q, r, tr in zip(qs, res, trs):
            _check_oracle(r, tr, *_oracle(*q), f"N={n_pts} B={B} {q}")


def test_nearest_spec_cauchy(monkeypatch):
    """VAR_NEAREST_SPEC (a loss other than Geman-McClure) and its _H form."""
    qs = _starts(130, 3)
    assert [_rejects(*q, loss="cauchy") > 0 for q in qs] == [True, False, True]
    probs = [_query(*q)[0] for q in qs]
    for helpers, variant in ((-1, "NEAREST_SPEC"), (0, "NEAREST_SPEC_H")):
        res, trs = _three_ways(probs, f"cauchy helpers={helpers}", (variant,), monkeypatch, loss="cauchy",
                               helpers=helpers)
        for q, r, tr in zip(qs, res, trs):
            _check_oracle(r, tr, *_oracle(*q, loss="cauchy"), f"cauchy {q}")


@pytest.mark.parametrize("n_iters", [0, 1])
def test_few_iterations(n_iters, monkeypatch):
    """n_iters = 0: `done` is set before the first burst, which must leave the loop with no evaluation;
    n_iters = 1: two evaluations, the second one's tail takes no step.  (50: every other case.)"""
    for q in (_starts(512, 1)[0], _starts(130, 1)[0]):
        (res,), _ = _three_ways([_query(*q)[0]], f"n_iters={n_iters} {q}", ("GM_SPEC_H", "GM_SPEC_H_512"), monkeypatch,
                                n_iters=n_iters)
        if n_iters == 0:
            host = _query(*q)[1]
            assert res["n_evals"] == 0 and res["n_steps"] == 0 and res["status"] & ~QUIET == 0
            np.testing.assert_array_equal(res["R"], np.asarray(host["R0"]).reshape(3, 3))
            np.testing.assert_array_equal(res["t"], np.asarray(host["t0"]).reshape(3))
        else:
            assert res["n_evals"] == 2 and res["n_steps"] == 1
            _check_oracle(res, None, *_oracle(*q, n_iters=1), f"n_iters=1 {q}")


def test_without_trace(monkeypatch):
    """The same launches with and without the trace give the same records."""
    qs = _starts(480, 3)
    probs = [_query(*q)[0] for q in qs]
    traced, trs = _three_ways(probs, "trace on", ("GM_SPEC_H_512",), monkeypatch, trace=True)
    assert all(tr is not None and len(tr["cost"]) == r["n_evals"] for r, tr in zip(traced, trs))
    plain, _ = _three_ways(probs, "trace off", ("GM_SPEC_H_512",), monkeypatch, trace=False)
    for q, (a, b) in enumerate(zip(traced, plain)):
        _same_records(_quiet(a), _quiet(b), f"trace on / off query {q}")


def test_compute_cost_mode():
    """compute_cost takes the plain variant (asserted, as tests/test_gpu_wave_release.py does): the
    changed code is not in it, and the cost is the oracle's."""
    q = _starts(512, 1)[0]
    prob, host = _query(*q)
    (res,), _ = rf.refine([prob], _options(mode=_lib.MODE_COMPUTE_COST, wgs_per_problem=1))
    info = _lib.last_launch()
    assert "SPEC" not in info["variant_name"], info
    assert res["status"] == 0 and res["n_evals"] == 1 and res["n_steps"] == 0
    want = orc.compute_cost(host["pts3d"], host["fref"], host["fmap"], host["K"], host["im_width"], host["im_height"],
                            host["R0"], host["t0"], None)
    assert res["initial_cost"] == pytest.approx(want, rel=1e-6)


def test_hundred_launches_on_one_async_batch(monkeypatch):
    """One AsyncBatch (one workspace, one result buffer) launched 100 times: every launch returns the
    records of the traced synchronous launch -- a burst that took a stale pose or state, even once,
    would show here."""
    qs = _starts(512, 3)
    probs = [_query(*q)[0] for q in qs]
    ref, _ = _three_ways(probs, "async B=3", ("GM_SPEC_H_512",), monkeypatch)
    ab = rf.AsyncBatch(probs, _options())
    for launch in range(100):
        ab.launch()
        got = ab.results()
        for q in range(3):
            assert got[q]["status"] & _lib.STATUS_SYNC_TIMEOUT == 0
            _same_records(_quiet(got[q]), _quiet(ref[q]), f"launch {launch} query {q}")
    assert "_SPEC" in _lib.last_launch()["variant_name"]
