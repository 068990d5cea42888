"""The trimmed texel gather trip of the speculating LM variants (fmpnp_lm_impl.h: reduce6_in32, rec_field6;
DESIGN 4.1.9).

In VAR_GM_SPEC, VAR_GM_SPEC_512, VAR_NEAREST_SPEC and their _H forms (and in the first-evaluation helpers that
serve them) a gathered point's six channel sums are reduced over the half-wave without the two zero slots, and
other lanes hold and store the record fields.  That may not change a bit of a result, so every case runs the same
problems through a trimmed _SPEC variant and through speculate=False (a plain variant: reduce8_in32, untouched
by the change), asserts the result records equal field by field (bench.py's DUMP_FIELDS, np.array_equal), asserts
that no run ends with FMPNP_STATUS_SYNC_TIMEOUT, and checks the trimmed run against the oracle at
tests/test_gpu_parity.py's tolerances for fp32 texels (pose within 1e-4 rad / 1e-4 m; n_evals, n_steps, n_accepted
and status identical; final_lambda and final_lr to 1e-12 relative).  For binary16 storage the oracle reads the
values as the pack rounds them (tests/f16_storage_cases.py).

The scalar-base loads with 32-bit offsets that were measured with this change were not adopted, so
the planner has no 4 GiB rule and there is no test of one.

Shapes: a 12 x 16 map (48 x 64 image), 50 iterations, Geman-McClure and Cauchy (the GM and NEAREST variants); a
batch of three (hard, easy, hard start) without helpers and one query with the first-evaluation helpers, whose
records must be the batch's for the same query.  N = 70 is a full block plus a partial one of 6 points (odd
dirty counts, a lone half-wave point), N = 512 the 512-point carve.  The channel forms, V = channels per 16-byte
vector (4 fp32, 2 fp64, 8 binary16):
  C = 64 V            both rounds in every lane (FULL)
  C = 48 V            a second round in half the lanes
  C = 40, C[0:128]    no second round
  C = 128 V, C[640:1664]   the four-round form with every round present, one / two chunks, the second with a
                      non-zero c_begin
  C = 80 V, C = 520 binary16   the four-round form with missing rounds
  C = 37              the scalar, non-vector form (whichever variant the planner routes it to)
The planner speculates above 64 V channels only with FMPNP_SPEC_MAXC (a measurement knob, read per plan), which
those cases set.
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

# id -> (storage, C, c_begin, c_end, N, FMPNP_SPEC_MAXC or None, the planner must speculate)
SHAPES = {
    "f32-C256-full": ("f32", 256, 0, None, 70, None, True),
    "f32-C256-N512": ("f32", 256, 0, None, 512, None, True),
    "f32-C192-half-second-round": ("f32", 192, 0, None, 70, None, True),
    "f32-C40-one-round": ("f32", 40, 0, None, 70, None, True),
    "f32-C512-four-rounds": ("f32", 512, 0, None, 70, 1024, True),
    "f32-C320-four-rounds-ragged": ("f32", 320, 0, None, 70, 1024, True),
    "f32-C1664-slice-640-1664": ("f32", 1664, 640, 1664, 70, 1024, True),
    "f32-C1664-slice-0-128": ("f32", 1664, 0, 128, 70, None, True),
    "f32-C37-scalar": ("f32", 37, 0, None, 70, None, None),
    "f64-C128-full": ("f64", 128, 0, None, 70, None, True),
    "f64-C96-half-second-round": ("f64", 96, 0, None, 70, None, True),
    "f64-C256-four-rounds": ("f64", 256, 0, None, 70, 1024, True),
    "f16-C512-full": ("f16", 512, 0, None, 70, None, True),
    "f16-C40-one-round": ("f16", 40, 0, None, 70, None, True),
    "f16-C520-four-rounds-ragged": ("f16", 520, 0, None, 70, 2048, True),
}

_INPUTS = {}


def _inputs(C, n_pts, seed, init):
    key = (C, n_pts, seed, init)
    if key not in _INPUTS:
        _INPUTS[key] = synth.problem_inputs(n_pts, C, HF, WF, seed=seed, device="cpu", init=init)
    return _INPUTS[key]


def _oracle(inp, storage, loss, cb, ce):
    """The oracle on the values the kernel reads: the fp32 map with the fp64 Sobel, or (binary16) every plane
    and the descriptors as the pack rounds them."""
    f = inp["fmap"].double().cpu().numpy()
    fref = inp["fref"].double().cpu().numpy()
    if storage == "f16":
        f, gx, gy, fref = rounded_maps(inp["fmap"].cpu().numpy(), fref)
    else:
        gx, gy = orc.sobel(f)
    p = orc.make_problem(inp["pts3d"], fref, f, gx, gy, inp["K"], inp["im_width"], inp["im_height"], inp["R0"],
                         inp["t0"], cb, f.shape[0] if ce is None else ce)
    return orc.forward(p, orc.make_options(ITERS, 0.01, loss), trace_cap=ITERS + 1)


def _problem(inp, storage, cb, ce):
    feats = rf.pack_features(inp["fmap"], storage=STORAGE[storage][0], device=DEV)
    return rf.make_problem(feats, inp["fref"], inp["pts3d"], inp["K"], inp["im_width"], inp["im_height"], inp["R0"],
                           inp["t0"], cb, ce)


def _quiet(r):
    return dict(r, status=r["status"] & ~QUIET)


def _same_records(a, b, what):
    for k in DUMP_FIELDS:
        assert np.array_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64),
                              equal_nan=True), (what, k, a[k], b[k])


def _both_ways(probs, dtype, loss, helpers, spec, what):
    """The problems through the planner's choice (a trimmed _SPEC variant where `spec`) and through
    speculate=False (a plain variant): records equal field by field, no timeout.  Returns the first
    run's results and its launch plan."""
    res, _ = rf.refine(probs, rf.make_options(ITERS, 0.01, LOSS[loss], dtype=dtype, helpers=helpers), trace=True)
    info = _lib.last_launch()
    if spec is not None:
        assert ("_SPEC" in info["variant_name"]) == spec, (what, info)
    assert info["wgs_per_problem"] == 1 and not info["team"], (what, info)
    plain, _ = rf.refine(probs, rf.make_options(ITERS, 0.01, LOSS[loss], dtype=dtype, helpers=helpers,
                                                speculate=False), trace=True)
    assert "SPEC" not in _lib.last_launch()["variant_name"], (what, _lib.last_launch())
    for q, (r, p) in enumerate(zip(res, plain)):
        assert r["status"] & _lib.STATUS_SYNC_TIMEOUT == 0 and p["status"] & _lib.STATUS_SYNC_TIMEOUT == 0, (what, q)
        _same_records(_quiet(r), _quiet(p), f"{what} query {q}: trimmed vs plain variant")
    return res, info


def _check_oracle(res, ores, what):
    """tests/test_gpu_parity.py's fp32 tolerances on the pose; the schedule identical."""
    assert ores["status"] == "ok" and res["status"] & ~QUIET == 0, (what, ores["status"], res["status"])
    assert nf.rot_angle(res["R"], ores["R"]) < 1e-4, what
    assert np.linalg.norm(res["t"] - ores["t"]) < 1e-4, what
    for k in ("n_evals", "n_steps", "n_accepted"):
        assert res[k] == ores[k], (what, k, res[k], ores[k])
    assert res["final_lambda"] == pytest.approx(ores["final_lambda"], rel=1e-12), what
    assert res["final_lr"] == pytest.approx(ores["final_lr"], rel=1e-12), what


@pytest.mark.parametrize("loss", ["geman_mcclure", "cauchy"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_trimmed_equals_plain_and_oracle(shape, loss, monkeypatch):
    storage, C, cb, ce, n_pts, maxc, spec = SHAPES[shape]
    if maxc is None:
        monkeypatch.delenv("FMPNP_SPEC_MAXC", raising=False)
    else:
        monkeypatch.setenv("FMPNP_SPEC_MAXC", str(maxc))
    dtype = STORAGE[storage][1]
    inps = [_inputs(C, n_pts, seed, init) for seed, init in STARTS]
    probs = [_problem(inp, storage, cb, ce) for inp in inps]
    # B = 3, no helpers
    res, info = _both_ways(probs, dtype, loss, -1, spec, f"{shape} {loss} B=3")
    assert info["helpers"] == 0, info
    for q, (r, inp) in enumerate(zip(res, inps)):
        _check_oracle(r, _oracle(inp, storage, loss, cb, ce)[0], f"{shape} {loss} B=3 query {q}")
    # B = 1 with the first-evaluation helpers: the helpers' sums are the main workgroup's
    one, info = _both_ways(probs[:1], dtype, loss, 0, spec, f"{shape} {loss} B=1 helpers")
    assert info["helpers"] > 0 and "_H" in info["variant_name"], info
    _same_records(_quiet(one[0]), _quiet(res[0]), f"{shape} {loss}: with helpers vs without")
