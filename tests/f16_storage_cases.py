"""Case tables and the yardstick of the binary16-storage tests (FMPNP_F16, include/fmpnp.h), shared by
tests/test_f16_storage_cpu.py and tests/test_gpu_f16_storage.py.  No device is touched here.

The yardstick is the oracle on the rounded values: f, the fp64 Sobel's gx, gy (through fp32) and fref are
narrowed to binary16 with numpy and widened to fp64, and the oracle runs on them.  The kernel and the twin
widen the same binary16 values exactly, so both sides read identical numbers and the tolerance is the
project's identical-inputs tier (tests/test_variant_coverage.py, fp64 texels): equal n_evals, n_steps,
per-evaluation support counts and best_num_inliers; costs 1e-10 relative; poses 1e-9; per-point costs 1e-12
relative.
"""
import numpy as np

import oracle.oracle as orc

from variant_recipes import C, HF, ITERS, WF, N_PTS  # noqa: F401  (the recipes' small shape: N = 128, C = 16, 48 x 64)

LOSSES = {"gm": "geman_mcclure", "cauchy": "cauchy"}

# --- the LM specialisations the planner chooses for binary16 storage ------------------------------------------
# recipe name -> (B, loss, mode, memo, speculate, wgs_per_problem, variant, build, team); each with ratio off /
# 0.8.  The rows of tests/variant_recipes.py that binary16 supports (no _512 carve, no bilinear, no layout "f").
RECIPES = {
    "gm_spec":        (128, "gm", "fwd", True, True, 0, "GM_SPEC", "latency", 0),
    "gm_spec_h":      (1, "gm", "fwd", True, True, 0, "GM_SPEC_H", "latency", 0),
    "nearest_spec":   (128, "cauchy", "fwd", True, True, 0, "NEAREST_SPEC", "latency", 0),
    "nearest_spec_h": (1, "cauchy", "fwd", True, True, 0, "NEAREST_SPEC_H", "latency", 0),
    "gm":             (128, "gm", "fwd", True, False, 0, "GM", "latency", 0),
    "gm_h":           (1, "gm", "fwd", True, False, 0, "GM_H", "latency", 0),
    "nearest":        (128, "cauchy", "fwd", True, False, 0, "NEAREST", "latency", 0),
    "nearest_h":      (1, "cauchy", "fwd", True, False, 0, "NEAREST_H", "latency", 0),
    "compute_cost":   (1, "gm", "cost", True, True, 0, "NEAREST", "latency", 1),
    "gm_team":        (1, "gm", "fwd", True, True, 2, "GM", "latency", 1),
    "nearest_team":   (1, "cauchy", "fwd", True, True, 2, "NEAREST", "latency", 1),
    "tp_gm":          (512, "gm", "fwd", True, True, 0, "GM", "throughput", 0),
    "tp_nearest":     (512, "cauchy", "fwd", True, True, 0, "NEAREST", "throughput", 0),
}
CASES = [(name, ratio) for name in RECIPES for ratio in (None, 0.8)]


def case_key(name, ratio):
    r = RECIPES[name]
    return ("f16", r[7], r[8], int(ratio is not None), r[6])


# --- the gather's channel paths: maps of 12 x 16 texels, N = 70 (a full and a partial block) -------------------
PATH_HF, PATH_WF, PATH_N = 12, 16, 70
# C: 20 = the scalar form (ragged), 512 = one trip with both rounds full, 520 = the four-round chunk with
# missing rounds, 1032 = two chunks
PATH_CHANNELS = (20, 512, 520, 1032)

# --- the consumer's call: C = 40, 24 x 32, N = 70; levels with aligned and unaligned starts --------------------
CALL_C, CALL_HF, CALL_WF, CALL_N = 40, 24, 32, 70
CALL_LEVELS = [(24, 40), (4, 24), (0, 4)]

# --- the pack: (C, H, W) -----------------------------------------------------------------------------------------
PACK_SHAPES = [(20, 5, 7), (16, 48, 64)]


def round16(a):
    """fp64 values as binary16 storage holds them, widened back: through fp32, never one rounding from fp64."""
    with np.errstate(over="ignore"):
        return np.asarray(a).astype(np.float32).astype(np.float16).astype(np.float64)


def rounded_maps(fmap32, fref):
    """(f, gx, gy, fref) in fp64 as the binary16 pack and gather store them: the Sobel is the pack's fp64 Sobel of
    the UNROUNDED fp32 map, then every plane and fref are narrowed."""
    f = np.asarray(fmap32).astype(np.float64)
    gx, gy = orc.sobel(f)
    return round16(f), round16(gx), round16(gy), round16(fref)


def oracle_forward(inp, maps, loss, ratio, n_iters=ITERS, lambda0=0.01, c_begin=0, c_end=None, barron_alpha=0.0):
    f, gx, gy, fref = maps
    p = orc.make_problem(inp["pts3d"], fref, f, gx, gy, inp["K"], inp["im_width"], inp["im_height"], inp["R0"],
                         inp["t0"], c_begin, c_end)
    return orc.forward(p, orc.make_options(n_iters, lambda0, loss, ratio, barron_alpha), trace_cap=n_iters + 1)


def oracle_cost(inp, maps, ratio):
    f, _, _, fref = maps
    return orc.compute_cost(inp["pts3d"], fref, f, inp["K"], inp["im_width"], inp["im_height"], inp["R0"], inp["t0"],
                            ratio)


_ORC_STATUS = {"ok": 0, "no_support": 1, "nan": 2, "no_support_trial": 4}


def check_identical_inputs(res, tr, ores, otr, what, ignore_status=0):
    """The identical-inputs tier (see the module comment)."""
    if isinstance(ores["status"], str) and ores["status"] in _ORC_STATUS:
        assert res["status"] & ~ignore_status == _ORC_STATUS[ores["status"]], (what, res["status"], ores["status"])
    assert res["n_evals"] == ores["n_evals"] and res["n_steps"] == ores["n_steps"], \
        (what, res["n_evals"], ores["n_evals"], res["n_steps"], ores["n_steps"])
    if tr is not None:
        np.testing.assert_array_equal(tr["n_supported"], otr["n_supported"], err_msg=what)
        np.testing.assert_allclose(tr["cost"], otr["cost"], rtol=1e-10, atol=0, err_msg=what)
    np.testing.assert_allclose(res["R"], ores["R"], rtol=0, atol=1e-9, err_msg=what)
    np.testing.assert_allclose(res["t"], ores["t"], rtol=0, atol=1e-9, err_msg=what)
    assert bool(res["has_best"]) == bool(ores["has_best"]), what
    if ores["has_best"]:
        assert res["best_num_inliers"] == ores["best_num_inliers"], what
        np.testing.assert_allclose(res["best_cost"], ores["best_cost"], rtol=1e-10, atol=0, err_msg=what)
