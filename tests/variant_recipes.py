"""The launch recipes of tests/test_variant_coverage.py -- one per LM kernel specialisation the
planner (featuremetric-pnp_amd/csrc/fmpnp_api.hip make_plan) can choose -- and the keys that
identify a specialisation, shared with tests/test_gpu_nonfinite.py.  No device is touched here."""
from fmpnp import _lib

ITERS = 50
N_PTS, C, HF, WF = 128, 16, 48, 64        # small problems: two 64-point blocks, 4x image
N_512 = 480                               # the _512 recipes: 449..512 points (eight blocks, the last partial)
M512 = ("gm_spec_512", "gm_spec_h_512")
LOSSES = {"gm": (_lib.GEMAN_MCCLURE, "geman_mcclure"), "cauchy": (_lib.CAUCHY, "cauchy")}

# recipe name -> (B, loss, mode, sampling, layout, memo, speculate, wgs_per_problem, variant,
#                 build, team).  Each recipe runs with ratio off / 0.8 and fp32 / fp64 texels
#                 (layout "f" is fp32 only).
RECIPES = {
    # latency build, one workgroup per problem
    "gm_spec":          (128, "gm", "fwd", "nearest", "fgrad", True, True, 0, "GM_SPEC", "latency", 0),
    "gm_spec_h":        (1, "gm", "fwd", "nearest", "fgrad", True, True, 0, "GM_SPEC_H", "latency", 0),
    # ... at 512 points per problem (the compile-time carve, fp32 only; N_512 points)
    "gm_spec_512":      (128, "gm", "fwd", "nearest", "fgrad", True, True, 0, "GM_SPEC_512", "latency", 0),
    "gm_spec_h_512":    (1, "gm", "fwd", "nearest", "fgrad", True, True, 0, "GM_SPEC_H_512", "latency", 0),
    "nearest_spec":     (128, "cauchy", "fwd", "nearest", "fgrad", True, True, 0, "NEAREST_SPEC", "latency", 0),
    "nearest_spec_h":   (1, "cauchy", "fwd", "nearest", "fgrad", True, True, 0, "NEAREST_SPEC_H", "latency", 0),
    "gm":               (128, "gm", "fwd", "nearest", "fgrad", True, False, 0, "GM", "latency", 0),
    "gm_h":             (1, "gm", "fwd", "nearest", "fgrad", True, False, 0, "GM_H", "latency", 0),
    "nearest":          (128, "cauchy", "fwd", "nearest", "fgrad", True, False, 0, "NEAREST", "latency", 0),
    "nearest_h":        (1, "cauchy", "fwd", "nearest", "fgrad", True, False, 0, "NEAREST_H", "latency", 0),
    # (compute_cost is one all-points evaluation: the planner keeps the team spread at B=1)
    "compute_cost":     (1, "gm", "cost", "nearest", "fgrad", True, True, 0, "NEAREST", "latency", 1),
    "bil_direct":       (1, "gm", "fwd", "bilinear", "fgrad", False, False, 1, "BIL_DIRECT", "latency", 0),
    "f_gm":             (1, "gm", "fwd", "nearest", "f", True, True, 1, "F_GM", "latency", 0),
    "f_nearest":        (1, "cauchy", "fwd", "nearest", "f", True, True, 1, "F_NEAREST", "latency", 0),
    # latency build, teams of workgroups
    "gm_team":          (1, "gm", "fwd", "nearest", "fgrad", True, True, 2, "GM", "latency", 1),
    "nearest_team":     (1, "cauchy", "fwd", "nearest", "fgrad", True, True, 2, "NEAREST", "latency", 1),
    "bil_direct_team":  (1, "gm", "fwd", "bilinear", "fgrad", False, False, 0, "BIL_DIRECT", "latency", 1),
    "f_gm_team":        (1, "gm", "fwd", "nearest", "f", True, True, 0, "F_GM", "latency", 1),
    "f_nearest_team":   (1, "cauchy", "fwd", "nearest", "f", True, True, 0, "F_NEAREST", "latency", 1),
    # throughput build (>= 2 problems per CU)
    "tp_gm":            (512, "gm", "fwd", "nearest", "fgrad", True, True, 0, "GM", "throughput", 0),
    "tp_nearest":       (512, "cauchy", "fwd", "nearest", "fgrad", True, True, 0, "NEAREST", "throughput", 0),
    "tp_bil_direct":    (512, "gm", "fwd", "bilinear", "fgrad", False, False, 0, "BIL_DIRECT", "throughput", 0),
    # wide build: the bilinear cell memo
    "bil_memo":         (128, "gm", "fwd", "bilinear", "fgrad", True, True, 0, "BILINEAR", "wide", 0),
    "bil_memo_team":    (1, "gm", "fwd", "bilinear", "fgrad", True, True, 0, "BILINEAR", "wide", 1),
}


def _cases():
    out = []
    for name, r in RECIPES.items():
        for dt in ("f32", "f64"):
            if (r[4] == "f" or name in M512) and dt == "f64":
                continue
            for ratio in (None, 0.8):
                out.append((name, dt, ratio))
    return out


CASES = _cases()


def case_key(name, dt, ratio):
    r = RECIPES[name]
    return (dt, r[9], r[10], int(ratio is not None), r[8])


def info_key(info):
    return (info["dtype_name"], info["build_name"], int(info["team"]), int(info["ratio"]), info["variant_name"])
