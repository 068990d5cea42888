"""What binary16 storage of the packed map and descriptors (FMPNP_F16, include/fmpnp.h) costs in pose accuracy:
the oracle on the rounded inputs against the oracle on the unrounded ones (CPU only, no device).

    python tools/f16_storage_accuracy.py [--out profiles/f16_storage_accuracy.json]

This is a property of the number format, not of the kernels (they compute what the oracle computes on the rounded
values: tests/test_gpu_f16_storage.py), so no test pins it.  Inputs: the fp32 golden cases, cfg2-shaped synthetic
queries (N = 512, C = 256, 240 x 320; 4 seeds, easy and hard starts, 50 iterations of Geman-McClure) and a
C = 1664 three-level pyramid (N = 295, 64 x 64 texels).  Per group: the largest rotation and translation deviation
of the final pose, the largest relative deviation of the best cost, and how many runs' accept / reject sequences
differ.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "featuremetric-pnp_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import oracle.oracle as orc  # noqa: E402
from fmpnp import synth  # noqa: E402
from golden_io import FORWARD_CASES, case  # noqa: E402

PYRAMID = [(640, 1664, None, None), (128, 640, None, None), (0, 128, None, None)]


def round16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a).astype(np.float32).astype(np.float16).astype(np.float64)


def rot_angle(Ra, Rb):
    c = (np.trace(np.asarray(Ra).T @ np.asarray(Rb)) - 1.0) / 2.0
    return math.acos(max(-1.0, min(1.0, c)))


def accepts(costs):
    acc, prev = [], costs[0] if len(costs) else 0.0
    for c in costs[1:]:
        a = not (c > prev)
        acc.append(a)
        if a:
            prev = c
    return acc


def both(fmap32, fref, run):
    """run(f, gx, gy, fref) -> (R, t, best_cost, [costs]) on the unrounded and on the rounded inputs."""
    f = np.asarray(fmap32).astype(np.float64)
    gx, gy = orc.sobel(f)
    fr = np.asarray(fref, dtype=np.float64)
    a = run(f, gx, gy, fr)
    b = run(round16(f), round16(gx), round16(gy), round16(fr))
    same = len(a[3]) == len(b[3]) and accepts(list(a[3])) == accepts(list(b[3]))
    dc = abs(b[2] - a[2]) / abs(a[2]) if a[2] == a[2] and b[2] == b[2] and a[2] != 0 else 0.0
    return dict(rotation_rad=rot_angle(a[0], b[0]), translation=float(np.linalg.norm(np.asarray(a[1]) - b[1])),
                best_cost_rel=dc, same_accepts=bool(same), n_evals=(len(a[3]), len(b[3])))


def forward_run(inp, n_iters, lambda0, loss, ratio, alpha=0.0):
    def run(f, gx, gy, fr):
        p = orc.make_problem(inp["pts3d"], fr, f, gx, gy, inp["K"], inp["im_width"], inp["im_height"], inp["R0"],
                             inp["t0"])
        res, tr = orc.forward(p, orc.make_options(n_iters, lambda0, loss, ratio, alpha), trace_cap=n_iters + 1)
        return res["R"], res["t"], res["best_cost"], tr["cost"]
    return run


def summarise(rows):
    return dict(runs=len(rows), max_rotation_rad=max(r["rotation_rad"] for r in rows),
                max_translation=max(r["translation"] for r in rows),
                max_best_cost_rel=max(r["best_cost_rel"] for r in rows),
                accept_sequences_differ=sum(not r["same_accepts"] for r in rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    groups = {}
    rows = []
    for name in FORWARD_CASES:
        inp, meta, _ = case(name)
        if "fmap32" not in inp:
            continue
        run = forward_run(inp, meta["n_iters"], meta["lambda0"], meta["loss"], meta.get("ratio_threshold"),
                          meta.get("barron_alpha") or 0.0)
        rows.append(dict(case=name, **both(inp["fmap32"], inp["fref"], run)))
    groups["golden_fp32_cases"] = dict(summarise(rows), cases=rows)
    rows = []
    for seed in range(4):
        for init in ("easy", "hard"):
            inp = synth.problem_inputs(512, 256, 240, 320, seed=seed, device="cpu", init=init)
            run = forward_run(inp, 50, 0.01, "geman_mcclure", None)
            rows.append(dict(case=f"cfg2 seed {seed} {init}", **both(inp["fmap"].numpy(), inp["fref"].numpy(), run)))
    groups["cfg2_synthetic"] = dict(summarise(rows), cases=rows)
    rows = []
    for init in ("easy", "hard"):
        inp = synth.problem_inputs(295, 1664, 64, 64, seed=23, device="cpu", init=init)

        def run(f, gx, gy, fr, inp=inp):
            R, t, attrs, traces = orc.multilevel(PYRAMID, inp["pts3d"], fr, f, gx, gy, inp["K"], inp["im_width"],
                                                 inp["im_height"], inp["R0"], inp["t0"], 50, loss="geman_mcclure",
                                                 trace_cap=51)
            return R, t, attrs["best_cost"], np.concatenate([tr["cost"] for _, tr in traces])
        rows.append(dict(case=f"C=1664 pyramid {init}", **both(inp["fmap"].numpy(), inp["fref"].numpy(), run)))
    groups["c1664_pyramid"] = dict(summarise(rows), cases=rows)
    for k, g in groups.items():
        print(k, json.dumps({x: g[x] for x in g if x != "cases"}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(groups, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
