"""fp32 against opt-in binary16 storage of the refiner's packed map and descriptors (FMPNP_F16, include/fmpnp.h),
alternated in one process on identical inputs (GPU machine only).

    python tools/f16_storage_bench.py [--out profiles/f16_storage_ab.json] [--runs 5] [--seconds 0.3]
                                      [--legs lm,consumer,pack]
    python tools/f16_storage_bench.py --kernel-only f16|f32      # pack + gather + LM once each, for a counter run

Legs (the baseline is always the fp32 leg of the same run):
  lm        the LM launch alone (fmpnp_refine_batch_async over resident descriptors) at cfg2 (N = 512, C = 256,
            240 x 320, Geman-McClure, 50 iterations), B = 128 distinct queries and B = 1.
  consumer  fmpnp_feature_pnp through fmpnp.feature_pnp(storage=...), one query per call, at cfg2 and at the
            RobotCar shape (C = 1664 at 256 x 256, three levels, N = 295 and 866); wall clock, host included.
  pack      the full fgrad pack (fmpnp_pack_features) at both shapes, and the windowed pack at the RobotCar shape
            (radius 6, N = 295 / 866; cfg2's call takes no window).  The windowed Sobel pack has no entry point of
            its own, so it is timed as the consumer's call with n_iters = 0: the pack with the call's fixed costs.

Timing: a host clock around blocks of calls that end in a device wait; fp32 and binary16 alternate, `runs` runs
each, and min / median / max are reported.  A "win" or "loss" is called only when the medians differ by more than
the two spreads added.  Bytes per query: the buffers' sizes (packed map, fref), fp32 against binary16; counters, if
wanted, come from a run of their own (--kernel-only under a counter-only profiler).
"""
import argparse
import json
import os
import statistics
import sys
import time
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "featuremetric-pnp_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fmpnp  # noqa: E402
from fmpnp import _lib, refine as rf, synth  # noqa: E402
from fmpnp.optimize_feature_pnp import window_radius  # noqa: E402

STORAGES = {"f32": torch.float32, "f16": torch.float16}
CODES = {"f32": _lib.F32, "f16": _lib.F16}
SHAPES = {  # name: (N, C, Hf, Wf, feature_pyramid)
    "cfg2": (512, 256, 240, 320, None),
    "robotcar_n295": (295, 1664, 256, 256, [(640, 1664, None, None), (128, 640, None, None), (0, 128, None, None)]),
    "robotcar_n866": (866, 1664, 256, 256, [(640, 1664, None, None), (128, 640, None, None), (0, 128, None, None)]),
}
Pred = namedtuple("Prediction", "points_3d reference_inliers matrix quaternion reference_filename")


def block_ms(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / n


def stats(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), runs=len(v))


def alternate(variants, a):
    """fp32 and binary16 one after the other, a.runs times (name -> callable; the block ends in a device wait)."""
    per = {}
    for k, fn in variants.items():
        for _ in range(3):
            fn()
        per[k] = max(2, int(a.seconds / max(block_ms(fn, 2) * 1e-3, 1e-5)))
    times = {k: [] for k in variants}
    for _ in range(a.runs):
        for k, fn in variants.items():
            times[k].append(block_ms(fn, per[k]))
    out = {k: dict(stats(v), calls_per_block=per[k]) for k, v in times.items()}
    d = out["f16"]["median_ms"] - out["f32"]["median_ms"]
    noise = out["f16"]["spread_ms"] + out["f32"]["spread_ms"]
    out["f16_minus_f32_ms"] = d
    out["f16_over_f32"] = out["f16"]["median_ms"] / out["f32"]["median_ms"]
    out["f16_vs_f32"] = "win" if d < -noise else ("loss" if d > noise else "within the spreads")
    return out


def lm_leg(B, dev, a):
    N, C, H, W, _ = SHAPES["cfg2"]
    opts = {k: rf.make_options(50, 0.01, _lib.GEMAN_MCCLURE, dtype=CODES[k]) for k in STORAGES}
    probs = {k: [] for k in STORAGES}
    for q in range(B):
        inp = synth.problem_inputs(N, C, H, W, seed=q, device=dev)
        for k, st in STORAGES.items():
            feats = rf.pack_features(inp["fmap"], storage=st, device=dev)
            probs[k].append(rf.make_problem(feats, inp["fref"], inp["pts3d"], inp["K"], inp["im_width"],
                                            inp["im_height"], inp["R0"], inp["t0"]))
    batches = {k: rf.AsyncBatch(probs[k], opts[k]) for k in STORAGES}
    entry = dict(leg="lm", shape="cfg2", B=B, N=N, C=C, H=H, W=W)
    for k, b in batches.items():
        b.launch()
        res = b.results()
        entry[f"{k}_launch"] = _lib.last_launch()
        entry[f"{k}_statuses"] = sorted({r["status"] for r in res})
        entry[f"{k}_mean_evals"] = float(np.mean([r["n_evals"] for r in res]))
        entry[f"{k}_texel_gathers"] = int(sum(r["texel_gathers"] for r in res))
        entry[f"{k}_packed_mb_per_query"] = probs[k][0].feats.buf.numel() * probs[k][0].feats.buf.element_size() / 2 ** 20
    entry.update(alternate({k: batches[k].launch for k in STORAGES}, a))
    return entry


def _consumer_query(name, dev, seed=23):
    N, C, H, W, pyr = SHAPES[name]
    (batch,), img = synth.pipeline_queries(1, 1, N, C, H, W, device=dev, seed0=seed)
    q, r, p, K = batch[0]
    return (q[None], r, Pred(p.points_3d, p.reference_inliers, p.matrix, np.array([1.0, 0, 0, 0]), "ref.png"), K,
            img), pyr


def consumer_leg(name, dev, a):
    N, C, H, W, _ = SHAPES[name]
    args, pyr = _consumer_query(name, dev)

    def call(st):
        m = fmpnp.sparseFeaturePnP(50, loss_fn=fmpnp.geman_mcclure_loss, lambda_=0.01)
        return fmpnp.feature_pnp(*args, feature_pyramid=pyr, model=m, storage=st)
    reruns = _lib.load().fmpnp_feature_pnp_reruns()
    out = {k: call(st) for k, st in STORAGES.items()}
    dR = out["f16"][0].numpy().T @ out["f32"][0].numpy()
    entry = dict(leg="consumer", shape=name, N=N, C=C, H=H, W=W, window=window_radius(C, H, W, N),
                 f16_vs_f32_rotation_rad=float(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))),
                 f16_vs_f32_translation=float(np.linalg.norm(out["f16"][1].numpy() - out["f32"][1].numpy())),
                 best_cost={k: float(v[2].best_cost_) for k, v in out.items()},
                 **alternate({k: (lambda st=st: call(st)) for k, st in STORAGES.items()}, a))
    entry["window_reruns"] = int(_lib.load().fmpnp_feature_pnp_reruns() - reruns)
    return entry


def pack_leg(name, dev, a):
    """The full fgrad pack into a buffer kept between calls, and the buffers' bytes per query (packed map, fref;
    with a window, the marked share of the map is what the windowed pack writes)."""
    N, C, H, W, _ = SHAPES[name]
    fmap = synth.feature_map(C, H, W, 23, dev)
    outs = {k: torch.zeros((H, W, 3, rf._cstride(C, st)), dtype=st, device=dev) for k, st in STORAGES.items()}
    packs = {k: (lambda k=k, st=st: rf.pack_features(fmap, storage=st, device=dev, out=outs[k]))
             for k, st in STORAGES.items()}
    equal = bool(torch.equal(packs["f16"]().buf[..., :C], packs["f32"]().buf[..., :C].half()))
    entry = dict(leg="pack", shape=name, C=C, H=H, W=W, f16_is_f32_narrowed=equal,
                 input_mb=C * H * W * 4 / 2 ** 20,
                 packed_mb={k: o.numel() * o.element_size() / 2 ** 20 for k, o in outs.items()},
                 fref_mb={k: N * rf._cstride(C, st) * outs[k].element_size() / 2 ** 20 for k, st in STORAGES.items()},
                 **alternate(packs, a))
    for k in STORAGES:  # HBM traffic the pack needs (input once, output once) over its median time
        entry[k]["needed_gb_per_s"] = (entry["input_mb"] + entry["packed_mb"][k]) / 1024 / (entry[k]["median_ms"] * 1e-3)
    return entry


def window_pack_leg(name, dev, a):
    """The windowed pack as fmpnp_feature_pnp runs it: the call with a model of zero iterations (upload, marks,
    windowed pack, gather, compute_cost, three empty LM launches, download) -- the pack dominates its device work."""
    N, C, H, W, pyr = SHAPES[name]
    args, _ = _consumer_query(name, dev)
    radius = window_radius(C, H, W, N)

    def call(st):
        m = fmpnp.sparseFeaturePnP(0, loss_fn=fmpnp.geman_mcclure_loss, lambda_=0.01)
        return fmpnp.feature_pnp(*args, feature_pyramid=pyr, model=m, storage=st, window=radius)
    return dict(leg="window_pack_call", shape=name, N=N, C=C, H=H, W=W, window=radius,
                note="feature_pnp with n_iters = 0: the windowed pack with the call's fixed costs",
                **alternate({k: (lambda st=st: call(st)) for k, st in STORAGES.items()}, a))


def kernel_only(kind, dev):
    """pack, gather and the LM launch once each at cfg2 (for a counter run of its own)."""
    N, C, H, W, _ = SHAPES["cfg2"]
    inp = synth.problem_inputs(N, C, H, W, seed=0, device=dev)
    st = STORAGES[kind]
    torch.cuda.synchronize()
    feats = rf.pack_features(inp["fmap"], storage=st, device=dev)
    prob = rf.make_problem(feats, inp["fref"], inp["pts3d"], inp["K"], inp["im_width"], inp["im_height"], inp["R0"],
                           inp["t0"])
    (res,), _ = rf.refine([prob], rf.make_options(50, 0.01, _lib.GEMAN_MCCLURE, dtype=CODES[kind]))
    print(json.dumps(dict(kernel_only=kind, best_cost=res["best_cost"], texel_gathers=res["texel_gathers"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.3, help="timed work per variant and run, about")
    ap.add_argument("--legs", default="lm,consumer,pack")
    ap.add_argument("--kernel-only", default=None, metavar="STORAGE")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.require_device(dev)
    if a.kernel_only:
        kernel_only(a.kernel_only, dev)
        return
    result = dict(device=torch.cuda.get_device_name(0), library_digest=_lib.library_digest(),
                  date=time.strftime("%Y-%m-%d"), runs=a.runs, legs=[])
    legs = a.legs.split(",")
    jobs = []
    if "lm" in legs:
        jobs += [lambda: lm_leg(1, dev, a), lambda: lm_leg(128, dev, a)]
    if "consumer" in legs:
        jobs += [lambda n=n: consumer_leg(n, dev, a) for n in SHAPES]
    if "pack" in legs:
        jobs += [lambda: pack_leg("cfg2", dev, a), lambda: pack_leg("robotcar_n295", dev, a)]
        jobs += [lambda n=n: window_pack_leg(n, dev, a) for n in ("robotcar_n295", "robotcar_n866")]
    for job in jobs:
        entry = job()
        result["legs"].append(entry)
        print(json.dumps(entry), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
