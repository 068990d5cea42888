"""The refiner's packed query map through the dense hypercolumn (assemble, then pack: the existing path) against
fmpnp.pack_hypercolumn / feature_pnp(query_layers=...) (straight from the layers), on identical inputs, interleaved
in one process (GPU machine only).

    python tools/hypercolumn_pack_bench.py [--out profiles/hypercolumn_pack_bench.json] [--rounds 7]
                                           [--seconds 0.3] [--legs pack,window,consumer]
    python tools/hypercolumn_pack_bench.py --kernel-only fgrad     # the fused kernels alone, for a counter run

Legs (the yardstick is always the existing path, never the new code against itself):
  pack      the full pack at the "robotcar" layers (128@256^2, 256@128^2, 256@64^2, 512@64^2, 512@32^2: C = 1664
            at 256 x 256), layouts "fgrad" and "f": assemble_hypercolumn + pack_features against pack_hypercolumn.
  window    pack_hypercolumn of the texels within 6 texels of N = 295 / 866 points' texels (the marks the one-call
            refiner's window makes) against the same composed FULL pack: the windowed Sobel pack of a dense map is
            no entry point of its own, it runs inside fmpnp_feature_pnp (the consumer legs time it there).
  consumer  feature_pnp with a three-level pyramid and the reference given as layers, at the robotcar shape
            (N = 295 and 866) and at a cfg2-like pair of layers (C = 256 at 240 x 320, N = 512): the dense query
            handed in (the assembly excluded), the same plus the assembly that produces it, and query_layers=.

Timing: a host clock around blocks of calls, each ending in a device wait.  Every round times a leg's variants
one after the other; `rounds` rounds give each variant's median and its max - min.  The outputs of the two paths
are compared for equality before anything is timed.  A "win" or "loss" is called only when the medians differ by
more than the two spreads added.  Peak device memory of one call of each variant (torch's allocator, above what
the inputs hold) is recorded beside the times.
"""
import argparse
import importlib
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
from fmpnp import _lib, synth  # noqa: E402

LAYERS = {
    "robotcar": [(128, 256, 256), (256, 128, 128), (256, 64, 64), (512, 64, 64), (512, 32, 32)],
    "cfg2": [(128, 240, 320), (128, 120, 160)],
}
PYRAMIDS = {
    "robotcar": [(640, 1664, None, None), (128, 640, None, None), (0, 128, None, None)],
    "cfg2": [(128, 256, None, None), (64, 128, None, None), (0, 64, None, None)],
}
Pred = namedtuple("Prediction", "points_3d reference_inliers matrix quaternion reference_filename")


def make_layers(name, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return [torch.randn(1, c, h, w, generator=g, device=dev) for c, h, w in LAYERS[name]]


def layers_of(fmap, name):
    """Layers whose hypercolumn resembles fmap [C, H, W]: its channels, split as LAYERS[name] and pooled down."""
    out, at = [], 0
    for c, h, w in LAYERS[name]:
        x = fmap[None, at:at + c]
        k = fmap.shape[1] // h
        out.append((torch.nn.functional.avg_pool2d(x, k) if k > 1 else x).contiguous())
        at += c
    return out


def block_ms(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t) * 1e3 / n


def stats(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), rounds=len(v))


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def measure(variants, a):
    """Interleaved rounds over the variants (name -> callable ending in a device wait)."""
    per = {}
    for k, fn in variants.items():
        for _ in range(3):
            fn()
        per[k] = max(2, int(a.seconds / max(block_ms(fn, 2) * 1e-3, 1e-5)))
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            times[k].append(block_ms(fn, per[k]))
    return {k: dict(stats(v), calls_per_block=per[k], peak_mb=peak_mb(variants[k])) for k, v in times.items()}


def verdict(entry, old, new):
    d = entry[new]["median_ms"] - entry[old]["median_ms"]
    noise = entry[old]["spread_ms"] + entry[new]["spread_ms"]
    entry[f"{new}_minus_{old}_ms"] = d
    entry[f"{new}_vs_{old}"] = "win" if d < -noise else ("loss" if d > noise else "within the spreads")


def waited(fn):
    def run():
        out = fn()
        torch.cuda.synchronize()
        return out
    return run


def window_marks(n_points, H, W, radius, dev):
    """The marks the one-call refiner's window makes: the squares of `radius` texels around the points' texels
    at the initial pose (fmpnp_pack.hip win_mark_kernel's rule), as a uint8 [H, W] device tensor."""
    X, K, img_w, img_h = synth.scene(n_points, H, W, 23)
    R0, t0 = synth.INITS["easy"]
    p = fmpnp.refine.project_pixels(R0, t0, X, K)
    ok = (p[:, 0] >= 0) & (p[:, 0] < img_w) & (p[:, 1] >= 0) & (p[:, 1] < img_h)
    rows = (p[ok, 1].astype(np.int64) * H) // img_h
    cols = (p[ok, 0].astype(np.int64) * W) // img_w
    marks = np.zeros((H, W), np.uint8)
    for r, c in zip(rows, cols):
        marks[max(r - radius, 0):r + radius + 1, max(c - radius, 0):c + radius + 1] = 1
    return torch.from_numpy(marks).to(dev)


def pack_leg(layout, dev, a, n_points=0, radius=6):
    layers = make_layers("robotcar", dev)
    H, W = (int(s) for s in layers[0].shape[2:])
    C = sum(int(m.shape[1]) for m in layers)
    composed = lambda: fmpnp.pack_features(fmpnp.assemble_hypercolumn(layers)[0], layout=layout)  # noqa: E731
    entry = dict(leg="window" if n_points else "pack", shape="robotcar", layout=layout, C=C, H=H, W=W)
    if n_points:
        marks = window_marks(n_points, H, W, radius, dev)
        # (into a buffer kept between calls, as the refiner does: a fresh one would be zeroed whole)
        keep = torch.zeros((H, W, 3, C) if layout == "fgrad" else (H, W, C), device=dev)
        fused = lambda: fmpnp.pack_hypercolumn(layers, layout=layout, marks=marks, out=keep)  # noqa: E731
        sel = marks.bool()
        equal = bool(torch.equal(composed().buf[sel], fused().buf[sel]))
        entry.update(N=n_points, radius=radius, marked_fraction=float(sel.float().mean()))
    else:
        fused = lambda: fmpnp.pack_hypercolumn(layers, layout=layout)  # noqa: E731
        equal = bool(torch.equal(composed().buf, fused().buf))
    planes = 3 if layout == "fgrad" else 1
    entry.update(outputs_equal=equal, layers_mb=sum(m.numel() for m in layers) * 4 / 2 ** 20,
                 dense_mb=C * H * W * 4 / 2 ** 20, packed_mb=planes * C * H * W * 4 / 2 ** 20,
                 **measure({"assemble_pack": waited(composed), "fused": waited(fused)}, a))
    verdict(entry, "assemble_pack", "fused")
    return entry


def consumer_leg(name, n_points, dev, a):
    C = sum(c for c, _, _ in LAYERS[name])
    _, H, W = LAYERS[name][0]
    (batch,), img = synth.pipeline_queries(1, 1, n_points, C, H, W, device=dev, seed0=23)
    q, _, p, K = batch[0]
    layers = layers_of(q, name)
    pred = Pred(p.points_3d, p.reference_inliers, p.matrix, np.array([1.0, 0, 0, 0]), "ref.png")
    dense = fmpnp.assemble_hypercolumn(layers)
    mk = lambda: fmpnp.sparseFeaturePnP(50, loss_fn=fmpnp.geman_mcclure_loss, lambda_=0.01)  # noqa: E731
    kw = dict(feature_pyramid=PYRAMIDS[name], reference_layers=layers)
    variants = {
        "map_given": lambda: fmpnp.feature_pnp(dense, None, pred, K, img, model=mk(), **kw),
        "assemble_then_call": lambda: fmpnp.feature_pnp(fmpnp.assemble_hypercolumn(layers), None, pred, K, img,
                                                        model=mk(), **kw),
        "query_layers": lambda: fmpnp.feature_pnp(None, None, pred, K, img, model=mk(), query_layers=layers, **kw),
    }
    reruns = _lib.load().fmpnp_feature_pnp_reruns()
    x, y = variants["map_given"](), variants["query_layers"]()
    equal = bool(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2].best_cost_, y[2].best_cost_))
    entry = dict(leg="consumer", shape=name, C=C, H=H, W=W, N=n_points, results_equal=equal,
                 window=importlib.import_module("fmpnp.optimize_feature_pnp").window_radius(C, H, W, n_points),
                 **measure(variants, a))
    entry["window_reruns"] = int(_lib.load().fmpnp_feature_pnp_reruns() - reruns)
    verdict(entry, "assemble_then_call", "query_layers")
    verdict(entry, "map_given", "query_layers")
    return entry


def kernel_only(layout, dev):
    """The fused kernels alone at the robotcar shape (for a counter run of its own): three launches."""
    layers = make_layers("robotcar", dev)
    torch.cuda.synchronize()
    for _ in range(3):
        fmpnp.pack_hypercolumn(layers, layout=layout)
    torch.cuda.synchronize()
    print(json.dumps(dict(kernel_only=layout, layers_mb=sum(m.numel() for m in layers) * 4 / 2 ** 20)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.3, help="timed work per variant and round, about")
    ap.add_argument("--legs", default="pack,window,consumer")
    ap.add_argument("--kernel-only", default=None, metavar="LAYOUT")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.require_device(dev)
    if a.kernel_only:
        kernel_only(a.kernel_only, dev)
        return
    result = dict(device=torch.cuda.get_device_name(0), library_digest=_lib.library_digest(),
                  date=time.strftime("%Y-%m-%d"), rounds=a.rounds, legs=[])
    jobs = []
    legs = a.legs.split(",")
    if "pack" in legs:
        jobs += [lambda: pack_leg("fgrad", dev, a), lambda: pack_leg("f", dev, a)]
    if "window" in legs:
        jobs += [lambda: pack_leg("fgrad", dev, a, 295), lambda: pack_leg("fgrad", dev, a, 866)]
    if "consumer" in legs:
        jobs += [lambda: consumer_leg("robotcar", 295, dev, a), lambda: consumer_leg("robotcar", 866, dev, a),
                 lambda: consumer_leg("cfg2", 512, dev, a)]
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
