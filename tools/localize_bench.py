"""One query against its top_N = 10 references, through the staged composition of the public stage functions
and through fmpnp.localize, on identical inputs, interleaved in one process (GPU machine only).

    python tools/localize_bench.py [--out profiles/localize_bench.json] [--rounds 7] [--seconds 0.4]

  staged      gather_sparse_descriptors per reference -> exhaustive_search_multi -> numpy masking
              (sparse_to_dense_predictor.py:161-175) -> solve_pnp_multi -> numpy best pick -> [feature_pnp]:
              what a user stitches by hand from INTEGRATION.md.  Host waits per query: the match's, the PnP's
              and the refiner's (3), plus one blocking upload of the points per reference in the gather and one
              of the PnP points.
  localize    fmpnp.localize(refine=False / True): one upload, one pinned download, one wait (2 with the refiner).

Shapes: "robotcar" (C = 1664, a 256 x 256 map, image 1024 x 1024, 1000 rows per reference, factor 0.006,
iters 5000) and "small" (C = 128, 64 x 64, image 256 x 256, 200 rows, factor 0.01, iters 1000).  Each reference:
60 % planted rows (the query's descriptor at the cell of the point's projection, plus noise), the rest random.
All references share one dense reference map (distinct cells per row), so the device holds two maps.

Timing: a host clock around blocks of calls (every call ends in a stream wait).  Each round times the four
variants one after the other; `rounds` rounds give each variant's median and its min..max spread.  The
expectation that is checked, not assumed: localize's median is not above staged's by more than staged's own
spread (max - min over the rounds).  The results of the two paths are compared for equality first.

    python tools/localize_bench.py --match-precision f16 [--out profiles/localize_bench_f16.json]

times fmpnp.localize with the opt-in fp16 match precision against the exact default instead (with and without
the refiner, the four variants interleaved in every round), and reports whether the two precisions pick the
same best reference with the same inlier count.

    python tools/localize_bench.py --refine batched [--batch 1,8,32] [--robotcar-batch 8]
                                   [--out profiles/localize_refine_bench.json]

times fmpnp.localize_multi over B queries with the per-query refinement (refine=True) against the batched
refinement stage (refine="batched": one wait per call instead of 1 + B), interleaved in every round, after
checking that the two return the same refined poses bit for bit.  The small shape runs at every B of --batch
with B different scenes; the RobotCar shape runs once, at --robotcar-batch queries (0: as many as
localize_multi's refine_group=None would take, which is also reported) that share one scene's references.

    python tools/localize_bench.py --query-layers [--out profiles/localize_layers_bench.json]

times one query given as its encoder layers (fmpnp.localize on the layers: layered matching, and with the refiner
the fused pack) against the dense-query chain on the same layers (assemble_hypercolumn, then fmpnp.localize on the
map), with and without the refiner, the variants interleaved in every round; the dense chain on a map assembled
beforehand is timed beside them.  The two paths' best reference and inlier count are reported (layered matching is
exact fp32 in another rounding order: near-ties may fall differently).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "featuremetric-pnp_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fmpnp  # noqa: E402
from fmpnp import _lib  # noqa: E402
from fmpnp.match import exhaustive_search_multi, gather_sparse_descriptors  # noqa: E402

SHAPES = {
    "robotcar": dict(C=1664, W=256, H=256, image=(1024, 1024), rows=1000, factor=0.006, iters=5000, f=400.0),
    "small": dict(C=128, W=64, H=64, image=(256, 256), rows=200, factor=0.01, iters=1000, f=100.0),
}
TOP_N = 10
PNP = dict(reprojection_threshold=12.0, minimum_matches=5, minimum_inliers=12, return_masked=True, seed=0)


def unit(t):
    return t / t.norm(dim=0, keepdim=True)


# --query-layers: the encoder layers (C_l, H_l, W_l) whose assembly is each shape's query map
QUERY_LAYERS = {
    "robotcar": [(128, 256, 256), (256, 128, 128), (256, 64, 64), (512, 64, 64), (512, 32, 32)],
    "small": [(32, 64, 64), (32, 32, 32), (64, 16, 16)],
}


def make_scene(shape, dev, seed=0, qmap=None):
    """qmap: the query map [C, W * H] to plant the rows from (default: a seeded random unit map)."""
    C, W, H, (im0, im1), n = shape["C"], shape["W"], shape["H"], shape["image"], shape["rows"]
    g = torch.Generator(device=dev).manual_seed(seed)
    rng = np.random.Generator(np.random.PCG64(seed))
    if qmap is None:
        qmap = unit(torch.randn(C, W * H, generator=g, device=dev))
    rmap = unit(torch.randn(C, W * H, generator=g, device=dev))
    f = shape["f"]
    K = np.array([[f, 0.0, im0 / 2], [0.0, f, im1 / 2], [0.0, 0.0, 1.0]])
    w = rng.normal(0.0, 0.2, 3)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    t = rng.normal(0.0, 0.5, 3)
    cells = rng.permutation(W * H)[:TOP_N * n].reshape(TOP_N, n)  # distinct reference cells
    cq0, cq1 = im0 / W, im1 / H
    refs = []
    for j in range(TOP_N):
        uv = np.stack([rng.uniform(cq0, im0 - cq0, n), rng.uniform(cq1, im1 - cq1, n)], 1)
        z = rng.uniform(4.0, 20.0, n)
        Pc = np.stack([(uv[:, 0] - K[0, 2]) / f * z, (uv[:, 1] - K[1, 2]) / f * z, z], 1)
        X = (Pc - t) @ R
        planted = rng.uniform(size=n) < 0.6
        qcell = (np.floor(uv[:, 1] / cq1) * H + np.floor(uv[:, 0] / cq0)).astype(np.int64)
        rc = torch.from_numpy(cells[j][planted]).to(dev)
        cols = qmap[:, torch.from_numpy(qcell[planted]).to(dev)]
        rmap[:, rc] = unit(cols + 1e-3 * torch.randn(cols.shape, generator=g, device=dev))
        i1, i0 = cells[j] // H, cells[j] % H
        p2 = np.stack([(i0 + rng.uniform(0.1, 0.9, n)) * (im1 / H), (i1 + rng.uniform(0.1, 0.9, n)) * (im0 / W)], 1)
        refs.append(dict(points_2D=p2, points_3D=X, intrinsics=K, distortion_coefficients=np.zeros(4),
                         image_resolution=(im0, im1), filename=f"ref{j}.png", planted=int(planted.sum())))
    rmap = rmap.reshape(C, W, H).contiguous()
    for r in refs:
        r["hypercolumn"] = rmap
    return qmap.reshape(C, W, H).contiguous(), refs


def staged(qmap, refs, shape, refine):
    C, W, H = qmap.shape
    image = shape["image"]
    sparse = [gather_sparse_descriptors(r["hypercolumn"], r["points_2D"], image[0] / W, image[1] / H) for r in refs]
    found = exhaustive_search_multi(qmap.reshape(C, -1), sparse, image, [W, H], None, shape["factor"])
    items = []
    for r, (pts, mask) in zip(refs, found):
        items.append((np.reshape(pts.cpu().numpy()[mask], (-1, 1, 2)), np.reshape(r["points_3D"][mask], (-1, 1, 3)),
                      r["filename"], r["points_2D"][mask], None))
    preds = fmpnp.solve_pnp_multi(items, refs[0]["intrinsics"], refs[0]["distortion_coefficients"], iters=shape["iters"],
                                  **PNP)
    ok = [(j, p) for j, p in enumerate(preds) if p.success]
    if not ok:
        return None, None
    j, best = ok[int(np.argmax([p.num_inliers for _, p in ok]))]
    out = None
    if refine:
        out = fmpnp.feature_pnp(qmap[None], refs[j]["hypercolumn"], best,
                                torch.from_numpy(np.asarray(refs[-1]["intrinsics"], np.float64)), image)
    return best, out


def chain(qmap, refs, shape, refine, match_precision="f32"):
    return fmpnp.localize(qmap, refs, shape["image"], factor=shape["factor"], iters=shape["iters"], refine=refine,
                          match_precision=match_precision, **PNP)


def precision_entry(name, shape, qmap, refs, user_refs, a):
    """localize under the two match precisions, interleaved."""
    variants = {
        "localize_f32": lambda: chain(qmap, user_refs, shape, False),
        "localize_f16": lambda: chain(qmap, user_refs, shape, False, "f16"),
        "localize_refine_f32": lambda: chain(qmap, user_refs, shape, True),
        "localize_refine_f16": lambda: chain(qmap, user_refs, shape, True, "f16"),
    }
    exact, half = variants["localize_f32"](), variants["localize_f16"]()
    per = {}
    for k, fn in variants.items():
        for _ in range(3):
            fn()
        per[k] = max(2, int(a.seconds / max(block_ms(fn, 2) * 1e-3, 1e-5)))
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            times[k].append(block_ms(fn, per[k]))
    entry = dict(shape=name, **{k: v for k, v in shape.items()}, planted=[r["planted"] for r in refs],
                 best_f32=exact.best, best_f16=half.best,
                 best_inliers_f32=None if exact.prediction is None else int(exact.prediction.num_inliers),
                 best_inliers_f16=None if half.prediction is None else int(half.prediction.num_inliers),
                 best_matches_f32=None if exact.prediction is None else int(exact.prediction.num_matches),
                 best_matches_f16=None if half.prediction is None else int(half.prediction.num_matches),
                 calls_per_block=per, **{k: stats(v) for k, v in times.items()})
    for k in ("localize", "localize_refine"):
        entry[f"{k}_speedup"] = entry[f"{k}_f32"]["median_ms"] / entry[f"{k}_f16"]["median_ms"]
    return entry


def layers_entry(name, shape, a, dev):
    """--query-layers: one query, given as its encoder layers, against its 10 references.  The dense-query chain as
    it stands without layered matching (assemble_hypercolumn of the layers, then localize on the map) against
    localize on the layers, with and without the refiner, interleaved; and the dense chain on a map assembled
    beforehand, for the assembly's share."""
    g = torch.Generator(device=dev).manual_seed(7)
    layers = [torch.randn((1, c, h, w), generator=g, device=dev) for c, h, w in QUERY_LAYERS[name]]
    C, W, H = shape["C"], shape["W"], shape["H"]
    qmap0 = fmpnp.assemble_hypercolumn(layers)[0]
    qmap, refs = make_scene(shape, dev, qmap=qmap0.reshape(C, W * H))
    user_refs = [{k: v for k, v in r.items() if k != "planted"} for r in refs]
    variants = {
        "dense": lambda: chain(fmpnp.assemble_hypercolumn(layers)[0], user_refs, shape, False),
        "layered": lambda: chain(layers, user_refs, shape, False),
        "dense_refine": lambda: chain(fmpnp.assemble_hypercolumn(layers)[0], user_refs, shape, True),
        "layered_refine": lambda: chain(layers, user_refs, shape, True),
        "dense_preassembled": lambda: chain(qmap, user_refs, shape, False),
    }
    d, l = variants["dense_refine"](), variants["layered_refine"]()
    per = {}
    for k, fn in variants.items():
        for _ in range(3):
            fn()
        per[k] = max(2, int(a.seconds / max(block_ms(fn, 2) * 1e-3, 1e-5)))
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            times[k].append(block_ms(fn, per[k]))
    t_d, t_l = (None if x.refined is None else np.asarray(x.refined[0], np.float64) for x in (d, l))
    entry = dict(shape=name, **{k: v for k, v in shape.items()}, query_layers=QUERY_LAYERS[name],
                 dense_map_bytes_not_allocated=4 * C * W * H, planted=[r["planted"] for r in refs],
                 best_dense=d.best, best_layered=l.best,
                 best_inliers_dense=None if d.prediction is None else int(d.prediction.num_inliers),
                 best_inliers_layered=None if l.prediction is None else int(l.prediction.num_inliers),
                 refined_t_difference=None if t_d is None or t_l is None else float(np.abs(t_d - t_l).max()),
                 calls_per_block=per, **{k: stats(v) for k, v in times.items()})
    for k in ("", "_refine"):
        entry[f"layered{k}_over_dense{k}"] = entry[f"layered{k}"]["median_ms"] / entry[f"dense{k}"]["median_ms"]
    entry["layered_over_dense_preassembled"] = entry["layered"]["median_ms"] / entry["dense_preassembled"]["median_ms"]
    return entry


def refine_entry(name, shape, B, scenes, a, fit=None):
    """localize_multi over B queries: refine=True (the per-query path) against refine="batched", interleaved."""
    queries = [scenes[b % len(scenes)] for b in range(B)]
    kw = dict(factor=shape["factor"], iters=shape["iters"], **PNP)
    variants = {
        "per_query": lambda: fmpnp.localize_multi(queries, shape["image"], refine=True, **kw),
        "batched": lambda: fmpnp.localize_multi(queries, shape["image"], refine="batched", **kw),
    }
    want, got = variants["per_query"](), variants["batched"]()
    same = all((x.refined is None) == (y.refined is None) and
               (x.refined is None or (np.asarray(x.refined[0]).tobytes() == np.asarray(y.refined[0]).tobytes()
                                      and np.asarray(x.refined[1]).tobytes() == np.asarray(y.refined[1]).tobytes()))
               for x, y in zip(want, got))
    per = {}
    for k, fn in variants.items():
        for _ in range(2):
            fn()
        per[k] = max(2, int(a.seconds / max(block_ms(fn, 2) * 1e-3, 1e-5)))
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            times[k].append(block_ms(fn, per[k]))
    entry = dict(shape=name, **{k: v for k, v in shape.items()}, batch=B, distinct_scenes=min(B, len(scenes)),
                 refine_group_fit=fit, refined=sum(x.refined is not None for x in got),
                 inliers=[None if x.prediction is None else int(x.prediction.num_inliers) for x in got][:8],
                 results_equal=bool(same), calls_per_block=per, host_waits=dict(per_query=1 + B, batched=1),
                 **{k: stats(v) for k, v in times.items()})
    entry["per_query_ms_per_query"] = entry["per_query"]["median_ms"] / B
    entry["batched_ms_per_query"] = entry["batched"]["median_ms"] / B
    entry["batched_minus_per_query_ms"] = entry["batched"]["median_ms"] - entry["per_query"]["median_ms"]
    entry["batched_not_slower_beyond_spread"] = bool(
        entry["batched"]["median_ms"] <= entry["per_query"]["median_ms"] + entry["per_query"]["spread_ms"])
    return entry


def refine_main(a, dev, result):
    from fmpnp import _localize as loc
    for name in a.shapes.split(","):
        shape = SHAPES[name]
        if name == "small":
            batches = [int(b) for b in a.batch.split(",")]
            scenes = []
            for b in range(max(batches)):
                qmap, refs = make_scene(shape, dev, seed=b)
                scenes.append((qmap, [{k: v for k, v in r.items() if k != "planted"} for r in refs]))
            fit = None
        else:
            qmap, refs = make_scene(shape, dev)
            scenes = [(qmap, [{k: v for k, v in r.items() if k != "planted"} for r in refs])]
            spec = loc._RefineSpec(shape["C"], shape["image"], None, None, None, "last")
            fit = loc._group_size(scenes, spec, None)
            batches = [a.robotcar_batch if a.robotcar_batch > 0 else fit]
        for B in batches:
            entry = refine_entry(name, shape, B, scenes, a, fit)
            result["shapes"].append(entry)
            print(json.dumps(entry), flush=True)
        del scenes
        torch.cuda.empty_cache()


def block_ms(fn, n):
    t = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t) * 1e3 / n


def stats(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), rounds=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.4, help="timed work per variant and round, about")
    ap.add_argument("--shapes", default="small,robotcar")
    ap.add_argument("--match-precision", choices=["f32", "f16"], default="f32",
                    help="f32: staged against localize; f16: localize with the fp16 match against the exact default")
    ap.add_argument("--refine", choices=["per-query", "batched"], default="per-query",
                    help="batched: localize_multi(refine=True) against refine=\"batched\" over --batch queries")
    ap.add_argument("--batch", default="1,8,32", help="--refine batched: the small shape's batch sizes")
    ap.add_argument("--robotcar-batch", type=int, default=8,
                    help="--refine batched: the RobotCar shape's batch size (0: what fits, refine_group=None's choice)")
    ap.add_argument("--query-layers", action="store_true",
                    help="the query as its encoder layers (layered matching) against the dense-query chain")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.require_device(dev)
    result = dict(device=torch.cuda.get_device_name(0), library_digest=_lib.library_digest(), top_n=TOP_N, pnp=PNP,
                  date=time.strftime("%Y-%m-%d"), match_precision=a.match_precision, host_waits=dict(staged=2, staged_refine=3, localize=1, localize_refine=2),
                  shapes=[])
    if a.refine == "batched":
        result["refine"] = "batched"
        refine_main(a, dev, result)
    for name in a.shapes.split(",") if a.refine != "batched" else ():
        shape = SHAPES[name]
        if a.query_layers:
            result["query"] = "layers"
            entry = layers_entry(name, shape, a, dev)
            result["shapes"].append(entry)
            print(json.dumps(entry), flush=True)
            torch.cuda.empty_cache()
            continue
        qmap, refs = make_scene(shape, dev)
        user_refs = [{k: v for k, v in r.items() if k != "planted"} for r in refs]
        if a.match_precision == "f16":
            entry = precision_entry(name, shape, qmap, refs, user_refs, a)
            result["shapes"].append(entry)
            print(json.dumps(entry), flush=True)
            del qmap, refs, user_refs
            torch.cuda.empty_cache()
            continue
        variants = {
            "staged": lambda: staged(qmap, user_refs, shape, False),
            "localize": lambda: chain(qmap, user_refs, shape, False),
            "staged_refine": lambda: staged(qmap, user_refs, shape, True),
            "localize_refine": lambda: chain(qmap, user_refs, shape, True),
        }
        # the two paths on identical inputs: equal results first
        sb, sr = staged(qmap, user_refs, shape, True)
        lb = chain(qmap, user_refs, shape, True)
        same = (sb is not None and lb.prediction is not None
                and all(np.asarray(getattr(sb, k)).tobytes() == np.asarray(getattr(lb.prediction, k)).tobytes()
                        for k in ("matrix", "inlier_mask", "points_3d", "query_inliers", "reference_inliers"))
                and sr[1].numpy().tobytes() == np.asarray(lb.refined[0]).tobytes())
        per = {}
        for k, fn in variants.items():  # warm-up, and the block length of each variant
            for _ in range(3):
                fn()
            per[k] = max(2, int(a.seconds / max(block_ms(fn, 2) * 1e-3, 1e-5)))
        times = {k: [] for k in variants}
        for _ in range(a.rounds):  # interleaved: every round runs the four variants one after the other
            for k, fn in variants.items():
                times[k].append(block_ms(fn, per[k]))
        entry = dict(shape=name, **{k: v for k, v in shape.items()}, planted=[r["planted"] for r in refs],
                     best_inliers=None if sb is None else int(sb.num_inliers), results_equal=bool(same),
                     calls_per_block=per, **{k: stats(v) for k, v in times.items()})
        for x, y in (("staged", "localize"), ("staged_refine", "localize_refine")):
            entry[f"{y}_minus_{x}_ms"] = entry[y]["median_ms"] - entry[x]["median_ms"]
            entry[f"{y}_not_slower_beyond_spread"] = bool(entry[y]["median_ms"] <= entry[x]["median_ms"] + entry[x]["spread_ms"])
        result["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        del qmap, refs, user_refs, variants
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
