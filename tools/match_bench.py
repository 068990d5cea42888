"""Dense exhaustive matching at the RobotCar shape: libfmpnp's path against the reference's method
restated in PyTorch-ROCm on the same GPU, interleaved in one process.

    python tools/match_bench.py [--out profiles/match_bench.json] [--seconds 0.6]

Shape: C = 1664, a 256 x 256 map, factor 0.006 (top_k = 393), N = 295, 866, 2048 reference points,
and one exhaustive_search_multi of 10 references of N = 866.
  ours      fmpnp.exhaustive_match: the fp32-MFMA correlation + the per-row radix select, host
            results (argmax, d1, d_k, mask) copied back, the stream waited for.
  baseline  exhaustive_search.py:45-49 restated: torch.mm, one batched topk(top_k) instead of the
            per-row Python loop (which only favours the baseline), the ratio test, the same results
            copied back.  torch's fp32 mm is rocBLAS / hipBLASLt, not a k-ordered fmaf chain: it is
            the speed yardstick, not a numeric one (the winners are compared and reported).
Each is timed with a host clock around calls that end in a device synchronise, in alternating blocks
(ours, baseline, ours, ...) after warming both; the median block is reported with min and max.
The correlation alone (fmpnp_correlation_async, device events) is reported as TFLOP/s against the
157.3 TF fp32-matrix peak; the select's time is the difference to the whole asynchronous sequence.

    python tools/match_bench.py --precision f16 [--out profiles/match_bench_f16.json]

times the opt-in fp16 precision against the exact one instead, every figure beside the f32 figure of the same
run in alternating blocks (median, min, max): the correlation alone by device events
(fmpnp_correlation_ex_async with FMPNP_MATCH_F16, the conversion of both operands included, against
fmpnp_correlation_async), the whole asynchronous sequence and the select's share of it, the whole
exhaustive_match by the host clock, ten references in one exhaustive_search_multi, and the fraction of rows on
which the two precisions pick the same argmax and the same mask.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "featuremetric-pnp_amd")]
import torch  # noqa: E402

import fmpnp  # noqa: E402
from fmpnp import _lib  # noqa: E402

C, W, H, FACTOR, RATIO = 1664, 256, 256, 0.006, 0.9
PEAK_TF = 157.3


def unit(x, dim):
    return x / x.norm(dim=dim, keepdim=True)


def baseline(sparse, dense, top_k):
    corr = torch.mm(sparse, dense)
    dist, ind = corr.topk(top_k, dim=-1, largest=True)
    mask = (RATIO ** 2) * dist[:, 0] >= dist[:, -1]
    return ind[:, 0].cpu(), dist[:, 0].cpu(), dist[:, -1].cpu(), mask.cpu()


def blocks(fns, seconds):
    """Alternating timed blocks of each function; returns per function the list of ms per call."""
    for f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    per = []
    for f in fns:  # calls per block: about `seconds` / 5 of work
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        per.append(max(2, int(seconds / 5 / max(time.perf_counter() - t, 1e-5))))
    out = [[] for _ in fns]
    for _ in range(5):
        for i, f in enumerate(fns):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(per[i]):
                f()
            torch.cuda.synchronize()
            out[i].append((time.perf_counter() - t) * 1e3 / per[i])
    return out


def stats(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def events_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def event_blocks(fns, reps, rounds=5):
    """Alternating device-event blocks of each function; per function the list of ms per call."""
    out = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            out[i].append(events_ms(f, reps))
    return out


def main_f16(a):
    dev = torch.device("cuda", 0)
    _lib.require_device(dev)
    L, st = _lib.load(), _lib.stream_ptr(dev)
    wh, top_k = W * H, int(FACTOR * W * H)
    g = torch.Generator(device="cpu").manual_seed(1)
    dense = unit(torch.randn((C, wh), generator=g), 0).to(dev)
    result = dict(device=torch.cuda.get_device_name(0), library_digest=_lib.library_digest(), C=C, map=[W, H],
                  factor=FACTOR, top_k=top_k, precision="f16", shapes=[])
    vp = ctypes.c_void_p
    for n in a.sizes:
        sparse = unit(torch.randn((n, C), generator=g), 1).to(dev)
        f16_ms, f32_ms = blocks([lambda: fmpnp.exhaustive_match(sparse, dense, top_k, RATIO, precision="f16"),
                                 lambda: fmpnp.exhaustive_match(sparse, dense, top_k, RATIO)], a.seconds)
        scores = torch.empty((n, wh), dtype=torch.float32, device=dev)
        outs = [torch.empty(n, dtype=t, device=dev) for t in (torch.int32, torch.float32, torch.float32, torch.uint8)]
        nbytes = int(L.fmpnp_match_workspace_size_ex(n, C, wh, _lib.MATCH_F16))
        ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=dev)

        def corr16():
            _lib.check(L.fmpnp_correlation_ex_async(vp(sparse.data_ptr()), n, C, vp(dense.data_ptr()), C, wh, wh,
                                                    vp(scores.data_ptr()), vp(ws.data_ptr()), nbytes, _lib.MATCH_F16, st),
                       "corr f16")

        def corr32():
            _lib.check(L.fmpnp_correlation_async(vp(sparse.data_ptr()), n, C, vp(dense.data_ptr()), C, wh, wh,
                                                 vp(scores.data_ptr()), st), "corr")

        def whole16():
            _lib.check(L.fmpnp_exhaustive_match_ex_async(vp(sparse.data_ptr()), n, C, vp(dense.data_ptr()), C, wh, wh, top_k,
                                                         RATIO, *[vp(o.data_ptr()) for o in outs], vp(scores.data_ptr()),
                                                         vp(ws.data_ptr()), nbytes, _lib.MATCH_F16, st), "match f16")

        def whole32():
            _lib.check(L.fmpnp_exhaustive_match_async(vp(sparse.data_ptr()), n, C, vp(dense.data_ptr()), C, wh, wh, top_k,
                                                      RATIO, *[vp(o.data_ptr()) for o in outs], vp(scores.data_ptr()),
                                                      None, 0, st), "match")
        reps = max(3, int(a.seconds / 3 / 0.004))
        c16, c32, w16, w32 = event_blocks([corr16, corr32, whole16, whole32], reps)
        flop = 2.0 * n * wh * C
        r16 = fmpnp.exhaustive_match(sparse, dense, top_k, RATIO, precision="f16")
        r32 = fmpnp.exhaustive_match(sparse, dense, top_k, RATIO)
        m16, m32 = statistics.median(c16), statistics.median(c32)
        sel = statistics.median(w16) - m16
        entry = dict(N=n, correlation_f16=stats(c16), correlation_f32=stats(c32), correlation_speedup=m32 / m16,
                     correlation_f16_tflops=flop / m16 / 1e9, correlation_f32_tflops=flop / m32 / 1e9,
                     async_sequence_f16=stats(w16), async_sequence_f32=stats(w32), select_f16_ms=sel,
                     select_share_of_f16_sequence=sel / statistics.median(w16),
                     exhaustive_match_f16=stats(f16_ms), exhaustive_match_f32=stats(f32_ms),
                     exhaustive_match_speedup=statistics.median(f32_ms) / statistics.median(f16_ms),
                     argmax_agree=float((r16["argmax"] == r32["argmax"]).mean()),
                     mask_agree=float((r16["mask"] == r32["mask"]).mean()))
        result["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        del scores, ws
    n = 866
    refs = [unit(torch.randn((n, C), generator=g), 1).to(dev) for _ in range(10)]
    args = ([1024, 1024], [W, H], [4, 4], FACTOR)
    m16, m32 = blocks([lambda: fmpnp.exhaustive_search_multi(dense, refs, *args, precision="f16"),
                       lambda: fmpnp.exhaustive_search_multi(dense, refs, *args)], a.seconds)
    result["multi"] = dict(references=10, N=n, multi_f16=stats(m16), multi_f32=stats(m32),
                           speedup=statistics.median(m32) / statistics.median(m16))
    print(json.dumps(result["multi"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


# the RobotCar hypercolumn's layers (C_l, H_l, W_l): 1664 channels on a 256 x 256 map
LAYERS = [(128, 256, 256), (256, 128, 128), (256, 64, 64), (512, 64, 64), (512, 32, 32)]


def main_layers(a):
    """--layers: the query given as its layers.  Two paths in alternating blocks in one process: (a) the path as it
    stands without layered matching, assemble_hypercolumn + exhaustive_match on the assembled [C, W * H] map, and
    (b) exhaustive_match_layers on the layers.  By device events, also in alternating blocks: the per-layer
    correlations alone (fmpnp_correlation_async on each layer), the layered score map without and with the norm
    (fmpnp_correlation_layers_async; the combine and the norm plane are the differences), and the whole
    asynchronous sequence."""
    dev = torch.device("cuda", 0)
    _lib.require_device(dev)
    L, st = _lib.load(), _lib.stream_ptr(dev)
    wh, top_k = W * H, int(FACTOR * W * H)
    g = torch.Generator(device="cpu").manual_seed(1)
    layers = [torch.randn((1, c, h, w), generator=g).to(dev) for c, h, w in LAYERS]
    from fmpnp.hypercolumn import _plane_layers
    desc, keep = _plane_layers(layers, "cuda")
    dense_bytes = 4 * C * wh
    result = dict(device=torch.cuda.get_device_name(0), library_digest=_lib.library_digest(), C=C, map=[W, H],
                  layers=LAYERS, factor=FACTOR, top_k=top_k, dense_map_bytes_not_allocated=dense_bytes,
                  macs_per_row_dense=C * wh, macs_per_row_layered=sum(c * h * w for c, h, w in LAYERS), shapes=[])
    vp = ctypes.c_void_p

    def dense_path(sparse):
        return fmpnp.exhaustive_match(sparse, fmpnp.assemble_hypercolumn(layers)[0].view(C, -1), top_k, RATIO)

    for n in a.sizes:
        sparse = unit(torch.randn((n, C), generator=g), 1).to(dev)
        dense_ms, lay_ms = blocks([lambda: dense_path(sparse), lambda: fmpnp.exhaustive_match_layers(sparse, layers, top_k, RATIO)],
                                  a.seconds)
        match_ms, = blocks([lambda: fmpnp.exhaustive_match(sparse, dmap, top_k, RATIO)
                            for dmap in [fmpnp.assemble_hypercolumn(layers)[0].view(C, -1)]], a.seconds)
        scores = torch.empty((n, wh), dtype=torch.float32, device=dev)
        outs = [torch.empty(n, dtype=t, device=dev) for t in (torch.int32, torch.float32, torch.float32, torch.uint8)]
        nbytes = int(L.fmpnp_match_layers_workspace_size(desc, len(keep), n, H, W))
        ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=dev)
        coarse = [torch.empty((n, h * w), dtype=torch.float32, device=dev) for _, h, w in LAYERS]

        def per_layer():
            off = 0
            for (c, h, w), m, out in zip(LAYERS, layers, coarse):
                _lib.check(L.fmpnp_correlation_async(vp(sparse.data_ptr() + 4 * off), n, C, vp(m.data_ptr()), c, h * w, h * w,
                                                     vp(out.data_ptr()), st), "corr")
                off += c

        def score_map(flags):
            _lib.check(L.fmpnp_correlation_layers_async(vp(sparse.data_ptr()), n, C, desc, len(keep), 1, 0, H, W, flags,
                                                        vp(scores.data_ptr()), vp(ws.data_ptr()), nbytes, st), "layers corr")

        def whole():
            _lib.check(L.fmpnp_exhaustive_match_layers_async(vp(sparse.data_ptr()), n, C, desc, len(keep), 1, 0, H, W,
                                                             _lib.HC_NORMALIZE, top_k, RATIO, *[vp(o.data_ptr()) for o in outs],
                                                             None, vp(ws.data_ptr()), nbytes, st), "layers match")
        reps = max(3, int(a.seconds / 3 / 0.002))
        e_corr, e_plain, e_norm, e_whole = event_blocks([per_layer, lambda: score_map(0), lambda: score_map(_lib.HC_NORMALIZE),
                                                         whole], reps)
        m_corr, m_plain, m_norm, m_whole = (statistics.median(x) for x in (e_corr, e_plain, e_norm, e_whole))
        rd, rl = dense_path(sparse), fmpnp.exhaustive_match_layers(sparse, layers, top_k, RATIO)
        entry = dict(N=n, dense_assemble_and_match=stats(dense_ms), dense_match_alone=stats(match_ms), layered=stats(lay_ms),
                     ratio_layered_over_dense=statistics.median(lay_ms) / statistics.median(dense_ms),
                     ratio_layered_over_dense_match_alone=statistics.median(lay_ms) / statistics.median(match_ms),
                     per_layer_correlations=stats(e_corr), score_map_without_norm=stats(e_plain),
                     score_map_with_norm=stats(e_norm), async_sequence=stats(e_whole),
                     combine_ms=m_plain - m_corr, norm_plane_and_division_ms=m_norm - m_plain, select_ms=m_whole - m_norm,
                     rounds=-(-n // max(1, (256 << 20) // (4 * (wh + sum(h * w for _, h, w in LAYERS))))),
                     argmax_agree=float((rd["argmax"] == rl["argmax"]).mean()), mask_agree=float((rd["mask"] == rl["mask"]).mean()))
        result["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        del scores, ws, coarse
    n = 866
    refs = [unit(torch.randn((n, C), generator=g), 1).to(dev) for _ in range(10)]
    dense_ms, lay_ms = blocks([lambda: fmpnp.exhaustive_search_multi(fmpnp.assemble_hypercolumn(layers)[0].view(C, -1), refs,
                                                                     [1024, 1024], [W, H], [4, 4], FACTOR),
                               lambda: fmpnp.exhaustive_search_layers_multi(layers, refs, [1024, 1024], [4, 4], FACTOR)],
                              a.seconds)
    result["multi"] = dict(references=10, N=n, dense_assemble_and_multi=stats(dense_ms), layered_multi=stats(lay_ms),
                           ratio_layered_over_dense=statistics.median(lay_ms) / statistics.median(dense_ms))
    print(json.dumps(result["multi"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", action="store_true",
                    help="the query as its encoder layers: layered matching against assemble + exhaustive_match")
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.6, help="timed work per variant and shape, about")
    ap.add_argument("--sizes", type=int, nargs="*", default=[295, 866, 2048])
    ap.add_argument("--precision", choices=["f32", "f16"], default="f32",
                    help="f32: ours against the PyTorch baseline; f16: the fp16 precision against the exact one")
    a = ap.parse_args()
    if a.layers:
        return main_layers(a)
    if a.precision == "f16":
        return main_f16(a)
    dev = torch.device("cuda", 0)
    _lib.require_device(dev)
    L, st = _lib.load(), _lib.stream_ptr(dev)
    wh, top_k = W * H, int(FACTOR * W * H)
    g = torch.Generator(device="cpu").manual_seed(1)
    dense = unit(torch.randn((C, wh), generator=g), 0).to(dev)
    result = dict(device=torch.cuda.get_device_name(0), library_digest=_lib.library_digest(), C=C, map=[W, H],
                  factor=FACTOR, top_k=top_k, peak_fp32_matrix_tflops=PEAK_TF, shapes=[])
    vp = ctypes.c_void_p
    for n in a.sizes:
        sparse = unit(torch.randn((n, C), generator=g), 1).to(dev)
        ours_ms, base_ms = blocks([lambda: fmpnp.exhaustive_match(sparse, dense, top_k, RATIO),
                                   lambda: baseline(sparse, dense, top_k)], a.seconds)
        # the correlation alone and the whole asynchronous sequence, by device events
        scores = torch.empty((n, wh), dtype=torch.float32, device=dev)
        outs = [torch.empty(n, dtype=t, device=dev) for t in (torch.int32, torch.float32, torch.float32, torch.uint8)]

        def corr():
            _lib.check(L.fmpnp_correlation_async(vp(sparse.data_ptr()), n, C, vp(dense.data_ptr()), C, wh, wh,
                                                 vp(scores.data_ptr()), st), "corr")

        def whole():
            _lib.check(L.fmpnp_exhaustive_match_async(vp(sparse.data_ptr()), n, C, vp(dense.data_ptr()), C, wh, wh, top_k,
                                                      RATIO, *[vp(o.data_ptr()) for o in outs], vp(scores.data_ptr()),
                                                      None, 0, st), "match")
        reps = max(3, int(a.seconds / 3 / 0.004))
        corr_ms, whole_ms = events_ms(corr, reps), events_ms(whole, reps)
        os.environ["FMPNP_MATCH_XCD"] = "0"  # the other block order (column tiles fastest), for the record
        corr_colmajor_ms = events_ms(corr, reps)
        del os.environ["FMPNP_MATCH_XCD"]
        mm_ms = events_ms(lambda: torch.mm(sparse, dense, out=scores), reps)
        flop = 2.0 * n * wh * C
        # do the two methods pick the same winners? (another summation order: equal except at near-ties)
        r, b = fmpnp.exhaustive_match(sparse, dense, top_k, RATIO), baseline(sparse, dense, top_k)
        entry = dict(N=n, ours=stats(ours_ms), baseline=stats(base_ms),
                     ratio_ours_over_baseline=statistics.median(ours_ms) / statistics.median(base_ms),
                     correlation_ms=corr_ms, correlation_tflops=flop / corr_ms / 1e9,
                     correlation_share_of_peak=flop / corr_ms / 1e9 / PEAK_TF,
                     correlation_column_order_ms=corr_colmajor_ms, torch_mm_ms=mm_ms,
                     torch_mm_tflops=flop / mm_ms / 1e9, async_sequence_ms=whole_ms, select_ms=whole_ms - corr_ms,
                     argmax_agree=float((torch.from_numpy(r["argmax"]).long() == b[0]).float().mean()),
                     mask_agree=float((torch.from_numpy(r["mask"]) == b[3]).float().mean()))
        result["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        del scores
    # ten references of one query in one call against ten baseline calls
    n = 866
    refs = [unit(torch.randn((n, C), generator=g), 1).to(dev) for _ in range(10)]
    args = ([1024, 1024], [W, H], [4, 4], FACTOR)
    multi_ms, sep_ms, base_ms = blocks([lambda: fmpnp.exhaustive_search_multi(dense, refs, *args),
                                        lambda: [fmpnp.exhaustive_search(dense, s, *args) for s in refs],
                                        lambda: [baseline(s, dense, top_k) for s in refs]], a.seconds)
    result["multi"] = dict(references=10, N=n, ours_multi=stats(multi_ms), ours_separate=stats(sep_ms),
                           baseline_separate=stats(base_ms),
                           ratio_multi_over_baseline=statistics.median(multi_ms) / statistics.median(base_ms))
    print(json.dumps(result["multi"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
