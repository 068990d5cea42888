"""The encoder's operators at VGG-16's shapes: libfmpnp's exact-fp32 convolution and HipEncoder's walk against
PyTorch-ROCm's own (MIOpen) on the same tensors and the same GPU, interleaved in one process.

    python tools/encoder_bench.py [--out profiles/encoder_bench.json] [--seconds 0.3]

Shapes: every distinct convolution of VGG-16's features up to child 24 (the last hypercolumn tap) at a
1024 x 1024 image (RobotCar's image_shape) and at 512 x 512, B = 1 and B = 4, with bias and the fused ReLU.
  ours      fmpnp.conv3x3(x, w, b, relu=True): one launch of the implicit-GEMM kernel.
  baseline  torch.relu_(torch.nn.functional.conv2d(x, w, b, padding=1)): the framework's choice of algorithm
            (which may be a Winograd form with fewer multiplications than an exact chain can have) and its
            in-place ReLU.  It is the speed yardstick, not a numeric one; the largest difference is reported.
Each is timed by device events around `reps` launches, in alternating blocks (ours, baseline, ours, ...) after
warming both; the median block is reported with min and max.  Per convolution: ms, TFLOP/s (2 * 9 * Cin * Cout *
B * H * W), and the share of the 157.3 TF exact-fp32 matrix peak, beside the match stage's correlation on its own
shapes (profiles/match_bench.json), the project's yardstick for the same instruction.
Then the walk to child 24 (HipEncoder.feature_maps against the reference's loop through the framework) and the whole
29-child encoder (the retrieval path: HipEncoder.forward against the nn.Sequential), by the host clock around calls
that end in a device synchronise, in the same alternating blocks.  No pass or fail ratio is set.

    python tools/encoder_bench.py --precision f16 [--out profiles/encoder_bench_f16.json]

The opt-in fp16 precision by the same method: per convolution three alternating blocks -- conv3x3(precision="f16") on
the weight image packed once, the exact kernel (the yardstick: its source is the parent commit's), and the framework
-- with the largest difference of the f16 output to the exact one; then the walk and the whole encoder for
HipEncoder(precision="f16"), HipEncoder and the framework, with the largest per-element difference between the two
walks' tapped maps and between their assembled L2-normalised hypercolumns.  Reported, not asserted.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "featuremetric-pnp_amd")]
import torch  # noqa: E402
from torch import nn  # noqa: E402

import fmpnp  # noqa: E402
from fmpnp import _lib  # noqa: E402

PEAK_TF = 157.3
# (Cin, Cout, divisor of the image size): VGG-16's distinct convolutions up to child 24
CONVS = [(3, 64, 1), (64, 64, 1), (64, 128, 2), (128, 128, 2), (128, 256, 4), (256, 256, 4), (256, 512, 8),
         (512, 512, 8)]
BLOCKS, WIDTHS = (2, 2, 3, 3, 3), (64, 128, 256, 512, 512)
TAPS = [9, 14, 17, 21, 24]


def vgg16_features():
    """torchvision's vgg16().features[:-2] written out (random weights: the speed does not depend on them)."""
    layers, cin = [], 3
    for n, width in zip(BLOCKS, WIDTHS):
        for _ in range(n):
            layers += [nn.Conv2d(cin, width, 3, padding=1), nn.ReLU(inplace=True)]
            cin = width
        layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
    return nn.Sequential(*layers[:-2]).eval()


def stats(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def events_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def event_blocks(fns, seconds, rounds=5):
    """Alternating device-event blocks of each function after warming each; per function the list of ms per call."""
    reps = []
    for f in fns:
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        reps.append(max(2, min(200, int(seconds / rounds / max(events_ms(f, 2) * 1e-3, 1e-6)))))
    out = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            out[i].append(events_ms(f, reps[i]))
    return out


def host_blocks(fns, seconds, rounds=5):
    """Alternating host-clock blocks of calls followed by a device synchronise; per function the list of ms per call."""
    per = []
    for f in fns:
        for _ in range(2):
            f()
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        per.append(max(1, min(50, int(seconds / rounds / max(time.perf_counter() - t, 1e-5)))))
    out = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(per[i]):
                f()
            torch.cuda.synchronize()
            out[i].append((time.perf_counter() - t) * 1e3 / per[i])
    return out


def torch_walk(net, batch):
    maps, j, fm = [], 0, batch
    with torch.no_grad():
        for i, layer in enumerate(net.children()):
            if j == len(TAPS):
                break
            if i == TAPS[j]:
                maps.append(fm)
                j += 1
            fm = layer(fm)
    return maps


def spread(ms):
    """(max - min) / median of a variant's blocks."""
    return (max(ms) - min(ms)) / statistics.median(ms)


def main_f16(a):
    dev = torch.device("cuda", 0)
    _lib.require_device(dev)
    result = dict(device=torch.cuda.get_device_name(0), library_digest=_lib.library_digest(), precision="f16",
                  peak_fp32_matrix_tflops=PEAK_TF, peak_fp16_matrix_tflops=16 * PEAK_TF, convs=[], walks=[])
    g = torch.Generator(device="cpu").manual_seed(1)
    for size in a.sizes:
        for batch in a.batches:
            for cin, cout, div in CONVS:
                h = w = size // div
                x = torch.randn((batch, cin, h, w), generator=g).to(dev)
                wt = (torch.randn((cout, cin, 3, 3), generator=g) / (9 * cin) ** 0.5).to(dev)
                bias = torch.randn((cout,), generator=g).to(dev)
                out = torch.empty((batch, cout, h, w), device=dev)
                out16 = torch.empty((batch, cout, h, w), device=dev)
                image = fmpnp.conv3x3_f16_weights(wt)

                def half():
                    fmpnp.conv3x3(x, image, bias, relu=True, out=out16, precision="f16")

                def exact():
                    fmpnp.conv3x3(x, wt, bias, relu=True, out=out)

                def base():
                    torch.relu_(torch.nn.functional.conv2d(x, wt, bias, padding=1))
                with torch.no_grad():
                    h_ms, e_ms, b_ms = event_blocks([half, exact, base], a.seconds)
                    diff = float((out16 - out).abs().max())
                    scale = float(out.abs().max())
                flop = 2.0 * 9 * cin * cout * batch * h * w
                mh, me, mb = statistics.median(h_ms), statistics.median(e_ms), statistics.median(b_ms)
                # "faster beyond the spread": the f16 blocks' slowest is below the exact blocks' fastest
                entry = dict(image=size, B=batch, Cin=cin, Cout=cout, H=h, W=w, gflop=flop / 1e9, f16=stats(h_ms),
                             exact=stats(e_ms), baseline=stats(b_ms), f16_tflops=flop / mh / 1e9,
                             f16_share_of_fp16_peak=flop / mh / 1e9 / (16 * PEAK_TF), exact_tflops=flop / me / 1e9,
                             baseline_tflops=flop / mb / 1e9, speedup_exact_over_f16=me / mh,
                             ratio_f16_over_baseline=mh / mb, f16_spread=spread(h_ms), exact_spread=spread(e_ms),
                             faster_beyond_spread=max(h_ms) < min(e_ms),
                             activation_mbytes=4.0 * batch * (cin + cout) * h * w / 1e6,
                             max_abs_difference_to_exact=diff, max_abs_exact=scale)
                result["convs"].append(entry)
                print(json.dumps(entry), flush=True)
                del x, wt, bias, out, out16, image
            torch.manual_seed(2)
            net = vgg16_features().to(dev)
            enc16, enc = fmpnp.HipEncoder(net, precision="f16"), fmpnp.HipEncoder(net)
            image = torch.randn((batch, 3, size, size), generator=g).to(dev)
            with torch.no_grad():
                wh, we, wb = host_blocks([lambda: enc16.feature_maps(image, TAPS), lambda: enc.feature_maps(image, TAPS),
                                          lambda: torch_walk(net, image)], a.seconds)
                eh, ee, eb = host_blocks([lambda: enc16(image), lambda: enc(image), lambda: net(image)], a.seconds)
                m16, m32 = enc16.feature_maps(image, TAPS), enc.feature_maps(image, TAPS)
                map_diffs = [dict(child=t, max_abs_difference=float((p - q).abs().max()), max_abs_exact=float(q.abs().max()))
                             for t, p, q in zip(TAPS, m16, m32)]
                hyper_diff = None
                if batch * size * size <= 4 * 512 * 512:  # (the dense hypercolumn of a 1024^2 batch of 4 is 9 GB)
                    hyper_diff = float((fmpnp.assemble_hypercolumn(m16) - fmpnp.assemble_hypercolumn(m32)).abs().max())
                del m16, m32

            def walk(hm, em, bm):
                return dict(f16=stats(hm), exact=stats(em), baseline=stats(bm),
                            speedup_exact_over_f16=statistics.median(em) / statistics.median(hm),
                            ratio_f16_over_baseline=statistics.median(hm) / statistics.median(bm),
                            faster_beyond_spread=max(hm) < min(em))
            entry = dict(image=size, B=batch, walk_to_child_24=walk(wh, we, wb), whole_encoder=walk(eh, ee, eb),
                         tapped_maps=map_diffs, max_abs_hypercolumn_difference=hyper_diff)
            result["walks"].append(entry)
            print(json.dumps(entry), flush=True)
            del net, enc, enc16, image
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.3, help="timed work per variant and shape, about")
    ap.add_argument("--sizes", type=int, nargs="*", default=[1024, 512])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 4])
    ap.add_argument("--precision", choices=("f32", "f16"), default="f32",
                    help="f16: the fp16 precision against the exact kernel and the framework")
    a = ap.parse_args()
    if a.precision == "f16":
        return main_f16(a)
    dev = torch.device("cuda", 0)
    _lib.require_device(dev)
    result = dict(device=torch.cuda.get_device_name(0), library_digest=_lib.library_digest(),
                  peak_fp32_matrix_tflops=PEAK_TF, convs=[], walks=[])
    try:  # the project's yardstick for v_mfma_f32_32x32x2_f32: the match stage's correlation on its own shapes
        with open(os.path.join(ROOT, "profiles", "match_bench.json")) as f:
            result["match_correlation_share_of_peak"] = {str(s["N"]): s["correlation_share_of_peak"]
                                                         for s in json.load(f)["shapes"]}
    except (OSError, KeyError, ValueError):
        result["match_correlation_share_of_peak"] = None
    g = torch.Generator(device="cpu").manual_seed(1)
    for size in a.sizes:
        for batch in a.batches:
            for cin, cout, div in CONVS:
                h = w = size // div
                x = torch.randn((batch, cin, h, w), generator=g).to(dev)
                wt = (torch.randn((cout, cin, 3, 3), generator=g) / (9 * cin) ** 0.5).to(dev)
                bias = torch.randn((cout,), generator=g).to(dev)
                out = torch.empty((batch, cout, h, w), device=dev)

                def ours():
                    fmpnp.conv3x3(x, wt, bias, relu=True, out=out)

                def base():
                    torch.relu_(torch.nn.functional.conv2d(x, wt, bias, padding=1))
                with torch.no_grad():
                    o_ms, b_ms = event_blocks([ours, base], a.seconds)
                    diff = float((out - torch.relu_(torch.nn.functional.conv2d(x, wt, bias, padding=1))).abs().max())
                flop = 2.0 * 9 * cin * cout * batch * h * w
                mo, mb = statistics.median(o_ms), statistics.median(b_ms)
                entry = dict(image=size, B=batch, Cin=cin, Cout=cout, H=h, W=w, gflop=flop / 1e9, ours=stats(o_ms),
                             baseline=stats(b_ms), ours_tflops=flop / mo / 1e9, ours_share_of_peak=flop / mo / 1e9 / PEAK_TF,
                             baseline_tflops=flop / mb / 1e9, ratio_ours_over_baseline=mo / mb,
                             max_abs_difference=diff)
                result["convs"].append(entry)
                print(json.dumps(entry), flush=True)
                del x, wt, bias, out
            torch.manual_seed(2)
            net = vgg16_features().to(dev)
            enc = fmpnp.HipEncoder(net)
            image = torch.randn((batch, 3, size, size), generator=g).to(dev)
            with torch.no_grad():
                wo, wb = host_blocks([lambda: enc.feature_maps(image, TAPS), lambda: torch_walk(net, image)], a.seconds)
                eo, eb = host_blocks([lambda: enc(image), lambda: net(image)], a.seconds)
            entry = dict(image=size, B=batch, walk_to_child_24=dict(
                ours=stats(wo), baseline=stats(wb), ratio_ours_over_baseline=statistics.median(wo) / statistics.median(wb)),
                whole_encoder=dict(ours=stats(eo), baseline=stats(eb),
                                   ratio_ours_over_baseline=statistics.median(eo) / statistics.median(eb)))
            result["walks"].append(entry)
            print(json.dumps(entry), flush=True)
            del net, enc, image
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
