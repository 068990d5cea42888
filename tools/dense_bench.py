"""The d2-net dense features' operators at a D2-Net trunk's shapes, against PyTorch-ROCm's own (MIOpen) on the same
tensors and the same GPU, interleaved in one process (tools/encoder_bench.py's method: alternating blocks after
warming each, the median block with min and max; device events around the launches of an operator, the host clock
around calls that end in a device synchronise for the walks).  No pass or fail ratio is set.

    python tools/dense_bench.py [--out profiles/dense_bench.json] [--seconds 0.3] [--tile-libs 4=PATH 6=PATH ...]

  convs     the dilated layers alone, 256 -> 512 and 512 -> 512 at 255 x 255 and 127 x 127, B = 1, bias and fused ReLU:
            fmpnp.conv3x3(dilation=2), this library's dilation=1 kernel on the same shape (the same multiply-adds:
            the difference is the halo), and torch.relu_(F.conv2d(dilation=2, padding=2)).
  tiles     the tile choice: the same launch through libraries built with EXTRA=-DFMPNP_CONV_D2_LW=n (the dilated
            form's widest tile is TW = 1 << n columns), each handed over as n=PATH, beside the library in use.
  step      fmpnp.dense_pyramid_step at C = 512, 255 x 255 from 127 x 127, against F.interpolate + add + F.normalize.
  pool      fmpnp.avgpool2x2s1 at 256 x 256 x 256 against F.avg_pool2d(2, 1).
  walks     DenseFeatureExtractor.extract on d2net_trunk() at 1024 x 1024, single scale and multiscale (its scale 2
            is a 2048 x 2048 image), backend "hip" against backend "torch" (trunk(x), F.relu, F.interpolate,
            F.normalize through the framework), with each one's peak device memory.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "featuremetric-pnp_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import fmpnp  # noqa: E402
from fmpnp import _lib  # noqa: E402

from encoder_bench import PEAK_TF, event_blocks, host_blocks, spread, stats  # noqa: E402

CONVS = [(256, 512, 255), (512, 512, 255), (256, 512, 127), (512, 512, 127)]  # (Cin, Cout, H = W)


def tile_launcher(path):
    """fmpnp_conv3x3_dilated_async of the library at `path` as f(x, w, b, out) on the current stream."""
    lib = ctypes.CDLL(path)
    fn = lib.fmpnp_conv3x3_dilated_async
    vp, i = ctypes.c_void_p, ctypes.c_int
    fn.argtypes = [vp, i, i, i, i, vp, vp, i, i, vp, i, vp]
    fn.restype = i

    def call(x, w, b, out):
        bsz, cin, h, wd = x.shape
        rc = fn(x.data_ptr(), bsz, cin, h, wd, w.data_ptr(), b.data_ptr(), w.shape[0], _lib.CONV_BIAS | _lib.CONV_RELU,
                out.data_ptr(), 2, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.3, help="timed work per variant and shape, about")
    ap.add_argument("--tile-libs", nargs="*", default=[], help="n=PATH: a library built with -DFMPNP_CONV_D2_LW=n")
    ap.add_argument("--skip-walks", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.require_device(dev)
    result = dict(device=torch.cuda.get_device_name(0), library_digest=_lib.library_digest(),
                  peak_fp32_matrix_tflops=PEAK_TF, convs=[], tiles=[], walks=[])
    tiles = {int(t.split("=", 1)[0]): tile_launcher(t.split("=", 1)[1]) for t in a.tile_libs}
    g = torch.Generator(device="cpu").manual_seed(1)
    with torch.no_grad():
        for cin, cout, size in CONVS:
            x = torch.randn((1, cin, size, size), generator=g).to(dev)
            wt = (torch.randn((cout, cin, 3, 3), generator=g) / (9 * cin) ** 0.5).to(dev)
            bias = torch.randn((cout,), generator=g).to(dev)
            out = torch.empty((1, cout, size, size), device=dev)
            flop = 2.0 * 9 * cin * cout * size * size

            def dilated():
                fmpnp.conv3x3(x, wt, bias, relu=True, out=out, dilation=2)

            def plain():
                fmpnp.conv3x3(x, wt, bias, relu=True, out=out)

            def base():
                torch.relu_(F.conv2d(x, wt, bias, padding=2, dilation=2))
            d_ms, p_ms, b_ms = event_blocks([dilated, plain, base], a.seconds)
            dilated()
            diff = float((out - torch.relu_(F.conv2d(x, wt, bias, padding=2, dilation=2))).abs().max())
            md, mp, mb = (statistics.median(v) for v in (d_ms, p_ms, b_ms))
            entry = dict(Cin=cin, Cout=cout, H=size, W=size, gflop=flop / 1e9, dilated=stats(d_ms), dilation_1=stats(p_ms),
                         baseline=stats(b_ms), dilated_tflops=flop / md / 1e9, dilated_share_of_peak=flop / md / 1e9 / PEAK_TF,
                         dilation_1_tflops=flop / mp / 1e9, baseline_tflops=flop / mb / 1e9,
                         ratio_dilated_over_dilation_1=md / mp, ratio_dilated_over_baseline=md / mb,
                         dilated_spread=spread(d_ms), dilation_1_spread=spread(p_ms), max_abs_difference=diff)
            result["convs"].append(entry)
            print(json.dumps(entry), flush=True)
            if tiles:
                want = out.clone()
                order = sorted(tiles)
                fns = [dilated] + [(lambda f=tiles[n]: f(x, wt, bias, out)) for n in order]
                blocks = event_blocks(fns, a.seconds)
                same = {}
                for n in order:  # (the choice changes no value)
                    out.zero_()
                    tiles[n](x, wt, bias, out)
                    same[n] = bool(torch.equal(out, want))
                entry = dict(Cin=cin, Cout=cout, H=size, W=size, in_use=stats(blocks[0]),
                             candidates={str(n): dict(stats(ms), spread=spread(ms), tflops=flop / statistics.median(ms) / 1e9,
                                                      same_bits=same[n]) for n, ms in zip(order, blocks[1:])})
                result["tiles"].append(entry)
                print(json.dumps(entry), flush=True)
            del x, wt, bias, out

        cur = torch.randn((1, 512, 255, 255), generator=g).to(dev)
        prev = torch.randn((1, 512, 127, 127), generator=g).to(dev)
        out = torch.empty_like(cur)
        o_ms, b_ms = event_blocks([lambda: fmpnp.dense_pyramid_step(cur, prev, out=out), lambda: F.normalize(
            cur + F.interpolate(prev, size=(255, 255), mode="bilinear", align_corners=True), dim=1)], a.seconds)
        traffic = 4.0 * (2 * cur.numel() + prev.numel())  # cur read, out written, prev read: once each, at least
        result["step"] = dict(C=512, size=[255, 255], prev=[127, 127], ours=stats(o_ms), baseline=stats(b_ms),
                              ratio_ours_over_baseline=statistics.median(o_ms) / statistics.median(b_ms),
                              ours_spread=spread(o_ms), ours_gbytes_per_s=traffic / statistics.median(o_ms) / 1e6,
                              max_abs_difference=float((fmpnp.dense_pyramid_step(cur, prev) - F.normalize(
                                  cur + F.interpolate(prev, size=(255, 255), mode="bilinear", align_corners=True),
                                  dim=1)).abs().max()))
        print(json.dumps(result["step"]), flush=True)
        del cur, prev, out
        x = torch.randn((1, 256, 256, 256), generator=g).to(dev)
        out = torch.empty((1, 256, 255, 255), device=dev)
        o_ms, b_ms = event_blocks([lambda: fmpnp.avgpool2x2s1(x, out=out), lambda: F.avg_pool2d(x, 2, 1)], a.seconds)
        result["pool"] = dict(shape=[1, 256, 256, 256], ours=stats(o_ms), baseline=stats(b_ms),
                              ratio_ours_over_baseline=statistics.median(o_ms) / statistics.median(b_ms),
                              ours_gbytes_per_s=4.0 * (x.numel() + out.numel()) / statistics.median(o_ms) / 1e6,
                              equals_the_frameworks=bool(torch.equal(fmpnp.avgpool2x2s1(x), F.avg_pool2d(x, 2, 1))))
        print(json.dumps(result["pool"]), flush=True)
        del x, out

        if not a.skip_walks:
            torch.manual_seed(2)
            trunk = fmpnp.d2net_trunk().to(dev)
            image = torch.randn((1, 3, 1024, 1024), generator=g).to(dev)
            for scales in ((1,), fmpnp.dense.MULTISCALE):
                hip = fmpnp.DenseFeatureExtractor(trunk, scales=scales)
                tor = fmpnp.DenseFeatureExtractor(trunk, scales=scales, backend="torch")
                peak = {}
                for name, ext in (("ours", hip), ("baseline", tor)):
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    torch.cuda.reset_peak_memory_stats()
                    got = ext.extract(image)
                    torch.cuda.synchronize()
                    peak[name] = torch.cuda.max_memory_allocated() / 2 ** 20
                    shape = list(got.shape)
                diff = float((hip.extract(image) - tor.extract(image)).abs().max())
                o_ms, b_ms = host_blocks([lambda: hip.extract(image), lambda: tor.extract(image)], a.seconds, rounds=3)
                entry = dict(image=1024, scales=list(scales), map=shape, ours=stats(o_ms), baseline=stats(b_ms),
                             ratio_ours_over_baseline=statistics.median(o_ms) / statistics.median(b_ms),
                             ours_spread=spread(o_ms), peak_mbytes=peak, max_abs_difference=diff)
                result["walks"].append(entry)
                print(json.dumps(entry), flush=True)
                torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
