"""The SuperPoint network's forward pass: HipSuperPointNet (libfmpnp's own operators) in "f32" and "f16" against the
same SuperPointNet through PyTorch-ROCm (MIOpen), on the same tensors and the same GPU, interleaved in one process.

    python tools/superpoint_net_bench.py [--out profiles/superpoint_net_bench.json] [--seconds 0.5]

GPU machine only: without a gfx950 device it fails; nothing falls back.
Shapes: 1024 x 1024 at B = 1 and B = 4, 512 x 512 at B = 1 (random weights: the speed does not depend on them).
  f32       HipSuperPointNet(net)(x): ten conv3x3 + ReLU launches, three maxpool2x2, two conv1x1, one normalisation.
  f16       HipSuperPointNet(net, precision="f16")(x): the 3x3 layers on the fp16 matrix cores, the heads exact.
  baseline  net(x) under torch.no_grad(): the framework's choice of algorithms.  The speed yardstick, not a numeric
            one; the largest differences of semi and desc to it are reported.
Before anything is timed, "f32" on the device must equal the CPU twins at a 16 x 24 image bit for bit (an error
otherwise).  Every shape is warmed for every variant first.  The forward passes are timed by the host clock around
blocks of calls, each call ending in a stream wait, the blocks alternating f32, f16, baseline over the rounds; the
medians are reported with min..max.  Then per layer, for the twelve convolutions at their own shapes in that walk:
ours (conv3x3 / conv1x1 with bias, and the ReLU where the walk has one), the fp16 form for the 3x3 layers, and the
framework's conv2d (+ relu_), by device events in alternating blocks.  No pass or fail ratio is set.
"""
import argparse
import copy
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
from fmpnp.superpoint import SP_CONVS, SP_HEADS  # noqa: E402

SHAPES = [(1024, 1), (1024, 4), (512, 1)]  # (image side, B)
DIV = dict(conv1a=1, conv1b=1, conv2a=2, conv2b=2, conv3a=4, conv3b=4, conv4a=8, conv4b=8, convPa=8, convPb=8, convDa=8,
           convDb=8)  # the layer's map is the image over this


def stats(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def host_blocks(fns, seconds, rounds=5):
    """Alternating host-clock blocks; every call ends in a wait for the stream.  Per function the ms per call."""
    def call(f):
        f()
        torch.cuda.current_stream().synchronize()
    per = []
    for f in fns:
        t = time.perf_counter()
        call(f)
        per.append(max(1, min(50, int(seconds / rounds / max(time.perf_counter() - t, 1e-5)))))
    out = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            t = time.perf_counter()
            for _ in range(per[i]):
                call(f)
            out[i].append((time.perf_counter() - t) * 1e3 / per[i])
    return out


def events_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def event_blocks(fns, seconds, rounds=5):
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


def check_twin(net_cpu, dev):
    x = torch.rand((1, 1, 16, 24), generator=torch.Generator().manual_seed(3))
    want = fmpnp.HipSuperPointNet(net_cpu)(x)
    got = fmpnp.HipSuperPointNet(copy.deepcopy(net_cpu).to(dev))(x.to(dev))
    for g, w, name in zip(got, want, ("semi", "desc")):
        if not torch.equal(g.cpu(), w):
            raise SystemExit(f'superpoint_net_bench: "f32" {name} on the device differs from the CPU twins at 16 x 24')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "superpoint_net_bench.json"))
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per variant and shape, about")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.require_device(dev)  # (an error without a gfx950 device: nothing falls back)
    torch.manual_seed(2)
    net_cpu = fmpnp.SuperPointNet().eval()
    check_twin(net_cpu, dev)
    net = net_cpu.to(dev)
    hip32, hip16 = fmpnp.HipSuperPointNet(net), fmpnp.HipSuperPointNet(net, precision="f16")
    result = dict(device=torch.cuda.get_device_name(0), library_digest=_lib.library_digest(),
                  f32_equals_twin_at_16x24=True, forward=[], layers=[])
    g = torch.Generator().manual_seed(1)
    images = {s: torch.rand((s[1], 1, s[0], s[0]), generator=g).to(dev) for s in SHAPES}
    with torch.no_grad():
        for s in SHAPES:  # every shape warmed for every variant before any is timed
            for f in (hip32, hip16, net):
                for _ in range(2):
                    f(images[s])
            torch.cuda.synchronize()
        for s in SHAPES:
            x = images[s]
            m32, m16, mb = host_blocks([lambda: hip32(x), lambda: hip16(x), lambda: net(x)], a.seconds)
            o32, o16, ob = hip32(x), hip16(x), net(x)
            entry = dict(image=s[0], B=s[1], f32=stats(m32), f16=stats(m16), baseline=stats(mb),
                         ratio_f32_over_baseline=statistics.median(m32) / statistics.median(mb),
                         ratio_f16_over_baseline=statistics.median(m16) / statistics.median(mb),
                         speedup_f32_over_f16=statistics.median(m32) / statistics.median(m16),
                         max_abs_semi_f32_to_baseline=float((o32[0] - ob[0]).abs().max()),
                         max_abs_desc_f32_to_baseline=float((o32[1] - ob[1]).abs().max()),
                         max_abs_semi_f16_to_baseline=float((o16[0] - ob[0]).abs().max()),
                         max_abs_desc_f16_to_baseline=float((o16[1] - ob[1]).abs().max()))
            result["forward"].append(entry)
            print(json.dumps(entry), flush=True)
            del o32, o16, ob
        for s in SHAPES:
            for name in SP_CONVS:
                m = getattr(net, name)
                head = name in SP_HEADS
                h = s[0] // DIV[name]
                cin, cout = m.in_channels, m.out_channels
                x = torch.rand((s[1], cin, h, h), generator=g).to(dev)
                w, b = m.weight.detach(), m.bias.detach()
                out = torch.empty((s[1], cout, h, h), device=dev)
                if head:
                    fns = [lambda: fmpnp.conv1x1(x, w, b, out=out), lambda: torch.nn.functional.conv2d(x, w, b)]
                else:
                    image = fmpnp.conv3x3_f16_weights(w)
                    fns = [lambda: fmpnp.conv3x3(x, w, b, relu=True, out=out),
                           lambda: torch.relu_(torch.nn.functional.conv2d(x, w, b, padding=1)),
                           lambda: fmpnp.conv3x3(x, image, b, relu=True, out=out, precision="f16")]
                ms = event_blocks(fns, a.seconds / 2)
                flop = 2.0 * (1 if head else 9) * cin * cout * s[1] * h * h
                entry = dict(image=s[0], B=s[1], layer=name, Cin=cin, Cout=cout, H=h, W=h, gflop=flop / 1e9,
                             ours=stats(ms[0]), baseline=stats(ms[1]), f16=None if head else stats(ms[2]),
                             ours_tflops=flop / statistics.median(ms[0]) / 1e9,
                             ratio_ours_over_baseline=statistics.median(ms[0]) / statistics.median(ms[1]))
                result["layers"].append(entry)
                print(json.dumps(entry), flush=True)
                del x, out
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
