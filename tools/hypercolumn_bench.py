"""Hypercolumn assembly at the RobotCar shape: libfmpnp's fused kernel against the reference's sequence
restated in PyTorch-ROCm on the same GPU, interleaved in one process.

    python tools/hypercolumn_bench.py [--out profiles/hypercolumn_bench.json] [--batches 1 4]

Shape: layers 128@256x256, 256@128x128, 256@64x64, 512@64x64, 512@32x32 -> 1664@256x256, B = 1 and 4.
  ours      fmpnp.assemble_hypercolumn into a preallocated output (one kernel), with the library's choice of
            stores (4-byte) and, for the record, with the 16-byte ones (the same results).
  baseline  network.py:154-173 restated: zeros, per layer interpolate(bilinear, align_corners=True) and the
            slice write, torch.norm(p=2, dim=1), the divide (the caching allocator is warm).
Each variant is timed by device events around a block of calls, in alternating blocks after warming all; the
median block is reported with min and max.  The floor is the bytes the work cannot avoid -- the output written
once plus every source read once -- at the 6.3 TB/s the microbenchmarks reach on this GPU.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "featuremetric-pnp_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import fmpnp  # noqa: E402
from fmpnp import _lib  # noqa: E402

LAYERS = [(128, 256, 256), (256, 128, 128), (256, 64, 64), (512, 64, 64), (512, 32, 32)]
ACHIEVABLE_TBS = 6.3


def baseline(maps):
    b, _, h, w = maps[0].shape
    hyper = torch.zeros(b, sum(m.shape[1] for m in maps), h, w, device=maps[0].device)
    at = 0
    for m in maps:
        hyper[:, at:at + m.shape[1]] = F.interpolate(m, size=(h, w), mode="bilinear", align_corners=True)
        at += m.shape[1]
    return hyper / torch.norm(hyper, p=2, dim=1, keepdim=True)


def blocks(fns, reps, rounds=7):
    """Alternating device-event-timed blocks of each function; per function the list of ms per call."""
    for f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                f()
            e.record()
            e.synchronize()
            out[i].append(s.elapsed_time(e) / reps)
    return out


def stats(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 4])
    ap.add_argument("--reps", type=int, default=20, help="calls per timed block")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.require_device(dev)
    result = dict(device=torch.cuda.get_device_name(0), library_digest=_lib.library_digest(), layers=LAYERS,
                  achievable_tb_per_s=ACHIEVABLE_TBS, shapes=[])
    g = torch.Generator(device="cpu").manual_seed(1)
    for b in a.batches:
        maps = [torch.randn((b, c, h, w), generator=g).relu_().to(dev) for c, h, w in LAYERS]
        channels = sum(c for c, _, _ in LAYERS)
        out = torch.empty((b, channels, 256, 256), dtype=torch.float32, device=dev)
        out_bytes = out.numel() * 4
        src_bytes = sum(m.numel() for m in maps) * 4
        floor_ms = (out_bytes + src_bytes) / (ACHIEVABLE_TBS * 1e12) * 1e3
        ours, vector, base = blocks([lambda: fmpnp.assemble_hypercolumn(maps, out=out),
                                     lambda: fmpnp.assemble_hypercolumn(maps, out=out, stores="vector"),
                                     lambda: baseline(maps)], a.reps)
        got = fmpnp.assemble_hypercolumn(maps, out=out)
        want = baseline(maps)
        diff = float((got - want).abs().max())
        same = bool(torch.equal(got, fmpnp.assemble_hypercolumn(maps, stores="vector")))
        del want
        med = statistics.median(ours)
        entry = dict(B=b, output_bytes=out_bytes, source_bytes=src_bytes, floor_ms=floor_ms, ours=stats(ours),
                     ours_vector_stores=stats(vector), baseline=stats(base),
                     ratio_baseline_over_ours=statistics.median(base) / med,
                     achieved_tb_per_s=(out_bytes + src_bytes) / med / 1e9,
                     share_of_floor=floor_ms / med, max_abs_diff_to_baseline=diff, store_widths_agree=same)
        result["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        del maps, out, got
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
