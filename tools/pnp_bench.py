"""P3P RANSAC + polish at the RobotCar shape: time per synchronous call and per asynchronous launch
sequence, the arithmetic floor of the point tests, and the CPU twin on 16 threads as context.

    python tools/pnp_bench.py [--out profiles/pnp_bench.json] [--seconds 0.6]

Shapes (iters = 5000, threshold 12 px, 60 % outliers, 1 px noise): B = 10 problems of M = 866 points (the
top_N = 10 references of one query), B = 10 of M = 295, B = 1 of M = 866.
  sync    fmpnp_pnp_ransac on host descriptors and points: upload, two kernels, results and mask copied
          back, the stream waited for -- a host clock around the C call, median of five blocks.
  async   fmpnp_pnp_ransac_async on device buffers, by device events around back-to-back launch sequences.
  twin    fmpnp_pnp_ransac_cpu on 16 threads, a host clock (context, not a yardstick).
  floor   the hypothesis kernel tests B x iters x M points; one test without distortion is 29 fp64 VALU
          operations (18 for R X + t, 2 for x / z and y / z, 6 for the pixel residual, 3 for its square) and
          one division (counted as 10 issue slots: 2 div_scale, rcp, 5 fma, div_fmas, div_fixup): 39 slots.
          The fp64 vector peak is 78.6 TFLOP/s with an fma counted as two, so 39.3 T slots/s.
There is no baseline to time: cv2 is not importable here and the parent commit has no such stage.
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
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fmpnp import _lib, pnp  # noqa: E402

ITERS, THRESHOLD = 5000, 12.0
SLOTS_PER_TEST, PEAK_FP64_TFLOPS = 39, 78.6
FACADE_CALL_MS = {"robotcar_N295": 1.28, "robotcar_N866": 1.80}  # DESIGN.md 6.-1, the refiner per query


def planted(M, seed, fo=0.6, sigma=1.0, f=400.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    K = np.array([[f, 0.0, 512.0], [0.0, f, 512.0], [0.0, 0.0, 1.0]])
    w = rng.normal(0.0, 0.3, 3)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    t = rng.normal(0.0, 1.0, 3)
    xn = rng.uniform(-472.0 / f, 472.0 / f, (M, 2))
    z = rng.uniform(5.0, 50.0, M)
    X = (np.concatenate([xn * z[:, None], z[:, None]], 1) - t) @ R
    x = xn * f + 512.0 + np.clip(rng.normal(0.0, sigma, (M, 2)), -3.0, 3.0)
    out = rng.uniform(size=M) < fo
    ang, mag = rng.uniform(0.0, 2 * np.pi, M), rng.uniform(40.0, 300.0, M)
    x = np.where(out[:, None], x + np.stack([np.cos(ang), np.sin(ang)], 1) * mag[:, None], x)
    return dict(points3d=X, points2d=x, K=K, dist=np.zeros(4), threshold=THRESHOLD, iters=ITERS, seed=0), int((~out).sum())


def host_blocks(fn, seconds):
    for _ in range(3):
        fn()
    t = time.perf_counter()
    fn()
    per = max(2, int(seconds / 5 / max(time.perf_counter() - t, 1e-5)))
    ms = []
    for _ in range(5):
        t = time.perf_counter()
        for _ in range(per):
            fn()
        ms.append((time.perf_counter() - t) * 1e3 / per)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), calls_per_block=per)


def events_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / reps)
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), launches_per_block=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.6, help="timed work per variant and shape, about")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.require_device(dev)
    L, st = _lib.load(), _lib.stream_ptr(dev)
    result = dict(device=torch.cuda.get_device_name(0), library_digest=_lib.library_digest(), iters=ITERS,
                  threshold=THRESHOLD, slots_per_point_test=SLOTS_PER_TEST, peak_fp64_vector_tflops=PEAK_FP64_TFLOPS,
                  facade_call_ms=FACADE_CALL_MS, date=time.strftime("%Y-%m-%d"), shapes=[])
    for B, M in ((10, 866), (10, 295), (1, 866)):
        made = [planted(M, 100 * M + i) for i in range(B)]
        probs, counts = [m[0] for m in made], [m[1] for m in made]
        arr, keep, total = pnp.make_problems(probs)
        res, mask = (_lib.PnpResult * B)(), np.zeros(total, np.uint8)

        def sync():
            _lib.check(L.fmpnp_pnp_ransac(arr, B, 0, res, mask.ctypes.data, total, st), "fmpnp_pnp_ransac")

        def twin():
            _lib.check(L.fmpnp_pnp_ransac_cpu(arr, B, res, mask.ctypes.data, total, 16), "fmpnp_pnp_ransac_cpu")
        sync_ms = host_blocks(sync, a.seconds)
        found = [res[i].num_inliers for i in range(B)]
        call = pnp.AsyncRansac(probs, dev)
        first = call.read()
        async_ms = events_ms(call.launch, max(3, int(a.seconds / 5 / max(sync_ms["median_ms"] * 1e-3, 1e-5))))
        twin_ms = host_blocks(twin, a.seconds)
        tests = B * ITERS * M
        floor_ms = tests * SLOTS_PER_TEST / (PEAK_FP64_TFLOPS / 2 * 1e12) * 1e3
        entry = dict(B=B, M=M, point_tests=tests, sync=sync_ms, async_sequence=async_ms, twin_16_threads=twin_ms,
                     arithmetic_floor_ms=floor_ms, async_over_floor=async_ms["median_ms"] / floor_ms,
                     planted_inliers=counts, found_inliers=found,
                     async_equals_sync=all(first[i]["num_inliers"] == found[i] for i in range(B)))
        result["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
