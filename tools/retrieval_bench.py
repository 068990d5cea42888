"""Retrieval at the production shape: libfmpnp's NetVLAD pooling and top-n ranking against PyTorch-ROCm on the
same GPU, interleaved in one process.

    python tools/retrieval_bench.py [--out profiles/retrieval_bench.json] [--batches 1 16 64]

Pooling: K = 64, C = 512, 64 x 64 positions (a 1024-pixel image through VGG-16's conv5), B = 1, 16 and 64.
  ours        fmpnp.netvlad_pool into a preallocated output (four kernels per round of images).
  reference   netvlad.py:45-70 as written: the Python loop over the 64 clusters (timed at B <= --ref-max-batch:
              it materialises a [B, 512, 4096] residual per cluster).
  vectorised  its restatement: normalize, bmm, softmax, bmm, the centroid term, the two normalisations.
Ranking: R = 4096, Q = 512, D = 1024, n = 30.
  ours        fmpnp.rank_topn (the fmaf-chain correlation and one selection kernel).
  baseline    torch.mm and torch.topk.
Each variant is timed by device events around a block of calls, in alternating blocks after warming all; the
median block is reported with min and max.  Floors: the pooling's two K x C x P products (0.54 GFLOP per image)
at the 157.3 TFLOP/s of the fp32-input MFMA, and its input read once at the 6.3 TB/s the microbenchmarks reach;
the larger of the two bounds the kernel (the MFMA one: 3.4 us against 1.3 us per image).
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

K, C, H, W = 64, 512, 64, 64
MFMA_F32_TFLOPS = 157.3
ACHIEVABLE_TBS = 6.3


def reference_forward(x, weight, centroids):
    """netvlad.py:45-70 as written (normalize_input = True)."""
    n, c = x.shape[:2]
    k = weight.shape[0]
    x = F.normalize(x, p=2, dim=1)
    soft_assign = F.conv2d(x, weight).view(n, k, -1)
    soft_assign = F.softmax(soft_assign, dim=1)
    x_flatten = x.view(n, c, -1)
    vlad = torch.zeros([n, k, c], dtype=x.dtype, device=x.device)
    for i in range(k):
        residual = x_flatten.unsqueeze(0).permute(1, 0, 2, 3) - \
            centroids[i:i + 1, :].expand(x_flatten.size(-1), -1, -1).permute(1, 2, 0).unsqueeze(0)
        residual *= soft_assign[:, i:i + 1, :].unsqueeze(2)
        vlad[:, i:i + 1, :] = residual.sum(dim=-1)
    vlad = F.normalize(vlad, p=2, dim=2)
    vlad = vlad.view(x.size(0), -1)
    return F.normalize(vlad, p=2, dim=1)


def vectorised_forward(x, weight, centroids):
    xf = F.normalize(x, p=2, dim=1).flatten(2)
    w = weight.reshape(weight.shape[0], -1)
    a = F.softmax(torch.matmul(w, xf), dim=1)
    vlad = torch.bmm(a, xf.transpose(1, 2)) - a.sum(dim=-1, keepdim=True) * centroids
    vlad = F.normalize(vlad, p=2, dim=2).flatten(1)
    return F.normalize(vlad, p=2, dim=1)


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
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--reps", type=int, default=10, help="calls per timed block")
    ap.add_argument("--ref-max-batch", type=int, default=16, help="largest B at which the reference's loop is timed")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.require_device(dev)
    torch.backends.cuda.matmul.allow_tf32 = False
    result = dict(device=torch.cuda.get_device_name(0), library_digest=_lib.library_digest(), K=K, C=C, positions=H * W,
                  mfma_f32_tflops=MFMA_F32_TFLOPS, achievable_tb_per_s=ACHIEVABLE_TBS, pooling=[], ranking=None)
    g = torch.Generator(device="cpu").manual_seed(1)
    weight = (F.normalize(torch.randn(K, C, generator=g), dim=1) * 290.0).reshape(K, C, 1, 1).to(dev)
    centroids = torch.randn(K, C, generator=g).to(dev)
    for b in a.batches:
        x = (torch.randn((b, C, H, W), generator=g).clamp_min_(0.0) ** 3).to(dev)
        out = torch.empty((b, K * C), dtype=torch.float32, device=dev)
        flop = 2 * 2.0 * K * C * H * W * b
        floor_mfma_ms = flop / (MFMA_F32_TFLOPS * 1e12) * 1e3
        floor_bytes_ms = x.numel() * 4 / (ACHIEVABLE_TBS * 1e12) * 1e3
        fns = [lambda: fmpnp.netvlad_pool(x, weight, centroids, out=out), lambda: vectorised_forward(x, weight, centroids)]
        with_ref = b <= a.ref_max_batch
        if with_ref:
            fns.append(lambda: reference_forward(x, weight, centroids))
        with torch.no_grad():
            times = blocks(fns, a.reps if b < 64 else max(2, a.reps // 3))
            got = fmpnp.netvlad_pool(x, weight, centroids, out=out)
            diff = float((got - vectorised_forward(x, weight, centroids)).abs().max())
            peak = float(got.abs().max())
        med = statistics.median(times[0])
        entry = dict(B=b, flop=flop, input_bytes=x.numel() * 4, floor_mfma_ms=floor_mfma_ms, floor_bytes_ms=floor_bytes_ms,
                     ours=stats(times[0]), vectorised=stats(times[1]), reference=stats(times[2]) if with_ref else None,
                     ratio_vectorised_over_ours=statistics.median(times[1]) / med,
                     ratio_reference_over_ours=statistics.median(times[2]) / med if with_ref else None,
                     share_of_mfma_floor=floor_mfma_ms / med, share_of_byte_floor=floor_bytes_ms / med,
                     achieved_tflops=flop / med / 1e9, max_abs_diff_to_vectorised=diff, max_abs_value=peak)
        result["pooling"].append(entry)
        print(json.dumps(entry), flush=True)
        del x, out, got
        torch.cuda.empty_cache()

    r, q, d, n = 4096, 512, 1024, 30
    ref = F.normalize(torch.randn(r, d, generator=g), dim=1).to(dev)
    qry = F.normalize(torch.randn(q, d, generator=g), dim=1).to(dev)
    ours, base = blocks([lambda: fmpnp.rank_topn(ref, qry, n),
                         lambda: torch.topk(torch.mm(qry, ref.t()), n, dim=1)], a.reps)
    idx, _ = fmpnp.rank_topn(ref, qry, n)
    want = torch.topk(torch.mm(qry, ref.t()), n, dim=1).indices
    flop = 2.0 * r * q * d
    med = statistics.median(ours)
    result["ranking"] = dict(R=r, Q=q, D=d, n=n, flop=flop, ours=stats(ours), mm_topk=stats(base),
                             ratio_mm_topk_over_ours=statistics.median(base) / med,
                             floor_mfma_ms=flop / (MFMA_F32_TFLOPS * 1e12) * 1e3,
                             share_of_mfma_floor=flop / (MFMA_F32_TFLOPS * 1e12) * 1e3 / med,
                             share_of_ranks_equal_to_topk=float((idx.long() == want).float().mean()))
    print(json.dumps(result["ranking"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
