"""The image front end against the host path it replaces, interleaved in one process (tools/dense_bench.py's method:
alternating blocks after warming each, the median block with min and max).  No pass or fail ratio is set.

    python tools/image_bench.py [--out profiles/image_bench.json] [--seconds 0.3]

Both paths start at decoded uint8 pixels in host memory (decoding a file is PIL's in both) and end with the float32
[B, 3, h, w] tensor on the device:
  host      Pillow's thumbnail with Image.LANCZOS where the shape asks for a resize, numpy's ToTensor + Normalize
            (fmpnp.d2net_preprocess(..., "torch")), then the upload of the floats: 12 bytes per output pixel over PCIe.
  ours      the upload of the bytes, 3 per source pixel, then fmpnp.image_to_tensor: one launch without a resize, two
            with one.
Per shape and batch: the kernels alone (device events, the bytes already on the device), both paths end to end (the host
clock around calls that end in a device synchronise), the bytes over PCIe, and the kernels' share of the HBM peak counting
every byte once (source read, intermediate written and read, floats written).
Shapes: 1024 x 1024 (RobotCar) and 768 x 1024 (CMU) without a resize, 1080 x 1920 -> thumbnail 1024 (576 x 1024); B = 1, 8.
The two passes of the resize are also timed alone at the last shape: what a single fused launch could save is bounded by
the intermediate's traffic and one kernel boundary.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "featuremetric-pnp_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fmpnp  # noqa: E402
from fmpnp import _lib  # noqa: E402

from encoder_bench import event_blocks, host_blocks, spread, stats  # noqa: E402

HBM_PEAK_GBS = 8000.0
SHAPES = [("robotcar", 1024, 1024, None), ("cmu", 768, 1024, None), ("full_hd", 1080, 1920, 1024)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.3, help="timed work per variant and shape, about")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.require_device(dev)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    result = dict(device=torch.cuda.get_device_name(0), library_digest=_lib.library_digest(), hbm_peak_gbytes_per_s=HBM_PEAK_GBS,
                  pillow=None if Image is None else __import__("PIL").__version__, shapes=[], passes=[])
    rng = np.random.RandomState(1)
    for name, h_in, w_in, image_size in SHAPES:
        if image_size is None:
            h, w = h_in, w_in
        else:
            w, h = fmpnp.thumbnail_size(w_in, h_in, image_size)
        for batch in (1, 8):
            u8 = rng.randint(0, 256, (batch, h_in, w_in, 3)).astype(np.uint8)
            on_dev = torch.from_numpy(u8).to(dev)
            out = torch.empty((batch, 3, h, w), device=dev)

            def kernels():
                fmpnp.image_to_tensor(on_dev, (h, w), out=out)

            def ours():
                fmpnp.image_to_tensor(torch.from_numpy(u8).to(dev), (h, w), out=out)

            def host():
                planes = []
                for b in range(batch):
                    img = u8[b]
                    if image_size is not None:
                        im = Image.fromarray(img)
                        im.thumbnail((image_size, image_size), Image.LANCZOS)
                        img = np.asarray(im)
                    planes.append(fmpnp.d2net_preprocess(img, "torch"))
                return torch.from_numpy(np.stack(planes)).to(dev)
            k_ms, = event_blocks([kernels], a.seconds)
            fns = [ours] + ([host] if Image is not None else [])
            e2e = host_blocks(fns, a.seconds)
            mid = 2 * batch * h_in * w * 3 if (w != w_in and h != h_in) else 0  # (written once, read once)
            traffic = batch * (3 * h_in * w_in + 12 * h * w) + mid
            mk = statistics.median(k_ms)
            entry = dict(name=name, B=batch, source=[h_in, w_in], output=[h, w], launches=1 if (h, w) == (h_in, w_in) else 2,
                         kernels=stats(k_ms), kernels_spread=spread(k_ms), kernel_bytes=traffic,
                         kernels_gbytes_per_s=traffic / mk / 1e6, kernels_share_of_hbm_peak=traffic / mk / 1e6 / HBM_PEAK_GBS,
                         ours_end_to_end=stats(e2e[0]), ours_pcie_bytes=int(u8.nbytes),
                         host_end_to_end=stats(e2e[1]) if Image is not None else None, host_pcie_bytes=12 * batch * h * w,
                         ratio_ours_over_host=(statistics.median(e2e[0]) / statistics.median(e2e[1])) if Image is not None else None)
            if Image is not None and image_size is None:  # (without a resize the two paths agree bit for bit)
                entry["equals_host_path"] = bool(torch.equal(out, host()))
            result["shapes"].append(entry)
            print(json.dumps(entry), flush=True)
            del on_dev, out
    # the resize's passes alone, 1080 x 1920 -> 576 x 1024, B = 1
    u8 = torch.from_numpy(rng.randint(0, 256, (1, 1080, 1920, 3)).astype(np.uint8)).to(dev)
    mid = fmpnp.resize_lanczos(u8, (1080, 1024))
    o_h, o_v, o_b = (torch.empty(s, dtype=torch.uint8, device=dev) for s in ((1, 1080, 1024, 3), (1, 576, 1024, 3), (1, 576, 1024, 3)))
    o_f = torch.empty((1, 3, 576, 1024), device=dev)
    h_ms, v_ms, b_ms, f_ms, t_ms = event_blocks([
        lambda: fmpnp.resize_lanczos(u8, (1080, 1024), out=o_h), lambda: fmpnp.resize_lanczos(mid, (576, 1024), out=o_v),
        lambda: fmpnp.resize_lanczos(u8, (576, 1024), out=o_b), lambda: fmpnp.image_to_tensor(u8, (576, 1024), out=o_f),
        lambda: fmpnp.image_to_tensor(o_b, out=o_f)], a.seconds)
    result["passes"] = dict(horizontal_only=stats(h_ms), vertical_only=stats(v_ms), both_uint8=stats(b_ms), both_float=stats(f_ms),
                            transform_only_576x1024=stats(t_ms), intermediate_bytes=1080 * 1024 * 3)
    print(json.dumps(result["passes"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
