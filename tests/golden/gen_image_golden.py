#!/usr/bin/env python3
"""Generate tests/golden/image_lanczos.npz: Pillow's own Lanczos results for the image front end's cases.

TEST INFRASTRUCTURE ONLY.  It imports Pillow and tests/image_cases.py and nothing else of the project: for every
(shape, kind) of image_cases.CASES it builds the seeded input, runs Image.fromarray(input).resize((w, h), Image.LANCZOS)
of the installed Pillow and records the output with the input's CRC-32 (the tests rebuild the inputs from the seeds and
check the CRC; with the inputs the file would pass its 256 KB).  The Pillow version is recorded too.  No test imports
this file, and the GPU tier needs no Pillow: it reads the fixture.

Run:  python tests/golden/gen_image_golden.py
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import image_cases as ic  # noqa: E402


def main():
    data = {"pillow_version": np.array(PIL.__version__)}
    for shape, kind in ic.CASES:
        h_in, w_in, h, w = shape
        a = ic.make_input((h_in, w_in), kind)
        out = np.asarray(Image.fromarray(a).resize((w, h), Image.LANCZOS))
        assert out.shape == (h, w, 3) and out.dtype == np.uint8
        k = ic.key(shape, kind)
        data["out_" + k] = out
        data["crc_" + k] = np.array(ic.crc(a), dtype=np.uint32)
    np.savez_compressed(ic.GOLDEN, **data)
    size = os.path.getsize(ic.GOLDEN)
    assert size < 256 * 1024, size
    print(f"{ic.GOLDEN}: {len(ic.CASES)} cases, Pillow {PIL.__version__}, {size} bytes")


if __name__ == "__main__":
    main()
