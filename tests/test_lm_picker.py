"""The LM kernel picker (csrc/fmpnp_lm_impl.h lm_pick, through lm_kernel_ptr) against its record.

build/test_lm_picker (csrc/test_lm_picker.hip, no device needed) asks lm_kernel_ptr for every storage type x
build x team x ratio x variant code and prints the symbol of the kernel it hands back, or null.  The record
tests/golden/lm_picker.txt is that listing as the hand-written per-type ladders gave it before the variant table
(fmpnp_internal.h VAR_TABLE, lm_built) replaced them.  Comparing line by line pins the set of kernels that is
built (58 fp32, 46 fp64, 36 fp16), the kernel each argument tuple maps to -- a wrong but valid kernel computes the
same results and no other test sees it -- and the mangled names that bench.py and the profiles refer to."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "featuremetric-pnp_amd")


def test_picker_hands_back_the_recorded_kernels():
    subprocess.run(["make", "-s", "-C", PKG, "build/test_lm_picker"], check=True, timeout=1200)
    r = subprocess.run([os.path.join(PKG, "build", "test_lm_picker")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout.splitlines()
    with open(os.path.join(ROOT, "tests", "golden", "lm_picker.txt")) as f:
        want = f.read().splitlines()
    assert len(want) == 3 * (2 * 2 + 2 * 2 + 2) * 18  # dtype x (wide, latency: team x ratio; throughput: ratio) x code
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    built = [w.split() for w in want if not w.endswith(" null")]
    assert {d: sum(1 for b in built if b[0] == d) for d in ("f32", "f64", "f16")} == {"f32": 58, "f64": 46, "f16": 36}
