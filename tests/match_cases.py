"""Shared inputs of the dense-matching tests (test_match_cpu.py, test_gpu_match.py): the goldens of
tests/golden/gen_golden_match.py, seeded operands for the shapes the kernels can go wrong at, and an
independent numpy statement of the row reduction's contract."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EDGE_CASES = ["nan", "inf", "tie", "top1", "topall"]
RATIO = 0.9

# (N, C, W, H): one element; ragged tiles on all three axes of the 128 x 128 x 32 block with a
# non-square map; more than one tile per axis; the production chain length in k
SHAPES = [(1, 1, 1, 1), (37, 40, 24, 20), (129, 33, 33, 40), (64, 1664, 64, 64)]


@functools.lru_cache(maxsize=None)
def golden(name):
    with np.load(os.path.join(GOLDEN, f"match_{name}.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def top_ks(wh):
    """1, 2, the two bound factors' int(factor * WH) and WH, where they are valid for this map."""
    return sorted({k for k in (1, 2, int(0.006 * wh), int(0.12 * wh), wh) if 1 <= k <= wh})


@functools.lru_cache(maxsize=None)
def operands(n, c, w, h, kind="normal"):
    """Seeded fp32 (sparse [n, c], dense [c, w * h]).  kind "normal": Gaussians, with sparse row 0 zero
    where there is more than one row (a row of one repeated score).  kind "ints": small integers with
    many zeros and both signs, so that scores are exact, heavily duplicated, and include +0, -0
    products and negative values."""
    rng = np.random.default_rng(1000 * n + 10 * c + w)
    if kind == "ints":
        sparse = rng.integers(-2, 3, (n, c)).astype(np.float32)
        dense = rng.integers(-2, 3, (c, w * h)).astype(np.float32)
        dense[:, ::7] = -0.0
    else:
        sparse = rng.standard_normal((n, c)).astype(np.float32)
        dense = rng.standard_normal((c, w * h)).astype(np.float32)
        if n > 1:
            sparse[0] = 0.0
    sparse.setflags(write=False)
    dense.setflags(write=False)
    return sparse, dense


def padded(a, pad):
    """A view of a with `pad` unused fp32 columns after every row (filled with NaN: never read)."""
    buf = np.full((a.shape[0], a.shape[1] + pad), np.nan, np.float32)
    buf[:, :a.shape[1]] = a
    return buf[:, :a.shape[1]]


def reduce_rows(scores, top_k, ratio=RATIO):
    """The row reduction's contract stated independently in numpy, on given fp32 scores: NaN above
    everything, -0 as +0, the lowest index among equal maxima, the exact top_k-th largest value, one
    fp32 product in the mask."""
    s = np.asarray(scores, np.float32) + np.float32(0)  # (-0 -> +0)
    nan = np.isnan(s)
    # fp64 ranks: finite scores as they are, +Inf above them (1e300), every NaN above that
    rank = np.where(nan, np.inf, np.where(s == np.inf, 1e300, s.astype(np.float64)))
    argmax = np.argmax(rank, axis=1).astype(np.int32)   # first occurrence
    srt = -np.sort(-rank, axis=1)

    def back(v):
        with np.errstate(over="ignore"):
            return np.where(np.isinf(v) & (v > 0), np.nan, np.where(v == 1e300, np.inf, v)).astype(np.float32)
    top, kth = back(srt[:, 0]), back(srt[:, top_k - 1])
    r2 = np.float32(ratio * ratio)
    with np.errstate(invalid="ignore"):
        mask = (r2 * top.astype(np.float32)).astype(np.float32) >= kth
    return argmax, top.astype(np.float32), kth.astype(np.float32), mask


def same_floats(a, b):
    """Equal under == with NaNs at the same positions."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool(np.all((a == b) | np.isnan(a)))


def assert_same_result(got, want, what=""):
    assert np.array_equal(got["argmax"], want["argmax"]), what
    assert same_floats(got["top"], want["top"]), what
    assert same_floats(got["kth"], want["kth"]), what
    assert np.array_equal(got["mask"], want["mask"]), what


@functools.lru_cache(maxsize=None)
def twin(n, c, w, h, top_k, kind="normal"):
    """The CPU twin's result on operands(...), computed once and shared (scores only at the first top_k)."""
    import fmpnp
    sparse, dense = operands(n, c, w, h, kind)
    return fmpnp.exhaustive_match_cpu(sparse, dense, top_k, RATIO, scores=(top_k == top_ks(w * h)[0]))
