"""Shared inputs and bounds of the fp16 match precision's tests (test_match_f16_cpu.py,
test_gpu_match_f16.py): the "normal" operands of match_cases.py with the fp16-subnormal range taken out, the
f16 CPU reference on them, the exact fp64 product, and the two per-score bounds of include/fmpnp.h."""
import functools

import numpy as np

import match_cases as mc

TINY = 2.0 ** -14  # the smallest normal fp16 magnitude


@functools.lru_cache(maxsize=None)
def operands(n, c, w, h):
    """mc.operands(..., "normal") with every element of magnitude below 2^-14 set to 0: whether the matrix
    instruction keeps or flushes an fp16-subnormal operand is unspecified, so both sides of a real-valued
    comparison see operands that have none.  (None rounds INTO the subnormal range either: the smallest
    magnitude kept is 2^-14, which fp16 holds exactly.)"""
    sparse, dense = (a.copy() for a in mc.operands(n, c, w, h, "normal"))
    sparse[np.abs(sparse) < TINY] = 0.0
    dense[np.abs(dense) < TINY] = 0.0
    sparse.setflags(write=False)
    dense.setflags(write=False)
    return sparse, dense


def zeroed(n, c, w, h):
    """How many elements of magnitude below 2^-14 operands() set to zero (sparse row 0, zero already, included)."""
    s0, d0 = mc.operands(n, c, w, h, "normal")
    return int((np.abs(s0) < TINY).sum() + (np.abs(d0) < TINY).sum())


@functools.lru_cache(maxsize=None)
def reference(n, c, w, h):
    """The f16 CPU reference's result on operands(), with scores, at the first top_k; computed once."""
    import fmpnp
    sparse, dense = operands(n, c, w, h)
    res = fmpnp.exhaustive_match_cpu(sparse, dense, mc.top_ks(w * h)[0], mc.RATIO, scores=True, precision="f16")
    res["scores"].setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def exact(n, c, w, h):
    """(s, sum_k |a| |b|) in fp64 from the fp32 operands()."""
    sparse, dense = (a.astype(np.float64) for a in operands(n, c, w, h))
    return sparse @ dense, np.abs(sparse) @ np.abs(dense)


@functools.lru_cache(maxsize=None)
def rounded(n, c, w, h):
    """(s16, sum_k |fl16(a)| |fl16(b)|) in fp64 from numpy's own binary16 rounding of operands()."""
    sparse, dense = (a.astype(np.float16).astype(np.float64) for a in operands(n, c, w, h))
    return sparse @ dense, np.abs(sparse) @ np.abs(dense)


def rounding_bound(n, c, w, h):
    """|s16 - s| per score: each operand's relative error 2^-11 (2 * 2^-11 + 2^-22 on a product), and the final
    rounding to fp32."""
    s, mag = exact(n, c, w, h)
    return (2.0 ** -10 + 2.0 ** -22) * mag + 2.0 ** -24 * np.abs(s)


def accumulation_bound(n, c, w, h):
    """|s_gpu - s_ref| per score: C * 2^-23 * sum_k |fl16(a)| |fl16(b)|, twice the any-order fp32 summation bound
    (C - 1) * 2^-24 * sum, which leaves room for an internal rounding that is not to-nearest; plus the
    reference's own final rounding."""
    ref = reference(n, c, w, h)["scores"].astype(np.float64)
    return c * 2.0 ** -23 * rounded(n, c, w, h)[1] + 2.0 ** -24 * np.abs(ref)
