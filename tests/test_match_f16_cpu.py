"""The fp16 precision of the match stage without a GPU: its CPU reference (fmpnp_exhaustive_match_ex_cpu with
FMPNP_MATCH_F16: operands rounded to binary16, fp64 accumulation, one rounding to fp32) against the exact twin
on integers, against numpy on real values and against the rounding bound of include/fmpnp.h, and the precision
argument of every new entry point."""
import ctypes

import numpy as np
import pytest

import fmpnp
from fmpnp import _lib, match

import match_cases as mc
import match_f16_cases as fc


@pytest.mark.parametrize("shape", mc.SHAPES, ids=str)
def test_reference_on_integers_equals_the_exact_twin(shape):
    """Integers in [-2, 2] are exact in fp16 and every partial sum is an integer of magnitude <= 4 * 1664:
    whatever the precision, the scores and the four outputs are the exact twin's, at every top_k."""
    n, c, w, h = shape
    sparse, dense = mc.operands(n, c, w, h, "ints")
    for i, top_k in enumerate(mc.top_ks(w * h)):
        want = mc.twin(n, c, w, h, top_k, "ints")
        got = fmpnp.exhaustive_match_cpu(sparse, dense, top_k, mc.RATIO, scores=(i == 0), precision="f16")
        mc.assert_same_result(got, want, (shape, top_k))
        if i == 0:
            assert mc.same_floats(got["scores"], want["scores"]), shape


def test_the_operands_without_fp16_subnormals():
    assert [fc.zeroed(*s) for s in mc.SHAPES] == [0, 40, 36, 1998]
    for s in mc.SHAPES:
        for a in fc.operands(*s):
            assert not ((a != 0) & (np.abs(a) < fc.TINY)).any()
            a16 = np.abs(a.astype(np.float16).astype(np.float32))
            assert not ((a16 != 0) & (a16 < fc.TINY)).any() and np.isfinite(a16).all()


@pytest.mark.parametrize("shape", mc.SHAPES, ids=str)
def test_reference_on_real_values_equals_numpy_within_one_ulp(shape):
    """numpy rounds the operands to binary16 itself and sums in fp64 in BLAS's order: that order matters only
    on an fp32 rounding boundary, so the two agree to one fp32 ulp."""
    got = fc.reference(*shape)["scores"]
    want = fc.rounded(*shape)[0].astype(np.float32)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    print(shape, "largest difference in ulp:", float((err / ulp).max()), "scores that differ:", int((err > 0).sum()))
    assert (err <= ulp).all()
    # the reduction is the contract's, on these scores
    for top_k in mc.top_ks(shape[2] * shape[3]):
        sparse, dense = fc.operands(*shape)
        res = fmpnp.exhaustive_match_cpu(sparse, dense, top_k, mc.RATIO, precision="f16")
        argmax, top, kth, mask = mc.reduce_rows(got, top_k)
        mc.assert_same_result(res, dict(argmax=argmax, top=top, kth=kth, mask=mask), (shape, top_k))


@pytest.mark.parametrize("shape", mc.SHAPES, ids=str)
def test_reference_is_within_the_rounding_bound_of_the_exact_product(shape):
    """|s16 - s| <= (2^-10 + 2^-22) sum_k |a| |b| + 2^-24 |s| per score, s the fp64 product of the fp32 operands."""
    got = fc.reference(*shape)["scores"].astype(np.float64)
    err, bound = np.abs(got - fc.exact(*shape)[0]), fc.rounding_bound(*shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        print(shape, "largest error / bound:", float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
    assert (err <= bound).all()
    if shape[1] > 1:
        assert err.max() > 0  # (the operands really are rounded)


def test_subnormal_and_non_finite_operands_of_the_reference():
    """fl16 by the book: ties to even, fp16 subnormals kept, 65520 and above -> Inf, NaN and Inf kept."""
    vals = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 2.0 ** -14 - 2.0 ** -25,
                     65504.0, 65519.99, 65520.0, 1e5, -1e5, np.inf, -np.inf, 3e-9, -2.0 ** -24], np.float32)
    with np.errstate(over="ignore"):
        want = vals.astype(np.float16).astype(np.float32)
    one = np.ones((1, 1), np.float32)
    for v, w in zip(vals, want):
        for a, b in ((np.full((1, 1), v, np.float32), one), (one, np.full((1, 1), v, np.float32))):
            got = fmpnp.exhaustive_match_cpu(a, b, 1, scores=True, precision="f16")["scores"][0, 0]
            assert got == w and np.signbit(got) == np.signbit(w), (v, got, w)
    got = fmpnp.exhaustive_match_cpu(np.full((1, 1), np.nan, np.float32), one, 1, scores=True, precision="f16")
    assert np.isnan(got["scores"][0, 0]) and np.isnan(got["top"][0])


def test_precision_argument():
    n, c, w, h = mc.SHAPES[1]
    sparse, dense = mc.operands(n, c, w, h)
    top_k = mc.top_ks(w * h)[2]
    want = mc.twin(n, c, w, h, mc.top_ks(w * h)[0])
    got = fmpnp.exhaustive_match_cpu(sparse, dense, mc.top_ks(w * h)[0], mc.RATIO, scores=True, precision="f32")
    mc.assert_same_result(got, want)
    assert got["scores"].tobytes() == want["scores"].tobytes()
    L = _lib.load()
    assert L.fmpnp_abi_version() == 4
    names = {"fmpnp_match_workspace_size_ex", "fmpnp_exhaustive_match_ex_async", "fmpnp_correlation_ex_async",
             "fmpnp_exhaustive_match_ex", "fmpnp_exhaustive_match_ex_cpu", "fmpnp_localize_ex"}
    assert names <= set(_lib.EXPORTS) and all(hasattr(L, name) for name in names)
    assert (_lib.MATCH_F32, _lib.MATCH_F16) == (0, 1)

    # the C entry point: F32 is the twin's bits, an unknown precision is FMPNP_EINVAL
    def ex_cpu(precision):
        out = dict(argmax=np.zeros(n, np.int32), top=np.zeros(n, np.float32), kth=np.zeros(n, np.float32),
                   mask=np.zeros(n, np.uint8))
        rc = L.fmpnp_exhaustive_match_ex_cpu(sparse.ctypes.data, n, c, dense.ctypes.data, c, w * h, w * h, top_k,
                                             mc.RATIO, out["argmax"].ctypes.data, out["top"].ctypes.data,
                                             out["kth"].ctypes.data, out["mask"].ctypes.data, None, 2, precision)
        out["mask"] = out["mask"].astype(bool)
        return rc, out
    rc, out = ex_cpu(_lib.MATCH_F32)
    assert rc == 0
    mc.assert_same_result(out, mc.twin(n, c, w, h, top_k))
    for bad in (2, -1, 16):
        assert ex_cpu(bad)[0] == _lib.EINVAL
    # the workspace: F32 is the old value; F16 adds the operand images; an unknown precision has none
    for (sn, sc, sw, sh) in mc.SHAPES + [(65, 2, 1 << 10, 1 << 10), (866, 1664, 256, 256)]:
        old = L.fmpnp_match_workspace_size(sn, sw * sh)
        assert L.fmpnp_match_workspace_size_ex(sn, sc, sw * sh, _lib.MATCH_F32) == old
        cp = (sc + 63) // 64 * 64
        images = 2 * cp * sw * sh + 2 * sn * cp
        assert old + images <= L.fmpnp_match_workspace_size_ex(sn, sc, sw * sh, _lib.MATCH_F16) <= old + images + 3 * 256
        assert L.fmpnp_match_workspace_size_ex(sn, sc, sw * sh, 2) == 0
    # the device entry points refuse an unknown precision before they touch a device or a pointer
    assert L.fmpnp_exhaustive_match_ex_async(None, 1, 1, None, 1, 1, 1, 1, 0.9, None, None, None, None, None, None, 0, 7,
                                             None) == _lib.EINVAL
    assert L.fmpnp_correlation_ex_async(None, 1, 1, None, 1, 1, 1, None, None, 0, 7, None) == _lib.EINVAL
    assert L.fmpnp_exhaustive_match_ex(None, 1, 1, None, 1, 1, 1, 1, 0.9, None, None, None, None, None, 7, None) == _lib.EINVAL
    assert L.fmpnp_localize_ex(None, None, 0, None, None, None, 0, 1, 0.9, None, 0, None, None, None, None, 7,
                               None) == _lib.EINVAL
    # the facade: anything but "f32" / "f16" is a ValueError, before any device work
    for bad in ("bf16", "F16", 16, None, 1):
        with pytest.raises(ValueError):
            fmpnp.exhaustive_match_cpu(sparse, dense, top_k, precision=bad)
        with pytest.raises(ValueError):
            fmpnp.exhaustive_match(sparse, dense, top_k, precision=bad)
        with pytest.raises(ValueError):
            fmpnp.exhaustive_search(dense, sparse, [96, 80], [w, h], [4, 4], 0.12, precision=bad)
        with pytest.raises(ValueError):
            fmpnp.exhaustive_search_multi(dense, [sparse], [96, 80], [w, h], [4, 4], 0.12, precision=bad)
    assert isinstance(ctypes.c_int(_lib.match_precision("f16")).value, int)
    assert match.exhaustive_match.__defaults__[-1] == "f32" and match.exhaustive_search_multi.__defaults__[-1] == "f32"


def test_localize_cpu_takes_the_match_precision():
    import localize_cases as lc
    sc = lc.scene("fallback_loses")
    refs = [lc.public(r) for r in sc["references"]]
    kw = dict(factor=lc.FACTOR, return_masked=True, return_all=True, **lc.PNP)
    base = fmpnp.localize_cpu(sc["query"], refs, lc.IMAGE, **kw)
    same = fmpnp.localize_cpu(sc["query"], refs, lc.IMAGE, match_precision="f32", **kw)
    lc.equal_prediction(same.prediction, base.prediction, "best")
    for x, y in zip(same.predictions, base.predictions):
        lc.equal_prediction(x, y)
    half = fmpnp.localize_cpu(sc["query"], refs, lc.IMAGE, match_precision="f16", **kw)
    assert half.kind == base.kind == "solved" and half.best == base.best
    assert half.prediction.num_matches == base.prediction.num_matches  # (the scene's ratio margins are wide)
    for bad in ("f64", 0):
        with pytest.raises(ValueError):
            fmpnp.localize_cpu(sc["query"], refs, lc.IMAGE, match_precision=bad, **kw)
        with pytest.raises(ValueError):
            fmpnp.localize(sc["query"], refs, lc.IMAGE, match_precision=bad, **kw)
        with pytest.raises(ValueError):
            fmpnp.localize_multi([(sc["query"], refs)], lc.IMAGE, match_precision=bad, **kw)
