"""Dense exhaustive matching without a GPU: the CPU twin (fmpnp_exhaustive_match_cpu) against the
reference's goldens (tests/golden/gen_golden_match.py) and against the contract, the closed-form
nearest cell against the reference's argmins, argument validation of every new entry point, and the
factor binding."""
import ctypes

import numpy as np
import pytest

import fmpnp
from fmpnp import _lib, config, match

import match_cases as mc


def search_cpu(dense, sparse, image_shape, map_size, factor):
    """exhaustive_search's return values formed from the twin's argmax and mask."""
    w, h = (int(v) for v in map_size)
    res = fmpnp.exhaustive_match_cpu(sparse, dense, int(factor * w * h), mc.RATIO)
    return match.points_in_query_space(res["argmax"], image_shape, w, h).numpy(), res["mask"]


def test_twin_matches_the_reference_on_every_row():
    g = mc.golden("main")
    for f in g["factors"]:
        pts, mask = search_cpu(g["dense"], g["sparse"], g["image_shape"], g["map_size"], float(f))
        assert pts.dtype == np.float32 and np.array_equal(pts, g[f"points_{f}"]), f
        assert np.array_equal(mask, g[f"mask_{f}"]), f
        assert mask.sum() >= 5 and (~mask).sum() >= 5  # (both outcomes are really compared)


@pytest.mark.parametrize("name", mc.EDGE_CASES)
def test_twin_matches_the_reference_on_the_edge_cases(name):
    g = mc.golden("edge_" + name)
    pts, mask = search_cpu(g["dense"], g["sparse"], g["image_shape"], g["map_size"], float(g["factor"]))
    assert np.array_equal(pts, g["points"])
    assert np.array_equal(mask, g["mask"])


def test_edge_cases_behave_as_recorded():
    """What each edge case pins, read off the twin's raw outputs."""
    g = mc.golden("edge_nan")
    w, h = (int(v) for v in g["map_size"])
    r = fmpnp.exhaustive_match_cpu(g["sparse"], g["dense"], int(float(g["factor"]) * w * h))
    assert np.all(r["argmax"] == int(g["column"])) and np.isnan(r["top"]).all() and not r["mask"].any()
    g = mc.golden("edge_inf")
    r = fmpnp.exhaustive_match_cpu(g["sparse"], g["dense"], int(float(g["factor"]) * w * h))
    pos = g["sparse"][:, 7] > 0
    assert np.all(r["argmax"][pos] == int(g["column"])) and np.all(r["top"][pos] == np.inf) and r["mask"][pos].all()
    assert np.isfinite(r["top"][~pos]).all()
    g = mc.golden("edge_tie")
    r = fmpnp.exhaustive_match_cpu(g["sparse"], g["dense"], int(float(g["factor"]) * w * h))
    assert r["argmax"][0] == r["argmax"][3] == int(g["column"])
    g = mc.golden("edge_top1")
    r = fmpnp.exhaustive_match_cpu(g["sparse"], g["dense"], 1)
    assert np.array_equal(r["top"], r["kth"]) and np.array_equal(r["mask"], r["top"] <= 0)
    r = fmpnp.exhaustive_match_cpu(g["sparse"], g["dense"], w * h, scores=True)
    assert np.array_equal(r["kth"], r["scores"].min(axis=1))


@pytest.mark.parametrize("shape", mc.SHAPES[:3] + [(8, 1664, 16, 16)], ids=str)
def test_twin_scores_against_fp64(shape):
    """|score - fp64| <= 4e-7 * sum |a b|: the fp32 chain's error for K <= 4096, with margin."""
    n, c, w, h = shape
    sparse, dense = mc.operands(n, c, w, h)
    got = fmpnp.exhaustive_match_cpu(sparse, dense, 1, scores=True)["scores"]
    s64, d64 = sparse.astype(np.float64), dense.astype(np.float64)
    err = np.abs(got.astype(np.float64) - s64 @ d64)
    assert np.all(err <= 4e-7 * (np.abs(s64) @ np.abs(d64)))


def test_twin_scores_are_the_ascending_fmaf_chain():
    """Bit for bit, on a shape small enough for a Python loop: fmaf in ascending k from +0 (an fp64
    product of two fp32 values is exact, so rounding fp64(a * b + acc) once is the fused operation
    whenever that fp64 sum is exact -- integer operands keep it so)."""
    sparse, dense = mc.operands(5, 7, 3, 4, "ints")
    got = fmpnp.exhaustive_match_cpu(sparse, dense, 1, scores=True)["scores"]
    acc = np.zeros((5, 12), np.float32)
    for k in range(7):
        acc = (sparse[:, k:k + 1].astype(np.float64) * dense[k:k + 1].astype(np.float64)
               + acc.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got, acc) and not np.any(np.signbit(got) & (got == 0))  # (from +0: never -0)


@pytest.mark.parametrize("kind", ["normal", "ints"])
@pytest.mark.parametrize("shape", mc.SHAPES[:3], ids=str)
def test_twin_reduction_obeys_the_contract(shape, kind):
    """argmax, d1, d_k and mask against an independent numpy statement of the contract on the twin's
    own scores: duplicated values, negative values, +-0, a constant row, every listed top_k."""
    n, c, w, h = shape
    sparse, dense = mc.operands(n, c, w, h, kind)
    scores = None
    for top_k in mc.top_ks(w * h):
        r = fmpnp.exhaustive_match_cpu(sparse, dense, top_k, scores=scores is None)
        scores = r["scores"] if scores is None else scores
        argmax, top, kth, mask = mc.reduce_rows(scores, top_k)
        mc.assert_same_result(r, dict(argmax=argmax, top=top, kth=kth, mask=mask), (shape, kind, top_k))
        for v in (r["top"], r["kth"]):
            assert not np.any(np.signbit(v) & (v == 0))  # (never -0)
    if kind == "normal" and n > 1:  # the zero sparse row: one repeated score
        assert r["argmax"][0] == 0 and r["top"][0] == 0 and r["kth"][0] == 0 and r["mask"][0]


def test_twin_non_finite_rows_obey_the_contract():
    sparse, dense = (a.copy() for a in mc.operands(37, 40, 24, 20))
    dense[3, 100], dense[4, 17], dense[5, 300], dense[6, 301] = np.nan, np.nan, np.inf, -np.inf
    for top_k in (1, 2, 3, 57, 480):
        r = fmpnp.exhaustive_match_cpu(sparse, dense, top_k, scores=True)
        argmax, top, kth, mask = mc.reduce_rows(r["scores"], top_k)
        mc.assert_same_result(r, dict(argmax=argmax, top=top, kth=kth, mask=mask), top_k)
    assert np.all(r["argmax"][1:] == 17)  # the lowest NaN (row 0 is the zero row: 0 * NaN is NaN too)


def test_twin_padded_rows_and_threads():
    sparse, dense = mc.operands(37, 40, 24, 20)
    want = fmpnp.exhaustive_match_cpu(sparse, dense, 57, scores=True, n_threads=1)
    got = fmpnp.exhaustive_match_cpu(mc.padded(sparse, 3), mc.padded(dense, 5), 57, scores=True, n_threads=4)
    mc.assert_same_result(got, want)
    assert mc.same_floats(got["scores"], want["scores"])


def test_nearest_cell_matches_the_reference_argmin():
    """The closed form per axis against fast_closest_points' argmin over the whole grid: random points
    (some outside the image) and, on the exact grid, every cell edge and centre (ties: the lower cell)."""
    g = mc.golden("assoc")
    for tag in ("exact", "ragged"):
        d1, d2 = (int(v) for v in g[f"{tag}_fmap"])
        grid, cells = match.generate_dense_keypoints([d1, d2], [int(v) for v in g[f"{tag}_res"]])
        assert np.array_equal(grid, g[f"{tag}_grid"]) and np.array_equal(np.array(cells), g[f"{tag}_cells"])
        got = match.nearest_cells(g[f"{tag}_points"], d1, d2, cells[0], cells[1])
        assert np.array_equal(got, g[f"{tag}_argmin"]), tag


def test_new_entry_points_reject_bad_arguments_without_a_device():
    L = _lib.load()
    vp = ctypes.c_void_p
    p = vp(4096)
    assert L.fmpnp_match_workspace_size(0, 16) == 0 and L.fmpnp_match_workspace_size(4, 0) == 0
    assert L.fmpnp_match_workspace_size(4, 16) == 4 * 16 * 4
    assert L.fmpnp_match_workspace_size(100000, 65536) == 256 << 20  # bounded for large N

    def args(N=4, lds=8, C=8, WH=16, ldd=16, top_k=2, ratio=0.9, sparse=p, dense=p, out=p):
        return [sparse, N, lds, dense, C, WH, ldd, top_k, ratio, out, out, out, out]

    bad = [dict(N=-1), dict(C=0), dict(WH=0), dict(lds=7), dict(ldd=15), dict(top_k=0), dict(top_k=17),
           dict(ratio=float("nan")), dict(sparse=None), dict(dense=None), dict(out=None)]
    for kw in bad:
        assert L.fmpnp_exhaustive_match_async(*args(**kw), None, p, 1 << 20, None) == -1, kw
        assert L.fmpnp_exhaustive_match(*args(**kw), None, None) == -1, kw
        assert L.fmpnp_exhaustive_match_cpu(*args(**kw), None, 1) == -1, kw
    for kw in bad[:5] + bad[8:]:
        a = args(**kw)
        assert L.fmpnp_correlation_async(*a[:7], a[9], None) == -1, kw
    assert L.fmpnp_correlation_async(*args(N=0)[:7], p, None) == 0
    big = args(WH=2 ** 31 - 1, ldd=2 ** 31 - 1)  # column indices are 32-bit: FMPNP_ETOOBIG
    assert L.fmpnp_exhaustive_match_async(*big, p, None, 0, None) == -4
    assert L.fmpnp_exhaustive_match(*big, None, None) == -4
    assert L.fmpnp_correlation_async(*big[:7], p, None) == -4
    # no scores map and no (or too small a) workspace
    assert L.fmpnp_exhaustive_match_async(*args(), None, None, 0, None) == -1
    assert L.fmpnp_exhaustive_match_async(*args(), None, p, 4 * 16 * 4 - 1, None) == -1
    assert L.fmpnp_exhaustive_match_cpu(*args(), None, -1) == -1  # n_threads
    # nothing to do
    assert L.fmpnp_exhaustive_match_async(*args(N=0), None, None, 0, None) == 0
    assert L.fmpnp_exhaustive_match(*args(N=0), None, None) == 0
    assert L.fmpnp_exhaustive_match_cpu(*args(N=0), None, 1) == 0

    def gargs(chw=p, C=4, D1=3, D2=5, pts=p, N=2, c0=8.0, c1=8.0, out=p, ld=4):
        return [chw, C, D1, D2, pts, N, c0, c1, out, ld, None]
    for kw in (dict(chw=None), dict(pts=None), dict(out=None), dict(C=0), dict(D1=0), dict(D2=0), dict(N=-1),
               dict(c0=0.0), dict(c1=-1.0), dict(c0=float("nan")), dict(c1=float("inf")), dict(ld=3)):
        assert L.fmpnp_gather_sparse_descriptors(*gargs(**kw)) == -1, kw
    assert L.fmpnp_gather_sparse_descriptors(*gargs(D1=1 << 16, D2=1 << 16)) == -4  # FMPNP_ETOOBIG
    assert L.fmpnp_gather_sparse_descriptors(*gargs(N=0)) == 0


def test_python_layer_checks_top_k_and_factor():
    with pytest.raises(IndexError):
        match._top_k(0.0001, 24, 20)   # int(factor * W * H) == 0: the reference raises IndexError
    with pytest.raises(IndexError):
        match._top_k(1.5, 24, 20)
    assert match._top_k(0.006, 256, 256) == 393 and match._top_k(0.12, 24, 20) == 57


def test_configure_binds_the_factor():
    before = config.exhaustive_search_kwargs()
    try:
        assert before == dict(factor=None)
        with pytest.raises(TypeError):
            match._factor(None)
        fmpnp.config.configure(exhaustive_search_factor=0.006)
        assert config.exhaustive_search_kwargs() == dict(factor=0.006)
        assert match._factor(None) == 0.006 and match._factor(0.12) == 0.12
        with pytest.raises(KeyError):
            fmpnp.config.configure(exhaustive_search_ratio=0.8)
        assert config.model_kwargs()["n_iters"] == 50  # (the other bindings are untouched)
    finally:
        config.configure(exhaustive_search_factor=before["factor"])
