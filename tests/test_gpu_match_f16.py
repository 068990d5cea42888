"""The fp16 precision of the match stage on the GPU (precision="f16": both operands converted to binary16,
v_mfma_f32_32x32x16_f16 with fp32 accumulation): bit for bit the exact twin on integers, within the
accumulation bound of its CPU reference on real values, the unchanged row reduction on its scores, its
decisions against the exact path, non-finite operands, launch independence, and the localisation chain."""
import numpy as np
import pytest
import torch

import fmpnp
from fmpnp import _lib
from fmpnp.match import exhaustive_search_multi, gather_sparse_descriptors

import localize_cases as lc
import match_cases as mc
import match_f16_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the shared operands are read-only)


def dev_padded(a, pad):
    """A CUDA view of a with `pad` unused columns after every row (NaN-filled: never read)."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = torch.from_numpy(np.array(a))
    return buf[:, :a.shape[1]]


def reduced(scores, top_k):
    argmax, top, kth, mask = mc.reduce_rows(scores, top_k)
    return dict(argmax=argmax, top=top, kth=kth, mask=mask)


@pytest.mark.parametrize("shape", mc.SHAPES, ids=str)
def test_integers_equal_the_exact_twin(shape):
    """The test of the lane maps, the k-blocked layout, the zero tails and the epilogue: small integers are exact
    in fp16 and so is every partial sum in fp32, so whatever the order inside the MFMA the scores and the four
    outputs are the exact twin's bit for bit.  The operands are asymmetric: a row / column swap cannot pass."""
    n, c, w, h = shape
    sparse, dense = mc.operands(n, c, w, h, "ints")
    ds, dd = dev(sparse), dev(dense)
    for i, top_k in enumerate(mc.top_ks(w * h)):
        want = mc.twin(n, c, w, h, top_k, "ints")
        got = fmpnp.exhaustive_match(ds, dd, top_k, mc.RATIO, scores=(i == 0), precision="f16")
        mc.assert_same_result(got, want, (shape, top_k))
        if i == 0:
            assert mc.same_floats(got["scores"].cpu().numpy(), want["scores"]), shape


@pytest.mark.parametrize("shape", mc.SHAPES, ids=str)
def test_scores_are_within_the_accumulation_bound_of_the_reference(shape):
    """|s_gpu - s_ref| <= C 2^-23 sum_k |fl16(a)| |fl16(b)| + 2^-24 |s_ref| per score, on operands without fp16
    subnormals; and the row reduction on those scores is the contract's at every top_k."""
    n, c, w, h = shape
    sparse, dense = fc.operands(n, c, w, h)
    ds, dd = dev(sparse), dev(dense)
    scores = None
    for i, top_k in enumerate(mc.top_ks(w * h)):
        got = fmpnp.exhaustive_match(ds, dd, top_k, mc.RATIO, scores=(i == 0), precision="f16")
        if i == 0:
            scores = got["scores"].cpu().numpy()
            ref = fc.reference(n, c, w, h)["scores"]
            err, bound = np.abs(scores.astype(np.float64) - ref.astype(np.float64)), fc.accumulation_bound(n, c, w, h)
            with np.errstate(invalid="ignore", divide="ignore"):
                print(shape, "largest error / bound:", float(np.nanmax(np.where(bound > 0, err / bound, 0.0))),
                      "scores that differ from the reference:", int((err > 0).sum()), "of", err.size)
            assert (err <= bound).all()
        mc.assert_same_result(got, reduced(scores, top_k), (shape, top_k))


@pytest.mark.parametrize("shape", mc.SHAPES[1:], ids=str)
def test_decisions_against_the_exact_path(shape):
    """E = the rounding bound plus the accumulation bound, the largest over the row's scores.  On every row whose
    exact best score leads its runner-up by more than 2 E the f16 argmax is the exact path's; and at least 3/4
    of the rows are such rows."""
    n, c, w, h = shape
    sparse, dense = fc.operands(n, c, w, h)
    exact = fmpnp.exhaustive_match_cpu(sparse, dense, 1, mc.RATIO, scores=True)
    got = fmpnp.exhaustive_match(dev(sparse), dev(dense), 1, mc.RATIO, precision="f16")
    e = (fc.rounding_bound(n, c, w, h) + fc.accumulation_bound(n, c, w, h)).max(axis=1)
    srt = np.sort(exact["scores"].astype(np.float64), axis=1)
    clear = (srt[:, -1] - srt[:, -2]) > 2 * e
    print(shape, "rows with a clear lead:", int(clear.sum()), "of", n, "; rows with the exact argmax:",
          int((got["argmax"] == exact["argmax"]).sum()))
    assert clear.sum() * 4 >= 3 * n
    assert np.array_equal(got["argmax"][clear], exact["argmax"][clear])


def test_non_finite_operands():
    """NaNs (two columns), +Inf, -Inf, and 1e5 (-> +Inf in fp16): the NaNs and the +-Infs of the scores sit where
    the reference's do, and the reduction on them is the contract's below, at and above the NaNs per row."""
    sparse, dense = (a.copy() for a in fc.operands(37, 40, 24, 20))
    dense[3, 100], dense[4, 17], dense[5, 300], dense[6, 301], dense[7, 55] = np.nan, np.nan, np.inf, -np.inf, 1e5
    ds, dd = dev(sparse), dev(dense)
    ref = fmpnp.exhaustive_match_cpu(sparse, dense, 1, scores=True, precision="f16")["scores"]
    assert np.isnan(ref[:, [17, 100]]).all() and np.isinf(ref[1:, 55]).sum() >= 30 and np.isnan(ref[0, 55])
    scores = None
    for i, top_k in enumerate((1, 2, 3, 57, 480)):
        got = fmpnp.exhaustive_match(ds, dd, top_k, scores=(i == 0), precision="f16")
        if i == 0:
            scores = got["scores"].cpu().numpy()
            assert np.array_equal(np.isnan(scores), np.isnan(ref))
            assert np.array_equal(scores == np.inf, ref == np.inf) and np.array_equal(scores == -np.inf, ref == -np.inf)
        mc.assert_same_result(got, reduced(scores, top_k), top_k)
    assert np.all(got["argmax"] == 17)


def test_exhaustive_search_multi_equals_the_separate_calls():
    """The bits of a score depend on its row, its column and C only: references at every offset inside the
    128-row tiles, in one launch over the once-converted dense map, equal one call each."""
    n, c, w, h = 129, 33, 33, 40
    sparse, dense = mc.operands(n, c, w, h)
    dd = dev(dense)
    parts = [sparse[:50], sparse[50:51], sparse[51:]]
    args = ([330, 400], [w, h], [10, 10], 0.12)
    multi = fmpnp.exhaustive_search_multi(dd, [dev(p) for p in parts], *args, precision="f16")
    assert len(multi) == 3
    for p, (pts, mask) in zip(parts, multi):
        pts1, mask1 = fmpnp.exhaustive_search(dd, dev(p), *args, precision="f16")
        assert pts.shape == (p.shape[0], 2) and torch.equal(pts, pts1) and np.array_equal(mask, mask1)
    # ... and the scores themselves, rows 50 and 51.. against the same rows inside the whole
    top_k = int(0.12 * w * h)
    whole = fmpnp.exhaustive_match(dev(sparse), dd, top_k, scores=True, precision="f16")
    at = 0
    for p in parts:
        one = fmpnp.exhaustive_match(dev(p), dd, top_k, scores=True, precision="f16")
        assert torch.equal(one["scores"], whole["scores"][at:at + p.shape[0]])
        mc.assert_same_result(one, {k: whole[k][at:at + p.shape[0]] for k in ("argmax", "top", "kth", "mask")})
        at += p.shape[0]


@pytest.mark.parametrize("shape", mc.SHAPES[1:3], ids=str)
def test_padded_rows_and_two_runs(shape):
    """ld_sparse = C + 3 and ld_dense = W H + 5 (odd: no alignment to lean on; the padding is NaN and never
    read) equal the contiguous call bit for bit, scores included; and so does a second run."""
    n, c, w, h = shape
    sparse, dense = mc.operands(n, c, w, h)
    top_k = mc.top_ks(w * h)[2]
    base = fmpnp.exhaustive_match(dev(sparse), dev(dense), top_k, mc.RATIO, scores=True, precision="f16")
    ds, dd = dev_padded(sparse, 3), dev_padded(dense, 5)
    assert ds.stride(0) == c + 3 and dd.stride(0) == w * h + 5
    for operands in ((ds, dd), (dev(sparse), dev(dense))):
        got = fmpnp.exhaustive_match(*operands, top_k, mc.RATIO, scores=True, precision="f16")
        mc.assert_same_result(got, base, shape)
        assert torch.equal(got["scores"].view(torch.int32), base["scores"].view(torch.int32))


def test_rows_in_more_than_one_round():
    """A map so large that the score workspace holds 64 rows: without a scores map 65 rows run in two rounds
    through it.  The outputs equal those of a call that writes a full scores map, row 64's scores equal a call
    of that row alone, and every row's top is the score at its argmax."""
    n, c, wh = 65, 2, 1 << 20
    L = _lib.load()
    assert L.fmpnp_match_workspace_size(n, wh) == 64 * wh * 4
    assert L.fmpnp_match_workspace_size_ex(n, c, wh, _lib.MATCH_F16) >= 64 * wh * 4 + 64 * wh * 2 + n * 64 * 2
    rng = np.random.default_rng(7)
    ds = dev(rng.standard_normal((n, c)).astype(np.float32))
    dd = dev(rng.standard_normal((c, wh)).astype(np.float32))
    top_k = int(0.006 * wh)
    rounds = fmpnp.exhaustive_match(ds, dd, top_k, precision="f16")
    full = fmpnp.exhaustive_match(ds, dd, top_k, scores=True, precision="f16")
    mc.assert_same_result(rounds, full)
    last = fmpnp.exhaustive_match(ds[64:], dd, top_k, scores=True, precision="f16")
    assert torch.equal(last["scores"][0].view(torch.int32), full["scores"][64].view(torch.int32))
    at = full["scores"][torch.arange(n, device=DEV), torch.from_numpy(full["argmax"]).to(DEV).long()].cpu().numpy()
    assert np.array_equal(at, rounds["top"]) and np.array_equal(full["scores"].max(dim=1).values.cpu().numpy(), rounds["top"])


def test_f32_through_the_new_entry_points_is_the_exact_path():
    n, c, w, h = mc.SHAPES[2]
    sparse, dense = mc.operands(n, c, w, h)
    ds, dd = dev(sparse), dev(dense)
    top_k = mc.top_ks(w * h)[0]
    want = mc.twin(n, c, w, h, top_k)
    got = fmpnp.exhaustive_match(ds, dd, top_k, mc.RATIO, scores=True, precision="f32")
    mc.assert_same_result(got, want)
    assert got["scores"].cpu().numpy().tobytes() == want["scores"].tobytes()
    # the C entry points with FMPNP_MATCH_F32, and the correlation alone under both precisions
    L = _lib.load()
    out = dict(argmax=np.zeros(n, np.int32), top=np.zeros(n, np.float32), kth=np.zeros(n, np.float32), mask=np.zeros(n, np.uint8))
    sp = _lib.stream_ptr(torch.device(DEV))
    rc = L.fmpnp_exhaustive_match_ex(ds.data_ptr(), n, c, dd.data_ptr(), c, w * h, w * h, top_k, mc.RATIO,
                                     out["argmax"].ctypes.data, out["top"].ctypes.data, out["kth"].ctypes.data,
                                     out["mask"].ctypes.data, None, _lib.MATCH_F32, sp)
    assert rc == 0
    out["mask"] = out["mask"].astype(bool)
    mc.assert_same_result(out, want)
    assert L.fmpnp_exhaustive_match_ex(ds.data_ptr(), n, c, dd.data_ptr(), c, w * h, w * h, top_k, mc.RATIO,
                                       out["argmax"].ctypes.data, out["top"].ctypes.data, out["kth"].ctypes.data,
                                       out["mask"].ctypes.data, None, 2, sp) == _lib.EINVAL
    corr = torch.empty((n, w * h), dtype=torch.float32, device=DEV)
    assert L.fmpnp_correlation_ex_async(ds.data_ptr(), n, c, dd.data_ptr(), c, w * h, w * h, corr.data_ptr(), None, 0,
                                        _lib.MATCH_F32, sp) == 0
    assert corr.cpu().numpy().tobytes() == want["scores"].tobytes()
    nbytes = int(L.fmpnp_match_workspace_size_ex(n, c, w * h, _lib.MATCH_F16))
    ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=DEV)
    assert L.fmpnp_correlation_ex_async(ds.data_ptr(), n, c, dd.data_ptr(), c, w * h, w * h, corr.data_ptr(), None, 0,
                                        _lib.MATCH_F16, sp) == _lib.EINVAL  # (the f16 images need the workspace)
    assert L.fmpnp_correlation_ex_async(ds.data_ptr(), n, c, dd.data_ptr(), c, w * h, w * h, corr.data_ptr(),
                                        ws.data_ptr(), nbytes, _lib.MATCH_F16, sp) == 0
    half = fmpnp.exhaustive_match(ds, dd, top_k, mc.RATIO, scores=True, precision="f16")
    assert torch.equal(corr.view(torch.int32), half["scores"].view(torch.int32))


# ---- the localisation chain -----------------------------------------------------------------------

def on_device(name):
    sc = lc.scene(name)
    refs = []
    for r in sc["references"]:
        r = lc.public(r)
        r["hypercolumn"] = torch.from_numpy(r["hypercolumn"]).to(DEV)
        refs.append(r)
    return torch.from_numpy(sc["query"]).to(DEV), refs


def staged_f16(qmap, refs):
    """The staged composition of the public stages with the f16 match (as test_gpu_localize.py's yardstick does
    for the exact path): exhaustive_search_multi(precision="f16") -> numpy masking -> solve_pnp_multi -> the
    fallback and the best pick in numpy."""
    sparse = []
    for r in refs:
        if "sparse_descriptors" in r:
            sparse.append(torch.from_numpy(r["sparse_descriptors"]).to(DEV))
        else:
            sparse.append(gather_sparse_descriptors(r["hypercolumn"], r["points_2D"], lc.IMAGE[0] / lc.W, lc.IMAGE[1] / lc.H))
    found = exhaustive_search_multi(qmap.reshape(lc.C, -1), sparse, lc.IMAGE, [lc.W, lc.H], None, lc.FACTOR,
                                    precision="f16")
    matches = [(pts.cpu().numpy(), mask) for pts, mask in found]

    def solve(points_2D, points_3D, ref, ref_2D):
        return fmpnp.solve_pnp_multi([(points_2D, points_3D, ref["filename"], ref_2D, None)], ref["intrinsics"],
                                     ref["distortion_coefficients"], return_masked=True, **lc.PNP)[0]
    return lc.staged(refs, matches, solve)


def equal_localization(a, b):
    lc.equal(a.export, b.export, "export")
    lc.equal_prediction(a.prediction, b.prediction, "best")
    assert a.kind == b.kind and a.best == b.best
    for j, (x, y) in enumerate(zip(a.predictions, b.predictions)):
        lc.equal_prediction(x, y, f"pair {j}")


@pytest.mark.parametrize("name", sorted(lc.SCENES))
def test_the_chain_equals_the_staged_composition(name):
    qmap, refs = on_device(name)
    kw = dict(factor=lc.FACTOR, return_masked=True, return_all=True, refine=False, **lc.PNP)
    every, eligible, _ = staged_f16(qmap, refs)
    export, best = lc.choose([p for _, p in eligible])
    got = fmpnp.localize(qmap, refs, lc.IMAGE, match_precision="f16", **kw)
    lc.equal(got.export, export, "export")
    lc.equal_prediction(got.prediction, best, "best")
    assert len(got.predictions) == len(every)
    for j, pred in enumerate(every):
        lc.equal_prediction(got.predictions[j], pred, f"pair {j}")
    if best is None:
        assert name == "none" and got.kind == "none"
    else:
        assert got.best == [k for k, p in eligible if p is best][0]
    # the exact default is what it is without the argument
    equal_localization(fmpnp.localize(qmap, refs, lc.IMAGE, match_precision="f32", **kw),
                       fmpnp.localize(qmap, refs, lc.IMAGE, **kw))


def test_localize_multi_and_the_async_form_equal_the_single_calls():
    from fmpnp import _localize as loc
    queries = [on_device(name) for name in lc.MULTI]
    kw = dict(factor=lc.FACTOR, return_masked=True, return_all=True, refine=False, **lc.PNP)
    multi = fmpnp.localize_multi(queries, lc.IMAGE, match_precision="f16", **kw)
    assert [m.kind for m in multi] == ["solved", "none", "fallback"]
    params = loc._pnp_params(return_masked=True, **lc.PNP)
    for (qmap, refs), m in zip(queries, multi):
        single = fmpnp.localize(qmap, refs, lc.IMAGE, match_precision="f16", **kw)
        equal_localization(m, single)
        launched, = loc.LocalizeLaunch([(qmap, refs)], lc.IMAGE, lc.FACTOR, params, return_all=True,
                                       match_precision="f16").read()
        equal_localization(launched, single)
