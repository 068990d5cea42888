"""Layered matching on the GPU (fmpnp_exhaustive_match_layers: per-layer correlations, combine_kernel, the select)
against its CPU twin bit for bit -- scores with NaNs in place, argmax, top, kth and mask -- on the cases of
tests/match_layers_cases.py, through several rounds, on a side stream, and through exhaustive_search_layers."""
import ctypes

import numpy as np
import pytest
import torch

import fmpnp
from fmpnp import _lib, hypercolumn
from fmpnp.match import exhaustive_search_layers, exhaustive_search_layers_multi, points_in_query_space

import match_cases as mc
import match_layers_cases as mlc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def on_device(maps):
    return [m.to(DEV) for m in maps]


def rows_on_device(d):
    return torch.from_numpy(np.array(d, np.float32)).to(DEV)  # (a writable copy: the shared inputs are read-only)


def gpu_match(case, d, top_k, normalize=True, scores=True):
    maps, size, item, _ = mlc.layers(case)
    return fmpnp.exhaustive_match_layers(rows_on_device(d), on_device(maps), top_k, mc.RATIO,
                                         size=size, item=item, normalize=normalize, scores=scores)


def same_scores(got, want):
    return mc.same_floats(got.cpu().numpy() if torch.is_tensor(got) else got, want)


@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "plain"])
@pytest.mark.parametrize("case", mlc.ALL)
def test_equals_the_twin(case, normalize):
    """Every case (vgg16x with 64 rows: the production chain lengths), every top_k, with and without the norm."""
    for i, top_k in enumerate(mlc.case_top_ks(case)):
        if not normalize and i:
            break  # (the reduction does not depend on the flag: one top_k without it)
        want = mlc.twin(case, top_k, normalize)
        got = gpu_match(case, mlc.sparse(case), top_k, normalize, scores=(i == 0))
        mc.assert_same_result(got, want, (case, top_k))
        if i == 0:
            assert same_scores(got["scores"], want["scores"]), case


def test_nans_fall_where_the_twins_do():
    got = gpu_match("zero_texel", mlc.sparse("zero_texel"), 2)
    s = got["scores"].cpu().numpy()
    assert np.isnan(s[:, 0]).all() and np.isfinite(s[:, 1:]).all() and (got["argmax"] == 0).all()
    want = mlc.twin("nonfinite", mlc.case_top_ks("nonfinite")[0])["scores"]
    assert np.isnan(want).any() and not np.isnan(want).all()  # (the equality itself: test_equals_the_twin)


@pytest.mark.parametrize("case", ["ragged3", "sized", "tiles2", "wide"])
def test_own_texel_descriptors_equal_the_twin(case):
    """The agreement test's inputs (descriptors near the map's own columns: scores near 1)."""
    maps, size, item, _ = mlc.layers(case)
    d = mlc.own_texel_descriptors(case, 1)
    top_k = mlc.case_top_ks(case)[-2]
    want = fmpnp.exhaustive_match_layers_cpu(d, maps, top_k, mc.RATIO, size=size, item=item, scores=True)
    got = gpu_match(case, d, top_k)
    mc.assert_same_result(got, want, case)
    assert same_scores(got["scores"], want["scores"])


def test_exact_operands_equal_the_dense_path_bit_for_bit():
    maps = mlc.int_layers([(33, 5, 3), (4, 5, 3), (40, 3, 2)], seed=11, batch=2)
    c = mlc.channels(maps)
    d = np.random.default_rng(3).integers(-2, 3, (37, c)).astype(np.float32)
    dm, dd = on_device(maps), rows_on_device(d)
    for item in (0, 1):
        dense = fmpnp.assemble_hypercolumn(dm, normalize=False)[item].reshape(c, -1)
        want = fmpnp.exhaustive_match(dd, dense, 3, mc.RATIO, scores=True)
        got = fmpnp.exhaustive_match_layers(dd, dm, 3, mc.RATIO, item=item, normalize=False, scores=True)
        mc.assert_same_result(got, want, item)
        assert torch.equal(got["scores"], want["scores"]) and float(want["scores"].abs().max()) > 0


def test_rows_do_not_depend_on_their_company():
    case = "tiles2"
    _, _, _, n = mlc.layers(case)
    d, top_k = mlc.sparse(case), mlc.case_top_ks(case)[2]
    want, scores = mlc.twin(case, top_k), mlc.twin(case, mlc.case_top_ks(case)[0])["scores"]
    perm = np.random.default_rng(5).permutation(n)
    for rows in (perm, np.arange(1) + 17, perm[:63], perm[:65]):
        got = gpu_match(case, d[rows], top_k)
        mc.assert_same_result(got, {k: want[k][rows] for k in ("argmax", "top", "kth", "mask")}, len(rows))
        assert same_scores(got["scores"], scores[rows])


def _async(case, d, top_k, rows_in_workspace, with_scores, stream=None, correlation=False):
    """The asynchronous entry points on torch buffers, the workspace sized for `rows_in_workspace` rows."""
    maps, size, item, _ = mlc.layers(case)
    desc, keep = hypercolumn._plane_layers(on_device(maps), "cuda")
    h, w = mlc.out_size(maps, size)
    n, c = d.shape
    L = _lib.load()
    ws_bytes = int(L.fmpnp_match_layers_workspace_size(desc, len(keep), rows_in_workspace, h, w))
    assert ws_bytes > 0
    ws = torch.full((ws_bytes + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    dd = rows_on_device(d)
    out = dict(argmax=torch.zeros(n, dtype=torch.int32, device=DEV), top=torch.zeros(n, device=DEV),
               kth=torch.zeros(n, device=DEV), mask=torch.zeros(n, dtype=torch.uint8, device=DEV))
    scores = torch.full((n, h * w), -7.0, device=DEV) if with_scores else None
    s = stream or torch.cuda.current_stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))  # (the buffers above were filled on the current stream)
    sp = ctypes.c_void_p(s.cuda_stream)
    head = (dd.data_ptr(), n, c, desc, len(keep), int(keep[0].shape[0]), item, h, w, _lib.HC_NORMALIZE)
    if correlation:
        rc = L.fmpnp_correlation_layers_async(*head, scores.data_ptr(), ws.data_ptr(), ws_bytes, sp)
    else:
        rc = L.fmpnp_exhaustive_match_layers_async(*head, top_k, mc.RATIO, out["argmax"].data_ptr(), out["top"].data_ptr(),
                                                   out["kth"].data_ptr(), out["mask"].data_ptr(),
                                                   scores.data_ptr() if with_scores else None, ws.data_ptr(), ws_bytes, sp)
    assert rc == 0
    s.synchronize()
    assert (ws[ws_bytes:] == 0x5A).all()  # (nothing is written past the stated size)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["mask"] = res["mask"].astype(bool)
    res["scores"] = scores
    return res


def test_several_rounds_equal_one():
    """A workspace sized for two rows with N = 5: three rounds; the same bits as one round, with and without a
    caller's scores map, and the score map alone."""
    case = "ragged3"
    d, top_k = mlc.sparse(case)[:5], mlc.case_top_ks(case)[2]
    want = mlc.twin(case, top_k)
    scores = mlc.twin(case, mlc.case_top_ks(case)[0])["scores"][:5]
    for rows, with_scores in ((2, False), (2, True), (5, True), (1, True)):
        got = _async(case, d, top_k, rows, with_scores)
        mc.assert_same_result(got, {k: want[k][:5] for k in ("argmax", "top", "kth", "mask")}, (rows, with_scores))
        if with_scores:
            assert same_scores(got["scores"], scores)
    assert same_scores(_async(case, d, top_k, 2, True, correlation=True)["scores"], scores)


def test_a_side_stream_and_a_second_run_change_nothing():
    case = "tiles2"
    d, top_k = mlc.sparse(case), mlc.case_top_ks(case)[1]
    want, scores = mlc.twin(case, top_k), mlc.twin(case, mlc.case_top_ks(case)[0])["scores"]
    # (a stream of the framework's high-priority pool, as test_gpu_encoder.py says: taking one of the default pool
    # would shift which two streams the tests that time two default-priority streams against each other draw)
    side = torch.cuda.Stream(device=DEV, priority=-1)
    with torch.cuda.stream(side):
        first = gpu_match(case, d, top_k)
        second = gpu_match(case, d, top_k)
    for got in (first, second, _async(case, d, top_k, 129, True, stream=side)):
        mc.assert_same_result(got, want)
        assert same_scores(got["scores"], scores)


def test_views_through_the_wrapper_equal_the_twin():
    maps, size, item, _ = mlc.layers("views")
    big = [torch.zeros(3, m.shape[1] + 2, m.shape[2] + 1, m.shape[3] + 3, device=DEV) for m in maps]
    views = []
    for b, m in zip(big, maps):
        v = b[1:, 1:m.shape[1] + 1, :m.shape[2], 2:2 + m.shape[3]]
        v.copy_(m)
        views.append(v)
    assert not any(v.is_contiguous() for v in views)
    top_k = mlc.case_top_ks("views")[0]
    d = torch.from_numpy(mc.padded(mlc.sparse("views"), 3).base).to(DEV)[:, :mlc.channels(maps)]
    got = fmpnp.exhaustive_match_layers(d, views, top_k, mc.RATIO, item=item, scores=True)
    want = mlc.twin("views", top_k)
    mc.assert_same_result(got, want)
    assert same_scores(got["scores"], want["scores"])


def test_exhaustive_search_layers_multi_equals_the_separate_calls():
    case = "tiles2"
    maps, size, item, n = mlc.layers(case)
    dm = on_device(maps)
    h, w = mlc.out_size(maps, size)
    image, factor = (4 * h, 4 * w), 0.12
    d = rows_on_device(mlc.sparse(case))
    parts = [d[:1], d[1:64], d[64:]]
    multi = exhaustive_search_layers_multi(dm, parts, image, None, factor)
    want = mlc.twin(case, int(factor * h * w))
    at = 0
    for part, (pts, mask) in zip(parts, multi):
        one_pts, one_mask = exhaustive_search_layers(dm, part, image, None, factor)
        assert torch.equal(pts, one_pts) and np.array_equal(mask, one_mask)
        k = part.shape[0]
        assert torch.equal(pts, points_in_query_space(want["argmax"][at:at + k], image, h, w))
        assert np.array_equal(mask, want["mask"][at:at + k])
        at += k
    # HypercolumnExtractor.match: the same call behind compute_feature_maps
    import hypercolumn_cases as hcc
    net = hcc.tiny_encoder().to(DEV)
    ex = fmpnp.HypercolumnExtractor(net, hcc.ENCODER_LAYERS)
    img = hcc.tiny_image().to(DEV)
    layers, res = ex.compute_feature_maps(img)
    rows = torch.randn(9, sum(m.shape[1] for m in layers), generator=torch.Generator().manual_seed(4)).to(DEV)
    found, res2 = ex.match(img, [rows], tuple(res), None, 0.12)
    pts, mask = exhaustive_search_layers(layers, rows, tuple(res), None, 0.12)
    assert tuple(res2) == tuple(res) and torch.equal(found[0][0], pts) and np.array_equal(found[0][1], mask)


def test_argument_errors_of_the_device_entry_points():
    maps, size, item, _ = mlc.layers("ragged3")
    dm = on_device(maps)
    d = rows_on_device(mlc.sparse("ragged3")[:5])
    with pytest.raises(ValueError):
        fmpnp.exhaustive_match_layers(d[:, :11], dm, 1)
    with pytest.raises(ValueError):
        fmpnp.exhaustive_match_layers(d, dm, 1, item=1)
    with pytest.raises(ValueError):
        fmpnp.exhaustive_match_layers(d.cpu(), dm, 1)
    with pytest.raises(_lib.FmpnpError):
        fmpnp.exhaustive_match_layers(d, dm, 64)
    with pytest.raises(_lib.FmpnpError):
        fmpnp.exhaustive_match_layers(d, dm, 0)
    L = _lib.load()
    desc, keep = hypercolumn._plane_layers(dm, "cuda")
    out = torch.zeros(64, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    sp = _lib.stream_ptr(torch.device(DEV))

    def call(n=5, ld=12, L_=3, item=0, h=9, w=7, flags=1, top_k=2, ws_ptr=None, ws_bytes=1 << 16):
        return L.fmpnp_exhaustive_match_layers_async(
            d.data_ptr(), n, ld, desc, L_, 1, item, h, w, flags, top_k, 0.9, out.data_ptr(), out.data_ptr(),
            out.data_ptr(), out.data_ptr(), None, ws.data_ptr() if ws_ptr is None else ws_ptr, ws_bytes, sp)
    E = _lib.EINVAL
    assert call(n=-1) == E and call(ld=11) == E and call(L_=0) == E and call(L_=9) == E and call(item=1) == E
    assert call(h=0) == E and call(flags=3) == E and call(top_k=0) == E and call(top_k=64) == E
    assert call(ws_bytes=256 + 4 * (63 + 20 + 6 + 63) - 1) == E  # (one byte short of the norm plane and one row)
    assert call(ws_ptr=ws.data_ptr() + 4) == E                 # (the workspace is 16-byte aligned)
    assert call(h=(1 << 24) + 1) == _lib.ETOOBIG
    assert L.fmpnp_correlation_layers_async(d.data_ptr(), 5, 12, desc, 3, 1, 0, 9, 7, 1, None, ws.data_ptr(), 1 << 16, sp) == E
    assert call(n=0) == 0
    torch.cuda.synchronize()
