"""Sparse hypercolumns on the GPU (fmpnp.sparse_hypercolumn / fmpnp_hypercolumn_sparse): equal to the CPU twin
and to the existing device composition "assemble, then gather" bit for bit, and the opt-in paths built on it
(feature_pnp(reference_layers=...), optimize_feature_pnp(sparse_reference=True), references carrying
feature_maps in localize / localize_multi) equal to the paths through the assembled map in every output.
Cases: tests/hypercolumn_sparse_cases.py; scenes: tests/localize_cases.py."""
import functools
import importlib
from collections import namedtuple

import numpy as np
import pytest
import torch

import fmpnp
from fmpnp import _lib, replay, synth
from fmpnp.match import fast_sparse_keypoint_descriptor, generate_dense_keypoints
from fmpnp.refine import gather_reference

import hypercolumn_cases as hc
import hypercolumn_sparse_cases as sc
import localize_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ofp = importlib.import_module("fmpnp.optimize_feature_pnp")


@functools.lru_cache(maxsize=None)
def dev(name):
    return [m.to(DEV) for m in sc.inputs(name)[0]]


def both(name, pts, mode, item=None, **kw):
    """(GPU rows on the host, twin rows)."""
    kw = {**sc.kwargs(name, mode), **kw}
    got = fmpnp.sparse_hypercolumn(dev(name), pts, item=item, **kw)
    assert got.is_cuda
    return got.cpu(), fmpnp.sparse_hypercolumn_cpu(sc.inputs(name)[0], pts, item=item, **kw)


@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("name", sc.ALL)
def test_gpu_equals_the_twin(name, normalize):
    """Every texel of every item, and the seeded fp64 points of the two other modes, at both output types.
    "vgg16x" is 26 blocks, "big" (70 000 channels) takes the chunked path, "views" is copied dense here."""
    tex, item = sc.all_texels(name)
    for dtype in (torch.float32, torch.float64):
        got, want = both(name, tex, "texel", item=item, normalize=normalize, dtype=dtype)
        assert got.dtype == dtype and hc.same_floats(got, want)
        for mode in ("reference", "cell"):
            pts, it = sc.good_points(name, mode)
            got, want = both(name, pts, mode, item=it, normalize=normalize, dtype=dtype)
            assert hc.same_floats(got, want)
    # ... and the twin is the dense twin at those texels (test_hypercolumn_sparse_cpu.py): close the loop once
    got, _ = both(name, tex, "texel", item=item, normalize=normalize)
    assert hc.same_floats(got, sc.expected(name, item, tex[:, 0], tex[:, 1], np.ones(len(tex), bool), normalize)[0])


@pytest.mark.parametrize("name", ["vgg16x", "batch3", sc.BIG])
def test_gpu_row_counts_and_independence(name):
    """N = 1, 63, 64, 65 and 257 rows (with repeats) equal the twin; a permutation permutes the rows."""
    tex, item = sc.all_texels(name)
    rng = np.random.Generator(np.random.PCG64(11))
    pick = rng.integers(0, len(tex), 257)
    tex, item = tex[pick], item[pick]
    base, want = both(name, tex, "texel", item=item)
    assert hc.same_floats(base, want)
    perm = rng.permutation(257)
    assert hc.same_floats(both(name, tex[perm], "texel", item=item[perm])[0], base[perm])
    for n in sc.SUBSETS:
        assert hc.same_floats(both(name, tex[:n], "texel", item=item[:n])[0], base[:n])


def test_gpu_many_rows_in_one_launch():
    """The ten-reference case's row count and beyond the grid's cap: 70 000 rows over three items."""
    name = "batch3"
    tex, item = sc.all_texels(name)
    pick = np.random.Generator(np.random.PCG64(12)).integers(0, len(tex), 70000)
    got, want = both(name, tex[pick], "texel", item=item[pick])
    assert hc.same_floats(got, want)


@pytest.mark.parametrize("name", ["ragged3", "vgg16x", "sized", "wide"])
def test_gpu_equals_assemble_then_gather(name):
    """The identity the feature rests on: assemble_hypercolumn followed by the existing device gathers
    (fmpnp.refine.gather_reference, fast_sparse_keypoint_descriptor) gives the same bits."""
    maps, size = sc.inputs(name)
    _, C, H, W = sc.shape(name)
    dense = fmpnp.assemble_hypercolumn(dev(name), size=size)
    for storage in (torch.float32, torch.float64):
        pts, _ = sc.good_points(name, "reference")
        want = gather_reference(dense, pts, sc.image_shape(name), cstride=C, storage=storage)
        got = fmpnp.sparse_hypercolumn(dev(name), pts, at="reference", image_shape=sc.image_shape(name), size=size,
                                       dtype=storage)
        assert hc.same_floats(got.cpu(), want.cpu())
    pts, _ = sc.good_points(name, "cell")
    grid, cell = generate_dense_keypoints((H, W), sc.cell_resolution(name))
    want = fast_sparse_keypoint_descriptor([pts.T], grid, dense)[0]
    got = fmpnp.sparse_hypercolumn(dev(name), pts, at="cell", cell_size=cell, size=size)
    assert hc.same_floats(got.cpu(), want.cpu())


def test_gpu_bad_points_give_zero_rows_and_index_error():
    """Ordinary validation on the device: error rows are zero, the flag raises IndexError, the other rows are
    the twin's; gather_reference raises for the same points; at="cell" never errors."""
    name = "batch3"
    B, C, H, W = sc.shape(name)
    good, item = sc.good_points(name, "reference")
    pts = np.concatenate([sc.bad_points(name), good])
    item = np.concatenate([np.zeros(len(sc.bad_points(name)), np.int32), item])
    item[-1], item[-2] = B, -1
    want = torch.full((len(pts), C), -7.0)
    with pytest.raises(IndexError):
        fmpnp.sparse_hypercolumn_cpu(sc.inputs(name)[0], pts, item=item, out=want, **sc.kwargs(name, "reference"))
    out = torch.full((len(pts), C), -7.0, device=DEV)
    with pytest.raises(IndexError):
        fmpnp.sparse_hypercolumn(dev(name), pts, item=item, out=out, **sc.kwargs(name, "reference"))
    assert hc.same_floats(out.cpu(), want) and int((want == 0).all(1).sum()) == len(sc.bad_points(name)) + 2
    with pytest.raises(IndexError):
        gather_reference(fmpnp.assemble_hypercolumn(dev(name))[0], pts, sc.image_shape(name))
    tex = np.array([(0, 0), (H, 0), (0, W), (-1, 0), (0, -1), (H - 1, W - 1)], np.int32)
    out = torch.full((len(tex), C), -7.0, device=DEV)
    with pytest.raises(IndexError):
        fmpnp.sparse_hypercolumn(dev(name), tex, at="texel", out=out)
    row, col, ok = sc.index(name, "texel", tex)
    assert hc.same_floats(out.cpu(), sc.expected(name, None, row, col, ok)[0])
    wild = np.array([(np.nan, np.nan), (1e300, -1e300), (-5.0, 1e9), (np.inf, -np.inf)], np.float64)
    got, twin = both(name, wild, "cell")
    assert hc.same_floats(got, twin)
    # the library stays usable, and the next call starts from a clean flag
    got, twin = both(name, good, "reference")
    assert hc.same_floats(got, twin)


def _strided_on_device(maps):
    """The views case's sources on the device with their strides: the wider tensors are rebuilt there."""
    out = []
    for m in maps:
        big = torch.full((3, m.shape[1] + 2, m.shape[2] + 1, m.shape[3] + 3), float("nan"), device=DEV)
        view = big[1:, 1:m.shape[1] + 1, :m.shape[2], 2:2 + m.shape[3]]
        view.copy_(m)
        assert view.stride() == m.stride() and not view.is_contiguous()
        out.append(view)
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_gpu_views(dtype):
    """B = 2, strided sources, an out= view with ld_out = C + 3 inside a larger prefilled buffer: the view equals
    the twin, every other element keeps the fill; N = 0 writes nothing."""
    name = "views"
    maps, _ = sc.inputs(name)
    _, C, _, _ = sc.shape(name)
    tex, item = sc.all_texels(name)
    n = len(tex)
    buf = torch.full((1 + n * (C + 3) + 5,), -7.0, dtype=dtype, device=DEV)
    view = buf[1:1 + n * (C + 3)].view(n, C + 3)[:, :C]
    got = fmpnp.sparse_hypercolumn(_strided_on_device(maps), tex, at="texel", item=item, dtype=dtype, out=view)
    assert got.data_ptr() == view.data_ptr()
    want = fmpnp.sparse_hypercolumn_cpu(maps, tex, at="texel", item=item, dtype=dtype)
    assert hc.same_floats(view.cpu(), want)
    view.fill_(-7.0)
    assert bool((buf == -7.0).all())
    empty = fmpnp.sparse_hypercolumn(_strided_on_device(maps), np.zeros((0, 2), np.int32), at="texel", dtype=dtype)
    assert tuple(empty.shape) == (0, C)
    assert bool((buf == -7.0).all())


def test_gpu_side_stream_and_two_runs():
    name = "vgg16x"
    pts, _ = sc.good_points(name, "reference")
    kw = sc.kwargs(name, "reference")
    base = fmpnp.sparse_hypercolumn(dev(name), pts, **kw)
    again = fmpnp.sparse_hypercolumn(dev(name), pts, **kw)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    got = fmpnp.sparse_hypercolumn(dev(name), pts, stream=side, **kw)
    cells, _ = sc.good_points(name, "cell")
    cell = fmpnp.sparse_hypercolumn(dev(name), cells, stream=side, **sc.kwargs(name, "cell"))  # (asynchronous)
    side.synchronize()
    assert torch.equal(base, again) and torch.equal(got, base)
    assert hc.same_floats(cell.cpu(), fmpnp.sparse_hypercolumn_cpu(sc.inputs(name)[0], cells, **sc.kwargs(name, "cell")))


def test_gpu_argument_errors():
    m = torch.zeros(1, 2, 3, 3, device=DEV)
    tex = np.zeros((1, 2), np.int32)
    with pytest.raises(ValueError):
        fmpnp.sparse_hypercolumn([m.cpu()], tex, at="texel")
    with pytest.raises(ValueError):
        fmpnp.sparse_hypercolumn([m], tex, at="texel", out=torch.zeros(1, 3, device=DEV))
    with pytest.raises(ValueError):
        fmpnp.sparse_hypercolumn([m], tex, at="texel", out=torch.zeros(1, 2))
    with pytest.raises(ValueError):
        fmpnp.sparse_hypercolumn([m], np.zeros((1, 2)), at="reference")
    with pytest.raises(fmpnp._lib.FmpnpError):
        fmpnp.sparse_hypercolumn([m], np.zeros((1, 2)), at="cell", cell_size=(0.0, 1.0))


# ---- feature_pnp with the reference given as layers ----------------------------------------------------------

Pred = namedtuple("Prediction", "points_3d reference_inliers matrix quaternion reference_filename")
PYRAMID = [(16, 32, None, None), (8, 16, None, None), (0, 8, None, None)]


@functools.lru_cache(maxsize=None)
def pnp_scene(init="easy", N=40):
    """localize_cases' sizes (C = 32, a 16 x 16 map, image 64 x 64): the query, the reference's layers -- the
    query map's channels 0..15 at full size, 16..23 at full size, 24..31 at half size -- the prediction, K."""
    (batch,), img = synth.pipeline_queries(1, 1, N, lc.C, lc.W, lc.H, device=DEV, seed0=31, init=init)
    q, _, p, K = batch[0]
    assert img == lc.IMAGE
    layers = [q[None, :16].contiguous(), q[None, 16:24].contiguous(),
              torch.nn.functional.avg_pool2d(q[None, 24:], 2).contiguous()]
    pred = Pred(p.points_3d, p.reference_inliers, p.matrix, np.array([1.0, 0, 0, 0]), "ref.png")
    return q[None], layers, pred, K, img


def run_pnp(one_call, monkeypatch, q, ref, layers, pred, K, img, **kw):
    """feature_pnp, with a spy on which path it took."""
    called = []
    real = ofp._feature_pnp_one_call

    def spy(*a, **k):
        called.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ofp, "_feature_pnp_one_call", spy)
    try:
        out = fmpnp.feature_pnp(q, ref, pred, K, img, reference_layers=layers, **kw)
    finally:
        monkeypatch.undo()
    assert bool(called) == one_call
    return out


def same_refinement(a, b):
    (Ra, ta, ma), (Rb, tb, mb) = a, b
    assert torch.equal(Ra, Rb) and torch.equal(ta, tb)
    for k in ("initial_cost_", "best_cost_"):
        va, vb = getattr(ma, k, None), getattr(mb, k, None)
        assert (va is None) == (vb is None), k
        if va is not None:
            assert torch.equal(va, vb), k
    assert getattr(ma, "best_num_inliers_", None) == getattr(mb, "best_num_inliers_", None)
    assert ma.status_ == mb.status_ == 0


@pytest.mark.parametrize("storage", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("pyramid", [None, PYRAMID], ids=["flat", "pyramid"])
def test_feature_pnp_with_layers_equals_the_assembled_map(pyramid, storage, monkeypatch):
    """The one-call path (fmpnp_feature_pnp_layers against fmpnp_feature_pnp on assemble_hypercolumn's map):
    R, t, initial_cost_, best_cost_ and best_num_inliers_ bit for bit."""
    q, layers, pred, K, img = pnp_scene()
    dense = fmpnp.assemble_hypercolumn(layers)
    mk = lambda: fmpnp.sparseFeaturePnP(20, loss_fn=fmpnp.geman_mcclure_loss, lambda_=0.01, storage=storage)  # noqa: E731
    a = run_pnp(True, monkeypatch, q, None, layers, pred, K, img, feature_pyramid=pyramid, model=mk(), window=0)
    b = run_pnp(True, monkeypatch, q, dense, None, pred, K, img, feature_pyramid=pyramid, model=mk(), window=0)
    same_refinement(a, b)


def test_feature_pnp_with_layers_through_the_window_rerun(monkeypatch):
    """window = 1 from a start 20 degrees and a metre off (the outer points sit two texels and more from where
    the refinement takes them): a point leaves its window, the call runs again fully packed, and the reference
    rows are formed again from the layers."""
    q, layers, pred, K, img = pnp_scene("hard", 200)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = synth.rot_z(20.0), (1.0, -0.8, 0.5)
    pred = pred._replace(matrix=T)
    dense = fmpnp.assemble_hypercolumn(layers)
    mk = lambda: fmpnp.sparseFeaturePnP(30, loss_fn=fmpnp.geman_mcclure_loss, lambda_=0.01)  # noqa: E731
    L = _lib.load()
    before = L.fmpnp_feature_pnp_reruns()
    a = run_pnp(True, monkeypatch, q, None, layers, pred, K, img, feature_pyramid=PYRAMID, model=mk(), window=1)
    reruns = L.fmpnp_feature_pnp_reruns() - before
    print(f"window re-runs of the layers call: {reruns}")
    assert reruns == 1
    b = run_pnp(True, monkeypatch, q, dense, None, pred, K, img, feature_pyramid=PYRAMID, model=mk(), window=1)
    c = run_pnp(True, monkeypatch, q, dense, None, pred, K, img, feature_pyramid=PYRAMID, model=mk(), window=0)
    same_refinement(a, b)
    same_refinement(a, c)


def test_feature_pnp_with_layers_on_the_step_by_step_path(monkeypatch):
    """track=True with the ratio test takes the step-by-step path: sparse_hypercolumn in place of
    gather_reference."""
    q, layers, pred, K, img = pnp_scene()
    dense = fmpnp.assemble_hypercolumn(layers)
    def mk():
        return fmpnp.sparseFeaturePnP(20, loss_fn=fmpnp.geman_mcclure_loss, lambda_=0.01, ratio_threshold=0.8)
    for pyramid in (None, PYRAMID):
        a = run_pnp(False, monkeypatch, q, None, layers, pred, K, img, feature_pyramid=pyramid, model=mk(), track=True)
        b = run_pnp(False, monkeypatch, q, dense, None, pred, K, img, feature_pyramid=pyramid, model=mk(), track=True)
        same_refinement(a, b)
        assert [float(x) for x in a[2].track_["costs"]] == [float(x) for x in b[2].track_["costs"]]


def test_feature_pnp_with_layers_raises_the_same_index_error(monkeypatch):
    q, layers, pred, K, img = pnp_scene()
    dense = fmpnp.assemble_hypercolumn(layers)
    inl = np.array(pred.reference_inliers, dtype=np.float64)
    inl[7] = (1e6, 5.0)
    bad = pred._replace(reference_inliers=inl)
    ratio = dict(ratio_threshold=0.8)
    for kw, model_kw in ((dict(), dict()), (dict(track=True), ratio)):  # (one call; step by step)
        for ref, lay in ((None, layers), (dense, None)):
            with pytest.raises(IndexError):
                fmpnp.feature_pnp(q, ref, bad, K, img, reference_layers=lay, model=fmpnp.sparseFeaturePnP(5, **model_kw),
                                  **kw)
    with pytest.raises(ValueError):
        fmpnp.feature_pnp(q, None, pred, K, img, model=fmpnp.sparseFeaturePnP(5))
    R, t, m = fmpnp.feature_pnp(q, None, pred, K, img, reference_layers=layers, model=fmpnp.sparseFeaturePnP(5))
    assert m.status_ == 0  # (the library stays usable after the error)


def test_optimize_feature_pnp_sparse_reference():
    """sparse_reference=True equals the default with a HypercolumnExtractor as net; a net without
    compute_feature_maps is a TypeError."""
    net, image = hc.tiny_encoder().to(DEV), hc.tiny_image().to(DEV)
    ex = fmpnp.HypercolumnExtractor(net, hc.ENCODER_LAYERS, image_loader=lambda paths, size, resize, device: image)
    query, resolution = ex.compute_hypercolumn(image)  # [1, 32, 20, 28]: the query is the reference image
    Hf, Wf = query.shape[2:]
    X, K, W, H = synth.scene(60, Hf, Wf, 5)
    p = fmpnp.refine.project_pixels(np.eye(3), np.zeros(3), X, K)
    rows, cols = (p[:, 1].astype(np.int64) * Hf) // H, (p[:, 0].astype(np.int64) * Wf) // W
    inl = np.stack([(cols + 0.5) * W / Hf, (rows + 0.5) * H / Wf], 1)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = synth.INITS["easy"]
    pred = Pred(X, inl, T, np.array([1.0, 0, 0, 0]), "ref.png")
    pyr = [(16, 32, None, None), (0, 16, None, None)]
    out = []
    for sparse in (False, True):
        model = fmpnp.sparseFeaturePnP(20, loss_fn=fmpnp.geman_mcclure_loss, lambda_=0.01)
        out.append(fmpnp.optimize_feature_pnp(query, ex, pred, K, image_shape=(W, H), feature_pyramid=pyr, model=model,
                                              verbose=False, sparse_reference=sparse))
    (ta, qa, ma), (tb, qb, mb) = out
    lc.equal(ta, tb, "t")
    lc.equal(qa, qb, "quaternion")
    assert torch.equal(ma.best_cost_, mb.best_cost_) and torch.equal(ma.initial_cost_, mb.initial_cost_)
    assert ma.best_num_inliers_ == mb.best_num_inliers_ and ma.status_ == mb.status_ == 0

    class Dense:
        compute_hypercolumn = ex.compute_hypercolumn
    with pytest.raises(TypeError):
        fmpnp.optimize_feature_pnp(query, Dense(), pred, K, image_shape=(W, H), feature_pyramid=pyr, verbose=False,
                                   sparse_reference=True)


# ---- the localisation chain with references carrying feature_maps --------------------------------------------

@functools.lru_cache(maxsize=None)
def layered_scene(name):
    """A scene of localize_cases whose references are all dense: (query, references carrying the assembled
    hypercolumn, the same references carrying feature_maps).  The layers are one batched pass over the
    references -- channels 0..19 and 20..31 of each reference map at full size -- told apart by feature_item."""
    scene = lc.scene(name)
    maps = torch.from_numpy(np.stack([r["hypercolumn"] for r in scene["references"]])).to(DEV)
    layers = [maps[:, :20].contiguous(), maps[:, 20:].contiguous()]
    dense = fmpnp.assemble_hypercolumn(layers)
    with_map, with_layers = [], []
    for j, r in enumerate(scene["references"]):
        r = lc.public(r)
        assert "sparse_descriptors" not in r
        del r["hypercolumn"]
        with_map.append(dict(r, hypercolumn=dense[j]))
        with_layers.append(dict(r, feature_maps=layers, feature_item=j))
    return torch.from_numpy(scene["query"]).to(DEV), with_map, with_layers


def equal_localization(a, b):
    lc.equal(a.export, b.export, "export")
    lc.equal_prediction(a.prediction, b.prediction, "best")
    assert a.kind == b.kind and a.best == b.best
    assert len(a.predictions) == len(b.predictions)
    for j, (x, y) in enumerate(zip(a.predictions, b.predictions)):
        lc.equal_prediction(x, y, f"pair {j}")
        for k in replay.ENTRY_KEYS:
            lc.equal(a.cached_matches[j][k], b.cached_matches[j][k], f"cached {j}.{k}")
    assert (a.refined is None) == (b.refined is None)
    if a.refined is not None:
        lc.equal(a.refined[0], b.refined[0], "t")
        lc.equal(a.refined[1], b.refined[1], "quaternion")
        for k in ("initial_cost_", "best_cost_", "best_num_inliers_"):
            x, y = getattr(a.refined[2], k, None), getattr(b.refined[2], k, None)
            assert (x is None) == (y is None), k
            if x is not None:
                lc.equal(x.cpu().numpy() if torch.is_tensor(x) else x, y.cpu().numpy() if torch.is_tensor(y) else y, k)


@pytest.mark.parametrize("refine", [False, True], ids=["unrefined", "refined"])
def test_localize_with_feature_maps_equals_the_assembled_maps(refine):
    """Three references, one of them a fallback, one solved: every Localization field, refined too."""
    q, with_map, with_layers = layered_scene("fallback_loses")
    assert len(with_map) >= 3 and any(r.get("fallback_pose") is not None for r in with_map)
    kw = dict(factor=lc.FACTOR, refine=refine, return_all=True, return_masked=True, **lc.PNP)
    a = fmpnp.localize(q, with_layers, lc.IMAGE, **kw)
    b = fmpnp.localize(q, with_map, lc.IMAGE, **kw)
    assert b.kind == "solved" and (b.refined is not None) == refine
    equal_localization(a, b)


def test_localize_multi_with_feature_maps_equals_the_assembled_maps():
    qa, map_a, lay_a = layered_scene("fallback_loses")
    qb, map_b, lay_b = layered_scene("fallback_wins")
    kw = dict(factor=lc.FACTOR, refine=True, return_all=True, return_masked=True, **lc.PNP)
    a = fmpnp.localize_multi([(qa, lay_a), (qb, lay_b)], lc.IMAGE, **kw)
    b = fmpnp.localize_multi([(qa, map_a), (qb, map_b)], lc.IMAGE, **kw)
    assert [x.kind for x in b] == ["solved", "fallback"]
    for x, y in zip(a, b):
        equal_localization(x, y)
