"""The fused hypercolumn pack on the GPU (fmpnp.pack_hypercolumn, feature_pnp(query_layers=...)): the device result
against the CPU twin and against the composed path on the device, pack_features(assemble_hypercolumn(layers)).
Every comparison is an equality (NaNs by position); buffers are prefilled with a sentinel so that a write outside
the named channels and texels shows."""
import functools

import numpy as np
import pytest
import torch

import fmpnp
from fmpnp import _lib, synth

import hypercolumn_cases as hc
import hypercolumn_pack_cases as pc
import localize_cases as lc
import test_gpu_hypercolumn_sparse as ts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ofp = ts.ofp  # (the module: the package attribute of that name is the function)


@functools.lru_cache(maxsize=None)
def dev(name):
    return [m.to(DEV) for m in pc.inputs(name)[0]]


def packed(name, maps=None, item=0, marks=None, out=None, **kw):
    """pack_hypercolumn into a buffer prefilled with the sentinel -> the buffer on the host (numpy)."""
    _, H, W, cs = pc.shape(name)
    layout, storage = kw.get("layout", "fgrad"), kw.get("storage", torch.float32)
    if out is None:
        out = torch.full((H, W, 3, cs) if layout == "fgrad" else (H, W, cs), pc.SENTINEL, dtype=storage, device=DEV)
    m = pc.marks_of(name, marks)
    got = fmpnp.pack_hypercolumn(dev(name) if maps is None else maps, size=pc.inputs(name)[1], item=item, out=out,
                                 marks=None if m is None else torch.from_numpy(m).to(DEV), **kw)
    assert got.buf.data_ptr() == out.data_ptr() and (got.C, got.H, got.W, got.cstride) == pc.shape(name)
    return out.cpu().numpy()


@pytest.mark.parametrize("name", pc.ALL)
def test_gpu_equals_the_twin(name):
    """Every case and batch item, both layouts, the four Sobel flag pairs, both storages, with and without the
    normalisation."""
    for item in pc.items(name):
        for normalize in (True, False):
            assert pc.same(packed(name, item=item, normalize=normalize, layout="f"),
                           pc.twin(name, item, normalize, "f")), (item, normalize, "f")
            for sn, rp in pc.FLAG_PAIRS:
                for storage in (torch.float32, torch.float64):
                    got = packed(name, item=item, normalize=normalize, sobel_normalized=sn, sobel_replicate_pad=rp,
                                 storage=storage)
                    assert pc.same(got, pc.twin(name, item, normalize, "fgrad", sn, rp, storage)), (
                        item, normalize, sn, rp, storage)


@pytest.mark.parametrize("layout", ["fgrad", "f"])
@pytest.mark.parametrize("name", ["ragged3", "blocks", "wide", "vec", "vgg16x", "sized", "cols33", "rows", "one", "c30",
                                  "zero_texel", "nonfinite"])
def test_gpu_equals_pack_features_of_the_assembled_map(name, layout):
    """The defining property on the device: the same buffer as the composed path's, padding channels included
    (both allocate them as zeros)."""
    maps, size = dev(name), pc.inputs(name)[1]
    dense = fmpnp.assemble_hypercolumn(maps, size=size)
    for kw in (dict(), dict(sobel_normalized=True, sobel_replicate_pad=True)):
        want = fmpnp.pack_features(dense[0], layout=layout, **kw)
        got = fmpnp.pack_hypercolumn(maps, size=size, layout=layout, **kw)
        assert (got.C, got.H, got.W, got.cstride, got.layout, got.sobel_flags) == (
            want.C, want.H, want.W, want.cstride, want.layout, want.sobel_flags)
        assert hc.same_floats(got.buf.cpu(), want.buf.cpu()), kw
    if layout == "fgrad":
        want = fmpnp.pack_features(dense[0], storage=torch.float64)
        got = fmpnp.pack_hypercolumn(maps, size=size, storage=torch.float64)
        assert got.buf.dtype == torch.float64 and hc.same_floats(got.buf.cpu(), want.buf.cpu())


@pytest.mark.parametrize("layout", ["fgrad", "f"])
@pytest.mark.parametrize("name,channels", pc.RANGES)
def test_gpu_channel_ranges(name, channels, layout):
    got = packed(name, channels=channels, layout=layout, sobel_replicate_pad=True)
    assert pc.same(got, pc.twin(name, layout=layout, replicate=True, channels=channels))


@pytest.mark.parametrize("layout", ["fgrad", "f"])
@pytest.mark.parametrize("name", ["cols33", "rows", "blocks", "one", "wide", "vgg16x"])
def test_gpu_marks(name, layout):
    """Only marked texels are written -- also by a launch whose norm plane was formed near the marks only."""
    for kind in pc.MARK_KINDS:
        assert pc.same(packed(name, marks=kind, layout=layout), pc.twin(name, layout=layout, marks=kind)), kind
    C = pc.shape(name)[0]
    rng = (1, min(C, 3))
    assert pc.same(packed(name, marks="random", channels=rng, layout=layout, storage=torch.float32),
                   pc.twin(name, layout=layout, channels=rng, marks="random"))


@pytest.mark.parametrize("storage", [torch.float32, torch.float64])
def test_gpu_strided_sources_and_a_padded_out_view(storage):
    """B = 2 with storage offsets and batch, channel and row strides; the output a view inside a larger prefilled
    buffer whose surroundings stay as they are."""
    name = "views"
    C, H, W, cs = pc.shape(name)
    maps = ts._strided_on_device(pc.inputs(name)[0])
    n = H * W * 3 * cs
    for item in pc.items(name):
        buf = torch.full((4 + n + 6,), pc.SENTINEL, dtype=storage, device=DEV)
        view = buf[4:4 + n].view(H, W, 3, cs)
        got = packed(name, maps=maps, item=item, out=view, storage=storage)
        assert pc.same(got, pc.twin(name, item, storage=storage))
        view.fill_(pc.SENTINEL)
        assert bool((buf == pc.SENTINEL).all())


def test_gpu_side_stream_and_two_runs():
    name = "vgg16x"
    base = packed(name)
    again = packed(name)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    _, H, W, cs = pc.shape(name)
    with torch.cuda.stream(side):
        out = torch.full((H, W, 3, cs), pc.SENTINEL, device=DEV)
    got = fmpnp.pack_hypercolumn(dev(name), out=out, stream=side)
    rest = fmpnp.pack_hypercolumn(dev(name), out=out, stream=side, channels=(0, 128), sobel_normalized=True)
    side.synchronize()
    assert np.array_equal(base, again) and pc.same(base, pc.twin(name))
    want = np.array(pc.twin(name))
    want[..., :128] = pc.twin(name, sobel_normalized=True, channels=(0, 128))[..., :128]
    assert got.buf.data_ptr() == rest.buf.data_ptr() and pc.same(out.cpu().numpy(), want)


def test_gpu_argument_errors():
    m = torch.zeros(1, 2, 3, 3, device=DEV)
    for kw in (dict(layout="x"), dict(storage=torch.float16), dict(layout="f", storage=torch.float64), dict(item=1),
               dict(channels=(1, 1)), dict(channels=(0, 3)), dict(marks=torch.zeros(2, 3, dtype=torch.uint8, device=DEV)),
               dict(marks=torch.zeros(3, 3, device=DEV)), dict(marks=torch.zeros(3, 3, dtype=torch.uint8)),
               dict(out=torch.zeros(3, 3, 3, 4, dtype=torch.float64, device=DEV)), dict(out=torch.zeros(3, 3, 3, 4)),
               dict(out=torch.zeros(3, 3, 3, 8, device=DEV)[..., :4])):
        with pytest.raises(ValueError):
            fmpnp.pack_hypercolumn([m], **kw)
    with pytest.raises(ValueError):
        fmpnp.pack_hypercolumn([m.cpu()])


# ---- feature_pnp with the query given as layers ---------------------------------------------------------------

def run_pnp(one_call, monkeypatch, query, query_layers, ref, ref_layers, pred, K, img, **kw):
    """feature_pnp, with a spy on which path it took."""
    called = []
    real = ofp._feature_pnp_one_call

    def spy(*a, **k):
        called.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ofp, "_feature_pnp_one_call", spy)
    try:
        out = fmpnp.feature_pnp(query, ref, pred, K, img, reference_layers=ref_layers, query_layers=query_layers, **kw)
    finally:
        monkeypatch.undo()
    assert bool(called) == one_call
    return out


def model(iters=20, **kw):
    return fmpnp.sparseFeaturePnP(iters, loss_fn=fmpnp.geman_mcclure_loss, lambda_=0.01, **kw)


@pytest.mark.parametrize("storage", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("pyramid", [None, ts.PYRAMID], ids=["flat", "pyramid"])
def test_feature_pnp_with_query_layers_equals_the_assembled_map(pyramid, storage, monkeypatch):
    """The one-call path (fmpnp_feature_pnp_query_layers against fmpnp_feature_pnp on assemble_hypercolumn's map):
    R, t, initial_cost_, best_cost_ and best_num_inliers_ bit for bit."""
    ref, layers, pred, K, img = ts.pnp_scene()
    dense = fmpnp.assemble_hypercolumn(layers)
    kw = dict(feature_pyramid=pyramid, window=0)
    a = run_pnp(True, monkeypatch, None, layers, ref, None, pred, K, img, model=model(storage=storage), **kw)
    b = run_pnp(True, monkeypatch, dense, None, ref, None, pred, K, img, model=model(storage=storage), **kw)
    ts.same_refinement(a, b)


def test_feature_pnp_with_query_layers_in_the_f_layout(monkeypatch):
    ref, layers, pred, K, img = ts.pnp_scene()
    dense = fmpnp.assemble_hypercolumn(layers)
    kw = dict(feature_pyramid=ts.PYRAMID, layout="f")
    a = run_pnp(True, monkeypatch, None, layers, ref, None, pred, K, img, model=model(), **kw)
    b = run_pnp(True, monkeypatch, dense, None, ref, None, pred, K, img, model=model(), **kw)
    ts.same_refinement(a, b)


@pytest.mark.parametrize("pyramid", [None, ts.PYRAMID], ids=["flat", "pyramid"])
def test_feature_pnp_with_layers_on_both_sides(pyramid, monkeypatch):
    """query_layers and reference_layers: no dense map on either side."""
    _, layers, pred, K, img = ts.pnp_scene()
    dense = fmpnp.assemble_hypercolumn(layers)
    kw = dict(feature_pyramid=pyramid, window=0)
    a = run_pnp(True, monkeypatch, None, layers, None, layers, pred, K, img, model=model(), **kw)
    b = run_pnp(True, monkeypatch, dense, None, dense, None, pred, K, img, model=model(), **kw)
    ts.same_refinement(a, b)


def test_feature_pnp_with_query_layers_through_the_window_rerun(monkeypatch):
    """window = 1 from the hard start: a point leaves its window and the call runs again fully packed, with the
    norm plane formed again over the whole map."""
    ref, layers, pred, K, img = ts.pnp_scene("hard", 200)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = synth.rot_z(20.0), (1.0, -0.8, 0.5)
    pred = pred._replace(matrix=T)
    dense = fmpnp.assemble_hypercolumn(layers)
    L = _lib.load()
    before = L.fmpnp_feature_pnp_reruns()
    a = run_pnp(True, monkeypatch, None, layers, ref, None, pred, K, img, feature_pyramid=ts.PYRAMID, model=model(30),
                window=1)
    reruns = L.fmpnp_feature_pnp_reruns() - before
    print(f"window re-runs of the query-layers call: {reruns}")
    assert reruns == 1
    b = run_pnp(True, monkeypatch, dense, None, ref, None, pred, K, img, feature_pyramid=ts.PYRAMID, model=model(30),
                window=1)
    c = run_pnp(True, monkeypatch, dense, None, ref, None, pred, K, img, feature_pyramid=ts.PYRAMID, model=model(30),
                window=0)
    ts.same_refinement(a, b)
    ts.same_refinement(a, c)
    # a window wide enough: no re-run, the same bits
    before = L.fmpnp_feature_pnp_reruns()
    ref, layers, pred, K, img = ts.pnp_scene()
    dense = fmpnp.assemble_hypercolumn(layers)
    d = run_pnp(True, monkeypatch, None, layers, ref, None, pred, K, img, feature_pyramid=ts.PYRAMID, model=model(),
                window=6)
    assert L.fmpnp_feature_pnp_reruns() == before
    e = run_pnp(True, monkeypatch, dense, None, ref, None, pred, K, img, feature_pyramid=ts.PYRAMID, model=model(),
                window=0)
    ts.same_refinement(d, e)


def test_feature_pnp_with_query_layers_on_the_step_by_step_path(monkeypatch):
    """track=True with the ratio test takes the step-by-step path: pack_hypercolumn in place of pack_features."""
    ref, layers, pred, K, img = ts.pnp_scene()
    dense = fmpnp.assemble_hypercolumn(layers)
    for pyramid in (None, ts.PYRAMID):
        kw = dict(feature_pyramid=pyramid, track=True)
        a = run_pnp(False, monkeypatch, None, layers, ref, None, pred, K, img, model=model(ratio_threshold=0.8), **kw)
        b = run_pnp(False, monkeypatch, dense, None, ref, None, pred, K, img, model=model(ratio_threshold=0.8), **kw)
        ts.same_refinement(a, b)
        assert [float(x) for x in a[2].track_["costs"]] == [float(x) for x in b[2].track_["costs"]]
    # a resized level is cut from the dense map: that path assembles it, with the same results
    pyramid = [(16, 32, 8, None), (0, 32, None, None)]
    a = run_pnp(False, monkeypatch, None, layers, ref, None, pred, K, img, feature_pyramid=pyramid, model=model())
    b = run_pnp(False, monkeypatch, dense, None, ref, None, pred, K, img, feature_pyramid=pyramid, model=model())
    ts.same_refinement(a, b)


@functools.lru_cache(maxsize=None)
def wide_scene(C, cuts, N=40):
    """ts.pnp_scene's sizes with C channels: the reference map, its layers (cut at `cuts`, the last one at half
    size), the prediction, K."""
    (batch,), img = synth.pipeline_queries(1, 1, N, C, lc.W, lc.H, device=DEV, seed0=47, init="easy")
    q, _, p, K = batch[0]
    a, b = cuts
    layers = [q[None, :a].contiguous(), q[None, a:b].contiguous(),
              torch.nn.functional.avg_pool2d(q[None, b:], 2).contiguous()]
    pred = ts.Pred(p.points_3d, p.reference_inliers, p.matrix, np.array([1.0, 0, 0, 0]), "ref.png")
    return q[None], layers, pred, K, img


@pytest.mark.parametrize("window", [0, 6])
def test_feature_pnp_with_query_layers_takes_the_two_stream_split(window, monkeypatch):
    """C = 96 with levels (32, 96), (0, 32): the first level's channels are packed on the main stream, the rest on
    the side stream, both from the one norm plane."""
    ref, layers, pred, K, img = wide_scene(96, (40, 72))
    dense = fmpnp.assemble_hypercolumn(layers)
    kw = dict(feature_pyramid=[(32, 96, None, None), (0, 32, None, None)], window=window)
    a = run_pnp(True, monkeypatch, None, layers, ref, None, pred, K, img, model=model(), **kw)
    b = run_pnp(True, monkeypatch, dense, None, ref, None, pred, K, img, model=model(), **kw)
    ts.same_refinement(a, b)


@pytest.mark.parametrize("layout", ["fgrad", "f"])
def test_feature_pnp_with_query_layers_of_30_channels(layout, monkeypatch):
    """cstride 32 > C = 30: the padding channels are zeroed by the call, not by the pack."""
    ref, layers, pred, K, img = wide_scene(30, (12, 20))
    dense = fmpnp.assemble_hypercolumn(layers)
    for pyramid in (None, [(16, 30, None, None), (0, 16, None, None)]):
        kw = dict(feature_pyramid=pyramid, layout=layout)
        a = run_pnp(True, monkeypatch, None, layers, ref, None, pred, K, img, model=model(), **kw)
        b = run_pnp(True, monkeypatch, dense, None, ref, None, pred, K, img, model=model(), **kw)
        ts.same_refinement(a, b)


def test_feature_pnp_query_layers_argument_errors():
    ref, layers, pred, K, img = ts.pnp_scene()
    with pytest.raises(ValueError):
        fmpnp.feature_pnp(ref, ref, pred, K, img, query_layers=layers, model=model(5))
    with pytest.raises(ValueError):
        fmpnp.feature_pnp(None, None, pred, K, img, query_layers=layers, model=model(5))
    with pytest.raises(ValueError):
        fmpnp.feature_pnp(None, ref, pred, K, img, query_layers=[m.cpu() for m in layers], model=model(5))
    with pytest.raises(ValueError):
        fmpnp.feature_pnp(None, ref, pred, K, img, query_layers=[m.repeat(2, 1, 1, 1) for m in layers], model=model(5))
    R, t, m = fmpnp.feature_pnp(None, ref, pred, K, img, query_layers=layers, model=model(5))
    assert m.status_ == 0


def test_optimize_feature_pnp_with_query_layers_and_a_sparse_reference():
    """query_layers with sparse_reference=True (no dense map on either side) equals the default."""
    net, image = hc.tiny_encoder().to(DEV), hc.tiny_image().to(DEV)
    ex = fmpnp.HypercolumnExtractor(net, hc.ENCODER_LAYERS, image_loader=lambda paths, size, resize, device: image)
    query, _ = ex.compute_hypercolumn(image)  # [1, 32, 20, 28]: the query is the reference image
    query_layers, _ = ex.compute_feature_maps(image)
    Hf, Wf = query.shape[2:]
    X, K, W, H = synth.scene(60, Hf, Wf, 5)
    p = fmpnp.refine.project_pixels(np.eye(3), np.zeros(3), X, K)
    rows, cols = (p[:, 1].astype(np.int64) * Hf) // H, (p[:, 0].astype(np.int64) * Wf) // W
    inl = np.stack([(cols + 0.5) * W / Hf, (rows + 0.5) * H / Wf], 1)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = synth.INITS["easy"]
    pred = ts.Pred(X, inl, T, np.array([1.0, 0, 0, 0]), "ref.png")
    pyr = [(16, 32, None, None), (0, 16, None, None)]
    out = []
    for kw in (dict(), dict(query_layers=query_layers, sparse_reference=True), dict(query_layers=query_layers)):
        out.append(fmpnp.optimize_feature_pnp(None if kw else query, ex, pred, K, image_shape=(W, H), feature_pyramid=pyr,
                                              model=model(), verbose=False, **kw))
    (ta, qa, ma) = out[0]
    for tb, qb, mb in out[1:]:
        lc.equal(ta, tb, "t")
        lc.equal(qa, qb, "quaternion")
        assert torch.equal(ma.best_cost_, mb.best_cost_) and torch.equal(ma.initial_cost_, mb.initial_cost_)
        assert ma.best_num_inliers_ == mb.best_num_inliers_ and ma.status_ == mb.status_ == 0
