"""The dense-feature kernels on the GPU: the dilated convolution (fmpnp.conv3x3(dilation=...)), the 2x2 / stride 1
average pool and the pyramid step against their CPU twins bit for bit and against torch's fp64 results (exactly on
integers, within the derived bounds of dense_cases.py on Gaussians), launch independence, the contract's edge rules,
the walk of a D2-Net style trunk, DenseFeatureExtractor and optimize_feature_pnp(features="d2-net").  The references
are computed on the CPU: the framework's own GPU convolution may take an algorithm that is not exact even on
integers."""
import copy
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fmpnp
from fmpnp import _lib, synth

import dense_cases as dc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run_conv(shape, kind, d, bias, relu, **kw):
    x, w, b = (t.to(DEV) for t in dc.conv_operands(shape, kind))
    return fmpnp.conv3x3(x, w, b if bias else None, relu=relu, dilation=d, **kw)


# ---- the dilated convolution ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias,relu", dc.FLAGS, ids=dc.FLAG_IDS)
@pytest.mark.parametrize("d", dc.DILATIONS)
@pytest.mark.parametrize("shape", dc.CONV_SHAPES, ids=dc.CONV_IDS)
def test_gpu_conv_equals_torch_on_integers(shape, d, bias, relu):
    """Small integers: every partial sum is exact, so == against conv2d(dilation=d, padding=d) in fp64 pins the taps,
    the k range and the tiles' edges."""
    got = run_conv(shape, "int", d, bias, relu)
    assert got.is_cuda and got.dtype == torch.float32
    assert torch.equal(got.cpu().double(), dc.conv_ref64(shape, "int", d, bias, relu))


@pytest.mark.parametrize("bias,relu", dc.FLAGS, ids=dc.FLAG_IDS)
@pytest.mark.parametrize("d", dc.DILATIONS)
@pytest.mark.parametrize("shape", dc.CONV_SHAPES, ids=dc.CONV_IDS)
def test_gpu_conv_equals_the_twin_within_the_chains_bound(shape, d, bias, relu):
    """Gaussian operands: torch.equal with the twin (the MFMA chain is the fmaf chain), within
    gamma_{9 Cin + 1} (sum |a||w| + |b|) of conv2d in fp64, and nothing is stored outside the output."""
    buf, out, pad = dc.guarded((shape[0], shape[2], shape[3], shape[4]), DEV)
    got = run_conv(shape, "gauss", d, bias, relu, out=out)
    assert got is out
    got = got.cpu()
    err = (got.double() - dc.conv_ref64(shape, "gauss", d, bias, relu)).abs()
    bnd = dc.conv_bound(shape, "gauss", d, bias)
    same = torch.equal(got, dc.conv_twin(shape, "gauss", d, bias, relu))
    print(f"{shape} d={d} bias={bias} relu={relu}: equals the twin: {same}; max error / bound "
          f"{float((err / bnd.clamp_min(1e-300)).max()):.3g}")
    assert dc.guards_intact(buf, pad)
    assert bool((err <= bnd).all())
    assert same


@pytest.mark.parametrize("shape", dc.CONV_SHAPES, ids=dc.CONV_IDS)
def test_gpu_dilation_1_through_the_new_entry_point_is_conv3x3(shape):
    x, w, b = (t.to(DEV) for t in dc.conv_operands(shape, "gauss"))
    bsz, cin, cout, h, wd = shape
    out = torch.empty(bsz, cout, h, wd, device=DEV)
    with torch.cuda.device(DEV):
        rc = _lib.load().fmpnp_conv3x3_dilated(x.data_ptr(), bsz, cin, h, wd, w.data_ptr(), b.data_ptr(), cout,
                                               _lib.CONV_BIAS | _lib.CONV_RELU, out.data_ptr(), 1,
                                               _lib.stream_ptr(torch.device(DEV)))
    assert rc == 0
    assert torch.equal(out, fmpnp.conv3x3(x, w, b, relu=True))
    assert torch.equal(out.cpu(), fmpnp.conv3x3_cpu(*dc.conv_operands(shape, "gauss"), relu=True))


def test_gpu_conv_batch_items_equal_single_calls():
    for shape in (dc.CONV_SHAPES[2], dc.CONV_SHAPES[5]):
        x, w, b = (t.to(DEV) for t in dc.conv_operands(shape, "gauss"))
        whole = fmpnp.conv3x3(x, w, b, relu=True, dilation=2)
        for i in range(shape[0]):
            assert torch.equal(fmpnp.conv3x3(x[i:i + 1].contiguous(), w, b, relu=True, dilation=2)[0], whole[i]), (shape, i)


def test_gpu_conv_side_stream_equals_the_default_stream():
    shape = dc.CONV_SHAPES[3]
    x, w, b = (t.to(DEV) for t in dc.conv_operands(shape, "gauss"))
    want = fmpnp.conv3x3(x, w, b, relu=True, dilation=2)
    torch.cuda.synchronize()
    # (a high-priority stream: the framework hands streams out of one round-robin pool per priority, and tests
    # elsewhere in the suite that time two default-priority streams against each other depend on which two they draw)
    side = torch.cuda.Stream(device=DEV, priority=-1)
    got = fmpnp.conv3x3(x, w, b, relu=True, dilation=2, stream=side)
    side.synchronize()
    assert torch.equal(got, want)


def test_gpu_off_map_taps_and_infinite_inputs_follow_the_fma_rule():
    """The kernel and the twin alike (the payload of a NaN apart): a NaN weight at a tap that is off the map for every
    pixel still makes the channel NaN (fma(0, w, acc) is not skipped); an infinite input gives +-Inf through a
    non-zero weight and NaN through a zero one, at the pixels whose taps meet it and nowhere else."""
    shape = dc.CONV_SHAPES[1]  # 2 x 3 at dilation 2: every tap but the centre is off the map
    x, w, b = (t.clone() for t in dc.conv_operands(shape, "gauss"))
    w[2, 1, 0, 2] = float("nan")
    got = fmpnp.conv3x3(x.to(DEV), w.to(DEV), b.to(DEV), dilation=2).cpu()
    assert bool(torch.isnan(got[:, 2]).all()) and int(torch.isnan(got).sum()) == 6
    assert dc.same_bits(got, fmpnp.conv3x3_cpu(x, w, b, dilation=2))
    for shape, (ci, y, xx) in ((dc.CONV_SHAPES[4], (3, 9, 8)), (dc.CONV_SHAPES[3], (1, 2, 127))):
        x, w, b = (t.clone() for t in dc.conv_operands(shape, "int"))
        x[0, ci, y, xx] = float("inf")
        x[0, 0, 0, 0] = -float("inf")
        w[0, ci, 1, 1] = 0.0
        got = fmpnp.conv3x3(x.to(DEV), w.to(DEV), None, dilation=2).cpu()
        want = fmpnp.conv3x3_cpu(x, w, None, dilation=2)
        assert bool(torch.isnan(got[0, 0, y, xx])) and int(torch.isfinite(got).logical_not().sum()) > 9
        assert dc.same_bits(got, want), shape


def test_gpu_conv_argument_errors_launch_nothing():
    x, w, b = (t.to(DEV) for t in dc.conv_operands(dc.CONV_SHAPES[1], "gauss"))
    for d in (0, 3, -1):
        with pytest.raises(ValueError, match="dilation"):
            fmpnp.conv3x3(x, w, b, dilation=d)
    with pytest.raises(ValueError, match="fp16"):
        fmpnp.conv3x3(x, w, b, dilation=2, precision="f16")
    out = torch.full((1, 5, 2, 3), 7.0, device=DEV)
    for d in (0, 3, -1):
        rc = _lib.load().fmpnp_conv3x3_dilated(x.data_ptr(), 1, 3, 2, 3, w.data_ptr(), None, 5, 0, out.data_ptr(), d,
                                               _lib.stream_ptr(torch.device(DEV)))
        assert rc == _lib.EINVAL
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    for bad in (dict(x=x.cpu()), dict(x=x.double()), dict(x=x.transpose(2, 3)), dict(weight=w[:, :2].contiguous()),
                dict(out=torch.empty(1, 5, 2, 4, device=DEV))):
        kw = dict(x=x, weight=w, bias=b, dilation=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            fmpnp.conv3x3(**kw)


# ---- the average pool -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dc.POOL_SHAPES, ids=dc.POOL_IDS)
def test_gpu_avgpool(shape):
    x = dc.pool_operand(shape, "int")
    assert torch.equal(fmpnp.avgpool2x2s1(x.to(DEV)).cpu().double(), dc.pool_ref64(x))
    x = dc.pool_operand(shape, "gauss")
    buf, out, pad = dc.guarded((shape[0], shape[1], shape[2] - 1, shape[3] - 1), DEV)
    got = fmpnp.avgpool2x2s1(x.to(DEV), out=out)
    assert got is out and dc.guards_intact(buf, pad)
    got = got.cpu()
    assert torch.equal(got, fmpnp.avgpool2x2s1_cpu(x))
    assert bool(((got.double() - dc.pool_ref64(x)).abs() <= dc.pool_bound(x)).all())
    print(f"{shape}: equals torch's fp32 CPU avg_pool2d: {torch.equal(got, F.avg_pool2d(x, 2, 1))}")  # (not relied on)


def test_gpu_avgpool_misaligned_base_nonfinite_values_and_errors():
    x = dc.pool_operand(dc.POOL_SHAPES[2], "gauss")
    shifted = torch.cat([torch.zeros(1, device=DEV), x.to(DEV).reshape(-1)])[1:].view(x.shape)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    buf, out, pad = dc.guarded((1, 4, 8, 259), DEV, pad=63)  # (the output's base is misaligned too)
    assert torch.equal(fmpnp.avgpool2x2s1(shifted, out=out).cpu(), fmpnp.avgpool2x2s1_cpu(x)) and dc.guards_intact(buf, pad)
    x = dc.pool_operand(dc.POOL_SHAPES[1], "gauss").clone()
    x[0, 0, 1, 1], x[0, 1, 2, 3], x[1, 2, 0, 0], x[1, 2, 0, 1] = float("nan"), float("inf"), float("inf"), -float("inf")
    got = fmpnp.avgpool2x2s1(x.to(DEV)).cpu()
    assert int(torch.isnan(got[0, 0]).sum()) == 4 and bool((got[0, 1, 1:3, 2:4] == float("inf")).all())
    assert bool(torch.isnan(got[1, 2, 0, 0])) and got[1, 2, 0, 1] == -float("inf")
    assert dc.same_bits(got, fmpnp.avgpool2x2s1_cpu(x))
    for bad in (torch.zeros(1, 1, 1, 5, device=DEV), torch.zeros(1, 1, 5, 1, device=DEV), torch.zeros(1, 1, 4, 4),
                torch.zeros(1, 1, 4, 4, device=DEV).double(), torch.zeros(1, 1, 4, 6, device=DEV).transpose(2, 3)):
        with pytest.raises(ValueError):
            fmpnp.avgpool2x2s1(bad)


# ---- the pyramid step -----------------------------------------------------------------------------------------------
def _dev(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize("pair", dc.STEP_PAIRS, ids=dc.STEP_IDS)
@pytest.mark.parametrize("c", dc.STEP_CHANNELS)
def test_gpu_step_equals_the_twin_within_the_derived_bound(c, pair):
    cur, prev = dc.step_operands(c, pair)
    for normalize in (True, False):
        want, bound = dc.step_bound(cur, prev, normalize=normalize)
        buf, out, pad = dc.guarded(tuple(cur.shape), DEV)
        got = fmpnp.dense_pyramid_step(_dev(cur), _dev(prev), normalize=normalize, out=out)
        assert got is out and dc.guards_intact(buf, pad)
        got = got.cpu()
        assert torch.equal(got, fmpnp.dense_pyramid_step_cpu(cur, prev, normalize=normalize)), normalize
        assert bool(((got.double() - want).abs() <= bound).all())


@pytest.mark.parametrize("c", dc.STEP_CHANNELS)
def test_gpu_step_equals_torch_on_integers_at_a_dyadic_scale(c):
    cur, prev = dc.step_operands(c, dc.STEP_PAIRS[0], "int")
    got = fmpnp.dense_pyramid_step(_dev(cur), _dev(prev), normalize=False)
    assert torch.equal(got.cpu().double(), dc.step_sum64(cur, prev))


def test_gpu_step_zero_column_nan_column_aliasing_and_streams():
    cur, prev = (t.clone() for t in dc.step_operands(65, dc.STEP_PAIRS[0]))
    prev.zero_()
    cur[0, :, 2, 3] = 0.0            # an all-zero column: exactly 0, not NaN
    cur[1, 7, 4, 8] = float("nan")   # one NaN: its column, and no other
    got = fmpnp.dense_pyramid_step(_dev(cur), _dev(prev)).cpu()
    assert bool((got[0, :, 2, 3] == 0).all())
    nan = torch.isnan(got)
    assert bool(nan[1, :, 4, 8].all()) and int(nan.sum()) == 65
    assert dc.same_bits(got, fmpnp.dense_pyramid_step_cpu(cur, prev))
    # out may be cur (the stated aliasing rule), on a row past one tile too
    for c, pair in ((130, dc.STEP_PAIRS[1]), (65, dc.STEP_PAIRS[4])):
        cur, prev = (_dev(t) for t in dc.step_operands(c, pair))
        for normalize in (True, False):
            want = fmpnp.dense_pyramid_step(cur, prev, normalize=normalize)
            inplace = cur.clone()
            assert fmpnp.dense_pyramid_step(inplace, prev, normalize=normalize, out=inplace) is inplace
            assert torch.equal(inplace, want)
    with pytest.raises(ValueError, match="prev"):
        fmpnp.dense_pyramid_step(cur, cur, out=cur)
    # a batch item equals its single call; a side stream equals the default stream
    whole = fmpnp.dense_pyramid_step(cur, prev)
    for i in range(cur.shape[0]):
        assert torch.equal(fmpnp.dense_pyramid_step(cur[i:i + 1].contiguous(), prev[i:i + 1].contiguous())[0], whole[i])
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV, priority=-1)
    got = fmpnp.dense_pyramid_step(cur, prev, stream=side)
    side.synchronize()
    assert torch.equal(got, whole)


def test_gpu_step_argument_errors_launch_nothing():
    cur, prev = (_dev(t) for t in dc.step_operands(65, dc.STEP_PAIRS[0]))
    for kw in (dict(cur=cur[0]), dict(cur=cur.cpu()), dict(cur=cur.double()), dict(cur=cur.transpose(2, 3)),
               dict(prev=prev[:, :64].contiguous()), dict(prev=prev.cpu()), dict(out=torch.empty(2, 65, 5, 8, device=DEV)),
               dict(out=torch.empty(2, 65, 5, 9))):
        args = dict(cur=cur, prev=prev)
        args.update(kw)
        with pytest.raises(ValueError):
            fmpnp.dense_pyramid_step(**args)


# ---- the walk ---------------------------------------------------------------------------------------------------------
def test_gpu_walk_equals_the_cpu_walk_and_torch_on_integers():
    net, x = dc.walk_trunk(), dc.walk_image()
    cpu = fmpnp.HipEncoder(net)(x)
    dev = fmpnp.HipEncoder(copy.deepcopy(net).to(DEV))
    assert torch.equal(dev(x.to(DEV)).cpu(), cpu)
    assert torch.equal(dev(x.to(DEV), relu=True).cpu(), dc.twin_walk(net, x, relu_last=True))
    net, x = dc.walk_trunk("int"), dc.walk_image("int")
    want = copy.deepcopy(net).double()(x.double()).detach()
    assert torch.equal(fmpnp.HipEncoder(copy.deepcopy(net).to(DEV))(x.to(DEV)).cpu().double(), want)
    with pytest.raises(TypeError, match="child 17"):
        fmpnp.HipEncoder(copy.deepcopy(dc.walk_trunk()).to(DEV), precision="f16")


@pytest.mark.parametrize("scales", [(1,), fmpnp.dense.MULTISCALE], ids=["single", "multiscale"])
def test_gpu_extractor_equals_the_cpu_extractor(scales):
    for kind in ("gauss", "pos"):
        net, x = dc.walk_trunk(kind), dc.walk_image(kind)
        cpu = fmpnp.DenseFeatureExtractor(net, scales=scales, device="cpu").extract(x)
        ext = fmpnp.DenseFeatureExtractor(copy.deepcopy(net).to(DEV), scales=scales)
        assert ext.device.type == "cuda"
        got = ext.extract(x)  # (the extractor moves the image to its device)
        assert got.is_cuda and tuple(got.shape) == (1, 8) + dc.WALK_SIZES[scales[-1]]
        assert torch.equal(got.cpu(), cpu), kind
    # "pos": within the running bound of the torch backend in fp64 on the CPU; unit channel norms
    want = fmpnp.DenseFeatureExtractor(copy.deepcopy(net).double(), scales=scales, device="cpu", backend="torch").extract(x)
    _, bound = dc.extractor_bound(net, x, scales)
    assert float(bound.max()) < 1e-3 and bool(((got.cpu().double() - want).abs() <= bound).all())
    assert float((got.cpu().double().norm(dim=1) - 1).abs().max()) <= (3 + 8) * dc.U


# ---- the facade -------------------------------------------------------------------------------------------------------
Pred = namedtuple("Prediction", "points_3d reference_inliers matrix quaternion reference_filename")


def test_gpu_optimize_feature_pnp_with_d2net_features():
    """features="d2-net" with a DenseFeatureExtractor runs, and returns exactly what features="s2dhm" returns when handed
    a stub net whose compute_hypercolumn gives the same dense map: the branch adds nothing but the extraction."""
    net = copy.deepcopy(dc.walk_trunk()).to(DEV)
    image = dc.walk_image(size=(96, 128)).to(DEV)
    ext = fmpnp.DenseFeatureExtractor(net, image_loader=lambda paths, size, resize, device: image)
    query, resolution = ext.compute_hypercolumn(image)  # [1, 8, 23, 31]: the query is the reference image
    assert tuple(query.shape) == (1, 8, 23, 31) and tuple(resolution) == (96, 128)
    Hf, Wf = query.shape[2:]
    X, K, W, H = synth.scene(60, Hf, Wf, 5)
    p = fmpnp.refine.project_pixels(np.eye(3), np.zeros(3), X, K)
    rows, cols = (p[:, 1].astype(np.int64) * Hf) // H, (p[:, 0].astype(np.int64) * Wf) // W
    inl = np.stack([(cols + 0.5) * W / Hf, (rows + 0.5) * H / Wf], 1)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = synth.INITS["easy"]
    pred = Pred(X, inl, T, np.array([1.0, 0, 0, 0]), "ref.png")
    pyr = [(4, 8, None, None), (0, 4, None, None)]

    class Stub:
        def compute_hypercolumn(self, image, image_size=None, resize=True, to_cpu=False):
            return query.clone(), resolution

    out = []
    for features, n in (("d2-net", ext), ("s2dhm", Stub())):
        model = fmpnp.sparseFeaturePnP(20, loss_fn=fmpnp.geman_mcclure_loss, lambda_=0.01)
        out.append(fmpnp.optimize_feature_pnp(query, n, pred, K, image_shape=(W, H), feature_pyramid=pyr, model=model,
                                              features=features, verbose=False))
    (ta, qa, ma), (tb, qb, mb) = out
    assert np.array_equal(np.asarray(ta), np.asarray(tb)) and np.array_equal(np.asarray(qa), np.asarray(qb))
    assert torch.equal(ma.best_cost_, mb.best_cost_) and torch.equal(ma.initial_cost_, mb.initial_cost_)
    assert ma.best_num_inliers_ == mb.best_num_inliers_ and ma.status_ == mb.status_ == 0
    assert np.isfinite(np.asarray(ta)).all()
    dpm = fmpnp.DirectPoseModel(n_iters=20, loss_fn=fmpnp.geman_mcclure_loss, lambda_=0.01, verbose=False,
                                ratio_threshold=None)
    t, q, _ = dpm.optimize_feature_pnp(query, ext, pred, K, (W, H), feature_pyramid=pyr, features="d2-net")
    assert np.array_equal(np.asarray(t), np.asarray(ta)) and np.array_equal(np.asarray(q), np.asarray(qa))
    with pytest.raises(TypeError, match="compute_hypercolumn"):
        fmpnp.optimize_feature_pnp(query, object(), pred, K, image_shape=(W, H), features="d2-net", verbose=False)
    for kw in (dict(sparse_reference=True), dict(query_layers=[query])):
        with pytest.raises(ValueError, match="d2-net"):
            fmpnp.optimize_feature_pnp(query, ext, pred, K, image_shape=(W, H), features="d2-net", verbose=False, **kw)
