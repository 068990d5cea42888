"""The dense-feature operators' CPU twins and everything of the feature that needs no GPU: the dilated convolution, the
2x2 / stride 1 average pool and the pyramid step against torch in fp64 (exactly on integers, within the derived bounds
of dense_cases.py on Gaussians), the contract's edge rules, HipEncoder's plan and walk over a D2-Net style trunk,
DenseFeatureExtractor on the CPU, the argument errors, the exports, and the stand-alone C++ program."""
import copy
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
from torch import nn
import torch.nn.functional as F

import fmpnp
from fmpnp import _lib

import dense_cases as dc

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "featuremetric-pnp_amd")
NEW_EXPORTS = ["fmpnp_conv3x3_dilated_async", "fmpnp_conv3x3_dilated", "fmpnp_conv3x3_dilated_cpu",
               "fmpnp_avgpool2x2s1_async", "fmpnp_avgpool2x2s1", "fmpnp_avgpool2x2s1_cpu",
               "fmpnp_dense_pyramid_step_async", "fmpnp_dense_pyramid_step", "fmpnp_dense_pyramid_step_cpu"]


def test_every_new_symbol_is_exported_and_the_abi_stays_4():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    for name in _lib.EXPORTS:
        assert hasattr(lib, name), name
    assert lib.fmpnp_abi_version() == 4 and _lib.ABI_VERSION == 4


# ---- the dilated convolution ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias,relu", dc.FLAGS, ids=dc.FLAG_IDS)
@pytest.mark.parametrize("d", dc.DILATIONS)
@pytest.mark.parametrize("shape", dc.CONV_SHAPES, ids=dc.CONV_IDS)
def test_twin_equals_torch_on_integers(shape, d, bias, relu):
    """Small integers: every partial sum is exact, so == against conv2d(dilation=d, padding=d) in fp64 pins the taps,
    the k range and the edges."""
    assert torch.equal(dc.conv_twin(shape, "int", d, bias, relu).double(), dc.conv_ref64(shape, "int", d, bias, relu))


@pytest.mark.parametrize("bias,relu", dc.FLAGS, ids=dc.FLAG_IDS)
@pytest.mark.parametrize("d", dc.DILATIONS)
@pytest.mark.parametrize("shape", dc.CONV_SHAPES, ids=dc.CONV_IDS)
def test_twin_within_the_chains_bound(shape, d, bias, relu):
    x, w, b = dc.conv_operands(shape, "gauss")
    buf, out, pad = dc.guarded((shape[0], shape[2], shape[3], shape[4]), "cpu")
    got = fmpnp.conv3x3_cpu(x, w, b if bias else None, relu=relu, dilation=d, out=out, n_threads=3)
    assert got is out and dc.guards_intact(buf, pad)
    assert torch.equal(got, dc.conv_twin(shape, "gauss", d, bias, relu))  # (any thread count)
    err = (got.double() - dc.conv_ref64(shape, "gauss", d, bias, relu)).abs()
    assert bool((err <= dc.conv_bound(shape, "gauss", d, bias)).all())


@pytest.mark.parametrize("shape", dc.CONV_SHAPES, ids=dc.CONV_IDS)
def test_dilation_1_through_the_new_entry_point_is_conv3x3_cpu(shape):
    x, w, b = dc.conv_operands(shape, "gauss")
    bsz, cin, cout, h, wd = shape
    out = torch.empty(bsz, cout, h, wd)
    rc = _lib.load().fmpnp_conv3x3_dilated_cpu(x.data_ptr(), bsz, cin, h, wd, w.data_ptr(), b.data_ptr(), cout,
                                               _lib.CONV_BIAS | _lib.CONV_RELU, out.data_ptr(), 1, 0)
    assert rc == 0
    assert torch.equal(out, fmpnp.conv3x3_cpu(x, w, b, relu=True))
    assert torch.equal(out, dc.conv_twin(shape, "gauss", 1, True, True))


def test_off_map_taps_and_infinite_inputs_follow_the_fma_rule_on_the_twin():
    """fma(0, w, acc) for a tap off the map: a NaN weight there makes the output NaN although no input meets it; an
    infinite input times a zero weight is NaN, times a finite one +-Inf."""
    shape = dc.CONV_SHAPES[1]  # 2 x 3 at dilation 2: every tap but the centre is off the map
    x, w, b = (t.clone() for t in dc.conv_operands(shape, "gauss"))
    w[2, 1, 0, 2] = float("nan")
    got = fmpnp.conv3x3_cpu(x, w, b, dilation=2)
    assert bool(torch.isnan(got[:, 2]).all())
    keep = [0, 1, 3, 4]
    assert torch.equal(got[:, keep], dc.conv_twin(shape, "gauss", 2, True, False)[:, keep])
    x, w, b = (t.clone() for t in dc.conv_operands(dc.CONV_SHAPES[4], "int"))
    x[0, 3, 9, 8] = float("inf")
    w[5, 3, 1, 1] = 0.0
    got = fmpnp.conv3x3_cpu(x, w, None, dilation=2)
    assert bool(torch.isnan(got[0, 5, 9, 8]))            # Inf * 0 at the centre tap
    touched = torch.zeros(19, 17, dtype=torch.bool)
    for dy in (-2, 0, 2):
        for dx in (-2, 0, 2):
            if 0 <= 9 + dy < 19 and 0 <= 8 + dx < 17:
                touched[9 + dy, 8 + dx] = True
    # (Inf * w is +-Inf for w != 0 and NaN for w == 0: no output that meets the texel stays finite, every other does)
    assert bool(torch.isfinite(got[0, :, ~touched]).all()) and not bool(torch.isfinite(got[0, :, touched]).any())
    want = F.conv2d(dc.conv_operands(dc.CONV_SHAPES[4], "int")[0].double(), w.double(), padding=2, dilation=2)
    assert torch.equal(got[0, :, ~touched].double(), want[0, :, ~touched])


def test_conv_argument_errors():
    x, w, b = dc.conv_operands(dc.CONV_SHAPES[1], "gauss")
    for d in (0, 3, -1, 2.0, True):
        with pytest.raises(ValueError, match="dilation"):
            fmpnp.conv3x3_cpu(x, w, b, dilation=d)
    with pytest.raises(ValueError, match="fp16"):
        fmpnp.conv3x3_cpu(x, w, b, dilation=2, precision="f16")
    lib = _lib.load()
    out = torch.empty(1, 5, 2, 3)
    for d in (0, 3, -1):
        rc = lib.fmpnp_conv3x3_dilated_cpu(x.data_ptr(), 1, 3, 2, 3, w.data_ptr(), None, 5, 0, out.data_ptr(), d, 1)
        assert rc == _lib.EINVAL


# ---- the average pool -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dc.POOL_SHAPES, ids=dc.POOL_IDS)
def test_avgpool_twin(shape):
    x = dc.pool_operand(shape, "int")
    assert torch.equal(fmpnp.avgpool2x2s1_cpu(x).double(), dc.pool_ref64(x))
    x = dc.pool_operand(shape, "gauss")
    buf, out, pad = dc.guarded((shape[0], shape[1], shape[2] - 1, shape[3] - 1), "cpu")
    got = fmpnp.avgpool2x2s1_cpu(x, out=out, n_threads=3)
    assert got is out and dc.guards_intact(buf, pad)
    assert torch.equal(got, fmpnp.avgpool2x2s1_cpu(x, n_threads=1))
    assert bool(((got.double() - dc.pool_ref64(x)).abs() <= dc.pool_bound(x)).all())
    print(f"{shape}: equals torch's fp32 avg_pool2d: {torch.equal(got, F.avg_pool2d(x, 2, 1))}")  # (observed, not relied on)


def test_avgpool_nonfinite_values_and_errors():
    x = dc.pool_operand(dc.POOL_SHAPES[1], "gauss").clone()
    x[0, 0, 1, 1], x[0, 1, 2, 3], x[1, 2, 0, 0], x[1, 2, 0, 1] = float("nan"), float("inf"), float("inf"), -float("inf")
    got = fmpnp.avgpool2x2s1_cpu(x)
    assert bool(torch.isnan(got[0, 0, 0:2, 0:2]).all()) and int(torch.isnan(got[0, 0]).sum()) == 4
    assert bool((got[0, 1, 1:3, 2:4] == float("inf")).all())
    assert bool(torch.isnan(got[1, 2, 0, 0])) and got[1, 2, 0, 1] == -float("inf")  # (Inf - Inf, then -Inf alone)
    for bad in (torch.zeros(1, 1, 1, 5), torch.zeros(1, 1, 5, 1), torch.zeros(3, 5, 5), torch.zeros(1, 1, 4, 4).double(),
                torch.zeros(1, 1, 4, 6).transpose(2, 3)):
        with pytest.raises(ValueError):
            fmpnp.avgpool2x2s1_cpu(bad)
    with pytest.raises(ValueError):
        fmpnp.avgpool2x2s1_cpu(torch.zeros(1, 1, 4, 4), out=torch.zeros(1, 1, 4, 4))


# ---- the pyramid step -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", dc.STEP_PAIRS, ids=dc.STEP_IDS)
@pytest.mark.parametrize("c", dc.STEP_CHANNELS)
def test_step_twin_within_the_derived_bound(c, pair):
    cur, prev = dc.step_operands(c, pair)
    for normalize in (True, False):
        want, bound = dc.step_bound(cur, prev, normalize=normalize)
        buf, out, pad = dc.guarded(tuple(cur.shape), "cpu")
        got = fmpnp.dense_pyramid_step_cpu(cur, prev, normalize=normalize, out=out, n_threads=3)
        assert got is out and dc.guards_intact(buf, pad)
        assert torch.equal(got, fmpnp.dense_pyramid_step_cpu(cur, prev, normalize=normalize, n_threads=1))
        err = (got.double() - want).abs()
        print(f"C={c} {pair} normalize={normalize}: max error / bound {float((err / bound.clamp_min(1e-300)).max()):.3g}")
        assert bool((err <= bound).all())
    if prev is None:
        assert torch.equal(fmpnp.dense_pyramid_step_cpu(cur, None, normalize=False), cur)  # (cur's own bits)


@pytest.mark.parametrize("c", dc.STEP_CHANNELS)
def test_step_twin_equals_torch_on_integers_at_a_dyadic_scale(c):
    """(5, 9) <- (3, 5): the scales are 1/2, the weights 0, 1/2 and 1, so on small integers every product and sum is
    exact: == with cur + F.interpolate(prev, align_corners=True) in fp64."""
    cur, prev = dc.step_operands(c, dc.STEP_PAIRS[0], "int")
    assert torch.equal(fmpnp.dense_pyramid_step_cpu(cur, prev, normalize=False).double(), dc.step_sum64(cur, prev))


def test_step_zero_column_nan_column_and_aliasing_on_the_twin():
    cur, prev = (t.clone() for t in dc.step_operands(65, dc.STEP_PAIRS[0]))
    prev.zero_()
    cur[0, :, 2, 3] = 0.0            # an all-zero column: 0 / max(0, 1e-12) = 0, not NaN
    cur[1, 7, 4, 8] = float("nan")   # one NaN: its column, and no other
    got = fmpnp.dense_pyramid_step_cpu(cur, prev)
    assert bool((got[0, :, 2, 3] == 0).all())
    nan = torch.isnan(got)
    assert bool(nan[1, :, 4, 8].all()) and int(nan.sum()) == 65
    # out may be cur
    cur, prev = dc.step_operands(130, dc.STEP_PAIRS[1])
    for normalize in (True, False):
        want = fmpnp.dense_pyramid_step_cpu(cur, prev, normalize=normalize)
        inplace = cur.clone()
        assert fmpnp.dense_pyramid_step_cpu(inplace, prev, normalize=normalize, out=inplace) is inplace
        assert torch.equal(inplace, want)
    with pytest.raises(ValueError, match="prev"):
        fmpnp.dense_pyramid_step_cpu(cur, cur, out=cur)  # (out must not be prev)


def test_step_argument_errors():
    cur, prev = dc.step_operands(65, dc.STEP_PAIRS[0])
    for kw in (dict(cur=cur[0]), dict(cur=cur.double()), dict(cur=cur.transpose(2, 3)), dict(prev=prev[:, :64].contiguous()),
               dict(prev=prev[:1].contiguous()), dict(prev=prev.double()), dict(out=torch.empty(2, 65, 5, 8)),
               dict(out=torch.empty(2, 65, 5, 9).double())):
        args = dict(cur=cur, prev=prev)
        args.update(kw)
        with pytest.raises(ValueError):
            fmpnp.dense_pyramid_step_cpu(**args)


# ---- the walk ---------------------------------------------------------------------------------------------------------
def test_trunk_has_the_d2net_shape():
    net = fmpnp.d2net_trunk()
    kinds = [type(m).__name__ for m in net]
    assert kinds == (["Conv2d", "ReLU"] * 2 + ["MaxPool2d"] + ["Conv2d", "ReLU"] * 2 + ["MaxPool2d"]
                     + ["Conv2d", "ReLU"] * 3 + ["AvgPool2d"] + ["Conv2d", "ReLU"] * 2 + ["Conv2d"])
    convs = [m for m in net if isinstance(m, nn.Conv2d)]
    assert [m.out_channels for m in convs] == [64, 64, 128, 128, 256, 256, 256, 512, 512, 512]
    assert [m.dilation[0] for m in convs] == [1] * 7 + [2] * 3 and all(m.padding == m.dilation for m in convs)
    with pytest.raises(ValueError):
        fmpnp.d2net_trunk((4, 4))


def test_hip_encoder_on_the_cpu_is_the_composition_of_the_twins():
    net, x = dc.walk_trunk(), dc.walk_image()
    enc = fmpnp.HipEncoder(net)
    assert enc._kinds.count("avgpool") == 1
    got = enc(x)
    assert tuple(got.shape) == (1, 8) + dc.WALK_SIZES[1]
    assert torch.equal(got, dc.twin_walk(net, x))
    assert torch.equal(enc(x, relu=True), dc.twin_walk(net, x, relu_last=True))
    want, bound = dc.trunk_bound(copy.deepcopy(net).double(), x, 0.0, False)
    assert bool(((got.double() - want).abs() <= bound).all())


def test_hip_encoder_equals_torch_on_integers():
    net, x = dc.walk_trunk("int"), dc.walk_image("int")
    want = copy.deepcopy(net).double()(x.double())
    assert 0 < float(want.detach().abs().max()) < 2.0 ** 12
    assert torch.equal(fmpnp.HipEncoder(net)(x).double(), want)


@pytest.mark.parametrize("scales", [(1,), fmpnp.dense.MULTISCALE], ids=["single", "multiscale"])
def test_extractor_on_the_cpu(scales):
    """Against backend="torch" in fp64 on the trunk without cancellation (dense_cases.walk_trunk("pos")), within the
    running bound of dense_cases.extractor_bound; the shape; unit channel norms."""
    net, x = dc.walk_trunk("pos"), dc.walk_image("pos")
    ext = fmpnp.DenseFeatureExtractor(net, scales=scales, device="cpu")
    got = ext.extract(x)
    assert tuple(got.shape) == (1, 8) + dc.WALK_SIZES[scales[-1]] and got.dtype == torch.float32
    torch_ext = fmpnp.DenseFeatureExtractor(copy.deepcopy(net).double(), scales=scales, device="cpu", backend="torch")
    want = torch_ext.extract(x)
    ref, bound = dc.extractor_bound(net, x, scales)
    assert want.dtype == torch.float64 and torch.allclose(want, ref, rtol=0, atol=1e-12)
    err = (got.double() - want).abs()
    print(f"{scales}: max error {float(err.max()):.3g}, max error / bound {float((err / bound).max()):.3g}, "
          f"largest bound {float(bound.max()):.3g}")
    assert float(bound.max()) < 1e-3  # (the bound says something: the values are of order 1 / sqrt(8))
    assert bool((err <= bound).all())
    # unit channel norms within fp32: the division's and the norm's roundings, 3 u, and C roundings of the squares' sum
    assert float((got.double().norm(dim=1) - 1).abs().max()) <= (3 + 8) * dc.U
    dense, resolution = ext.compute_hypercolumn([x[0]], to_cpu=True)
    assert isinstance(dense, np.ndarray) and tuple(resolution) == dc.WALK_IMAGE and np.array_equal(dense, got.numpy())
    # the signed trunk, ReLUs at work: the same map from the composition of the twins, and the rigorous bound holds
    net, x = dc.walk_trunk(), dc.walk_image()
    got = fmpnp.DenseFeatureExtractor(net, scales=scales, device="cpu").extract(x)
    prev = None
    for s in scales:
        size = (int(dc.WALK_IMAGE[0] * s), int(dc.WALK_IMAGE[1] * s))
        scaled = x if s == 1 else fmpnp.assemble_hypercolumn_cpu([x], size, normalize=False)
        prev = fmpnp.dense_pyramid_step_cpu(dc.twin_walk(net, scaled, relu_last=True), prev)
    assert torch.equal(got, prev)


def test_extractor_multiscale_flag_and_errors():
    net = dc.walk_trunk()
    assert fmpnp.DenseFeatureExtractor(net, multiscale=True, device="cpu").scales == (0.5, 1, 2)
    ext = fmpnp.DenseFeatureExtractor(net, device="cpu")
    with pytest.raises(ValueError, match="one image"):
        ext.extract(torch.zeros(2, 3, 38, 52))
    with pytest.raises(TypeError):
        ext.compute_hypercolumn(["a/path.png"])
    with pytest.raises(TypeError):
        fmpnp.DenseFeatureExtractor(nn.Conv2d(3, 3, 3))
    with pytest.raises(ValueError):
        fmpnp.DenseFeatureExtractor(net, backend="miopen")
    with pytest.raises(ValueError):
        fmpnp.DenseFeatureExtractor(net, scales=(0,))


@pytest.mark.parametrize("child", [nn.Conv2d(3, 8, 3, padding=3, dilation=3), nn.Conv2d(3, 8, 3, padding=1, dilation=2),
                                   nn.Conv2d(3, 8, 3, padding=2, dilation=1), nn.Conv2d(3, 8, 3, padding=2, dilation=(2, 1)),
                                   nn.AvgPool2d(2, 2), nn.AvgPool2d(3, 1), nn.AvgPool2d(2, 1, padding=1),
                                   nn.AvgPool2d(2, 1, ceil_mode=True)],
                         ids=["dilation3", "pad1-dil2", "pad2-dil1", "dil2x1", "avg2s2", "avg3s1", "avgpad1", "avgceil"])
def test_plan_rejects_other_dilations_and_average_pools_naming_the_child(child):
    with pytest.raises(TypeError, match="child 1"):
        fmpnp.HipEncoder(nn.Sequential(nn.ReLU(), child))


def test_plan_takes_the_trunks_children_and_f16_rejects_the_dilated_one():
    fmpnp.HipEncoder(nn.Sequential(nn.Conv2d(3, 4, 3, padding=2, dilation=2), nn.AvgPool2d(2, 1, count_include_pad=False),
                                   nn.AvgPool2d((2, 2), stride=(1, 1))))
    fmpnp.HypercolumnExtractor(dc.walk_trunk(), [3, 8], backend="hip")  # (the new children for free)
    with pytest.raises(TypeError, match="child 17"):  # the first dilated convolution
        fmpnp.HipEncoder(dc.walk_trunk(), precision="f16")
    from fmpnp import superpoint as sp
    net = sp.SuperPointNet()
    net.conv1b = nn.Conv2d(64, 64, 3, padding=2, dilation=2)
    with pytest.raises(TypeError, match="conv1b"):  # (HipSuperPointNet's checks keep dilation 1)
        sp.HipSuperPointNet(net)


def test_preprocess():
    img = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3) * 7
    caffe = fmpnp.d2net_preprocess(img, "caffe")
    assert caffe.shape == (3, 2, 3) and caffe.dtype == np.float32
    assert np.array_equal(caffe[0], img[:, :, 2].astype(np.float32) - np.float32(103.939))
    assert np.array_equal(caffe[2], img[:, :, 0].astype(np.float32) - np.float32(123.68))
    tor = fmpnp.d2net_preprocess(img, "torch")
    assert np.allclose(tor[1], (img[:, :, 1] / 255.0 - 0.456) / 0.224, atol=1e-6)
    with pytest.raises(ValueError):
        fmpnp.d2net_preprocess(img, "tf")


# ---- the facade's checks (the run itself needs the GPU: test_gpu_dense.py) -------------------------------------------
def test_d2net_facade_rejects_what_it_cannot_serve():
    class P:
        quaternion, matrix, reference_filename = [1, 0, 0, 0], np.eye(4), "ref"
    ext = fmpnp.DenseFeatureExtractor(dc.walk_trunk(), device="cpu")
    with pytest.raises(TypeError, match="compute_hypercolumn"):
        fmpnp.optimize_feature_pnp(None, object(), P(), np.eye(3), (8, 8), features="d2-net", verbose=False)
    with pytest.raises(ValueError, match="d2-net"):
        fmpnp.optimize_feature_pnp(None, ext, P(), np.eye(3), (8, 8), features="d2-net", verbose=False, sparse_reference=True)
    with pytest.raises(ValueError, match="d2-net"):
        fmpnp.optimize_feature_pnp(None, ext, P(), np.eye(3), (8, 8), features="d2-net", verbose=False, query_layers=[1])


def test_the_standalone_program_passes():
    """csrc/test_dense_cpu.cpp's own checks (the build `make dense-sanitize` runs under ASan + UBSan): the twins against
    plain restatements, dilation 1 against fmpnp_conv3x3_cpu, guard words around every output, by exit status."""
    subprocess.run(["make", "-s", "-C", PKG, "build/test_dense_cpu"], check=True, timeout=600)
    out = subprocess.run([os.path.join(PKG, "build", "test_dense_cpu")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout[-2000:]
