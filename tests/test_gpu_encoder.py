"""The encoder's kernels on the GPU (fmpnp/encoder.py): the convolution's indexing against torch's fp64 conv2d on
exact integers, its rounding within the chain's derived bound, the kernel against its CPU twin bit for bit on every
shape, launch independence (batch, stream), the pool and the ReLU, the layer walk, and the VGG-16 topology end to
end into the hypercolumn.  The references are computed on the CPU: the framework's own GPU convolution may take
an algorithm that is not exact even on integers."""
import pytest
import torch

import fmpnp

import encoder_cases as ec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLAGS = [(False, False), (True, False), (False, True), (True, True)]
FLAG_IDS = ["plain", "bias", "relu", "bias-relu"]


def run(shape, kind, bias, relu, **kw):
    x, w, b = (t.to(DEV) for t in ec.operands(shape, kind))
    return fmpnp.conv3x3(x, w, b if bias else None, relu=relu, **kw)


@pytest.mark.parametrize("bias,relu", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("shape", ec.SHAPES, ids=ec.IDS)
def test_gpu_indexing_equals_torch_on_integers(shape, bias, relu):
    """Small integers: every partial sum is exact, so == against conv2d in fp64 pins the tap orientation, the
    padding, the k order's range and the tiles' edges against torch."""
    got = run(shape, "int", bias, relu)
    assert got.is_cuda and got.dtype == torch.float32
    assert torch.equal(got.cpu().double(), ec.ref64(shape, "int", bias, relu))


@pytest.mark.parametrize("bias,relu", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("shape", ec.SHAPES, ids=ec.IDS)
def test_gpu_equals_the_twin_within_the_chains_bound(shape, bias, relu):
    """Gaussian operands: torch.equal with the twin (the MFMA chain is the fmaf chain at this K), within
    gamma_{K+1} (sum |a||w| + |b|) of conv2d in fp64, and nothing is stored outside the output."""
    buf, out, pad = ec.guarded((shape[0], shape[2], shape[3], shape[4]), DEV)
    got = run(shape, "gauss", bias, relu, out=out)
    assert got is out
    got = got.cpu()
    err = (got.double() - ec.ref64(shape, "gauss", bias, relu)).abs()
    bnd = ec.bound(shape, "gauss", bias)
    same = torch.equal(got, ec.twin(shape, "gauss", bias, relu))
    print(f"{shape} bias={bias} relu={relu}: equals the twin: {same}; max error / bound "
          f"{float((err / bnd.clamp_min(1e-300)).max()):.3g}")
    assert ec.guards_intact(buf, pad)
    assert bool((err <= bnd).all())
    assert same


def test_gpu_batch_items_equal_single_calls():
    shape = ec.SHAPES[4]
    x, w, b = (t.to(DEV) for t in ec.operands(shape, "gauss"))
    whole = fmpnp.conv3x3(x, w, b, relu=True)
    for i in range(shape[0]):
        assert torch.equal(fmpnp.conv3x3(x[i:i + 1].contiguous(), w, b, relu=True)[0], whole[i]), i
    shape = ec.SHAPES[2]  # (more than one tile of every kind)
    x, w, b = (t.to(DEV) for t in ec.operands(shape, "gauss"))
    whole = fmpnp.conv3x3(x, w, b)
    for i in range(shape[0]):
        assert torch.equal(fmpnp.conv3x3(x[i:i + 1].contiguous(), w, b)[0], whole[i]), i


def test_gpu_side_stream_equals_the_default_stream():
    shape = ec.SHAPES[3]
    x, w, b = (t.to(DEV) for t in ec.operands(shape, "gauss"))
    want = fmpnp.conv3x3(x, w, b, relu=True)
    torch.cuda.synchronize()
    # (a high-priority stream: the framework hands streams out of one round-robin pool per priority, and tests
    # elsewhere in the suite that time two default-priority streams against each other depend on which two they draw)
    side = torch.cuda.Stream(device=DEV, priority=-1)
    got = fmpnp.conv3x3(x, w, b, relu=True, stream=side)
    pooled = fmpnp.maxpool2x2(got, stream=side)
    act = fmpnp.relu(x, stream=side)
    side.synchronize()
    assert torch.equal(got, want) and torch.equal(pooled, fmpnp.maxpool2x2(want)) and torch.equal(act, fmpnp.relu(x))


def pool_relu_input(h, w):
    x = torch.randn((2, 3, h, w), generator=torch.Generator().manual_seed(h * 1000 + w))
    flat = x.view(-1)
    flat[0] = -0.0
    if flat.numel() > 4:
        flat[1], flat[2], flat[3] = 0.0, -3.0, -0.0
    return x


@pytest.mark.parametrize("h,w", [(5, 7), (1, 1), (2, 258), (6, 8)])
def test_gpu_relu_and_pool_equal_torch_and_the_twins(h, w):
    """(6, 8): the 16-byte path of the pool; (5, 7), (2, 258): one output per thread.  The ReLU takes its 16-byte
    path on a whole allocation and its 4-byte path on a view one float in."""
    x = pool_relu_input(h, w)
    xd = x.to(DEV)
    r = fmpnp.relu(xd).cpu()
    assert torch.equal(r, torch.relu(x)) and not bool(torch.signbit(r).any())
    assert torch.equal(r.view(torch.int32), fmpnp.relu_cpu(x).view(torch.int32))
    n = x.numel()
    buf, view, pad = ec.guarded((n,), DEV, pad=5)  # (20 bytes in: not 16-byte aligned)
    src = torch.cat([torch.zeros(1), x.view(-1)]).to(DEV)[1:]
    assert fmpnp.relu(src, out=view) is view and ec.guards_intact(buf, pad)
    assert torch.equal(view.cpu(), r.view(-1))
    y = xd.clone()
    assert fmpnp.relu(y, out=y) is y and torch.equal(y.cpu(), r)  # in place
    if min(h, w) < 2:
        with pytest.raises(ValueError):
            fmpnp.maxpool2x2(xd)
        return
    buf, out, pad = ec.guarded((2, 3, h // 2, w // 2), DEV)
    got = fmpnp.maxpool2x2(xd, out=out).cpu()
    assert ec.guards_intact(buf, pad)
    assert torch.equal(got, torch.nn.functional.max_pool2d(x, 2, 2))
    assert torch.equal(got.view(torch.int32), fmpnp.maxpool2x2_cpu(x).view(torch.int32))


def test_gpu_nan_stays_in_relu_and_wins_in_pool():
    x = pool_relu_input(4, 8)
    x[0, 0, 1, 1] = float("nan")
    xd = x.to(DEV)
    assert int(torch.isnan(fmpnp.relu(xd)).sum()) == 1
    got, want = fmpnp.maxpool2x2(xd).cpu(), fmpnp.maxpool2x2_cpu(x)
    assert torch.isnan(got[0, 0, 0, 0]) and torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "outofplace"])
def test_gpu_walk_equals_the_references_loop(inplace):
    """conv-ReLU-conv-ReLU-pool-conv on integers on the GPU against the reference's loop (exact on the CPU): every
    tap position, a tap on a ReLU child with inplace True and False."""
    net, batch = ec.walk_net(inplace), ec.walk_batch()
    enc = fmpnp.HipEncoder(ec.walk_net(inplace).to(DEV))
    for taps in ec.WALK_TAPS:
        got, want = enc.feature_maps(batch.to(DEV), taps), ec.torch_walk(net, batch, taps)
        assert len(got) == len(taps)
        for t, g, w in zip(taps, got, want):
            assert g.is_cuda and torch.equal(g.cpu(), w), (taps, t)
    with torch.no_grad():
        assert torch.equal(enc(batch.to(DEV)).cpu(), net(batch.clone()))


def test_gpu_topology_equals_the_twin_into_the_hypercolumn():
    """VGG-16's features[:-2] at small widths, taps [9, 14, 17, 21, 24]: the GPU's maps are the twin's bit for bit,
    and HypercolumnExtractor(backend="hip").compute_hypercolumn is assemble_hypercolumn_cpu of the twin's maps."""
    twin_maps = ec.vgg_twin_maps()
    net = ec.vgg16_topology().to(DEV)
    maps = fmpnp.HipEncoder(net).feature_maps(ec.vgg_batch().to(DEV), ec.VGG_TAPS)
    for t, g, w in zip(ec.VGG_TAPS, maps, twin_maps):
        assert torch.equal(g.cpu(), w), t
    ext = fmpnp.HypercolumnExtractor(net, ec.VGG_TAPS, backend="hip")
    hyper, resolution = ext.compute_hypercolumn(ec.vgg_batch())
    assert hyper.is_cuda and tuple(resolution) == (32, 32)
    assert torch.equal(hyper.cpu(), fmpnp.assemble_hypercolumn_cpu(list(twin_maps)))
    whole = fmpnp.HipEncoder(net)(ec.vgg_batch().to(DEV))
    assert torch.equal(whole.cpu(), fmpnp.HipEncoder(ec.vgg16_topology())(ec.vgg_batch()))


def test_gpu_torch_backend_is_unchanged():
    """The default and backend="torch" are the walk written out by hand through the framework, then the assembly."""
    net = ec.vgg16_topology().to(DEV)
    batch = ec.vgg_batch().to(DEV)
    ec.torch_walk(net, batch, ec.VGG_TAPS)  # (the framework settles on its algorithms in a first pass)
    want = fmpnp.assemble_hypercolumn(ec.torch_walk(net, batch, ec.VGG_TAPS))
    for kw in ({}, {"backend": "torch"}):
        hyper, _ = fmpnp.HypercolumnExtractor(net, ec.VGG_TAPS, **kw).compute_hypercolumn(batch)
        assert torch.equal(hyper, want), kw


def test_gpu_argument_errors_launch_nothing():
    x, w, b = (t.to(DEV) for t in ec.operands(ec.SHAPES[0], "gauss"))
    for bad in (dict(x=x[0]), dict(x=x.double()), dict(x=x.transpose(2, 3)), dict(x=x.cpu()),
                dict(weight=w[:, :2].contiguous()), dict(weight=w.cpu()), dict(bias=b[:3].contiguous()),
                dict(bias=b.cpu()), dict(out=torch.empty(1, 5, 5, 6, device=DEV)), dict(out=torch.empty(1, 5, 5, 7))):
        kw = dict(x=x, weight=w, bias=b)
        kw.update(bad)
        with pytest.raises(ValueError):
            fmpnp.conv3x3(**kw)
    with pytest.raises(ValueError):
        fmpnp.HipEncoder(ec.walk_net(True).to(DEV))(ec.walk_batch())  # the batch on another device
