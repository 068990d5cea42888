"""The fp16 precision of the encoder's convolution on the GPU (fmpnp.conv3x3(..., precision="f16")): the kernel
against torch's fp64 conv2d and the exact kernel bit for bit on exact integers (lane maps, taps, padding, tile edges),
within the contract's bound of the CPU reference on Gaussians, the GPU weight pack against the CPU pack, the
conversion at its boundaries, launch independence (batch, stream, packed image), HipEncoder and
HypercolumnExtractor with precision="f16".  The references are computed on the CPU."""
import copy

import pytest
import torch

import fmpnp

import encoder_cases as ec
import encoder_f16_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run(shape, kind, bias, relu, **kw):
    x, w, b = (t.to(DEV) for t in fc.operands(shape, kind))
    return fmpnp.conv3x3(x, w, b if bias else None, relu=relu, precision="f16", **kw)


@pytest.mark.parametrize("bias,relu", fc.FLAGS, ids=fc.FLAG_IDS)
@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.IDS)
def test_gpu_f16_equals_torch_and_the_exact_kernel_on_integers(shape, bias, relu):
    """Operands exact in fp16, partial sums exact in fp32: every order gives the same bits, so == against conv2d in
    fp64 pins the fragment maps, the tap orientation, the padding, the channel tails and the tiles' edges."""
    got = run(shape, "int", bias, relu)
    assert got.is_cuda and got.dtype == torch.float32
    assert torch.equal(got.cpu().double(), fc.ref64(shape, "int", bias, relu))
    x, w, b = (t.to(DEV) for t in fc.operands(shape, "int"))
    assert torch.equal(got, fmpnp.conv3x3(x, w, b if bias else None, relu=relu))


@pytest.mark.parametrize("bias,relu", fc.FLAGS, ids=fc.FLAG_IDS)
@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.IDS)
def test_gpu_f16_within_the_bound_of_the_reference(shape, bias, relu):
    """|gpu - reference| <= K_p 2^-23 sum |fl16 a||fl16 w| + 2^-24 |s| + 2^-24 |s + b| on every element, and nothing
    is stored outside the output."""
    buf, out, pad = ec.guarded((shape[0], shape[2], shape[3], shape[4]), DEV)
    got = run(shape, "gauss", bias, relu, out=out)
    assert got is out
    err = (got.cpu().double() - fc.reference(shape, "gauss", bias, relu).double()).abs()
    bnd = fc.gpu_bound(shape, "gauss", bias)
    print(f"{shape} bias={bias} relu={relu}: max error {float(err.max()):.3g}, max error / bound "
          f"{float((err / bnd.clamp_min(1e-300)).max()):.3g}")
    assert ec.guards_intact(buf, pad)
    assert bool(torch.isfinite(got).all())
    assert bool((err <= bnd).all())


@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.IDS)
def test_gpu_weight_pack_equals_the_cpu_pack(shape):
    _, w, _ = fc.operands(shape, "gauss")
    want = fmpnp.conv3x3_f16_weights(w)
    got = fmpnp.conv3x3_f16_weights(w.to(DEV))
    assert got.is_cuda and got.dtype == torch.float16 and got.shape == want.shape and got.fmpnp_cout == shape[2]
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


def test_gpu_conversion_is_nearest_even():
    """The conversion values through the kernel, as the input (the staging's conversion) and as the weight (the
    pack's)."""
    for value, want in fc.CONVERSIONS:
        one, v = torch.zeros(1, 1, 3, 3), torch.zeros(1, 1, 3, 3)
        one[0, 0, 1, 1], v[0, 0, 1, 1] = 1.0, value
        as_input = fmpnp.conv3x3(torch.full((1, 1, 1, 1), value).to(DEV), one.to(DEV), precision="f16")
        as_weight = fmpnp.conv3x3(torch.ones(1, 1, 1, 1).to(DEV), v.to(DEV), precision="f16")
        assert float(as_input) == want and float(as_weight) == want, value


def test_gpu_f16_batch_items_equal_single_calls():
    for shape, relu in ((fc.SHAPES[4], True), (fc.SHAPES[2], False)):  # ([2]: more than one tile of every kind)
        x, w, b = (t.to(DEV) for t in fc.operands(shape, "gauss"))
        whole = fmpnp.conv3x3(x, w, b, relu=relu, precision="f16")
        for i in range(shape[0]):
            alone = fmpnp.conv3x3(x[i:i + 1].contiguous(), w, b, relu=relu, precision="f16")
            assert torch.equal(alone[0], whole[i]), (shape, i)


def test_gpu_f16_side_stream_and_packed_image():
    shape = fc.SHAPES[3]
    x, w, b = (t.to(DEV) for t in fc.operands(shape, "gauss"))
    want = fmpnp.conv3x3(x, w, b, relu=True, precision="f16")
    image = fmpnp.conv3x3_f16_weights(w)
    assert torch.equal(fmpnp.conv3x3(x, image, b, relu=True, precision="f16"), want)  # packed once == packed per call
    assert torch.equal(fmpnp.conv3x3(x, image.clone(), precision="f16", cout=shape[2]),
                       fmpnp.conv3x3(x, w, precision="f16"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV, priority=-1)  # (test_gpu_encoder.py says why a high-priority one)
    got = fmpnp.conv3x3(x, w, b, relu=True, stream=side, precision="f16")
    side.synchronize()
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        fmpnp.conv3x3(x, image)  # an image needs precision="f16"
    with pytest.raises(ValueError):
        fmpnp.conv3x3(x, image.cpu(), b, precision="f16")  # on another device
    with pytest.raises(ValueError):
        fmpnp.conv3x3(x, image[:32].contiguous(), precision="f16", cout=shape[2])  # wrong shape


def test_gpu_f16_encoder_equals_the_chained_calls():
    net, batch = ec.vgg16_topology().to(DEV), ec.vgg_batch().to(DEV)
    enc = fmpnp.HipEncoder(net, precision="f16")
    with torch.no_grad():
        got = enc(batch)
    assert torch.equal(got, fc.chained(net, batch, fmpnp.conv3x3, fmpnp.relu, fmpnp.maxpool2x2))
    assert torch.equal(enc(batch), got)  # (the cached images)


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "outofplace"])
def test_gpu_f16_walk_is_exact_on_the_integer_net(inplace):
    net, batch = fc.int_net(inplace), fc.int_batch()
    enc = fmpnp.HipEncoder(fc.int_net(inplace).to(DEV), precision="f16")
    for taps in ec.WALK_TAPS:
        got, want = enc.feature_maps(batch.to(DEV), taps), ec.torch_walk(net, batch, taps)
        assert len(got) == len(taps)
        for t, g, w in zip(taps, got, want):
            assert g.is_cuda and torch.equal(g.cpu(), w), (taps, t)


def test_gpu_f16_topology_and_the_extractor():
    """VGG-16's topology: the tapped maps are finite (their difference to the exact walk is printed, not asserted);
    the extractor's hypercolumn is assemble_hypercolumn of the f16 walk's maps, L2-normalised."""
    net, batch = ec.vgg16_topology().to(DEV), ec.vgg_batch().to(DEV)
    maps = fmpnp.HipEncoder(net, precision="f16").feature_maps(batch, ec.VGG_TAPS)
    exact = fmpnp.HipEncoder(net).feature_maps(batch, ec.VGG_TAPS)
    for t, g, e in zip(ec.VGG_TAPS, maps, exact):
        assert g.shape == e.shape and bool(torch.isfinite(g).all()), t
        print(f"child {t}: max |f16 - exact| {float((g - e).abs().max()):.3g}, max |exact| {float(e.abs().max()):.3g}")
    ext = fmpnp.HypercolumnExtractor(net, ec.VGG_TAPS, backend="hip", precision="f16")
    hyper, resolution = ext.compute_hypercolumn(ec.vgg_batch())
    channels = sum(int(m.shape[1]) for m in maps)
    assert hyper.is_cuda and tuple(resolution) == (32, 32)
    assert tuple(hyper.shape) == (2, channels) + tuple(maps[0].shape[2:])
    assert torch.equal(hyper, fmpnp.assemble_hypercolumn(maps))
    assert torch.allclose(hyper.double().pow(2).sum(1), torch.ones((), dtype=torch.float64, device=DEV), atol=1e-5)


def test_gpu_f16_weight_cache_rebuilds_after_an_in_place_change():
    net, batch = fc.int_net(True).to(DEV), fc.int_batch().to(DEV)
    enc = fmpnp.HipEncoder(net, precision="f16")
    with torch.no_grad():
        before = enc(batch).cpu()
        list(net.children())[0].weight.neg_()  # (the same magnitudes: still exact; data_ptr stays, the version moves)
        after = enc(batch).cpu()
        want = copy.deepcopy(net).cpu()(fc.int_batch())
    assert torch.equal(after, want) and not torch.equal(before, after)
