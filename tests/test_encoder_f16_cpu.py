"""The CPU side of the encoder's fp16 precision: the reference (fmpnp_conv3x3_f16_cpu) against torch's fp64 conv2d on
exact integers and within the contract's rounding terms on Gaussians, the nearest-even conversion at its boundaries,
the CPU weight pack, batch and thread independence, HipEncoder(precision="f16") on the CPU, and the argument errors
of every layer (host checks: nothing is launched)."""
import ctypes

import pytest
import torch

import fmpnp
from fmpnp import _lib

import encoder_cases as ec
import encoder_f16_cases as fc

NEW = ["fmpnp_conv3x3_f16_weights_size", "fmpnp_conv3x3_pack_weights_f16_async", "fmpnp_conv3x3_pack_weights_f16_cpu",
       "fmpnp_conv3x3_f16_async", "fmpnp_conv3x3_f16", "fmpnp_conv3x3_f16_cpu"]


def test_exports_and_abi():
    L = _lib.load()
    assert set(NEW) <= set(_lib.EXPORTS) and all(hasattr(L, n) for n in NEW)
    assert L.fmpnp_abi_version() == 4  # (exports were only added)


@pytest.mark.parametrize("bias,relu", fc.FLAGS, ids=fc.FLAG_IDS)
@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.IDS)
def test_reference_equals_torch_and_the_exact_twin_on_integers(shape, bias, relu):
    """Integers exact in fp16 with exact partial sums: == against conv2d in fp64 pins taps, padding and the channel
    blocks against torch; the exact twin gives the same bits."""
    x, w, b = fc.operands(shape, "int")
    got = fc.reference(shape, "int", bias, relu)
    assert got.dtype == torch.float32
    assert torch.equal(got.double(), fc.ref64(shape, "int", bias, relu))
    assert torch.equal(got, fmpnp.conv3x3_cpu(x, w, b if bias else None, relu=relu, precision="f32"))


@pytest.mark.parametrize("bias,relu", fc.FLAGS, ids=fc.FLAG_IDS)
@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.IDS)
def test_reference_within_its_roundings_of_fp64_on_gaussians(shape, bias, relu):
    """|reference - conv2d(fp64) of the rounded operands| <= 2^-24 |s| + 2^-24 |s + b| + the fp64-order term."""
    err = (fc.reference(shape, "gauss", bias, relu).double() - fc.ref64(shape, "gauss", bias, relu)).abs()
    bnd = fc.reference_bound(shape, "gauss", bias)
    print(f"{shape} bias={bias} relu={relu}: max error {float(err.max()):.3g}, "
          f"max error / bound {float((err / bnd.clamp_min(1e-300)).max()):.3g}")
    assert bool((err <= bnd).all())


def test_gaussian_operands_hold_no_fp16_subnormals():
    for shape in fc.SHAPES:
        x, w, _ = fc.operands(shape, "gauss")
        for t in (x, w):
            assert not bool(((t != 0) & (t.abs() < fc.TINY)).any())


@pytest.mark.parametrize("value,want", fc.CONVERSIONS, ids=[repr(v) for v, _ in fc.CONVERSIONS])
def test_conversion_is_nearest_even(value, want):
    """1 -> 1 channel, a 1 x 1 image, only the centre weight set: the output is fl16(value) * 1, once with the value as
    the input and once as the weight."""
    assert float(torch.tensor(value).half()) == want  # (the expectation itself, by torch.half)
    one, v = torch.zeros(1, 1, 3, 3), torch.zeros(1, 1, 3, 3)
    one[0, 0, 1, 1], v[0, 0, 1, 1] = 1.0, value
    as_input = fmpnp.conv3x3_cpu(torch.full((1, 1, 1, 1), value), one, precision="f16")
    as_weight = fmpnp.conv3x3_cpu(torch.ones(1, 1, 1, 1), v, precision="f16")
    assert float(as_input) == want and float(as_weight) == want
    assert float(fmpnp.conv3x3_f16_weights(v)[0, 0, 4, 0]) == want


@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.IDS)
def test_cpu_weight_pack_layout_and_tails(shape):
    _, w, _ = fc.operands(shape, "gauss")
    cout, cin = w.shape[:2]
    image = fmpnp.conv3x3_f16_weights(w)
    cb = (cin + 15) // 16
    assert image.dtype == torch.float16 and image.device.type == "cpu" and image.is_contiguous()
    assert tuple(image.shape[1:]) == (cb, 9, 16) and image.shape[0] >= cout and image.shape[0] % 32 == 0
    assert image.numel() * 2 == _lib.load().fmpnp_conv3x3_f16_weights_size(cin, cout)
    want = torch.zeros((image.shape[0], 16 * cb, 9), dtype=torch.float16)
    want[:cout, :cin] = w.reshape(cout, cin, 9).half()
    want = want.view(image.shape[0], cb, 16, 9).permute(0, 1, 3, 2)  # [co, cb, t, c] = w[co, 16 cb + c, t // 3, t % 3]
    assert torch.equal(image.view(torch.int16), want.contiguous().view(torch.int16))  # bit for bit, zero tails


@pytest.mark.parametrize("shape", [fc.SHAPES[0], fc.SHAPES[2], fc.SHAPES[8]], ids=[fc.IDS[0], fc.IDS[2], fc.IDS[8]])
def test_a_packed_image_equals_the_fp32_weights(shape):
    x, w, b = fc.operands(shape, "gauss")
    image = fmpnp.conv3x3_f16_weights(w)
    assert torch.equal(fmpnp.conv3x3_cpu(x, image, b, relu=True, precision="f16"), fc.reference(shape, "gauss", True, True))
    moved = image.clone()  # (a copy does not carry Cout: the bias, out or cout= gives it)
    assert torch.equal(fmpnp.conv3x3_cpu(x, moved, precision="f16", cout=shape[2]), fc.reference(shape, "gauss", False, False))
    with pytest.raises(ValueError):
        fmpnp.conv3x3_cpu(x, moved, precision="f16")


def test_reference_batch_items_and_threads_do_not_matter():
    shape = fc.SHAPES[4]
    x, w, b = fc.operands(shape, "gauss")
    whole = fc.reference(shape, "gauss", True, True)
    for i in range(shape[0]):
        alone = fmpnp.conv3x3_cpu(x[i:i + 1].contiguous(), w, b, relu=True, precision="f16")
        assert torch.equal(alone[0], whole[i]), i
    for n in (1, 2, 5):
        assert torch.equal(fmpnp.conv3x3_cpu(x, w, b, relu=True, n_threads=n, precision="f16"), whole)
    out = torch.empty_like(whole)
    assert fmpnp.conv3x3_cpu(x, w, b, relu=True, out=out, precision="f16") is out and torch.equal(out, whole)


def test_f32_is_the_call_without_the_argument():
    shape = fc.SHAPES[0]
    x, w, b = fc.operands(shape, "gauss")
    assert torch.equal(fmpnp.conv3x3_cpu(x, w, b, relu=True, precision="f32"), fmpnp.conv3x3_cpu(x, w, b, relu=True))
    net, batch = ec.walk_net(True), ec.walk_batch()
    for got, want in zip(fmpnp.HipEncoder(net, precision="f32").feature_maps(batch, [1, 3, 5]),
                         fmpnp.HipEncoder(net).feature_maps(batch, [1, 3, 5])):
        assert torch.equal(got, want)
    assert not torch.equal(fmpnp.conv3x3_cpu(x, w, b, precision="f16"), fmpnp.conv3x3_cpu(x, w, b))  # (f16 does differ)


def test_encoder_on_the_cpu_equals_the_chained_calls():
    net, batch = ec.vgg16_topology(), ec.vgg_batch()
    enc = fmpnp.HipEncoder(net, precision="f16")
    with torch.no_grad():
        got = enc(batch)
    want = fc.chained(net, batch, fmpnp.conv3x3_cpu, fmpnp.relu_cpu, fmpnp.maxpool2x2_cpu)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert not torch.equal(got, fmpnp.HipEncoder(net)(batch))


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "outofplace"])
def test_encoder_walk_is_exact_on_the_integer_net(inplace):
    """Activations at most 1542 <= 2048 are exact in fp16, the sums exact in fp32: the f16 walk is torch's own."""
    net, batch = fc.int_net(inplace), fc.int_batch()
    enc = fmpnp.HipEncoder(net, precision="f16")
    for taps in ec.WALK_TAPS:
        got, want = enc.feature_maps(batch, taps), ec.torch_walk(net, batch, taps)
        assert len(got) == len(want) == len(taps)
        for t, g, w in zip(taps, got, want):
            assert g.shape == w.shape and torch.equal(g, w), (taps, t)
    assert float(ec.torch_walk(net, batch, [5])[0].abs().max()) <= 2048.0  # (the premise: what the last conv reads)
    ext = fmpnp.HypercolumnExtractor(net, [1, 3, 5], backend="hip", precision="f16")
    for g, w in zip(ext.feature_maps(batch), ec.torch_walk(net, batch, [1, 3, 5])):
        assert torch.equal(g, w)


def test_python_errors():
    x, w, b = fc.operands(fc.SHAPES[0], "gauss")
    for bad in ("bf16", "F16", None, 16):
        with pytest.raises(ValueError):
            fmpnp.conv3x3_cpu(x, w, precision=bad)
        with pytest.raises(ValueError):
            fmpnp.conv3x3(x, w, precision=bad)  # (checked before the device is)
        with pytest.raises(ValueError):
            fmpnp.HipEncoder(fc.int_net(True), precision=bad)
        with pytest.raises(ValueError):
            fmpnp.HypercolumnExtractor(fc.int_net(True), [1], backend="hip", precision=bad)
    with pytest.raises(ValueError):
        fmpnp.HypercolumnExtractor(fc.int_net(True), [1], backend="torch", precision="f16")
    fmpnp.HypercolumnExtractor(fc.int_net(True), [1], backend="torch", precision="f32")
    image = fmpnp.conv3x3_f16_weights(w)
    with pytest.raises(ValueError):
        fmpnp.conv3x3_cpu(x, image)  # an image needs precision="f16"
    with pytest.raises(ValueError):
        fmpnp.conv3x3_cpu(x, image[:, :, :8].contiguous(), precision="f16", cout=5)  # wrong image shape
    with pytest.raises(ValueError):
        fmpnp.conv3x3_cpu(x, image, precision="f16", cout=40)  # (another Cout_p)
    with pytest.raises(ValueError):
        fmpnp.conv3x3_cpu(x, w.double(), precision="f16")  # wrong dtype
    with pytest.raises(ValueError):
        fmpnp.conv3x3_cpu(x, image.to(torch.bfloat16), precision="f16", cout=5)
    with pytest.raises(ValueError):
        fmpnp.conv3x3_f16_weights(w.double())
    with pytest.raises(ValueError):
        fmpnp.conv3x3_f16_weights(w[:, :, :2])


def test_plan_rejects_weights_fp16_cannot_hold():
    net = fc.int_net(True)
    with torch.no_grad():
        list(net.children())[2].weight[1, 2, 0, 1] = -65520.0
    with pytest.raises(ValueError, match="65520"):
        fmpnp.HipEncoder(net, precision="f16")
    fmpnp.HipEncoder(net)  # (the exact precision takes it)
    with torch.no_grad():
        list(net.children())[2].weight[1, 2, 0, 1] = 65519.0
    fmpnp.HipEncoder(net, precision="f16")


def test_c_entry_point_errors():
    L = _lib.load()
    buf = (ctypes.c_float * 64)()
    img = (ctypes.c_uint16 * (32 * 9 * 16 + 16))()
    p, z = ctypes.addressof(buf), None
    base = ctypes.addressof(img)
    ip = base + (-base) % 16  # 16-byte aligned
    assert L.fmpnp_conv3x3_f16_weights_size(2, 1) == 32 * 9 * 16 * 2
    assert L.fmpnp_conv3x3_f16_weights_size(17, 33) == 64 * 2 * 9 * 16 * 2
    assert L.fmpnp_conv3x3_f16_weights_size(0, 1) == 0 and L.fmpnp_conv3x3_f16_weights_size(1, -1) == 0
    assert L.fmpnp_conv3x3_f16_weights_size(1 << 15, 1 << 15) == 0  # 9 * 2^30 weights
    assert L.fmpnp_conv3x3_f16_weights_size(1, 1 << 24) == 0        # the padded image would pass 2^31 elements
    pack = L.fmpnp_conv3x3_pack_weights_f16_cpu
    assert pack(p, 2, 1, ip) == 0
    assert pack(z, 2, 1, ip) == _lib.EINVAL and pack(p, 2, 1, z) == _lib.EINVAL
    assert pack(p, 0, 1, ip) == _lib.EINVAL and pack(p, 2, 0, ip) == _lib.EINVAL
    assert pack(p, 2, 1, ip + 2) == _lib.EINVAL  # not 16-byte aligned
    assert pack(p, 1 << 15, 1 << 15, ip) == _lib.ETOOBIG and pack(p, 1, 1 << 24, ip) == _lib.ETOOBIG
    apack = L.fmpnp_conv3x3_pack_weights_f16_async  # (argument errors come back before anything is launched)
    assert apack(z, 2, 1, ip, z) == _lib.EINVAL and apack(p, 2, 1, z, z) == _lib.EINVAL
    assert apack(p, -1, 1, ip, z) == _lib.EINVAL and apack(p, 1, 1 << 24, ip, z) == _lib.ETOOBIG
    assert apack(p, 2, 1, ip + 4, z) == _lib.EINVAL
    ref = L.fmpnp_conv3x3_f16_cpu
    assert ref(p, 1, 2, 2, 2, p, z, 1, 0, p, 1) == 0
    assert ref(z, 1, 2, 2, 2, p, z, 1, 0, p, 1) == _lib.EINVAL and ref(p, 1, 2, 2, 2, z, z, 1, 0, p, 1) == _lib.EINVAL
    assert ref(p, 1, 2, 2, 2, p, z, 1, 0, z, 1) == _lib.EINVAL and ref(p, 1, 2, 2, 2, p, z, 1, 1, p, 1) == _lib.EINVAL
    assert ref(p, 0, 2, 2, 2, p, z, 1, 0, p, 1) == _lib.EINVAL and ref(p, 1, 2, 2, 2, p, z, 1, 4, p, 1) == _lib.EINVAL
    assert ref(p, 1, 2, 2, 2, p, z, 1, 0, p, -1) == _lib.EINVAL
    assert ref(p, 1, 1, 65536, 32768, p, z, 1, 0, p, 1) == _lib.ETOOBIG
    assert ref(p, 1, 1, 2, 2, p, z, 1 << 24, 0, p, 1) == _lib.ETOOBIG
    for fn in (L.fmpnp_conv3x3_f16_async, L.fmpnp_conv3x3_f16):
        assert fn(z, 1, 2, 2, 2, ip, z, 1, 0, p, z) == _lib.EINVAL and fn(p, 1, 2, 2, 2, z, z, 1, 0, p, z) == _lib.EINVAL
        assert fn(p, 1, 2, 2, 2, ip, z, 1, 0, z, z) == _lib.EINVAL and fn(p, 1, 2, 2, 2, ip, z, 1, 1, p, z) == _lib.EINVAL
        assert fn(p, 1, 2, 0, 2, ip, z, 1, 0, p, z) == _lib.EINVAL and fn(p, 1, 2, 2, 2, ip, z, 1, 8, p, z) == _lib.EINVAL
        assert fn(p, 1, 2, 2, 2, ip + 8, z, 1, 0, p, z) == _lib.EINVAL  # the image is not 16-byte aligned
        assert fn(p, 1, 1, 65536, 32768, ip, z, 1, 0, p, z) == _lib.ETOOBIG
        assert fn(p, 1, 1, 2, 2, ip, z, 1 << 24, 0, p, z) == _lib.ETOOBIG
