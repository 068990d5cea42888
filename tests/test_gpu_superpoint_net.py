"""HipSuperPointNet on the GPU: its outputs against the CPU module's (the twins) bit for bit at three sizes, the
frontend from the image on against the CPU stages on the CPU module's outputs, the fp16 precision on an exact integer
first block and its exact heads, and the wrong-device error."""
import functools

import numpy as np
import pytest
import torch

import fmpnp

import localize_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def fresh():
    torch.manual_seed(1234)
    return fmpnp.SuperPointNet().eval()


@functools.lru_cache(maxsize=None)
def cpu_module():
    return fmpnp.HipSuperPointNet(fresh())


@functools.lru_cache(maxsize=None)
def gpu_module(precision="f32"):
    return fmpnp.HipSuperPointNet(fresh().to(DEV), precision=precision)


def rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


def same(got, want):
    """torch.equal with NaN positions compared as positions."""
    got = got.cpu()
    return (got.shape == want.shape and torch.equal(torch.isnan(got), torch.isnan(want))
            and torch.equal(torch.nan_to_num(got), torch.nan_to_num(want)))


@pytest.mark.parametrize("shape,seed", [((1, 1, 16, 24), 21), ((2, 1, 24, 40), 22), ((1, 1, 64, 96), 24)],
                         ids=["16x24", "2x24x40", "64x96"])
def test_gpu_equals_the_cpu_module(shape, seed):
    """64 x 96: the first block's 3x3 layers run more than one pixel tile."""
    x = rand(shape, seed)
    semi, desc = gpu_module()(x.to(DEV))
    want_semi, want_desc = cpu_module()(x)
    assert semi.is_cuda and desc.is_cuda
    assert semi.shape == (shape[0], 65, shape[2] // 8, shape[3] // 8)
    assert same(semi, want_semi) and same(desc, want_desc)


def test_gpu_frontend_from_the_image_equals_the_cpu_stages():
    """SuperPointFrontend around the module, unchanged: (pts, desc, heat) of the GPU chain from the image on equal the
    CPU stages on the CPU module's outputs, so the baseline is the same bits on both sides."""
    img = rand((64, 96), 24)
    front = fmpnp.SuperPointFrontend(gpu_module(), nms_dist=4, conf_thresh=0.015, nn_thresh=0.7)
    got = front.run(img)
    semi, coarse = cpu_module()(img.view(1, 1, 64, 96))
    want = fmpnp.superpoint_postprocess(semi, coarse, (64, 96), 4, 0.015, cpu=True)
    assert len(got) == len(want) == 3
    assert want[2] is not None and want[0].shape[1] > 0  # (the case does reach the NMS and the sampling)
    for g, w, what in zip(got, want, ("pts", "desc", "heat")):
        lc.equal(g, w, what)


def integer_first_block(net):
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for name in ("conv1a", "conv1b"):
            m = getattr(net, name)
            m.weight.copy_(torch.randint(-1, 2, m.weight.shape, generator=g).float())
            m.bias.copy_(torch.randint(-3, 4, m.bias.shape, generator=g).float())
    return net


def test_gpu_f16_is_exact_on_an_integer_first_block():
    """Image in [-2, 2], conv1a and conv1b weights in [-1, 1] and biases in [-3, 3], all integers.  conv1a's outputs
    are integers of at most 9 * 2 + 3 = 21: binary16 holds them, so conv1b's fp16 operands are its fp32 operands; its
    partial sums are integers of at most 9 * 64 * 21 + 3 = 12099 < 2^24: exact in the fp32 accumulators in any order.
    So "f16" equals "f32" bit for bit through conv2a's input (the pooled conv1b output)."""
    img = torch.randint(-2, 3, (1, 1, 16, 24), generator=torch.Generator().manual_seed(78)).float()
    net = integer_first_block(fresh())
    w1, b1, w2, b2 = (p.detach().double() for p in (net.conv1a.weight, net.conv1a.bias, net.conv1b.weight, net.conv1b.bias))
    first = torch.relu(torch.nn.functional.conv2d(img.double(), w1, b1, padding=1))
    assert float(first.max()) <= 21 and bool((first == first.round()).all())  # the precondition, on the case itself
    assert 9 * 64 * 21 + 3 < 2 ** 24 and 21 <= 2048
    want = torch.nn.functional.max_pool2d(torch.relu(torch.nn.functional.conv2d(first, w2, b2, padding=1)), 2, 2)
    net = net.to(DEV)
    maps = {}
    for precision in ("f32", "f16"):
        maps[precision] = fmpnp.HipSuperPointNet(net, precision=precision).walk(img.to(DEV), taps=("conv2a",))[2]["conv2a"]
        assert torch.equal(maps[precision].cpu().double(), want), precision
    assert torch.equal(maps["f16"], maps["f32"])


def test_gpu_f16_outputs_are_finite_and_its_heads_exact():
    """The seeded Gaussian net at 16 x 24 in "f16": finite outputs, and the two heads, given the walk's own head
    inputs, are conv1x1 of those inputs bit for bit (they stayed exact fp32)."""
    hip = gpu_module("f16")
    semi, desc, maps = hip.walk(rand((1, 1, 16, 24), 21).to(DEV), taps=("convPb", "convDb"))
    assert bool(torch.isfinite(semi).all()) and bool(torch.isfinite(desc).all())
    net = hip.net
    assert torch.equal(semi, fmpnp.conv1x1(maps["convPb"], net.convPb.weight.detach(), net.convPb.bias.detach()))
    raw = fmpnp.conv1x1(maps["convDb"], net.convDb.weight.detach(), net.convDb.bias.detach())
    assert torch.equal(desc, fmpnp.assemble_hypercolumn([raw]))
    # (and those inputs are not the exact walk's: the 3x3 layers did run in the fp16 precision)
    exact = gpu_module().walk(rand((1, 1, 16, 24), 21).to(DEV), taps=("convPb",))[2]["convPb"]
    assert not torch.equal(exact, maps["convPb"])


def test_gpu_wrong_device_raises():
    with pytest.raises(ValueError):
        gpu_module()(rand((1, 1, 16, 24), 21))  # a CPU batch for a CUDA module
    with pytest.raises(ValueError):
        cpu_module()(rand((1, 1, 16, 24), 21).to(DEV))
