"""HipSuperPointNet on the CPU (the twins): the wiring against the walk written out by hand from the public twins, each
layer's arithmetic against an fp64 conv2d of that layer's own input within the chain's derived bound, the pools and
the descriptor normalisation, closeness to the module itself, shapes, batch independence and the plan's errors."""
import functools

import pytest
import torch
from torch import nn

import fmpnp

import conv1x1_cases as cc

BODY = ["conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b"]


@functools.lru_cache(maxsize=None)
def net():
    torch.manual_seed(1234)
    return fmpnp.SuperPointNet().eval()


@functools.lru_cache(maxsize=None)
def image():
    return torch.rand((1, 1, 16, 24), generator=torch.Generator().manual_seed(21))


@functools.lru_cache(maxsize=None)
def batch():
    return torch.rand((2, 1, 24, 40), generator=torch.Generator().manual_seed(22))


@functools.lru_cache(maxsize=None)
def hand_walk():
    """SuperPointNet.forward on image() through the public twins, in its order -> (semi, desc, raw, the records
    [(name, input, output, relu)] of the twelve convolutions, the pools [(input, output)])."""
    n, x = net(), image()
    convs, pools = [], []

    def conv(name, x, relu=True):
        m = getattr(n, name)
        op = fmpnp.conv1x1_cpu if m.kernel_size == (1, 1) else fmpnp.conv3x3_cpu
        y = op(x, m.weight.detach(), m.bias.detach(), relu=relu)
        convs.append((name, x, y, relu))
        return y

    for blk in "123":
        x = conv(f"conv{blk}a", x)
        y = conv(f"conv{blk}b", x)
        x = fmpnp.maxpool2x2_cpu(y)
        pools.append((y, x))
    x = conv("conv4b", conv("conv4a", x))
    semi = conv("convPb", conv("convPa", x), relu=False)
    raw = conv("convDb", conv("convDa", x), relu=False)
    desc = fmpnp.assemble_hypercolumn_cpu([raw])
    return semi, desc, raw, convs, pools


def test_wiring_equals_the_walk_written_out_by_hand():
    semi, desc = fmpnp.HipSuperPointNet(net())(image())
    want_semi, want_desc = hand_walk()[:2]
    assert semi.shape == (1, 65, 2, 3) and desc.shape == (1, 256, 2, 3)
    assert semi.dtype == desc.dtype == torch.float32
    assert torch.equal(semi, want_semi) and torch.equal(desc, want_desc)


def test_each_layers_arithmetic_within_its_own_bound():
    """Every convolution of the hand-written walk against an fp64 conv2d of the fp32 input the walk gave it:
    |out - ref| <= gamma_{K+1} (sum |a||w| + |b|), K = Cin * kh * kw (the ReLU is 1-Lipschitz).  No error compounds,
    so no number is measured.  The pooled maps equal max_pool2d of their inputs."""
    n = net()
    _, _, _, convs, pools = hand_walk()
    assert [c[0] for c in convs] == BODY + ["convPa", "convPb", "convDa", "convDb"]
    for name, x, y, relu in convs:
        m = getattr(n, name)
        w, b = m.weight.detach(), m.bias.detach()
        ref = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), padding=m.padding)
        ref = torch.relu(ref) if relu else ref
        bnd = cc.chain_bound(x, w, b, w.shape[1] * w.shape[2] * w.shape[3])
        err = (y.double() - ref).abs()
        print(f"{name}: max error / bound {float((err / bnd.clamp_min(1e-300)).max()):.3g}")
        assert y.shape == ref.shape and bool((err <= bnd).all()), name
    assert len(pools) == 3
    for x, y in pools:
        assert torch.equal(y, torch.nn.functional.max_pool2d(x, 2, 2))


def test_descriptor_normalisation_within_three_ulp():
    """desc = fl32(raw / fl32(sqrt(S))), S the fp64 sum of squares; the yardstick is fl32(raw / sqrt(S)) formed in
    fp64.  Three roundings separate the two -- the norm's to fp32, the division's, the yardstick's -- each a relative
    error of at most u = 2^-24, which is below one ulp of the value: at most 3 ulp (the fp64 terms are 2^-29 of
    one)."""
    _, desc, raw, _, _ = hand_walk()
    want = (raw.double() / raw.double().norm(dim=1, keepdim=True)).float()
    assert bool(torch.isfinite(desc).all()) and bool((desc.sign() == want.sign()).all())
    ulps = (desc.view(torch.int32) - want.view(torch.int32)).abs().max()
    print(f"desc: {int(ulps)} ulp at most from raw / ||raw|| in fp64")
    assert int(ulps) <= 3


def test_close_to_the_module_itself():
    """A gross check of the wiring against SuperPointNet.forward: atol 1e-3 is loose by three orders of magnitude
    against fp32 noise at these sizes."""
    with torch.no_grad():
        want_semi, want_desc = net()(image())
    semi, desc = fmpnp.HipSuperPointNet(net())(image())
    print(f"max |semi - torch| {float((semi - want_semi).abs().max()):.3g}, "
          f"max |desc - torch| {float((desc - want_desc).abs().max()):.3g}")
    assert torch.allclose(semi, want_semi, rtol=0, atol=1e-3) and torch.allclose(desc, want_desc, rtol=0, atol=1e-3)


def test_shapes_floor_and_too_small():
    hip = fmpnp.HipSuperPointNet(net())
    img = torch.rand((1, 1, 18, 29), generator=torch.Generator().manual_seed(23))
    semi, desc = hip(img)
    assert semi.shape == (1, 65, 2, 3) and desc.shape == (1, 256, 2, 3)
    for h, w in ((7, 24), (16, 7)):
        with pytest.raises(ValueError):
            hip(torch.rand(1, 1, h, w))
    for bad in (torch.rand(1, 16, 24), torch.rand(1, 3, 16, 24), torch.rand(1, 1, 16, 24).double()):
        with pytest.raises(ValueError):
            hip(bad)


def test_batch_item_equals_its_own_call():
    hip = fmpnp.HipSuperPointNet(net())
    semi, desc = hip(batch())
    assert semi.shape == (2, 65, 3, 5) and desc.shape == (2, 256, 3, 5)
    one_semi, one_desc = hip(batch()[1:2].contiguous())
    assert torch.equal(semi[1], one_semi[0]) and torch.equal(desc[1], one_desc[0])


def fresh():
    torch.manual_seed(5)
    return fmpnp.SuperPointNet().eval()


def test_plan_errors():
    n = fresh()
    n.convPb = nn.Conv2d(256, 65, 3, padding=1)
    with pytest.raises(TypeError, match="convPb"):
        fmpnp.HipSuperPointNet(n)
    n = fresh()
    n.conv2a = nn.Conv2d(64, 64, 1)
    with pytest.raises(TypeError, match="conv2a"):
        fmpnp.HipSuperPointNet(n)
    n = fresh()
    del n.convDa
    with pytest.raises(TypeError, match="convDa"):
        fmpnp.HipSuperPointNet(n)
    with pytest.raises(TypeError, match="conv1a"):
        fmpnp.HipSuperPointNet(fresh().double())
    n = fresh()
    with torch.no_grad():
        n.convDb.bias[3] = float("inf")
    with pytest.raises(ValueError, match="convDb"):
        fmpnp.HipSuperPointNet(n)
    with pytest.raises(ValueError):
        fmpnp.HipSuperPointNet(fresh(), precision="bf16")
    n = fresh()
    with torch.no_grad():
        n.conv3a.weight[0, 0, 0, 0] = 65520.0
    fmpnp.HipSuperPointNet(n)  # (finite: the exact precision takes it)
    with pytest.raises(ValueError, match="conv3a"):
        fmpnp.HipSuperPointNet(n, precision="f16")
    n = fresh()
    with torch.no_grad():
        n.convPb.weight[0, 0, 0, 0] = 65520.0
    fmpnp.HipSuperPointNet(n, precision="f16")  # (the heads stay fp32: no binary16 limit on them)


class OtherNet(nn.Module):
    """Not fmpnp.SuperPointNet: the twelve attributes, declared in another order, and a forward of its own."""

    def __init__(self):
        super().__init__()
        self.convDb, self.convDa = nn.Conv2d(256, 256, 1), nn.Conv2d(128, 256, 3, padding=1)
        self.convPb, self.convPa = nn.Conv2d(256, 65, 1), nn.Conv2d(128, 256, 3, padding=1)
        for name, (cin, cout) in dict(conv1a=(1, 64), conv1b=(64, 64), conv2a=(64, 64), conv2b=(64, 64), conv3a=(64, 128),
                                      conv3b=(128, 128), conv4a=(128, 128), conv4b=(128, 128)).items():
            setattr(self, name, nn.Conv2d(cin, cout, 3, padding=1))

    def forward(self, x):
        raise NotImplementedError


def test_other_classes_with_the_twelve_attributes():
    torch.manual_seed(8)
    other = OtherNet().eval()
    ours = fmpnp.SuperPointNet().eval()
    ours.load_state_dict(other.state_dict())
    hip = fmpnp.HipSuperPointNet(other)
    assert hip.net is other and len(list(hip.parameters())) == 24 and set(hip.state_dict()) == {
        f"net.{k}" for k in other.state_dict()}
    semi, desc = hip(image())
    want_semi, want_desc = fmpnp.HipSuperPointNet(ours)(image())
    assert torch.equal(semi, want_semi) and torch.equal(desc, want_desc)


def test_f16_on_the_cpu_runs_the_reference():
    """precision="f16" on the CPU: the ten 3x3 convolutions through the fp16 reference (not a twin), the heads through
    conv1x1_cpu; finite outputs of the right shapes."""
    semi, desc = fmpnp.HipSuperPointNet(net(), precision="f16")(image())
    assert semi.shape == (1, 65, 2, 3) and desc.shape == (1, 256, 2, 3)
    assert bool(torch.isfinite(semi).all()) and bool(torch.isfinite(desc).all())
