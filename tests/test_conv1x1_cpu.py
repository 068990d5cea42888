"""The 1x1 convolution's CPU twin (fmpnp_conv1x1_cpu, fmpnp.conv1x1_cpu): the indexing against torch's fp64 conv2d on
exact integers, the rounding within the chain's derived bound, thread independence, guard bands, the two weight
layouts, the argument errors of the Python and the C forms (host checks: nothing is launched)."""
import ctypes

import pytest
import torch

import fmpnp
from fmpnp import _lib

import conv1x1_cases as cc

NEW = ["fmpnp_conv1x1_async", "fmpnp_conv1x1", "fmpnp_conv1x1_cpu"]


def test_exports_and_abi():
    L = _lib.load()
    assert set(NEW) <= set(_lib.EXPORTS) and all(hasattr(L, n) for n in NEW)
    assert L.fmpnp_abi_version() == 4  # (exports were only added)


@pytest.mark.parametrize("bias,relu", cc.FLAGS, ids=cc.FLAG_IDS)
@pytest.mark.parametrize("shape", cc.SHAPES, ids=cc.IDS)
def test_twin_equals_torch_on_integers(shape, bias, relu):
    """Small integers: every partial sum is exact, so == against conv2d in fp64 pins the indexing against torch."""
    got, want = cc.twin(shape, "int", bias, relu), cc.ref64(shape, "int", bias, relu)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got.double(), want)


@pytest.mark.parametrize("bias,relu", cc.FLAGS, ids=cc.FLAG_IDS)
@pytest.mark.parametrize("shape", cc.SHAPES, ids=cc.IDS)
def test_twin_rounding_threads_and_guards(shape, bias, relu):
    """|twin - conv2d(fp64)| <= gamma_{Cin+1} (sum |a||w| + |b|) on every element (the ReLU is 1-Lipschitz); the same
    bits from 1 and 3 threads; nothing written outside the output."""
    x, w, b = cc.operands(shape, "gauss")
    got = cc.twin(shape, "gauss", bias, relu)
    err, bnd = (got.double() - cc.ref64(shape, "gauss", bias, relu)).abs(), cc.bound(shape, "gauss", bias)
    print(f"{shape} bias={bias} relu={relu}: max error {float(err.max()):.3g}, "
          f"max error / bound {float((err / bnd.clamp_min(1e-300)).max()):.3g}")
    assert bool((err <= bnd).all())
    for n in (1, 3):
        buf, out, pad = cc.guarded(tuple(got.shape), "cpu")
        assert fmpnp.conv1x1_cpu(x, w, b if bias else None, relu=relu, out=out, n_threads=n) is out
        assert cc.guards_intact(buf, pad) and torch.equal(out, got), n


def test_twin_both_weight_layouts():
    x, w, b = cc.operands(cc.SHAPES[2], "gauss")
    assert w.dim() == 4
    flat = w.reshape(w.shape[0], w.shape[1])
    assert torch.equal(fmpnp.conv1x1_cpu(x, flat, b, relu=True), cc.twin(cc.SHAPES[2], "gauss", True, True))
    assert torch.equal(fmpnp.conv1x1_cpu(x, flat), cc.twin(cc.SHAPES[2], "gauss", False, False))


def test_twin_batch_items_equal_single_calls():
    for shape in (cc.SHAPES[2], cc.SHAPES[5]):
        x, w, b = cc.operands(shape, "gauss")
        whole = cc.twin(shape, "gauss", True, False)
        for i in range(shape[0]):
            assert torch.equal(fmpnp.conv1x1_cpu(x[i:i + 1].contiguous(), w, b)[0], whole[i]), (shape, i)


def test_python_argument_errors():
    x, w, b = cc.operands(cc.SHAPES[1], "gauss")
    for bad in (dict(x=x[0]), dict(x=x.double()), dict(x=x.transpose(2, 3)), dict(weight=w[:, :2].contiguous()),
                dict(weight=w.double()), dict(weight=torch.zeros(5, 3, 3, 3)), dict(weight=torch.zeros(5, 3, 1)),
                dict(weight=w.expand(5, 3, 1, 2)), dict(bias=b[:3].contiguous()), dict(bias=b.double()),
                dict(out=torch.empty(1, 5, 5, 6)), dict(out=torch.empty(1, 5, 5, 7, dtype=torch.float64)),
                dict(x=torch.empty(0, 3, 5, 7))):
        kw = dict(x=x, weight=w, bias=b)
        kw.update(bad)
        with pytest.raises(ValueError):
            fmpnp.conv1x1_cpu(**kw)
    with pytest.raises(TypeError):
        fmpnp.conv1x1_cpu(x, w, b, precision="f16")  # there is no precision argument


def test_c_entry_points_validate_without_a_device():
    """FMPNP_EINVAL / FMPNP_ETOOBIG of all three forms are decided on the host, before anything touches a device."""
    L = _lib.load()
    x, w, b = cc.operands(cc.SHAPES[1], "gauss")
    out = torch.empty(1, 5, 5, 7)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    good = dict(x=vp(x), B=1, Cin=3, H=5, W=7, w=vp(w), b=vp(b), Cout=5, flags=3, out=vp(out))
    bads = [dict(B=0), dict(Cin=0), dict(H=0), dict(W=-1), dict(Cout=0), dict(flags=4), dict(b=None, flags=1),
            dict(x=None), dict(w=None), dict(out=None)]
    big = [dict(H=65536, W=32768), dict(B=4, Cin=2, H=32768, W=8192), dict(Cout=1 << 30, H=3, W=3),
           dict(Cin=1 << 16, Cout=1 << 15, H=1, W=1)]
    for fn, last in ((L.fmpnp_conv1x1_async, None), (L.fmpnp_conv1x1, None), (L.fmpnp_conv1x1_cpu, 1)):
        for bad, want in [(k, _lib.EINVAL) for k in bads] + [(k, _lib.ETOOBIG) for k in big]:
            a = dict(good)
            a.update(bad)
            rc = fn(a["x"], a["B"], a["Cin"], a["H"], a["W"], a["w"], a["b"], a["Cout"], a["flags"], a["out"], last)
            assert rc == want, (fn.__name__, bad, rc)
    assert L.fmpnp_conv1x1_cpu(*[good[k] for k in ("x", "B", "Cin", "H", "W", "w", "b", "Cout", "flags", "out")], -1) \
        == _lib.EINVAL
    assert L.fmpnp_conv1x1_cpu(*[good[k] for k in ("x", "B", "Cin", "H", "W", "w", "b", "Cout", "flags", "out")], 2) == 0
    assert torch.equal(out, cc.twin(cc.SHAPES[1], "gauss", True, True))
