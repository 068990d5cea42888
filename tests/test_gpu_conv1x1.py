"""The 1x1 convolution's kernel on the GPU (fmpnp.conv1x1): its indexing against torch's fp64 conv2d on exact
integers, the kernel against its CPU twin bit for bit and within the chain's derived bound on every shape, launch
independence (batch, stream, the load width, the match stage's own correlation) and the argument errors.  The
references are computed on the CPU: the framework's own GPU convolution may take an algorithm that is not exact
even on integers."""
import pytest
import torch

import fmpnp

import conv1x1_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run(shape, kind, bias, relu, **kw):
    x, w, b = (t.to(DEV) for t in cc.operands(shape, kind))
    return fmpnp.conv1x1(x, w, b if bias else None, relu=relu, **kw)


@pytest.mark.parametrize("bias,relu", cc.FLAGS, ids=cc.FLAG_IDS)
@pytest.mark.parametrize("shape", cc.SHAPES, ids=cc.IDS)
def test_gpu_equals_torch_on_integers(shape, bias, relu):
    """Small integers: every partial sum is exact, so == against conv2d in fp64 pins the indexing, the k range and the
    tiles' edges against torch."""
    got = run(shape, "int", bias, relu)
    assert got.is_cuda and got.dtype == torch.float32
    assert torch.equal(got.cpu().double(), cc.ref64(shape, "int", bias, relu))


@pytest.mark.parametrize("bias,relu", cc.FLAGS, ids=cc.FLAG_IDS)
@pytest.mark.parametrize("shape", cc.SHAPES, ids=cc.IDS)
def test_gpu_equals_the_twin_within_the_chains_bound(shape, bias, relu):
    """Gaussian operands: torch.equal with the twin (the MFMA chain is the fmaf chain), within
    gamma_{Cin+1} (sum |a||w| + |b|) of conv2d in fp64, and nothing is stored outside the output."""
    buf, out, pad = cc.guarded((shape[0], shape[2], shape[3], shape[4]), DEV)
    got = run(shape, "gauss", bias, relu, out=out)
    assert got is out
    got = got.cpu()
    err = (got.double() - cc.ref64(shape, "gauss", bias, relu)).abs()
    bnd = cc.bound(shape, "gauss", bias)
    same = torch.equal(got, cc.twin(shape, "gauss", bias, relu))
    print(f"{shape} bias={bias} relu={relu}: equals the twin: {same}; max error / bound "
          f"{float((err / bnd.clamp_min(1e-300)).max()):.3g}")
    assert cc.guards_intact(buf, pad)
    assert bool((err <= bnd).all())
    assert same


def test_gpu_batch_items_equal_single_calls():
    for shape in (cc.SHAPES[2], cc.SHAPES[5]):  # (odd P: image 1's planes are misaligned; B = 3 on the 16-byte path)
        x, w, b = (t.to(DEV) for t in cc.operands(shape, "gauss"))
        whole = fmpnp.conv1x1(x, w, b, relu=True)
        for i in range(shape[0]):
            assert torch.equal(fmpnp.conv1x1(x[i:i + 1].contiguous(), w, b, relu=True)[0], whole[i]), (shape, i)


def test_gpu_side_stream_equals_the_default_stream():
    shape = cc.SHAPES[3]
    x, w, b = (t.to(DEV) for t in cc.operands(shape, "gauss"))
    want = fmpnp.conv1x1(x, w, b, relu=True)
    torch.cuda.synchronize()
    # (a high-priority stream: the framework hands streams out of one round-robin pool per priority, and tests
    # elsewhere in the suite that time two default-priority streams against each other depend on which two they draw)
    side = torch.cuda.Stream(device=DEV, priority=-1)
    got = fmpnp.conv1x1(x, w, b, relu=True, stream=side)
    side.synchronize()
    assert torch.equal(got, want)


@pytest.mark.parametrize("shape", [cc.SHAPES[3], cc.SHAPES[8]], ids=[cc.IDS[3], cc.IDS[8]])
def test_gpu_load_width_changes_no_bit(shape):
    """P % 4 == 0 from an aligned base takes the 16-byte loads; the same tensor one float into an allocation takes
    the 4-byte loads.  Same bits, in both forms of the kernel."""
    x, w, b = (t.to(DEV) for t in cc.operands(shape, "gauss"))
    shifted = torch.cat([torch.zeros(1, device=DEV), x.reshape(-1)])[1:].view(x.shape)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
    assert torch.equal(fmpnp.conv1x1(shifted, w, b), fmpnp.conv1x1(x, w, b))


def test_gpu_equals_the_match_stages_score_map():
    """conv1x1(x, w)[b] is the correlation of sparse = w with dense = x[b]: the match stage's score map bit for bit."""
    shape = cc.SHAPES[2]
    x, w, _ = (t.to(DEV) for t in cc.operands(shape, "gauss"))
    got = fmpnp.conv1x1(x, w)
    flat = w.reshape(shape[2], shape[1]).contiguous()
    for i in range(shape[0]):
        scores = fmpnp.exhaustive_match(flat, x[i].reshape(shape[1], -1), top_k=1, scores=True)["scores"]
        assert torch.equal(scores.reshape(got[i].shape), got[i]), i


def test_gpu_argument_errors_launch_nothing():
    x, w, b = (t.to(DEV) for t in cc.operands(cc.SHAPES[1], "gauss"))
    for bad in (dict(x=x[0]), dict(x=x.double()), dict(x=x.transpose(2, 3)), dict(x=x.cpu()),
                dict(weight=w[:, :2].contiguous()), dict(weight=w.cpu()), dict(weight=torch.zeros(5, 3, 3, 3, device=DEV)),
                dict(bias=b[:3].contiguous()), dict(bias=b.cpu()), dict(out=torch.empty(1, 5, 5, 6, device=DEV)),
                dict(out=torch.empty(1, 5, 5, 7))):
        kw = dict(x=x, weight=w, bias=b)
        kw.update(bad)
        with pytest.raises(ValueError):
            fmpnp.conv1x1(**kw)
