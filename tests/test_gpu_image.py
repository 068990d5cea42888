"""The image front end on the GPU: fmpnp.resize_lanczos against the CPU twin and Pillow's recorded results
(tests/golden/image_lanczos.npz) under ==, fmpnp.image_to_tensor against the twin under torch.equal for the four
transforms, guard words around both kinds of output, launch independence (batch, stream, strides, the table cache) and
the two extractors from a uint8 array end to end.  No Pillow is needed here: the fixture holds its results."""
import copy

import numpy as np
import pytest
import torch

import fmpnp

import dense_cases as dc
import encoder_cases as ec
import image_cases as ic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return (torch.from_numpy(a) if isinstance(a, np.ndarray) else a).to(DEV)


def guarded_u8(shape, pad=64):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[pad:pad + n].view(shape), pad


def u8_guards_intact(buf, pad):
    return bool((buf[:pad] == 0xA5).all()) and bool((buf[-pad:] == 0xA5).all())


# ---- the resize -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind", ic.CASES, ids=ic.CASE_IDS)
def test_gpu_resize_equals_twin_and_pillow_fixture(shape, kind):
    a, want = ic.fixture(shape, kind)
    buf, out, pad = guarded_u8(shape[2:] + (3,))
    got = fmpnp.resize_lanczos(dev(a), shape[2:], out=out)
    assert got.is_cuda and got.dtype == torch.uint8 and got.data_ptr() == out.data_ptr()
    assert u8_guards_intact(buf, pad)
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got.cpu(), fmpnp.resize_lanczos_cpu(a, shape[2:]))


def test_gpu_resize_with_coefficients_left_in_global_memory():
    """A shrink of 100 along a row: 601 coefficients per output column, more than the horizontal pass stages in LDS."""
    a = ic.make_input((3, 500), "random")
    assert torch.equal(fmpnp.resize_lanczos(dev(a), (2, 5)).cpu(), fmpnp.resize_lanczos_cpu(a, (2, 5)))
    assert np.array_equal(fmpnp.resize_lanczos_cpu(a, (2, 5)).numpy(), ic.restate_resize(a, (2, 5)))


# ---- the value transforms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preprocessing", ic.TRANSFORMS, ids=[str(t) for t in ic.TRANSFORMS])
@pytest.mark.parametrize("shape", ic.SHAPES, ids=ic.SHAPE_IDS)
def test_gpu_to_tensor_equals_twin(shape, preprocessing):
    a = ic.make_input(shape[:2], "random")
    want = fmpnp.image_to_tensor_cpu(a, shape[2:], preprocessing)
    buf, out, pad = ec.guarded(tuple(want.shape), DEV)
    got = fmpnp.image_to_tensor(dev(a), shape[2:], preprocessing, out=out)
    assert got.data_ptr() == out.data_ptr() and ec.guards_intact(buf, pad)
    assert torch.equal(got.cpu(), want)


def test_gpu_to_tensor_on_every_byte_and_options():
    u8 = torch.from_numpy(ic.all_bytes_image())
    for pre in ic.TRANSFORMS:
        assert torch.equal(fmpnp.image_to_tensor(dev(u8), preprocessing=pre).cpu(), ic.torch_transform(u8, pre)), pre
    mean, std = (0.5, 0.25, 0.125), (0.3, 0.2, 0.1)
    assert torch.equal(fmpnp.image_to_tensor(dev(u8), preprocessing="torch", mean=mean, std=std).cpu(),
                       ic.torch_transform(u8, "torch", mean, std))
    assert torch.equal(fmpnp.image_to_tensor(dev(u8), preprocessing="caffe", mean=(1.5, 2.5, 3.5)).cpu(),
                       ic.torch_transform(u8, "caffe", (1.5, 2.5, 3.5)))
    for swap in (True, False):
        assert torch.equal(fmpnp.image_to_tensor(dev(u8), preprocessing="gray", swap_rb=swap).cpu(),
                           ic.torch_transform(u8, "gray", swap_rb=swap))


# ---- launch independence --------------------------------------------------------------------------------------------
BATCH_SHAPES = [(37, 53, 16, 24), (37, 53, 37, 20), (37, 53, 11, 53), (37, 53, 37, 53)]


@pytest.mark.parametrize("shape", BATCH_SHAPES, ids=["%dx%d-%dx%d" % s for s in BATCH_SHAPES])
def test_gpu_batch_equals_single_calls(shape):
    a = np.stack([ic.make_input(shape[:2], k) for k in ic.KINDS])
    size = shape[2:]
    got_u8, got_f = fmpnp.resize_lanczos(dev(a), size), fmpnp.image_to_tensor(dev(a), size, "torch")
    got_g = fmpnp.image_to_tensor(dev(a), size, "gray")
    assert torch.equal(got_u8.cpu(), fmpnp.resize_lanczos_cpu(a, size))
    for b in range(3):
        assert torch.equal(fmpnp.resize_lanczos(dev(a[b]), size), got_u8[b])
        assert torch.equal(fmpnp.image_to_tensor(dev(a[b]), size, "torch")[0], got_f[b])
        assert torch.equal(fmpnp.image_to_tensor(dev(a[b:b + 1]), size, "gray")[0], got_g[b])


def test_gpu_stream_independence():
    """The non-default stream comes from the framework's high-priority pool, so the default pool's round-robin position,
    which decides which streams the later tests of a whole-suite run are handed, stays where it was."""
    a = dev(ic.make_input((96, 128), "random"))
    want_u8, want_f = fmpnp.resize_lanczos(a, (25, 33)), fmpnp.image_to_tensor(a, (25, 33), "caffe")
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV, priority=-1)
    got_u8, got_f = fmpnp.resize_lanczos(a, (25, 33), stream=s), fmpnp.image_to_tensor(a, (25, 33), "caffe", stream=s)
    s.synchronize()
    assert torch.equal(got_u8, want_u8) and torch.equal(got_f, want_f)
    with torch.cuda.stream(s):
        again = fmpnp.image_to_tensor(a, (25, 33), "caffe")
    s.synchronize()
    assert torch.equal(again, want_f)


@pytest.mark.parametrize("size", [(16, 24), (37, 20), (11, 53), (37, 53)])
def test_gpu_strided_crop_equals_its_contiguous_copy(size):
    """The crop starts at an odd byte offset with a row stride that is no multiple of 4 (the byte-load path); the copy is
    4-byte aligned (the dword path) whenever its row length allows."""
    big = dev(np.stack([ic.make_input((45, 65), "random", seed=s) for s in range(2)]))
    view = big[:, 3:40, 5:58]
    assert not view.is_contiguous() and tuple(view.shape) == (2, 37, 53, 3)
    packed = view.contiguous()
    want = fmpnp.resize_lanczos_cpu(packed.cpu(), size)
    assert torch.equal(fmpnp.resize_lanczos(view, size).cpu(), want)
    assert torch.equal(fmpnp.resize_lanczos(packed, size).cpu(), want)
    for pre in ("torch", "gray"):
        assert torch.equal(fmpnp.image_to_tensor(view, size, pre), fmpnp.image_to_tensor(packed, size, pre))
    # aligned rows (3 w a multiple of 4) with a strided source: 52 columns
    view4 = big[:, 3:40, 4:56]
    assert torch.equal(fmpnp.resize_lanczos(view4, (20, 52)).cpu(), fmpnp.resize_lanczos_cpu(view4.cpu(), (20, 52)))
    assert torch.equal(fmpnp.image_to_tensor(view4, (20, 52)).cpu(), fmpnp.image_to_tensor_cpu(view4.cpu(), (20, 52)))
    # ... and their packed copy: a vertical pass alone that reads the caller's rows by dwords
    assert torch.equal(fmpnp.resize_lanczos(view4.contiguous(), (20, 52)), fmpnp.resize_lanczos(view4, (20, 52)))


def test_gpu_table_cache_reuse():
    """A size pair, five others (more axis tables than the cache holds), then the first pair again."""
    a = dev(ic.make_input((37, 53), "random"))
    first = fmpnp.resize_lanczos(a, (16, 24)).clone()
    for size in [(11, 20), (30, 40), (17, 29), (64, 80), (9, 9)]:
        got = fmpnp.resize_lanczos(a, size)
        assert torch.equal(got.cpu(), fmpnp.resize_lanczos_cpu(a.cpu(), size)), size
    assert torch.equal(fmpnp.resize_lanczos(a, (16, 24)), first)
    assert torch.equal(first.cpu(), fmpnp.resize_lanczos_cpu(a.cpu(), (16, 24)))
    # back to back without a look in between: the second call's tables replace cached ones while the first is queued
    x, y = fmpnp.resize_lanczos(a, (21, 33)), fmpnp.resize_lanczos(a, (13, 47))
    z = fmpnp.resize_lanczos(a, (21, 33))
    assert torch.equal(x, z) and torch.equal(y.cpu(), fmpnp.resize_lanczos_cpu(a.cpu(), (13, 47)))


def test_gpu_argument_errors_launch_nothing():
    a = dev(ic.make_input((8, 8), "random"))
    with pytest.raises(ValueError):
        fmpnp.resize_lanczos(a.cpu(), (4, 4))
    with pytest.raises(ValueError):
        fmpnp.image_to_tensor(a, (4, 4), out=torch.empty(1, 3, 4, 4))
    with pytest.raises(fmpnp._lib.FmpnpError, match="ETOOBIG"):
        fmpnp.resize_lanczos(a, (4, 16385))


# ---- end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image_size", [1024, 40], ids=["fits", "thumbnail"])
def test_gpu_hypercolumn_extractor_from_uint8(image_size):
    """From a 48 x 64 uint8 array to the hypercolumn: the loader's tensor is the twin's, so is the hypercolumn."""
    a = ic.make_input((48, 64), "random")
    size = (48, 64) if image_size == 1024 else (30, 40)
    assert fmpnp.thumbnail_size(64, 48, image_size) == size[::-1]
    net = ec.vgg16_topology().to(DEV)
    ext = fmpnp.HypercolumnExtractor(net, ec.VGG_TAPS, image_loader=fmpnp.image_loader(), backend="hip")
    got, resolution = ext.compute_hypercolumn([a], image_size, True)
    assert got.is_cuda and tuple(resolution) == size
    fed = fmpnp.image_to_tensor_cpu(a, size)
    want, _ = fmpnp.HypercolumnExtractor(net, ec.VGG_TAPS, backend="hip").compute_hypercolumn(fed)
    assert torch.equal(got, want)


@pytest.mark.parametrize("image_size", [1024, 40], ids=["fits", "thumbnail"])
def test_gpu_dense_extractor_from_uint8(image_size):
    a = ic.make_input((48, 64), "random")
    size = (48, 64) if image_size == 1024 else (30, 40)
    net = copy.deepcopy(dc.walk_trunk()).to(DEV)
    ext = fmpnp.DenseFeatureExtractor(net, image_loader=fmpnp.image_loader("caffe"))
    got, resolution = ext.compute_hypercolumn([a], image_size, True)
    assert got.is_cuda and tuple(resolution) == size
    fed = fmpnp.image_to_tensor_cpu(a, size, "caffe")
    want, _ = fmpnp.DenseFeatureExtractor(net).compute_hypercolumn(fed)
    assert torch.equal(got, want)


def test_gpu_superpoint_image():
    a = ic.make_input((24, 36), "random")
    got = fmpnp.superpoint_image(a, device=DEV)
    assert got.is_cuda and tuple(got.shape) == (1, 1, 24, 36)
    assert torch.equal(got.cpu(), fmpnp.superpoint_image(a, device="cpu"))
