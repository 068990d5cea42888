"""Hypercolumn assembly on the GPU: the kernel against its CPU twin bit for bit on every case (4-byte and
16-byte stores), views in and out with the surrounding bytes untouched, a side stream, and
HypercolumnExtractor end to end into the sparse gather and the exhaustive search."""
import numpy as np
import pytest
import torch

import fmpnp

import hypercolumn_cases as hc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(maps):
    return [m.to(DEV) for m in maps]  # (copies: the shared inputs are read-only; strides are not preserved)


@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("name", [n for n in hc.ALL if n != "views"])
def test_gpu_equals_the_twin(name, normalize):
    """== on every element, NaNs at the same positions, with the library's choice of stores, the 4-byte and the
    16-byte ones (the results do not depend on the launch)."""
    maps, size = hc.inputs(name)
    want = hc.twin(name, normalize)
    for stores in (None, "dword", "vector"):
        got = fmpnp.assemble_hypercolumn(dev(maps), size=size, normalize=normalize, stores=stores)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape
        assert hc.same_floats(got.cpu(), want), (name, normalize, stores)


def test_gpu_equal_size_without_normalisation_is_a_copy():
    (m,), _ = hc.inputs("single")
    assert torch.equal(fmpnp.assemble_hypercolumn(dev([m]), normalize=False).cpu(), m)


def test_gpu_zero_texel_and_nonfinite_masks_equal_the_restatements():
    for name in hc.POISONED:
        maps, _ = hc.inputs(name)
        got = fmpnp.assemble_hypercolumn(dev(maps)).cpu()
        for dtype in (torch.float32, torch.float64):
            r = hc.ref(maps, dtype)
            assert torch.equal(torch.isnan(got), torch.isnan(r)) and torch.equal(torch.isinf(got), torch.isinf(r))
    got = fmpnp.assemble_hypercolumn(dev(hc.inputs("zero_texel")[0])).cpu()
    want = torch.zeros_like(got, dtype=torch.bool)
    want[:, :, 0, 0] = True
    assert torch.equal(torch.isnan(got), want)


def _strided_on_device(maps):
    """The views case's sources on the device with their strides: the wider tensors are rebuilt there."""
    out = []
    for m in maps:
        big = torch.full((3, m.shape[1] + 2, m.shape[2] + 1, m.shape[3] + 3), float("nan"), device=DEV)
        view = big[1:, 1:m.shape[1] + 1, :m.shape[2], 2:2 + m.shape[3]]
        view.copy_(m)
        assert view.stride() == m.stride() and not view.is_contiguous()
        out.append(view)
    return out


@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "raw"])
def test_gpu_views(normalize):
    """B = 2, strided sources, an out= view one float into a larger buffer with padded rows: the view equals
    the twin and every other element of the buffer keeps its value."""
    maps, _ = hc.inputs("views")
    want = hc.twin("views", normalize)
    buf, view = hc.view_out(*want.shape, device=DEV)
    assert view.data_ptr() % 16 == 4
    for stores in (None, "vector"):  # (no alignment: the 16-byte request falls back to 4-byte stores)
        got = fmpnp.assemble_hypercolumn(_strided_on_device(maps), normalize=normalize, out=view, stores=stores)
        assert got.data_ptr() == view.data_ptr()
        assert hc.same_floats(view.cpu(), want)
        view.fill_(-7.0)
        assert bool((buf == -7.0).all())


def test_gpu_side_stream():
    maps, _ = hc.inputs("vgg16x")
    d = dev(maps)
    base = fmpnp.assemble_hypercolumn(d)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    got = fmpnp.assemble_hypercolumn(d, stream=side, stores="vector")
    side.synchronize()
    assert torch.equal(got, base) and hc.same_floats(got.cpu(), hc.twin("vgg16x"))


def test_gpu_argument_errors():
    m = torch.zeros(1, 2, 3, 3, device=DEV)
    with pytest.raises(ValueError):
        fmpnp.assemble_hypercolumn([m.cpu()])
    with pytest.raises(ValueError):
        fmpnp.assemble_hypercolumn([m], out=torch.zeros(1, 2, 3, 4, device=DEV))
    with pytest.raises(ValueError):
        fmpnp.assemble_hypercolumn([m] * 9)


def test_gpu_extractor_end_to_end():
    """compute_hypercolumn on the tiny encoder: within the restatement's tolerance of ref(fp64) on the device,
    equal to the kernel on the recorded maps, and consumed as it is by the sparse gather and the search."""
    net, image = hc.tiny_encoder().to(DEV), hc.tiny_image().to(DEV)
    ex = fmpnp.HypercolumnExtractor(net, hc.ENCODER_LAYERS)
    hyper, resolution = ex.compute_hypercolumn(image)
    assert hyper.is_cuda and tuple(hyper.shape) == (1, 32, 20, 28) and tuple(resolution) == (20, 28)
    maps = hc.restated_walk(net, image)
    assert torch.equal(hyper, fmpnp.assemble_hypercolumn(maps))
    assert hc.same_floats(hyper.cpu(), fmpnp.assemble_hypercolumn_cpu([m.cpu() for m in maps]))
    r32, r64 = hc.ref(maps, torch.float32), hc.ref(maps, torch.float64)
    assert r64.is_cuda
    bound, e_ref = hc.tolerance(r32, r64)
    err = hc.max_error(hyper, r64)
    print(f"extractor: error {err:.3g}, e_ref {e_ref:.3g}, bound {bound:.3g}")
    assert err <= bound

    width, height = hyper.shape[2:]
    grid, cell = fmpnp.generate_dense_keypoints((width, height), (160, 224))
    rng = np.random.default_rng(5)
    keypoints = [np.stack([rng.uniform(0, 224, 40), rng.uniform(0, 160, 40)])]
    copy = hyper.contiguous().clone()
    (sparse,), (sparse_copy,) = (fmpnp.fast_sparse_keypoint_descriptor(keypoints, grid, h) for h in (hyper, copy))
    assert torch.equal(sparse, sparse_copy) and tuple(sparse.shape) == (40, 32)
    found = [fmpnp.exhaustive_search(h.squeeze().view(32, -1), sparse, (160, 224), (width, height), cell, factor=0.1)
             for h in (hyper, copy)]
    assert torch.equal(found[0][0], found[1][0]) and (found[0][1] == found[1][1]).all()
