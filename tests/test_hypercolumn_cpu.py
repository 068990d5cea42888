"""The hypercolumn assembly's CPU twin (fmpnp_hypercolumn_assemble_cpu) against the PyTorch restatement of
network.py:149-173 in fp64, within a tolerance taken from the restatement's own fp32 error at each run; exact
copies, batch- and thread-independence, views, the argument errors, and HypercolumnExtractor's layer walk."""
import ctypes

import pytest
import torch

import fmpnp
from fmpnp import _lib

import hypercolumn_cases as hc


@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("name", hc.ALL)
def test_twin_within_the_restatements_own_error(name, normalize):
    """|twin - ref(fp64)| <= 4 e_ref + 2^-23 max |ref(fp64)|, e_ref = max |ref(fp32) - ref(fp64)|; the NaN and
    Inf masks equal ref(fp32)'s and ref(fp64)'s."""
    maps, size = hc.inputs(name)
    got = hc.twin(name, normalize)
    r32, r64 = hc.ref(maps, torch.float32, size, normalize), hc.ref(maps, torch.float64, size, normalize)
    bound, e_ref = hc.tolerance(r32, r64)
    err = hc.max_error(got, r64)
    print(f"{name} normalize={normalize}: twin error {err:.3g}, e_ref {e_ref:.3g}, bound {bound:.3g}")
    assert got.shape == r64.shape and got.dtype == torch.float32
    for r in (r32, r64):
        assert torch.equal(torch.isnan(got), torch.isnan(r)), name
        assert torch.equal(torch.isinf(got), torch.isinf(r)), name
    assert err <= bound, (name, err, e_ref, bound)


def test_zero_texel_is_nan_there_and_nowhere_else():
    got = hc.twin("zero_texel")
    want = torch.zeros_like(got, dtype=torch.bool)
    want[:, :, 0, 0] = True
    assert torch.equal(torch.isnan(got), want)
    assert not torch.isnan(hc.twin("zero_texel", False)).any()


def test_nonfinite_inputs_reach_the_output():
    got = hc.twin("nonfinite", False)
    assert torch.isnan(got).any() and torch.isinf(got).any()


def test_equal_size_without_normalisation_is_a_copy():
    (m,), _ = hc.inputs("single")
    assert torch.equal(hc.twin("single", False), m)


def test_normalised_texels_have_unit_length():
    got = hc.twin("vgg16x").double()
    assert float(((got * got).sum(dim=1) - 1.0).abs().max()) < 1e-6


def test_batch_items_are_independent():
    maps, _ = hc.inputs("batch3")
    whole = hc.twin("batch3")
    for b in range(3):
        alone = fmpnp.assemble_hypercolumn_cpu([m[b:b + 1] for m in maps])
        assert torch.equal(alone[0], whole[b]), b


@pytest.mark.parametrize("name", ["ragged3", "blocks", "batch3"])
def test_thread_count_does_not_matter(name):
    maps, size = hc.inputs(name)
    for n in (1, 2, 5):
        assert hc.same_floats(fmpnp.assemble_hypercolumn_cpu(maps, size=size, n_threads=n), hc.twin(name))


def test_views_in_and_out():
    """Strided sources give what their contiguous copies give; an out= view inside a larger buffer is filled
    and no other element of the buffer is touched."""
    maps, _ = hc.inputs("views")
    want = fmpnp.assemble_hypercolumn_cpu([m.contiguous() for m in maps])
    assert torch.equal(hc.twin("views"), want)
    buf, view = hc.view_out(*want.shape)
    before = buf.clone()
    got = fmpnp.assemble_hypercolumn_cpu(maps, out=view)
    assert got.data_ptr() == view.data_ptr() and torch.equal(view, want)
    view.fill_(-7.0)
    assert torch.equal(buf, before)


def _layer(t):
    d = _lib.HcLayer()
    d.data, (d.C, d.H, d.W) = t.data_ptr(), t.shape[1:]
    d.stride_b, d.stride_c, d.stride_y = t.stride()[:3]
    return d


def test_argument_errors_write_nothing():
    src = torch.arange(8, dtype=torch.float32).view(1, 2, 2, 2)
    out = torch.full((1, 2, 2, 2), -7.0)
    L = _lib.load()

    def call(layers, n, batch=1, o=out.data_ptr(), h=2, w=2, sy=2, flags=_lib.HC_NORMALIZE):
        arr = (_lib.HcLayer * 9)(*layers) if layers is not None else None
        return L.fmpnp_hypercolumn_assemble_cpu(arr, n, batch, o, h, w, 8, 4, sy, flags, 1)

    good = _layer(src)
    assert call([good], 1) == 0 and not (out == -7.0).any()
    out.fill_(-7.0)
    assert call([good], 0) == _lib.EINVAL                      # L out of range
    assert call([good] * 9, 9) == _lib.EINVAL
    assert call([good], 1, batch=0) == _lib.EINVAL             # a zero dimension
    assert call([good], 1, h=0) == _lib.EINVAL
    assert call([good], 1, w=0) == _lib.EINVAL
    assert call(None, 1) == _lib.EINVAL                        # a null pointer
    assert call([good], 1, o=None) == _lib.EINVAL
    assert call([good], 1, sy=1) == _lib.EINVAL                # a row stride below the width
    assert call([good], 1, flags=8) == _lib.EINVAL
    for field, value in (("data", None), ("C", 0), ("H", 0), ("W", 0), ("stride_y", 1), ("stride_c", -1)):
        bad = _layer(src)
        setattr(bad, field, value)
        assert call([good, bad], 2) == _lib.EINVAL, field
    assert (out == -7.0).all()


def test_facade_argument_errors():
    m = torch.zeros(1, 2, 3, 3)
    with pytest.raises(ValueError):
        fmpnp.assemble_hypercolumn_cpu([])
    with pytest.raises(ValueError):
        fmpnp.assemble_hypercolumn_cpu([m] * 9)
    with pytest.raises(ValueError):
        fmpnp.assemble_hypercolumn_cpu([m.double()])
    with pytest.raises(ValueError):
        fmpnp.assemble_hypercolumn_cpu([m, torch.zeros(2, 2, 3, 3)])
    with pytest.raises(ValueError):
        fmpnp.assemble_hypercolumn_cpu([m], out=torch.zeros(1, 2, 3, 4))


def test_abi_names_and_struct():
    L = _lib.load()
    for name in ("fmpnp_hypercolumn_assemble_async", "fmpnp_hypercolumn_assemble", "fmpnp_hypercolumn_assemble_cpu"):
        assert hasattr(L, name)
    assert ctypes.sizeof(_lib.HcLayer) == 48


def test_extractor_walks_the_encoder_and_assembles():
    net, image = hc.tiny_encoder(), hc.tiny_image()
    want_maps = hc.restated_walk(net, image)
    ex = fmpnp.HypercolumnExtractor(net, hc.ENCODER_LAYERS)
    maps = ex.feature_maps(image)
    assert len(maps) == 3 and all(torch.equal(a, b) for a, b in zip(maps, want_maps))
    assert [tuple(m.shape[1:]) for m in maps] == [(8, 20, 28), (12, 10, 14), (12, 5, 7)]
    hyper, resolution = ex.compute_hypercolumn([image[0]], to_cpu=False, resize=True)
    assert tuple(resolution) == (20, 28) and tuple(hyper.shape) == (1, 32, 20, 28)
    assert torch.equal(hyper, fmpnp.assemble_hypercolumn_cpu(want_maps))
    r32, r64 = hc.ref(want_maps, torch.float32), hc.ref(want_maps, torch.float64)
    bound, _ = hc.tolerance(r32, r64)
    assert hc.max_error(hyper, r64) <= bound
    as_numpy, _ = ex.compute_hypercolumn(image, to_cpu=True)
    assert as_numpy.dtype.name == "float32" and (as_numpy == hyper.numpy()).all()
    with pytest.raises(TypeError):
        ex.compute_hypercolumn(["query.jpg"])
    loaded = fmpnp.HypercolumnExtractor(net, hc.ENCODER_LAYERS, image_loader=lambda paths, size, resize, device: image)
    assert torch.equal(loaded.compute_hypercolumn(["query.jpg"])[0], hyper)
