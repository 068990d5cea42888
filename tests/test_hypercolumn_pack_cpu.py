"""fmpnp_hypercolumn_pack_cpu, the CPU twin of the fused hypercolumn pack, against the numpy restatement of the
composed path (assemble_hypercolumn_cpu's map, the Sobel in the Sobel pack's fp64 association, one rounding, the
channels moved last).  Equalities only; no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import fmpnp
from fmpnp import _lib

import hypercolumn_pack_cases as pc


def twin(name, item=0, fill=pc.SENTINEL, out=None, **kw):
    """pack_hypercolumn_cpu into a buffer prefilled with the sentinel."""
    maps, size = pc.inputs(name)
    C, H, W, cs = pc.shape(name)
    layout, storage = kw.get("layout", "fgrad"), kw.get("storage", torch.float32)
    if out is None:
        out = np.full((H, W, 3, cs) if layout == "fgrad" else (H, W, cs), fill, pc.DTYPES[storage])
    got = fmpnp.pack_hypercolumn_cpu(maps, size=size, item=item, out=out, **kw)
    assert got is out
    return out


@pytest.mark.parametrize("name", pc.ALL)
def test_twin_equals_the_restatement(name):
    """Every case and batch item, both layouts, the four Sobel flag pairs, both storages, with and without the
    normalisation: the written elements equal the restatement, the padding channels keep the sentinel."""
    for item in pc.items(name):
        for normalize in (True, False):
            got = twin(name, item, normalize=normalize, layout="f")
            assert pc.same(got, pc.expected(name, item, normalize=normalize, layout="f")), (item, normalize, "f")
            for sn, rp in pc.FLAG_PAIRS:
                for storage in (torch.float32, torch.float64):
                    got = twin(name, item, normalize=normalize, sobel_normalized=sn, sobel_replicate_pad=rp,
                               storage=storage)
                    want = pc.expected(name, item, normalize=normalize, sobel_normalized=sn, replicate=rp,
                                       storage=storage)
                    assert pc.same(got, want), (item, normalize, sn, rp, storage)


@pytest.mark.parametrize("name", pc.hc.POISONED)
def test_poisoned_inputs_have_their_nans_where_the_composed_path_has_them(name):
    want = pc.restated(name)
    got = twin(name, fill=0.0)
    assert np.isnan(want).any() and (np.isnan(got) == np.isnan(want)).all()
    assert pc.same(got, want)


@pytest.mark.parametrize("layout", ["fgrad", "f"])
@pytest.mark.parametrize("name,channels", pc.RANGES)
def test_channel_ranges(name, channels, layout):
    """Only the range is written, and its values do not depend on it (the norm runs over all channels)."""
    got = twin(name, channels=channels, layout=layout, sobel_replicate_pad=True)
    assert pc.same(got, pc.expected(name, 0, channels=channels, layout=layout, replicate=True))


@pytest.mark.parametrize("layout", ["fgrad", "f"])
@pytest.mark.parametrize("name", ["cols33", "rows", "blocks", "one", "wide"])
def test_marks(name, layout):
    C, H, W, _ = pc.shape(name)
    for marks in (pc.random_marks(name), np.zeros((H, W), np.uint8), pc.single_mark(name)):
        got = twin(name, marks=marks, layout=layout)
        assert pc.same(got, pc.expected(name, 0, marks=marks, layout=layout))
    marks = pc.random_marks(name, seed=9)
    got = twin(name, marks=torch.from_numpy(marks.astype(bool)), channels=(1, min(C, 3)), layout=layout)
    assert pc.same(got, pc.expected(name, 0, marks=marks, channels=(1, min(C, 3)), layout=layout))


@pytest.mark.parametrize("storage", [torch.float32, torch.float64])
def test_a_padded_out_view_keeps_its_surroundings(storage):
    name = "cols33"
    C, H, W, cs = pc.shape(name)
    n = H * W * 3 * cs
    buf = np.full(3 + n + 5, pc.SENTINEL, pc.DTYPES[storage])
    view = buf[3:3 + n].reshape(H, W, 3, cs)
    twin(name, out=view, storage=storage)
    assert pc.same(view, pc.expected(name, 0, storage=storage))
    assert (buf[:3] == pc.SENTINEL).all() and (buf[3 + n:] == pc.SENTINEL).all()


@pytest.mark.parametrize("name", ["rows", "vgg16x", "batch3"])
def test_thread_counts_change_no_bit(name):
    item = len(pc.items(name)) - 1
    base = twin(name, item, n_threads=1)
    for nt in (0, 2, 5):
        assert pc.same(twin(name, item, n_threads=nt), base)


def test_without_out_the_buffer_starts_as_zeros():
    maps, size = pc.inputs("c30")
    got = fmpnp.pack_hypercolumn_cpu(maps, size=size)
    assert pc.same(got, pc.restated("c30"))
    got = fmpnp.pack_hypercolumn_cpu(maps, size=size, layout="f", channels=(7, 30))
    assert pc.same(got, pc.expected("c30", 0, channels=(7, 30), layout="f", fill=0.0))


def _call(layers, L=1, B=1, item=0, H=3, W=3, flags=1, c0=0, c1=2, layout=0, dtype=0, cs=4, sn=0, rp=0, marks=None,
          out=None, nt=1):
    return _lib.load().fmpnp_hypercolumn_pack_cpu(layers, L, B, item, H, W, flags, c0, c1, layout, dtype, cs, sn, rp,
                                                  marks, out, nt)


def test_argument_errors():
    """Every argument error returns its code and writes nothing."""
    m = torch.randn(1, 2, 3, 3)
    layers = (_lib.HcLayer * 1)()
    layers[0].data, layers[0].C, layers[0].H, layers[0].W = m.data_ptr(), 2, 3, 3
    layers[0].stride_b, layers[0].stride_c, layers[0].stride_y = 18, 9, 3
    out = np.full((3, 3, 3, 4), pc.SENTINEL, np.float32)
    o = out.ctypes.data
    assert _call(layers, out=o) == 0
    assert (out[..., :2] != pc.SENTINEL).all() and (out[..., 2:] == pc.SENTINEL).all()
    out[:] = pc.SENTINEL
    bad = [dict(L=0), dict(L=9), dict(B=0), dict(item=1), dict(item=-1), dict(H=0), dict(W=0), dict(flags=2),
           dict(flags=5), dict(c0=-1), dict(c0=2), dict(c1=3), dict(c0=1, c1=1), dict(layout=2), dict(layout=-1),
           dict(dtype=2), dict(cs=1), dict(layout=1, dtype=1), dict(layout=1, cs=6), dict(out=None), dict(nt=-1)]
    for kw in bad:
        kw.setdefault("out", o)
        assert _call(layers, **kw) == -1, kw  # FMPNP_EINVAL
    assert _call(None, out=o) == -1
    assert _call(layers, out=o + 2) == -2 and _call(layers, out=o + 4, dtype=1) == -2  # FMPNP_EALIGN
    assert _call(layers, H=1 << 25, out=o) == -4                                     # FMPNP_ETOOBIG
    layers[0].stride_y = 2
    assert _call(layers, out=o) == -1
    assert (out == pc.SENTINEL).all()
    # the workspace of the device entry point: 4 H W rounded up to 256; 0 for an invalid size
    L = _lib.load()
    assert L.fmpnp_hypercolumn_pack_workspace_size(3, 5) == 256 and L.fmpnp_hypercolumn_pack_workspace_size(0, 5) == 0
    assert L.fmpnp_hypercolumn_pack_workspace_size(256, 256) == 256 * 256 * 4
    # ... and the device entry points validate before any device call
    for fn in (L.fmpnp_hypercolumn_pack_async, L.fmpnp_hypercolumn_pack):
        assert fn(layers, 1, 1, 0, 3, 3, 1, 0, 2, 0, 0, 4, 0, 0, None, None, None, 0, None) == -1
    layers[0].stride_y = 3
    assert L.fmpnp_hypercolumn_pack_async(layers, 1, 1, 0, 3, 3, 1, 0, 2, 0, 0, 4, 0, 0, None, ctypes.c_void_p(o),
                                          None, 0, None) == -1  # (normalised, no workspace)


def test_python_argument_errors():
    m = torch.randn(1, 2, 3, 3)
    for kw in (dict(layout="x"), dict(storage=torch.float16), dict(layout="f", storage=torch.float64), dict(item=1),
               dict(channels=(1, 1)), dict(channels=(0, 3)), dict(marks=np.zeros((2, 3), np.uint8)),
               dict(marks=np.zeros((3, 3), np.float32)), dict(out=np.zeros((3, 3, 3, 4), np.float64)),
               dict(out=np.zeros((3, 3, 4), np.float32)), dict(out=np.zeros((3, 3, 3, 8), np.float32)[..., :4])):
        with pytest.raises(ValueError):
            fmpnp.pack_hypercolumn_cpu([m], **kw)
    with pytest.raises(ValueError):
        fmpnp.pack_hypercolumn_cpu([m.double()])


def test_feature_pnp_refuses_both_query_forms():
    m = torch.randn(1, 2, 3, 3)
    with pytest.raises(ValueError):
        fmpnp.feature_pnp(m, m, None, np.eye(3), (8, 8), query_layers=[m])
