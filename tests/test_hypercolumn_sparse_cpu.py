"""Sparse hypercolumns, CPU twin (fmpnp.sparse_hypercolumn_cpu / fmpnp_hypercolumn_sparse_cpu): the rows equal
the DENSE twin's map indexed by a numpy restatement of the three index rules, bit for bit with NaNs in place
(tests/hypercolumn_sparse_cases.py).  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import fmpnp
from fmpnp import _lib
from fmpnp.hypercolumn import _layers
from fmpnp.match import generate_dense_keypoints, nearest_cells

import hypercolumn_cases as hc
import hypercolumn_sparse_cases as sc


def run(name, pts, mode, item=None, **kw):
    maps, _ = sc.inputs(name)
    return fmpnp.sparse_hypercolumn_cpu(maps, pts, item=item, **{**sc.kwargs(name, mode), **kw})


@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("name", sc.ALL)
def test_every_texel_equals_the_dense_twin(name, normalize):
    """at="texel" over every texel of every item (in mixed order): sparse == dense, exhaustively.  "views" has
    strided sources, "batch3" / "views" several items, "big" more channels than fit on chip, "zero_texel" an
    all-NaN row at texel (0, 0) and nowhere else; normalize=False gives the raw resized values."""
    tex, item = sc.all_texels(name)
    got = run(name, tex, "texel", item=item, normalize=normalize)
    want, ok = sc.expected(name, item, tex[:, 0], tex[:, 1], np.ones(len(tex), bool), normalize)
    assert ok.all() and got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape)
    assert hc.same_floats(got, want)
    if name == "zero_texel" and normalize:
        nan_rows = torch.isnan(got).all(1).numpy()
        assert np.array_equal(nan_rows, (tex[:, 0] == 0) & (tex[:, 1] == 0)) and nan_rows.sum() == 1
        assert not torch.isnan(got[~torch.from_numpy(nan_rows)]).any()


@pytest.mark.parametrize("mode", ["reference", "cell"])
@pytest.mark.parametrize("name", sc.ALL)
def test_fp64_points_equal_the_dense_twin(name, mode):
    """Corners, a duplicate, an exact edge, a negative coordinate, just inside the last texel and seeded points,
    with item covering every item in mixed order; fp64 output is the fp32 output widened."""
    pts, item = sc.good_points(name, mode)
    row, col, ok = sc.index(name, mode, pts)
    assert ok.all()
    _, _, H, W = sc.shape(name)
    assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)} <= set(zip(row.tolist(), col.tolist()))
    got = run(name, pts, mode, item=item)
    want, _ = sc.expected(name, item, row, col, ok)
    assert hc.same_floats(got, want)
    got64 = run(name, pts, mode, item=item, dtype=torch.float64)
    assert got64.dtype == torch.float64 and hc.same_floats(got64, got.double())
    if sc.shape(name)[0] == 1:  # item=None is item 0
        assert hc.same_floats(run(name, pts, mode), want)


def test_the_specials_land_where_the_rules_say():
    """The restated rules on the special points of a non-square case: wrap, lower cell on an edge, last texel."""
    _, _, H, W = sc.shape("ragged3")  # 9 x 7
    pts, _ = sc.good_points("ragged3", "reference")
    row, col, _ = sc.index("ragged3", "reference", pts)
    assert (row[5], col[5]) == (1, 2) and col[6] == W - 1 and (row[7], col[7]) == (H - 1, W - 1)
    pts, _ = sc.good_points("ragged3", "cell")
    row, col, _ = sc.index("ragged3", "cell", pts)
    assert (row[5], col[5]) == (0, 1) and col[6] == 0 and (row[7], col[7]) == (H - 1, W - 1)


@pytest.mark.parametrize("name", ["ragged3", "batch3", "views"])
def test_error_rows_are_zero_and_the_others_right(name):
    """Out-of-map, NaN and huge points, an out-of-range texel and out-of-range items: IndexError, zero rows,
    every other row right; through the C entry the flag and FMPNP_ERANGE."""
    B, C, H, W = sc.shape(name)
    good, item = sc.good_points(name, "reference")
    pts = np.concatenate([sc.bad_points(name), good])
    item = np.concatenate([np.zeros(len(sc.bad_points(name)), np.int32), item])
    item[-1], item[-2] = B, -1
    row, col, ok = sc.index(name, "reference", pts)
    want, ok = sc.expected(name, item, row, col, ok)
    assert (~ok).sum() == len(sc.bad_points(name)) + 2
    out = torch.full((len(pts), C), -7.0)
    with pytest.raises(IndexError):
        run(name, pts, "reference", item=item, out=out)
    assert hc.same_floats(out, want) and bool((out[torch.from_numpy(~ok)] == 0).all())
    # texels
    tex = np.array([(0, 0), (H, 0), (0, W), (-1, 0), (0, -1), (H - 1, W - 1)], np.int32)
    row, col, ok = sc.index(name, "texel", tex)
    assert ok.tolist() == [True, False, False, False, False, True]
    want, _ = sc.expected(name, None, row, col, ok)
    out = torch.full((len(tex), C), -7.0)
    with pytest.raises(IndexError):
        run(name, tex, "texel", out=out)
    assert hc.same_floats(out, want)
    # the C entry: the flag is ORed, the return is FMPNP_ERANGE
    maps, size = sc.inputs(name)
    layers, keep = _layers(maps, "cpu")
    t = torch.from_numpy(tex)
    out = torch.full((len(tex), C), -7.0)
    flag = ctypes.c_int(4)
    rc = _lib.load().fmpnp_hypercolumn_sparse_cpu(layers, len(keep), B, H, W, t.data_ptr(), None, len(tex),
                                                  _lib.HC_AT_TEXEL, 0.0, 0.0, out.data_ptr(), _lib.F32, C,
                                                  _lib.HC_NORMALIZE, ctypes.addressof(flag), 1)
    assert rc == _lib.ERANGE and flag.value == 5 and hc.same_floats(out, want)


def test_cell_mode_never_errors_and_nan_is_cell_zero():
    name = "ragged3"
    _, C, H, W = sc.shape(name)
    pts = np.array([(np.nan, np.nan), (1e300, -1e300), (-5.0, 1e9), (np.inf, -np.inf)], np.float64)
    row, col, ok = sc.index(name, "cell", pts)
    assert (row[0], col[0]) == (0, 0) and (row[1], col[1]) == (0, W - 1) and (row[2], col[2]) == (H - 1, 0)
    got = run(name, pts, "cell")
    assert hc.same_floats(got, sc.expected(name, None, row, col, ok)[0])


@pytest.mark.parametrize("mode", ["texel", "cell"])
def test_untouched_bytes(mode):
    """out= a view with ld_out = C + 3 inside a larger prefilled buffer: the padding and everything outside the
    view keep the fill; N = 0 writes nothing."""
    name = "blocks"
    _, C, _, _ = sc.shape(name)
    pts = sc.all_texels(name)[0] if mode == "texel" else sc.good_points(name, "cell")[0]
    n = len(pts)
    buf = torch.full((2 + n * (C + 3) + 5,), -7.0)
    view = buf[2:2 + n * (C + 3)].view(n, C + 3)[:, :C]
    got = run(name, pts, mode, out=view)
    assert got.data_ptr() == view.data_ptr()
    row, col, ok = sc.index(name, mode, pts)
    assert hc.same_floats(view, sc.expected(name, None, row, col, ok)[0])
    view.fill_(-7.0)
    assert bool((buf == -7.0).all())
    empty = run(name, np.zeros((0, 2), np.int32 if mode == "texel" else np.float64), mode)
    assert tuple(empty.shape) == (0, C)
    layers, keep = _layers(sc.inputs(name)[0], "cpu")
    rc = _lib.load().fmpnp_hypercolumn_sparse_cpu(layers, len(keep), 1, 4, 5, None, None, 0, _lib.HC_AT_TEXEL, 0.0, 0.0,
                                                  None, _lib.F32, C, 1, None, 1)
    assert rc == 0


@pytest.mark.parametrize("name", ["vgg16x", "batch3"])
def test_rows_depend_on_their_own_point_only(name):
    """A permutation of the points permutes the rows; subsets of 1, 63, 64, 65 and 257 points (with repeats)
    give the same rows; thread counts change nothing."""
    tex, item = sc.all_texels(name)
    rng = np.random.Generator(np.random.PCG64(11))
    pick = rng.integers(0, len(tex), 257)
    tex, item = tex[pick], item[pick]
    base = run(name, tex, "texel", item=item, n_threads=1)
    perm = rng.permutation(257)
    assert hc.same_floats(run(name, tex[perm], "texel", item=item[perm], n_threads=3), base[perm])
    for n in sc.SUBSETS:
        assert hc.same_floats(run(name, tex[:n], "texel", item=item[:n]), base[:n])


def test_argument_errors():
    maps, _ = sc.inputs("ragged3")
    layers, keep = _layers(maps, "cpu")
    L = _lib.load()
    C, H, W = 12, 9, 7
    tex = torch.zeros(1, 2, dtype=torch.int32)
    out = torch.zeros(1, C + 1)

    def call(layers=layers, n_layers=3, B=1, H=H, W=W, points=tex.data_ptr(), N=1, at=_lib.HC_AT_TEXEL, p0=0.0,
             p1=0.0, out=out.data_ptr(), dtype=_lib.F32, ld=C, flags=1, threads=1):
        return L.fmpnp_hypercolumn_sparse_cpu(layers, n_layers, B, H, W, points, None, N, at, p0, p1, out, dtype, ld,
                                              flags, None, threads)
    assert call() == 0
    for bad in (dict(ld=C - 1), dict(at=3), dict(at=-1), dict(dtype=2), dict(flags=2), dict(flags=5), dict(N=-1),
                dict(points=None), dict(out=None), dict(n_layers=0), dict(n_layers=9), dict(B=0), dict(H=0), dict(W=0),
                dict(threads=-1), dict(at=_lib.HC_AT_REFERENCE, p0=0.0, p1=1.0), dict(at=_lib.HC_AT_CELL, p0=1.0, p1=-1.0),
                dict(at=_lib.HC_AT_CELL, p0=float("nan"), p1=1.0)):
        assert call(**bad) == _lib.EINVAL, bad
    for big in (dict(H=(1 << 24) + 1), dict(W=(1 << 24) + 1), dict(B=(1 << 24) + 1)):
        assert call(**big) == _lib.ETOOBIG, big
    broken = (_lib.HcLayer * 3)(*layers)
    broken[1].stride_y = broken[1].W - 1
    assert call(layers=broken) == _lib.EINVAL
    broken = (_lib.HcLayer * 3)(*layers)
    broken[2].C = 1 << 24  # the channel total passes 2^24
    assert call(layers=broken) == _lib.ETOOBIG
    # the GPU entry points validate before any device call: no GPU needed
    for fn in (L.fmpnp_hypercolumn_sparse_async, L.fmpnp_hypercolumn_sparse):
        rc = fn(layers, 3, 1, H, W, tex.data_ptr(), None, 1, 7, 0.0, 0.0, out.data_ptr(), 0, C, 1, None, None)  # at = 7
        assert rc == _lib.EINVAL
        assert fn(layers, 3, 1, H, W, None, None, 0, 0, 0.0, 0.0, None, 0, C, 1, None, None) == 0  # N == 0
    # the Python surface
    with pytest.raises(ValueError):
        fmpnp.sparse_hypercolumn_cpu(maps, tex, at="pixel")
    with pytest.raises(ValueError):
        fmpnp.sparse_hypercolumn_cpu(maps, np.zeros((1, 2)), at="reference")  # no image_shape
    with pytest.raises(ValueError):
        fmpnp.sparse_hypercolumn_cpu(maps, np.zeros((1, 2)), at="cell")  # no cell_size
    with pytest.raises(ValueError):
        fmpnp.sparse_hypercolumn_cpu(maps, tex, at="texel", dtype=torch.float16)
    with pytest.raises(ValueError):
        fmpnp.sparse_hypercolumn_cpu(maps, tex, at="texel", item=[0, 0])
    with pytest.raises(ValueError):
        fmpnp.sparse_hypercolumn_cpu(maps, tex, at="texel", out=torch.zeros(1, C + 1))


@pytest.mark.parametrize("name", ["ragged3", "sized", "wide"])
def test_agrees_with_the_existing_cpu_form_of_the_cell_gather(name):
    """fmpnp.match.nearest_cells is the CPU form of fast_sparse_keypoint_descriptor's gather (localize_cpu uses
    it on the host map): the rows equal the dense twin at those cells, with cell_size as generate_dense_keypoints
    returns it.  (gather_reference has no CPU form; the GPU tests pin that equality.)"""
    _, C, H, W = sc.shape(name)
    _, cell = generate_dense_keypoints((H, W), sc.cell_resolution(name))
    assert tuple(cell) == sc.CELL
    pts, _ = sc.good_points(name, "cell")
    cells = nearest_cells(pts, H, W, cell[0], cell[1])
    want = sc.dense(name)[0].reshape(C, -1)[:, torch.from_numpy(cells)].T
    assert hc.same_floats(run(name, pts, "cell", cell_size=cell), want)


def test_compute_feature_maps_is_the_first_half_of_compute_hypercolumn():
    net, image = hc.tiny_encoder(), hc.tiny_image()
    ex = fmpnp.HypercolumnExtractor(net, hc.ENCODER_LAYERS, device="cpu")
    maps, resolution = ex.compute_feature_maps(image)
    hyper, resolution2 = ex.compute_hypercolumn(image)
    assert tuple(resolution) == tuple(resolution2) == (20, 28)
    assert all(torch.equal(a, b) for a, b in zip(maps, hc.restated_walk(net, image)))
    assert hc.same_floats(fmpnp.assemble_hypercolumn_cpu(maps), hyper)
    # ... and compute_sparse_hypercolumn is its descriptors at points
    tex = np.array([(0, 0), (19, 27), (7, 13)], np.int32)
    rows, resolution3 = ex.compute_sparse_hypercolumn(image, tex, at="texel")
    assert tuple(resolution3) == (20, 28)
    assert hc.same_floats(rows, hyper[0][:, tex[:, 0], tex[:, 1]].T)
