"""Dense exhaustive matching on the GPU: the MFMA correlation and the row reduction against the CPU
twin (bit for bit), fmpnp.exhaustive_search against the reference's goldens, exhaustive_search_multi
against the separate calls, the gather kernel against the reference's argmins, and the synchronous
entry point on two streams."""
import threading

import numpy as np
import pytest
import torch

import fmpnp
from fmpnp import match

import match_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the shared operands are read-only)


def dev_padded(a, pad):
    """A CUDA view of a with `pad` unused columns after every row (NaN-filled: never read)."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = torch.from_numpy(np.array(a))  # (a copy: the shared operands are read-only)
    return buf[:, :a.shape[1]]


# (the integer operands are about the reduction; the long k chain runs with the Gaussians)
@pytest.mark.parametrize("shape,kind", [(s, "normal") for s in mc.SHAPES] + [(s, "ints") for s in mc.SHAPES[:3]],
                         ids=str)
def test_gpu_equals_the_twin(shape, kind):
    """Scores equal under == with NaNs at the same positions; argmax, d1, d_k and mask equal on every
    row, at top_k = 1, 2, int(0.006 WH), int(0.12 WH), WH.  "normal" has a row of one repeated value;
    "ints" has heavily duplicated scores, negative values and +-0."""
    n, c, w, h = shape
    sparse, dense = mc.operands(n, c, w, h, kind)
    ds, dd = dev(sparse), dev(dense)
    for i, top_k in enumerate(mc.top_ks(w * h)):
        want = mc.twin(n, c, w, h, top_k, kind)
        got = fmpnp.exhaustive_match(ds, dd, top_k, mc.RATIO, scores=(i == 0))
        mc.assert_same_result(got, want, (shape, kind, top_k))
        if i == 0:
            assert mc.same_floats(got["scores"].cpu().numpy(), want["scores"]), (shape, kind)


@pytest.mark.parametrize("shape", mc.SHAPES[1:3], ids=str)
def test_gpu_padded_rows(shape):
    """ld_sparse > C and ld_dense > W * H (odd paddings: no alignment to lean on)."""
    n, c, w, h = shape
    sparse, dense = mc.operands(n, c, w, h)
    top_k = mc.top_ks(w * h)[0]
    want = mc.twin(n, c, w, h, top_k)
    ds, dd = dev_padded(sparse, 3), dev_padded(dense, 5)
    assert ds.stride(0) == c + 3 and dd.stride(0) == w * h + 5
    got = fmpnp.exhaustive_match(ds, dd, top_k, mc.RATIO, scores=True)
    mc.assert_same_result(got, want, shape)
    assert mc.same_floats(got["scores"].cpu().numpy(), want["scores"])


def test_gpu_non_finite_scores_equal_the_twin():
    """NaNs (two columns: the lowest wins), +Inf and -Inf in the map, at top_k below, at and above the
    number of NaNs per row."""
    sparse, dense = (a.copy() for a in mc.operands(37, 40, 24, 20))
    dense[3, 100], dense[4, 17], dense[5, 300], dense[6, 301] = np.nan, np.nan, np.inf, -np.inf
    ds, dd = dev(sparse), dev(dense)
    for i, top_k in enumerate((1, 2, 3, 57, 480)):
        want = fmpnp.exhaustive_match_cpu(sparse, dense, top_k, scores=(i == 0))
        got = fmpnp.exhaustive_match(ds, dd, top_k, scores=(i == 0))
        mc.assert_same_result(got, want, top_k)
        if i == 0:
            assert mc.same_floats(got["scores"].cpu().numpy(), want["scores"])
    assert np.all(got["argmax"][1:] == 17)


def test_gpu_rows_in_more_than_one_round():
    """A map so large that the score workspace holds 64 rows: 65 rows run in two rounds."""
    n, c, wh = 65, 2, 1 << 20
    assert fmpnp._lib.load().fmpnp_match_workspace_size(n, wh) == 64 * wh * 4
    rng = np.random.default_rng(7)
    sparse = rng.standard_normal((n, c)).astype(np.float32)
    dense = rng.standard_normal((c, wh)).astype(np.float32)
    top_k = int(0.006 * wh)
    want = fmpnp.exhaustive_match_cpu(sparse, dense, top_k)
    got = fmpnp.exhaustive_match(dev(sparse), dev(dense), top_k)
    mc.assert_same_result(got, want)


def test_exhaustive_search_matches_the_reference_goldens():
    g = mc.golden("main")
    dense, sparse = dev(g["dense"]), dev(g["sparse"])
    for f in g["factors"]:
        pts, mask = fmpnp.exhaustive_search(dense, sparse, list(g["image_shape"]), list(g["map_size"]), [8, 8], float(f))
        assert isinstance(pts, torch.Tensor) and pts.dtype == torch.float32 and not pts.is_cuda
        assert isinstance(mask, np.ndarray) and mask.dtype == bool
        assert np.array_equal(pts.numpy(), g[f"points_{f}"]), f
        assert np.array_equal(mask, g[f"mask_{f}"]), f


@pytest.mark.parametrize("name", mc.EDGE_CASES)
def test_exhaustive_search_matches_the_reference_edge_cases(name):
    g = mc.golden("edge_" + name)
    try:
        fmpnp.config.configure(exhaustive_search_factor=float(g["factor"]))  # factor=None reads the binding
        pts, mask = fmpnp.exhaustive_search(dev(g["dense"]), dev(g["sparse"]), list(g["image_shape"]),
                                            list(g["map_size"]), [8, 8])
    finally:
        fmpnp.config.configure(exhaustive_search_factor=None)
    assert np.array_equal(pts.numpy(), g["points"])
    assert np.array_equal(mask, g["mask"])


def test_exhaustive_search_multi_equals_the_separate_calls():
    """Several references of one query in one launch: bit-identical to one call each (the rows are
    independent and the result does not depend on the grid).  Row counts that put every reference at
    another offset inside the 128-row tiles."""
    n, c, w, h = 129, 33, 33, 40
    sparse, dense = mc.operands(n, c, w, h)
    dd = dev(dense)
    parts = [sparse[:50], sparse[50:51], sparse[51:]]
    args = ([330, 400], [w, h], [10, 10], 0.12)
    multi = fmpnp.exhaustive_search_multi(dd, [dev(p) for p in parts], *args)
    assert len(multi) == 3
    for p, (pts, mask) in zip(parts, multi):
        pts1, mask1 = fmpnp.exhaustive_search(dd, dev(p), *args)
        assert pts.shape == (p.shape[0], 2) and torch.equal(pts, pts1) and np.array_equal(mask, mask1)


def test_gather_kernel_matches_the_reference_argmins():
    g = mc.golden("assoc")
    rng = np.random.default_rng(3)
    for tag in ("exact", "ragged"):
        d1, d2 = (int(v) for v in g[f"{tag}_fmap"])
        cells = g[f"{tag}_cells"]
        chw = rng.standard_normal((67, d1, d2)).astype(np.float32)  # (more channels than one wave's lanes)
        pts = g[f"{tag}_points"]
        out = fmpnp.gather_sparse_descriptors(dev(chw), pts, float(cells[0]), float(cells[1]))
        want = chw.reshape(67, -1)[:, g[f"{tag}_argmin"]].T
        assert np.array_equal(out.cpu().numpy(), want), tag
        # a padded output: the columns beyond C stay untouched
        buf = torch.full((pts.shape[0], 70), -7.0, dtype=torch.float32, device=DEV)
        fmpnp.gather_sparse_descriptors(dev(chw), pts, float(cells[0]), float(cells[1]), out=buf[:, :67])
        assert np.array_equal(buf[:, :67].cpu().numpy(), want) and bool((buf[:, 67:] == -7.0).all())


def test_fast_sparse_keypoint_descriptor_is_a_drop_in():
    g = mc.golden("assoc")
    grid, _ = match.generate_dense_keypoints([24, 20], [192, 120])
    out = fmpnp.fast_sparse_keypoint_descriptor([g["fsk_kp0"], g["fsk_kp1"]], torch.from_numpy(grid),
                                                torch.from_numpy(g["fsk_desc"]))
    assert len(out) == 2
    assert np.array_equal(out[0].cpu().numpy(), g["fsk_out0"]) and np.array_equal(out[1].cpu().numpy(), g["fsk_out1"])


def test_synchronous_entry_point_on_two_streams():
    """Two host threads, each on its own stream, against the serial results: the scratch is per (device,
    stream), so concurrent calls do not share buffers.  (No timing is asserted.)"""
    shapes = [mc.SHAPES[1], mc.SHAPES[2]]
    top_k = {s: mc.top_ks(s[2] * s[3])[-2] for s in shapes}
    want = {s: mc.twin(*s, top_k[s]) for s in shapes}
    ops = {s: tuple(dev(a) for a in mc.operands(*s)) for s in shapes}
    torch.cuda.synchronize()
    results, errors = {}, []

    def run(s):
        try:
            stream = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(stream):
                results[s] = [fmpnp.exhaustive_match(*ops[s], top_k[s]) for _ in range(4)]
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=run, args=(s,)) for s in shapes]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for s in shapes:
        for got in results[s]:
            mc.assert_same_result(got, want[s], s)
