"""Layered matching without a GPU: the CPU twin (fmpnp_exhaustive_match_layers_cpu) against the fp64 restatement
within the derived bound of include/fmpnp.h, against the row reduction's contract, against the dense twins bit for
bit where every intermediate is exact, against the dense twins' decisions where the inputs separate the first two
candidates by more than twice the bound, and the independence, non-finite and argument rules."""
import ctypes

import numpy as np
import pytest
import torch

import fmpnp
from fmpnp import _lib, hypercolumn

import hypercolumn_cases as hcc
import match_cases as mc
import match_layers_cases as mlc


def _within(case, got, d, normalize):
    """(largest error / bound over the scores where all three are finite and the bound is positive, everything
    within the bound)"""
    ref, b = mlc.ref_scores(case, d, normalize), mlc.bound(case, d, normalize)
    got = np.asarray(got, np.float64)
    ok = np.isfinite(got) & np.isfinite(ref) & np.isfinite(b)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref)
    pos = ok & (b > 0)
    ratio = float((err[pos] / b[pos]).max()) if pos.any() else 0.0
    return ratio, bool((err[ok] <= b[ok]).all()), int(ok.sum())


@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "plain"])
@pytest.mark.parametrize("case", mlc.ALL)
def test_twin_is_within_the_bound_of_the_fp64_restatement(case, normalize):
    """ref(maps, float64), then a matmul; the bound is include/fmpnp.h's expression evaluated in fp64.  The
    non-finite scores fall where the restatement's do."""
    tw = mlc.twin(case, mlc.case_top_ks(case)[0], normalize)
    ratio, inside, compared = _within(case, tw["scores"], mlc.sparse(case), normalize)
    print(case, normalize, "largest error / bound:", ratio, "scores compared:", compared)
    assert inside
    ref = mlc.ref_scores(case, mlc.sparse(case), normalize)
    assert np.array_equal(np.isfinite(tw["scores"]), np.isfinite(ref))
    if case != "nonfinite":
        assert compared == np.isfinite(ref).sum() > 0


@pytest.mark.parametrize("case", mlc.ALL)
def test_row_reduction_is_the_contract_on_the_twins_own_scores(case):
    scores = mlc.twin(case, mlc.case_top_ks(case)[0])["scores"]
    for top_k in mlc.case_top_ks(case):
        argmax, top, kth, mask = mc.reduce_rows(scores, top_k)
        mc.assert_same_result(mlc.twin(case, top_k), dict(argmax=argmax, top=top, kth=kth, mask=mask), (case, top_k))


EXACT_SETS = {
    "equal": [(4, 5, 3), (3, 5, 3)],                 # equal sizes: every weight 1 or 0
    "dyadic": [(4, 5, 3), (3, 5, 3), (5, 3, 2)],     # 3 -> 5 and 2 -> 3: weights 0, 1/2, 1
    "blocks": [(33, 5, 3), (40, 3, 2)],              # ragged k, channel offsets beyond one k step
}


@pytest.mark.parametrize("name", EXACT_SETS)
def test_exact_operands_equal_the_dense_twins_bit_for_bit(name):
    """Small integers, normalize=False: every product, chain, weight and sum is exact in fp32, so the layered
    scores equal exhaustive_match_cpu on assemble_hypercolumn_cpu's map under ==.  Pins the channel offsets, the
    layer order and the flat index."""
    maps = mlc.int_layers(EXACT_SETS[name], seed=len(name) + 5, batch=2)
    c = mlc.channels(maps)
    rng = np.random.default_rng(len(name))
    d = rng.integers(-2, 3, (37, c)).astype(np.float32)
    for item in (0, 1):
        dense = fmpnp.assemble_hypercolumn_cpu(maps, normalize=False)[item].reshape(c, -1).numpy()
        assert len(np.unique(dense)) > 3  # (a real map, with the resize's halves and quarters where it has them)
        for i, top_k in enumerate(mc.top_ks(dense.shape[1])):
            want = fmpnp.exhaustive_match_cpu(d, dense, top_k, mc.RATIO, scores=(i == 0))
            got = fmpnp.exhaustive_match_layers_cpu(d, maps, top_k, mc.RATIO, item=item, normalize=False, scores=(i == 0))
            mc.assert_same_result(got, want, (name, item, top_k))
            if i == 0:
                assert (got["scores"] == want["scores"]).all() and np.abs(want["scores"]).max() > 0


AGREEMENT_SEEDS = {"wide": 4}  # (the seed at which every row of the case meets the gap condition; default 1)


@pytest.mark.parametrize("case", mlc.FINITE)
def test_decisions_agree_with_the_dense_twins_where_the_inputs_separate(case):
    """Each descriptor is a texel of the query's own hypercolumn plus seeded noise.  The condition on the INPUTS,
    asserted here for every row: the fp64 top-two gap exceeds twice the bound -- both paths lie within the bound of
    the fp64 value, so neither can prefer the runner-up.  Then argmax and mask equal the dense twin's."""
    maps, size, item, n = mlc.layers(case)
    d = mlc.own_texel_descriptors(case, AGREEMENT_SEEDS.get(case, 1))
    ref, b = mlc.ref_scores(case, d), mlc.bound(case, d)
    assert np.isfinite(ref).all() and np.isfinite(b).all()
    if ref.shape[1] > 1:
        srt = np.sort(ref, axis=1)
        assert (srt[:, -1] - srt[:, -2] > 2.0 * b.max(axis=1)).all()
    dense = fmpnp.assemble_hypercolumn_cpu(maps, size=size)[item]
    dense = dense.reshape(dense.shape[0], -1).numpy()
    top_k = mc.top_ks(dense.shape[1])[-2] if len(mc.top_ks(dense.shape[1])) > 1 else 1
    want = fmpnp.exhaustive_match_cpu(d, dense, top_k, mc.RATIO, scores=True)
    got = fmpnp.exhaustive_match_layers_cpu(d, maps, top_k, mc.RATIO, size=size, item=item, scores=True)
    assert np.array_equal(got["argmax"], np.argmax(ref, axis=1)) and np.array_equal(got["argmax"], want["argmax"])
    # the dense twin's scores are inside the same bound
    assert (np.abs(want["scores"].astype(np.float64) - ref) <= b).all()
    # the mask compares ratio^2 * d1 with d_k: equal decisions unless a row sits within the bound of that edge
    r2 = float(np.float32(mc.RATIO * mc.RATIO))
    kth = -np.sort(-ref, axis=1)[:, top_k - 1]
    clear = np.abs(r2 * ref.max(axis=1) - kth) > 3.0 * b.max(axis=1)
    assert clear.all(), "an input row sits on the ratio test's edge: choose another seed"
    assert np.array_equal(got["mask"], want["mask"])


def test_rows_do_not_depend_on_their_company_or_the_threads():
    """Permuted rows, subsets of 1 / 63 / 65 rows and the thread count change no row."""
    case = "tiles2"
    maps, size, item, n = mlc.layers(case)
    d, top_k = mlc.sparse(case), mlc.case_top_ks(case)[2]
    want = fmpnp.exhaustive_match_layers_cpu(d, maps, top_k, scores=True, n_threads=1)
    mc.assert_same_result(want, mlc.twin(case, top_k))
    assert want["scores"].tobytes() == mlc.twin(case, mlc.case_top_ks(case)[0])["scores"].tobytes()
    perm = np.random.default_rng(5).permutation(n)
    for rows, threads in ((perm, 3), (np.arange(1) + 17, 2), (perm[:63], 0), (perm[:65], 5)):
        got = fmpnp.exhaustive_match_layers_cpu(d[rows], maps, top_k, scores=True, n_threads=threads)
        mc.assert_same_result(got, {k: want[k][rows] for k in ("argmax", "top", "kth", "mask")}, len(rows))
        assert got["scores"].tobytes() == want["scores"][rows].tobytes()


def test_a_zero_texel_scores_nan_in_every_row():
    scores = mlc.twin("zero_texel", mlc.case_top_ks("zero_texel")[0])["scores"]
    assert np.isnan(scores[:, 0]).all() and np.isfinite(scores[:, 1:]).all()
    plain = mlc.twin("zero_texel", mlc.case_top_ks("zero_texel")[0], False)["scores"]
    assert (plain[:, 0] == 0).all() and np.isfinite(plain).all()
    tw = mlc.twin("zero_texel", 2)
    assert (tw["argmax"] == 0).all() and np.isnan(tw["top"]).all()  # (NaN above everything, as the dense path)


def test_views_through_the_wrapper_equal_their_contiguous_copies():
    maps, size, item, _ = mlc.layers("views")
    assert not any(m.is_contiguous() for m in maps)
    d = mc.padded(mlc.sparse("views"), 3)
    top_k = mlc.case_top_ks("views")[0]
    got = fmpnp.exhaustive_match_layers_cpu(d, maps, top_k, item=item, scores=True)
    same = fmpnp.exhaustive_match_layers_cpu(np.ascontiguousarray(d), [m.contiguous() for m in maps], top_k, item=item,
                                             scores=True)
    mc.assert_same_result(got, same)
    assert got["scores"].tobytes() == same["scores"].tobytes() == mlc.twin("views", top_k)["scores"].tobytes()
    # a channel stride longer than the plane is read in place; anything else is copied by the wrapper
    wide = torch.randn(2, 4, 5 * 6 + 7)[:, :, :30].view(2, 4, 5, 6)
    desc, keep = hypercolumn._plane_layers([wide], "cpu")
    assert keep[0].data_ptr() == wide.data_ptr() and desc[0].stride_c == 37 and desc[0].stride_y == 6
    desc, keep = hypercolumn._plane_layers([maps[0]], "cpu")
    assert keep[0].data_ptr() != maps[0].data_ptr() and desc[0].stride_y == maps[0].shape[3]


def _call_cpu(d, maps, top_k=1, item=0, size=None, flags=1, scores=None, edit=None, ld=None, ratio=mc.RATIO, threads=1,
              null=()):
    """The C entry point on host arrays with one argument bent: edit(desc) changes the layer descriptors; null:
    names of pointers passed as NULL."""
    desc, keep = hypercolumn._plane_layers(maps, "cpu")
    n, c = d.shape
    h, w = mlc.out_size(keep, size)
    L, B = len(keep), int(keep[0].shape[0])
    if edit:
        L, B, h, w = edit(desc, L, B, h, w)
    out = dict(argmax=np.zeros(max(n, 1), np.int32), top=np.zeros(max(n, 1), np.float32),
               kth=np.zeros(max(n, 1), np.float32), mask=np.zeros(max(n, 1), np.uint8))
    ptr = {k: (None if k in null else v.ctypes.data) for k, v in out.items()}
    rc = _lib.load().fmpnp_exhaustive_match_layers_cpu(
        None if "sparse" in null else d.ctypes.data, n, c if ld is None else ld, None if "layers" in null else desc, L, B,
        item, h, w, flags, top_k, ratio, ptr["argmax"], ptr["top"], ptr["kth"], ptr["mask"],
        None if scores is None else scores.ctypes.data, threads)
    return rc, out


def test_argument_errors():
    maps, size, item, _ = mlc.layers("ragged3")
    d = np.ascontiguousarray(mlc.sparse("ragged3")[:5])
    wh = 63
    assert _call_cpu(d, maps)[0] == 0
    E, BIG = _lib.EINVAL, _lib.ETOOBIG

    def bend(**kw):
        def edit(desc, L, B, h, w):
            for k, v in kw.items():
                if k in ("L", "B", "h", "w"):
                    continue
                setattr(desc[int(k[-1])], k[:-1], v)
            return kw.get("L", L), kw.get("B", B), kw.get("h", h), kw.get("w", w)
        return edit
    bad = [dict(edit=bend(L=0)), dict(edit=bend(L=9)), dict(edit=bend(B=0)), dict(edit=bend(h=0)), dict(edit=bend(w=0)),
           dict(edit=bend(C1=0)), dict(edit=bend(H1=0)), dict(edit=bend(W2=0)), dict(edit=bend(data0=None)),
           dict(edit=bend(stride_y0=8)), dict(edit=bend(stride_y1=3)), dict(edit=bend(stride_c1=19)),
           dict(edit=bend(stride_b0=-1)), dict(ld=11), dict(top_k=0), dict(top_k=wh + 1), dict(flags=2), dict(flags=5),
           dict(item=-1), dict(item=1), dict(ratio=float("nan")), dict(threads=-1), dict(null=("sparse",)),
           dict(null=("layers",)), dict(null=("argmax",)), dict(null=("top",)), dict(null=("kth",)),
           dict(null=("mask",))]
    for kw in bad:
        assert _call_cpu(d, maps, **kw)[0] == E, kw
    assert _call_cpu(d, maps, edit=bend(h=(1 << 24) + 1))[0] == BIG
    assert _call_cpu(d, maps, edit=bend(H1=(1 << 24) + 1))[0] == BIG
    # N < 0 is an error, N == 0 is not and touches nothing
    rc = _lib.load().fmpnp_exhaustive_match_layers_cpu(None, -1, 12, hypercolumn._plane_layers(maps, "cpu")[0], 3, 1, 0, 9, 7,
                                                       1, 1, 0.9, None, None, None, None, None, 1)
    assert rc == E
    rc = _lib.load().fmpnp_exhaustive_match_layers_cpu(None, 0, 12, hypercolumn._plane_layers(maps, "cpu")[0], 3, 1, 0, 9, 7,
                                                       1, 1, 0.9, None, None, None, None, None, 1)
    assert rc == 0
    # the wrapper's own checks
    with pytest.raises(ValueError):
        fmpnp.exhaustive_match_layers_cpu(d[:, :11], maps, 1)
    with pytest.raises(ValueError):
        fmpnp.exhaustive_match_layers_cpu(d, maps, 1, item=1)
    with pytest.raises(ValueError):
        fmpnp.exhaustive_match_layers_cpu(d, [m.double() for m in maps], 1)
    with pytest.raises(_lib.FmpnpError):
        fmpnp.exhaustive_match_layers_cpu(d, maps, wh + 1)
    names = {"fmpnp_match_layers_workspace_size", "fmpnp_exhaustive_match_layers_async", "fmpnp_correlation_layers_async",
             "fmpnp_exhaustive_match_layers", "fmpnp_exhaustive_match_layers_cpu", "fmpnp_localize_layers"}
    L = _lib.load()
    assert names <= set(_lib.EXPORTS) and all(hasattr(L, name) for name in names)


def test_padded_operands_and_a_scores_map_inside_a_larger_buffer():
    """Padded descriptor rows read only their C columns; a scores map in the middle of a larger buffer is written
    and its surroundings are not."""
    maps, size, item, n = mlc.layers("sized")
    d = mlc.sparse("sized")
    h, w = mlc.out_size(maps, size)
    top_k = mlc.case_top_ks("sized")[0]
    want = mlc.twin("sized", top_k)
    buf = np.full(5 + n * h * w + 7, -7.0, np.float32)
    padded = mc.padded(d, 5)
    rc, out = _call_cpu(padded, maps, top_k=top_k, size=size, scores=buf[5:], ld=padded.strides[0] // 4, threads=2)
    assert rc == 0
    out["mask"] = out["mask"].astype(bool)
    mc.assert_same_result(out, want)
    assert buf[5:5 + n * h * w].tobytes() == want["scores"].tobytes()
    assert (buf[:5] == -7.0).all() and (buf[5 + n * h * w:] == -7.0).all()
    # the workspace size: the norm plane and one round of coarse maps and score rows; 0 for an invalid shape
    desc, keep = hypercolumn._plane_layers(maps, "cpu")
    size_of = _lib.load().fmpnp_match_layers_workspace_size
    coarse = sum(m.shape[2] * m.shape[3] for m in maps)
    up = lambda x: (x + 255) // 256 * 256  # noqa: E731
    assert size_of(desc, len(keep), 5, h, w) == up(4 * h * w) + 5 * 4 * (coarse + h * w)
    assert size_of(desc, len(keep), 2, h, w) == up(4 * h * w) + 2 * 4 * (coarse + h * w)
    assert size_of(desc, len(keep), 0, h, w) == size_of(desc, 0, 5, h, w) == size_of(desc, len(keep), 5, 0, w) == 0
    assert size_of(None, len(keep), 5, h, w) == 0
    assert isinstance(ctypes.sizeof(_lib.LocQueryLayers), int)
