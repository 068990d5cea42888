"""The batched refinement stage of the localisation chain on the GPU (localize / localize_multi with
refine="batched", LocalizeLaunch with a refine spec): equal to the per-query path (refine=True) bit for bit, its
prep and gather kernels equal to the CPU twin, its compute_cost equal to fmpnp_compute_cost_async.
Scenes: tests/localize_cases.py; shared pieces: tests/localize_refine_cases.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import localize_cases as lc
import localize_refine_cases as rc
import fmpnp
from fmpnp import _lib, config
from fmpnp import _localize as loc
from fmpnp.model import sparseFeaturePnP
from fmpnp.refine import RESULT_DTYPE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = rc.FILL
STORAGE = {"f32": torch.float32, "f64": torch.float64}


@functools.lru_cache(maxsize=None)
def on_device(name):
    sc = lc.scene(name)
    refs = []
    for r in sc["references"]:
        r = lc.public(r)
        r["hypercolumn"] = torch.from_numpy(r["hypercolumn"]).to(DEV)
        refs.append(r)
    return torch.from_numpy(sc["query"]).to(DEV), refs


def queries_of(names=rc.NAMES):
    return [on_device(n) for n in names]


def kw_of(levels, storage, masked, **more):
    return dict(factor=lc.FACTOR, return_masked=masked, return_all=True, feature_pyramid=rc.LEVELS if levels else None,
                storage=STORAGE[storage], **lc.PNP, **more)


@functools.lru_cache(maxsize=None)
def per_query(levels, storage, masked):
    return fmpnp.localize_multi(queries_of(), lc.IMAGE, refine=True, **kw_of(levels, storage, masked))


@functools.lru_cache(maxsize=None)
def batched(levels, storage, masked):
    return fmpnp.localize_multi(queries_of(), lc.IMAGE, refine="batched", **kw_of(levels, storage, masked))


def equal_refined(a, b):
    if a is None or b is None:
        assert a is None and b is None
        return
    lc.equal(a[0], b[0], "t")
    lc.equal(a[1], b[1], "quaternion")
    for k in ("initial_cost_", "best_cost_", "best_num_inliers_"):
        x, y = getattr(a[2], k, None), getattr(b[2], k, None)
        assert (x is None) == (y is None), k
        if x is not None:
            lc.equal(x.cpu().numpy() if torch.is_tensor(x) else x, y.cpu().numpy() if torch.is_tensor(y) else y, k)


def equal_localization(a, b):
    lc.equal(a.export, b.export, "export")
    lc.equal_prediction(a.prediction, b.prediction, "best")
    assert a.kind == b.kind and a.best == b.best
    assert (a.predictions is None) == (b.predictions is None)
    for j, (x, y) in enumerate(zip(a.predictions or [], b.predictions or [])):
        lc.equal_prediction(x, y, f"pair {j}")
    equal_refined(a.refined, b.refined)


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("levels", [False, True])
def test_batched_equals_the_per_query_path(levels, storage, masked):
    want, got = per_query(levels, storage, masked), batched(levels, storage, masked)
    assert [g.kind for g in got] == ["solved", "solved", "solved", "fallback", "none"]
    for a, b in zip(got, want):
        equal_localization(a, b)
    assert got[4].refined is None and got[3].refined is not None
    assert len({g.prediction.points_3d.shape[0] for g in got[:4]}) == 4  # (with "none": five different N)
    for g in got[:4]:
        assert np.isfinite(np.asarray(g.refined[0])).all() and np.isfinite(np.asarray(g.refined[1])).all()


def test_the_counts_lie_below_the_capacities():
    """mixed's best pair has 1000 rows of capacity and about 600 inliers, tie's 357 and about 300: N is below the
    host descriptors' N (the capacity) and falls in another count of 64-point blocks."""
    got = batched(True, "f32", True)
    for qi, (cap, about) in ((0, (1000, 600)), (1, (357, 300))):
        refs = queries_of()[qi][1]
        n = got[qi].prediction.points_3d.shape[0]
        assert max(len(r["points_2D"]) for r in refs) == cap and len(refs[got[qi].best]["points_2D"]) == cap
        assert abs(n - about) < 60 and n < cap and (n + 63) // 64 != (cap + 63) // 64


def test_none_and_the_fallback_winner():
    got = batched(False, "f32", True)
    assert got[4].kind == "none" and got[4].refined is None and got[4].prediction is None
    fw = got[3]
    assert fw.kind == "fallback" and fw.prediction.inlier_mask is None and fw.refined is not None
    # refined FROM the fallback pose: the per-query call on that prediction, whose matrix is the fallback's
    refs = queries_of()[3][1]
    assert np.array_equal(np.asarray(fw.prediction.matrix), refs[fw.best]["fallback_pose"][1])
    equal_refined(fw.refined, per_query(False, "f32", True)[3].refined)


def test_refine_intrinsics_last_against_best():
    qmap, refs = on_device("fallback_loses")
    kw = dict(factor=lc.FACTOR, return_masked=True, **lc.PNP)
    out = {}
    for which in ("last", "best"):
        out[which] = fmpnp.localize(qmap, refs, lc.IMAGE, refine="batched", refine_intrinsics=which, **kw)
        equal_refined(out[which].refined, fmpnp.localize(qmap, refs, lc.IMAGE, refine_intrinsics=which, **kw).refined)
    assert np.asarray(out["best"].refined[0]).tobytes() != np.asarray(out["last"].refined[0]).tobytes()
    with pytest.raises(ValueError):
        fmpnp.localize(qmap, refs, lc.IMAGE, refine="batched", refine_intrinsics="first", **kw)


def launch(levels, storage="f32", model=None, stream=None):
    spec = loc._RefineSpec(lc.C, lc.IMAGE, rc.LEVELS if levels else None, model, STORAGE[storage], "last")
    params = loc._pnp_params(return_masked=True, **lc.PNP)
    la = loc.LocalizeLaunch(queries_of(), lc.IMAGE, lc.FACTOR, params, return_all=True, fill=FILL, refine=spec)
    return la, la.read()


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("levels", [False, True])
def test_prep_and_gather_kernels_equal_the_cpu_twin(levels, storage):
    la, _ = launch(levels, storage)
    plan, spec = la.plan, la.refine
    dtype = np.float64 if storage == "f64" else np.float32
    host = loc._views(la.out_dev.cpu().numpy(), la.lay)         # the pick step's outputs, as the device holds them
    src, _ = rc.host_sources(plan, np.float32)
    maps = (_lib.LocRefineMap * plan.n_queries)()
    for qi, feat in enumerate(la.feats):
        maps[qi].feat, maps[qi].Hf, maps[qi].Wf = feat.data_ptr(), plan.dims[qi][1], plan.dims[qi][2]
    fref = np.full(max(plan.out_rows, 1) * spec.params.cstride * spec.elem, FILL, np.uint8).view(dtype)
    flags = np.full(plan.n_queries, -1, np.int32)
    want = loc.glue_refine_prep_cpu(plan, host, src, maps, spec.params, spec.opts.dtype, fref, flags)
    Q, n_res = plan.n_queries, spec.n_res
    got = (_lib.Problem * (Q * n_res)).from_buffer_copy(la.r_probs.cpu().numpy().tobytes()[:ctypes.sizeof(_lib.Problem) * Q * n_res])
    # the rows, the 0xA5 past every N included, and the flags
    assert la.r_fref.cpu().numpy().tobytes() == fref.view(np.uint8).tobytes()
    dev_flags = la.r_out.cpu().numpy()[la.r_flags_at:la.r_flags_at + 4 * Q].view(np.int32)
    assert list(dev_flags) == list(flags) == [0] * Q
    base_x3 = la.out_dev.data_ptr() + la.lay["b_pts3d"][0]
    for r in range(n_res):
        for qi in range(Q):
            a, b = got[r * Q + qi], want[r * Q + qi]
            for f in ("feat", "Hf", "Wf", "cstride", "c_begin", "c_end", "ld_ref", "N", "im_width", "im_height", "window"):
                assert getattr(a, f) == getattr(b, f), (r, qi, f)
            assert list(a.K) == list(b.K)
            assert a.fref - la.r_fref.data_ptr() == b.fref - fref.ctypes.data
            assert a.pts3d - base_x3 == b.pts3d - host["b_pts3d"].ctypes.data
            if r <= 1:  # (a later level's pose is the previous level's result by now)
                assert bytes(a.R0) == bytes(b.R0) and bytes(a.t0) == bytes(b.t0)
    assert [got[qi].N for qi in range(Q)][4] == 0 and min(got[qi].N for qi in range(4)) > 0


def make_model(ratio):
    kw = dict(config.model_kwargs())
    kw["ratio_threshold"] = ratio
    return sparseFeaturePnP(**kw)


@pytest.mark.parametrize("ratio", [None, 0.5])
def test_batched_compute_cost_equals_the_per_query_launch(ratio):
    la, _ = launch(True, "f32", make_model(ratio))
    plan, spec, L = la.plan, la.refine, _lib.load()
    assert bool(spec.opts.use_ratio) == (ratio is not None)
    Q, n_res = plan.n_queries, spec.n_res
    probs = (_lib.Problem * (Q * n_res)).from_buffer_copy(la.r_probs.cpu().numpy().tobytes()[:ctypes.sizeof(_lib.Problem) * Q * n_res])
    res = la.r_out.cpu().numpy()[:ctypes.sizeof(_lib.Result) * Q * n_res].view(RESULT_DTYPE).reshape(Q, n_res)
    cost = torch.zeros(1024, dtype=torch.float64, device=DEV)
    sup = torch.zeros(1024, dtype=torch.int32, device=DEV)
    one = torch.zeros(ctypes.sizeof(_lib.Result), dtype=torch.uint8, device=DEV)
    seen = 0
    for qi in range(Q):
        p = probs[qi]  # (slot 0: compute_cost over [0, C) at the record's pose; its pointers are the launch's buffers)
        assert (p.c_begin, p.c_end) == (0, lc.C) and p.N <= 1024
        rc_ = L.fmpnp_compute_cost_async(ctypes.byref(p), spec.opts.layout, spec.opts.dtype, spec.opts.use_ratio,
                                         spec.opts.ratio_threshold, cost.data_ptr(), sup.data_ptr(), one.data_ptr(),
                                         _lib.stream_ptr(torch.device(DEV)))
        assert rc_ == 0
        torch.cuda.synchronize(DEV)
        want = one.cpu().numpy().view(RESULT_DTYPE)[0]
        assert res[qi, 0].tobytes() == want.tobytes(), qi
        seen += int(np.isfinite(want["initial_cost"]))
    # (without the ratio test every refined query has a finite mean; with it a query may keep no point: NaN by contract)
    assert seen == 4 if ratio is None else seen >= 1


def test_the_grouping_does_not_matter():
    kw = kw_of(True, "f32", True)
    whole = batched(True, "f32", True)
    ones = fmpnp.localize_multi(queries_of(), lc.IMAGE, refine="batched", refine_group=1, **kw)
    twos = fmpnp.localize_multi(queries_of(), lc.IMAGE, refine="batched", refine_group=2, **kw)
    for (qmap, refs), a, b, c in zip(queries_of(), whole, ones, twos):
        equal_localization(a, b)
        equal_localization(a, c)
        equal_localization(a, fmpnp.localize(qmap, refs, lc.IMAGE, refine="batched", **kw))
    with pytest.raises(ValueError):
        fmpnp.localize_multi(queries_of(), lc.IMAGE, refine="batched", refine_group=0, **kw)


def test_two_runs_are_bit_identical():
    kw = kw_of(True, "f32", True)
    again = fmpnp.localize_multi(queries_of(), lc.IMAGE, refine="batched", **kw)
    for a, b in zip(batched(True, "f32", True), again):
        equal_localization(a, b)


@pytest.mark.parametrize("levels", [False, True])
def test_the_async_form_on_another_stream_equals_the_synchronous_one(levels):
    stream = torch.cuda.Stream(DEV)
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(stream):
        la, got = launch(levels)
        assert la.stream.cuda_stream == stream.cuda_stream != torch.cuda.default_stream(DEV).cuda_stream
    for a, b in zip(got, batched(levels, "f32", True)):
        equal_localization(a, b)


def test_an_inlier_outside_the_map_raises_as_the_per_query_path():
    qmap, refs = on_device("tie")
    best = batched(False, "f32", True)[1].best
    moved = [dict(r) for r in refs]
    p2 = np.array(moved[best]["points_2D"], np.float64)
    p2[np.flatnonzero(lc.scene("tie")["references"][best]["kind"] == "in")[:8], 0] = 64.0  # col = 16: one past the map
    moved[best]["points_2D"] = p2
    assert "sparse_descriptors" in moved[best]  # (its rows do not come from points_2D: only the refinement reads them)
    kw = dict(factor=lc.FACTOR, return_masked=True, **lc.PNP)
    with pytest.raises(IndexError) as per:
        fmpnp.localize(qmap, moved, lc.IMAGE, refine=True, **kw)
    with pytest.raises(IndexError, match="query 1") as bat:
        fmpnp.localize_multi([on_device("mixed"), (qmap, moved), on_device("none")], lc.IMAGE, refine="batched", **kw)
    assert type(per.value) is type(bat.value)


def test_unsupported_arguments_name_the_per_query_path():
    qmap, refs = on_device("fallback_loses")
    kw = dict(factor=lc.FACTOR, return_masked=True, refine="batched", **lc.PNP)
    layers = [dict(r) for r in refs]
    layers[0]["feature_maps"] = [layers[0].pop("hypercolumn")[None]]
    for bad, r in ((dict(track=True), refs), (dict(window=3), refs), (dict(layout="f"), refs), ({}, layers),
                   (dict(feature_pyramid=[(0, 16, (8, 8), None)]), refs)):
        with pytest.raises(ValueError, match="refine=True"):
            fmpnp.localize(qmap, r, lc.IMAGE, **bad, **kw)
    with pytest.raises(ValueError):
        fmpnp.localize(qmap, refs, lc.IMAGE, **dict(kw, refine="batch"))
