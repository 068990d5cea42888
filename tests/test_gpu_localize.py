"""The localisation chain on the GPU (fmpnp.localize / localize_multi / LocalizeLaunch): equal to the CPU twins'
chain bit for bit up to the best prediction, and equal to the staged composition of the public stages
(exhaustive_search_multi -> numpy masking -> solve_pnp_multi -> numpy best pick -> feature_pnp) through the
refinement.  Scenes and yardstick: tests/localize_cases.py."""
import functools
import os

import numpy as np
import pytest
import torch

import localize_cases as lc
import fmpnp
from fmpnp import _localize as loc  # (the module: fmpnp.localize is the function)
from fmpnp import replay
from fmpnp.match import exhaustive_search_multi, gather_sparse_descriptors
from fmpnp.matrix_utils import matrix_quaternion

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5


@functools.lru_cache(maxsize=None)
def on_device(name):
    """(query map, references) of a scene with the maps on the device."""
    sc = lc.scene(name)
    refs = []
    for r in sc["references"]:
        r = lc.public(r)
        r["hypercolumn"] = torch.from_numpy(r["hypercolumn"]).to(DEV)
        refs.append(r)
    return torch.from_numpy(sc["query"]).to(DEV), refs


def refine_as_the_adapter(qmap, ref, prediction, K):
    """optimize_feature_pnp.py:73-91 around feature_pnp."""
    R, t, model = fmpnp.feature_pnp(qmap[None], ref["hypercolumn"], prediction, torch.from_numpy(np.asarray(K, np.float64)),
                                    lc.IMAGE)
    T = np.eye(4)
    T[:3, :3], T[3, :3] = R.numpy(), t.numpy()
    return list(t.numpy()), list(matrix_quaternion(T)), model


@functools.lru_cache(maxsize=None)
def gpu_yardstick(name, return_masked=True):
    qmap, refs = on_device(name)
    sparse = []
    for r in refs:
        if "sparse_descriptors" in r:
            sparse.append(torch.from_numpy(r["sparse_descriptors"]).to(DEV))
        else:
            sparse.append(gather_sparse_descriptors(r["hypercolumn"], r["points_2D"], lc.IMAGE[0] / lc.W, lc.IMAGE[1] / lc.H))
    found = exhaustive_search_multi(qmap.reshape(lc.C, -1), sparse, lc.IMAGE, [lc.W, lc.H], None, lc.FACTOR)
    matches = [(pts.cpu().numpy(), mask) for pts, mask in found]

    def solve(points_2D, points_3D, ref, ref_2D):
        return fmpnp.solve_pnp_multi([(points_2D, points_3D, ref["filename"], ref_2D, None)], ref["intrinsics"],
                                     ref["distortion_coefficients"], return_masked=return_masked, **lc.PNP)[0]
    return lc.staged(refs, matches, solve)


@functools.lru_cache(maxsize=None)
def chain(name, return_masked=True):
    qmap, refs = on_device(name)
    return fmpnp.localize(qmap, refs, lc.IMAGE, factor=lc.FACTOR, return_masked=return_masked, refine=False,
                          return_all=True, **lc.PNP)


def equal_localization(a, b, refined=False):
    lc.equal(a.export, b.export, "export")
    lc.equal_prediction(a.prediction, b.prediction, "best")
    assert a.kind == b.kind and a.best == b.best
    assert (a.predictions is None) == (b.predictions is None)
    for j, (x, y) in enumerate(zip(a.predictions or [], b.predictions or [])):
        lc.equal_prediction(x, y, f"pair {j}")
        for k in replay.ENTRY_KEYS:
            lc.equal(a.cached_matches[j][k], b.cached_matches[j][k], f"cached {j}.{k}")
    if refined:
        equal_refined(a.refined, b.refined)


def equal_refined(a, b):
    if a is None or b is None:
        assert a is None and b is None
        return
    lc.equal(a[0], b[0], "t")
    lc.equal(a[1], b[1], "quaternion")
    for k in ("initial_cost_", "best_cost_", "best_num_inliers_"):
        x, y = getattr(a[2], k, None), getattr(b[2], k, None)
        assert (x is None) == (y is None), k
        if x is None:
            continue
        lc.equal(x.cpu().numpy() if torch.is_tensor(x) else x, y.cpu().numpy() if torch.is_tensor(y) else y, k)


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("name", sorted(lc.SCENES))
def test_localize_equals_the_cpu_chain(name, masked):
    sc = lc.scene(name)
    cpu = fmpnp.localize_cpu(sc["query"], [lc.public(r) for r in sc["references"]], lc.IMAGE, factor=lc.FACTOR,
                             return_masked=masked, return_all=True, **lc.PNP)
    equal_localization(chain(name, masked), cpu)


@pytest.mark.parametrize("name", sorted(lc.SCENES))
def test_refined_equals_the_staged_yardstick(name):
    qmap, refs = on_device(name)
    every, eligible, arrays = gpu_yardstick(name)
    export, best = lc.choose([p for _, p in eligible])
    got = fmpnp.localize(qmap, refs, lc.IMAGE, factor=lc.FACTOR, return_masked=True, return_all=True, **lc.PNP)
    lc.equal(got.export, export, "export")
    lc.equal_prediction(got.prediction, best, "best")
    for j, pred in enumerate(every):
        lc.equal_prediction(got.predictions[j], pred, f"pair {j}")
    if best is None:
        assert name == "none" and got.refined is None and got.kind == "none"
        return
    j = [k for k, p in eligible if p is best][0]
    assert got.best == j and got.kind == ("fallback" if best.inlier_mask is None else "solved")
    want = refine_as_the_adapter(qmap, refs[j], best, refs[-1]["intrinsics"])  # the LAST reference's K (:143,167,244)
    equal_refined(got.refined, want)
    assert np.isfinite(np.asarray(got.refined[0])).all() and np.isfinite(np.asarray(got.refined[1])).all()


def test_the_gpu_yardstick_reaches_the_branches():
    mm = lc.PNP["minimum_matches"]
    reached = {name: lc.branches(on_device(name)[1], *gpu_yardstick(name), mm) for name in lc.SCENES}
    assert {"mask_all_zero", "count_le_minimum_matches", "too_few_inliers_absent", "solved"} <= reached["mixed"]
    assert "tie_earlier_wins" in reached["tie"] and "fallback_wins" in reached["fallback_wins"]
    assert {"too_few_inliers_with_fallback", "solved"} <= reached["fallback_loses"] and "none" in reached["none"]


def test_return_masked_false_through_the_refinement():
    qmap, refs = on_device("mixed")
    every, eligible, _ = gpu_yardstick("mixed", False)
    _, best = lc.choose([p for _, p in eligible])
    got = fmpnp.localize(qmap, refs, lc.IMAGE, factor=lc.FACTOR, return_masked=False, **lc.PNP)
    lc.equal_prediction(got.prediction, best, "best")
    assert best.points_3d.shape[0] == best.num_matches > best.num_inliers == len(best.inlier_mask)
    j = [k for k, p in eligible if p is best][0]
    equal_refined(got.refined, refine_as_the_adapter(qmap, refs[j], best, refs[-1]["intrinsics"]))


def test_refine_intrinsics_last_against_best():
    qmap, refs = on_device("fallback_loses")
    _, eligible, _ = gpu_yardstick("fallback_loses")
    _, best = lc.choose([p for _, p in eligible])
    j = [k for k, p in eligible if p is best][0]
    assert not np.array_equal(refs[-1]["intrinsics"], refs[j]["intrinsics"])
    kw = dict(factor=lc.FACTOR, return_masked=True, **lc.PNP)
    last = fmpnp.localize(qmap, refs, lc.IMAGE, **kw)
    same = fmpnp.localize(qmap, refs, lc.IMAGE, refine_intrinsics="last", **kw)
    bst = fmpnp.localize(qmap, refs, lc.IMAGE, refine_intrinsics="best", **kw)
    equal_refined(last.refined, refine_as_the_adapter(qmap, refs[j], best, refs[-1]["intrinsics"]))
    equal_refined(same.refined, last.refined)
    equal_refined(bst.refined, refine_as_the_adapter(qmap, refs[j], best, refs[j]["intrinsics"]))
    assert np.asarray(bst.refined[0]).tobytes() != np.asarray(last.refined[0]).tobytes()
    with pytest.raises(ValueError):
        fmpnp.localize(qmap, refs, lc.IMAGE, refine_intrinsics="first", **kw)


def test_localize_multi_equals_single_calls():
    queries = [on_device(name) for name in lc.MULTI]
    kw = dict(factor=lc.FACTOR, return_masked=True, return_all=True, **lc.PNP)
    multi = fmpnp.localize_multi(queries, lc.IMAGE, **kw)
    kinds = [m.kind for m in multi]
    assert kinds == ["solved", "none", "fallback"]
    for (qmap, refs), m in zip(queries, multi):
        equal_localization(m, fmpnp.localize(qmap, refs, lc.IMAGE, **kw), refined=True)


def test_async_form_on_another_stream_with_prefilled_buffers():
    params = loc._pnp_params(return_masked=True, **lc.PNP)
    stream = torch.cuda.Stream(DEV)
    for name in ("mixed", "fallback_wins", "none"):
        qmap, refs = on_device(name)
        torch.cuda.synchronize(DEV)
        with torch.cuda.stream(stream):
            launch = loc.LocalizeLaunch([(qmap, refs)], lc.IMAGE, lc.FACTOR, params, return_all=True, fill=FILL)
            assert launch.stream.cuda_stream == stream.cuda_stream != torch.cuda.default_stream(DEV).cuda_stream
            got, = launch.read()
        equal_localization(got, chain(name))
        # the rows past a pair's count keep the fill: nothing but the contract's bytes is written
        out = launch.out_dev.cpu().numpy()
        v = loc._views(out, launch.lay)
        for g in range(launch.plan.n_pairs):
            off, n, cnt = launch.plan.pairs[g].row_offset, launch.plan.pairs[g].n_rows, int(v["counts"][g])
            assert (v["m_x3"].reshape(-1, 3)[off + cnt:off + n].view(np.uint8) == FILL).all()
            assert (v["m_src"][off + cnt:off + n].view(np.uint8) == FILL).all()


def test_two_runs_are_bit_identical():
    qmap, refs = on_device("mixed")
    kw = dict(factor=lc.FACTOR, return_masked=True, return_all=True, **lc.PNP)
    # (the synchronous form's host arrays pre-filled too: only the contract's rows are written, none is read)
    params = loc._pnp_params(return_masked=True, **lc.PNP)
    filled, = loc._run_sync([(qmap, refs)], lc.IMAGE, lc.FACTOR, params, True, fill=FILL)
    equal_localization(filled, chain("mixed"))
    equal_localization(fmpnp.localize(qmap, refs, lc.IMAGE, **kw), fmpnp.localize(qmap, refs, lc.IMAGE, **kw), refined=True)


def test_return_all_round_trips_through_the_flat_cache(tmp_path):
    got = chain("fallback_loses")
    entries = {f"query.png:{e['reference_filename']}": e for e in got.cached_matches}
    path = os.path.join(tmp_path, "cache.npz")
    replay.save_flat(entries, path)
    back = replay.load_flat(path)
    assert list(back) == list(entries)
    for key, e in entries.items():
        for k in replay.ENTRY_KEYS:
            a, b = e[k], back[key][k]
            if a is None:
                assert b is None
            else:
                assert np.asarray(a).tobytes() == np.asarray(b).tobytes() and np.asarray(a).shape == np.asarray(b).shape, (key, k)
    solved = back[f"query.png:{got.prediction.reference_filename}"]
    assert solved["success"] and solved["num_inliers"] == got.prediction.num_inliers
    assert np.array_equal(solved["inlier_mask"], got.prediction.inlier_mask)
