"""The localisation chain with the query given as its encoder layers (fmpnp_localize_layers behind fmpnp.localize):
equal to the staged composition exhaustive_search_layers_multi -> solve_pnp_multi -> pick bit for bit, to the CPU
twins' chain, and through the refinement to feature_pnp(query_layers=, reference_layers=) on the picked prediction.
The scenes are tests/localize_cases.py's smallest, rebuilt by its own builder around a query map that is the
assembly of two seeded layers."""
import functools

import numpy as np
import pytest
import torch

import fmpnp
import localize_cases as lc
from fmpnp.match import exhaustive_search_layers_multi, exhaustive_search_multi, gather_sparse_descriptors
from fmpnp.matrix_utils import matrix_quaternion
from test_gpu_localize import equal_localization, equal_refined

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ITEM = 1  # the query is item 1 of a batch of two
SCENES = ("fallback_loses", "tie")
SPLIT = 20  # the references' two equal-size layers: channels [0, 20) and [20, 32)


@functools.lru_cache(maxsize=None)
def scene(name):
    """localize_cases.scene with its query map replaced by assemble_hypercolumn_cpu of two seeded layers (a
    full-size one and one of half the size): dict(layers (CPU), query [C, W, H], references)."""
    seed, specs = lc.SCENES[name]
    rng = np.random.Generator(np.random.PCG64(seed))
    g = torch.Generator().manual_seed(seed)
    layers = [torch.randn(2, SPLIT, lc.W, lc.H, generator=g), torch.randn(2, lc.C - SPLIT, lc.W // 2, lc.H // 2, generator=g)]
    qmap = fmpnp.assemble_hypercolumn_cpu(layers)[ITEM].numpy().copy()
    R, t = lc._pose(rng)
    refs = []
    for j, spec in enumerate(specs):
        if spec[0] == "same":
            r = dict(refs[spec[1]])
            r["filename"] = f"{name}/ref{j}.png"
            refs.append(r)
            continue
        kinds, K, dense, fallback = spec
        refs.append(lc._reference(rng, f"{name}/ref{j}.png", qmap, R, t, K, kinds, dense, fallback, 1000 * seed + j))
    return dict(layers=layers, query=qmap, references=refs)


@functools.lru_cache(maxsize=None)
def on_device(name, as_layers=False):
    """(query layers, dense query map, references) on the device; as_layers: every reference carries feature_maps
    (its map cut in two equal-size layers) in place of hypercolumn."""
    sc = scene(name)
    refs = []
    for r in sc["references"]:
        r = lc.public(r)
        hc = torch.from_numpy(r["hypercolumn"]).to(DEV)
        if as_layers:
            del r["hypercolumn"]
            r["feature_maps"] = [hc[None, :SPLIT].contiguous(), hc[None, SPLIT:].contiguous()]
        else:
            r["hypercolumn"] = hc
        refs.append(r)
    return [m.to(DEV) for m in sc["layers"]], torch.from_numpy(sc["query"]).to(DEV), refs


def rows_of(r):
    if "sparse_descriptors" in r:
        return torch.from_numpy(r["sparse_descriptors"]).to(DEV)
    cell = (lc.IMAGE[0] / lc.W, lc.IMAGE[1] / lc.H)
    if "feature_maps" in r:
        return fmpnp.sparse_hypercolumn(r["feature_maps"], r["points_2D"], at="cell", cell_size=cell)
    return gather_sparse_descriptors(r["hypercolumn"], r["points_2D"], *cell)


def staged(name, as_layers=False, dense_query=False):
    layers, qmap, refs = on_device(name, as_layers)
    sparse = [rows_of(r) for r in refs]
    if dense_query:
        found = exhaustive_search_multi(qmap.reshape(lc.C, -1), sparse, lc.IMAGE, [lc.W, lc.H], None, lc.FACTOR)
    else:
        found = exhaustive_search_layers_multi(layers, sparse, lc.IMAGE, None, lc.FACTOR, item=ITEM)
    matches = [(pts.cpu().numpy(), mask) for pts, mask in found]

    def solve(points_2D, points_3D, ref, ref_2D):
        return fmpnp.solve_pnp_multi([(points_2D, points_3D, ref["filename"], ref_2D, None)], ref["intrinsics"],
                                     ref["distortion_coefficients"], return_masked=True, **lc.PNP)[0]
    return lc.staged(refs, matches, solve)


def assert_equals_staged(got, every, eligible):
    export, best = lc.choose([p for _, p in eligible])
    lc.equal(got.export, export, "export")
    lc.equal_prediction(got.prediction, best, "best")
    for j, pred in enumerate(every):
        lc.equal_prediction(got.predictions[j], pred, f"pair {j}")
    return best


def query_of(layers):
    return dict(feature_maps=layers, feature_item=ITEM)


@pytest.mark.parametrize("name", SCENES)
def test_layered_query_equals_the_staged_composition_and_the_cpu_chain(name):
    layers, _, refs = on_device(name)
    every, eligible, _ = staged(name)
    got = fmpnp.localize(query_of(layers), refs, lc.IMAGE, factor=lc.FACTOR, return_masked=True, refine=False,
                         return_all=True, **lc.PNP)
    best = assert_equals_staged(got, every, eligible)
    assert best is not None and best.inlier_mask is not None and got.kind == "solved"  # (the scene solves)
    sc = scene(name)
    cpu = fmpnp.localize_cpu(query_of(sc["layers"]), [lc.public(r) for r in sc["references"]], lc.IMAGE, factor=lc.FACTOR,
                             return_masked=True, return_all=True, **lc.PNP)
    equal_localization(got, cpu)
    # a list of layers is the same query as the mapping (its item: slice it)
    again = fmpnp.localize([m[ITEM:ITEM + 1] for m in layers], refs, lc.IMAGE, factor=lc.FACTOR, return_masked=True,
                           refine=False, return_all=True, **lc.PNP)
    equal_localization(again, got)


def test_localize_multi_with_layered_queries_equals_the_single_calls():
    queries = [(query_of(on_device(name)[0]), on_device(name)[2]) for name in SCENES]
    multi = fmpnp.localize_multi(queries, lc.IMAGE, factor=lc.FACTOR, return_masked=True, refine=False, return_all=True,
                                 **lc.PNP)
    for (q, refs), got in zip(queries, multi):
        one = fmpnp.localize(q, refs, lc.IMAGE, factor=lc.FACTOR, return_masked=True, refine=False, return_all=True,
                             **lc.PNP)
        equal_localization(got, one)


def test_refined_without_any_dense_hypercolumn_equals_feature_pnp_on_the_layers():
    name = "fallback_loses"
    layers, _, refs = on_device(name, as_layers=True)
    assert all("hypercolumn" not in r for r in refs)
    every, eligible, _ = staged(name, as_layers=True)
    got = fmpnp.localize(query_of(layers), refs, lc.IMAGE, factor=lc.FACTOR, return_masked=True, return_all=True, **lc.PNP)
    best = assert_equals_staged(got, every, eligible)
    j = [k for k, p in eligible if p is best][0]
    assert got.best == j and got.kind == "solved"
    K = torch.from_numpy(np.asarray(refs[-1]["intrinsics"], np.float64))  # the LAST reference's K
    R, t, model = fmpnp.feature_pnp(None, None, best, K, lc.IMAGE, query_layers=[m[ITEM:ITEM + 1] for m in layers],
                                    reference_layers=refs[j]["feature_maps"])
    T = np.eye(4)
    T[:3, :3], T[3, :3] = R.numpy(), t.numpy()
    equal_refined(got.refined, (list(t.numpy()), list(matrix_quaternion(T)), model))
    assert np.isfinite(np.asarray(got.refined[0])).all() and np.isfinite(np.asarray(got.refined[1])).all()


def test_what_a_layered_query_cannot_be_combined_with():
    layers, qmap, refs = on_device("fallback_loses")
    kw = dict(factor=lc.FACTOR, return_masked=True, **lc.PNP)
    with pytest.raises(ValueError, match="match_precision"):
        fmpnp.localize(query_of(layers), refs, lc.IMAGE, match_precision="f16", **kw)
    with pytest.raises(ValueError, match="refine"):
        fmpnp.localize(query_of(layers), refs, lc.IMAGE, refine="batched", **kw)
    with pytest.raises(ValueError, match="match_precision"):
        fmpnp.localize_cpu(query_of(scene("fallback_loses")["layers"]), refs, lc.IMAGE, match_precision="f16", **kw)
    with pytest.raises(ValueError):
        fmpnp.localize_multi([(query_of(layers), refs), (qmap, refs)], lc.IMAGE, refine=False, **kw)
    with pytest.raises(ValueError):
        fmpnp.localize(dict(feature_maps=layers, feature_item=2), refs, lc.IMAGE, refine=False, **kw)


def test_the_dense_query_on_the_same_scene_keeps_its_bits():
    """The dense-query chain is untouched: on the same scene it still equals its own staged composition
    (exhaustive_search_multi on the assembled map), whose bits are not the layered path's."""
    name = "fallback_loses"
    layers, qmap, refs = on_device(name)
    every, eligible, _ = staged(name, dense_query=True)
    got = fmpnp.localize(qmap, refs, lc.IMAGE, factor=lc.FACTOR, return_masked=True, refine=False, return_all=True, **lc.PNP)
    assert_equals_staged(got, every, eligible)
    assert torch.equal(fmpnp.assemble_hypercolumn(layers)[ITEM], qmap)
