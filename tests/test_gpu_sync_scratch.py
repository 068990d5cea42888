"""The scratch of the synchronous entry points (csrc/fmpnp_internal.h SyncCall) through a grow on the call's own
stream: every scratch-owning entry point, one per pool, runs on one non-default stream at its smallest
meaningful shape, then at a shape whose scratch exceeds the pool's minimum (1 MB; 64 MB for fmpnp_feature_pnp),
so the pool frees and reallocates stream-ordered under the call's lock, then at the small shape again.  The two
small calls return the same bits, and where the stage has a CPU twin the small result is the twin's, as the
stage's own GPU test asserts.  (fmpnp_feature_pnp and fmpnp_localize have no twin; the f16 match has a reference
within a bound, not a twin; the LM refiner's twin and the GPU both reproduce the reference's golden trajectory to
1e-9 in the pose and 1e-10 in the cost (test_cpu_twin.py, test_gpu_parity.py), so they lie within twice that of
each other.)  No error path is provoked.  Shapes: the stages' own test cases."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest
import torch

import localize_cases as lc
import match_cases as mc
import pnp_cases as pc
import retrieval_cases as rc
import superpoint_cases as sc
import oracle.oracle as orc
from golden_io import case, maps64

import fmpnp
from fmpnp import _lib, cpu, pnp, refine as rf, superpoint as sp, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MB = 1 << 20
Pred = namedtuple("Prediction", "points_3d reference_inliers matrix quaternion reference_filename")


@pytest.fixture(scope="module")
def stream():
    return torch.cuda.Stream(device=DEV)


def small_large_small(stream, call, small, large):
    """call(small), call(large), call(small) on the stream; the two small results."""
    torch.cuda.synchronize()  # (the operands were formed on the default stream)
    with torch.cuda.stream(stream):
        first = call(small)
        call(large)
        return first, call(small)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def test_refine_batch(stream):
    inp, meta, _ = case("gm_c16")
    f, gx, gy = maps64(inp, orc.sobel)
    feats = rf.pack_features(torch.from_numpy(f), torch.from_numpy(gx), torch.from_numpy(gy), storage=torch.float64,
                             device=DEV)
    args = (inp["fref"], inp["pts3d"], inp["K"], inp["im_width"], inp["im_height"], inp["R0"], inp["t0"])
    small = [rf.make_problem(feats, torch.from_numpy(args[0]), *args[1:])]
    opts = rf.make_options(meta["n_iters"], meta["lambda0"], _lib.GEMAN_MCCLURE, dtype=_lib.F64)
    # 192 problems with a trace of 51 entries of 136 bytes: 1.33 MB of trace alone
    big = []
    for q in range(192):
        s = synth.problem_inputs(512, 8, 12, 16, seed=q, device=DEV)
        big.append(rf.make_problem(rf.pack_features(s["fmap"], storage=torch.float32, device=DEV), s["fref"], s["pts3d"],
                                   s["K"], s["im_width"], s["im_height"], s["R0"], s["t0"]))
    big_opts = rf.make_options(50, 0.01, _lib.GEMAN_MCCLURE, dtype=_lib.F32)
    assert 192 * 51 * ctypes.sizeof(_lib.TraceEntry) > MB

    def call(probs):
        return rf.refine(probs, big_opts if probs is big else opts, trace=True)
    ((a,), (ta,)), ((b,), (tb,)) = small_large_small(stream, call, small, big)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for k in ta:
        assert np.asarray(ta[k]).tobytes() == np.asarray(tb[k]).tobytes(), k
    (twin,), _ = cpu.refine_cpu([cpu.problem_host(cpu.pack_host(f, gx, gy, np.float64), *args)], opts, n_threads=1)
    assert np.allclose(a["R"], twin["R"], rtol=0, atol=2e-9) and np.allclose(a["t"], twin["t"], rtol=0, atol=2e-9)
    assert a["best_cost"] == pytest.approx(twin["best_cost"], rel=2e-10)
    assert (a["n_steps"], a["best_num_inliers"]) == (twin["n_steps"], twin["best_num_inliers"])


def test_feature_pnp(stream):
    def query(C, Hf, Wf, N):
        (batch,), img = synth.pipeline_queries(1, 1, N, C, Hf, Wf, device=DEV, seed0=5)
        q, r, p, K = batch[0]
        return q[None], r, Pred(p.points_3d, p.reference_inliers, p.matrix, np.array([1.0, 0, 0, 0]), "ref.png"), K, img
    # the packed map alone: 240 x 320 texels x 3 planes x 96 channels x 4 bytes = 88 MB
    small, large = query(8, 12, 16, 64), query(96, 240, 320, 512)
    assert 240 * 320 * 3 * 96 * 4 > 64 * MB

    def call(args):
        m = fmpnp.sparseFeaturePnP(50, loss_fn=fmpnp.geman_mcclure_loss, lambda_=0.01)
        R, t, m = fmpnp.feature_pnp(*args, model=m)
        return R, t, float(m.best_cost_), m.best_num_inliers_
    a, b = small_large_small(stream, call, small, large)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_exhaustive_match(stream, precision):
    small, large = (3, 8, 8, 5), (70, 8, 100, 50)  # (N, C, W, H): 70 rows of 5000 scores are 1.4 MB
    assert _lib.load().fmpnp_match_workspace_size(70, 5000) > MB
    ops = {s: tuple(dev(a) for a in mc.operands(*s)) for s in (small, large)}
    top_k = {small: 2, large: 30}

    def call(s):
        return fmpnp.exhaustive_match(*ops[s], top_k[s], mc.RATIO, precision=precision)
    a, b = small_large_small(stream, call, small, large)
    for k in ("argmax", "top", "kth", "mask"):
        assert a[k].tobytes() == b[k].tobytes(), k
    if precision == "f32":
        mc.assert_same_result(a, mc.twin(*small, top_k[small]), small)


def test_pnp_ransac(stream):
    def problems(n, M, iters):
        return [pc.problem(pc.generate(M, 0.3, 0.5, 400.0, (0.0, 0.0, 0.0, 0.0), 7000 + M + i, iters)) for i in range(n)]
    small, large = problems(1, 13, 64), problems(8, 4100, 64)  # (8 x 4100 points of 40 bytes are 1.3 MB)
    assert 8 * 4100 * 40 > MB
    a, b = small_large_small(stream, lambda probs: pnp.ransac(probs, DEV), small, large)
    (twin,) = pnp.ransac_cpu(small, 4)
    for k in ("R", "t", "R_hyp", "t_hyp", "cost", "num_inliers", "best_h", "status", "polish_iters", "mask"):
        assert np.asarray(a[0][k]).tobytes() == np.asarray(b[0][k]).tobytes(), k
        assert np.asarray(a[0][k]).tobytes() == np.asarray(twin[k]).tobytes(), k


def test_netvlad_pool(stream):
    lib = _lib.load()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(args):
        x, weight, centroids = args
        b, c, h, w = x.shape
        k = weight.shape[0]
        out = torch.full((b, k * c), -7.0, device=DEV)
        rc_ = lib.fmpnp_netvlad_pool(vp(x), b, c, h * w, c * h * w, h * w, vp(weight), k, c, vp(centroids), c, 1, vp(out),
                                     out.stride(0), ctypes.c_void_p(stream.cuda_stream))
        assert rc_ == 0
        return out.cpu()
    small = [t.to(DEV) for t in rc.inputs("ragged")]
    large = [t.to(DEV) for t in rc.inputs("production", 8)]
    assert lib.fmpnp_netvlad_workspace_size(8, 64, 512, 99) > MB
    a, b = small_large_small(stream, call, small, large)
    assert torch.equal(a, b) and torch.equal(a, rc.twin("ragged"))


def test_rank_topn(stream):
    lib = _lib.load()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(args):
        ref, qry, n = args
        ref_t = ref.to(DEV).t().contiguous()
        q = qry.to(DEV)
        (nq, d), r = q.shape, ref_t.shape[1]
        idx = torch.full((nq, n), -1, dtype=torch.int32, device=DEV)
        top = torch.full((nq, n), -7.0, device=DEV)
        rc_ = lib.fmpnp_rank_topn(vp(q), nq, d, vp(ref_t), d, r, r, n, vp(idx), vp(top), None,
                                  ctypes.c_void_p(stream.cuda_stream))
        assert rc_ == 0
        return idx.cpu(), top.cpu()
    ref, qry = rc.rank_inputs("order")
    gen = torch.Generator().manual_seed(11)
    large = (torch.randn(3000, 8, generator=gen), torch.randn(100, 8, generator=gen), 10)  # 100 x 3000 scores: 1.2 MB
    assert lib.fmpnp_match_workspace_size(100, 3000) > MB
    (ia, ta), (ib, tb) = small_large_small(stream, call, (ref, qry, 3), large)
    widx, wtop = fmpnp.rank_topn_cpu(ref, qry, 3)[:2]
    assert torch.equal(ia, ib) and rc.same_floats(ta, tb)
    assert torch.equal(ia, widx) and rc.same_floats(ta, wtop)


def test_localize(stream):
    def on_device(name):
        scene = lc.scene(name)
        refs = []
        for r in scene["references"]:
            r = lc.public(r)
            r["hypercolumn"] = torch.from_numpy(r["hypercolumn"]).to(DEV)
            refs.append(r)
        return torch.from_numpy(scene["query"]).to(DEV), refs
    # "mixed": 1479 rows against a 16 x 16 map: 1.5 MB of match scores; "fallback_loses": 113 rows
    assert _lib.load().fmpnp_match_workspace_size(1479, lc.W * lc.H) > MB

    def call(args):
        return fmpnp.localize(*args, lc.IMAGE, factor=lc.FACTOR, return_masked=True, refine=False, return_all=True,
                              **lc.PNP)
    a, b = small_large_small(stream, call, on_device("fallback_loses"), on_device("mixed"))
    assert a.kind == b.kind == "solved" and a.best == b.best
    lc.equal(a.export, b.export, "export")
    lc.equal_prediction(a.prediction, b.prediction, "best")
    for j, (x, y) in enumerate(zip(a.predictions, b.predictions)):
        lc.equal_prediction(x, y, f"pair {j}")


def test_sp_match(stream):
    def operands(name):
        d1, d2 = sc.matching_inputs(name, int(sc.golden("matching")[f"{name}.seed"]))
        return dev(d1), dev(d2), sc.MATCHING[name][3]
    assert _lib.load().fmpnp_match_workspace_size(1000, 1000) > MB  # (1000 x 1000 scores: 4 MB)
    a, b = small_large_small(stream, lambda args: sp.two_nearest(*args), operands("two"), operands("n1000_1000"))
    d1, d2 = sc.matching_inputs("two", int(sc.golden("matching")["two.seed"]))
    twin = sp.two_nearest(d1, d2, sc.MATCHING["two"][3], cpu=True)
    for k in ("idx", "dist", "ok", "matches"):
        lc.equal(a[k], b[k], k)
        lc.equal(a[k], twin[k], k)
