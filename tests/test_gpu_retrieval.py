"""Retrieval on the GPU: the pooling kernels and the top-n selection against their CPU twins bit for bit on
every case, synchronously and on a side stream, an image alone against the same image inside batches of 3 and
65, out= views, a poisoned workspace, NetVLAD.forward and compute_embedding end to end, and compute_ranks on
GPU tensors against the reference's golden ranks."""
import ctypes

import numpy as np
import pytest
import torch

import fmpnp
from fmpnp import _lib

import retrieval_cases as rc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(*tensors):
    return [t.to(DEV) for t in tensors]


@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("name", rc.ALL)
def test_gpu_pool_equals_the_twin(name, normalize):
    """== on every element, with the case's own batch, a batch of 3 and strided batch slices."""
    for batch in (None, 3):
        x, weight, centroids = rc.inputs(name, batch)
        want = rc.twin(name, normalize, batch)
        got = fmpnp.netvlad_pool(*dev(x, weight, centroids), normalize)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape
        assert torch.equal(got.cpu(), want), (name, normalize, batch)
    sliced = fmpnp.netvlad_pool(rc.strided(x, DEV), *dev(weight, centroids), normalize)
    assert torch.equal(sliced.cpu(), want), (name, normalize, "strided")


@pytest.mark.parametrize("name", rc.pool_golden_cases())
def test_gpu_pool_golden(name):
    """The reference's inputs: the twin's bits, and so within the reference's own error of its fp64 run."""
    g = rc.golden_pool(name)
    x, weight, centroids = (torch.from_numpy(g[k]) for k in ("x", "weight", "centroids"))
    got = fmpnp.netvlad_pool(*dev(x, weight, centroids)).cpu()
    assert torch.equal(got, fmpnp.netvlad_pool_cpu(x, weight, centroids))
    err, bound = float(np.abs(got.double().numpy() - g["v64"]).max()), rc.tolerance(g["e_ref"], g["v64"])
    print(f"{name}: kernel error {err:.3g}, bound {bound:.3g}")
    assert err <= bound


def _pool_raw(entry, x, weight, centroids, out, stream, workspace=None):
    """The C entry points on contiguous CUDA tensors: entry = "sync" or "async"."""
    lib = _lib.load()
    b, c, h, w = x.shape
    k = weight.shape[0]
    args = [ctypes.c_void_p(x.data_ptr()), b, c, h * w, c * h * w, h * w, ctypes.c_void_p(weight.data_ptr()), k, c,
            ctypes.c_void_p(centroids.data_ptr()), c, 1, ctypes.c_void_p(out.data_ptr()), out.stride(0)]
    if entry == "sync":
        return lib.fmpnp_netvlad_pool(*args, ctypes.c_void_p(stream.cuda_stream))
    return lib.fmpnp_netvlad_pool_async(*args, ctypes.c_void_p(workspace.data_ptr()), workspace.numel() * 4,
                                        ctypes.c_void_p(stream.cuda_stream))


@pytest.mark.parametrize("name", ["ragged", "segments", "clusters70"])
def test_gpu_pool_entry_points_streams_and_poisoned_workspace(name):
    """The synchronous entry point (its own scratch) and the asynchronous one over a NaN-filled and a
    garbage-filled workspace, on the current stream and on a side stream: the twin's bits every time."""
    x, weight, centroids = dev(*rc.inputs(name, 3))
    want = rc.twin(name, True, 3)
    lib = _lib.load()
    b, c, h, w = x.shape
    nbytes = lib.fmpnp_netvlad_workspace_size(b, weight.shape[0], c, h * w)
    assert nbytes > 0
    side = torch.cuda.Stream(device=DEV)
    for stream in (torch.cuda.current_stream(DEV), side):
        stream.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(stream):
            out = torch.full(want.shape, -7.0, device=DEV)
            assert _pool_raw("sync", x, weight, centroids, out, stream) == 0
            assert torch.equal(out.cpu(), want)
            for poison in (float("nan"), 3.0e38):
                ws = torch.full((nbytes // 4 + 1,), poison, device=DEV)
                out = torch.full(want.shape, -7.0, device=DEV)
                assert _pool_raw("async", x, weight, centroids, out, stream, ws) == 0
                stream.synchronize()
                assert torch.equal(out.cpu(), want), (name, poison)
    short = torch.zeros(4, device=DEV)
    assert _pool_raw("async", x, weight, centroids, out, side, short) == _lib.EINVAL
    got = fmpnp.netvlad_pool(x, weight, centroids, stream=side)
    side.synchronize()
    assert torch.equal(got.cpu(), want)


def test_gpu_pool_image_alone_in_3_and_in_65():
    """The bits of an image do not depend on the batch around it or its place in it."""
    x, weight, centroids = dev(*rc.inputs("segments"))
    alone = fmpnp.netvlad_pool(x, weight, centroids)
    assert torch.equal(alone.cpu(), rc.twin("segments"))
    filler = torch.randn(65, *x.shape[1:], device=DEV).clamp_min(0.0) ** 3
    for batch, at in ((3, 1), (65, 0), (65, 64), (65, 37)):
        xs = filler[:batch].clone()
        xs[at] = x[0]
        got = fmpnp.netvlad_pool(xs, weight, centroids)
        assert torch.equal(got[at], alone[0]), (batch, at)


def test_gpu_pool_out_view():
    x, weight, centroids = dev(*rc.inputs("small", 3))
    want = rc.twin("small", True, 3)
    buf, view = rc.view_out(*want.shape, device=DEV)
    assert view.data_ptr() % 16 == 4
    got = fmpnp.netvlad_pool(x, weight, centroids, out=view)
    assert got.data_ptr() == view.data_ptr() and torch.equal(view.cpu(), want)
    view.fill_(-7.0)
    assert bool((buf == -7.0).all())


def test_gpu_netvlad_module_and_compute_embedding():
    """NetVLAD.forward end to end: the reference's parameters in, the kernel's (= the twin's) descriptors out,
    within the reference's error of its golden; compute_embedding batches equal-sized images through it."""
    g = rc.golden_pool("clusters64")
    net = fmpnp.NetVLAD(num_clusters=64, dim=128)
    net.init_params(g["clsts"].copy(), g["train"].copy())
    net = net.to(DEV).eval()
    x = torch.from_numpy(g["x"])
    with torch.no_grad():
        got = net(x.to(DEV))
    assert torch.equal(got.cpu(), fmpnp.netvlad_pool_cpu(x, torch.from_numpy(g["weight"]), torch.from_numpy(g["centroids"])))
    assert float(np.abs(got.cpu().double().numpy() - g["v64"]).max()) <= rc.tolerance(g["e_ref"], g["v64"])

    torch.manual_seed(20262)
    encoder = torch.nn.Sequential(torch.nn.Conv2d(3, 128, 3, stride=2, padding=1), torch.nn.ReLU()).to(DEV).eval()
    images = [torch.randn(3, 18, 22), torch.randn(3, 18, 22), torch.randn(3, 18, 22), torch.randn(3, 14, 10)]
    desc = fmpnp.compute_embedding(encoder, net, images, batch=2)
    assert desc.is_cuda and tuple(desc.shape) == (4, 64 * 128)
    with torch.no_grad():  # (the groups it forms: two of the three equal-sized images, the third, the smaller one)
        for lo, hi in ((0, 2), (2, 3), (3, 4)):
            assert torch.equal(desc[lo:hi], net(encoder(torch.stack(images[lo:hi]).to(DEV)))), (lo, hi)


def _rank_raw(entry, qry, ref_t, n, stream, scores=None, workspace=None):
    lib = _lib.load()
    (q, d), r = qry.shape, ref_t.shape[1]
    idx = torch.full((q, n), -1, dtype=torch.int32, device=DEV)
    top = torch.full((q, n), -7.0, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    args = [vp(qry), q, d, vp(ref_t), d, r, r, n, vp(idx), vp(top), vp(scores)]
    if entry == "sync":
        rc_ = lib.fmpnp_rank_topn(*args, ctypes.c_void_p(stream.cuda_stream))
    else:
        rc_ = lib.fmpnp_rank_topn_async(*args, vp(workspace), workspace.numel() * 4 if workspace is not None else 0,
                                        ctypes.c_void_p(stream.cuda_stream))
    return rc_, idx, top


@pytest.mark.parametrize("name", ["order", "wide", "golden"])
def test_gpu_rank_equals_the_twin(name):
    """idx, top and the score map equal the twin's under == (NaNs at the same places) for n = 1, a middle n, the
    cap or R; both entry points, the current and a side stream, a poisoned workspace."""
    if name == "golden":
        g = rc.golden("rank")
        ref, qry = torch.from_numpy(g["ref"]), torch.from_numpy(g["qry"])
    else:
        ref, qry = rc.rank_inputs(name)
    r = ref.shape[0]
    dref, dqry = dev(ref, qry)
    ref_t = dref.t().contiguous()
    side = torch.cuda.Stream(device=DEV)
    for n in sorted({1, min(10, r), min(r, _lib.RANK_TOPN_CAP)}):
        widx, wtop, wscores = fmpnp.rank_topn_cpu(ref, qry, n, scores=True)
        idx, top, scores = fmpnp.rank_topn(dref, dqry, n, scores=True)
        assert torch.equal(idx.cpu(), widx) and rc.same_floats(top.cpu(), wtop)
        assert rc.same_floats(scores.cpu(), wscores)
        idx, top = fmpnp.rank_topn(dref, dqry, n, stream=side)
        side.synchronize()
        assert torch.equal(idx.cpu(), widx) and rc.same_floats(top.cpu(), wtop)
        for stream in (torch.cuda.current_stream(DEV), side):
            stream.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(stream):
                rc_, idx, top = _rank_raw("sync", dqry, ref_t, n, stream)
                assert rc_ == 0 and torch.equal(idx.cpu(), widx)
                ws = torch.full((_lib.load().fmpnp_match_workspace_size(qry.shape[0], r) // 4 + 1,), float("nan"),
                                device=DEV)
                rc_, idx, top = _rank_raw("async", dqry, ref_t, n, stream, workspace=ws)
                stream.synchronize()
                assert rc_ == 0 and torch.equal(idx.cpu(), widx)
                assert rc.same_floats(top.cpu(), wtop)
    if name == "golden":
        assert np.array_equal(fmpnp.rank_topn(dref, dqry, 30)[0].cpu().numpy().T, g["ranks_raw"][:30])


def test_gpu_rank_argument_errors():
    qry, ref_t = torch.zeros(2, 3, device=DEV), torch.zeros(3, 2000, device=DEV)
    s = torch.cuda.current_stream(DEV)
    assert _rank_raw("sync", qry, ref_t, 0, s)[0] == _lib.EINVAL
    assert _rank_raw("sync", qry, ref_t, 2001, s)[0] == _lib.EINVAL
    assert _rank_raw("sync", qry, ref_t, _lib.RANK_TOPN_CAP + 1, s)[0] == _lib.ETOOBIG
    assert _rank_raw("async", qry, ref_t, 5, s, workspace=None)[0] == _lib.EINVAL  # (no score map, no workspace)
    with pytest.raises(ValueError):
        fmpnp.rank_topn(qry.cpu(), ref_t.t().contiguous(), 3)
    with pytest.raises(ValueError):
        fmpnp.netvlad_pool(torch.zeros(1, 2, 3, 3), torch.zeros(4, 2, device=DEV), torch.zeros(4, 2, device=DEV))


def test_gpu_compute_ranks_equals_the_references():
    g = rc.golden("rank")
    ref, qry = dev(torch.from_numpy(g["ref"]), torch.from_numpy(g["qry"]))
    for use_pca, key in ((True, "ranks_pca"), (False, "ranks_raw")):
        full = fmpnp.compute_ranks(ref, qry, use_pca)
        assert full.is_cuda and np.array_equal(full.cpu().numpy(), g[key]), key
        for top_n in (10, 30):
            ranks = fmpnp.compute_ranks(ref, qry, use_pca, top_n=top_n)  # (the kernel's path)
            assert ranks.is_cuda and np.array_equal(ranks.cpu().numpy(), g[key][:top_n]), (key, top_n)
    rp, qp = fmpnp.learn_and_apply_pca(ref, qry, ndim=int(g["ndim"]))
    assert rp.is_cuda
    scores = (rp @ qp.T).cpu().numpy()
    assert float(np.abs(scores - g["scores64"]).max()) <= 4.0 * float(g["e_ref_scores"])
    assert np.array_equal(np.argsort(-scores, axis=0), g["ranks_pca16"])
