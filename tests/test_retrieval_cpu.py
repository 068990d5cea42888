"""The retrieval stage's CPU twins (fmpnp_netvlad_pool_cpu, fmpnp_rank_topn_cpu) and its torch plumbing against
the goldens recorded from the reference's NetVLAD, learn_and_apply_pca and compute_ranks, within the
reference's own fp32 error; batch-, stride- and thread-independence under ==, the shared exponential's
recorded accuracy, the module interface, the ranking order and the argument errors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import fmpnp
from fmpnp import _lib

import retrieval_cases as rc

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "featuremetric-pnp_amd")


@pytest.mark.parametrize("name", rc.pool_golden_cases())
def test_twin_within_the_references_own_error(name):
    """|twin - fp64| <= 4 e_ref + 2^-23 max |fp64|, e_ref = max |reference fp32 - reference fp64| from the golden."""
    g = rc.golden_pool(name)
    got = fmpnp.netvlad_pool_cpu(torch.from_numpy(g["x"]), torch.from_numpy(g["weight"]),
                                 torch.from_numpy(g["centroids"]))
    assert got.dtype == torch.float32 and tuple(got.shape) == g["v64"].shape
    assert bool(torch.isfinite(got).all())
    err = float(np.abs(got.double().numpy() - g["v64"]).max())
    bound = rc.tolerance(g["e_ref"], g["v64"])
    print(f"{name}: twin error {err:.3g}, e_ref {float(g['e_ref']):.3g}, bound {bound:.3g}")
    assert err <= bound, (name, err, float(g["e_ref"]), bound)


@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("name", rc.ALL)
def test_twin_against_the_restatement(name, normalize):
    """The same form of bound on every shape, e_ref taken from the restatement's own fp32 run."""
    x, weight, centroids = rc.inputs(name)
    got = rc.twin(name, normalize)
    r32, r64 = (rc.ref(x, weight, centroids, dt, normalize) for dt in (torch.float32, torch.float64))
    e_ref = float((r32.double() - r64).abs().max())
    err, bound = float((got.double() - r64).abs().max()), rc.tolerance(e_ref, r64.numpy())
    print(f"{name} normalize={normalize}: twin error {err:.3g}, e_ref {e_ref:.3g}, bound {bound:.3g}")
    assert bool(torch.isfinite(got).all()), name
    assert err <= bound, (name, err, e_ref, bound)


def test_zero_position_and_zero_image_are_finite_unit_descriptors():
    got = rc.twin("zeros").double()
    assert bool(torch.isfinite(got).all())
    assert float(((got * got).sum(dim=1) - 1.0).abs().max()) < 1e-6


def test_large_logits_do_not_overflow():
    x, weight, centroids = rc.inputs("alpha")
    logits = torch.einsum("kc,ncp->nkp", weight.reshape(8, 32).double(),
                          torch.nn.functional.normalize(x.double(), dim=1).flatten(2))
    assert float(logits.abs().max()) > 200.0
    assert bool(torch.isfinite(rc.twin("alpha")).all())


@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("name", rc.ALL)
def test_batch_items_are_independent(name, normalize):
    """Each image of a batch of 3 has the bits it has alone, as a strided batch slice too."""
    x, weight, centroids = rc.inputs(name, 3)
    whole = rc.twin(name, normalize, 3)
    sliced = fmpnp.netvlad_pool_cpu(rc.strided(x), weight, centroids, normalize)
    assert torch.equal(sliced, whole), name
    for b in range(3):
        alone = fmpnp.netvlad_pool_cpu(x[b:b + 1], weight, centroids, normalize)
        assert torch.equal(alone[0], whole[b]), (name, b)


@pytest.mark.parametrize("name", ["ragged", "segments", "zeros"])
def test_thread_count_does_not_matter(name):
    x, weight, centroids = rc.inputs(name, 3)
    for n in (1, 2, 5):
        assert torch.equal(fmpnp.netvlad_pool_cpu(x, weight, centroids, n_threads=n), rc.twin(name, True, 3))


def test_out_view():
    x, weight, centroids = rc.inputs("small", 3)
    want = rc.twin("small", True, 3)
    buf, view = rc.view_out(*want.shape)
    before = buf.clone()
    got = fmpnp.netvlad_pool_cpu(x, weight, centroids, out=view)
    assert got.data_ptr() == view.data_ptr() and torch.equal(view, want)
    view.fill_(-7.0)
    assert torch.equal(buf, before)


def test_exp_accuracy_is_the_recorded_one():
    """The host program sweeps the shared exponential against libm over [-104, 0] (every 64th float here; every
    float gave the recorded value); include/fmpnp.h records the maximum in ulp."""
    with open(os.path.join(PKG, "..", "include", "fmpnp.h")) as f:
        recorded = float(re.search(r"#define FMPNP_NETVLAD_EXP_MAX_ULP ([0-9.]+)f", f.read()).group(1))
    assert recorded == _lib.NETVLAD_EXP_MAX_ULP == 1.011
    out = subprocess.run([os.path.join(PKG, "build", "test_retrieval_cpu"), "exp", "64"], check=True,
                         capture_output=True, text=True).stdout
    seen = float(re.search(r"exp_max_ulp=([0-9.]+)", out).group(1))
    print(out.strip())
    assert 0.5 < seen <= recorded


def test_host_program_passes():
    """csrc/test_retrieval_cpu.cpp's own checks (the build `make retrieval-sanitize` runs under ASan + UBSan)."""
    run = subprocess.run([os.path.join(PKG, "build", "test_retrieval_cpu")], capture_output=True, text=True)
    assert run.returncode == 0 and "all ok" in run.stdout, run.stdout[-2000:]


def test_host_plumbing_program_passes():
    """csrc/test_host_parallel.cpp: the work dealing and the fmaf chains of csrc/fmpnp_host.h, which every twin
    here runs on (the build `make host-sanitize` runs under ASan + UBSan and under the thread sanitizer)."""
    run = subprocess.run([os.path.join(PKG, "build", "test_host_parallel")], capture_output=True, text=True)
    assert run.returncode == 0 and "all ok" in run.stdout, run.stdout[-2000:]


def test_module_interface_is_the_references():
    g = rc.golden_pool("small")
    net = fmpnp.NetVLAD(num_clusters=8, dim=32)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()] == g["shapes"].tolist()
    net.init_params(g["clsts"].copy(), g["train"].copy())
    assert net.alpha == float(g["alpha"])
    assert np.array_equal(net.conv.weight.detach().numpy(), g["weight"])
    assert np.array_equal(net.centroids.detach().numpy(), g["centroids"])
    fresh = fmpnp.NetVLAD(num_clusters=8, dim=32)
    fresh.load_state_dict({"conv.weight": torch.from_numpy(g["weight"]), "centroids": torch.from_numpy(g["centroids"])})
    with pytest.raises(_lib.FmpnpError):
        net(torch.from_numpy(g["x"]))  # (no CPU fallback)


def test_pca_scores_and_ranks_equal_the_references():
    g = rc.golden("rank")
    ref, qry = torch.from_numpy(g["ref"]), torch.from_numpy(g["qry"])
    rp, qp = fmpnp.learn_and_apply_pca(ref, qry, ndim=int(g["ndim"]))
    assert rp.dtype == torch.float64 and tuple(rp.shape) == g["ref_pca64"].shape
    scores = (rp @ qp.T).numpy()
    err, bound = float(np.abs(scores - g["scores64"]).max()), 4.0 * float(g["e_ref_scores"])
    print(f"pca scores: error {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    assert np.array_equal(np.argsort(-scores, axis=0), g["ranks_pca16"])
    # the descriptors themselves up to one sign per component
    for got, want in ((rp.numpy(), g["ref_pca64"]), (qp.numpy(), g["qry_pca64"])):
        signs = np.sign((np.concatenate([rp.numpy(), qp.numpy()]) * np.concatenate([g["ref_pca64"], g["qry_pca64"]])).sum(0))
        assert float(np.abs(got * signs - want).max()) <= bound


def test_compute_ranks_equals_the_references():
    g = rc.golden("rank")
    ref, qry = torch.from_numpy(g["ref"]), torch.from_numpy(g["qry"])
    for use_pca, key in ((True, "ranks_pca"), (False, "ranks_raw")):
        ranks = fmpnp.compute_ranks(ref, qry, use_pca)
        assert tuple(ranks.shape) == g[key].shape and np.array_equal(ranks.numpy(), g[key]), key
        assert np.array_equal(fmpnp.compute_ranks(ref, qry, use_pca, top_n=10).numpy(), g[key][:10])
    with pytest.raises(TypeError):
        fmpnp.compute_ranks(ref, qry)
    fmpnp.config.configure(compute_ranks_use_pca=False)
    try:
        assert np.array_equal(fmpnp.compute_ranks(ref, qry).numpy(), g["ranks_raw"])
    finally:
        fmpnp.config.configure(compute_ranks_use_pca=None)


@pytest.mark.parametrize("n", [1, 10, 30, 40])
def test_rank_topn_cpu_equals_the_golden_ranks(n):
    g = rc.golden("rank")
    idx, top, scores = fmpnp.rank_topn_cpu(torch.from_numpy(g["ref"]), torch.from_numpy(g["qry"]), n, scores=True)
    assert np.array_equal(idx.numpy().T, g["ranks_raw"][:n])
    assert torch.equal(top, torch.gather(scores, 1, idx.long()))
    idx1, top1 = fmpnp.rank_topn_cpu(torch.from_numpy(g["ref"]), torch.from_numpy(g["qry"]), n, n_threads=3)
    assert torch.equal(idx1, idx) and torch.equal(top1, top)


def test_rank_order_ties_zeros_nan_and_all():
    """Equal scores: the lower index first; -0 counts as +0; NaN last; n = R ranks everything."""
    ref, qry = rc.rank_inputs("order")
    r = ref.shape[0]
    idx, top, scores = fmpnp.rank_topn_cpu(ref, qry, r, scores=True)
    s = scores.numpy()
    assert np.isnan(s[:, 7]).all() and (s[:, 3] == s[:, 11]).all() and (s[:, 5] == 0).all() and (s[:, 9] == 0).all()
    assert np.signbit(s[:, 5]).all() and not np.signbit(s[:, 9]).any()  # (-0 before +0 by index alone)
    assert np.array_equal(idx.numpy(), rc.expected_order(s))
    order = idx.numpy()
    for q in range(order.shape[0]):
        row = list(order[q])
        assert row[-1] == 7 and row.index(11) > row.index(3) and row.index(9) > row.index(5)
    for n in (1, 4, r - 1):
        assert np.array_equal(fmpnp.rank_topn_cpu(ref, qry, n)[0].numpy(), order[:, :n])
    wide_ref, wide_qry = rc.rank_inputs("wide")
    idx, top, scores = fmpnp.rank_topn_cpu(wide_ref, wide_qry, 64, scores=True)
    assert np.array_equal(idx.numpy(), rc.expected_order(scores.numpy())[:, :64])


def test_argument_errors():
    lib = _lib.load()
    x = np.zeros(64, np.float32)
    out = np.zeros(64, np.float32)
    idx = np.zeros(64, np.int32)
    p, o, ip = x.ctypes.data, out.ctypes.data, idx.ctypes.data

    def pool(B=1, C=2, P=3, sb=6, sc=3, w=p, K=2, ld_w=2, cent=p, ld_c=2, flag=1, out_=o, ld_out=4, nt=1, x_=p):
        return lib.fmpnp_netvlad_pool_cpu(x_, B, C, P, sb, sc, w, K, ld_w, cent, ld_c, flag, out_, ld_out, nt)

    assert pool() == 0
    assert pool(B=0, x_=None) == 0
    for bad in (dict(B=-1), dict(K=0), dict(C=0), dict(P=0), dict(sc=2), dict(sb=-1), dict(ld_w=1), dict(ld_c=1),
                dict(ld_out=3), dict(flag=2), dict(flag=-1), dict(w=None), dict(cent=None), dict(out_=None),
                dict(x_=None), dict(nt=-1)):
        assert pool(**bad) == _lib.EINVAL, bad
    assert pool(P=1 << 24, sc=1 << 24, sb=1 << 25) == _lib.ETOOBIG
    assert pool(K=1 << 16, C=1 << 15, ld_w=1 << 15, ld_c=1 << 15, ld_out=1 << 31) == _lib.ETOOBIG
    assert lib.fmpnp_netvlad_workspace_size(1, 64, 512, 4096) > 0
    assert lib.fmpnp_netvlad_workspace_size(1, 0, 512, 4096) == 0
    # a batch of any size needs no more than a bounded round of images
    assert lib.fmpnp_netvlad_workspace_size(4096, 64, 512, 4096) == lib.fmpnp_netvlad_workspace_size(512, 64, 512, 4096)

    def rank(Q=2, ld_q=3, D=3, R=5, ld_r=5, n=2, q_=p, r_=p, idx_=ip, top_=o, nt=1):
        return lib.fmpnp_rank_topn_cpu(q_, Q, ld_q, r_, D, R, ld_r, n, idx_, top_, None, nt)

    assert rank() == 0
    assert rank(Q=0, q_=None) == 0
    for bad in (dict(Q=-1), dict(D=0), dict(R=0), dict(ld_q=2), dict(ld_r=4), dict(n=0), dict(n=6), dict(q_=None),
                dict(r_=None), dict(idx_=None), dict(top_=None), dict(nt=-1)):
        assert rank(**bad) == _lib.EINVAL, bad
    cap = _lib.RANK_TOPN_CAP
    assert cap >= 64
    assert rank(R=cap + 8, ld_r=cap + 8, n=cap + 1) == _lib.ETOOBIG  # (validated before anything is read)
    with pytest.raises(ValueError):
        fmpnp.netvlad_pool_cpu(torch.zeros(1, 2, 3, 3), torch.zeros(4, 3), torch.zeros(4, 3))
    with pytest.raises(ValueError):
        fmpnp.netvlad_pool_cpu(torch.zeros(1, 2, 3, 3), torch.zeros(4, 2), torch.zeros(4, 2), out=torch.zeros(1, 7))
    with pytest.raises(ValueError):
        fmpnp.compute_ranks(torch.zeros(4, 3), torch.zeros(2, 3), False, top_n=5)
