#!/usr/bin/env python3
"""Generate tests/golden/retrieval_*.npz from the reference's retrieval code.

TEST INFRASTRUCTURE ONLY, like gen_golden_match.py: it runs the *reference* s2dhm/network/netvlad.py,
s2dhm/image_retrieval/pca.py and s2dhm/image_retrieval/rank_images.py unmodified (read-only at
/root/reference) on small seeded inputs and records what they compute; it refuses to run where the reference
is absent.  Stand-ins are written into a temporary directory OUTSIDE the repository, ahead of the reference
on sys.path: a no-op `gin`, and empty `datasets.base_dataset` / `network.network` modules (rank_images.py
names them in annotations only); netvlad.py is loaded by path, since the stand-in shadows its package.
compute_ranks gets a stub dataset and a stub network whose compute_embedding returns the arrays.

retrieval_pool.npz: per case the activations, the weights from NetVLAD.init_params, the module's fp32 output,
its fp64 output (the same module and input in double) and e_ref = max |fp32 - fp64|; the module's
state_dict keys, shapes and alpha.
retrieval_rank.npz: descriptors, learn_and_apply_pca's outputs at ndim = 16 in fp32 and fp64 with the score
maps and e_ref_scores, and compute_ranks' ranks with and without PCA.  The generator asserts that in every
ranking case the fp64 gap between consecutive sorted scores of every column is >= 1e-4, so the tests compare
every rank with no exclusions.  The PCA cases stay at sizes where sklearn takes its full solver (the
randomised one it takes at production size has no fixed seed).

Run:  python tests/golden/gen_golden_retrieval.py
"""
import importlib.util
import os
import sys
import tempfile

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
S2DHM = os.path.join(REF, "s2dhm")

if not os.path.isfile(os.path.join(S2DHM, "network", "netvlad.py")):
    raise SystemExit("gen_golden_retrieval.py needs the reference at /root/reference; use the committed fixtures instead")


def _install_shims():
    d = tempfile.mkdtemp(prefix="fmpnp_refshims_")
    with open(os.path.join(d, "gin.py"), "w") as f:
        f.write(
            "def _deco(*a, **k):\n"
            "    if len(a) == 1 and callable(a[0]) and not k:\n"
            "        return a[0]\n"
            "    return lambda f: f\n"
            "configurable = _deco\n"
            "register = _deco\n")
    for pkg, mod, cls in (("datasets", "base_dataset", "BaseDataset"), ("network", "network", "ImageRetrievalModel")):
        os.makedirs(os.path.join(d, pkg))
        with open(os.path.join(d, pkg, "__init__.py"), "w") as f:
            f.write("# empty stand-in\n")
        with open(os.path.join(d, pkg, mod + ".py"), "w") as f:
            f.write(f"class {cls}:\n    pass\n")
    sys.path[:0] = [d, S2DHM]
    return d


TMP = _install_shims()

import torch  # noqa: E402

torch.set_num_threads(1)

_spec = importlib.util.spec_from_file_location("ref_netvlad", os.path.join(S2DHM, "network", "netvlad.py"))
ref_netvlad = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref_netvlad)  # s2dhm/network/netvlad.py
from image_retrieval import pca as ref_pca  # noqa: E402  s2dhm/image_retrieval/pca.py
from image_retrieval import rank_images as ref_rank  # noqa: E402  s2dhm/image_retrieval/rank_images.py

# name: (K, C, h, w, B, zero position, zero image)
POOL_CASES = {
    "small": (8, 32, 5, 7, 2, False, False),
    "ragged": (5, 24, 3, 5, 1, True, False),
    "segments": (16, 64, 11, 47, 1, True, False),   # P = 517: two segments of 256 and five positions
    "clusters64": (64, 128, 9, 11, 2, True, True),
}


def gen_pool():
    out = {}
    rng = np.random.default_rng(20260201)
    for name, (K, C, h, w, B, zero_pos, zero_img) in POOL_CASES.items():
        clsts = rng.standard_normal((K, C)).astype(np.float32)
        train = rng.standard_normal((300, C)).astype(np.float32)
        train /= np.linalg.norm(train, axis=1, keepdims=True)
        mod = ref_netvlad.NetVLAD(num_clusters=K, dim=C)
        mod.init_params(clsts, train)
        # heavy-tailed, non-negative (post-ReLU) activations
        x = (np.maximum(rng.standard_normal((B, C, h, w)), 0.0) ** 3).astype(np.float32)
        if zero_pos:
            x[0, :, 1, 2] = 0.0
        if zero_img:
            x[B - 1] = 0.0
        with torch.no_grad():
            v32 = mod(torch.from_numpy(x)).numpy().copy()
            v64 = mod.double()(torch.from_numpy(x).double()).numpy().copy()
        assert v32.dtype == np.float32 and v64.dtype == np.float64 and v32.shape == (B, K * C)
        assert np.isfinite(v32).all() and np.isfinite(v64).all(), name
        e_ref = float(np.abs(v32.astype(np.float64) - v64).max())
        sd = mod.float().state_dict()
        out[f"{name}_x"], out[f"{name}_weight"] = x, sd["conv.weight"].numpy().copy()
        out[f"{name}_centroids"], out[f"{name}_v32"], out[f"{name}_v64"] = sd["centroids"].numpy().copy(), v32, v64
        out[f"{name}_e_ref"], out[f"{name}_alpha"] = np.float64(e_ref), np.float64(mod.alpha)
        out[f"{name}_clsts"], out[f"{name}_train"] = clsts, train
        out[f"{name}_keys"] = np.array(list(sd.keys()))
        out[f"{name}_shapes"] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()])
        print(f"retrieval_pool {name}: alpha {mod.alpha:.1f}, max |v| {np.abs(v64).max():.3g}, e_ref {e_ref:.3g} "
              f"({e_ref / np.abs(v64).max() * 1e6:.2f} ppm)")
    out["cases"] = np.array(list(POOL_CASES))
    np.savez_compressed(os.path.join(HERE, "retrieval_pool.npz"), **out)


class _Dataset:
    def __init__(self, r, q):
        self.data = dict(name="golden", reference_image_names=[f"r{i}" for i in range(r)],
                         query_image_names=[f"q{i}" for i in range(q)])


class _Network:
    def __init__(self, ref, qry):
        self.ref, self.qry = ref, qry

    def compute_embedding(self, names):
        return (self.ref if names[0].startswith("r") else self.qry).copy()


def min_gap(scores64):
    srt = -np.sort(-scores64, axis=0)
    return float((srt[:-1] - srt[1:]).min())


def gen_rank():
    R, Q, D, NDIM = 40, 7, 96, 16
    for seed in range(20260301, 20260401):
        rng = np.random.default_rng(seed)
        base = rng.standard_normal((5, D))
        ref = (rng.standard_normal((R, 5)) @ base + 0.7 * rng.standard_normal((R, D))).astype(np.float32)
        qry = (ref[rng.choice(R, Q, replace=False)] + 0.5 * rng.standard_normal((Q, D))).astype(np.float32)
        ref /= np.linalg.norm(ref, axis=1, keepdims=True)
        qry /= np.linalg.norm(qry, axis=1, keepdims=True)
        r64, q64 = ref.astype(np.float64), qry.astype(np.float64)
        rp32, qp32 = ref_pca.learn_and_apply_pca(ref, qry, ndim=NDIM)
        rp64, qp64 = ref_pca.learn_and_apply_pca(r64, q64, ndim=NDIM)
        rf64, qf64 = ref_pca.learn_and_apply_pca(r64, q64)
        s32, s64 = np.dot(rp32, qp32.T), np.dot(rp64, qp64.T)
        gaps = dict(pca16=min_gap(s64), pca_full=min_gap(np.dot(rf64, qf64.T)), raw=min_gap(np.dot(r64, q64.T)))
        if min(gaps.values()) >= 1e-4:
            break
    else:
        raise SystemExit("no seed gave every ranking case a minimum gap of 1e-4")
    assert rp32.dtype == np.float32 and rp64.dtype == np.float64
    for tag, g in gaps.items():
        assert g >= 1e-4, (tag, g)
    ranks = {}
    for tag, use_pca in (("pca", True), ("raw", False)):
        path = os.path.join(TMP, f"ranks_{tag}", "golden.npz")
        ranks[tag] = ref_rank.compute_ranks(path, _Dataset(R, Q), _Network(ref, qry), use_pca)
        assert ranks[tag].shape == (R, Q)
    # the reference's own fp32 ranks are those of the fp64 evaluation (the gaps are far above its error)
    assert np.array_equal(ranks["raw"], np.argsort(-np.dot(r64, q64.T), axis=0))
    assert np.array_equal(ranks["pca"], np.argsort(-np.dot(rf64, qf64.T), axis=0))
    ranks16 = np.argsort(-s32, axis=0)
    assert np.array_equal(ranks16, np.argsort(-s64, axis=0))
    e_ref = float(np.abs(s32.astype(np.float64) - s64).max())
    print(f"retrieval_rank: seed {seed}, min gaps {gaps}, e_ref_scores {e_ref:.3g}")
    np.savez_compressed(os.path.join(HERE, "retrieval_rank.npz"), ref=ref, qry=qry, ndim=np.int64(NDIM),
                        ref_pca32=rp32, qry_pca32=qp32, ref_pca64=rp64, qry_pca64=qp64, scores32=s32, scores64=s64,
                        e_ref_scores=np.float64(e_ref), ranks_pca16=ranks16, ranks_pca=ranks["pca"],
                        ranks_raw=ranks["raw"], min_gap=np.float64(min(gaps.values())))


if __name__ == "__main__":
    gen_pool()
    gen_rank()
