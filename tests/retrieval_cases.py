"""Shared inputs of the retrieval tests (test_retrieval_cpu.py, test_gpu_retrieval.py): the goldens recorded
from the reference's own NetVLAD, PCA and compute_ranks (tests/golden/gen_golden_retrieval.py), the smallest
pooling shapes that reach each branch of the kernels and their CPU twin, the PyTorch restatement of
netvlad.py:45-70 and the tolerance derived from the reference's own fp32 error.  Every input is seeded; the
twin's result per case is computed once and shared."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

import fmpnp
from fmpnp import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEG = _lib.NETVLAD_SEGMENT

# name -> (batch, K, C, h, w, scale of the logits); every shape also runs with batch 3, without the input
# normalisation and as strided batch slices (the tests' parameters)
SHAPES = {
    "small": (1, 8, 32, 5, 7, 30.0),
    "ragged": (1, 5, 24, 3, 5, 30.0),            # nothing is a multiple of a tile
    "production": (1, 64, 512, 9, 11, 290.0),    # the production K and C; alpha as init_params gives it
    "segments": (1, 6, 20, 11, 47, 30.0),        # P = 517 = two segments and five positions
    "clusters70": (1, 70, 130, 5, 8, 30.0),      # a second round of 64 clusters and a second channel tile
    "zeros": (2, 8, 32, 5, 7, 30.0),             # an all-zero position (image 0) and an all-zero image (image 1)
    "alpha": (1, 8, 32, 5, 7, 600.0),            # logits beyond +-200
}
ALL = tuple(SHAPES)
assert SHAPES["segments"][3] * SHAPES["segments"][4] == 2 * SEG + 5


def _gen(name):
    return torch.Generator().manual_seed(sum(ord(ch) for ch in name) + 20260)


@functools.lru_cache(maxsize=None)
def inputs(name, batch=None):
    """(x [B, C, h, w], weight [K, C, 1, 1], centroids [K, C]): CPU float32 tensors, never modified.  The
    activations are heavy-tailed and non-negative; the weight rows are unit vectors times the logit scale."""
    b, k, c, h, w, scale = SHAPES[name]
    b = b if batch is None else batch
    g = _gen(name)
    x = torch.randn(b, c, h, w, generator=g).clamp_min(0.0) ** 3
    weight = F.normalize(torch.randn(k, c, generator=g), dim=1) * scale
    centroids = torch.randn(k, c, generator=g)
    if name == "zeros":
        x[0, :, 1, 2] = 0.0
        x[b - 1] = 0.0
    return x, weight.reshape(k, c, 1, 1), centroids


def ref(x, weight, centroids, dtype, normalize_input=True):
    """netvlad.py:45-70 restated without its loop over the clusters (residuals summed = a . x^ - sum(a) c), in
    `dtype`, on x's device."""
    x, centroids = x.to(dtype), centroids.to(dtype)
    w = weight.to(dtype).reshape(weight.shape[0], -1)
    if normalize_input:
        x = F.normalize(x, p=2, dim=1)
    xf = x.flatten(2)
    a = F.softmax(torch.einsum("kc,ncp->nkp", w, xf), dim=1)
    vlad = torch.einsum("nkp,ncp->nkc", a, xf) - a.sum(dim=-1)[..., None] * centroids[None]
    vlad = F.normalize(vlad, p=2, dim=2).flatten(1)
    return F.normalize(vlad, p=2, dim=1)


def tolerance(e_ref, ref64):
    """A result must lie within 4 e_ref + 2^-23 max |ref(fp64)| of ref(fp64): e_ref is the reference's own fp32
    error (the contract makes the same number of fp32 roundings in another order: the hypercolumn tests'
    margin), the floor one fp32 rounding at the largest magnitude."""
    return 4.0 * float(e_ref) + 2.0 ** -23 * float(np.abs(np.asarray(ref64)).max())


@functools.lru_cache(maxsize=None)
def twin(name, normalize_input=True, batch=None):
    """The CPU twin's result of a case (computed once; read-only)."""
    x, weight, centroids = inputs(name, batch)
    return fmpnp.netvlad_pool_cpu(x, weight, centroids, normalize_input)


def strided(x, device="cpu"):
    """x as batch slices of a wider tensor: every second image, a channel offset, padded channel rows (P + 3
    elements apart); the filler is NaN, so a read outside the view shows."""
    b, c, h, w = x.shape
    big = torch.full((2 * b, c + 2, h * w + 3), float("nan"), device=device)
    view = big[::2, 1:c + 1, :h * w]
    view.copy_(x.flatten(2).to(device))
    assert not view.is_contiguous() and view.stride(2) == 1
    return view


def view_out(batch, width, device="cpu", fill=-7.0):
    """(buffer, view): a [B, width] output view one float into a larger buffer with 5 unused floats per row."""
    buf = torch.full((1 + batch * (width + 5) + 2,), fill, dtype=torch.float32, device=device)
    return buf, buf[1:1 + batch * (width + 5)].view(batch, width + 5)[:, :width]


@functools.lru_cache(maxsize=None)
def golden(which):
    return np.load(os.path.join(GOLDEN, f"retrieval_{which}.npz"))


def golden_pool(name):
    g = golden("pool")
    return {k: g[f"{name}_{k}"] for k in ("x", "weight", "centroids", "v32", "v64", "e_ref", "alpha", "clsts", "train",
                                          "keys", "shapes")}


def pool_golden_cases():
    return [str(n) for n in golden("pool")["cases"]]


@functools.lru_cache(maxsize=None)
def rank_inputs(name):
    """(ref [R, D], qry [Q, D]) CPU float32 for the order cases: scores with ties, zeros of both signs and NaN."""
    g = _gen(name)
    if name == "order":
        # integer-valued descriptors: the scores are exact, so equal scores are equal bits.  References 3 and 11
        # are copies (a tie in every row), reference 5 scores -0 against every query (its one product underflows
        # from below) and reference 9 scores +0, reference 7 is NaN.
        ref, qry = torch.randint(-3, 4, (17, 6), generator=g).float(), torch.randint(-3, 4, (5, 6), generator=g).float()
        ref[:, 5], qry[:, 5] = 0.0, 1e-30
        ref[11] = ref[3]
        ref[5] = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, -1e-30])
        ref[9] = 0.0
        ref[7, 2] = float("nan")
        return ref, qry
    if name == "wide":
        # R = 1500 > one pass of the selection's threads, D = 70: several key bytes decide
        return F.normalize(torch.randn(1500, 70, generator=g), dim=1), F.normalize(torch.randn(9, 70, generator=g), dim=1)
    raise KeyError(name)


def expected_order(scores):
    """The contract's order on a [Q, R] score map, by a stable sort: descending, -0 = +0, NaN last, equal scores
    by ascending index (numpy's argsort(-scores, kind="stable") is that order)."""
    return np.argsort(-(np.asarray(scores, dtype=np.float64) + 0.0), axis=1, kind="stable")


def same_floats(a, b):
    """Equal under == with NaNs at the same positions."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and bool((na == nb).all()) and bool((a[~na] == b[~nb]).all())
