"""Retrieval on the GPU: which reference images a query is matched against.

The reference's stage in three pieces -- NetVLAD.forward (s2dhm/network/netvlad.py:45-70) per image through
ImageRetrievalModel.compute_embedding (network.py:88-108), learn_and_apply_pca (image_retrieval/pca.py) and
compute_ranks' scores and argsort (image_retrieval/rank_images.py:81-84) -- with the pooling and the top-n
ranking in libfmpnp (fmpnp_netvlad_pool, fmpnp_rank_topn; include/fmpnp.h states the numeric contract) and
the PCA as torch plumbing in fp64.

NetVLAD is the reference's module (same parameters, same init_params, its checkpoint keys load) whose forward
runs the kernel; netvlad_pool is the functional form and netvlad_pool_cpu / rank_topn_cpu are the CPU twins
(bit-identical results; explicit entry points, never fallbacks).
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib, config


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _pool_operands(x, weight, centroids, out, device_kind):
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.device.type != device_kind or x.dim() not in (3, 4):
        raise ValueError(f"x must be a float32 {device_kind} tensor [N, C, h, w] or [N, C, P]")
    x = x.detach()
    if x.dim() == 4:  # (positions must be contiguous; the batch and channel strides are free)
        if x.stride(3) != 1 or x.stride(2) != x.shape[3]:
            x = x.contiguous()
        x = x.flatten(2)
    batch, chans, pos = (int(s) for s in x.shape)
    if chans < 1 or pos < 1:
        raise ValueError(f"empty feature map {tuple(x.shape)}")
    if (pos > 1 and x.stride(2) != 1) or (chans > 1 and x.stride(1) < pos) or (batch > 1 and x.stride(0) < 0):
        x = x.contiguous()
    sb = int(x.stride(0)) if batch > 1 else chans * pos
    sc = int(x.stride(1)) if chans > 1 else pos
    weight = weight.detach().reshape(weight.shape[0], -1)
    centroids = centroids.detach()
    for name, t in (("weight", weight), ("centroids", centroids)):
        if t.dtype != torch.float32 or t.device != x.device or t.dim() != 2 or t.shape[1] != chans:
            raise ValueError(f"{name} must be float32 [K, {chans}] on {x.device}")
    if weight.shape[0] != centroids.shape[0] or weight.shape[0] < 1:
        raise ValueError("weight and centroids must have the same number of clusters")
    weight, centroids = weight.contiguous(), centroids.contiguous()
    clusters = int(weight.shape[0])
    shape = (batch, clusters * chans)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif (not torch.is_tensor(out) or tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != x.device
          or (shape[1] > 1 and out.stride(1) != 1) or (batch > 1 and out.stride(0) < shape[1])):
        raise ValueError(f"out must be a float32 tensor {shape} on {x.device} with dense rows")
    ld_out = int(out.stride(0)) if batch > 1 else shape[1]
    return x, (batch, chans, pos, sb, sc), weight, centroids, clusters, out, ld_out


def netvlad_pool(x, weight, centroids, normalize_input=True, out=None, stream=None):
    """NetVLAD.forward on the GPU.  x: float32 CUDA [N, C, h, w] (or [N, C, P]; any batch and channel strides,
    so batch slices and channel-padded maps are read in place), weight: conv.weight [K, C, 1, 1] or [K, C],
    centroids [K, C] -> the [N, K * C] float32 descriptors.  out: a tensor of that shape to write into (rows
    may be padded).  Asynchronous on `stream` (default: the device's current stream)."""
    x, (batch, chans, pos, sb, sc), weight, centroids, clusters, out, ld_out = _pool_operands(
        x, weight, centroids, out, "cuda")
    if batch == 0:
        return out
    device = x.device
    _lib.require_device(device)
    lib = _lib.load()
    s = torch.cuda.current_stream(device) if stream is None else stream
    with torch.cuda.device(device), torch.cuda.stream(s):
        nbytes = lib.fmpnp_netvlad_workspace_size(batch, clusters, chans, pos)
        ws = torch.empty(max(int(nbytes), 4) // 4 + 1, dtype=torch.float32, device=device)
        rc = lib.fmpnp_netvlad_pool_async(_vp(x), batch, chans, pos, sb, sc, _vp(weight), clusters, chans,
                                          _vp(centroids), chans, int(bool(normalize_input)), _vp(out), ld_out,
                                          _vp(ws), ws.numel() * 4, ctypes.c_void_p(s.cuda_stream))
    _lib.check(rc, "fmpnp_netvlad_pool_async")
    for t in (x, weight, centroids, out, ws):
        t.record_stream(s)  # (the caching allocator must not hand the memory on before the kernels have run)
    return out


def netvlad_pool_cpu(x, weight, centroids, normalize_input=True, out=None, n_threads=0):
    """The CPU twin (fmpnp_netvlad_pool_cpu) on float32 CPU tensors: netvlad_pool's result bit for bit."""
    x, (batch, chans, pos, sb, sc), weight, centroids, clusters, out, ld_out = _pool_operands(
        x, weight, centroids, out, "cpu")
    rc = _lib.load().fmpnp_netvlad_pool_cpu(_vp(x), batch, chans, pos, sb, sc, _vp(weight), clusters, chans,
                                            _vp(centroids), chans, int(bool(normalize_input)), _vp(out), ld_out,
                                            int(n_threads))
    _lib.check(rc, "fmpnp_netvlad_pool_cpu")
    return out


class NetVLAD(nn.Module):
    """The reference's NetVLAD layer (s2dhm/network/netvlad.py): conv.weight [K, C, 1, 1] and centroids [K, C],
    init_params as there, so its checkpoints load.  forward takes a CUDA [N, C, h, w] map and runs the kernel
    (inference only: no autograd through it); there is no CPU fallback -- netvlad_pool_cpu is the explicit
    twin."""

    def __init__(self, num_clusters=64, dim=128, normalize_input=True):
        super().__init__()
        self.num_clusters = num_clusters
        self.dim = dim
        self.alpha = 0
        self.normalize_input = normalize_input
        self.conv = nn.Conv2d(dim, num_clusters, kernel_size=(1, 1), bias=False)
        self.centroids = nn.Parameter(torch.rand(num_clusters, dim))

    def init_params(self, clsts, traindescs):
        clsts_assign = clsts / np.linalg.norm(clsts, axis=1, keepdims=True)
        dots = np.dot(clsts_assign, traindescs.T)
        dots.sort(0)
        dots = dots[::-1, :]  # sort, descending
        self.alpha = (-np.log(0.01) / np.mean(dots[0, :] - dots[1, :])).item()
        self.centroids = nn.Parameter(torch.from_numpy(clsts))
        self.conv.weight = nn.Parameter(torch.from_numpy(self.alpha * clsts_assign).unsqueeze(2).unsqueeze(3))
        self.conv.bias = None

    def forward(self, x):
        if not x.is_cuda:
            raise _lib.FmpnpError("NetVLAD.forward runs on the GPU (no CPU fallback); netvlad_pool_cpu is the twin")
        return netvlad_pool(x.float(), self.conv.weight.float(), self.centroids.float(), self.normalize_input)


def compute_embedding(encoder, pool, images, batch=16):
    """ImageRetrievalModel.compute_embedding (network.py:88-108) on tensors: images is a [n, 3, H, W] tensor or a
    sequence of [3, H, W] tensors (sizes may differ) -> the [n, K * C] descriptors on the encoder's device, row i
    for image i.  Consecutive images of equal size go through the encoder and one pooling call together, up to
    `batch` at a time; the descriptors do not depend on the grouping beyond the encoder's own batching."""
    items = list(images) if not torch.is_tensor(images) else list(images.unbind(0) if images.dim() == 4 else [images])
    p = next(encoder.parameters(), None)
    device = p.device if p is not None else torch.device("cuda")
    out = None
    with torch.no_grad():
        i = 0
        while i < len(items):
            j = i + 1
            while j < len(items) and j - i < int(batch) and items[j].shape == items[i].shape:
                j += 1
            group = torch.stack([t.squeeze(0) if t.dim() == 4 else t for t in items[i:j]])
            desc = pool(encoder(group.to(device=device, dtype=torch.float32)))
            if out is None:
                out = torch.empty((len(items), desc.shape[1]), dtype=torch.float32, device=desc.device)
            out[i:j] = desc
            i = j
    if out is None:
        raise ValueError("compute_embedding: no images")
    return out


def _normalize(a):
    return a / torch.linalg.norm(a, dim=-1, keepdim=True)


def learn_and_apply_pca(ref_desc, qry_desc, ndim=1024):
    """image_retrieval/pca.py in torch, fp64, on the descriptors' device: normalise, centre on the reference
    mean, the first min(ndim, R) right singular vectors of the centred references (sklearn's full solver with
    its svd_flip sign convention), project both sets, normalise.  Returns fp64 tensors.  (At production size
    sklearn takes its randomised solver, which has no fixed seed: parity there is with the exact PCA only.)"""
    ref = _normalize(torch.as_tensor(ref_desc).to(torch.float64))
    qry = _normalize(torch.as_tensor(qry_desc).to(device=ref.device, dtype=torch.float64))
    n = min(int(ndim), ref.shape[0])
    mean = ref.mean(dim=0, keepdim=True)
    _, _, vt = torch.linalg.svd(ref - mean, full_matrices=False)
    # sklearn's svd_flip(u_based_decision=False): the entry of largest magnitude in each component is positive
    pick = vt.abs().argmax(dim=1)
    signs = torch.sign(vt[torch.arange(vt.shape[0], device=vt.device), pick])
    signs[signs == 0] = 1.0
    comp = (vt * signs[:, None])[:n]
    return _normalize((ref - mean) @ comp.T), _normalize((qry - mean) @ comp.T)


def _rank_rows(t, name, kind):
    if not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.float32 or t.device.type != kind:
        raise ValueError(f"{name} must be a 2-D float32 {kind} tensor")
    return t.detach().contiguous()


def rank_topn(ref_desc, qry_desc, n, scores=False, stream=None):
    """fmpnp_rank_topn on CUDA tensors: ref_desc [R, D], qry_desc [Q, D] (fp32) -> (idx int32 [Q, n], top
    float32 [Q, n]) CUDA tensors: the n best references of every query in descending score order (equal scores:
    the lower index first; NaN last), plus the [Q, R] score map when asked.  Asynchronous on `stream`."""
    ref = _rank_rows(ref_desc, "ref_desc", "cuda")
    qry = _rank_rows(qry_desc, "qry_desc", "cuda")
    if ref.shape[1] != qry.shape[1] or ref.device != qry.device:
        raise ValueError("ref_desc and qry_desc must share the descriptor size and the device")
    (r, d), q = ref.shape, qry.shape[0]
    device = ref.device
    _lib.require_device(device)
    lib = _lib.load()
    s = torch.cuda.current_stream(device) if stream is None else stream
    with torch.cuda.device(device), torch.cuda.stream(s):
        ref_t = ref.t().contiguous()  # the correlation's `dense` operand: transposed once
        idx = torch.empty((q, int(n)), dtype=torch.int32, device=device)
        top = torch.empty((q, int(n)), dtype=torch.float32, device=device)
        if scores:
            smap, ws, nbytes = torch.empty((q, r), dtype=torch.float32, device=device), None, 0
        else:
            nbytes = int(lib.fmpnp_match_workspace_size(q, r))
            smap, ws = None, torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=device)
        rc = lib.fmpnp_rank_topn_async(_vp(qry), q, d, _vp(ref_t), d, r, r, int(n), _vp(idx), _vp(top),
                                       _vp(smap) if scores else None, _vp(ws) if ws is not None else None,
                                       ws.numel() * 4 if ws is not None else 0, ctypes.c_void_p(s.cuda_stream))
    _lib.check(rc, "fmpnp_rank_topn_async")
    for t in (ref, qry, ref_t, idx, top, smap, ws):
        if t is not None:
            t.record_stream(s)
    return (idx, top, smap) if scores else (idx, top)


def rank_topn_cpu(ref_desc, qry_desc, n, scores=False, n_threads=0):
    """The CPU twin (fmpnp_rank_topn_cpu) on float32 CPU tensors: rank_topn's results bit for bit."""
    ref = _rank_rows(ref_desc, "ref_desc", "cpu")
    qry = _rank_rows(qry_desc, "qry_desc", "cpu")
    if ref.shape[1] != qry.shape[1]:
        raise ValueError("ref_desc and qry_desc must share the descriptor size")
    (r, d), q = ref.shape, qry.shape[0]
    ref_t = ref.t().contiguous()
    idx = torch.empty((q, int(n)), dtype=torch.int32)
    top = torch.empty((q, int(n)), dtype=torch.float32)
    smap = torch.empty((q, r), dtype=torch.float32) if scores else None
    rc = _lib.load().fmpnp_rank_topn_cpu(_vp(qry), q, d, _vp(ref_t), d, r, r, int(n), _vp(idx), _vp(top),
                                         _vp(smap) if scores else None, int(n_threads))
    _lib.check(rc, "fmpnp_rank_topn_cpu")
    return (idx, top, smap) if scores else (idx, top)


def compute_ranks(ref_desc, qry_desc, use_pca=None, top_n=None):
    """compute_ranks (rank_images.py:75-84) on descriptors: ranks [R or top_n, Q] (int64, on the descriptors'
    device), column q the references of query q in descending score order, as the reference returns.
    use_pca: learn_and_apply_pca first (None: fmpnp.config's compute_ranks_use_pca binding).  With top_n within
    FMPNP_RANK_TOPN_CAP and CUDA descriptors the kernel ranks (fp32 descriptors, exact fmaf-chain scores);
    otherwise a stable descending sort of the exact score map in the descriptors' precision."""
    if use_pca is None:
        use_pca = config.compute_ranks_kwargs()["use_pca"]
    if use_pca is None:
        raise TypeError("compute_ranks: use_pca is not bound (pass it, or "
                        "fmpnp.config.configure(compute_ranks_use_pca=...))")
    ref, qry = torch.as_tensor(ref_desc), torch.as_tensor(qry_desc)
    qry = qry.to(ref.device)
    if use_pca:
        ref, qry = learn_and_apply_pca(ref, qry)
    if top_n is not None and not 1 <= int(top_n) <= ref.shape[0]:
        raise ValueError(f"top_n must be in 1..{ref.shape[0]}")
    if top_n is not None and int(top_n) <= _lib.RANK_TOPN_CAP and ref.is_cuda:
        idx, _ = rank_topn(ref.float(), qry.float(), int(top_n))
        return idx.t().contiguous().long()
    scores = ref @ qry.to(ref.dtype).T
    ranks = torch.sort(-scores, dim=0, stable=True).indices
    return ranks if top_n is None else ranks[:int(top_n)]
