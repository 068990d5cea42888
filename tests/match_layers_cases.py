"""Shared inputs of the layered-matching tests (test_match_layers_cpu.py, test_gpu_match_layers.py,
test_gpu_localize_layers.py): the layer sets of hypercolumn_cases chosen for the combine's branches and one set with
more than one correlation tile, seeded descriptors, the fp64 restatement (hypercolumn_cases.ref in float64, then a
matmul), the error bound of include/fmpnp.h ("layered matching") evaluated in fp64, and the CPU twin's result per
case, computed once and shared."""
import functools

import numpy as np
import torch

import fmpnp
import hypercolumn_cases as hcc
from match_cases import RATIO, top_ks

# the new set: 480 columns in the full-size layer (four 128-column correlation tiles, the last ragged), a coarse
# layer, and channel counts that are no multiple of the 32-deep k step
TILES2 = [(33, 24, 20), (40, 12, 10)]

# name -> (layer set, batch item, rows)
CASES = {
    "ragged3": ("ragged3", 0, 37), "ragged3_n1": ("ragged3", 0, 1), "ragged3_n129": ("ragged3", 0, 129),
    "single": ("single", 0, 37), "blocks": ("blocks", 0, 37), "line": ("line", 0, 37), "dot": ("dot", 0, 37),
    "down": ("down", 0, 37), "sized": ("sized", 0, 37), "vgg16x": ("vgg16x", 0, 64), "wide": ("wide", 0, 37),
    "batch3_item0": ("batch3", 0, 37), "batch3_item2": ("batch3", 2, 37), "views": ("views", 1, 37),
    "zero_texel": ("zero_texel", 0, 37), "nonfinite": ("nonfinite", 0, 37), "tiles2": ("tiles2", 0, 129),
}
FINITE = tuple(k for k in CASES if k not in ("zero_texel", "nonfinite"))
ALL = tuple(CASES)


@functools.lru_cache(maxsize=None)
def layer_set(name):
    """(feature maps (CPU float32 tensors, never modified), output size or None)."""
    if name == "tiles2":
        g = torch.Generator().manual_seed(20261)
        return [torch.randn(1, c, h, w, generator=g) for c, h, w in TILES2], None
    return hcc.inputs(name)


def layers(case):
    """(maps, size, item, rows) of a case."""
    name, item, n = CASES[case]
    maps, size = layer_set(name)
    return maps, size, item, n


def out_size(maps, size):
    return tuple(int(s) for s in (maps[0].shape[2:] if size is None else size))


def channels(maps):
    return sum(int(m.shape[1]) for m in maps)


@functools.lru_cache(maxsize=None)
def sparse(case):
    """Seeded Gaussian descriptors [rows, C] (read-only); row 0 is zero where there is more than one row: a row
    of one repeated score."""
    maps, _, _, n = layers(case)
    rng = np.random.default_rng(sum(ord(ch) for ch in case) + 977)
    d = rng.standard_normal((n, channels(maps))).astype(np.float32)
    if n > 1:
        d[0] = 0.0
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def ref64(case, normalize=True):
    """The fp64 restatement's dense operand [C, H * W] of the case's batch item (a numpy array)."""
    maps, size, item, _ = layers(case)
    hyper = hcc.ref([m[item:item + 1] for m in maps], torch.float64, size=size, normalize=normalize)
    return hyper[0].reshape(hyper.shape[1], -1).numpy()


def ref_scores(case, d, normalize=True):
    """The fp64 restatement: ref(maps, float64), then a matmul."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(d, np.float64) @ ref64(case, normalize)


U = 2.0 ** -24


def _g(k):
    return k * U / (1.0 - k * U)


def bound(case, d, normalize=True):
    """include/fmpnp.h, "layered matching", `bound`, evaluated in fp64 for descriptors d [N, C]: [N, H * W].
    (NaN / Inf where the operands are not finite or the norm is zero: the callers compare where it is finite.)"""
    maps, size, item, _ = layers(case)
    maps = [m[item:item + 1].double() for m in maps]
    h, w = out_size(maps, size)
    C, L = channels(maps), len(maps)
    a = np.abs(np.asarray(d, np.float64))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r_abs = hcc.ref([m.abs() for m in maps], torch.float64, size=(h, w), normalize=False)[0].reshape(C, -1).numpy()
        a_max = np.concatenate([m.abs().amax(dim=(2, 3))[0].numpy() for m in maps])
        w_l = np.concatenate([np.full(m.shape[1], 4.0 * U * (m.shape[2] + m.shape[3] - 2)) for m in maps])
        M = a @ r_abs
        G = (a * (w_l * a_max)).sum(axis=1, keepdims=True)
        e_t = _g(C + L + 5) * (M + G) + G
        if not normalize:
            return e_t
        n = np.sqrt((ref64(case, normalize=False) ** 2).sum(axis=0))
        dn = np.sqrt(((_g(5) * r_abs + (w_l * a_max)[:, None]) ** 2).sum(axis=0)) + U * n
        rho = dn / n
        e = (e_t + M * rho) / (n * (1.0 - rho))
        return e + U * (M / n + e)


def own_texel_descriptors(case, seed, noise=0.05):
    """The agreement test's descriptors: each row a texel of the query's own (fp64, normalised) hypercolumn plus
    seeded Gaussian noise, as float32 [rows, C]; the texels are drawn without replacement where the map has enough."""
    maps, _, _, n = layers(case)
    dense = ref64(case)
    rng = np.random.default_rng(seed)
    wh = dense.shape[1]
    cols = rng.permutation(wh)[:n] if wh >= n else rng.integers(0, wh, n)
    d = dense[:, cols].T + noise / np.sqrt(dense.shape[0]) * rng.standard_normal((n, dense.shape[0]))
    return np.ascontiguousarray(d.astype(np.float32))


@functools.lru_cache(maxsize=None)
def twin(case, top_k, normalize=True):
    """The CPU twin's result on (layers(case), sparse(case)), computed once and shared (scores only at the first
    top_k of the map)."""
    maps, size, item, _ = layers(case)
    h, w = out_size(maps, size)
    return fmpnp.exhaustive_match_layers_cpu(sparse(case), maps, top_k, RATIO, size=size, item=item, normalize=normalize,
                                             scores=(top_k == top_ks(h * w)[0]))


def case_top_ks(case):
    maps, size, _, _ = layers(case)
    h, w = out_size(maps, size)
    return top_ks(h * w)


def int_layers(shapes, seed, batch=1):
    """Small-integer layers (values in -2 .. 2 with many zeros): every product, chain and dyadic resize is exact."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(-2, 3, (batch, c, h, w), generator=g).float() for c, h, w in shapes]
