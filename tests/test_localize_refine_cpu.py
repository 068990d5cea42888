"""The batched refinement stage without a GPU: fmpnp_localize_refine_prep_cpu, the CPU twin of the stage's prep and
gather kernels, on localize_cpu's records of the scenes mixed, tie, fallback_loses, fallback_wins and none, against
a numpy restatement (tests/localize_refine_cases.py).  (The twin's stand-alone sanitizer program is
csrc/test_localize_refine_cpu.cpp, `make localize-refine-sanitize`.)"""
import ctypes

import numpy as np
import pytest

import localize_cases as lc
import localize_refine_cases as rc
from fmpnp import _lib
from fmpnp import _localize as loc


def run_twin(plan, bufs, src, params, dtype=np.float32):
    """(probs, fref [rows, cstride] of dtype, flags), every output pre-filled with 0xA5."""
    fref = np.full(max(plan.out_rows, 1) * params.cstride * np.dtype(dtype).itemsize, rc.FILL, np.uint8).view(dtype)
    flags = np.full(max(plan.n_queries, 1), -1, np.int32)
    probs = loc.glue_refine_prep_cpu(plan, bufs, src, rc.query_maps(plan), params,
                                     _lib.F64 if dtype == np.float64 else _lib.F32, fref, flags)
    return probs, fref.reshape(-1, params.cstride), flags


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("levels", [(), tuple((a, b) for a, b, _, _ in rc.LEVELS)])
def test_prep_twin_against_numpy(levels, dtype):
    plan, bufs, locs = rc.picked()
    src, maps = rc.host_sources(plan, dtype)
    cs = lc.C + 4  # (padding channels beside the C = 32 the scenes have)
    params = rc.refine_params(cs, levels)
    probs, fref, flags = run_twin(plan, bufs, src, params, dtype)
    Q, n_res = plan.n_queries, len(levels) + 1 if levels else 1
    qm = rc.query_maps(plan)
    assert [l.kind for l in locs] == ["solved", "solved", "solved", "fallback", "none"]
    for qi, got in enumerate(locs):
        q = plan.qdesc[qi]
        o, cap = q.out_offset, q.out_cap
        n = 0 if got.prediction is None else len(got.prediction.points_3d)
        assert flags[qi] == 0
        for r in range(n_res):
            p = probs[r * Q + qi]
            assert p.N == n and p.Hf == lc.W and p.Wf == lc.H and p.cstride == cs and p.ld_ref == cs
            assert (p.c_begin, p.c_end) == ((0, lc.C) if not levels or r == 0 else levels[r - 1])
            assert p.im_width == lc.IMAGE[0] and p.im_height == lc.IMAGE[1] and not p.window
            assert p.feat == qm[qi].feat
            assert p.fref == fref.ctypes.data + o * cs * fref.itemsize and p.pts3d == bufs["b_pts3d"].ctypes.data + 24 * o
            assert list(p.K) == list(np.asarray(plan.refs[qi][-1]["intrinsics"], np.float64).reshape(-1))  # the LAST pair's
            if got.prediction is None:
                assert not any(p.R0) and not any(p.t0)
            else:
                m = np.asarray(got.prediction.matrix, np.float64)
                assert list(p.R0) == list(m[:3, :3].reshape(-1)) and list(p.t0) == list(m[:3, 3])
        if n:
            g = q.pair_begin + got.best
            want, bad = rc.reference_rows(maps[g], np.asarray(got.prediction.reference_inliers, np.float64))
            assert not bad.any()
            assert fref[o:o + n, :lc.C].tobytes() == want.astype(dtype).tobytes()
            assert (fref[o:o + n, lc.C:] == 0).all()                       # the padding channels are zero
        assert (fref[o + n:o + cap].view(np.uint8) == rc.FILL).all()      # rows past N are untouched
    # a fallback winner starts from the fallback pose
    fw = rc.NAMES.index("fallback_wins")
    m = plan.refs[fw][locs[fw].best]["fallback_pose"][1]
    assert list(probs[fw].R0) == list(m[:3, :3].reshape(-1)) and list(probs[fw].t0) == list(m[:3, 3])
    assert probs[rc.NAMES.index("none")].N == 0


def test_refine_intrinsics_last_against_best():
    plan, bufs, locs = rc.picked()
    src, _ = rc.host_sources(plan)
    fl = rc.NAMES.index("fallback_loses")
    refs = plan.refs[fl]
    assert not np.array_equal(refs[-1]["intrinsics"], refs[locs[fl].best]["intrinsics"])
    last, _, _ = run_twin(plan, bufs, src, rc.refine_params(intrinsics=_lib.LOC_K_LAST))
    best, _, _ = run_twin(plan, bufs, src, rc.refine_params(intrinsics=_lib.LOC_K_BEST))
    assert list(last[fl].K) == list(np.asarray(refs[-1]["intrinsics"], np.float64).reshape(-1))
    assert list(best[fl].K) == list(np.asarray(refs[locs[fl].best]["intrinsics"], np.float64).reshape(-1))
    assert list(last[fl].K) != list(best[fl].K)


def test_a_null_source_gives_no_rows():
    plan, bufs, locs = rc.picked()
    tie = rc.NAMES.index("tie")
    g = plan.qdesc[tie].pair_begin + locs[tie].best
    src, _ = rc.host_sources(plan, drop=(g,))
    probs, fref, flags = run_twin(plan, bufs, src, rc.refine_params())
    q = plan.qdesc[tie]
    assert probs[tie].N == 0 and flags[tie] == 0
    assert (fref[q.out_offset:q.out_offset + q.out_cap].view(np.uint8) == rc.FILL).all()
    assert probs[0].N == len(locs[0].prediction.points_3d) > 0  # the others keep theirs


@pytest.mark.parametrize("value", ["outside", "nan"])
def test_an_inlier_outside_its_map_flags_its_query_only(value):
    plan, bufs, locs = rc.picked()
    src, maps = rc.host_sources(plan)
    clean = run_twin(plan, bufs, src, rc.refine_params())
    tie = rc.NAMES.index("tie")
    o, n = plan.qdesc[tie].out_offset, len(locs[tie].prediction.points_3d)
    row = 7
    bufs["b_ref2d"].reshape(-1, 2)[o + row] = (lc.IMAGE[0] * 1.0, 10.0) if value == "outside" else (np.nan, 10.0)
    probs, fref, flags = run_twin(plan, bufs, src, rc.refine_params())
    assert flags[tie] == 1 and [int(f) for i, f in enumerate(flags) if i != tie] == [0] * (plan.n_queries - 1)
    assert (fref[o + row] == 0).all()                                          # that row is zeroed
    keep = np.ones(len(fref), bool)
    keep[o + row] = False
    assert fref[keep].tobytes() == clean[1][keep].tobytes()                    # every other row is untouched
    assert [p.N for p in probs] == [p.N for p in clean[0]]


def test_a_small_negative_coordinate_wraps():
    plan, bufs, locs = rc.picked()
    src, maps = rc.host_sources(plan)
    mixed = rc.NAMES.index("mixed")
    o = plan.qdesc[mixed].out_offset
    g = plan.qdesc[mixed].pair_begin + locs[mixed].best
    r2 = bufs["b_ref2d"].reshape(-1, 2)
    r2[o + 0] = (-5.0, 9.0)      # col = trunc(-1.25) = -1 -> H_ref - 1
    r2[o + 1] = (9.0, -64.0)     # row = trunc(-16.0) = -16 -> 0: the lowest index that still wraps
    r2[o + 2] = (-0.5, -3.9)     # trunc toward zero: (-0.125, -0.975) -> (0, 0), no wrap
    r2[o + 3] = (9.0, -64.1)     # row = trunc(-16.025) = -16 -> 0
    r2[o + 4] = (9.0, -68.0)     # row = -17: outside
    probs, fref, flags = run_twin(plan, bufs, src, rc.refine_params())
    m = maps[g]
    assert fref[o + 0].tobytes() == m[:, int(9.0 * 0.25), lc.W - 1].tobytes()
    assert fref[o + 1].tobytes() == m[:, 0, 2].tobytes() and fref[o + 3].tobytes() == m[:, 0, 2].tobytes()
    assert fref[o + 2].tobytes() == m[:, 0, 0].tobytes()
    assert (fref[o + 4] == 0).all() and flags[mixed] == 1
    want, bad = rc.reference_rows(m, r2[o:o + 5])
    assert list(bad) == [False, False, False, False, True]
    assert fref[o:o + 5].tobytes() == want.astype(np.float32).tobytes()


def test_host_validation_and_exports():
    L = _lib.load()
    assert {"fmpnp_localize_refine_workspace_size", "fmpnp_localize_refine_async", "fmpnp_localize_refined",
            "fmpnp_localize_refine_prep_cpu"} <= set(_lib.EXPORTS)
    assert all(hasattr(L, n) for n in _lib.EXPORTS) and L.fmpnp_abi_version() == 4
    plan, bufs, _ = rc.picked()
    src, _ = rc.host_sources(plan)
    fref, flags = np.zeros(plan.out_rows * lc.C, np.float32), np.zeros(plan.n_queries, np.int32)
    for bad in (dict(cstride=lc.C - 1), dict(levels=((0, lc.C + 1),)), dict(levels=((8, 8),)), dict(intrinsics=2)):
        with pytest.raises(_lib.FmpnpError, match="EINVAL"):
            loc.glue_refine_prep_cpu(plan, bufs, src, rc.query_maps(plan), rc.refine_params(**bad), _lib.F32, fref, flags)
    with pytest.raises(_lib.FmpnpError, match="EINVAL"):
        loc.glue_refine_prep_cpu(plan, bufs, src, rc.query_maps(plan), rc.refine_params(), 7, fref, flags)
    # the HIP entry points validate on the host before they touch the device
    prm, opt = rc.refine_params(), _lib.Options()
    opt.layout = _lib.LAYOUT_F
    assert L.fmpnp_localize_refine_workspace_size(plan.qdesc, plan.n_queries, rc.query_maps(plan), ctypes.byref(prm),
                                                  ctypes.byref(opt)) == 0

