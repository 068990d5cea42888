#!/usr/bin/env python3
"""Generate tests/golden/superpoint_*.npz from the reference's SuperPoint baseline.

TEST INFRASTRUCTURE ONLY, like gen_golden_match.py: it runs the *reference*
third_party/SuperPointPretrainedNetwork/demo_superpoint.py (SuperPointFrontend.run and nms_fast),
pose_prediction/keypoint_association.py (fast_keypoint_matching, fast_closest_points) and
pose_prediction/superpoint_predictor.py (_assemble_matches) unmodified (read-only at /root/reference), on CPU,
on the seeded inputs of tests/superpoint_cases.py, and records what they compute; it refuses to run where the
reference is absent and no test imports it.  Stand-ins live in sys.modules only: a no-op `gin`, a `cv2` that
has nothing but a version when cv2 is not installed, and empty modules for what superpoint_predictor.py
imports beside the three files above (the two reference files it needs are loaded by path).  The frontend
is built without weights (object.__new__ and its attributes); its net is a stub whose forward returns the
case's (semi, coarse_desc).

The reference's sort ties, topk ties and fp32 exp are not reproducible bit for bit, so per case the generator
takes the first seed for which the reference's own outputs satisfy, and asserts:
  - no heat value within 64 fp32 ulps of the threshold;
  - any two candidates within one NMS window, and any two kept points, differ by more than 64 ulps;
  - per matching row |d0 - r^2 d1| > 1e-4, d1 - d0 > 1e-5 and d2 - d1 > 1e-5 (fp64 distances);
  - no two landmarks equidistant from a keypoint within 1e-9.
Detector files hold the inputs, the reference's pts / desc / heatmap, the fp64 restatements of the heatmap and
the descriptors and e_ref = max |reference fp32 - fp64 restatement| of each; the matching file holds, per case,
the seed, both neighbours' indices, the mask, the match list, the argmins and the assembled arrays (no
descriptors: the tests rebuild them from the seed).

Run:  python tests/golden/gen_golden_superpoint.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
S2DHM = os.path.join(REF, "s2dhm")
DEMO = os.path.join(S2DHM, "third_party", "SuperPointPretrainedNetwork", "demo_superpoint.py")

if not os.path.isfile(DEMO):
    raise SystemExit("gen_golden_superpoint.py needs the reference at /root/reference; use the committed fixtures instead")

sys.path.insert(0, os.path.dirname(HERE))
import superpoint_cases as sc  # noqa: E402


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _deco(*a, **k):
    if len(a) == 1 and callable(a[0]) and not k:
        return a[0]
    return lambda f: f


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


_stub("gin", configurable=_deco, register=_deco)
if importlib.util.find_spec("cv2") is None:
    _stub("cv2", __version__="4.0.0")

import torch  # noqa: E402

torch.set_num_threads(1)

ref_demo = _load("third_party.SuperPointPretrainedNetwork.demo_superpoint", DEMO)
ref_ka = _load("pose_prediction.keypoint_association", os.path.join(S2DHM, "pose_prediction", "keypoint_association.py"))
_stub("pose_prediction.predictor", PosePredictor=type("PosePredictor", (), {}))
_stub("pose_prediction.solve_pnp")
_stub("pose_prediction.exhaustive_search")
_stub("pose_prediction", predictor=sys.modules["pose_prediction.predictor"], keypoint_association=ref_ka,
      solve_pnp=sys.modules["pose_prediction.solve_pnp"], exhaustive_search=sys.modules["pose_prediction.exhaustive_search"])
_stub("superpoint.detect_and_compute_superpoint")
_stub("superpoint", detect_and_compute_superpoint=sys.modules["superpoint.detect_and_compute_superpoint"])
_stub("third_party.SuperPointPretrainedNetwork", demo_superpoint=ref_demo)
_stub("third_party", SuperPointPretrainedNetwork=sys.modules["third_party.SuperPointPretrainedNetwork"])
_stub("visualization.plot_correspondences")
_stub("visualization", plot_correspondences=sys.modules["visualization.plot_correspondences"])
ref_sp = _load("pose_prediction.superpoint_predictor", os.path.join(S2DHM, "pose_prediction", "superpoint_predictor.py"))

ULPS = 64
MAX_SEEDS = 400


class _Net:
    def __init__(self, semi, coarse):
        self.out = (torch.from_numpy(semi.copy())[None], torch.from_numpy(coarse.copy())[None])

    def forward(self, inp):
        return self.out


def frontend(name, seed):
    H, W, D, nms_dist, conf, _, _ = sc.DETECTOR[name]
    fe = object.__new__(ref_demo.SuperPointFrontend)
    fe.name, fe.cuda, fe.nms_dist, fe.conf_thresh, fe.nn_thresh = "SuperPoint", False, nms_dist, conf, 0.7
    fe.cell, fe.border_remove = 8, 4
    fe.net = _Net(*sc.detector_inputs(name, seed))
    return fe


def detector_ok(name, fe, heat):
    """The margins of the reference's own heatmap; returns the kept points before the border removal, or None."""
    H, W, _, d, conf, _, _ = sc.DETECTOR[name]
    thr = np.float32(conf)
    if (sc.ulps32(heat, np.full_like(heat, thr)) <= ULPS).any():
        return None
    ys, xs = np.where(heat >= thr)
    for y, x in zip(ys, xs):
        win = heat[max(0, y - d):y + d + 1, max(0, x - d):x + d + 1]
        c = win[win >= thr]
        if (sc.ulps32(c, np.full_like(c, heat[y, x])) <= ULPS).sum() > 1:  # (itself)
            return None
    pts = np.zeros((3, len(xs)))
    pts[0], pts[1], pts[2] = xs, ys, heat[ys, xs]
    kept, _ = fe.nms_fast(pts, H, W, dist_thresh=d)
    conf_kept = np.sort(kept[2].astype(np.float32))
    if len(conf_kept) > 1 and (sc.ulps32(conf_kept[1:], conf_kept[:-1]) <= ULPS).any():
        return None
    return kept


def gen_detector(name):
    H, W, D, d, conf, _, peaks = sc.DETECTOR[name]
    for seed in range(MAX_SEEDS):
        fe = frontend(name, seed)
        semi, coarse = sc.detector_inputs(name, seed)
        pts, desc, heat = fe.run(np.zeros((H, W), np.float32))
        if name == "none":
            assert pts.shape == (3, 0) and desc is None and heat is None
            assert not (sc.heat64(semi) >= conf * 0.5).any()
            out = dict(seed=seed, semi=semi, coarse=coarse, pts=pts)
            break
        kept = detector_ok(name, fe, heat)
        if kept is None:
            continue
        assert heat.dtype == np.float32 and desc.dtype == np.float32 and pts.dtype == np.float64
        h64 = sc.heat64(semi)
        d64 = sc.desc64(coarse, pts, H, W, False)
        out = dict(seed=seed, semi=semi, coarse=coarse, pts=pts, desc=desc, heatmap=heat, heat64=h64, desc64=d64,
                   e_ref_heat=np.abs(heat - h64).max(), e_ref_desc=np.abs(desc - d64).max(),
                   n_kept_before_border=kept.shape[1], n_candidates=int((heat >= np.float32(conf)).sum()))
        # what the case is there to pin
        n_border = kept.shape[1] - pts.shape[1]
        if name == "border":
            assert n_border >= 2, n_border
            got = {(int(x), int(y)) for x, y in pts[:2].T}
            assert (5, 22) not in got and (2, 20) not in got and (43, 5) not in got and (30, 30) in got, got
        if name in ("main", "dense"):
            got = {(int(x), int(y)) for x, y in pts[:2].T}
            chain = [(x, y) for x, y, _ in peaks[:9]]
            assert chain[0] in got and chain[1] not in got and chain[2] in got and chain[3] not in got, (chain, got)
        break
    else:
        raise SystemExit(f"{name}: no seed below {MAX_SEEDS} keeps the margins")
    path = os.path.join(HERE, f"superpoint_det_{name}.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    print(f"{name}: seed {out['seed']}, {pts.shape[1]} keypoints, {os.path.getsize(path)} bytes",
          {k: float(out[k]) for k in ("e_ref_heat", "e_ref_desc") if k in out})


class _Self:
    _network = types.SimpleNamespace(device="cpu")


def gen_matching():
    out = {}
    for name, (N1, N2, D, ratio) in sc.MATCHING.items():
        for seed in range(MAX_SEEDS):
            desc1, desc2 = sc.matching_inputs(name, seed)
            dist = 2 * (1 - desc1.astype(np.float64) @ desc2.astype(np.float64).T)
            order = np.argsort(dist, axis=1, kind="stable")
            srt = np.take_along_axis(dist, order, axis=1)
            d0, d1 = srt[:, 0], srt[:, 1]
            if (np.abs(d0 - ratio ** 2 * d1) <= 1e-4).any() or (d1 - d0 <= 1e-5).any():
                continue
            if N2 > 2 and (srt[:, 2] - d1 <= 1e-5).any():
                continue
            q_kp, r_kp, p2, p3 = sc.assembly_inputs(name, seed)
            dl = ((r_kp[:2].T[:, None, :] - p2[None]) ** 2).sum(-1)
            dls = np.sort(dl, axis=1)
            if (dls[:, 1] - dls[:, 0] <= 1e-9).any():
                continue
            break
        else:
            raise SystemExit(f"{name}: no seed below {MAX_SEEDS} keeps the margins")
        matches = ref_ka.fast_keypoint_matching(desc1, desc2, ratio)
        ok = d0 <= ratio ** 2 * d1
        assert matches.dtype == np.int64 and np.array_equal(matches[:, 0], np.flatnonzero(ok)), name
        assert np.array_equal(matches[:, 1], order[ok, 0]), name
        if N1 >= 63:
            assert ok.sum() >= 5 and (~ok).sum() >= 5, (name, ok.sum())
        argmins = ref_ka.fast_closest_points(torch.from_numpy(r_kp[:2].copy()), torch.from_numpy(p2.copy())).numpy()
        assert np.array_equal(argmins, dl.argmin(axis=1))
        x2, r2, x3 = ref_sp.SuperPointPredictor._assemble_matches(_Self(), q_kp.copy(), r_kp.copy(), p2.copy(), p3.copy(),
                                                                   matches)
        counts = np.bincount(matches[:, 1], minlength=N2)
        assert counts.max() >= 2 and (counts == 0).any() or N1 < 63, name
        out.update({f"{name}.seed": seed, f"{name}.nn_idx": order[:, :2].astype(np.int32), f"{name}.ok": ok,
                    f"{name}.matches": matches, f"{name}.argmins": argmins.astype(np.int64), f"{name}.x2D": x2,
                    f"{name}.x2D_reference": r2, f"{name}.x3D": x3})
        print(f"{name}: seed {seed}, {len(matches)} matches of {N1} rows, {x2.shape[0]} assembled")
    path = os.path.join(HERE, "superpoint_matching.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)


def gen_net():
    net = ref_demo.SuperPointNet()
    sd = net.state_dict()
    np.savez_compressed(os.path.join(HERE, "superpoint_net.npz"), names=np.array(list(sd.keys())),
                        shapes=np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], np.int64),
                        ndims=np.array([v.dim() for v in sd.values()], np.int64))


if __name__ == "__main__":
    for case in sc.DETECTOR:
        gen_detector(case)
    gen_matching()
    gen_net()
