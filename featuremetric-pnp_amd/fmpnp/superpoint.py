"""The SuperPoint baseline on the GPU: the reference's sparse-to-sparse predictor (SuperPointPredictor,
s2dhm/pose_prediction/superpoint_predictor.py) between the network's two output tensors and the best
prediction.

    SuperPointNet                       the network (demo_superpoint.py:72-124), its parameter names and shapes
    superpoint_postprocess(...)         SuperPointFrontend.run after the forward pass (:238-284): detector head,
                                        NMS and descriptor sampling, three HIP stages
    SuperPointFrontend(net, ...).run    the forward pass (the caller's PyTorch-ROCm module) and the above
    HipSuperPointNet(net)               opt-in: that forward pass through libfmpnp's own operators (exact-fp32 3x3
                                        and 1x1 convolutions, max-pool, the descriptor normalisation), bit-identical
                                        to its CPU twins; SuperPointFrontend takes it in the net's place
    fast_keypoint_matching(...)         keypoint_association.py:88-108 (the MFMA correlation and a two-nearest
                                        row reduction)
    fast_closest_points(...)            keypoint_association.py:77-86
    assemble_matches(...)               _assemble_matches (superpoint_predictor.py:45-65)
    superpoint_localize(...)            SuperPointPredictor.run for one query (:74-127): stages 4-5 per reference
                                        in rank order, one solve_pnp_multi, the fallback and the best pick

Every stage has a CPU twin (cpu=True here) that computes the same bits from the same code; it is an explicit
choice, never a fallback.  A device-resident chain is out of scope: every stage ends with one host wait (the
count after the NMS has to reach the host anyway).
"""
import ctypes

import numpy as np
import torch

from . import _lib, config
from . import encoder as _enc
from .hypercolumn import assemble_hypercolumn, assemble_hypercolumn_cpu
from .localize import KINDS, Localization, _fallback, _ref_get
from .pnp import _bound, solve_pnp_cpu, solve_pnp_multi

CELL, BORDER = _lib.SP_CELL, _lib.SP_BORDER
NMS_GROUP = 4  # NMS rounds queued per host read of the live count


class SuperPointNet(torch.nn.Module):
    """The SuperPoint network: a shared VGG-style encoder with a detector head (65 channels per 8 x 8 cell)
    and a descriptor head (256 channels, L2-normalised).  The parameter names and shapes are those of
    superpoint_v1.pth, so load_state_dict takes that file."""

    def __init__(self):
        super().__init__()
        conv = torch.nn.Conv2d
        self.relu = torch.nn.ReLU(inplace=True)
        self.pool = torch.nn.MaxPool2d(kernel_size=2, stride=2)
        widths = {"1": (1, 64), "2": (64, 64), "3": (64, 128), "4": (128, 128)}
        for name, (c_in, c_out) in widths.items():
            setattr(self, f"conv{name}a", conv(c_in, c_out, kernel_size=3, stride=1, padding=1))
            setattr(self, f"conv{name}b", conv(c_out, c_out, kernel_size=3, stride=1, padding=1))
        self.convPa = conv(128, 256, kernel_size=3, stride=1, padding=1)
        self.convPb = conv(256, CELL * CELL + 1, kernel_size=1, stride=1, padding=0)
        self.convDa = conv(128, 256, kernel_size=3, stride=1, padding=1)
        self.convDb = conv(256, 256, kernel_size=1, stride=1, padding=0)

    def forward(self, x):
        """x [N, 1, H, W] -> semi [N, 65, H/8, W/8], desc [N, 256, H/8, W/8]."""
        for name in "123":
            x = self.relu(getattr(self, f"conv{name}a")(x))
            x = self.pool(self.relu(getattr(self, f"conv{name}b")(x)))
        x = self.relu(self.conv4b(self.relu(self.conv4a(x))))
        semi = self.convPb(self.relu(self.convPa(x)))
        desc = self.convDb(self.relu(self.convDa(x)))
        return semi, desc / torch.norm(desc, p=2, dim=1).unsqueeze(1)


SP_BODY = ("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b")
SP_CONVS = SP_BODY + ("convPa", "convPb", "convDa", "convDb")  # in the order of SuperPointNet.forward
SP_HEADS = ("convPb", "convDb")  # the two 1x1 convolutions


class HipSuperPointNet(torch.nn.Module):
    """A SuperPoint network the caller built -- SuperPointNet, or any module with the twelve convolutions under
    SuperPoint's names (conv1a .. conv4b, convPa, convPb, convDa, convDb), such as the reference's own class with
    superpoint_v1.pth loaded -- run through libfmpnp's operators instead of the framework's.  forward(x) follows
    SuperPointNet.forward exactly: x [N, 1, H, W] float32 -> (semi [N, 65, H // 8, W // 8], desc [N, 256, H // 8,
    W // 8]).  Every convolution and the ReLU behind it are one launch (conv3x3; conv1x1 for convPb and convDb, with
    no ReLU), the three pools are maxpool2x2, and desc is the raw convDb output divided by its L2 norm over the
    channels by assemble_hypercolumn of that one map (FMPNP_HC_NORMALIZE's contract: a zero vector gives NaN, as
    torch's division does).  SuperPointFrontend(HipSuperPointNet(net), ...) is the baseline from the image on with
    no framework kernel in it.

    The plan is built once: every convolution is checked (a missing attribute, a wrong kernel size, stride,
    padding or channel count, or parameters that are not float32 raise TypeError naming the attribute) and the
    weights and biases are checked finite on the host (ValueError).  The net stays a submodule: .to(),
    state_dict() and parameters() work as before; the finite check is not repeated when the parameters change.
    Where the module lives decides what runs: the kernels on a CUDA device, the CPU twins on the CPU (conv3x3_cpu,
    conv1x1_cpu, maxpool2x2_cpu, assemble_hypercolumn_cpu), bit-identical to the device with precision="f32".
    Inference only, under torch.no_grad().

    precision="f16" (opt-in) runs the ten 3x3 convolutions through conv3x3(precision="f16"), their packed weight
    images cached per convolution as HipEncoder caches them; the plan then also rejects 3x3 weights of magnitude
    >= 65520.  The two 1x1 heads stay exact fp32: they are well under 1 % of the network's multiply-adds, and
    conv1x1 has no fp16 form.  On the CPU "f16" runs the fp16 reference, which is not a twin."""

    def __init__(self, net, precision="f32"):
        super().__init__()
        self.precision = _enc._precision(precision)
        if not isinstance(net, torch.nn.Module):
            raise TypeError("HipSuperPointNet takes an nn.Module with SuperPoint's twelve convolutions")
        cin = {"conv1a": 1}
        for prev, name in zip(SP_BODY, SP_BODY[1:]):
            cin[name] = prev
        cin.update(convPa="conv4b", convPb="convPa", convDa="conv4b", convDb="convDa")
        for name in SP_CONVS:
            m = getattr(net, name, None)
            if not isinstance(m, torch.nn.Conv2d):
                raise TypeError(f"HipSuperPointNet: attribute {name} is {'missing' if m is None else repr(m)}: the net "
                                f"must carry a Conv2d under each of {', '.join(SP_CONVS)}")
            _enc._check_child(name, m, self.precision, owner="HipSuperPointNet", what="attribute",
                              ksize=1 if name in SP_HEADS else 3)
            want = cin[name] if isinstance(cin[name], int) else getattr(net, cin[name]).out_channels
            if m.in_channels != want:
                raise TypeError(f"HipSuperPointNet: attribute {name} ({m!r}) takes {m.in_channels} channels, "
                                f"the walk gives it {want}")
        self.net = net
        self._images = {}  # attribute name -> ((device, data_ptr, version), packed image)

    def forward(self, x):
        """x [N, 1, H, W] float32 on the network's device -> (semi, desc)."""
        return self.walk(x)[:2]

    def walk(self, x, taps=()):
        """forward, which also records the inputs of the convolutions named in taps -> (semi, desc, {name: input})."""
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 1 or x.dtype != torch.float32:
            raise ValueError("HipSuperPointNet takes a float32 [N, 1, H, W] tensor")
        if not set(taps) <= set(SP_CONVS):
            raise ValueError(f"taps must be among {', '.join(SP_CONVS)}")
        p = next(self.net.parameters())
        if p.device != x.device:
            raise ValueError(f"the batch is on {x.device}, the network on {p.device}")
        if x.shape[0] < 1 or x.shape[2] < CELL or x.shape[3] < CELL:
            raise ValueError(f"a {tuple(x.shape)} batch: H and W must be at least {CELL} (a pool would be empty)")
        x = x.detach().contiguous()
        cuda = x.is_cuda
        conv3, conv1, pool, unit = ((_enc.conv3x3, _enc.conv1x1, _enc.maxpool2x2, assemble_hypercolumn) if cuda else
                                    (_enc.conv3x3_cpu, _enc.conv1x1_cpu, _enc.maxpool2x2_cpu, assemble_hypercolumn_cpu))
        maps = {}

        def params(name, x):
            if name in taps:
                maps[name] = x
            m = getattr(self.net, name)
            return m, m.weight.detach().contiguous(), None if m.bias is None else m.bias.detach().contiguous()

        def c3(name, x):  # the 3x3 convolution and the ReLU behind it: one launch
            m, w, b = params(name, x)
            if self.precision == "f16":  # (the reference rounds the float32 weights itself)
                image = cuda and m.weight.is_contiguous()
                return conv3(x, _enc._cached_image(self._images, name, m.weight) if image else w, b, relu=True,
                             precision="f16")
            return conv3(x, w, b, relu=True)

        def c1(name, x):  # a head's 1x1 convolution: exact fp32 in either precision, no ReLU
            _, w, b = params(name, x)
            return conv1(x, w, b)

        with torch.no_grad():
            for block in "123":
                x = pool(c3(f"conv{block}b", c3(f"conv{block}a", x)))
            x = c3("conv4b", c3("conv4a", x))
            semi = c1("convPb", c3("convPa", x))
            raw = c1("convDb", c3("convDa", x))
            return semi, unit([raw]), maps


def _host32(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32)


def _host64(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64)


def _tensor(a):
    if isinstance(a, np.ndarray) and not a.flags.writeable:
        a = np.array(a)  # (torch wraps writable arrays only)
    return torch.as_tensor(a)


def _dev32(a, device):
    return _tensor(a).to(device=device, dtype=torch.float32).contiguous()


def _dev64(a, device):
    return _tensor(a).to(device=device, dtype=torch.float64).contiguous()


def _device(device, *tensors):
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return torch.device(device if device is not None else "cuda")


def _squeeze_maps(semi, coarse_desc):
    if semi.ndim == 4:
        semi = semi[0]
    if coarse_desc.ndim == 4:
        coarse_desc = coarse_desc[0]
    if semi.ndim != 3 or semi.shape[0] != CELL * CELL + 1:
        raise ValueError("semi must be [65, Hc, Wc]")
    if coarse_desc.ndim != 3 or tuple(coarse_desc.shape[1:]) != tuple(semi.shape[1:]):
        raise ValueError("coarse_desc must be [D, Hc, Wc]")
    return semi, coarse_desc


# ---- the stages ------------------------------------------------------------------------------------------------
def heatmap(semi, cpu=False, device=None):
    """Stage 1: semi [65, Hc, Wc] -> the heatmap [8 Hc, 8 Wc] (fp32; a device tensor, or an array with cpu)."""
    L = _lib.load()
    if cpu:
        semi = _host32(semi)
        heat = np.empty((semi.shape[1] * CELL, semi.shape[2] * CELL), np.float32)
        _lib.check(L.fmpnp_sp_heatmap_cpu(semi.ctypes.data, semi.shape[1], semi.shape[2], heat.ctypes.data),
                   "fmpnp_sp_heatmap_cpu")
        return heat
    dev = _device(device, semi)
    _lib.require_device(dev)
    semi = _dev32(semi, dev)
    heat = torch.empty((semi.shape[1] * CELL, semi.shape[2] * CELL), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.fmpnp_sp_heatmap_async(semi.data_ptr(), semi.shape[1], semi.shape[2], heat.data_ptr(),
                                            _lib.stream_ptr(dev)), "fmpnp_sp_heatmap_async")
    return heat


def nms(heat, conf_thresh, nms_dist, border=BORDER, cpu=False, group=NMS_GROUP, info=None):
    """Stage 2: the heatmap -> pts [3, N] fp64 (x, y, confidence) in descending confidence: nms_fast's greedy
    result with the border points dropped.  On the GPU a device tensor; info (a dict) receives the rounds."""
    L = _lib.load()
    H, W = int(heat.shape[0]), int(heat.shape[1])
    cap = int(L.fmpnp_sp_nms_capacity(H, W, int(nms_dist)))
    n = ctypes.c_int(0)
    if cpu:
        heat = _host32(heat)
        pts = np.empty((3, max(cap, 1)), np.float64)
        _lib.check(L.fmpnp_sp_nms_cpu(heat.ctypes.data, H, W, float(conf_thresh), int(nms_dist), int(border),
                                      pts.ctypes.data, pts.shape[1], ctypes.byref(n)), "fmpnp_sp_nms_cpu")
        return np.ascontiguousarray(pts[:, :n.value])
    dev = _device(None, heat)
    _lib.require_device(dev)
    heat = _dev32(heat, dev)
    rounds = ctypes.c_int(0)
    with torch.cuda.device(dev):
        pts = torch.empty((3, max(cap, 1)), dtype=torch.float64, device=dev)
        ws_bytes = int(L.fmpnp_sp_nms_workspace_size(H, W, int(nms_dist)))
        ws = torch.empty(max(ws_bytes, 8) // 8 + 1, dtype=torch.int64, device=dev)
        rc = L.fmpnp_sp_nms_async(heat.data_ptr(), H, W, float(conf_thresh), int(nms_dist), int(border), pts.data_ptr(),
                                  pts.shape[1], None, int(group), ctypes.byref(n), ctypes.byref(rounds), ws.data_ptr(),
                                  ws.numel() * 8, _lib.stream_ptr(dev))
    _lib.check(rc, "fmpnp_sp_nms_async")
    if info is not None:
        info["rounds"] = rounds.value
    return pts[:, :n.value].contiguous()


def describe(coarse_desc, pts, image_hw, align_corners=False, cpu=False):
    """Stage 3: coarse_desc [D, Hc, Wc] sampled at pts [>= 2, N] -> desc [D, N] fp32, unit columns."""
    L = _lib.load()
    H, W = int(image_hw[0]), int(image_hw[1])
    D, Hc, Wc = (int(v) for v in coarse_desc.shape)
    N = int(pts.shape[1])
    if cpu:
        coarse_desc, pts = _host32(coarse_desc), _host64(pts)
        desc = np.empty((D, N), np.float32)
        _lib.check(L.fmpnp_sp_describe_cpu(coarse_desc.ctypes.data, D, Hc, Wc, pts.ctypes.data, N, N, H, W,
                                           int(bool(align_corners)), desc.ctypes.data, N), "fmpnp_sp_describe_cpu")
        return desc
    dev = _device(None, coarse_desc, pts)
    _lib.require_device(dev)
    coarse_desc, pts = _dev32(coarse_desc, dev), _dev64(pts, dev)
    desc = torch.empty((D, N), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = L.fmpnp_sp_describe_async(coarse_desc.data_ptr(), D, Hc, Wc, pts.data_ptr(), N, N, H, W,
                                       int(bool(align_corners)), desc.data_ptr(), N, _lib.stream_ptr(dev))
    _lib.check(rc, "fmpnp_sp_describe_async")
    return desc


def superpoint_postprocess(semi, coarse_desc, image_hw, nms_dist, conf_thresh, align_corners=False, cpu=False,
                           info=None):
    """SuperPointFrontend.run after the forward pass (demo_superpoint.py:238-284): (pts [3, N] fp64, desc [D, N]
    fp32, heatmap [H, W] fp32) as numpy arrays, and (zeros((3, 0)), None, None) when no pixel reaches
    conf_thresh.  align_corners: what grid_sample does with the reference's call as written is False (the
    installed torch's default); True is the torch the reference was written for."""
    semi, coarse_desc = _squeeze_maps(semi, coarse_desc)
    H, W = int(image_hw[0]), int(image_hw[1])
    if (H // CELL, W // CELL) != tuple(int(v) for v in semi.shape[1:]):
        raise ValueError(f"semi is {tuple(semi.shape[1:])} cells for a {H} x {W} image")
    heat = heatmap(semi, cpu=cpu)
    thresh = np.float32(conf_thresh)
    some = bool((heat >= float(thresh)).any())  # (the one host wait of stage 1)
    if not some:
        return np.zeros((3, 0)), None, None
    pts = nms(heat, conf_thresh, nms_dist, cpu=cpu, info=info)
    D = int(coarse_desc.shape[0])
    if pts.shape[1] == 0:
        desc = np.zeros((D, 0))  # (demo_superpoint.py:270: a float64 array)
    else:
        desc = describe(coarse_desc, pts, (H, W), align_corners, cpu=cpu)
    if not cpu:
        heat, pts = heat.cpu().numpy(), pts.cpu().numpy()
        desc = desc.cpu().numpy() if torch.is_tensor(desc) else desc
    return pts, desc, heat


class SuperPointFrontend:
    """SuperPointFrontend (demo_superpoint.py:127-284) around a network the caller built: run(img) takes an
    H x W float32 image in [0, 1] (tensor or array) and returns (pts, desc, heatmap).  The cv2 preprocessing
    stays the caller's."""

    def __init__(self, net, nms_dist, conf_thresh, nn_thresh, device=None, align_corners=False):
        self.name = "SuperPoint"
        self.net = net
        self.nms_dist, self.conf_thresh, self.nn_thresh = nms_dist, conf_thresh, nn_thresh
        self.cell, self.border_remove = CELL, BORDER
        self.device = device
        self.align_corners = align_corners

    def run(self, img):
        img = torch.as_tensor(img)
        if img.dim() != 2:
            raise ValueError("Image must be grayscale.")
        if img.dtype != torch.float32:
            raise ValueError("Image must be float32.")
        H, W = img.shape
        dev = self.device if self.device is not None else next(iter(self.net.parameters())).device
        with torch.no_grad():
            semi, coarse_desc = self.net(img.to(dev).view(1, 1, H, W))
        return superpoint_postprocess(semi, coarse_desc, (H, W), self.nms_dist, self.conf_thresh, self.align_corners)


def two_nearest(desc1, desc2, ratio_thresh, cpu=False, device=None):
    """Stage 4 with every output: desc1 [N1, D], desc2 [N2, D] -> dict(idx [N1, 2], dist [N1, 2], ok [N1],
    matches [n, 2] int64) as numpy arrays."""
    L = _lib.load()
    N1, D = int(desc1.shape[0]), int(desc1.shape[1])
    N2 = int(desc2.shape[0])
    if int(desc2.shape[1]) != D:
        raise ValueError("the descriptors differ in length")
    n = ctypes.c_int(0)
    idx, dist = np.zeros((N1, 2), np.int32), np.zeros((N1, 2), np.float32)
    ok, matches = np.zeros(N1, np.uint8), np.zeros((N1, 2), np.int64)
    if cpu:
        a, b = _host32(desc1), np.ascontiguousarray(_host32(desc2).T)
        rc = L.fmpnp_sp_match_cpu(a.ctypes.data, N1, D, b.ctypes.data, D, N2, N2, float(ratio_thresh), idx.ctypes.data,
                                  dist.ctypes.data, ok.ctypes.data, matches.ctypes.data, ctypes.byref(n))
        _lib.check(rc, "fmpnp_sp_match_cpu")
    else:
        dev = _device(device, desc1, desc2)
        _lib.require_device(dev)
        a, b = _dev32(desc1, dev), _dev32(desc2, dev).t().contiguous()
        with torch.cuda.device(dev):
            rc = L.fmpnp_sp_match(a.data_ptr(), N1, D, b.data_ptr(), D, N2, N2, float(ratio_thresh), idx.ctypes.data,
                                  dist.ctypes.data, ok.ctypes.data, matches.ctypes.data, ctypes.byref(n),
                                  _lib.stream_ptr(dev))
        _lib.check(rc, "fmpnp_sp_match")
    return dict(idx=idx, dist=dist, ok=ok.astype(bool), matches=matches[:n.value].copy())


def fast_keypoint_matching(desc1, desc2, ratio_thresh, is_torch=False, cpu=False):
    """fast_keypoint_matching (keypoint_association.py:88-108): desc1 [N1, D], desc2 [N2, D] (unit rows) ->
    matches [n, 2] int64, (row of desc1, its nearest row of desc2) of the rows that pass the ratio test."""
    return two_nearest(desc1, desc2, ratio_thresh, cpu=cpu)["matches"]


def assemble_matches(query_keypoints, keypoints, points_2D, points_3D, matches, cpu=False, device=None,
                     return_argmins=False):
    """_assemble_matches (superpoint_predictor.py:45-65): (x2D [n, 1, 2], x2D_reference [n, 1, 2], x3D [n, 1, 3]),
    one row per reference keypoint that occurs in matches[:, 1], in ascending keypoint order."""
    L = _lib.load()
    q, r = _host64(query_keypoints), _host64(keypoints)
    p2, p3 = _host64(points_2D).reshape(-1, 2), _host64(points_3D).reshape(-1, 3)
    m = np.ascontiguousarray(np.asarray(matches, np.int64).reshape(-1, 2))
    N1, N2, M = q.shape[1], r.shape[1], p2.shape[0]
    if p3.shape[0] != M:
        raise ValueError(f"{p3.shape[0]} 3D points for {M} 2D points")
    argmin = np.zeros(N2, np.int32)
    x2, r2, x3 = np.zeros((N2, 2)), np.zeros((N2, 2)), np.zeros((N2, 3))
    n = ctypes.c_int(0)
    if cpu:
        rc = L.fmpnp_sp_assemble_cpu(q.ctypes.data, N1, N1, r.ctypes.data, N2, N2, p2.ctypes.data, p3.ctypes.data, M,
                                     m.ctypes.data, m.shape[0], argmin.ctypes.data, x2.ctypes.data, r2.ctypes.data,
                                     x3.ctypes.data, ctypes.byref(n))
        _lib.check(rc, "fmpnp_sp_assemble_cpu")
    else:
        dev = _device(device)
        _lib.require_device(dev)
        dq, dr, d2, d3 = (_dev64(a, dev) for a in (q, r, p2, p3))
        dm = _tensor(m).to(dev)
        with torch.cuda.device(dev):
            rc = L.fmpnp_sp_assemble(dq.data_ptr(), N1, N1, dr.data_ptr(), N2, N2, d2.data_ptr(), d3.data_ptr(), M,
                                     dm.data_ptr(), m.shape[0], argmin.ctypes.data, x2.ctypes.data, r2.ctypes.data,
                                     x3.ctypes.data, ctypes.byref(n), _lib.stream_ptr(dev))
        _lib.check(rc, "fmpnp_sp_assemble")
    out = (x2[:n.value].reshape(-1, 1, 2), r2[:n.value].reshape(-1, 1, 2), x3[:n.value].reshape(-1, 1, 3))
    return out + (argmin,) if return_argmins else out


def fast_closest_points(points, reference_points, cpu=False):
    """fast_closest_points (keypoint_association.py:77-86): points [2, k], reference_points [M, 2] -> for each
    point the index of the closest reference point (int64 [k])."""
    points = _host64(points)
    if points.shape[0] != 2 or np.asarray(reference_points).shape[1] != 2:
        raise ValueError("points must be [2, k] and reference_points [M, 2]")
    M = np.asarray(reference_points).shape[0]
    out = assemble_matches(np.zeros((2, 0)), points, reference_points, np.zeros((M, 3)), np.zeros((0, 2), np.int64),
                           cpu=cpu, return_argmins=True)
    return out[3].astype(np.int64)


def _sp_bound(name, value):
    if value is None:
        value = config.superpoint_kwargs()[name]
    if value is None:
        raise TypeError(f"SuperPointPredictor: {name} is not bound (pass it, or "
                        f"fmpnp.config.configure(superpoint_{name}=...))")
    return value


def _same_camera(a, b):
    return (np.array_equal(np.asarray(_ref_get(a, "intrinsics")), np.asarray(_ref_get(b, "intrinsics")))
            and np.array_equal(np.asarray(_ref_get(a, "distortion_coefficients")),
                               np.asarray(_ref_get(b, "distortion_coefficients"))))


def superpoint_localize(query, references, frontend=None, top_N=None, ratio=None, reprojection_threshold=None,
                        minimum_matches=None, minimum_inliers=None, return_masked=None, iters=None, seed=None,
                        return_all=False, cpu=False, n_threads=0):
    """SuperPointPredictor.run for one query (superpoint_predictor.py:74-127).  query: (pts [3, N], desc [D, N]),
    or an image for frontend.run.  references, in rank order (the first top_N are used): mappings with points_2D,
    points_3D, intrinsics, distortion_coefficients, filename, optionally fallback_pose = (quaternion, matrix), and
    either keypoints [3, n] + descriptors [D, n] or image (run through the frontend, as the reference does per
    query).  Per reference stages 4-5, then solve_pnp_multi over the references (one launch sequence per run of
    references with the same camera), the reference's-own-pose fallback and the best pick of fmpnp.localize.
    top_N and ratio left None come from fmpnp.config (configure(superpoint_top_N=..., superpoint_ratio=...)), the
    solve_pnp arguments from its bindings.  Returns a Localization (refined is None: this predictor has no
    refinement)."""
    top_N, ratio = int(_sp_bound("top_N", top_N)), float(_sp_bound("ratio", ratio))
    minimum_inliers = _bound("minimum_inliers", minimum_inliers)
    if isinstance(query, (tuple, list)):
        q_pts, q_desc = query[0], query[1]
    else:
        if frontend is None:
            raise ValueError("an image query needs a frontend")
        q_pts, q_desc, _ = frontend.run(query)
    q_pts = _host64(q_pts)
    q_desc = np.zeros((1, 0), np.float32) if q_desc is None else q_desc
    refs = list(references)[:top_N]
    items, kps = [], []
    for ref in refs:
        r_pts, r_desc = _ref_get(ref, "keypoints"), _ref_get(ref, "descriptors")
        if r_pts is None or r_desc is None:
            if frontend is None:
                raise ValueError("a reference needs keypoints and descriptors, or an image and a frontend")
            r_pts, r_desc, _ = frontend.run(_ref_get(ref, "image"))
        r_pts = _host64(r_pts)
        desc1 = q_desc.T if torch.is_tensor(q_desc) else np.asarray(q_desc).T
        desc2 = r_desc.T if torch.is_tensor(r_desc) else np.asarray(r_desc).T
        matches = fast_keypoint_matching(desc1, desc2, ratio, cpu=cpu)
        x2, r2, x3 = assemble_matches(q_pts, r_pts, _ref_get(ref, "points_2D"), _ref_get(ref, "points_3D"), matches,
                                      cpu=cpu)
        items.append((x2, x3, _ref_get(ref, "filename"), r2, r_pts))
        kps.append(r_pts)
    kw = dict(reprojection_threshold=reprojection_threshold, minimum_matches=minimum_matches,
              minimum_inliers=minimum_inliers, return_masked=return_masked, iters=iters, seed=seed)
    preds, g = [], 0
    while g < len(refs):  # (one solve_pnp_multi per run of references that share a camera: usually one)
        e = g + 1
        while e < len(refs) and _same_camera(refs[g], refs[e]):
            e += 1
        K, dist = _ref_get(refs[g], "intrinsics"), _ref_get(refs[g], "distortion_coefficients")
        if cpu:
            preds += [solve_pnp_cpu(it[0], it[1], K, dist, reference_filename=it[2], reference_2D_points=it[3],
                                    reference_keypoints=it[4], n_threads=n_threads, **kw) for it in items[g:e]]
        else:
            preds += solve_pnp_multi(items[g:e], K, dist, **kw)
        g = e
    # superpoint_predictor.py:117-124 and predictor.py:48-54: the fallback, then the maximum of num_inliers, the
    # lowest rank among equals (fmpnp_localize_impl.h pair_score / pick_best)
    best, best_score, best_kind, finals = None, -1, _lib.LOC_NONE, []
    for j, (ref, pred, it) in enumerate(zip(refs, preds, items)):
        kind, score = _lib.LOC_NONE, -1
        if pred.success:
            kind, score = _lib.LOC_SOLVED, pred.num_inliers
        elif _ref_get(ref, "fallback_pose") is not None:
            pred = _fallback(ref, it[0].shape[0], it[3], it[0], it[1])
            kind, score = _lib.LOC_FALLBACK, 0
        finals.append(pred)
        if score > best_score:
            best, best_score, best_kind = j, score, kind
    prediction = finals[best] if best is not None else None
    export = None if prediction is None else [*prediction.quaternion, *list(np.asarray(prediction.matrix)[:3, 3])]
    return Localization(export=export, prediction=prediction, refined=None, kind=KINDS[best_kind], best=best,
                        predictions=finals if return_all else None, cached_matches=None)
