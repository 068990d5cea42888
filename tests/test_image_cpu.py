"""The image front end on the CPU tier: the twins (fmpnp.resize_lanczos_cpu, fmpnp.image_to_tensor_cpu) against Pillow's
recorded results (tests/golden/image_lanczos.npz), the numpy restatement of image_cases.py and, where Pillow is
installed, live Image.resize / Image.thumbnail -- all under ==; the value transforms against torch's own CPU operations
under torch.equal; thumbnail_size; load_images; thread-count independence; every error path; strided sources; the ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import fmpnp
from fmpnp import _lib

import image_cases as ic

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "featuremetric-pnp_amd")


# ---- the resize -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind", ic.CASES, ids=ic.CASE_IDS)
def test_twin_equals_pillow_fixture_and_restatement(shape, kind):
    a, want = ic.fixture(shape, kind)
    got = fmpnp.resize_lanczos_cpu(a, shape[2:])
    assert got.dtype == torch.uint8 and tuple(got.shape) == shape[2:] + (3,)
    assert np.array_equal(got.numpy(), want)
    assert np.array_equal(ic.restate_resize(a, shape[2:]), want)


def test_fixture_records_its_pillow():
    assert str(ic.golden()["pillow_version"]) == "12.2.0"
    assert os.path.getsize(ic.GOLDEN) < 256 * 1024


def test_twin_equals_live_pillow_on_random_shape_pairs():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(2024)
    for n in range(20):
        h_in, w_in, h, w = (int(v) for v in rng.randint(1, 90, 4))
        a = rng.randint(0, 256, (h_in, w_in, 3)).astype(np.uint8)
        want = np.asarray(Image.fromarray(a).resize((w, h), Image.LANCZOS))
        got = fmpnp.resize_lanczos_cpu(a, (h, w)).numpy()
        assert np.array_equal(got, want), (n, h_in, w_in, h, w)


THUMB_SIZES = [(1920, 1080, 1024), (1080, 1920, 1024), (1024, 1024, 1024), (1024, 768, 1024), (800, 600, 1024),
               (1025, 3, 1024), (3, 1025, 1024), (5000, 1, 64), (1, 5000, 64), (300, 200, 150), (200, 300, 150),
               (2048, 2048, 1024), (1000, 3000, 100), (3000, 1000, 100), (7, 5, 3), (640, 427, 512), (1296, 972, 1024),
               (101, 100, 100), (100, 101, 100), (150, 100, 100), (2, 3, 1), (1027, 1025, 1024)]


def test_thumbnail_size_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    for w, h, s in THUMB_SIZES:
        im = Image.new("RGB", (w, h))
        im.thumbnail((s, s), Image.LANCZOS)
        assert fmpnp.thumbnail_size(w, h, s) == im.size, (w, h, s)
    with pytest.raises(ValueError):
        fmpnp.thumbnail_size(0, 5, 4)


def test_thumbnail_size_without_pillow():
    """The values Pillow 12.2.0 gives, recorded: an image that fits, a tie of the aspects, one-pixel results."""
    assert fmpnp.thumbnail_size(800, 600, 1024) == (800, 600)
    assert fmpnp.thumbnail_size(1920, 1080, 1024) == (1024, 576)
    assert fmpnp.thumbnail_size(1080, 1920, 1024) == (576, 1024)
    assert fmpnp.thumbnail_size(5000, 1, 64) == (64, 1)
    assert fmpnp.thumbnail_size(1, 5000, 64) == (1, 64)
    assert fmpnp.thumbnail_size(1024, 768, 1024) == (1024, 768)


@pytest.mark.parametrize("preprocessing", ["torch", "caffe"])
def test_load_images_equals_thumbnail_and_transform(preprocessing, tmp_path):
    """Where the shrink is below 4x on both axes Image.thumbnail is the fair resampling; from a file and from an array."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(5)
    for (h, w, s) in [(60, 90, 48), (90, 60, 48), (50, 70, 20), (40, 40, 64)]:
        a = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        im = Image.fromarray(a)
        im.thumbnail((s, s), Image.LANCZOS)
        thumb = np.asarray(im)
        assert a.shape[0] / thumb.shape[0] < 4 and a.shape[1] / thumb.shape[1] < 4
        want = ic.torch_transform(torch.from_numpy(thumb.copy())[None], preprocessing)
        path = str(tmp_path / f"im_{h}_{w}.png")
        Image.fromarray(a).save(path)
        for item in (a, path, torch.from_numpy(a)):
            got = fmpnp.load_images([item], s, True, "cpu", preprocessing=preprocessing)
            assert torch.equal(got, want), (h, w, s)
        got = fmpnp.image_loader(preprocessing)([path, a], s, True, torch.device("cpu"))
        assert torch.equal(got, torch.cat([want, want]))
    # no resize; a square resize without the ratio; sizes that do not agree
    a = rng.randint(0, 256, (9, 12, 3)).astype(np.uint8)
    assert torch.equal(fmpnp.load_images([a], 4, False, "cpu", preprocessing=preprocessing),
                       ic.torch_transform(torch.from_numpy(a)[None], preprocessing))
    sq = fmpnp.load_images([a], 6, True, "cpu", preserve_ratio=False, preprocessing=preprocessing)
    assert torch.equal(sq, ic.torch_transform(fmpnp.resize_lanczos_cpu(a, (6, 6))[None], preprocessing))
    with pytest.raises(ValueError, match="one size"):
        fmpnp.load_images([a, a[:5]], 4, False, "cpu")


def test_superpoint_image_is_the_swapped_gray():
    a = ic.make_input((12, 17), "random")
    got = fmpnp.superpoint_image(a, device="cpu")
    assert tuple(got.shape) == (1, 1, 12, 17)
    assert torch.equal(got, ic.torch_transform(torch.from_numpy(a)[None], "gray", swap_rb=True))


# ---- the value transforms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preprocessing", ic.TRANSFORMS, ids=[str(t) for t in ic.TRANSFORMS])
def test_transform_equals_torch_on_every_byte(preprocessing):
    u8 = torch.from_numpy(ic.all_bytes_image())
    for c in range(3):
        assert len(set(u8[..., c].flatten().tolist())) == 256
    got = fmpnp.image_to_tensor_cpu(u8, preprocessing=preprocessing)
    want = ic.torch_transform(u8, preprocessing)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got, want)


def test_a_reciprocal_would_not_equal_torch():
    """The check above has teeth: the same transform with * (1 / 255) differs from torch's somewhere."""
    u8 = torch.from_numpy(ic.all_bytes_image())
    f = u8.permute(0, 3, 1, 2).float()
    col = lambda v: torch.tensor(v, dtype=torch.float32).view(1, 3, 1, 1)  # noqa: E731
    cheap = ((f * torch.tensor(1.0 / 255.0, dtype=torch.float32)) - col(ic.TORCH_MEAN)) / col(ic.TORCH_STD)
    assert not torch.equal(cheap, ic.torch_transform(u8, "torch"))


def test_transform_custom_mean_std_and_caffe_order():
    u8 = torch.from_numpy(ic.all_bytes_image())
    mean, std = (0.5, 0.25, 0.125), (0.3, 0.2, 0.1)
    assert torch.equal(fmpnp.image_to_tensor_cpu(u8, preprocessing="torch", mean=mean, std=std),
                       ic.torch_transform(u8, "torch", mean, std))
    cm = (1.5, 2.5, 3.5)
    got = fmpnp.image_to_tensor_cpu(u8, preprocessing="caffe", mean=cm)
    assert torch.equal(got, ic.torch_transform(u8, "caffe", cm))
    # output channel 0 is the source's blue, less the FIRST mean
    assert torch.equal(got[:, 0], u8[..., 2].float() - 1.5) and torch.equal(got[:, 2], u8[..., 0].float() - 3.5)
    default = fmpnp.image_to_tensor_cpu(u8, preprocessing="caffe")
    assert torch.equal(default[:, 0], u8[..., 2].float() - torch.tensor(103.939, dtype=torch.float32))
    # d2net_preprocess, the host-side transform the library already has, agrees
    for pre in ("caffe", "torch", None):
        host = torch.from_numpy(fmpnp.d2net_preprocess(u8[0].numpy(), pre))[None]
        assert torch.equal(fmpnp.image_to_tensor_cpu(u8, preprocessing=pre), host)


@pytest.mark.parametrize("swap_rb", [True, False])
def test_gray_equals_the_integer_formula(swap_rb):
    u8 = torch.from_numpy(np.concatenate([ic.all_bytes_image()[0], ic.make_input((16, 48), "random")]))[None]
    got = fmpnp.image_to_tensor_cpu(u8, preprocessing="gray", swap_rb=swap_rb)
    assert tuple(got.shape) == (1, 1, 32, 48)
    assert torch.equal(got, ic.torch_transform(u8, "gray", swap_rb=swap_rb))
    p = u8[0].numpy().astype(np.int64)
    a, b = (p[..., 2], p[..., 0]) if swap_rb else (p[..., 0], p[..., 2])
    y = (9798 * a + 19235 * p[..., 1] + 3735 * b + 16384) >> 15
    assert np.array_equal(np.rint(got[0, 0].numpy().astype(np.float64) * 255).astype(np.int64), y)
    assert not torch.equal(got, fmpnp.image_to_tensor_cpu(u8, preprocessing="gray", swap_rb=not swap_rb))


@pytest.mark.parametrize("preprocessing", ic.TRANSFORMS, ids=[str(t) for t in ic.TRANSFORMS])
def test_to_tensor_with_a_resize_is_the_transform_of_the_resize(preprocessing):
    for shape in ic.SHAPES[:5]:
        a = ic.make_input(shape[:2], "random")
        got = fmpnp.image_to_tensor_cpu(a, shape[2:], preprocessing)
        want = ic.torch_transform(torch.from_numpy(ic.fixture(shape, "random")[1])[None], preprocessing)
        assert torch.equal(got, want), shape


# ---- independence of the call's shape -------------------------------------------------------------------------------
def test_thread_count_independence():
    a = np.stack([ic.make_input((96, 128), "random", seed=s) for s in range(3)])
    one_u8 = fmpnp.resize_lanczos_cpu(a, (25, 33), n_threads=1)
    one_f = fmpnp.image_to_tensor_cpu(a, (25, 33), n_threads=1)
    for nt in (2, 5, 0):
        assert torch.equal(fmpnp.resize_lanczos_cpu(a, (25, 33), n_threads=nt), one_u8)
        assert torch.equal(fmpnp.image_to_tensor_cpu(a, (25, 33), n_threads=nt), one_f)
    for b in range(3):  # (and of the batch)
        assert torch.equal(fmpnp.resize_lanczos_cpu(a[b], (25, 33)), one_u8[b])


@pytest.mark.parametrize("size", [(16, 24), (37, 20), (11, 53), (37, 53)])
def test_strided_source_equals_its_contiguous_copy(size):
    big = torch.from_numpy(np.stack([ic.make_input((45, 64), "random", seed=s) for s in range(2)]))
    view = big[:, 3:40, 5:58]
    assert not view.is_contiguous() and tuple(view.shape) == (2, 37, 53, 3)
    copy = view.contiguous()
    assert torch.equal(fmpnp.resize_lanczos_cpu(view, size), fmpnp.resize_lanczos_cpu(copy, size))
    assert torch.equal(fmpnp.image_to_tensor_cpu(view, size, "caffe"), fmpnp.image_to_tensor_cpu(copy, size, "caffe"))
    assert torch.equal(fmpnp.resize_lanczos_cpu(view[0], size), fmpnp.resize_lanczos_cpu(copy, size)[0])
    # a view whose pixels are not three consecutive bytes is copied, not misread
    flipped = copy.flip(3)
    assert torch.equal(fmpnp.resize_lanczos_cpu(flipped, size), fmpnp.resize_lanczos_cpu(flipped.contiguous(), size))


def test_out_argument():
    a = torch.from_numpy(ic.make_input((37, 53), "random"))
    out = torch.empty((16, 24, 3), dtype=torch.uint8)
    assert fmpnp.resize_lanczos_cpu(a, (16, 24), out=out).data_ptr() == out.data_ptr()
    assert torch.equal(out, fmpnp.resize_lanczos_cpu(a, (16, 24)))
    fo = torch.empty((1, 3, 16, 24))
    assert fmpnp.image_to_tensor_cpu(a, (16, 24), out=fo) is fo
    with pytest.raises(ValueError):
        fmpnp.resize_lanczos_cpu(a, (16, 24), out=torch.empty((16, 25, 3), dtype=torch.uint8))
    with pytest.raises(ValueError):
        fmpnp.image_to_tensor_cpu(a, (16, 24), out=torch.empty((1, 3, 16, 24), dtype=torch.float64))


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_python_argument_errors():
    a = torch.from_numpy(ic.make_input((8, 8), "random"))
    with pytest.raises(ValueError):
        fmpnp.resize_lanczos_cpu(a.float(), (4, 4))
    with pytest.raises(ValueError):
        fmpnp.resize_lanczos_cpu(a[..., :2], (4, 4))
    with pytest.raises(ValueError):
        fmpnp.resize_lanczos_cpu(a, (0, 4))
    with pytest.raises(ValueError):
        fmpnp.resize_lanczos_cpu(a, 4)
    with pytest.raises(ValueError):
        fmpnp.resize_lanczos(a, (4, 4))  # (a CPU tensor is not the GPU form's business: no quiet fallback)
    with pytest.raises(ValueError):
        fmpnp.image_to_tensor_cpu(a, preprocessing="tf")
    with pytest.raises(ValueError):
        fmpnp.image_to_tensor_cpu(a, preprocessing="caffe", std=(1, 1, 1))
    with pytest.raises(ValueError):
        fmpnp.image_to_tensor_cpu(a, preprocessing=None, mean=(1, 1, 1))
    with pytest.raises(ValueError):
        fmpnp.image_to_tensor_cpu(a, preprocessing="torch", std=(1, 0, 1))
    with pytest.raises(ValueError):
        fmpnp.image_to_tensor_cpu(a, preprocessing="torch", mean=(1, 1))
    with pytest.raises(ValueError):
        fmpnp.image_loader("tf")
    with pytest.raises(_lib.FmpnpError, match="ETOOBIG"):
        fmpnp.resize_lanczos_cpu(a, (4, 16385))


def test_c_abi_error_paths():
    L = _lib.load()
    src = np.ones((8, 8, 3), np.uint8)
    dst = np.zeros((8, 8, 3), np.uint8)
    fdst = np.zeros((3, 8, 8), np.float32)
    sp, dp, fp = (ctypes.c_void_p(x.ctypes.data) for x in (src, dst, fdst))
    three = (ctypes.c_float * 3)(1, 1, 1)

    def rs(src=sp, istride=0, rstride=24, b=1, h_in=8, w_in=8, h=4, w=4, dst=dp, nt=1):
        return L.fmpnp_image_resize_u8_cpu(src, istride, rstride, b, h_in, w_in, h, w, dst, nt)

    def tt(src=sp, istride=0, rstride=24, b=1, h_in=8, w_in=8, h=4, w=4, mode=0, flags=0, mean=None, std=None, dst=fp,
           nt=1):
        return L.fmpnp_image_to_tensor_cpu(src, istride, rstride, b, h_in, w_in, h, w, mode, flags, mean, std, dst, nt)

    assert rs() == 0 and tt() == 0
    for call in (rs, tt):
        assert call(src=None) == _lib.EINVAL
        assert call(dst=None) == _lib.EINVAL
        for name in ("b", "h_in", "w_in", "h", "w"):
            assert call(**{name: 0}) == _lib.EINVAL and call(**{name: -3}) == _lib.EINVAL
        assert call(rstride=23) == _lib.EINVAL
        assert call(b=2, h_in=4, istride=4 * 24 - 1) == _lib.EINVAL  # (an image stride smaller than an image)
        assert call(b=2, h_in=4, istride=4 * 24) == 0
        assert call(nt=-1) == _lib.EINVAL
        assert call(w=16385) == _lib.ETOOBIG and call(b=16385) == _lib.ETOOBIG
        # a destination that overlaps the source, from either side
        assert call(dst=ctypes.c_void_p(src.ctypes.data + 100)) == _lib.EINVAL
        own = dst if call is rs else fdst
        assert call(src=ctypes.c_void_p(own.ctypes.data + 4)) == _lib.EINVAL
    assert tt(mode=4) == _lib.EINVAL and tt(mode=-1) == _lib.EINVAL
    assert tt(mode=_lib.IMAGE_TORCH, flags=_lib.IMAGE_SWAP_RB) == _lib.EINVAL
    assert tt(mode=_lib.IMAGE_GRAY, flags=2) == _lib.EINVAL
    assert tt(mode=_lib.IMAGE_GRAY, flags=_lib.IMAGE_SWAP_RB) == 0
    assert tt(mode=_lib.IMAGE_RAW, mean=three) == _lib.EINVAL
    assert tt(mode=_lib.IMAGE_CAFFE, std=three) == _lib.EINVAL
    assert tt(mode=_lib.IMAGE_GRAY, mean=three) == _lib.EINVAL
    assert tt(mode=_lib.IMAGE_CAFFE, mean=three) == 0 and tt(mode=_lib.IMAGE_TORCH, mean=three, std=three) == 0
    # the GPU forms validate before they touch a device: the same codes without one
    assert L.fmpnp_image_resize_u8_async(None, 0, 24, 1, 8, 8, 4, 4, dp, None) == _lib.EINVAL
    assert L.fmpnp_image_resize_u8(sp, 0, 23, 1, 8, 8, 4, 4, dp, None) == _lib.EINVAL
    assert L.fmpnp_image_to_tensor_async(sp, 0, 24, 1, 8, 8, 4, 4, 9, 0, None, None, fp, None) == _lib.EINVAL
    assert L.fmpnp_image_to_tensor(sp, 0, 24, 1, 8, 8, 0, 4, 0, 0, None, None, fp, None) == _lib.EINVAL


def test_abi():
    names = ["fmpnp_image_resize_u8_async", "fmpnp_image_resize_u8", "fmpnp_image_resize_u8_cpu",
             "fmpnp_image_to_tensor_async", "fmpnp_image_to_tensor", "fmpnp_image_to_tensor_cpu"]
    L = _lib.load()
    for n in names:
        assert n in _lib.EXPORTS and hasattr(L, n)
    assert L.fmpnp_abi_version() == 4 and _lib.ABI_VERSION == 4
    for n in ("thumbnail_size", "resize_lanczos", "resize_lanczos_cpu", "image_to_tensor", "image_to_tensor_cpu",
              "load_images", "image_loader", "superpoint_image"):
        assert callable(getattr(fmpnp, n))


def test_the_standalone_program_passes():
    """csrc/test_image_cpu.cpp's own checks (the build `make image-sanitize` runs under ASan + UBSan): the twins against
    a plain restatement, guard bytes around every output, a strided source, the error codes; by exit status."""
    subprocess.run(["make", "-s", "-C", PKG, "build/test_image_cpu"], check=True, timeout=600)
    out = subprocess.run([os.path.join(PKG, "build", "test_image_cpu")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "test_image_cpu: OK" in out.stdout, out.stdout[-2000:]
