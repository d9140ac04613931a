"""CPU-only tests of the view-image ops (C ABI moss_view_images_prepare / moss_view_images_load, moss_amd.images): the symbols,
declarations and ctypes blocks, the refusals that need no device, the torch statement against the numpy oracle of
tests/view_images_oracle.py -- every byte, no tolerance -- the identity at D = 0 / scale 1, and ``ViewImages.K`` / ``.fov`` against
the reader's arithmetic."""
import ctypes
import math
import os
import re
import threading

import numpy as np
import pytest
import torch

from tests import view_images_oracle as vo
from tests.helpers import c_layout, ctypes_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("moss_view_images_prepare", "moss_view_images_load")


def test_symbols_exported_and_declared(hip_lib):
    text = open(os.path.join(ROOT, "include", "moss_raster.h")).read()
    assert re.search(r"#define\s+MOSS_ABI_VERSION\s+7\b", text)
    from moss_amd import _lib
    assert _lib.ABI_VERSION == 7 and hip_lib.moss_abi_version() == 7
    diag = re.search(r"#ifdef MOSS_DIAG\n(.*?)#endif", text, flags=re.S).group(0)
    public = re.sub(r"/\*.*?\*/", "", text.replace(diag, ""), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, public), name
        assert hasattr(hip_lib, name), name
        assert getattr(hip_lib, name).argtypes is not None, name
    assert "} moss_view_images_prepare_args;" in public and "} moss_view_images_load_args;" in public
    for cite in ("scene/dataset_readers.py:613-654", ":361-407", ":830-868", "utils/general_utils.py:22-28", "additive in ABI 7"):
        assert cite in text, cite
    build = open(os.path.join(ROOT, "moss_amd", "build.py")).read()
    assert re.search(r'"view_images\.hip":\s*\["-ffp-contract=off"\]', build)
    import moss_amd
    from moss_amd import images
    assert moss_amd.prepare_views is images.prepare_views and moss_amd.prepare_views_torch is images.prepare_views_torch


@pytest.mark.parametrize("cname,pyname", [("moss_view_images_prepare_args", "ViewImagesPrepareArgs"),
                                          ("moss_view_images_load_args", "ViewImagesLoadArgs")])
def test_ctypes_blocks_match_the_c_layout(tmp_path, cname, pyname):
    from moss_amd import _lib
    cls = getattr(_lib, pyname)
    assert c_layout(tmp_path, cname, [f[0] for f in cls._fields_]) == ctypes_layout(cls)


def test_c_abi_refuses_bad_arguments(hip_lib):
    """Host-side validation needs no device (in a thread of its own: the error text is per thread)."""
    failures = []

    def run():
        try:
            _refusals(hip_lib)
        except BaseException as e:                                # noqa: BLE001
            failures.append(e)

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if failures:
        raise failures[0]


def _good_block():
    from moss_amd._lib import ViewImagesPrepareArgs
    a = ViewImagesPrepareArgs()
    a.num_views, a.H0, a.W0, a.scale, a.background, a.mask_mode = 2, 8, 12, 2, 0, 0
    for b in range(2):
        a.rgb[b] = a.mask[b] = a.gt_u8[b] = a.bkgd_u8[b] = 256   # (never dereferenced on the host)
        a.K[b][:] = [10.0, 0.0, 6.0, 0.0, 11.0, 4.0, 0.0, 0.0, 1.0]
    return a


def _refusals(lib):
    from moss_amd._lib import ViewImagesLoadArgs
    err = lib.moss_last_error
    prepare = lambda a: lib.moss_view_images_prepare(ctypes.byref(a), None)       # noqa: E731
    assert lib.moss_view_images_prepare(None, None) == -1 and b"moss_view_images_prepare: null argument block" in err()
    for n in (0, -1, 9):
        a = _good_block()
        a.num_views = n
        assert prepare(a) == -1 and b"num_views outside 1..8" in err(), n
    for H0, W0 in ((0, 12), (8, 0), (-8, 12)):
        a = _good_block()
        a.H0, a.W0 = H0, W0
        assert prepare(a) == -1 and b"H0 <= 0 or W0 <= 0" in err()
    a = _good_block()
    a.H0, a.W0 = 32768, 32768
    assert prepare(a) == -1 and b"must be < 2^31" in err()
    for scale in (0, 3, 8, -2):
        a = _good_block()
        a.scale = scale
        assert prepare(a) == -1 and b"scale is none of 1, 2, 4" in err(), scale
    for H0, W0, scale in ((9, 12, 2), (8, 13, 2), (8, 10, 4), (6, 12, 4)):
        a = _good_block()
        a.H0, a.W0, a.scale = H0, W0, scale
        assert prepare(a) == -1 and b"scale does not divide H0 and W0" in err(), (H0, W0, scale)
    a = _good_block()
    a.background = 2
    assert prepare(a) == -1 and b"background is neither 0 nor 1" in err()
    a = _good_block()
    a.mask_mode = 2
    assert prepare(a) == -1 and b"mask_mode is neither 0 (round) nor 1 (any)" in err()
    for field, text in (("rgb", b"null rgb or mask"), ("mask", b"null rgb or mask"), ("gt_u8", b"null gt_u8 or bkgd_u8"),
                        ("bkgd_u8", b"null gt_u8 or bkgd_u8")):
        a = _good_block()
        getattr(a, field)[1] = None
        assert prepare(a) == -1 and text in err(), field
    a = _good_block()
    a.K[1][1] = 1e-300
    assert prepare(a) == -1 and b"K[0][1] (skew) of a view is not 0" in err()
    for at, value in ((0, 0.0), (0, -10.0), (4, 0.0), (4, -1.0), (0, float("nan")), (4, float("nan"))):
        a = _good_block()
        a.K[1][at] = value
        assert prepare(a) == -1 and b"fx or fy of a view is not positive" in err(), (at, value)
    a = _good_block()
    a.num_views = 1
    a.K[1][0] = -1.0                                             # (a slot beyond num_views is not looked at: the next refusal is another)
    a.rgb[0] = None
    assert prepare(a) == -1 and b"null rgb or mask" in err()

    load = lambda b: lib.moss_view_images_load(ctypes.byref(b), None)             # noqa: E731
    assert lib.moss_view_images_load(None, None) == -1 and b"moss_view_images_load: null argument block" in err()
    b = ViewImagesLoadArgs()
    b.H, b.W = 0, 4
    assert load(b) == -1 and b"H <= 0 or W <= 0" in err()
    b.H, b.W = 32768, 32768
    assert load(b) == -1 and b"must be < 2^31" in err()
    b.H, b.W = 4, 6
    assert load(b) == -1 and b"null gt_u8 or bkgd_u8" in err()
    b.gt_u8 = b.bkgd_u8 = 257
    assert load(b) == -1 and b"null gt_image or bkgd_mask" in err()
    b.gt_image, b.bkgd_mask = 256, 258
    assert load(b) == -1 and b"not 4-byte aligned" in err()


def test_python_surface_refuses_cpu_tensors_and_bad_inputs():
    from moss_amd import images
    rgb, mask, K, D = vo.case((8, 12), 1, "zero", "round", False)[:4]
    rgb, mask = torch.from_numpy(rgb.copy()), torch.from_numpy(mask.copy())
    with pytest.raises(RuntimeError, match="needs GPU tensors.*prepare_views_torch"):
        images.prepare_views(rgb, mask, K, D)
    vi = images.prepare_views_torch(rgb, mask, K, D, scale=2)
    with pytest.raises(RuntimeError, match="needs GPU tensors"):
        vi.load(0, torch.empty(3, 4, 6), torch.empty(1, 4, 6))
    for fn in (images.prepare_views, images.prepare_views_torch):            # (what is refused before the device is looked at)
        with pytest.raises(ValueError, match="uint8"):
            fn(rgb.float(), mask, K, D)
        with pytest.raises(ValueError, match="mask must be a uint8 tensor of shape"):
            fn(rgb, mask[:3], K, D)
        with pytest.raises(ValueError, match=r"rgb must be a \(B,H0,W0,3\) tensor"):
            fn(rgb[0], mask[0], K[0], D[0])
    for fn in (images.prepare_views_torch,):
        with pytest.raises(ValueError, match="scale must be one of"):
            fn(rgb, mask, K, D, scale=3)
        with pytest.raises(ValueError, match="does not divide"):
            fn(rgb[:, :6], mask[:, :6], K, D, scale=4)
        with pytest.raises(ValueError, match="mask_mode"):
            fn(rgb, mask, K, D, mask_mode="nearest")
        with pytest.raises(ValueError, match=r"K must be \(3,3\) or"):
            fn(rgb, mask, K[:2], D)
        skew = K.copy()
        skew[4, 0, 1] = 0.5
        with pytest.raises(ValueError, match="skew"):
            fn(rgb, mask, skew, D)
        flat = K.copy()
        flat[7, 1, 1] = 0.0
        with pytest.raises(ValueError, match="positive"):
            fn(rgb, mask, flat, D)


def _compare(tag, vi, gt, bkgd, B):
    assert vi.gt_u8.dtype == vi.bkgd_u8.dtype == torch.uint8
    assert tuple(vi.gt_u8.shape) == (B,) + gt.shape[1:] and tuple(vi.bkgd_u8.shape) == (B,) + bkgd.shape[1:]
    got_gt, got_bk = vi.gt_u8.cpu().numpy(), vi.bkgd_u8.cpu().numpy()
    bad_gt, bad_bk = int((got_gt != gt[:B]).sum()), int((got_bk != bkgd[:B]).sum())
    assert bad_gt == 0 and bad_bk == 0, f"{tag}: {bad_gt} colour bytes and {bad_bk} mask bytes differ from the oracle"


@pytest.mark.parametrize("lens_name", vo.LENSES)
@pytest.mark.parametrize("size", vo.SIZES)
def test_torch_statement_equals_the_oracle(size, lens_name):
    from moss_amd.images import prepare_views_torch
    for scale in vo.scales_of(size):
        for mode in ("round", "any"):
            for white in (False, True):
                rgb, mask, K, D, gt, bkgd, counts = vo.case(size, scale, lens_name, mode, white)
                if lens_name == "strong":
                    assert min(counts[k] for k in ("left", "right", "top", "bottom")) > 0, counts
                if mode == "round":
                    assert set(np.unique(bkgd)) <= {0, 255}
                assert 0 < int((bkgd != 0).sum()) < bkgd.size
                for B in (1, 3, 9):
                    vi = prepare_views_torch(torch.from_numpy(rgb[:B].copy()), torch.from_numpy(mask[:B].copy()), K[:B], D[:B], scale=scale,
                                             white_background=white, mask_mode=mode)
                    _compare((size, scale, lens_name, mode, white, B), vi, gt, bkgd, B)
                    assert vi.nbytes == 4 * B * (size[0] // scale) * (size[1] // scale)


def test_half_pixel_centre_and_the_exact_half_tie():
    """A principal point on half-integers with zero distortion against a checkerboard mask.  Under the contract's map a lens without
    distortion samples every pixel at itself wherever the principal point lies (su = fx ((u - cx) / fx) + cx = u to far within 1/64):
    ax = ay = 0 and the rounding rule meets no tie -- asserted, so that the case is not taken for more than it is.  The ties come with
    the mild distortion over the same checkerboard: every sample with ax = 16 or ay = 16 has exactly half its weight on foreground
    taps.  Asserted too, and the torch statement rounds them up as the oracle does."""
    from moss_amd.images import prepare_views_torch
    size = (64, 48)
    for lens_name, tied in (("zero", False), ("mild", True)):
        for scale in (1, 2):
            rgb, mask, K, D, gt, bkgd, counts = vo.case(size, scale, lens_name, "round", False, B=3, half_pixel_centre=True, checkerboard=True)
            assert (counts["ties"] > 100) if tied else (counts["ties"] == 0), counts
            vi = prepare_views_torch(torch.from_numpy(rgb.copy()), torch.from_numpy(mask.copy()), K, D, scale=scale)
            _compare((lens_name, scale), vi, gt, bkgd, 3)


def test_identity_without_distortion_at_scale_one():
    """D = 0, scale = 1, mask all foreground: ``gt_u8`` is the input, because trunc((k / 255.f) * 255.f) == k for all 256 bytes."""
    from moss_amd.images import prepare_views_torch
    k = np.arange(256, dtype=np.float32)
    assert np.array_equal(np.trunc((k / np.float32(255)) * np.float32(255)), k)
    unit = torch.arange(256, dtype=torch.float32) / 255.0
    assert torch.equal((unit * 255).to(torch.uint8), torch.arange(256, dtype=torch.uint8))
    rgb, _, K, D = vo.case((36, 52), 1, "zero", "round", False)[:4]
    rgb = torch.from_numpy(rgb[:3].copy())
    rgb[0].view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
    mask = torch.full(rgb.shape[:3], 7, dtype=torch.uint8)
    for mode in ("round", "any"):
        vi = prepare_views_torch(rgb, mask, K[:3], None, scale=1, white_background=True, mask_mode=mode)
        assert torch.equal(vi.gt_u8, rgb.permute(0, 3, 1, 2))
        want = 255 if mode == "round" else int(np.trunc(np.float32(7) / np.float32(255) * np.float32(255)))
        assert bool((vi.bkgd_u8 == want).all())
        for i in range(3):
            assert torch.equal(vi.original_image(i), vi.gt_u8[i].float() / 255.0)
            assert torch.equal(vi.bkgd_mask(i), vi.bkgd_u8[i].float().reshape(1, 36, 52) / 255.0)
            assert vi.original_image(i).dtype == torch.float32 and vi.original_image(i).data_ptr() != vi.original_image(i).data_ptr()


def test_scaled_intrinsics_and_fov_are_the_readers():
    """dataset_readers.py:652,656-659 and utils/graphics_utils.py:108-109, written out."""
    from moss_amd.images import prepare_views_torch
    H0, W0 = 36, 52
    rgb, mask, K, D = vo.case((H0, W0), 2, "mild", "round", False)[:4]
    for scale, ratio in ((1, 1.0), (2, 0.5), (4, 0.25)):
        vi = prepare_views_torch(torch.from_numpy(rgb.copy()), torch.from_numpy(mask.copy()), K, D, scale=scale)
        assert vi.K.dtype == np.float64 and vi.K.shape == (9, 3, 3) and (vi.H, vi.W) == (int(H0 * ratio), int(W0 * ratio)) and len(vi) == 9
        for i in range(9):
            k = np.array(K[i])
            k[:2] = k[:2] * ratio
            assert np.array_equal(vi.K[i], k)
            fov = (2 * math.atan(vi.W / (2 * k[0, 0])), 2 * math.atan(vi.H / (2 * k[1, 1])))
            assert vi.fov(i) == fov
    once = prepare_views_torch(torch.from_numpy(rgb.copy()), torch.from_numpy(mask.copy()), K[2], D[2].reshape(5, 1), scale=2)
    each = prepare_views_torch(torch.from_numpy(rgb.copy()), torch.from_numpy(mask.copy()), np.repeat(K[2:3], 9, 0), np.repeat(D[2:3], 9, 0), scale=2)
    assert torch.equal(once.gt_u8, each.gt_u8) and torch.equal(once.bkgd_u8, each.bkgd_u8) and np.array_equal(once.K, each.K)
