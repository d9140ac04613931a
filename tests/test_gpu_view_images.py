"""The view-image kernels (csrc/view_images.hip) on the MI355X against the numpy oracle of tests/view_images_oracle.py: every byte
equal, no tolerance, no excluded pixel.  Sizes 8 x 12, 36 x 52 (the factor 4: 13 output columns, 117 output pixels -- no multiple of a
wave, of four, of anything) and 64 x 48; 1, 3 and 9 views (9 crosses the chunk of eight); both mask rules, both backgrounds; no, mild
and strong distortion (the strong one sends border samples outside on all four sides: asserted); the exact-half tie of the rounding
rule; ``load`` bit for bit, eager and replayed from a graph; poisoned allocator memory; inputs and outputs at odd byte addresses."""
import ctypes

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import view_images_oracle as vo

pytestmark = pytest.mark.gpu


def _dev(a, gpu):
    return torch.from_numpy(a.copy()).to(gpu)


def _compare(tag, vi, gt, bkgd, B):
    assert vi.gt_u8.dtype == vi.bkgd_u8.dtype == torch.uint8 and vi.gt_u8.is_cuda and vi.bkgd_u8.is_cuda
    assert tuple(vi.gt_u8.shape) == (B,) + gt.shape[1:] and tuple(vi.bkgd_u8.shape) == (B,) + bkgd.shape[1:]
    got_gt, got_bk = vi.gt_u8.cpu().numpy(), vi.bkgd_u8.cpu().numpy()
    bad_gt, bad_bk = int((got_gt != gt[:B]).sum()), int((got_bk != bkgd[:B]).sum())
    print(f"{tag}: {bad_gt} of {got_gt.size} colour bytes and {bad_bk} of {got_bk.size} mask bytes differ")
    assert bad_gt == 0 and bad_bk == 0, f"{tag}: {bad_gt} colour bytes and {bad_bk} mask bytes differ from the oracle"


@pytest.mark.parametrize("lens_name", vo.LENSES)
@pytest.mark.parametrize("size", vo.SIZES)
def test_prepare_equals_the_oracle(gpu, hip_lib, size, lens_name):
    from moss_amd.images import prepare_views
    for scale in vo.scales_of(size):
        for mode in ("round", "any"):
            for white in (False, True):
                rgb, mask, K, D, gt, bkgd, counts = vo.case(size, scale, lens_name, mode, white)
                if lens_name == "strong":
                    assert min(counts[k] for k in ("left", "right", "top", "bottom")) > 0, counts
                rgb_d, mask_d = _dev(rgb, gpu), _dev(mask, gpu)
                for B in (1, 3, 9):
                    vi = prepare_views(rgb_d[:B], mask_d[:B], K[:B], D[:B], scale=scale, white_background=white, mask_mode=mode)
                    _compare((size, scale, lens_name, mode, white, B), vi, gt, bkgd, B)
                    assert vi.nbytes == 4 * B * (size[0] // scale) * (size[1] // scale) and (vi.H, vi.W) == (size[0] // scale, size[1] // scale)


def test_half_pixel_centre_and_the_exact_half_tie(gpu, hip_lib):
    """The checkerboard mask under a principal point on half-integers: without distortion (every sample on its pixel: no tie, see the
    CPU test of the same name) and with the mild distortion, where every sample with ax = 16 or ay = 16 is an exact-half tie --
    asserted -- that the kernel must round up as the oracle does."""
    from moss_amd.images import prepare_views
    size = (64, 48)
    for lens_name, tied in (("zero", False), ("mild", True)):
        for scale in (1, 2):
            rgb, mask, K, D, gt, bkgd, counts = vo.case(size, scale, lens_name, "round", False, B=3, half_pixel_centre=True, checkerboard=True)
            assert (counts["ties"] > 100) if tied else (counts["ties"] == 0), counts
            vi = prepare_views(_dev(rgb, gpu), _dev(mask, gpu), K, D, scale=scale)
            _compare((lens_name, scale, "ties", counts["ties"]), vi, gt, bkgd, 3)


def test_identity_and_one_lens_for_all_views(gpu, hip_lib):
    """D = None, scale 1, a mask that is foreground everywhere: the image comes back as it went in; K / D given once serve every view."""
    from moss_amd.images import prepare_views, prepare_views_torch
    rgb, mask, K, D = vo.case((36, 52), 1, "mild", "any", False)[:4]
    rgb_d, mask_d = _dev(rgb, gpu), _dev(mask, gpu)
    vi = prepare_views(rgb_d, torch.full_like(mask_d, 3), K[0], None, scale=1, white_background=True, mask_mode="any")
    assert torch.equal(vi.gt_u8, rgb_d.permute(0, 3, 1, 2))
    once = prepare_views(rgb_d, mask_d, K[2], D[2].reshape(5, 1), scale=2, mask_mode="any")
    want = prepare_views_torch(torch.from_numpy(rgb.copy()), torch.from_numpy(mask.copy()), K[2], D[2], scale=2, mask_mode="any")
    assert torch.equal(once.gt_u8.cpu(), want.gt_u8) and torch.equal(once.bkgd_u8.cpu(), want.bkgd_u8) and np.array_equal(once.K, want.K)
    with pytest.raises(ValueError, match="contiguous"):
        prepare_views(rgb_d.permute(0, 2, 1, 3), mask_d.permute(0, 2, 1), K, D, scale=2)
    with pytest.raises(ValueError, match="does not divide"):
        prepare_views(rgb_d[:, :, :50].contiguous(), mask_d[:, :, :50].contiguous(), K, D, scale=4)


@pytest.mark.parametrize("size,scale", [((64, 48), 2), ((36, 52), 4), ((8, 12), 1)])
def test_load_is_the_division_bit_for_bit_eager_and_replayed(gpu, hip_lib, size, scale):
    """``load`` against ``torch.from_numpy(u8) / 255.0`` -- eager, then replayed from a graph after the packed bytes were overwritten in
    place (every byte value is among the new ones) -- and the fresh tensors of ``original_image`` / ``bkgd_mask``."""
    from moss_amd.graphs import capturing
    from moss_amd.images import prepare_views
    rgb, mask, K, D, gt, bkgd, _ = vo.case(size, scale, "mild", "any", True)
    vi = prepare_views(_dev(rgb, gpu)[:3], _dev(mask, gpu)[:3], K[:3], D[:3], scale=scale, white_background=True, mask_mode="any")
    H, W = vi.H, vi.W
    gt_image, bkgd_mask = torch.full((3, H, W), -1.0, device=gpu), torch.full((1, H, W), -1.0, device=gpu)

    def check(i, gt_bytes, bkgd_bytes):
        want_gt, want_bk = torch.from_numpy(gt_bytes.copy()) / 255.0, torch.from_numpy(bkgd_bytes.copy()).reshape(1, H, W) / 255.0
        assert want_gt.dtype == torch.float32
        assert torch.equal(gt_image.cpu().view(torch.int32), want_gt.view(torch.int32)), i
        assert torch.equal(bkgd_mask.cpu().view(torch.int32), want_bk.view(torch.int32)), i
    for i in range(3):
        back = vi.load(i, gt_image, bkgd_mask)
        assert back[0] is gt_image and back[1] is bkgd_mask
        check(i, gt[i], bkgd[i])
        fresh = vi.original_image(i), vi.bkgd_mask(i)
        assert fresh[0].data_ptr() != gt_image.data_ptr() and tuple(fresh[0].shape) == (3, H, W) and tuple(fresh[1].shape) == (1, H, W)
        assert torch.equal(fresh[0], gt_image) and torch.equal(fresh[1], bkgd_mask)
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    with capturing(graph, collect=True):
        vi.load(1, gt_image, bkgd_mask)
    rng = np.random.Generator(np.random.PCG64(5))
    for _ in range(2):
        new_gt = rng.integers(0, 256, size=(3, H, W), dtype=np.uint8)
        new_gt.reshape(-1)[:256 if new_gt.size >= 256 else new_gt.size] = np.arange(256, dtype=np.uint8)[:new_gt.size]
        new_bk = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
        vi.gt_u8[1].copy_(torch.from_numpy(new_gt).to(gpu))
        vi.bkgd_u8[1].copy_(torch.from_numpy(new_bk).to(gpu))
        gt_image.fill_(-1.0)
        bkgd_mask.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize(gpu)
        check("replay", new_gt, new_bk)
    with pytest.raises(ValueError, match="gt_image"):
        vi.load(0, gt_image.double(), bkgd_mask)
    with pytest.raises(ValueError, match="bkgd_mask"):
        vi.load(0, gt_image, torch.empty(1, H, W + 1, device=gpu))


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_every_output_byte_is_written_on_poisoned_memory(gpu, hip_lib, byte):
    """``prepare`` (packed stores at 64 x 48 / 2, byte stores at 36 x 52 / 4; 9 views: two launches) and ``load`` with their outputs
    taken from an allocator whose every block holds ``byte``: the results are the oracle's, so nothing was left as it was found."""
    from moss_amd.images import prepare_views
    for size, scale in (((64, 48), 2), ((36, 52), 4)):
        rgb, mask, K, D, gt, bkgd, _ = vo.case(size, scale, "strong", "any", byte == 0x00)
        rgb_d, mask_d = _dev(rgb, gpu), _dev(mask, gpu)                  # (inputs: made before the seeding, outside the poison)
        with hp.poisoned_allocator(gpu, byte) as poison:
            vi = prepare_views(rgb_d, mask_d, K, D, scale=scale, white_background=byte == 0x00, mask_mode="any")
            gt_image = torch.empty((3, vi.H, vi.W), dtype=torch.float32, device=gpu)
            bkgd_mask = torch.empty((1, vi.H, vi.W), dtype=torch.float32, device=gpu)
            vi.load(8, gt_image, bkgd_mask)
            poison.assert_owns(vi.gt_u8, vi.bkgd_u8, gt_image, bkgd_mask)
            torch.cuda.synchronize(gpu)
            host = vi.gt_u8.cpu().numpy(), vi.bkgd_u8.cpu().numpy(), gt_image.cpu(), bkgd_mask.cpu()
            del vi, gt_image, bkgd_mask
        assert np.array_equal(host[0], gt) and np.array_equal(host[1], bkgd), (size, scale)
        assert torch.equal(host[2].view(torch.int32), (torch.from_numpy(gt[8].copy()) / 255.0).view(torch.int32))
        assert torch.equal(host[3].view(torch.int32), (torch.from_numpy(bkgd[8].copy()).reshape(host[3].shape) / 255.0).view(torch.int32))


@pytest.mark.parametrize("size,scale", [((36, 52), 2), ((64, 48), 1), ((36, 52), 4)])
def test_odd_byte_addresses(gpu, hip_lib, size, scale):
    """``rgb`` and ``mask`` views whose storage starts 1 and 3 bytes into an allocation (the fall-back from the wide loads), through the
    Python surface; then the C entry points on outputs at odd addresses between guard bytes: exactly the output bytes are written."""
    from moss_amd._lib import ViewImagesLoadArgs, ViewImagesPrepareArgs, call
    from moss_amd.images import MASK_MODES, prepare_views
    H0, W0 = size
    B = 3
    for mode in ("round", "any"):
        rgb, mask, K, D, gt, bkgd, _ = vo.case(size, scale, "mild", mode, False)
        n_rgb, n_mask = B * H0 * W0 * 3, B * H0 * W0
        for o_rgb, o_mask in ((1, 3), (2, 1), (4, 4)):
            store_rgb = torch.zeros(n_rgb + 8, dtype=torch.uint8, device=gpu)
            store_mask = torch.zeros(n_mask + 8, dtype=torch.uint8, device=gpu)
            rgb_v = store_rgb[o_rgb:o_rgb + n_rgb].view(B, H0, W0, 3)
            mask_v = store_mask[o_mask:o_mask + n_mask].view(B, H0, W0)
            rgb_v.copy_(_dev(rgb[:B], gpu))
            mask_v.copy_(_dev(mask[:B], gpu))
            assert rgb_v.data_ptr() % 4 == o_rgb % 4 and mask_v.data_ptr() % 4 == o_mask % 4
            vi = prepare_views(rgb_v, mask_v, K[:B], D[:B], scale=scale, mask_mode=mode)
            _compare((size, scale, mode, o_rgb, o_mask), vi, gt, bkgd, B)
        # outputs at odd addresses, guard bytes all around
        H, W = H0 // scale, W0 // scale
        n = H * W
        guard = 0xAB
        for o_gt, o_bk in ((1, 3), (4, 2), (8, 8)):
            buf_gt = torch.full((B, 3 * n + 16), guard, dtype=torch.uint8, device=gpu)
            buf_bk = torch.full((B, n + 16), guard, dtype=torch.uint8, device=gpu)
            a = ViewImagesPrepareArgs()
            a.num_views, a.H0, a.W0, a.scale, a.background, a.mask_mode = B, H0, W0, scale, 0, MASK_MODES.index(mode)
            for b in range(B):
                a.rgb[b], a.mask[b] = rgb_v[b].data_ptr(), mask_v[b].data_ptr()
                a.gt_u8[b], a.bkgd_u8[b] = buf_gt[b].data_ptr() + o_gt, buf_bk[b].data_ptr() + o_bk
                a.K[b][:] = K[b].reshape(-1).tolist()
                a.D[b][:] = D[b].tolist()
            call("moss_view_images_prepare", gpu, ctypes.byref(a))
            got_gt, got_bk = buf_gt.cpu().numpy(), buf_bk.cpu().numpy()
            assert np.array_equal(got_gt[:, o_gt:o_gt + 3 * n].reshape(B, 3, H, W), gt[:B]), (mode, o_gt)
            assert np.array_equal(got_bk[:, o_bk:o_bk + n].reshape(B, H, W), bkgd[:B]), (mode, o_bk)
            assert (got_gt[:, :o_gt] == guard).all() and (got_gt[:, o_gt + 3 * n:] == guard).all(), (mode, o_gt)
            assert (got_bk[:, :o_bk] == guard).all() and (got_bk[:, o_bk + n:] == guard).all(), (mode, o_bk)
            # load from those bytes into floats between guard words
            out_gt = torch.full((3 * n + 8,), -7.0, device=gpu)
            out_bk = torch.full((n + 8,), -7.0, device=gpu)
            for o_f in (1, 4):
                la = ViewImagesLoadArgs()
                la.H, la.W = H, W
                la.gt_u8, la.bkgd_u8 = buf_gt[1].data_ptr() + o_gt, buf_bk[1].data_ptr() + o_bk
                la.gt_image, la.bkgd_mask = out_gt.data_ptr() + 4 * o_f, out_bk.data_ptr() + 4 * o_f
                out_gt.fill_(-7.0)
                out_bk.fill_(-7.0)
                call("moss_view_images_load", gpu, ctypes.byref(la))
                f_gt, f_bk = out_gt.cpu(), out_bk.cpu()
                assert torch.equal(f_gt[o_f:o_f + 3 * n].view(torch.int32), (torch.from_numpy(gt[1].copy()).reshape(-1) / 255.0).view(torch.int32))
                assert torch.equal(f_bk[o_f:o_f + n].view(torch.int32), (torch.from_numpy(bkgd[1].copy()).reshape(-1) / 255.0).view(torch.int32))
                assert bool((f_gt[:o_f] == -7.0).all()) and bool((f_gt[o_f + 3 * n:] == -7.0).all())
                assert bool((f_bk[:o_f] == -7.0).all()) and bool((f_bk[o_f + n:] == -7.0).all())
