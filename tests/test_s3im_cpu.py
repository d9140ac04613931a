"""CPU tests of the S3IM term's torch form (moss_amd.loss.s3im, the yardstick of the HIP kernels of csrc/s3im.hip) and of the MOSS-side
patch that switches train_ZJU.py:123 to the fused form."""
import os

import numpy as np
import pytest
import torch

from moss_amd.loss import s3im, s3im_fused, s3im_loss_roi_fused, ssim
from tests import helpers as hp
from tests.test_host_cpu import _apply_exactly, _diff_hunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "s3im.npz")


def _case(g, name):
    src = torch.from_numpy(g[f"{name}_src_q"]).double() / 128.0
    tar = torch.from_numpy(g[f"{name}_tar_q"]).double() / 128.0
    return src, tar


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
@pytest.mark.parametrize("R", [10, 3])
def test_s3im_matches_the_reference_golden(name, R):
    """moss_amd.loss.s3im in float64 against the reference's own s3im_fun (tests/golden/s3im.npz, utils/loss_utils.py:17-38): the value
    to 1e-12, the gradient w.r.t. the source to float32 rounding of the stored gradient."""
    g = np.load(GOLDEN)
    src, tar = _case(g, name)
    a = src.unsqueeze(0).requires_grad_(True)
    v = s3im(a, tar.unsqueeze(0), repeat_time=R)
    v.backward()
    assert abs(float(v.detach()) - float(g[f"{name}_value_r{R}"])) < 1e-12
    grad = a.grad[0].numpy()
    if name == "e":
        grad = grad[:, g["e_grad_rows"]]
    assert hp.rel_err(grad, g[f"{name}_grad_r{R}"]) < 1e-6


@pytest.mark.parametrize("shape,R", [((3, 37, 23), 10), ((3, 64, 41), 10), ((3, 5, 3), 10), ((1, 9, 14), 1), ((2, 11, 7), 16)])
def test_s3im_at_batch_one_is_ssim_of_the_repeated_crop_and_draws_nothing(shape, R):
    """At batch 1 (MOSS's call) every permutation is [0]: s3im == 1 - ssim(repeat_interleave(R, -1)), value and gradient, and the
    default generator's state is untouched (randperm(1) draws nothing)."""
    g = torch.Generator().manual_seed(sum(shape) * R)
    src = torch.rand(1, *shape, generator=g, dtype=torch.float64); tar = torch.rand(1, *shape, generator=g, dtype=torch.float64)
    a = src.clone().requires_grad_(True); b = src.clone().requires_grad_(True)
    state = torch.random.get_rng_state()
    v = s3im(a, tar, repeat_time=R)
    assert torch.equal(state, torch.random.get_rng_state())
    ref = 1.0 - ssim(b.repeat_interleave(R, -1), tar.repeat_interleave(R, -1))
    v.backward(); ref.backward()
    assert abs(float(v.detach()) - float(ref.detach())) < 1e-14
    assert float((a.grad - b.grad).abs().max()) < 1e-15


def test_s3im_at_batch_two_draws_like_the_reference():
    """At batch 2 the reference draws repeat_time - 1 permutations of torch.randperm(2) from the default generator and its reshape to
    one (1, C, h, w R) image then fails (twice the elements).  s3im draws the same numbers -- the caller's RNG stream advances exactly as
    with the reference -- and raises a RuntimeError as well; so does s3im_fused, which hands a batch > 1 to s3im."""
    src = torch.rand(2, 3, 6, 5, dtype=torch.float64); tar = torch.rand(2, 3, 6, 5, dtype=torch.float64)
    for R in (10, 3):
        torch.manual_seed(7)
        for _ in range(R - 1):
            torch.randperm(2)
        expected = torch.random.get_rng_state()
        for fn in (s3im, s3im_fused):
            torch.manual_seed(7)
            with pytest.raises(RuntimeError):
                fn(src, tar, repeat_time=R)
            assert torch.equal(torch.random.get_rng_state(), expected)


def test_s3im_fused_refuses_cpu_tensors():
    """The product path has no CPU fallback: CPU tensors are refused (the torch form is moss_amd.loss.s3im)."""
    a = torch.rand(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        s3im_fused(a, a)
    with pytest.raises(RuntimeError, match="GPU"):
        s3im_loss_roi_fused(a[0], a[0], None)


def test_s3im_patch_applies_after_its_two_predecessors():
    """patches/train_ZJU_s3im.diff applies exactly (each hunk at its line, no fuzz) on top of train_ZJU.diff and
    train_ZJU_one_call_loss.diff, replaces MOSS's s3im_fun call by the fused form on the full frames, keeps the crops LPIPS reads, and
    calls s3im_loss_roi_fused with the argument names it has."""
    import inspect
    text = []
    for name in ("train_ZJU.diff", "train_ZJU_one_call_loss.diff", "train_ZJU_s3im.diff"):
        target, hunks = _diff_hunks(os.path.join(ROOT, "patches", name))
        assert target == "train_ZJU.py"
        text = _apply_exactly(text, hunks)
    src = "\n".join(s for s in text if s is not None)
    assert "s3im_loss = s3im_loss_roi_fused(image, gt_image, viewpoint_cam.moss_region)" in src
    assert "from moss_amd.loss import s3im_loss_roi_fused" in src
    assert "s3im_loss = s3im_fun(" not in src
    assert "lpips_loss = loss_fn_vgg(img_pred, img_gt)" in src and "img_pred = image[:, y:y + h, x:x + w]" in src
    assert list(inspect.signature(s3im_loss_roi_fused).parameters)[:3] == ["image", "gt_image", "region"]
