#!/usr/bin/env python3
"""Generates tests/golden/eval_metrics.npz by IMPORTING the reference's own metric functions from a MOSS checkout (make_golden.py, the
other fixtures' generator, is separate and unchanged).

    python tests/golden/make_golden_eval.py <path of a MOSS checkout>

Reference functions exercised, on the CPU, composed exactly as train_ZJU.py:244-253 (training_report) composes them:
  utils/image_utils.py  psnr (:19-21)
  utils/loss_utils.py   l1_loss (:41-42), ssim (:57-87)

    image = torch.clamp(render, 0.0, 1.0)
    gt_image = torch.clamp(gt, 0.0, 1.0)
    image.permute(1,2,0)[bound_mask[0]==0] = 0 if bg.sum().item() == 0 else 1
    l1_test += l1_loss(image, gt_image).mean().double()      (psnr_test, ssim_test alike)

Three sets of views -- the views of one set share a size and a background, as a split does -- keyed <set>_<name>:
  a: 97 x 131 (odd), black background, 6 views: partial / no / all-zero masks; both images reach outside [0, 1]
  b: 64 x 48, white background, 5 views: the same kinds of mask
  c: 256 x 256, white background, 2 views: a partial mask; a render identical to its ground truth (PSNR = +inf)
Per set: image_q, gt_q (N,3,H,W) uint8 -- the images are on a grid of 1/128 and the float32 values are EXACTLY q / 128 - 0.25
(every step exact; [-0.25, 1.25]: the fixture compresses to a few hundred KB); bound (N,H,W) uint8 (the bound_mask; all ones where
has_bound is 0: that view is evaluated without a mask); bg (3,); per view l1, psnr, ssim (N,) float32 = the reference's tensors; mean_l1, mean_psnr, mean_ssim float64 = the
reference's double accumulation / N.
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
QMAX = 192                                  # q / 128 - 0.25 spans [-0.25, 1.25]


def quantize(v):
    """The grid point nearest to v (clipped to the grid's range): (int q, the float32 image q / 128 - 0.25, exact)."""
    q = torch.clamp(torch.round((v + 0.25) * 128.0), 0, QMAX).to(torch.int32)
    return q, q.to(torch.float32) / 128.0 - 0.25


def _view(g, H, W, bg, kind):
    """A render-like pair: a textured blob on the background, the render a noisy version of the ground truth, both stretched past
    [0, 1] in places; the mask a box around the blob ("partial"), nothing ("zero") or everything ("none")."""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    cy, cx = H * (0.4 + 0.2 * float(torch.rand(1, generator=g))), W * (0.4 + 0.2 * float(torch.rand(1, generator=g)))
    blob = (((yy - cy) / (0.3 * H)) ** 2 + ((xx - cx) / (0.25 * W)) ** 2 < 1.0).float()
    # (texture and noise on a grid of 1/32: fewer distinct values per pixel, a smaller fixture; the images are on the 1/128 grid)
    tex = torch.round(torch.rand(3, H, W, generator=g) * 1.4 * 32) / 32 - 0.2
    bgv = torch.tensor(bg, dtype=torch.float32).view(3, 1, 1)
    gt = blob * tex + (1 - blob) * bgv
    gt = gt + (torch.rand(3, H, W, generator=g) < 0.01).float() * 0.5             # a few out-of-range specks on the background too
    image = gt + blob * torch.round(0.15 * 32 * torch.randn(3, H, W, generator=g)) / 32
    image = image - (torch.rand(3, H, W, generator=g) < 0.01).float() * 0.7
    _, gt = quantize(gt)
    _, image = quantize(image)
    bound = torch.ones(H, W, dtype=torch.uint8)
    if kind == "partial":
        y0, y1 = int(max(cy - 0.35 * H, 0)), int(min(cy + 0.35 * H, H))
        x0, x1 = int(max(cx - 0.3 * W, 0)), int(min(cx + 0.3 * W, W))
        bound = torch.zeros(H, W, dtype=torch.uint8)
        bound[y0:y1, x0:x1] = 1
    elif kind == "zero":
        bound = torch.zeros(H, W, dtype=torch.uint8)
    elif kind == "identical":
        image = gt.clone()
    return image, gt, bound, kind in ("partial", "zero")


def _reference_metrics(image, gt, bound, has_bound, bg):
    """train_ZJU.py:244-253 on one view, the reference's functions (CPU)."""
    image = torch.clamp(image, 0.0, 1.0)
    gt_image = torch.clamp(gt, 0.0, 1.0)
    if has_bound:
        bound_mask = bound.float()[None]                                          # (1,H,W), as viewpoint.bound_mask
        image.permute(1, 2, 0)[bound_mask[0] == 0] = 0 if torch.tensor(bg).sum().item() == 0 else 1
    return l1_loss(image, gt_image).mean(), psnr(image, gt_image).mean(), ssim(image, gt_image).mean()


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    global psnr, l1_loss, ssim
    from utils.image_utils import psnr
    from utils.loss_utils import l1_loss, ssim
    g = torch.Generator().manual_seed(20261015)
    sets = {"a": (97, 131, [0.0, 0.0, 0.0], ["partial", "none", "zero", "partial", "partial", "none"]),
            "b": (64, 48, [1.0, 1.0, 1.0], ["partial", "zero", "none", "partial", "partial"]),
            "c": (256, 256, [1.0, 1.0, 1.0], ["partial", "identical"])}
    out = {}
    for key, (H, W, bg, kinds) in sets.items():
        imgs, gts, bounds, has, m = [], [], [], [], []
        l1_test = psnr_test = ssim_test = 0.0
        for kind in kinds:
            image, gt, bound, hb = _view(g, H, W, bg, kind)
            l1, p, s = _reference_metrics(image.clone(), gt.clone(), bound, hb, bg)
            l1_test += l1.double()
            psnr_test += p.double()
            ssim_test += s.double()
            (qi, fi), (qg, fg) = quantize(image), quantize(gt)
            assert torch.equal(fi, image) and torch.equal(fg, gt)              # (the stored grid IS what the reference was given)
            imgs.append(qi.numpy()); gts.append(qg.numpy()); bounds.append(bound.numpy()); has.append(int(hb))
            m.append((l1.item(), p.item(), s.item()))
        n = len(kinds)
        out[f"{key}_image_q"] = np.stack(imgs).astype(np.uint8)
        out[f"{key}_gt_q"] = np.stack(gts).astype(np.uint8)
        out[f"{key}_bound"] = np.stack(bounds).astype(np.uint8)
        out[f"{key}_has_bound"] = np.array(has, dtype=np.uint8)
        out[f"{key}_bg"] = np.array(bg, dtype=np.float32)
        for j, name in enumerate(("l1", "psnr", "ssim")):
            out[f"{key}_{name}"] = np.array([v[j] for v in m], dtype=np.float32)
        out[f"{key}_mean_l1"] = np.float64((l1_test / n).item())
        out[f"{key}_mean_psnr"] = np.float64((psnr_test / n).item())
        out[f"{key}_mean_ssim"] = np.float64((ssim_test / n).item())
        print(key, H, W, kinds, [tuple(round(x, 6) for x in v) for v in m])
    np.savez_compressed(os.path.join(OUT, "eval_metrics.npz"), **out)


if __name__ == "__main__":
    main()
