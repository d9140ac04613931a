#!/usr/bin/env python3
"""Time per view of the evaluation metrics (L1, PSNR, SSIM of MOSS's training_report, train_ZJU.py:244-253; LPIPS excluded): the torch
composition the reference runs per view -- clamp, boolean-mask fill with its host read, l1 / psnr / ssim, three `.double()` adds -- against
moss_amd.metrics.QualityReport (two HIP kernels per call of up to eight views, sums on the device).  512^2 and 1024^2, B = 1 and B = 8
views per call; device-synchronised wall time over many repetitions after a warm-up.  Also prints the bytes each view moves and the
share of HBM bandwidth that is.

    python scripts/eval_metrics_times.py [--reps 50] [--json eval_metrics_times.json]

For the per-kernel picture run it under `rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python scripts/eval_metrics_times.py --reps 20`.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from moss_amd.loss import ViewRegion, l1_loss, ssim  # noqa: E402
from moss_amd.metrics import QualityReport  # noqa: E402

HBM_BYTES_PER_S = 8.0e12            # MI355X peak HBM3E bandwidth (MI355X_MICROARCH: 8 TB/s)


def torch_report(views, bg):
    """The reference's per-view lines, literally (train_ZJU.py:244-253 without LPIPS)."""
    l1_test = psnr_test = ssim_test = 0.0
    for render, gt, mask in views:
        image = torch.clamp(render, 0.0, 1.0)
        gt_image = torch.clamp(gt, 0.0, 1.0)
        image.permute(1, 2, 0)[mask[0] == 0] = 0 if bg.sum().item() == 0 else 1
        l1_test += l1_loss(image, gt_image).mean().double()
        mse = ((image - gt_image) ** 2).view(image.shape[0], -1).mean(1, keepdim=True)
        psnr_test += (20 * torch.log10(1.0 / torch.sqrt(mse))).mean().double()
        ssim_test += ssim(image, gt_image).mean().double()
    return l1_test, psnr_test, ssim_test


def timed(fn, reps, dev):
    fn()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    dev = torch.device("cuda:0")
    bg = torch.zeros(3, device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    rows = []
    for S in (512, 1024):
        views = []
        for i in range(8):
            gt = torch.rand(3, S, S, device=dev, generator=g)
            render = gt + 0.1 * torch.randn(3, S, S, device=dev, generator=g)
            mask = torch.zeros(1, S, S, device=dev)
            mask[:, S // 8:S - S // 8, S // 4:S - S // 4] = 1
            views.append((render.contiguous(), gt.contiguous(), mask))
        regions = [ViewRegion(m) for _, _, m in views]
        rep = QualityReport(dev, 3, S, S, bg)
        # bytes per view that the kernels must move: render + gt read (fp32), the mask (1 B per pixel); workspace traffic is < 1 %
        bytes_view = 3 * S * S * 4 * 2 + S * S
        for B in (1, 8):
            vs = views[:B]
            t_torch = timed(lambda: torch_report(vs, bg), a.reps, dev) / B
            items = [(r, gt, reg) for (r, gt, _), reg in zip(vs, regions)]
            t_kern = timed(lambda: rep.add_many(items), a.reps, dev) / B
            row = {"size": S, "B": B, "torch_us_per_view": round(t_torch * 1e6, 1), "kernel_us_per_view": round(t_kern * 1e6, 1),
                   "bytes_per_view": bytes_view, "kernel_hbm_fraction": round(bytes_view / t_kern / HBM_BYTES_PER_S, 4),
                   "speedup": round(t_torch / t_kern, 1)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
