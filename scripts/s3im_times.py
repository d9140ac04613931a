"""MOSS's S3IM term (train_ZJU.py:123, s3im_fun with repeat_time 10) forward + backward in three forms, on the masked two-body frames
and bound rectangles of scripts/loss_times_roi.py at 512 x 512 and 1024 x 1024:
  torch  -- moss_amd.loss.s3im, eager, on the (1,3,h,w) crops (what MOSS runs: the widened images, five depthwise 11x11 convolutions,
            the elementwise graph and its autograd mirror);
  fused  -- moss_amd.loss.s3im_fused, eager, on the same crops (the crop copies included);
  roi    -- moss_amd.loss.s3im_loss_roi_fused on the full frames, a hipGraph of 20 calls (no crop copies, the rectangle on the device).
hipEvents after warm-up; one JSON row per size and form.  ``hbm_bound_us``: the two kernels' HBM traffic -- (2 + 3) + (3 + 2 + 1) floats
per crop pixel-channel plus the zeroed gradient off the crop -- at 6.3 TB/s (the achievable copy rate of MI355X_MICROARCH).
Kernel times: run under ``rocprofv3 --kernel-trace --stats`` (``--size N``: one size only).
usage: python scripts/s3im_times.py [--size 512|1024] [--json FILE]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from moss_amd.graphs import capturing
from moss_amd.loss import ViewRegion, backward_from_loss, s3im, s3im_fused, s3im_loss_roi_fused

dev = torch.device("cuda:0")
C, R = 3, 10
rows = []
SIZES = (int(sys.argv[sys.argv.index("--size") + 1]),) if "--size" in sys.argv else (512, 1024)
for H in SIZES:
    W = H
    g = torch.Generator().manual_seed(3)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    body = lambda cx, cy, rx, ry: (((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1.0).float()
    k_ = H / 512.0
    m1, m2 = body(250 * k_, 260 * k_, 70 * k_, 200 * k_), body(262 * k_, 256 * k_, 74 * k_, 196 * k_)
    img = (torch.rand(C, H, W, generator=g) * m1).to(dev).contiguous(); gt = (torch.rand(C, H, W, generator=g) * m2).to(dev).contiguous()
    u = (m1 + m2) > 0
    ys, xs = u.any(1).nonzero().flatten(), u.any(0).nonzero().flatten()
    bm = torch.zeros(1, H, W, dtype=torch.uint8)
    bm[0, max(int(ys[0]) - 12, 0):int(ys[-1]) + 13, max(int(xs[0]) - 12, 0):int(xs[-1]) + 13] = 1
    region = ViewRegion(bm.to(dev))
    x, y, w, h = region.xywh
    val = torch.zeros((), device=dev)

    def crops(fn):
        X = img.clone().requires_grad_(True)

        def call():
            X.grad = None
            v = fn(X[:, y:y + h, x:x + w].unsqueeze(0), gt[:, y:y + h, x:x + w].unsqueeze(0))
            v.backward()
            val.copy_(v.detach())
        return call

    Xg = img.clone().requires_grad_(True)

    def roi():
        # (as the capture test does: a leaf of its own, warmed up and captured on one side stream, no autograd graph kept alive
        # between calls -- a leaf whose AccumulateGrad node lives on another stream breaks the capture)
        Xg.grad = None
        v = s3im_loss_roi_fused(Xg, gt, region)
        backward_from_loss(v)
        val.copy_(v.detach())

    hbm = (C * w * h * (5 + 6) + C * (H * W - w * h)) * 4
    side = torch.cuda.Stream(dev)
    for form, call, graphed in (("torch", crops(s3im), False), ("fused", crops(s3im_fused), False), ("roi", roi, True)):
        n = 20
        if graphed:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(5):
                    call()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with capturing(gr, stream=side):
                for _ in range(n):
                    call()
            for _ in range(3):
                gr.replay()
            run, reps = gr.replay, 10
        else:
            for _ in range(5):
                call()
            run, reps = (lambda: [call() for _ in range(n)]), 5
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        row = {"size": H, "form": form, "us_per_fwd_bwd": round(e0.elapsed_time(e1) / (reps * n) * 1e3, 2), "rect_xywh": [x, y, w, h],
               "repeat": R, "value": float(val), "hbm_bytes": hbm, "hbm_bound_us": round(hbm / 6.3e12 * 1e6, 2)}
        rows.append(row)
        print(json.dumps(row), flush=True)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(rows, f, indent=1)
