#!/usr/bin/env python3
"""Times of ``moss_amd.images`` (profiles/view_images_notes.md):

    prepare_8     ``prepare_views`` of 8 views of 1024 x 1024 at ``scale = 2`` -- one launch; every call takes the NEXT eight of the
                  374 views, so that no call finds its input in a cache the call before it filled
    prepare_374   ``prepare_views`` of 374 views (a ZJU test split: 17 poses x 22 cameras) -- 47 launches
    load          ``ViewImages.load`` at 512 x 512, eager launches back to back, a new view per call
    torch_cpu     ``prepare_views_torch`` on the CPU with the process's threads (``--cpu-views`` views of 1024 x 1024): the torch
                  statement's time, NOT OpenCV's

The GPU times are host clocks around device-synchronised windows after warm-up calls of the same shapes; every window is taken
``--rounds`` times and all of them are printed.  Bytes moved per view = the raw bytes in (4 per full-resolution pixel) plus the packed
bytes out (4 per output pixel); ``share_of_hbm`` is that over the time, over ``--hbm-gbs``.  The lens is a ZJU-like one (k1 = -0.28).
Without a GPU the script fails; it does not fall back.

    python scripts/view_images_times.py [--views 374] [--side 1024] [--scale 2] [--rounds 3] [--hbm-gbs 8000] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

D = (-0.28, 0.09, 3e-4, -2e-4, 0.02)


def _window(fn, calls, dev, warmup=3):
    import torch
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(calls):
        fn(i)
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=374)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--scale", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls-8", type=int, default=2000)
    ap.add_argument("--calls-all", type=int, default=40)
    ap.add_argument("--calls-load", type=int, default=20000)
    ap.add_argument("--cpu-views", type=int, default=2)
    ap.add_argument("--cpu-calls", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM rate the share is quoted against, GB/s")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from moss_amd.host import limit_cpu_threads
    from moss_amd.images import prepare_views, prepare_views_torch
    limit_cpu_threads()
    if not torch.cuda.is_available():
        raise SystemExit("view_images_times.py measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    n, side, scale = a.views, a.side, a.scale
    g = torch.Generator(device=dev).manual_seed(1)
    rgb = torch.randint(0, 256, (n, side, side, 3), dtype=torch.uint8, device=dev, generator=g)
    yy, xx = torch.meshgrid(torch.arange(side, device=dev), torch.arange(side, device=dev), indexing="ij")
    person = (((yy - side * 0.5) / (side * 0.42)) ** 2 + ((xx - side * 0.5) / (side * 0.18)) ** 2 <= 1.0).to(torch.uint8) * 255
    mask = person[None].repeat(n, 1, 1)
    K = np.array([[1.05 * side, 0, side / 2 - 3.3], [0, 1.05 * side, side / 2 + 2.1], [0, 0, 1]])
    bytes_per_view = 4 * side * side + 4 * (side // scale) ** 2
    rows = {"views": n, "side": side, "scale": scale, "bytes_per_view": bytes_per_view, "hbm_gbs": a.hbm_gbs,
            "cpu_threads": torch.get_num_threads(), "device": torch.cuda.get_device_name(dev)}
    groups = n // 8

    def eight(i):
        k = 8 * (i % groups)
        return prepare_views(rgb[k:k + 8], mask[k:k + 8], K, D, scale=scale)

    def rate(seconds_per_view):
        gbs = bytes_per_view / seconds_per_view / 1e9
        return {"us_per_view": round(seconds_per_view * 1e6, 3), "gb_per_s": round(gbs, 1), "share_of_hbm": round(gbs / a.hbm_gbs, 4)}
    rows["prepare_8"] = [rate(_window(eight, a.calls_8, dev) / 8) for _ in range(a.rounds)]
    rows["prepare_374"] = [rate(_window(lambda i: prepare_views(rgb, mask, K, D, scale=scale), a.calls_all, dev) / n) for _ in range(a.rounds)]
    small = prepare_views(rgb[:8], mask[:8], K, D, scale=scale)
    gt_image = torch.empty((3, small.H, small.W), dtype=torch.float32, device=dev)
    bkgd_mask = torch.empty((1, small.H, small.W), dtype=torch.float32, device=dev)
    load_bytes = 4 * small.H * small.W * 5                       # 4 bytes in and 16 out per pixel
    rows["load"] = []
    for _ in range(a.rounds):
        dt = _window(lambda i: small.load(i % 8, gt_image, bkgd_mask), a.calls_load, dev, warmup=20)
        rows["load"].append({"H": small.H, "W": small.W, "us_per_call": round(dt * 1e6, 3), "gb_per_s": round(load_bytes / dt / 1e9, 1)})
    graph = torch.cuda.CUDAGraph()
    from moss_amd.graphs import capturing
    with capturing(graph, collect=True):
        for i in range(8):
            small.load(i, gt_image, bkgd_mask)
    rows["load_replayed_8_per_graph"] = [{"us_per_call": round(_window(lambda i: graph.replay(), a.calls_load // 8, dev) / 8 * 1e6, 3)}
                                         for _ in range(a.rounds)]
    cpu_rgb, cpu_mask = rgb[:a.cpu_views].cpu(), mask[:a.cpu_views].cpu()
    rows["torch_cpu"] = []
    for _ in range(a.rounds):
        prepare_views_torch(cpu_rgb, cpu_mask, K, D, scale=scale)
        t0 = time.perf_counter()
        for _ in range(a.cpu_calls):
            prepare_views_torch(cpu_rgb, cpu_mask, K, D, scale=scale)
        rows["torch_cpu"].append({"us_per_view": round((time.perf_counter() - t0) / a.cpu_calls / a.cpu_views * 1e6, 1)})
    print(json.dumps(rows), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
