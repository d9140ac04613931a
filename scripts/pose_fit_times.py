#!/usr/bin/env python3
"""Times one step of ``moss_amd.posefit.PoseFitter`` -- pose head and LBS-weight network under no_grad, ``posed_frame``, one 512 x 512
render with transforms / translation in the op, MOSS's photometric loss, the backward to poses / Rh / Th, one AdamW launch -- eagerly
and replayed from a hipGraph, at P = 6 890 and 45 695 Gaussians (J = 24, a synthetic body of V = 6 890 vertices, networks with their
default initialisation).  Beside it the same step with ``posed_frame_torch`` in float32 on the device in place of ``posed_frame``
(eager only: its ``torch.inverse`` synchronises with the host, so it cannot be captured).

    timeout 600 python scripts/pose_fit_times.py [--iters 100] [--repeats 3] [--json profiles/pose_fit_times.json]

Every measurement is a fixed number of steps in this one process between two device events, with ONE synchronisation per batch; after
each batch the rasterizer's status and the device's error state are checked, and the first error ends the script (an exception: a
non-zero exit).  Run it under ``timeout``.  Needs a GPU; there is no CPU timing.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from moss_amd import lbs as mlbs  # noqa: E402
from moss_amd import posefit  # noqa: E402

V, J, SIDE = 6890, 24, 512


def avatar(P, dev):
    from moss_amd import lbs_weights as mlw
    from moss_amd import pose as mpose
    from moss_amd import scenes
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import camera_view
    from moss_amd.knn_cuda import KNN
    torch.manual_seed(P)
    s = scenes.body_scene(P, SIDE, SIDE, 540.0, init_like=False, name="posefit")
    pc = GaussianSet(s, device=dev, unified_features=True)
    body = mlbs.synthetic_body_model(V, J, seed=21, device=dev)
    pc.SMPL_NEUTRAL, pc.knn = body, KNN(k=1, transpose_mode=True)
    pc.auto_regression = mpose.head_module().to(dev)
    pc.cross_attention_lbs = mlw.lbs_weight_module().to(dev)
    pc.motion_offset_flag = True
    cam = camera_view(s.camera, dev)
    cam.big_pose_smpl_param = {k: v.to(dev) for k, v in mlbs.synthetic_frame(0, J, big_pose=True).items()}
    cam.big_pose_world_vertex = body["v_template"].clone()
    g = torch.Generator().manual_seed(500)
    axis = torch.randn(1, 3, generator=g)
    frame = {"poses": 0.15 * torch.randn(1, 3 * J, generator=g), "shapes": 0.3 * torch.randn(1, 10, generator=g),
             "R": mlbs.batch_rodrigues(0.3 * axis / axis.norm())[0], "Th": 0.05 * torch.randn(1, 3, generator=g)}
    return pc, cam, {k: v.to(dev) for k, v in frame.items()}, s


def timed(fitter, iters, dev):
    """us per step of ``iters`` steps: one synchronisation, then the error checks."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fitter.step()
    b.record()
    torch.cuda.synchronize(dev)                                 # (raises if a kernel of the batch failed)
    for v in fitter._views:
        v.context.check_status()                                # (raises if a view overflowed the binning capacity)
    if not all(bool(torch.isfinite(p).all()) for p in (fitter.poses, fitter.Th, fitter.Rh)):
        raise RuntimeError("pose_fit_times: a fitted parameter is not finite")
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pose_fit_times.py measures on the GPU; none is available")
    from moss_amd.loss import ViewRegion
    dev = torch.device("cuda:0")
    bg = torch.zeros(3, device=dev)
    rows = []
    for P in (6890, 45695):
        pc, cam, frame, scene = avatar(P, dev)
        gt = scenes_target(scene).to(dev)
        mask = torch.ones(1, SIDE, SIDE, device=dev)
        region = ViewRegion(torch.ones(1, SIDE, SIDE, device=dev))
        forms = {}
        for name, capture, torch_form in (("fused_eager_us", False, False), ("fused_graph_us", True, False), ("torch_eager_us", False, True)):
            f = posefit.PoseFitter(pc, cam, bg, lr=1e-4, capture=capture)
            if torch_form:
                f._frame_fn = posefit.posed_frame_torch
            f.fit(cam, (gt, mask), region, frame, 3)             # (loads the statics, warms up, captures)
            forms[name] = f
        r = {"P": P, "V": V, "J": J, "H": SIDE, "W": SIDE, "iters": args.iters, "repeats": args.repeats}
        samples = {k: [] for k in forms}
        for _ in range(args.repeats):                           # (the forms alternate inside a repeat)
            for k, f in forms.items():
                samples[k].append(timed(f, args.iters if k != "torch_eager_us" else max(args.iters // 4, 10), dev))
        for k, v in samples.items():
            r[k] = statistics.median(v)
            r[k + "_min_max"] = [min(v), max(v)]
        rows.append(r)
        print(json.dumps({k: (round(v, 1) if isinstance(v, float) else [round(x, 1) for x in v] if isinstance(v, list) else v)
                          for k, v in r.items()}), flush=True)
        del forms
    if args.json:
        os.makedirs(os.path.dirname(args.json) or ".", exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


def scenes_target(scene):
    from moss_amd import scenes
    return scenes.synthetic_target(scene.camera.H, scene.camera.W)


if __name__ == "__main__":
    main()
