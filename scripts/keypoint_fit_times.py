#!/usr/bin/env python3
"""Times the keypoint fit of ``moss_amd.keypoints`` at V = 6 890 vertices, J = 24 joints, Kp = 25 keypoints, C = 4 cameras (both
parts of the loss, both robustifiers):

* the op chain -- ``posed_vertices_fn`` -> ``keypoint_loss`` -> backward to poses, R and Th (the vertex forward, the loss op, the
  vertex backward) -- eagerly and replayed from a hipGraph, against ``bounds.posed_vertices_torch`` + ``keypoint_loss_torch`` in
  float32 on the device (eager: its Python loop over the joints is what a capture would only hide);
* one keypoint-only step of ``PoseFitter`` (``photometric=False``), eager and replayed;
* one combined step (one 512 x 512 render, MOSS's photometric loss, plus the keypoint term), eager and replayed.

    python scripts/keypoint_fit_times.py [--iters 200] [--repeats 3] [--limit 300] [--json profiles/keypoint_fit_times.json]

Every measurement is a fixed number of calls in this one process between two device events, with ONE synchronisation per batch; after
each batch the device's error state is checked, and the first error ends the script (an exception: a non-zero exit).  The script
ends itself after ``--limit`` seconds (SIGALRM's default action: also out of a blocked synchronisation).  Needs a GPU; nothing here is
a promise, and bench.py does not run it.
"""
import argparse
import json
import os
import signal
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from moss_amd import bounds as mb  # noqa: E402
from moss_amd import keypoints as kp  # noqa: E402
from moss_amd import lbs as mlbs  # noqa: E402
from moss_amd import posefit  # noqa: E402
from scripts.pose_fit_times import SIDE, avatar, scenes_target  # noqa: E402

V, J, KP, C = 6890, 24, 25, 4


def make_targets(body, frame, dev):
    """Kp local means of vertices; uv and xyz of the frame's own keypoints, a few pixels / centimetres off."""
    g = torch.Generator().manual_seed(7)
    vt = body["v_template"].double()
    centre = vt[torch.arange(KP, device=dev) * 271 + 13]
    reg = torch.exp(-((vt[None] - centre[:, None]) ** 2).sum(-1) / (2 * 0.05 ** 2))
    reg = (reg / reg.sum(1, keepdim=True)).float().contiguous()
    world = mb.posed_vertices(body, frame)[0]
    K = torch.tensor([[540.0, 0.0, SIDE / 2], [0.0, 540.0, SIDE / 2], [0.0, 0.0, 1.0]]).repeat(C, 1, 1)
    Rc = mlbs.batch_rodrigues(0.2 * torch.randn(C, 3, generator=g))
    RT = torch.cat([Rc, torch.tensor([0.0, 0.0, 4.0]).repeat(C, 1)[:, :, None]], 2).float().contiguous()
    K, RT = K.to(dev), RT.to(dev)
    X = reg @ world
    u, z = kp.project_torch(X, K, RT)
    if float(z.min()) <= 0.5:
        raise RuntimeError("keypoint_fit_times: a keypoint is too close to a camera")
    return kp.KeypointTargets(reg, K=K, RT=RT, uv=(u + 3.0 * torch.randn(C, KP, 2, generator=g).to(dev)).contiguous(),
                              conf=torch.rand(C, KP, generator=g).to(dev), xyz=(X + 0.02 * torch.randn(KP, 3, generator=g).to(dev)).contiguous(),
                              conf3=torch.rand(KP, generator=g).to(dev), sigma=50.0, sigma3=0.2, weight2d=1e-3, weight3d=1.0)


def timed(fn, iters, dev, finite):
    """us per call of ``iters`` calls: one synchronisation, then the error checks."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize(dev)                                 # (raises if a kernel of the batch failed)
    if not all(bool(torch.isfinite(t).all()) for t in finite()):
        raise RuntimeError("keypoint_fit_times: a result is not finite")
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds after which the script ends itself")
    ap.add_argument("--json", default=None, help="also write the row to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("keypoint_fit_times.py measures on the GPU; none is available")
    signal.alarm(args.limit)
    from moss_amd.graphs import GraphedStep
    from moss_amd.loss import ViewRegion
    dev = torch.device("cuda:0")
    bg = torch.zeros(3, device=dev)
    pc, cam, frame, scene = avatar(V, dev)
    body = {k: (v.float().contiguous() if v.is_floating_point() else v) for k, v in pc.SMPL_NEUTRAL.items()}
    frame = {k: v.contiguous() for k, v in frame.items()}
    tg = make_targets(body, frame, dev)
    leaves = {k: frame[k].clone().requires_grad_(True) for k in ("poses", "R", "Th")}

    def chain(vertices, loss_fn):
        def fn():
            for t in leaves.values():
                t.grad = None
            loss = loss_fn(vertices(body, {**frame, **leaves}), tg)
            loss.backward()
            return [loss.detach()] + [t.grad for t in leaves.values()]
        return fn

    fused = chain(kp.posed_vertices_fn, kp.keypoint_loss)
    in_torch = chain(lambda b, p: mb.posed_vertices_torch(b, p, 0.0)[0], kp.keypoint_loss_torch)
    fused()
    graphed = GraphedStep(fused, warmup=2, device=dev)
    forms = {"ops_fused_eager_us": (fused, lambda: fused()), "ops_fused_graph_us": (graphed, lambda: graphed.outputs),
             "ops_torch_eager_us": (in_torch, lambda: in_torch())}
    gt, mask = scenes_target(scene).to(dev), torch.ones(1, SIDE, SIDE, device=dev)
    region = ViewRegion(torch.ones(1, SIDE, SIDE, device=dev))
    for name, capture, photometric in (("step_keypoints_eager_us", False, False), ("step_keypoints_graph_us", True, False),
                                       ("step_combined_eager_us", False, True), ("step_combined_graph_us", True, True)):
        f = posefit.PoseFitter(pc, cam, bg, lr=1e-4, capture=capture)
        if photometric:
            f.fit(cam, (gt, mask), region, frame, 3, keypoints=tg)      # (loads the statics, warms up, captures)
        else:
            f.fit(None, None, None, frame, 3, keypoints=tg, photometric=False)
        forms[name] = (f.step, (lambda f=f: (f.poses, f.Th, f.Rh)))
    row = {"V": V, "J": J, "Kp": KP, "C": C, "H": SIDE, "W": SIDE, "iters": args.iters, "repeats": args.repeats}
    samples = {k: [] for k in forms}
    for _ in range(args.repeats):                               # (the forms alternate inside a repeat)
        for k, (fn, finite) in forms.items():
            samples[k].append(timed(fn, args.iters if "torch" not in k else max(args.iters // 8, 10), dev, finite))
    for k, v in samples.items():
        row[k] = statistics.median(v)
        row[k + "_min_max"] = [min(v), max(v)]
    print(json.dumps({k: (round(v, 1) if isinstance(v, float) else [round(x, 1) for x in v] if isinstance(v, list) else v)
                      for k, v in row.items()}), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(args.json) or ".", exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump([row], fh, indent=1)
    signal.alarm(0)


if __name__ == "__main__":
    main()
