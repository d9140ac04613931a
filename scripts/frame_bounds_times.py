#!/usr/bin/env python3
"""Times the frame-bounds ops (moss_amd.bounds; C ABI moss_smpl_vertices / moss_bound_mask) against the same math composed in torch
on the same device, as the parent would run it:

* the vertex call at V = 6 890, J = 24: ``posed_vertices`` buffers (3 launches) vs ``posed_vertices_torch`` in float32; for the fused
  call also posedirs' bytes (12 V 9 (J - 1)) over its time, as a share of the 8 TB/s HBM peak -- the whole call's time, three launches
  and their two boundaries, not the streaming kernel's alone, so the share is a lower bound of that kernel's (whose own time is in
  the kernel trace, see ``--once``);
* the mask call at C = 1, 4 and 22 for 512 x 512 and 1024 x 1024 (2 launches) vs :func:`masks_torch` (the rules in torch int64 ops,
  one camera after another);
* ``dataset_regions`` for 100 poses x 4 cameras at 512 x 512, end to end on the host clock (it ends in its one host read).

    python scripts/frame_bounds_times.py [--iters 200] [--repeats 5] [--json profiles/frame_bounds_times.json]

The fused calls are timed eagerly, replayed from a captured hipGraph of one call, and from a graph of 20 back-to-back calls (per
call: the replay of a graph this small costs the host more than its kernels take; the 20-call graph shows the device's time); the
torch forms eagerly (they read the host: ``nonzero``, the parent table).  ``--once`` runs 20 updates of a 22-camera 1024 x 1024
``FrameBounds`` and exits: the kernel times of a ``rocprofv3 --kernel-trace --stats`` run come from it.  Device events around ``iters`` back-to-back calls after a warm-up, per call; every row is measured ``--repeats`` times
and the median and the spread (min, max) are kept.  Needs a GPU; there is no CPU timing.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from moss_amd import bounds as mb  # noqa: E402
from moss_amd import lbs as mlbs  # noqa: E402

V, J = 6890, 24
HBM_PEAK = 8.0e12


def timed(fn, iters, dev):
    for _ in range(5):
        fn()
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) * 1e3 / iters                  # us per call


def graphed(fn, dev, calls=1):
    """A replay of ``calls`` back-to-back calls of ``fn`` captured in one hipGraph (a replay of a graph this small costs more on the
    host than its kernels take on the device: ``calls`` > 1 shows the device's time per call)."""
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(calls):
            fn()
    return g.replay


def look_at(seed, centre, dist, H, W):
    rng = np.random.Generator(np.random.PCG64(seed))
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    pos = centre + dist * d
    z = (centre - pos) / np.linalg.norm(centre - pos)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z], 0)
    K = np.array([[1.1 * W, 0, W / 2], [0, 1.1 * W, H / 2], [0, 0, 1]])
    return torch.tensor(K, dtype=torch.float32), torch.tensor(np.concatenate([R, (-R @ pos)[:, None]], 1), dtype=torch.float32)


def masks_torch(world_bound, K, RT, H, W):
    """``bound_masks`` in torch ops on the device: float64 projection, np.round, the six faces by rules (a) and (b) in int64, the
    rectangle by ``nonzero`` -- camera after camera."""
    dev = world_bound.device
    wb = world_bound.double()
    i = torch.arange(8, device=dev)
    c = torch.stack([wb[(i >> 2) & 1, 0], wb[(i >> 1) & 1, 1], wb[i & 1, 2]], 1)
    y, x = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    bounds, rects = [], []
    for cam in range(K.shape[0]):
        uvw = (c @ RT[cam, :, :3].double().t() + RT[cam, :, 3].double()) @ K[cam].double().t()
        q = torch.round(uvw[:, :2] / uvw[:, 2:]).long()
        bound = torch.zeros((H, W), dtype=torch.bool, device=dev)
        for face in mb.FACES:
            f = q[list(face)]
            inbox = (x >= f[:, 0].min()) & (x <= f[:, 0].max()) & (y >= f[:, 1].min()) & (y <= f[:, 1].max())
            ge, le, edge = inbox.clone(), inbox.clone(), torch.zeros_like(inbox)
            for k in range(4):
                q0, q1 = f[k], f[(k + 1) % 4]
                dx, dy = q1[0] - q0[0], q1[1] - q0[1]
                cr = dx * (y - q0[1]) - dy * (x - q0[0])
                ge &= cr >= 0
                le &= cr <= 0
                ebox = (x >= torch.minimum(q0[0], q1[0])) & (x <= torch.maximum(q0[0], q1[0])) & (y >= torch.minimum(q0[1], q1[1])) \
                    & (y <= torch.maximum(q0[1], q1[1]))
                edge |= ebox & ((2 * cr).abs() <= torch.maximum(dx.abs(), dy.abs()))
            bound |= ge | le | edge
        ys, xs = bound.any(1).nonzero().flatten(), bound.any(0).nonzero().flatten()
        rects.append(torch.stack([xs[0], ys[0], xs[-1] - xs[0] + 1, ys[-1] - ys[0] + 1, bound.sum()]) if ys.numel() else
                     torch.zeros(5, dtype=torch.long, device=dev))
        bounds.append(bound.to(torch.uint8))
    return torch.stack(bounds), torch.stack(rects).int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--once", action="store_true", help="run the vertex call and the 1024x1024 C=22 mask call 20 times each and exit: "
                                                        "for a rocprofv3 --kernel-trace --stats run")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frame_bounds_times.py needs a GPU: there is no CPU timing")
    dev = torch.device("cuda:0")
    body = {k: v.to(dev) for k, v in mlbs.synthetic_body_model(V, J, seed=1).items()}
    fr = {k: v.to(dev).contiguous() for k, v in mlbs.synthetic_frame(3, J).items()}
    rows = {}

    def row(name, fn, iters, per=1, **extra):
        t = [timed(fn, iters, dev) / per for _ in range(args.repeats)]
        rows[name] = dict(us=statistics.median(t), min=min(t), max=max(t), **extra)
        more = "".join(f", {k} {v}" for k, v in extra.items())
        print(f"{name:44s} {rows[name]['us']:10.1f} us  ({min(t):.1f} .. {max(t):.1f}){more}", flush=True)

    fb = mb.FrameBounds(body, [look_at(0, np.zeros(3), 3.0, 512, 512)], 512, 512)
    fb.load(fr)
    pad = fb.pad

    def vertices():
        mb._launch_vertices(body, V, J, fb._par, fb.smpl_param["poses"], fb.smpl_param["shapes"], fb.smpl_param["R"], fb.smpl_param["Th"],
                            pad, fb.world_vertex, fb.world_bound, fb.joints, fb._ws_v)
    posedirs_bytes = 4 * V * 3 * 9 * (J - 1)
    if args.once:
        m = mb.FrameBounds(body, [look_at(10 + c, np.zeros(3), 3.0, 1024, 1024) for c in range(22)], 1024, 1024)
        m.load(fr)
        for _ in range(20):
            m.update()
        torch.cuda.synchronize(dev)
        return
    row("vertices fused eager", vertices, args.iters)
    row("vertices fused graph", graphed(vertices, dev), args.iters)
    row("vertices fused graph of 20 calls, per call", graphed(vertices, dev, 20), max(args.iters // 10, 5), per=20)
    best = rows["vertices fused graph of 20 calls, per call"]
    best["posedirs_share_of_hbm_peak"] = posedirs_bytes / (best["us"] * 1e-6) / HBM_PEAK
    print(f"    posedirs {posedirs_bytes / 1e6:.1f} MB over the call's time: "
          f"{100 * best['posedirs_share_of_hbm_peak']:.1f} % of the 8 TB/s HBM peak")
    with torch.no_grad():
        row("vertices torch float32 eager", lambda: mb.posed_vertices_torch(body, fr, 0.1), max(args.iters // 10, 5))
    fb.update()
    wb = fb.world_bound.clone()
    centre = wb.mean(0).cpu().numpy().astype(np.float64)
    for size in (512, 1024):
        for C in (1, 4, 22):
            cams = [look_at(10 + c, centre, 3.0, size, size) for c in range(C)]
            m = mb.FrameBounds(body, cams, size, size)
            m.world_bound.copy_(wb)

            def masks(m=m):
                mb._launch_masks(m.world_bound, m.K, m.RT, m.H, m.W, m.bound, m.rect, m.corners, m.flags, m._ws_m)
            masks()
            ref_b, ref_r = masks_torch(wb, m.K, m.RT, size, size)
            assert torch.equal(ref_b, m.bound) and torch.equal(ref_r, m.rect), "the torch composition and the kernel disagree"
            row(f"masks fused eager  {size}x{size} C={C}", masks, args.iters)
            row(f"masks fused graph  {size}x{size} C={C}", graphed(masks, dev), args.iters)
            row(f"masks fused graph of 20 calls, per call  {size}x{size} C={C}", graphed(masks, dev, 20), max(args.iters // 10, 5), per=20)
            with torch.no_grad():
                row(f"masks torch eager  {size}x{size} C={C}", lambda m=m: masks_torch(wb, m.K, m.RT, size, size), 3 if C > 4 else 10)
    poses = [{k: v.numpy() for k, v in mlbs.synthetic_frame(100 + p, J).items()} for p in range(100)]
    cams = [[look_at(200 + 4 * p + c, centre, 3.0, 512, 512) for c in range(4)] for p in range(100)]
    mb.dataset_regions(body, poses[:2], cams[:2], 512, 512)
    t = []
    for _ in range(args.repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = mb.dataset_regions(body, poses, cams, 512, 512)
        t.append((time.perf_counter() - t0) * 1e3)
        del out
    rows["dataset_regions 100 poses x 4 cameras 512x512"] = dict(ms=statistics.median(t), min=min(t), max=max(t))
    print(f"dataset_regions 100 poses x 4 cameras 512x512: {statistics.median(t):.1f} ms end to end ({min(t):.1f} .. {max(t):.1f})")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
