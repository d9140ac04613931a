#!/usr/bin/env python3
"""Times the per-frame, per-subject part of coarse_deform_c2source: the torch form (moss_amd.lbs.smpl_joint_transforms twice,
vertex_offsets and the gather D[ids] -- about 320 launches per training step) against the fused op (moss_amd.lbs.smpl_frame_fused, C ABI
moss_smpl_frame_forward / _backward: 2 + 3 launches), forward and forward + backward (the gradient of correct_Rs from cotangents of
A_obs and d), float32, V = 6 890, J = 24, at P = 6 890 / 45 695 / 100 000.

    python scripts/smpl_frame_times.py [--iters 200] [--json profiles/smpl_frame_times.json] [--only torch|fused] [--once]

Times are device events around ``iters`` back-to-back calls after a warm-up, per call; each row is measured ``--repeats`` times and
the median and the spread (min, max) are kept.  Both forms are timed eagerly and replayed from a captured hipGraph (neither
synchronises with the host).  ``--once`` runs each selected form once at P = 45 695 and exits: the launch counts of a
``rocprofv3 --kernel-trace --stats`` run come from it.  Needs a GPU; there is no CPU timing.
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

V, J = 6890, 24


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


def graphed(fn, dev):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn()
    return g.replay


def forms(P, dev):
    body = {k: v.to(dev) for k, v in mlbs.synthetic_body_model(V, J, seed=1).items()}
    fr = {k: v.to(dev) for k, v in mlbs.synthetic_frame(3, J).items()}
    big = {k: v.to(dev) for k, v in mlbs.synthetic_frame(0, J, big_pose=True).items()}
    g = torch.Generator().manual_seed(P)
    ids = torch.randint(0, V, (P,), generator=g).to(dev)
    cR = mlbs.batch_rodrigues(0.1 * torch.randn(J - 1, 3, generator=g)).to(dev).requires_grad_(True)
    gA, gd = torch.randn(J, 4, 4, generator=g).to(dev), torch.randn(P, 3, generator=g).to(dev)

    def torch_part():
        A_big = mlbs.smpl_joint_transforms(body, big)[0][0]
        rot = mlbs.batch_rodrigues(fr["poses"].reshape(-1, 3))
        rot = torch.cat([rot[:1], rot[1:] @ cR], 0)
        A_obs = mlbs.smpl_joint_transforms(body, fr, rot_mats=rot)[0][0]
        return A_big, A_obs, mlbs.vertex_offsets(body, fr, big, rot)[ids]

    def fused_part():
        return mlbs.smpl_frame_fused(body, fr, big, ids, correct_Rs=cR)[:3]

    def fwd(part):
        def fn():
            with torch.no_grad():
                return part()
        return fn

    def fwdbwd(part):
        def fn():
            cR.grad = None
            _, A_obs, d = part()
            torch.autograd.backward([A_obs, d], [gA, gd])
        return fn

    return {"torch": (fwd(torch_part), fwdbwd(torch_part)), "fused": (fwd(fused_part), fwdbwd(fused_part))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=("torch", "fused"), default=None)
    ap.add_argument("--once", action="store_true", help="one eager forward + backward of each selected form at P = 45 695 (for a kernel trace)")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("smpl_frame_times.py measures on the GPU; none is available")
    dev = torch.device("cuda:0")
    names = [args.only] if args.only else ["torch", "fused"]
    if args.once:
        f = forms(45695, dev)
        for n in names:
            f[n][1]()
        torch.cuda.synchronize(dev)
        return
    rows = []
    for P in (6890, 45695, 100000):
        f = forms(P, dev)
        r = {"P": P, "V": V, "J": J, "iters": args.iters, "repeats": args.repeats}
        for n in names:
            runs = {f"{n}_fwd_us": f[n][0], f"{n}_fwd_graph_us": graphed(f[n][0], dev),
                    f"{n}_fwdbwd_us": f[n][1], f"{n}_fwdbwd_graph_us": graphed(f[n][1], dev)}
            samples = {k: [] for k in runs}
            for _ in range(args.repeats):                       # (the forms alternate inside a repeat)
                for k, fn in runs.items():
                    samples[k].append(timed(fn, args.iters if n == "fused" else max(args.iters // 4, 10), dev))
            for k, v in samples.items():
                r[k] = statistics.median(v)
                r[k + "_min_max"] = [min(v), max(v)]
        rows.append(r)
        print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(args.json) or ".", exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
