#!/usr/bin/env python3
"""Times the fused LBS deformation (moss_amd.lbs.lbs_deform, C ABI moss_lbs_deform_forward / _backward) against the same math in
float32 torch (moss_amd.lbs.deform_torch: gather, softmax, two (P,J)x(J,16) blends, torch.inverse, batched 3x3 products -- the
stand-in for MOSS's chain), forward and forward+backward, J = 24, at P = 6 890 / 45 695 / 100 000.

    python scripts/lbs_times.py [--iters 200] [--json PATH]

Times are device events around ``iters`` back-to-back calls after a warm-up, per call.  The fused op is timed eagerly and replayed
from a captured hipGraph (the launch cost then disappears); the torch chain eagerly only (torch.inverse synchronises: it cannot be
captured).  The HBM fraction counts the bytes the kernels must move -- forward: ids 8 B, L and the written w 2 x 4J B, d and x 24 B,
T, t, p 60 B per Gaussian (the W rows of 256 vertices stay in cache); backward: the forward's reads + gT, gt, gp 60 B + gL 4J B +
gd, gx 24 B -- over the 8 TB/s HBM peak.  Needs a GPU; there is no CPU timing.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from moss_amd import lbs as mlbs  # noqa: E402

HBM_PEAK = 8.0e12


def inputs(P, J, dev):
    body = mlbs.synthetic_body_model(256, J, seed=1)
    A_big = mlbs.smpl_joint_transforms(body, mlbs.synthetic_frame(0, J, big_pose=True))[0][0]
    A_obs, R, Th = mlbs.smpl_joint_transforms(body, mlbs.synthetic_frame(3, J))
    g = torch.Generator().manual_seed(P)
    ids = torch.randint(0, 256, (P,), generator=g)
    c = {"ids": ids, "W": body["weights"], "L": 0.7 * torch.randn(P, J, generator=g), "A_big": A_big, "A_obs": A_obs[0],
         "d": 0.01 * torch.randn(P, 3, generator=g), "R": R.reshape(3, 3), "Th": Th.reshape(3),
         "x": body["v_template"][ids] + 0.03 * torch.randn(P, 3, generator=g)}
    return {k: v.to(dev).contiguous() for k, v in c.items()}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lbs_times.py measures on the GPU; none is available")
    dev = torch.device("cuda:0")
    J = 24
    rows = []
    for P in (6890, 45695, 100000):
        c = inputs(P, J, dev)
        leaves = {k: c[k].clone().requires_grad_(True) for k in ("L", "A_obs", "d", "x")}
        cot = [torch.randn(P, 3, 3, device=dev), torch.randn(P, 3, device=dev), torch.randn(P, 3, device=dev)]

        def fused_fwd():
            with torch.no_grad():
                return mlbs.lbs_deform(c["ids"], c["W"], c["L"], c["A_big"], c["A_obs"], c["d"], c["R"], c["Th"], x=c["x"],
                                       want_weights=True)

        def fused_fb():
            T, t, p, _ = mlbs.lbs_deform(c["ids"], c["W"], leaves["L"], c["A_big"], leaves["A_obs"], leaves["d"], c["R"], c["Th"],
                                         x=leaves["x"], want_weights=True)
            torch.autograd.backward([T, t, p], cot)

        def torch_fwd():
            with torch.no_grad():
                return mlbs.deform_torch(c["ids"], c["W"], c["L"], c["A_big"], c["A_obs"], c["d"], c["R"], c["Th"], x=c["x"])

        def torch_fb():
            T, t, p, _ = mlbs.deform_torch(c["ids"], c["W"], leaves["L"], c["A_big"], leaves["A_obs"], leaves["d"], c["R"], c["Th"],
                                           x=leaves["x"])
            torch.autograd.backward([T, t, p], cot)

        def graphed(fn):
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

        fwd_bytes = P * (8 + 2 * 4 * J + 24 + 60)
        bwd_bytes = P * (8 + 4 * J + 24 + 60 + 4 * J + 24)
        r = {"P": P, "J": J,
             "fused_fwd_us": timed(fused_fwd, args.iters, dev), "fused_fwd_graph_us": timed(graphed(fused_fwd), args.iters, dev),
             "fused_fwdbwd_us": timed(fused_fb, args.iters, dev), "fused_fwdbwd_graph_us": timed(graphed(fused_fb), args.iters, dev),
             "torch_fwd_us": timed(torch_fwd, max(args.iters // 4, 10), dev),
             "torch_fwdbwd_us": timed(torch_fb, max(args.iters // 4, 10), dev),
             "fwd_bytes": fwd_bytes, "fwdbwd_bytes": fwd_bytes + bwd_bytes}
        r["fwd_graph_hbm_fraction"] = fwd_bytes / (r["fused_fwd_graph_us"] * 1e-6) / HBM_PEAK
        r["fwdbwd_graph_hbm_fraction"] = (fwd_bytes + bwd_bytes) / (r["fused_fwdbwd_graph_us"] * 1e-6) / HBM_PEAK
        rows.append(r)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(args.json) or ".", exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
