#!/usr/bin/env python3
"""Times MOSS's pose-refinement head + matrix-Fisher NLL: the torch form (moss_amd.pose.autoregression_torch + matrix_fisher_nll in
float32 on the GPU -- the stand-in for MOSS's chain: the MLP, the loop over 23 joint layers, Rodrigues, a batched SVD, the quadrature
and its three backward integrals) eagerly, and the fused op (moss_amd.pose.pose_head_fused, one HIP kernel each way) eagerly and
replayed from a captured hipGraph; forward alone and forward + backward to the 52 parameters.

    python scripts/pose_head_times.py [--iters 200] [--json PATH]

Every measurement is a process of its own under ``timeout``; the script stops at the first one that does not exit with 0.  A time is
the wall clock around ``iters`` back-to-back calls between two device synchronisations, per call, after a warm-up -- so a host-bound
chain is charged its host time, as a training loop would be.  The torch form cannot be captured (its SVD checks a status word on the
host).  Needs a GPU; there is no CPU timing.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("torch_fwd", "torch_fwd_bwd", "fused_fwd", "fused_fwd_bwd", "fused_fwd_graph", "fused_fwd_bwd_graph")
STEP_TIMEOUT = 120


def measure(step, iters):
    import torch
    from moss_amd import lbs as mlbs
    from moss_amd import pose as mpose
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    net = mpose.head_module(init_val=1e-2).to(dev)
    plist = mpose.head_parameters(net)
    params = dict(zip(mpose.PARAM_NAMES, plist))
    poses = (1.2 * torch.rand(1, 72) - 0.6).to(dev)
    target_R = mlbs.batch_rodrigues(0.4 * torch.randn(23, 3)).to(dev)
    g_Rs = (1e-2 * torch.randn(23, 3, 3)).to(dev)
    backward = "bwd" in step

    def torch_form():
        o = mpose.autoregression_torch(params, poses)
        nll = mpose.matrix_fisher_nll(o["Rs"], o["pose_U"], o["pose_S"], o["pose_V"], target_R)
        return o["Rs"], nll

    def fused():
        o = mpose.pose_head_fused(net, poses, target_R)
        return o["Rs"], o["nll"]

    head = torch_form if step.startswith("torch") else fused

    def call():
        if not backward:
            with torch.no_grad():
                Rs, nll = head()
            return [Rs, nll]
        Rs, nll = head()
        return [g.detach() for g in torch.autograd.grad(0.06 * nll.mean() + (Rs * g_Rs).sum(), plist)]

    run = call
    if step.endswith("graph"):
        from moss_amd.graphs import capturing
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                call()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with capturing(graph, collect=True, stream=side, capture_error_mode="thread_local"):
            keep = call()                                    # noqa: F841  (the static outputs live as long as the graph)
        run = graph.replay
    for _ in range(20):
        run()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(iters):
        run()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one measurement in this process and print its JSON line")
    args = ap.parse_args()
    if args.step:
        print(json.dumps({"step": args.step, "us_per_call": measure(args.step, args.iters), "iters": args.iters}))
        return 0
    res = {}
    for step in STEPS:
        p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", step,
                            "--iters", str(args.iters)], stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"{step}: exit status {p.returncode}; stopping here", flush=True)
            return p.returncode
        res[step] = json.loads(p.stdout.strip().splitlines()[-1])["us_per_call"]
        print(f"{step:22s} {res[step]:10.1f} us per call", flush=True)
    for kind in ("fwd", "fwd_bwd"):
        t, e, g = res[f"torch_{kind}"], res[f"fused_{kind}"], res[f"fused_{kind}_graph"]
        print(f"{kind}: torch eager / fused eager = {t / e:.1f}x, torch eager / fused from a graph = {t / g:.1f}x")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"iters": args.iters, "us_per_call": res}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
