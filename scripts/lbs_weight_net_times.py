#!/usr/bin/env python3
"""Times MOSS's LBS-weight network (CrossAttention_lbs): the torch form (moss_amd.lbs_weights.cross_attention_lbs_torch on the
module's float32 parameters on the GPU -- the stand-in for MOSS's module: the embedding, five 1x1 convolutions, three Linears, two
matmuls, a softmax) and the fused op (moss_amd.lbs_weights.cross_attention_lbs_fused: one HIP launch forward, three backward), each
eagerly and replayed from a captured hipGraph; forward alone and forward + backward to x, Rs and the 16 parameters.

    python scripts/lbs_weight_net_times.py [--iters 50] [--sizes 45695,100000] [--precision f32|bf16x3] [--package-root DIR] [--json PATH]

``--precision bf16x3``: the fused op in its split-bf16 mode (``cross_attention_lbs_fused(precision="bf16x3")``); the share of the matrix
peak is then that of the bf16 peak with three products per multiply-add counted as the work done.  ``--package-root DIR``: import
``moss_amd`` from another BUILT checkout (the parent commit's, to compare against): with ``--precision f32`` the op is then called
without the argument, so a checkout that has no precisions serves.

Every (implementation, size) is a process of its own under ``timeout``; the script stops at the first one that does not exit with 0.
A time is the wall clock around ``iters`` back-to-back calls between two device synchronisations, per call, after a warm-up -- so a
host-bound chain is charged its host time, as a training loop would be; the replayed graph shows the device time.  Needs a GPU;
there is no CPU timing.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IMPLS = ("torch", "fused")
MODES = ("fwd", "fwd_graph", "fwd_bwd", "fwd_bwd_graph")
STEP_TIMEOUT = 150
MACS_PER_POINT = 63 * 128 + 2 * 128 * 128 + 191 * 128 + 128 * 24 + 24 * 24 + 2 * 24 * 9     # 69 360 (+ biases, softmax)
F32_MFMA_PEAK = 157.3e12
BF16_MFMA_PEAK = 16 * F32_MFMA_PEAK                          # v_mfma_f32_32x32x16_bf16: 16 times the f32 instruction's rate


def measure(impl, P, iters, precision="f32"):
    import torch
    from moss_amd import lbs as mlbs
    from moss_amd import lbs_weights as mlw
    from moss_amd.graphs import capturing
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    net = mlw.lbs_weight_module().to(dev)
    plist = mlw.net_parameters(net)
    params = dict(net.named_parameters())
    x = (2 * torch.rand(P, 3) - 1).to(dev).requires_grad_(True)
    Rs = mlbs.batch_rodrigues(0.4 * torch.randn(23, 3)).to(dev).requires_grad_(True)
    cot = torch.randn(1, P, 24).to(dev)
    if impl == "torch":
        head = lambda: mlw.cross_attention_lbs_torch(params, x[None], Rs)              # noqa: E731
    else:
        kw = {} if precision == "f32" else {"precision": precision}
        head = lambda: mlw.cross_attention_lbs_fused(net, x[None], Rs, **kw)           # noqa: E731
    res = {}
    for mode in MODES:
        if "bwd" in mode:
            def call():
                return [g.detach() for g in torch.autograd.grad((head() * cot).sum(), [x, Rs] + plist)]
        else:
            def call():
                with torch.no_grad():
                    return [head()]
        run = call
        if mode.endswith("graph"):
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(3):
                    call()
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            graph = torch.cuda.CUDAGraph()
            with capturing(graph, collect=True, stream=side, capture_error_mode="thread_local"):
                keep = call()                                # noqa: F841  (the static outputs live as long as the graph)
            run = graph.replay
        for _ in range(10):
            run()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(iters):
            run()
        torch.cuda.synchronize(dev)
        res[mode] = (time.perf_counter() - t0) / iters * 1e6
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sizes", default="45695,100000")
    ap.add_argument("--json", default=None)
    ap.add_argument("--precision", default="f32", choices=("f32", "bf16x3"), help="the fused op's precision (cross_attention_lbs_fused(precision=))")
    ap.add_argument("--package-root", default=ROOT, help="the built checkout moss_amd is imported from (default: this one)")
    ap.add_argument("--step", default=None, help="(internal) IMPL:P -- run that measurement in this process and print its JSON line")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    if args.step:
        impl, P = args.step.split(":")
        print(json.dumps({"impl": impl, "P": int(P), "precision": args.precision, "us_per_call": measure(impl, int(P), args.iters, args.precision),
                          "iters": args.iters}))
        return 0
    peak, peak_name, work = (BF16_MFMA_PEAK, "bf16", 3) if args.precision == "bf16x3" else (F32_MFMA_PEAK, "f32", 1)
    res = {}
    for P in (int(s) for s in args.sizes.split(",")):
        for impl in IMPLS:
            p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step",
                                f"{impl}:{P}", "--iters", str(args.iters), "--precision", args.precision, "--package-root",
                                args.package_root], stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                print(f"{impl} P={P}: exit status {p.returncode}; stopping here", flush=True)
                return p.returncode
            res[f"{impl}_{P}"] = json.loads(p.stdout.strip().splitlines()[-1])["us_per_call"]
            print(f"P = {P:6d} {impl:5s} " + "  ".join(f"{m} {res[f'{impl}_{P}'][m]:9.1f} us" for m in MODES), flush=True)
        t, f = res[f"torch_{P}"], res[f"fused_{P}"]
        for m in ("fwd", "fwd_bwd"):
            flop = 2 * MACS_PER_POINT * P * (3 if m == "fwd_bwd" else 1) * work
            print(f"P = {P:6d} {m}: torch eager / fused eager = {t[m] / f[m]:.1f}x, torch graph / fused graph = "
                  f"{t[m + '_graph'] / f[m + '_graph']:.1f}x, fused ({args.precision}) graph = "
                  f"{flop / (f[m + '_graph'] * 1e-6) / peak * 100:.1f} % of the {peak_name} matrix peak ({flop / 1e9:.1f} GFLOP)",
                  flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"iters": args.iters, "precision": args.precision, "us_per_call": res}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
