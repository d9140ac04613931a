#!/usr/bin/env python3
"""Times MOSS's LPIPS term (VGG16): the fused op (moss_amd.lpips.lpips_vgg_fused, the HIP kernels of csrc/lpips.hip) replayed from a
captured hipGraph, and the torch form (moss_amd.lpips.lpips_vgg_torch in float32 on the GPU -- the stand-in for MOSS's module: 26 MIOpen
convolutions and the small kernels around them) replayed from a graph and eagerly, after a warm-up that lets MIOpen finish its
search.  Forward alone (the evaluation call, under no_grad) and forward + backward to x (the training call); the peak device memory
of one training call of each form on top of what is allocated before it (torch.cuda.max_memory_allocated).

    python scripts/lpips_times.py [--iters 20] [--sizes 256x176,512x352,512x512:fwd,1024x1024:fwd] [--precision f32|bf16] [--json PATH]

A size with ``:fwd`` is timed forward only.  Every (implementation, size) is a process of its own under ``timeout``; the script stops
at the first one that does not exit with 0.  A time is the wall clock around ``iters`` back-to-back calls between two device
synchronisations, per call, after a warm-up.  The weights are synthetic (moss_amd.lpips.synthetic_weights): the arithmetic does not
depend on their values.  ``--precision bf16`` times the fused op's bf16-operand mode (``LpipsVGG(precision="bf16")``; the torch form
is float32 either way, and the share printed stays that of the f32 matrix peak).  Needs a GPU; there is no CPU timing.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMPLS = ("fused", "torch")
STEP_TIMEOUT = 280
F32_MFMA_PEAK = 157.3e12


def flop_per_pass(H, W):
    """Multiply-adds x 2 of one VGG16 features[0:30] pass over one H x W image (the convolutions only)."""
    from moss_amd.lpips import CONV_SHAPES, POOL_AFTER_CONV
    total, h, w = 0, H, W
    for i, (co, ci, _, _) in enumerate(CONV_SHAPES):
        total += 2 * 9 * ci * co * h * w
        if i in POOL_AFTER_CONV:
            h, w = h // 2, w // 2
    return total


def measure(impl, H, W, fwd_only, iters, precision="f32"):
    import torch
    from moss_amd import lpips as mlp
    from moss_amd.graphs import capturing
    dev = torch.device("cuda:0")
    params = mlp.cast_params(mlp.synthetic_weights(1), device=dev)
    gen = torch.Generator().manual_seed(1)
    y = torch.rand(3, H, W, generator=gen).to(dev)
    x = (y + 0.05 * torch.randn(3, H, W, generator=gen).to(dev)).clamp(0, 1).requires_grad_(True)
    if impl == "torch":
        term = lambda: mlp.lpips_vgg_torch(params, x, y)                            # noqa: E731
    else:
        net = mlp.LpipsVGG.from_tensors(params["conv_weights"], params["conv_biases"], params["lin_weights"], params["shift"], params["scale"],
                                        precision=precision)
        term = lambda: mlp.lpips_vgg_fused(net, x, y)                               # noqa: E731

    def fwd():
        with torch.no_grad():
            return [term()]

    def fwd_bwd():
        return [g.detach() for g in torch.autograd.grad(term().sum(), [x])]

    res = {}
    modes = [("fwd", fwd)] + ([] if fwd_only else [("fwd_bwd", fwd_bwd)])
    for name, call in modes:
        for _ in range(3):                                   # (MIOpen's first-use search happens here)
            call()
        torch.cuda.synchronize(dev)
        if name == "fwd_bwd":
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            call()
            torch.cuda.synchronize(dev)
            res["train_peak_mib"] = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
        variants = [("graph", None)] + ([("eager", call)] if impl == "torch" else [])
        for vname, run in variants:
            if run is None:
                side = torch.cuda.Stream(dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    call()
                torch.cuda.current_stream(dev).wait_stream(side)
                torch.cuda.synchronize(dev)
                graph = torch.cuda.CUDAGraph()
                with capturing(graph, collect=True, stream=side, capture_error_mode="thread_local"):
                    keep = call()                            # noqa: F841  (the static outputs live as long as the graph)
                run = graph.replay
            for _ in range(3):
                run()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(iters):
                run()
            torch.cuda.synchronize(dev)
            res[f"{name}_{vname}"] = (time.perf_counter() - t0) / iters * 1e6
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", default="256x176,512x352,512x512:fwd,1024x1024:fwd")
    ap.add_argument("--impls", default=",".join(IMPLS))
    ap.add_argument("--precision", default="f32", choices=("f32", "bf16"), help="the fused op's operand precision")
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help="(internal) IMPL:HxW[:fwd] -- run that measurement in this process and print its JSON line")
    args = ap.parse_args()
    if args.step:
        impl, size, *rest = args.step.split(":")
        H, W = (int(v) for v in size.split("x"))
        print(json.dumps({"impl": impl, "size": size, "us_per_call": measure(impl, H, W, bool(rest), args.iters, args.precision), "iters": args.iters}))
        return 0
    res = {}
    for spec in args.sizes.split(","):
        size = spec.split(":")[0]
        H, W = (int(v) for v in size.split("x"))
        for impl in args.impls.split(","):
            p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step",
                                f"{impl}:{spec}", "--iters", str(args.iters), "--precision", args.precision], stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                print(f"{impl} {size}: exit status {p.returncode}; stopping here", flush=True)
                return p.returncode
            r = res[f"{impl}_{size}"] = json.loads(p.stdout.strip().splitlines()[-1])["us_per_call"]
            print(f"{size:>9s} {impl:5s} " + "  ".join(f"{k} {v:10.1f}" + (" MiB" if k.endswith("mib") else " us") for k, v in r.items()), flush=True)
            if impl == "fused":
                # both images forward (2 passes); the data gradient of x is one more pass less conv 1_1's share
                for mode, passes in (("fwd_graph", 2), ("fwd_bwd_graph", 3)):
                    if mode in r:
                        flop = passes * flop_per_pass(H, W)
                        print(f"{size:>9s} fused {mode}: {flop / 1e9:.1f} GFLOP, {flop / (r[mode] * 1e-6) / 1e12:.1f} TFLOP/s = "
                              f"{flop / (r[mode] * 1e-6) / F32_MFMA_PEAK * 100:.1f} % of the f32 matrix peak", flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"iters": args.iters, "precision": args.precision, "results": res}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
