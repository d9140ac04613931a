#!/usr/bin/env python3
"""Times the LPIPS term's bf16-operand mode (``LpipsVGG(precision="bf16")``; ``moss_lpips_vgg_forward_bf16`` / ``_backward_bf16``) and its
split-bf16 mode (``precision="bf16x3"``; ``moss_lpips_vgg_forward_bf16x3`` / ``_backward_bf16x3``) against the float32 call, by the
interleaved-graphs method of scripts/lpips_dynamic_times.py: per size and per call (forward alone, keeping nothing; forward +
backward), every variant is the pair of C entry points captured in a hipGraph of its own,

    f32             the float32 call of this build
    f32 again       the same once more, a second graph with buffers of its own: the control -- what two captures of ONE code differ by
    f32 other       ``--other-lib``: the float32 call of ANOTHER build of libmoss_raster.so (the parent commit's: has the float32 path moved?)
    bf16            the bf16-operand call
    bf16x3          the split-bf16 (three-product) call

all in one process: a round replays every variant's graph ``--inner`` times between two device events, in an order that rotates from
round to round; the first three rounds are discarded.  Reported per variant: the median, the minimum and the 10th / 90th percentile of
the per-call time, and the median over the rounds of its ratio to ``f32`` IN THAT ROUND with the percentiles of that ratio -- the
spread a difference has to exceed.

    python scripts/lpips_precision_times.py [--sizes 256x176,512x352,512x512] [--rounds 40] [--inner 5] [--other-lib PATH] [--json PATH]

The weights are synthetic (``moss_amd.lpips.synthetic_weights``), y uniform in [0,1], x = clamp(y + 0.05 normal).  Needs a GPU.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from lpips_dynamic_times import WARMUP_ROUNDS, Variant, load_other, pair, percentile  # noqa: E402


class PrecisionVariant(Variant):
    """The static call of ``lib`` with ``net``'s precision; ``backward`` False: the forward alone, with nothing kept."""

    def __init__(self, name, lib, net, image, gt, rect, size, backward):
        super().__init__(name, lib, net, image, gt, rect, size, size, None)
        from moss_amd.lpips import _SUFFIX
        suffix = _SUFFIX[net.precision]
        self.calls = [(getattr(lib, "moss_lpips_vgg_forward" + suffix), self.a)]
        if backward:
            self.calls.append((getattr(lib, "moss_lpips_vgg_backward" + suffix), self.b))
        else:
            self.a.saved = None

    def enqueue(self):
        import torch
        s = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        for fn, blk in self.calls:
            rc = fn(ctypes.byref(blk), s)
            if rc != 0:
                raise RuntimeError(f"{self.name}: the entry point returned {rc}: {self.lib.moss_last_error().decode()}")


def measure(variants, rounds, inner):
    import torch
    times = {v.name: [] for v in variants}
    for r in range(rounds + WARMUP_ROUNDS):
        order = variants[r % len(variants):] + variants[:r % len(variants)]
        this = {}
        for v in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                v.graph.replay()
            e1.record()
            e1.synchronize()
            this[v.name] = e0.elapsed_time(e1) * 1e3 / inner
        if r >= WARMUP_ROUNDS:
            for k, t in this.items():
                times[k].append(t)
    res = {}
    for v in variants:
        t = times[v.name]
        ratio = [a / b for a, b in zip(t, times[variants[0].name])]
        res[v.name] = {"median_us": statistics.median(t), "min_us": min(t), "p10_us": percentile(t, 0.1), "p90_us": percentile(t, 0.9),
                       "ratio_median": statistics.median(ratio), "ratio_p10": percentile(ratio, 0.1), "ratio_p90": percentile(ratio, 0.9)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256x176,512x352,512x512")
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--other-lib", default=None, help="another build of libmoss_raster.so whose float32 call is timed alongside")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    from moss_amd import lpips as mlp
    from moss_amd._lib import lib
    if not torch.cuda.is_available():
        print("lpips_precision_times: no GPU; there is no CPU timing", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    params = mlp.cast_params(mlp.synthetic_weights(1), device=dev)
    nets = {p: mlp.LpipsVGG.from_tensors(params["conv_weights"], params["conv_biases"], params["lin_weights"], params["shift"], params["scale"],
                                         precision=p) for p in mlp.ALL_PRECISIONS}
    other = load_other(args.other_lib) if args.other_lib else None
    out = {}
    for size in (pair(s) for s in args.sizes.split(",")):
        h, w = size
        gen = torch.Generator().manual_seed(1)
        gt = torch.rand(3, h, w, generator=gen).to(dev)
        image = (gt + 0.05 * torch.randn(3, h, w, generator=gen).to(dev)).clamp(0, 1)
        rect = torch.tensor([0, 0, w, h, h * w], dtype=torch.int32, device=dev)
        for backward in (False, True):
            what = "forward + backward" if backward else "forward"
            variants = [PrecisionVariant(n, lib(), nets["f32"], image, gt, rect, size, backward) for n in ("f32", "f32 again")]
            if other is not None:
                variants.append(PrecisionVariant("f32 other", other, nets["f32"], image, gt, rect, size, backward))
            reduced = [PrecisionVariant(p, lib(), nets[p], image, gt, rect, size, backward) for p in mlp.ALL_PRECISIONS[1:]]
            variants += reduced
            for v in variants:
                v.capture()
                for _ in range(3):
                    v.graph.replay()
            torch.cuda.synchronize(dev)
            base = variants[0]
            for v in variants[1:-len(reduced)]:
                same = torch.equal(v.out, base.out) and (not backward or torch.equal(v.d_x, base.d_x))
                print(f"{h}x{w} {what}: {v.name} is {'bit-identical to' if same else 'DIFFERENT from'} f32", flush=True)
            for b in reduced:
                rel = abs(float(b.out[0]) - float(base.out[0])) / float(base.out[0])
                grel = float((b.d_x - base.d_x).norm() / base.d_x.norm()) if backward else float("nan")
                print(f"{h}x{w} {what}: {b.name} value {float(b.out[0]):.8g} against f32 {float(base.out[0]):.8g} (relative {rel:.3g}), gradient "
                      f"relative L2 difference {grel:.3g}", flush=True)
            res = out[f"{h}x{w} {what}"] = measure(variants, args.rounds, args.inner)
            print(f"{h}x{w} {what} from a graph, {args.rounds} rounds x {args.inner} replays, us per call")
            for v in variants:
                s = res[v.name]
                print(f"  {v.name:10s} median {s['median_us']:9.1f}  min {s['min_us']:9.1f}  p10..p90 {s['p10_us']:9.1f} .. {s['p90_us']:9.1f}   "
                      f"/ f32 {s['ratio_median']:.4f} ({s['ratio_p10']:.4f} .. {s['ratio_p90']:.4f})", flush=True)
            del variants, reduced, base, b
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"rounds": args.rounds, "inner": args.inner, "results": out}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
