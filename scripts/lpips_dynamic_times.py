#!/usr/bin/env python3
"""Times the LPIPS call whose crop size is read from the device (``cap_H``, ``cap_W`` of ``moss_lpips_vgg_args``) against the static
call, on one crop inside one frame: what a capacity costs -- the workgroups that leave at once, and the kernel shapes being picked by
the capacity's row count.

    python scripts/lpips_dynamic_times.py [--crop 256x176] [--frame 512x512] [--capacities 256x176,320x224,512x512]
                                          [--rounds 40] [--inner 5] [--other-lib PATH] [--json PATH]

Every variant is the same pair of C entry points (``moss_lpips_vgg_forward`` + ``_backward``: the training call) on the same frames and
the same rectangle, captured in a hipGraph of its own; they differ in the argument block alone:

    static          cap = 0: the crop's size is a launch argument
    static again    the same once more, a second graph with buffers of its own: the control -- what two captures of ONE code differ by
    dynamic HxW     the capacity H x W, the crop's size read from the rectangle on the device
    other static    ``--other-lib``: the static call of ANOTHER build of libmoss_raster.so (the parent commit's, to see that the static
                    path has not moved); it is handed the same argument block, of which it reads the part it knows

The variants are interleaved in one process: a round replays every variant's graph ``--inner`` times between two device events, in an
order that rotates from round to round; the first three rounds are discarded.  Reported per variant: the median, the minimum and the
10th / 90th percentile of the per-call time over the rounds, and the median over the rounds of its ratio to ``static`` IN THAT ROUND
(with the percentiles of that ratio: the spread a difference has to exceed).  The values and gradients of the variants are compared
bit for bit with ``static`` and the outcome is printed.  Needs a GPU; there is no CPU timing.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP_ROUNDS = 3


def pair(text):
    h, w = (int(v) for v in text.lower().split("x"))
    return h, w


class Variant:
    """One captured forward + backward through the C ABI of ``lib``."""

    def __init__(self, name, lib, net, image, gt, rect, crop, frame, cap):
        import torch
        from moss_amd._lib import LpipsVggArgs, LpipsVggBackwardArgs
        dev = image.device
        self.name, self.lib, self.dev = name, lib, dev
        size = cap or crop
        nws, nsv = int(lib.moss_lpips_vgg_workspace_bytes(*size)), int(lib.moss_lpips_vgg_saved_bytes(*size))
        self.keep = (torch.empty(nws, dtype=torch.uint8, device=dev), torch.empty(nsv, dtype=torch.uint8, device=dev),
                     torch.ones(1, device=dev), net, image, gt, rect)
        self.out, self.d_x = torch.zeros(6, device=dev), torch.zeros((3,) + tuple(frame), device=dev)
        a, b = LpipsVggArgs(), LpipsVggBackwardArgs()
        a.x, a.y = image.data_ptr(), gt.data_ptr()
        for blk in (a, b):
            blk.H, blk.W = crop
            blk.frame_H, blk.frame_W = frame
            blk.rect = rect.data_ptr()
            blk.cap_H, blk.cap_W = cap or (0, 0)
            blk.workspace, blk.workspace_bytes, blk.saved = self.keep[0].data_ptr(), nws, self.keep[1].data_ptr()
        for i in range(13):
            a.weights[i], a.biases[i], b.weights_bwd[i] = net.w_fwd[i].data_ptr(), net.biases[i].data_ptr(), net.w_bwd[i].data_ptr()
        for i in range(5):
            a.lin[i] = net.lin[i].data_ptr()
        a.shift, a.scale, a.out, a.terms = net.shift.data_ptr(), net.scale.data_ptr(), self.out.data_ptr(), self.out[1:].data_ptr()
        b.scale, b.g_out, b.dL_dx = net.scale.data_ptr(), self.keep[2].data_ptr(), self.d_x.data_ptr()
        self.a, self.b = a, b
        self.graph = None

    def enqueue(self):
        import torch
        s = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        for fn, blk in ((self.lib.moss_lpips_vgg_forward, self.a), (self.lib.moss_lpips_vgg_backward, self.b)):
            rc = fn(ctypes.byref(blk), s)
            if rc != 0:
                raise RuntimeError(f"{self.name}: the entry point returned {rc}: {self.lib.moss_last_error().decode()}")

    def capture(self):
        import torch
        from moss_amd.graphs import capturing
        side = torch.cuda.Stream(self.dev)
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):
            self.enqueue()
        torch.cuda.current_stream(self.dev).wait_stream(side)
        torch.cuda.synchronize(self.dev)
        self.graph = torch.cuda.CUDAGraph()
        with capturing(self.graph, collect=True, stream=side, capture_error_mode="thread_local"):
            self.enqueue()
        torch.cuda.synchronize(self.dev)


def load_other(path):
    """Another build's library with the prototypes of the float32 LPIPS calls alone (it may lack entry points newer than those)."""
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in ("moss_lpips_vgg_forward", "moss_lpips_vgg_backward"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]
    for name in ("moss_lpips_vgg_workspace_bytes", "moss_lpips_vgg_saved_bytes"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]
    lib.moss_last_error.restype = ctypes.c_char_p
    return lib


def percentile(values, q):
    v = sorted(values)
    return v[min(len(v) - 1, max(0, int(round(q * (len(v) - 1)))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crop", type=pair, default=(256, 176))
    ap.add_argument("--frame", type=pair, default=(512, 512))
    ap.add_argument("--capacities", default="256x176,320x224,512x512")
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--other-lib", default=None, help="another build of libmoss_raster.so whose static call is timed alongside")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    from moss_amd import lpips as mlp
    from moss_amd._lib import lib
    if not torch.cuda.is_available():
        print("lpips_dynamic_times: no GPU; there is no CPU timing", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    (h, w), (FH, FW) = args.crop, args.frame
    caps = [pair(c) for c in args.capacities.split(",") if c]
    for c in caps + [args.crop]:
        if c[0] > FH or c[1] > FW or c[0] < h or c[1] < w:
            raise SystemExit(f"{c[0]}x{c[1]}: every capacity must hold the crop and fit the frame")
    params = mlp.cast_params(mlp.synthetic_weights(1), device=dev)
    net = mlp.LpipsVGG.from_tensors(params["conv_weights"], params["conv_biases"], params["lin_weights"], params["shift"], params["scale"])
    gen = torch.Generator().manual_seed(1)
    gt = torch.rand(3, FH, FW, generator=gen).to(dev)
    image = (gt + 0.05 * torch.randn(3, FH, FW, generator=gen).to(dev)).clamp(0, 1)
    x0, y0 = (FW - w) // 2 | 1, (FH - h) // 2 | 1
    rect = torch.tensor([x0, y0, w, h, h * w], dtype=torch.int32, device=dev)
    variants = [Variant(n, lib(), net, image, gt, rect, args.crop, args.frame, None) for n in ("static", "static again")]
    if args.other_lib:
        variants.append(Variant("other static", load_other(args.other_lib), net, image, gt, rect, args.crop, args.frame, None))
    variants += [Variant(f"dynamic {c[0]}x{c[1]}", lib(), net, image, gt, rect, args.crop, args.frame, c) for c in caps]
    for v in variants:
        v.capture()
        for _ in range(3):
            v.graph.replay()
    torch.cuda.synchronize(dev)
    base = variants[0]
    for v in variants[1:]:
        same = torch.equal(v.out, base.out) and torch.equal(v.d_x, base.d_x)
        worst = float((v.d_x - base.d_x).abs().max() / base.d_x.abs().max())
        print(f"{v.name:18s} value and gradient {'bit-identical to static' if same else f'differ from static (max |d grad| / max |grad| = {worst:.2e})'}",
              flush=True)
    times = {v.name: [] for v in variants}
    for r in range(args.rounds + WARMUP_ROUNDS):
        order = variants[r % len(variants):] + variants[:r % len(variants)]
        this = {}
        for v in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                v.graph.replay()
            e1.record()
            e1.synchronize()
            this[v.name] = e0.elapsed_time(e1) * 1e3 / args.inner
        if r >= WARMUP_ROUNDS:
            for k, t in this.items():
                times[k].append(t)
    res = {}
    print(f"crop {h}x{w} at ({x0},{y0}) of a {FH}x{FW} frame, forward + backward from a graph, {args.rounds} rounds x {args.inner} replays, us per call")
    for v in variants:
        t = times[v.name]
        ratio = [a / b for a, b in zip(t, times["static"])]
        res[v.name] = {"median_us": statistics.median(t), "min_us": min(t), "p10_us": percentile(t, 0.1), "p90_us": percentile(t, 0.9),
                       "ratio_median": statistics.median(ratio), "ratio_p10": percentile(ratio, 0.1), "ratio_p90": percentile(ratio, 0.9)}
        s = res[v.name]
        print(f"{v.name:18s} median {s['median_us']:9.1f}  min {s['min_us']:9.1f}  p10..p90 {s['p10_us']:9.1f} .. {s['p90_us']:9.1f}   "
              f"/ static {s['ratio_median']:.4f} ({s['ratio_p10']:.4f} .. {s['ratio_p90']:.4f})", flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"crop": args.crop, "frame": args.frame, "rounds": args.rounds, "inner": args.inner, "results": res}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
