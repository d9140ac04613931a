#!/usr/bin/env python3
"""Times the LPIPS term against a REFERENCE (``moss_lpips_vgg_forward_ref``: VGG16 on the render alone, the ground truth's tapped
activations read from a block computed once) against the two-image call, by the interleaved-graphs method of
scripts/lpips_precision_times.py: per size, precision and call (forward alone, keeping nothing; forward + backward) every variant is
the C entry points captured in a hipGraph of its own,

    two-image        the call of this build on (x, y)
    two-image again  the same once more, a second graph with buffers of its own: the control
    reference        the forward on x alone against y's reference block (+ the unchanged backward)

and, at the 256 x 176 sizes, on their own: ``reference pass`` (``moss_lpips_vgg_reference``: what is paid once per camera) and ``copy``
(``LpipsReference.copy_``: what a captured step pays per frame to change view).  All in one process: a round replays every variant's
graph ``--inner`` times between two device events, in an order that rotates from round to round, after a warm-up of every graph; the
first three rounds are discarded.  THE WHOLE SEQUENCE RUNS TWICE: the spread a difference has to exceed is that between the two
repetitions of the two-image call (and, inside a repetition, of ``two-image again`` to ``two-image``).

    python scripts/lpips_reference_times.py [--rounds 30] [--inner 5] [--precisions f32,bf16,bf16x3] [--json PATH]

Sizes: 256x176 static; 256x176 under a 320x224 capacity (512x512 frame); 512x352 static; 512x512 forward only (the evaluation call).
The weights are synthetic, y uniform in [0,1], x = clamp(y + 0.05 normal).  Needs a GPU.
"""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from lpips_dynamic_times import Variant  # noqa: E402
from lpips_precision_times import measure  # noqa: E402

# (crop, frame, capacity or None, the calls timed)
SIZES = [((256, 176), (256, 176), None, ("forward", "forward + backward")),
         ((256, 176), (512, 512), (320, 224), ("forward", "forward + backward")),
         ((512, 352), (512, 352), None, ("forward", "forward + backward")),
         ((512, 512), (512, 512), None, ("forward",))]


class Call(Variant):
    """A list of (entry point, block) captured in one graph.  ``kind``: "two-image", "reference" (the forward against ``block``),
    "pass" (the reference pass into ``block``) or "copy" (``dst.copy_(src)`` of two LpipsReference)."""

    def __init__(self, name, kind, lib, net, image, gt, rect, crop, frame, cap, backward, block=None, copy=None):
        super().__init__(name, lib, net, image, gt, rect, crop, frame, cap)
        from moss_amd._lib import LpipsVggForwardRefArgs, LpipsVggReferenceArgs
        from moss_amd.lpips import _SUFFIX
        suffix = _SUFFIX[net.precision]
        self.copy = copy
        fwd = self.a
        if kind in ("reference", "pass"):
            fwd = LpipsVggReferenceArgs() if kind == "pass" else LpipsVggForwardRefArgs()
            for f in ("H", "W", "frame_H", "frame_W", "rect", "shift", "scale", "workspace", "workspace_bytes", "cap_H", "cap_W"):
                setattr(fwd, f, getattr(self.a, f))
            for i in range(13):
                fwd.weights[i], fwd.biases[i] = self.a.weights[i], self.a.biases[i]
            fwd.reference, fwd.reference_bytes = block.data_ptr(), block.numel()
            if kind == "pass":
                fwd.y = gt.data_ptr()
            else:
                for i in range(5):
                    fwd.lin[i] = self.a.lin[i]
                fwd.x, fwd.out, fwd.terms, fwd.saved = self.a.x, self.a.out, self.a.terms, self.a.saved
        if not backward and kind != "pass":
            fwd.saved = None
        entry = {"two-image": "moss_lpips_vgg_forward", "reference": "moss_lpips_vgg_forward_ref", "pass": "moss_lpips_vgg_reference"}
        self.calls = [] if kind == "copy" else [(getattr(lib, entry[kind] + suffix), fwd)]
        if backward:
            self.calls.append((getattr(lib, "moss_lpips_vgg_backward" + suffix), self.b))

    def enqueue(self):
        import torch
        if self.copy is not None:
            self.copy[0].copy_(self.copy[1])
        s = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        for fn, blk in self.calls:
            rc = fn(ctypes.byref(blk), s)
            if rc != 0:
                raise RuntimeError(f"{self.name}: the entry point returned {rc}: {self.lib.moss_last_error().decode()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--precisions", default="f32,bf16,bf16x3")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    from moss_amd import lpips as mlp
    from moss_amd._lib import lib
    from moss_amd.loss import ViewRegion
    if not torch.cuda.is_available():
        print("lpips_reference_times: no GPU; there is no CPU timing", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    params = mlp.cast_params(mlp.synthetic_weights(1), device=dev)
    out = {}
    for precision in args.precisions.split(","):
        net = mlp.LpipsVGG.from_tensors(params["conv_weights"], params["conv_biases"], params["lin_weights"], params["shift"], params["scale"],
                                        precision=precision)
        for crop, frame, cap, calls in SIZES:
            (h, w), (FH, FW) = crop, frame
            gen = torch.Generator().manual_seed(1)
            gt = torch.rand(3, FH, FW, generator=gen).to(dev)
            image = (gt + 0.05 * torch.randn(3, FH, FW, generator=gen).to(dev)).clamp(0, 1)
            x0, y0 = ((FW - w) // 2 | 1, (FH - h) // 2 | 1) if frame != crop else (0, 0)
            region = ViewRegion(torch.ones(1, FH, FW, device=dev), rect=(x0, y0, w, h))
            ref = mlp.lpips_vgg_roi_reference(net, gt, region, capacity=cap)
            where = f"{h}x{w}" + (f" under {cap[0]}x{cap[1]}" if cap else "")
            for what in calls:
                backward = what == "forward + backward"
                mk = lambda name, kind, **kw: Call(name, kind, lib(), net, image, gt, region.rect, crop, frame, cap, backward, **kw)  # noqa: E731
                variants = [mk("two-image", "two-image"), mk("two-image again", "two-image"), mk("reference", "reference", block=ref.block)]
                if backward and crop == (256, 176):                      # (once per size: these two have no backward)
                    scratch, static = mlp.LpipsReference.empty(net, cap or crop, static=cap is None), mlp.LpipsReference.empty(net, cap or crop, static=cap is None)
                    variants += [Call("reference pass", "pass", lib(), net, image, gt, region.rect, crop, frame, cap, False, block=scratch.block),
                                 Call("copy", "copy", lib(), net, image, gt, region.rect, crop, frame, cap, False, copy=(static, ref))]
                for v in variants:
                    v.capture()
                    for _ in range(3):
                        v.graph.replay()
                torch.cuda.synchronize(dev)
                base, again, refv = variants[:3]
                for v in (again, refv):
                    same = torch.equal(v.out, base.out) and (not backward or torch.equal(v.d_x, base.d_x))
                    rel = abs(float(v.out[0]) - float(base.out[0])) / float(base.out[0])
                    grel = float((v.d_x - base.d_x).norm() / base.d_x.norm()) if backward else 0.0
                    print(f"{precision} {where} {what}: {v.name} is " + ("bit-identical to two-image" if same else
                          f"NOT bit-identical to two-image (the kernel shapes differ): value relative {rel:.3g}, gradient relative L2 {grel:.3g}"),
                          flush=True)
                reps = [measure(variants, args.rounds, args.inner) for _ in range(2)]         # the whole sequence, twice
                key = f"{precision} {where} {what}"
                t2 = [r["two-image"]["median_us"] for r in reps]
                spread = abs(t2[0] - t2[1]) / (0.5 * (t2[0] + t2[1]))
                ratios = [r["reference"]["ratio_median"] for r in reps]
                control = [r["two-image again"]["ratio_median"] for r in reps]
                out[key] = {"repetitions": reps, "control_spread": spread, "reference_over_two_image": ratios, "again_over_two_image": control,
                            "reference_bytes": ref.nbytes}
                print(f"{key} from a graph, 2 x {args.rounds} rounds x {args.inner} replays, median us per call (repetition 1, 2)")
                for v in variants:
                    print(f"  {v.name:16s} {reps[0][v.name]['median_us']:9.1f} {reps[1][v.name]['median_us']:9.1f}   / two-image "
                          f"{reps[0][v.name]['ratio_median']:.4f} {reps[1][v.name]['ratio_median']:.4f}  (p10..p90 of repetition 1: "
                          f"{reps[0][v.name]['ratio_p10']:.4f} .. {reps[0][v.name]['ratio_p90']:.4f})", flush=True)
                faster = max(ratios) < 1.0 - spread and max(ratios) < min(control + [1.0]) - abs(control[0] - control[1])
                print(f"  control: two-image repetition 1 against 2 differ by {100 * spread:.2f} %; the reference call is "
                      f"{100 * (1 - max(ratios)):.1f} .. {100 * (1 - min(ratios)):.1f} % faster: "
                      f"{'the margin exceeds the spread' if faster else 'the margin does NOT exceed the spread'}; block {ref.nbytes} bytes", flush=True)
                del variants, base, again, refv, v
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"rounds": args.rounds, "inner": args.inner, "results": out}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
