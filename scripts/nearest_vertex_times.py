#!/usr/bin/env python3
"""Times the nearest-template-vertex query (``moss_nearest_vertex_query``, csrc/nearest_vertex.hip) against what answers the same
question today, by the interleaved-graphs method of scripts/lpips_precision_times.py: per cell every variant is its C entry points
captured in a hipGraph of its own,

    n           the new query on an index built before the clock starts
    n again     the same once more, a second graph with outputs of its own: the control -- what two captures of ONE code differ by
    g           today's path as ``lbs.coarse_deform_c2source`` runs it on every step: ``moss_knn_grid_build`` + ``moss_knn_grid_query``
                (the workspace is allocated once here; ``knn()`` also allocates it per call)
    g kept      ``moss_knn_grid_query`` alone on a grid that is kept (``KnnGrid``)
    b           ``moss_knn_query``: brute force

all in one process, the graphs replayed in an order that rotates from round to round, the first three rounds discarded; reported per
variant: the median and the 10th / 90th percentile of the time, and the median and those percentiles of its per-round ratio to ``n``.
Before the timing the ids and distances of every variant are compared with ``b``'s.

The cells: P in {6 890, 45 695} x geometry x index order.  Geometry "near": template = ``scenes.body_points(6890)``, queries =
``scenes.body_points(P)`` (MOSS's regime: the Gaussians start on the template's vertices); "far": the world of
scripts/moss_step_times.py (the same queries against ``lbs.synthetic_body_model``'s template, which is another body).  Index order:
random, or ``densify.spatial_order``.

    python scripts/nearest_vertex_times.py [--sizes 6890,45695] [--geometries near,far] [--orders random,spatial] [--rounds 40] [--inner 5]
                                           [--calls 8] [--json PATH]

``--calls``: how many times a variant's graph holds its calls, back to back (the reported time is per call): a graph of ONE small
kernel is mostly the graph's own launch, which the captured training step does not pay per kernel.

Needs a GPU.
"""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from lpips_precision_times import measure  # noqa: E402

V = 6890


class Variant:
    def __init__(self, name, calls, P, dev, repeat=1):
        import torch
        self.name, self.calls, self.dev, self.repeat = name, calls, dev, repeat
        self.ids = torch.full((P,), -2, dtype=torch.int64, device=dev)
        self.dist = torch.full((P,), -1.0, dtype=torch.float32, device=dev)
        self.graph = None

    def enqueue(self):
        import torch
        from moss_amd._lib import check, lib
        s = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        for _ in range(self.repeat):
            for name, args in self.calls(self):
                check(getattr(lib(), name)(*args, s), name)

    def capture(self):
        import torch
        side = torch.cuda.Stream(self.dev)
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):
            self.enqueue()
        torch.cuda.current_stream(self.dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.enqueue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="6890,45695")
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--geometries", default="near,far")
    ap.add_argument("--orders", default="random,spatial")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    from moss_amd import lbs as mlbs
    from moss_amd import scenes
    from moss_amd._lib import lib
    from moss_amd.densify import spatial_order
    from moss_amd.knn_cuda import KnnGrid, TemplateIndex
    if not torch.cuda.is_available():
        print("nearest_vertex_times: no GPU; there is no CPU timing", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    templates = {"near": scenes.body_points(V, torch.Generator().manual_seed(3)).to(dev).contiguous(),
                 "far": mlbs.synthetic_body_model(V, 24, seed=21, device=dev)["v_template"].contiguous()}
    out = {}
    print("| P | geometry | order | n us | n again / n (p10 .. p90) | g / n | g kept / n | b / n | n < g by > 3 bands | n < b by > 3 bands |\n"
          "|---|---|---|---|---|---|---|---|---|---|")
    for P in (int(x) for x in args.sizes.split(",")):
        base = scenes.body_points(P, torch.Generator().manual_seed(4)).to(dev)
        for geometry in args.geometries.split(","):
            ref = templates[geometry]
            for order in args.orders.split(","):
                perm = torch.randperm(P, generator=torch.Generator().manual_seed(5)).to(dev) if order == "random" else spatial_order(base)
                q = base[perm].contiguous()
                index, grid = TemplateIndex(ref), KnnGrid(ref)
                ws = torch.empty(grid._bytes, dtype=torch.uint8, device=dev)        # (g)'s own grid, rebuilt by every replay
                new = lambda v: [("moss_nearest_vertex_query", (V, P, index._index.data_ptr(), index._bytes, q.data_ptr(), v.ids.data_ptr(), v.dist.data_ptr()))]  # noqa: E731
                variants = [
                    Variant("n", new, P, dev, args.calls), Variant("n again", new, P, dev, args.calls),
                    Variant("g", lambda v: [("moss_knn_grid_build", (V, ref.data_ptr(), ws.data_ptr(), grid._bytes)),
                                            ("moss_knn_grid_query", (V, P, 1, ws.data_ptr(), grid._bytes, q.data_ptr(), v.dist.data_ptr(), v.ids.data_ptr()))], P, dev, args.calls),
                    Variant("g kept", lambda v: [("moss_knn_grid_query", (V, P, 1, grid._ws.data_ptr(), grid._bytes, q.data_ptr(), v.dist.data_ptr(), v.ids.data_ptr()))], P, dev, args.calls),
                    Variant("b", lambda v: [("moss_knn_query", (V, P, 1, ref.data_ptr(), q.data_ptr(), v.dist.data_ptr(), v.ids.data_ptr()))], P, dev, args.calls)]
                for v in variants:
                    v.capture()
                    for _ in range(3):
                        v.graph.replay()
                torch.cuda.synchronize(dev)
                brute = variants[-1]
                for v in variants[:-1]:
                    if not (torch.equal(v.ids, brute.ids) and torch.equal(v.dist, brute.dist)):
                        raise SystemExit(f"P {P} {geometry} {order}: {v.name} DIFFERS from the brute-force query")
                res = out[f"{P} {geometry} {order}"] = measure(variants, args.rounds, args.inner)
                for stats in res.values():                                       # per call, not per graph
                    for k in ("median_us", "min_us", "p10_us", "p90_us"):
                        stats[k] /= args.calls
                band = res["n again"]["ratio_p90"] - res["n again"]["ratio_p10"]
                r = {k: res[k]["ratio_median"] for k in res}
                print(f"| {P} | {geometry} | {order} | {res['n']['median_us']:.1f} | {r['n again']:.3f} ({res['n again']['ratio_p10']:.3f} .. "
                      f"{res['n again']['ratio_p90']:.3f}) | {r['g']:.2f} | {r['g kept']:.2f} | {r['b']:.2f} | "
                      f"{'yes' if res['g']['ratio_p10'] - 1 > 3 * band else 'NO'} | {'yes' if res['b']['ratio_p10'] - 1 > 3 * band else 'NO'} |", flush=True)
                for v in variants:
                    s = res[v.name]
                    print(f"    {v.name:8s} median {s['median_us']:8.1f} us  p10..p90 {s['p10_us']:8.1f} .. {s['p90_us']:8.1f}   / n {s['ratio_median']:.3f} "
                          f"({s['ratio_p10']:.3f} .. {s['ratio_p90']:.3f})", file=sys.stderr, flush=True)
                del variants, brute
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"rounds": args.rounds, "inner": args.inner, "calls_per_graph": args.calls, "results": out}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
