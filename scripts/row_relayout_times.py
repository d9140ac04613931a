#!/usr/bin/env python3
"""Times the ROW SURGERY of a densification event in its two forms, in one process, alternating, on the same seeded sets of 6 890,
45 695 and 100 000 Gaussians (unified-feature GaussianSet + GradBucket + capturable FlatAdamW + DensifyStats, no rasterizer):

  default    ``densification_event(...)``: FlatAdamW.append_rows / prune_rows per step of the event (torch indexing, two copies)
  one_pass   ``densification_event(..., one_pass=True)``: one row map, one gather launch (C ABI moss_rows_relayout)

  event      a scripted clone + split + prune (moss_amd.scenes.scripted_densification); the figure is the report's ``surgery_ms``
  decision   one ``densify_and_prune_fused`` with its appends and prunes (``one_pass`` False / True), host clock around the call,
             device-synchronised at both ends.  Above 45 695 rows MOSS skips the three phases: the decision is then the final prune.

    python scripts/row_relayout_times.py [--repeats 9] [--json profiles/row_relayout_times.json]
    python scripts/row_relayout_times.py --profile-run      # five one-pass events at 100 000 for a kernel trace; prints the bytes

Every run starts from a FRESH copy of the set (same seed), so both forms see the same rows; two warm-up runs per form fill torch's
caching allocator.  Median and (min, max) of ``--repeats`` runs are kept: the spread is the (min, max) of the same call.
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import densify_decision_times as ddt  # noqa: E402
from moss_amd import densify as D  # noqa: E402
from moss_amd import dist as mdist  # noqa: E402
from moss_amd import scenes  # noqa: E402
from moss_amd.gaussian_model import GaussianSet  # noqa: E402
from moss_amd.optim import FlatAdamW  # noqa: E402
from moss_amd.surgery import densification_event, reserve_workspace  # noqa: E402

SIZES = (6890, 45695, 100000)


def fresh(g, dev):
    """The set, its optimizer with non-trivial moments, and statistics -- from the inputs ``g`` (scripts/densify_decision_times.py)."""
    sc = SimpleNamespace(P=int(g["xyz"].shape[0]), means3D=g["xyz"], shs=torch.cat((g["features_dc"], g["features_rest"]), 1),
                         scales=torch.exp(g["scaling"]), rotations=g["rotation"], opacities=torch.sigmoid(g["opacity"]))
    pc = GaussianSet(sc, sh_degree=3, device=dev, unified_features=True)
    bucket = mdist.GradBucket(list(pc.parameters()))
    opt = FlatAdamW(pc.param_groups(), bucket, eps=1e-15, capturable=True)
    with torch.no_grad():
        pc._opacity.copy_(g["opacity"]); pc._scaling.copy_(g["scaling"])
        gen = torch.Generator(device=dev); gen.manual_seed(1)
        opt.exp_avg.copy_(torch.randn(opt.exp_avg.shape, generator=gen, device=dev))
        opt.exp_avg_sq.copy_(torch.rand(opt.exp_avg_sq.shape, generator=gen, device=dev))
        for n, off, nxt in zip(bucket.sizes, bucket.offsets, list(bucket.offsets[1:]) + [bucket.n_params]):
            opt.exp_avg[off + n:nxt] = 0; opt.exp_avg_sq[off + n:nxt] = 0
    stats = D.DensifyStats(sc.P, device=dev)
    stats.xyz_gradient_accum.copy_(g["accum"]); stats.denom.copy_(g["denom"]); stats.max_radii2D.copy_(g["max_radii2D"])
    return pc, opt, stats


def tensors(pc):
    return {"xyz": pc._xyz.data, "f_dc": pc._features.data[:, :1], "f_rest": pc._features.data[:, 1:], "opacity": pc._opacity.data,
            "scaling": pc._scaling.data, "rotation": pc._rotation.data}


def run_event(g, dev, one_pass):
    pc, opt, stats = fresh(g, dev)
    ev = scenes.scripted_densification(tensors(pc), 100, dev, reset_opacity=False)
    rep = densification_event(pc, opt, append=ev["append"], prune=ev["prune"], stats=stats, one_pass=one_pass)
    return rep["surgery_ms"], opt


def run_decision(g, dev, one_pass):
    pc, opt, stats = fresh(g, dev)
    gen = torch.Generator(device=dev); gen.manual_seed(2)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    rep = D.densify_and_prune_fused(pc, opt, stats, g["joint_F"], g["lbs_weights"], ddt.MAX_GRAD, ddt.MIN_OPACITY, ddt.EXTENT, 20, g["t_vertices"],
                                    generator=gen, percent_dense=ddt.PD, one_pass=one_pass)
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0), opt, rep


def relayout_bytes(rows_old, rows_app, rows_new, floats_per_row=59):
    """Bytes of ONE relayout computed from shapes: parameters and both moments written for every new row; read for every kept row (an
    appended row reads its parameters only); the int32 map."""
    kept = rows_new - min(rows_app, rows_new)
    return 4 * (3 * rows_new * floats_per_row + 3 * kept * floats_per_row + (rows_new - kept) * floats_per_row + rows_new)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-run", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("row_relayout_times.py measures on the GPU; none is available")
    dev = torch.device("cuda:0")
    reserve_workspace(3000 * 140000, dev)
    if args.profile_run:
        g = ddt.inputs(100000, dev)
        for _ in range(5):
            pc, opt, stats = fresh(g, dev)
            ev = scenes.scripted_densification(tensors(pc), 100, dev, reset_opacity=False)
            app = sum(int(a["new_xyz"].shape[0]) for a in ev["append"])
            rep = densification_event(pc, opt, append=ev["append"], prune=ev["prune"], stats=stats, one_pass=True)
        print(json.dumps({"P": 100000, "rows_app": app, "rows_after": rep["rows_after"],
                          "relayout_bytes": relayout_bytes(100000, app, rep["rows_after"])}), flush=True)
        return
    rows = []
    for P in SIZES:
        g = ddt.inputs(P, dev)
        r = {"P": P, "repeats": args.repeats}
        for what, fn in (("event_surgery", run_event), ("decision", run_decision)):
            ms = {False: [], True: []}
            for i in range(2 + args.repeats):                 # alternate the forms; the first two rounds warm up
                for one_pass in (False, True):
                    out = fn(g, dev, one_pass)
                    if i >= 2:
                        ms[one_pass].append(out[0])
                    last = out
            for one_pass, name in ((False, "default"), (True, "one_pass")):
                r[f"{what}_{name}_ms"] = statistics.median(ms[one_pass])
                r[f"{what}_{name}_ms_min_max"] = [min(ms[one_pass]), max(ms[one_pass])]
            r[f"{what}_below_by_more_than_spread"] = max(ms[True]) < min(ms[False])
            if what == "decision":
                r["decision_report_one_pass"] = {k: v for k, v in last[2].items()}
        rows.append(r)
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(args.json) or ".", exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
