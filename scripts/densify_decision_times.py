#!/usr/bin/env python3
"""Times ONE whole densify-and-prune decision (scene/gaussian_model.py:621-666: joint table, clone, split, merge, final prune -- the
selections and the new rows, not the appends and prunes of the optimizer state, which both forms share) in two forms on the same
inputs, float32, V = 6 890, at P = 6 890 and P = 45 695:

  fused   moss_amd.densify.joint_tables / select_* / *_rows / prune_mask (C ABI moss_densify_joint_table / _select / _emit)
  torch   the ``*_torch`` composition on the device: the decision as a caller had to write it before these ops, with this project's
          cal_kl arithmetic already in place of MOSS's Python loop over P

    python scripts/densify_decision_times.py [--repeats 7] [--json profiles/densify_decision_times.json]

Each form runs the phases on the SAME set (no rows are appended between the phases: the sizes stay fixed and the forms comparable),
with the k = 2 and k = 1 neighbour queries of this project in both.  A run is device-synchronised at its start and end and timed
with the host clock (a decision contains host reads by nature); the median and (min, max) of ``--repeats`` runs after two warm-up runs
are kept.  Host reads: counted by moss_amd.densify.host_reads() for the fused form; for the torch form every boolean-mask index
(``torch.nonzero`` inside ``x[mask]``) is one, counted here.  Needs a GPU; there is no CPU timing.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from moss_amd import densify as D  # noqa: E402
from moss_amd.knn_cuda import knn  # noqa: E402

V = 6890
MAX_GRAD, MIN_OPACITY, EXTENT, PD = 0.0002, 0.1, 1.0, 0.01


def inputs(P, dev):
    rng = np.random.Generator(np.random.PCG64(P))
    f = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=dev)       # noqa: E731
    tv = rng.uniform(-0.5, 0.5, size=(V, 3))
    xyz = tv[rng.integers(0, V, size=P)] + 0.01 * rng.normal(size=(P, 3))
    denom = rng.integers(1, 9, size=(P, 1)).astype(np.float64)
    th = rng.uniform(0.05, 0.4, size=(23, 1, 1))
    ax = rng.normal(size=(23, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    Kx = np.zeros((23, 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    return {"xyz": f(xyz), "features_dc": f(rng.normal(size=(P, 1, 3))), "features_rest": f(rng.normal(size=(P, 15, 3))),
            "opacity": f(2 * rng.normal(size=(P, 1))), "scaling": f(np.log(PD * EXTENT) - 0.55 + 0.7 * rng.normal(size=(P, 3))),
            "rotation": f(rng.normal(size=(P, 4))), "accum": f(rng.uniform(0, 2 * MAX_GRAD, size=(P, 1)) * denom), "denom": f(denom),
            "max_radii2D": f(rng.uniform(0, 40, size=P)), "t_vertices": f(tv), "lbs_weights": f(denom[0, 0] * rng.dirichlet(np.ones(24), size=P)),
            "joint_F": f(denom[0, 0] * (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx))), "noise": f(rng.normal(size=(2 * P, 3)))}


PARAMS = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")


def fused(g):
    p = [g[k] for k in PARAMS]
    accum, denom = g["accum"].reshape(-1), g["denom"].reshape(-1)
    table = D.joint_tables(g["joint_F"], denom)
    ids = knn(g["xyz"][None], g["xyz"][None], 2)[1][0]
    m, idx, n = D.select_clone(g["xyz"], g["rotation"], g["scaling"], ids, accum, denom, MAX_GRAD, EXTENT, PD, 0.4)
    rows = [D.clone_rows(idx, g["noise"][:n].contiguous(), *p, g["lbs_weights"], denom, table)]
    ids = knn(g["xyz"][None], g["xyz"][None], 2)[1][0]
    m, idx, n = D.select_split(g["xyz"], g["rotation"], g["scaling"], ids, accum, denom, MAX_GRAD, EXTENT, PD, 0.4)
    rows.append(D.split_rows(idx, g["noise"][:2 * n].contiguous(), *p))
    ids = knn(g["xyz"][None], g["xyz"][None], 2)[1][0]
    m, idx, n = D.select_merge(g["xyz"], g["rotation"], g["scaling"], ids, accum, denom, MAX_GRAD, EXTENT, PD, 0.4)   # (0.4: random sets hold no near-duplicates; the merge still selects)
    rows.append(D.merge_rows(idx, ids, m.clone(), *p))
    dist = knn(g["t_vertices"][None], g["xyz"][None], 1)[0].reshape(-1)
    return rows, D.prune_mask(g["opacity"], g["scaling"], g["max_radii2D"], dist, MIN_OPACITY, EXTENT, 20)


def torch_form(g):
    p = [g[k] for k in PARAMS]
    accum, denom = g["accum"].reshape(-1), g["denom"].reshape(-1)
    table = D.joint_tables_torch(g["joint_F"], denom)
    ids = knn(g["xyz"][None], g["xyz"][None], 2)[1][0]
    m, idx, n = D.select_clone_torch(g["xyz"], g["rotation"], g["scaling"], ids, accum, denom, MAX_GRAD, EXTENT, PD, 0.4)
    rows = [D.clone_rows_torch(idx, g["noise"][:n], *p, g["lbs_weights"], denom, table)]
    ids = knn(g["xyz"][None], g["xyz"][None], 2)[1][0]
    m, idx, n = D.select_split_torch(g["xyz"], g["rotation"], g["scaling"], ids, accum, denom, MAX_GRAD, EXTENT, PD, 0.4)
    rows.append(D.split_rows_torch(idx, g["noise"][:2 * n], *p))
    ids = knn(g["xyz"][None], g["xyz"][None], 2)[1][0]
    m, idx, n = D.select_merge_torch(g["xyz"], g["rotation"], g["scaling"], ids, accum, denom, MAX_GRAD, EXTENT, PD, 0.4)
    rows.append(D.merge_rows_torch(idx, ids, m.clone(), *p))
    dist = knn(g["t_vertices"][None], g["xyz"][None], 1)[0].reshape(-1)
    return rows, D.prune_mask_torch(g["opacity"], g["scaling"], g["max_radii2D"], dist, MIN_OPACITY, EXTENT, 20)


class _CountNonzero(torch.overrides.TorchFunctionMode):
    """Counts the calls that make the host wait for a size: nonzero (also inside boolean-mask indexing) and .item()-like reads."""

    def __init__(self):
        super().__init__()
        self.reads = 0

    def __torch_function__(self, func, types, args=(), kwargs=None):
        name = getattr(func, "__name__", "")
        if name in ("nonzero", "item", "__bool__", "__int__") or (name == "__getitem__" and any(
                torch.is_tensor(a) and a.dtype == torch.bool for a in (args[1] if isinstance(args[1], tuple) else (args[1],)))):
            self.reads += 1
        return func(*args, **(kwargs or {}))


def timed(fn, g, repeats, dev):
    for _ in range(2):
        fn(g)
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn(g)
        torch.cuda.synchronize(dev)
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("densify_decision_times.py measures on the GPU; none is available")
    dev = torch.device("cuda:0")
    rows = []
    with torch.no_grad():
        for P in (6890, 45695):
            g = inputs(P, dev)
            r = {"P": P, "V": V, "repeats": args.repeats}
            for name, fn in (("fused", fused), ("torch", torch_form)):
                ms = timed(fn, g, args.repeats, dev)
                r[f"{name}_ms"], r[f"{name}_ms_min_max"] = statistics.median(ms), [min(ms), max(ms)]
            before = D.host_reads()
            fused(g)
            r["fused_host_reads"] = D.host_reads() - before
            with _CountNonzero() as c:
                torch_form(g)
            r["torch_host_reads"] = c.reads
            rows.append(r)
            print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(args.json) or ".", exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
