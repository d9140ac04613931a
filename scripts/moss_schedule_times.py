#!/usr/bin/env python3
"""Times MOSS's whole training SCHEDULE (``train_ZJU.py:82-95,171-186``) on ``moss_amd.train.MossStep``: 3 000 iterations from P = 6 890
Gaussians, the densification event every 100 iterations from 400 to 2 000 (MOSS's own decision, ``step.densify_and_prune``), the SH
degree raised at 1 000, 2 000 and 3 000 from degree 0, the position's learning rate decayed every iteration, three frames drawn
without replacement -- ``moss_amd.train.run_schedule`` -- in two forms on the same commit:

    captured   the step replayed from its hipGraph, captured again by every event and degree raise
    eager      the same schedule with ``step.compute()`` in the place of the replay (same events, same decision, same noise)

    python scripts/moss_schedule_times.py [--iterations 3000] [--only captured,eager] [--out DIR]

The body, the networks, the LPIPS weights, the targets and the three frames are those of ``scripts/moss_step_times.py``: SYNTHETIC.  What the
densification decision does on them (how many Gaussians it clones, splits and prunes, the size the set ends with) says nothing about
MOSS's data; the times per iteration at a given size and per event do.  Each form is a process of its own under ``timeout -k 10``; the
script stops at the first one that does not exit with 0.  A form's time is the wall clock of ``run_schedule`` between two device
synchronisations (the events synchronise by nature, and the ends of the three phases are synchronised to time them).  Needs a GPU.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FORM_TIMEOUT = 900
P0 = 6890
# MOSS's arguments (arguments/__init__.py, train_ZJU.py:177): densify_grad_threshold, the minimum opacity, the position rate's decay
MAX_GRAD, MIN_OPACITY = 0.0002, 0.005
LR_XYZ_INIT, LR_XYZ_FINAL, LR_XYZ_STEPS = 0.00016, 0.0000016, 30000


def xyz_rate(i):
    """``get_expon_lr_func`` without a delay: log-linear from the initial to the final rate over ``LR_XYZ_STEPS`` iterations."""
    t = min(max(i / LR_XYZ_STEPS, 0.0), 1.0)
    return math.exp(math.log(LR_XYZ_INIT) * (1 - t) + math.log(LR_XYZ_FINAL) * t)


def measure(form, iterations):
    import torch
    sys.path.insert(0, HERE)
    import moss_step_times as mst
    from moss_amd.densify import DensifyStats
    from moss_amd.train import MossStep, run_schedule
    dev = torch.device("cuda:0")
    w = mst._world(P0, dev, unified=True)
    pc = w["pc"]
    pc.active_sh_degree = 0                                  # MOSS starts at degree 0 with features_rest = 0 (scene/gaussian_model.py:179-181)
    with torch.no_grad():
        pc._features[:, 1:, :] = 0.0
        # (scene.cameras_extent comes from the training cameras; this scene has one, so the body's own radius stands in)
        extent = 1.1 * float((pc._xyz - pc._xyz.mean(dim=0)).norm(dim=1).max())
    step = MossStep(pc, w["cam"], w["gt"], w["bkgd"], w["region"], w["bg"], w["lpips"],
                    {"auto_regression": mst.LR_HEAD, "cross_attention_lbs": mst.LR_NET}, stats=DensifyStats(P0, dev))
    frames = [mst._frame(k, dev) for k in range(3)]

    def load(k):                                             # a new frame: five small copies into the static inputs
        for key, v in frames[k].items():
            w["cam"].smpl_param[key].copy_(v)

    if form == "captured":
        step.capture(warmup=3)                               # (undoes its warm-up steps: both forms start from the same model)
    else:
        state = step._state()                                # the same three warm-up steps, undone the same way: the process's
        for _ in range(3):                                   # first-call costs stay out of both clocks
            step.compute()
        step._restore(state)
    report = run_schedule(step, 3, iterations, lr_schedule=lambda i: {"xyz": xyz_rate(i)}, load_frame=load,
                          densify=dict(max_grad=MAX_GRAD, min_opacity=MIN_OPACITY, extent=extent,
                                       generator=torch.Generator(device=dev).manual_seed(0)))
    torch.cuda.synchronize(dev)
    if form != "captured":
        step.context.check_status()
    assert bool(torch.isfinite(step.terms).all()) and report["rows"] > 0
    events = report.pop("events")
    med = lambda k: round(statistics.median(e[k] for e in events), 3) if events else None      # noqa: E731
    return dict(report, form=form, extent=round(extent, 4), sh_degree=int(pc.active_sh_degree), steps=list(step.step_counts()),
                total_loss=float(step.terms[-1]), n_events=len(events),
                event_ms_median={k: med(k) for k in ("event_ms", "surgery_ms", "probe_ms", "capture_ms")},
                event_ms_max=max((e["event_ms"] for e in events), default=None),
                events=[{k: e[k] for k in ("iteration", "rows_before", "cloned", "split", "merged", "pruned", "rows_after", "relayouts",
                                           "host_reads", "event_ms", "surgery_ms", "probe_ms", "capture_ms", "recaptured")} for e in events])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=3000)
    ap.add_argument("--only", default="captured,eager")
    ap.add_argument("--out", default="moss_step_times_out")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.worker:
        print("RESULT " + json.dumps(measure(a.worker, a.iterations)), flush=True)
        return
    os.makedirs(a.out, exist_ok=True)
    results = []
    for form in a.only.split(","):
        cmd = ["timeout", "-k", "10", str(FORM_TIMEOUT), sys.executable, os.path.abspath(__file__), "--iterations", str(a.iterations), "--worker", form]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
        log = os.path.join(a.out, f"schedule_{form}.log")
        with open(log, "w") as f:
            f.write(r.stdout)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            print(f"{form}: exit {r.returncode}; stopping (log: {log})\n" + r.stdout[-3000:], flush=True)
            raise SystemExit(1)
        res = json.loads(line[7:])
        results.append(res)
        print(json.dumps({k: v for k, v in res.items() if k != "events"}), flush=True)
        print("| iteration | rows before | cloned | split | merged | pruned | rows after | event ms | surgery | probe | capture |\n|---|---|---|---|---|---|---|---|---|---|---|")
        for e in res["events"]:
            print(f"| {e['iteration']} | {e['rows_before']} | {e['cloned']} | {e['split']} | {e['merged']} | {e['pruned']} | {e['rows_after']} | "
                  f"{e['event_ms']:.2f} | {e['surgery_ms']:.2f} | {e['probe_ms']:.2f} | {e['capture_ms']:.2f} |", flush=True)
    with open(os.path.join(a.out, "schedule_results.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
