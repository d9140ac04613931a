#!/usr/bin/env python3
"""Wall time and file size of ``moss_amd.checkpoint``'s four calls at P = 6 890 and 45 695 Gaussians, beside the per-step time of the same
build (scripts/moss_step_times.py's world, frames and timer), so that the cost reads as "k steps":

    save_checkpoint     a captured MossStep with statistics -> one file
    load_checkpoint     that file into a captured step of the same size (probe and re-capture included); at the larger size also into a
                        captured step built from the 6 890-vertex initialisation (the rows are re-laid first)
    save_scene          MOSS's model directory: point_cloud.ply + ckpt.pth
    load_scene          that directory into a fresh model (no optimizer)

Every call is device-synchronised before and after and run three times.  Prints one JSON line per size; ``--out FILE`` also writes them.

    python scripts/checkpoint_times.py [--sizes 6890,45695] [--replays 200] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def _step(w, capture=True):
    from moss_amd.densify import DensifyStats
    from moss_amd.train import MossStep
    from moss_step_times import LR_HEAD, LR_NET
    pc = w["pc"]
    step = MossStep(pc, w["cam"], w["gt"], w["bkgd"], w["region"], w["bg"], w["lpips"], {"auto_regression": LR_HEAD, "cross_attention_lbs": LR_NET},
                    stats=DensifyStats(int(pc._xyz.shape[0]), pc._xyz.device))
    return step.capture(warmup=3) if capture else step


def measure(P, replays, folder):
    import torch
    from moss_amd import checkpoint as ck
    from moss_step_times import _frame, _timed, _world
    dev = torch.device("cuda:0")

    def timed(fn):
        out = []
        for _ in range(3):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            out.append(round(1e3 * (time.perf_counter() - t0), 2))
        return out
    w = _world(P, dev, unified=True)
    step = _step(w)
    frames = [_frame(k, dev) for k in range(3)]

    def load(i):
        for key, v in frames[i % 3].items():
            w["cam"].smpl_param[key].copy_(v)
    dt = _timed(step, replays, dev, load)
    step.check()
    path, root = os.path.join(folder, f"chkpnt_{P}.pth"), os.path.join(folder, f"model_{P}")
    row = {"P": P, "us_per_step": round(dt * 1e6, 1), "steps_at_save": list(step.step_counts())}
    row["save_checkpoint_ms"] = timed(lambda: ck.save_checkpoint(step, path, 1))
    row["checkpoint_bytes"] = os.path.getsize(path)
    row["load_checkpoint_captured_ms"] = timed(lambda: ck.load_checkpoint(step, path))
    row["save_scene_ms"] = timed(lambda: ck.save_scene(root, 1, w["pc"]))
    ply, ckpt = ck._ply_path(root, 1), ck._mlp_path(root, 1)
    row["ply_bytes"], row["ckpt_pth_bytes"] = os.path.getsize(ply), os.path.getsize(ckpt)
    fresh = [_world(P, dev, unified=True)["pc"] for _ in range(3)]
    row["load_scene_ms"] = timed(lambda: ck.load_scene(root, fresh.pop()))
    out = step()
    torch.cuda.synchronize(dev)
    assert step.dropped_frames == 0 and float(out["render"].abs().max()) > 0 and bool(torch.isfinite(out["terms"]).all())
    if P > 6890:
        small = [_step(_world(6890, dev, unified=True)) for _ in range(3)]
        row["load_checkpoint_into_6890_captured_ms"] = timed(lambda: ck.load_checkpoint(small.pop(), path))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="6890,45695")
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    with tempfile.TemporaryDirectory() as folder:
        for P in (int(x) for x in a.sizes.split(",")):
            rows.append(measure(P, a.replays, folder))
            print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
