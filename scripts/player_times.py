#!/usr/bin/env python3
"""Times of ``moss_amd.play`` on the GPU (scripts/moss_step_times.py's world and frames, 512 x 512):

    control         eager ``gaussian_renderer.render`` with the seven in-op flags under ``torch.no_grad()``, a new frame per call: what a
                    caller had before ``MossPlayer`` (this configuration imports nothing of ``moss_amd.play``)
    frame           ``MossPlayer.frame()`` replayed, a new frame per call        pose / render: its two halves alone
    frame_index     the same with ``template_index=True`` (the nearest-vertex query through an index built once)     pose_index: its pose half
    split_grouped   ``evaluate_split`` per view on a synthetic split of 17 poses x 4 cameras of different intrinsics, LPIPS included;
    split_ungrouped the same views without ``pose_id`` (posed per view)
    u8              ``frames_to_u8`` at 512 x 512 and 1024 x 1024, 1 and 8 frames per launch, RGB and RGBA: us per launch, bytes moved per
                    frame (12 or 16 read + 1 of the mask, 3 or 4 written per pixel) and the share of ``--hbm-gbs`` that is

Every configuration runs in a process of its own; the list is gone through ``--rounds`` times (default 2), so that the runs of one
configuration are minutes apart and alternate with the others; the summary gives each configuration's runs, the ratio to the control
of the same size, and the control's own spread (max / min of its runs) beside it.  Times are host clocks around device-synchronised
windows of ``--calls`` calls after 20 warm-up calls.

    python scripts/player_times.py [--sizes 6890,45695] [--calls 300] [--rounds 2] [--configs control,frame,...] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

FLAGS = ("lbs_in_op", "pose_head_in_op", "lbs_weights_in_op", "smpl_frame_in_op", "transforms_in_op", "pose_in_op", "raw_parameters_in_op")


def _world_and_frames(P, dev):
    from moss_step_times import _frame, _world
    w = _world(P, dev, unified=True)
    return w, [_frame(k, dev) for k in range(3)]


def _cameras(cam, n, dev):
    """``n`` cameras of different focal lengths on a ring around the body, each with the view's pose inputs."""
    from moss_amd import scenes
    from moss_amd.gaussian_renderer import camera_view
    out = []
    for i, (R, t) in enumerate(scenes.look_at_ring(4 * n, radius=3.0)[:n]):
        c = camera_view(scenes.make_camera(512, 512, 540.0 + 25.0 * i, 540.0 + 20.0 * i, 268.0 - 3 * i, 247.0 + 2 * i, R, t), dev)
        c.big_pose_smpl_param, c.big_pose_world_vertex = cam.big_pose_smpl_param, cam.big_pose_world_vertex
        out.append(c)
    return out


def child(a):
    import torch
    from moss_step_times import _timed
    dev = torch.device("cuda:0")
    row = {"config": a.child, "P": a.P}
    if a.child == "u8":
        from moss_amd.play import frames_to_u8
        g = torch.Generator().manual_seed(1)
        cases = []
        for side in (512, 1024):
            images = [torch.rand(3, side, side, generator=g).to(dev) for _ in range(8)]
            alphas = [torch.rand(1, side, side, generator=g).to(dev) for _ in range(8)]
            bounds = [(torch.rand(side, side, generator=g) > 0.5).to(torch.uint8).to(dev) for _ in range(8)]
            for B in (1, 8):
                for C in (3, 4):
                    outs = [torch.empty(side, side, C, dtype=torch.uint8, device=dev) for _ in range(B)]
                    kw = dict(alphas=alphas[:B] if C == 4 else None, regions=bounds[:B], out=outs)
                    dt = _timed(lambda: frames_to_u8(images[:B], **kw), a.calls, dev, lambda i: None)
                    nbytes = side * side * (12 + 1 + (4 if C == 4 else 0) + C)
                    cases.append({"side": side, "frames": B, "channels": C, "us_per_launch": round(dt * 1e6, 2), "bytes_per_frame": nbytes,
                                  "gb_per_s": round(B * nbytes / dt / 1e9, 1), "share_of_hbm": round(B * nbytes / dt / 1e9 / a.hbm_gbs, 4)})
        row["cases"] = cases
        print(json.dumps(row), flush=True)
        return
    w, frames = _world_and_frames(a.P, dev)
    pc, cam, bg = w["pc"], w["cam"], w["bg"]

    def load(i):
        for key, v in frames[i % 3].items():
            cam.smpl_param[key].copy_(v)
    if a.child == "control":
        from types import SimpleNamespace
        from moss_amd.diff_gaussian_rasterization import RasterContext
        from moss_amd.gaussian_renderer import render
        cx = RasterContext()
        cx.set_async(True)
        pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raster_context=cx, **dict.fromkeys(FLAGS, True))

        def fn():
            with torch.no_grad():
                return render(cam, pc, pipe, bg)["render"]
        dt = _timed(fn, a.calls, dev, load)
        cx.check_status()
        row["us_per_call"] = round(dt * 1e6, 1)
    elif a.child in ("frame", "pose", "render", "frame_index", "pose_index"):
        from moss_amd.play import MossPlayer
        player = MossPlayer(pc, cam, bg, template_index=a.child.endswith("_index")).capture(warmup=3)
        fn = {"frame": player.frame, "pose": player.pose, "render": player.render}[a.child.split("_")[0]]
        dt = _timed(fn, a.calls, dev, load)
        player.check()
        out = player.frame()
        torch.cuda.synchronize(dev)
        assert player.dropped_frames == 0 and float(out["render"].abs().max()) > 0
        row.update(us_per_call=round(dt * 1e6, 1), captures=player.captures)
    elif a.child in ("split_grouped", "split_ungrouped"):
        import copy
        from moss_amd.play import MossPlayer, evaluate_split
        from moss_step_times import _frame
        cams = _cameras(cam, 4, dev)
        views = []
        for k in range(17):
            f = _frame(k, dev)
            for c in cams:
                v = copy.copy(c)
                v.smpl_param = f
                if a.child == "split_grouped":
                    v.pose_id = k
                views.append(v)
        n = len(views)
        gts, regions = [w["gt"]] * n, [w["region"]] * n
        player = MossPlayer(pc, cam, bg).capture(warmup=3)
        times = []
        for _ in range(4):                                   # (the first pass captures the four cameras' graphs)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            res = evaluate_split(player, views, gts, regions, lpips=w["lpips"], keep_tables=False)
            torch.cuda.synchronize(dev)
            times.append(round(1e6 * (time.perf_counter() - t0) / n, 1))
        row.update(views=n, us_per_view_first_pass=times[0], us_per_view=times[1:], poses=player.poses, captures=player.captures,
                   psnr=res["psnr"])
    else:
        raise SystemExit(f"unknown configuration {a.child}")
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="6890,45695")
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM rate the u8 kernel's share is quoted against, GB/s")
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", default=None, help="comma-separated subset of the configurations (default: all)")
    ap.add_argument("--child", default=None)
    ap.add_argument("--P", type=int, default=6890)
    a = ap.parse_args()
    if a.child:
        return child(a)
    sizes = [int(x) for x in a.sizes.split(",")]
    per_size = ("control", "frame", "pose", "render", "frame_index", "pose_index")
    configs = [(c, P) for P in sizes for c in per_size]
    configs += [("split_grouped", sizes[-1]), ("split_ungrouped", sizes[-1]), ("u8", 0)]
    if a.configs:
        configs = [(c, P) for c, P in configs if c in a.configs.split(",")]
    rows = []
    for r in range(a.rounds):
        for c, P in configs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", c, "--P", str(P), "--calls", str(a.calls), "--hbm-gbs", str(a.hbm_gbs)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"{c} at P = {P} failed with status {p.returncode}")
            row = dict(json.loads(p.stdout.strip().splitlines()[-1]), round=r)
            rows.append(row)
            print(json.dumps(row), flush=True)
    summary = []
    for P in sizes:
        control = [x["us_per_call"] for x in rows if x["config"] == "control" and x["P"] == P]
        if not control:
            continue
        line = {"P": P, "control_us": control, "control_spread": round(max(control) / min(control), 3)}
        for c in per_size[1:]:
            mine = [x["us_per_call"] for x in rows if x["config"] == c and x["P"] == P]
            if not mine:
                continue
            line[c + "_us"] = mine
            line[c + "_over_control"] = round((sum(mine) / len(mine)) / (sum(control) / len(control)), 3)
        summary.append(line)
        print(json.dumps({"summary": line}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"rows": rows, "summary": summary}, f, indent=1)


if __name__ == "__main__":
    main()
