#!/usr/bin/env python3
"""Times MOSS's whole training iteration -- all six loss terms, all eight parameter groups -- at P = 6 890 and 45 695 Gaussians, 512 x 512,
SH degree 3, synthetic LPIPS weights, a 192 x 256 region:

    captured   ``moss_amd.train.MossStep`` replayed from its hipGraph (three FlatAdamW, the Gaussians' inside the backward kernel, both
               networks in one launch)
    baseline   the same composition -- ``render()`` with the same ``*_in_op`` flags, the same four fused loss calls -- run eagerly with
               ``moss_amd.optim.AdamW`` over MOSS's eight parameter groups (its two network groups take torch's ``_foreach`` launches).
               It uses nothing newer than the drop-in optimizer, so it also runs on a checkout from before ``MossStep`` existed:
               ``--only baseline --package-root <that checkout>``
    profile    ``rocprofv3 --kernel-trace --stats`` over the captured step at the larger size; the per-kernel table is printed

    python scripts/moss_step_times.py [--replays 300] [--sizes 6890,45695] [--only captured,baseline,profile] [--out DIR]
                                      [--lpips-precision f32|bf16|bf16x3]
    python scripts/moss_step_times.py --lpips-reference [--replays 300]
    python scripts/moss_step_times.py --template-index [--replays 300] [--only profile]
    python scripts/moss_step_times.py --lbs-weights-precision bf16x3 [--template-index] [--lpips-precision bf16] [--replays 300]

``--lpips-reference``: the captured step at P = 45 695 over its three frames WITH ``MossStep(lpips_reference=)`` -- one
``lpips.LpipsReference`` per frame built before the clock starts, ``step.lpips_reference.copy_(refs[k])`` per replay INSIDE the timed
window beside the five input copies -- and without, LPIPS precisions f32 and bf16, the four runs alternated and the whole sequence
twice (eight processes); the table gives each pair's ratio and the spread of the control between the two repetitions.

``--template-index``: the captured step at P = 45 695 WITH ``MossStep(template_index=True)`` -- the nearest-vertex query through a
``knn_cuda.TemplateIndex`` built once -- and without, in the same eight-process scheme; with ``--only profile`` instead ONE
``rocprofv3 --kernel-trace --stats`` run of the step with the index.

``--lbs-weights-precision bf16x3``: the captured step at P = 45 695 WITH ``MossStep(lbs_weights_precision="bf16x3")`` -- the LBS-weight
network's split-bf16 mode -- and without (the control), at the given ``--lpips-precision`` and, with ``--template-index``, with the
index in both; the two runs alternated and the sequence twice (four processes); the table gives the ratio, the control's spread and
the last step's total loss of both.

Every measurement is a process of its own under ``timeout -k 10``; the script stops at the first one that does not exit with 0.  A time
is the wall clock around ``replays`` back-to-back steps between two device synchronisations, after a warm-up.  Needs a GPU.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
STEP_TIMEOUT = 240
FLAGS = ("lbs_in_op", "pose_head_in_op", "lbs_weights_in_op", "smpl_frame_in_op", "transforms_in_op", "pose_in_op", "raw_parameters_in_op")
LR_HEAD, LR_NET = 2.5e-4, 1e-4
V = 6890


def _frame(k, dev):
    """A frame that keeps the body in view: small joint rotations, a small global rotation and translation, and target rotations
    near the frame's own."""
    import torch
    from moss_amd import lbs as mlbs
    g = torch.Generator().manual_seed(500 + k)
    axis = torch.randn(1, 3, generator=g)
    f = {"poses": 0.15 * torch.randn(1, 72, generator=g), "shapes": 0.3 * torch.randn(1, 10, generator=g),
         "R": mlbs.batch_rodrigues(0.3 * axis / axis.norm())[0], "Th": 0.05 * torch.randn(1, 3, generator=g)}
    f["pose_rotmats"] = mlbs.batch_rodrigues(f["poses"].reshape(24, 3)[1:] + 0.05 * torch.randn(23, 3, generator=g))
    return {k_: v.to(dev) for k_, v in f.items()}


def _world(P, dev, unified, lpips_precision="f32"):
    """Model, camera and targets: MOSS's initialisation at 6 890 Gaussians, post-densification statistics above."""
    import torch
    from moss_amd import lbs as mlbs
    from moss_amd import lbs_weights as mlw
    from moss_amd import lpips as mlp
    from moss_amd import pose as mpose
    from moss_amd import scenes
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import camera_view
    from moss_amd.knn_cuda import KNN
    from moss_amd.loss import ViewRegion

    class DeformableSet(GaussianSet):
        def coarse_deform_c2source(self, *a, **k):           # (render() only asks whether the model has one: lbs_in_op runs the fused op)
            raise NotImplementedError

    torch.manual_seed(1)
    s = scenes.body_scene(P, 512, 512, 540.0, init_like=P <= 6890, name="moss_step")
    pc = DeformableSet(s, sh_degree=3, device=dev, unified_features=unified)
    body = mlbs.synthetic_body_model(V, 24, seed=21, device=dev)
    pc.SMPL_NEUTRAL, pc.knn = body, KNN(k=1, transpose_mode=True)
    pc.auto_regression = mpose.head_module().to(dev)
    pc.cross_attention_lbs = mlw.lbs_weight_module().to(dev)
    pc.motion_offset_flag = True
    cam = camera_view(s.camera, dev)
    cam.big_pose_smpl_param = {k: v.to(dev) for k, v in mlbs.synthetic_frame(0, 24, big_pose=True).items()}
    cam.big_pose_world_vertex = body["v_template"].clone()
    cam.smpl_param = _frame(0, dev)
    H, W = s.camera.H, s.camera.W
    g = torch.Generator().manual_seed(77)
    bound = torch.zeros(1, H, W)
    bound[:, 128:384, 160:352] = 1
    lp = mlp.cast_params(mlp.synthetic_weights(), device=dev)
    net = mlp.LpipsVGG.from_tensors(lp["conv_weights"], lp["conv_biases"], lp["lin_weights"], lp["shift"], lp["scale"],
                                    precision=lpips_precision)
    return dict(pc=pc, cam=cam, gt=torch.rand(3, H, W, generator=g).to(dev), bkgd=(torch.rand(1, H, W, generator=g) > 0.5).float().to(dev),
                region=ViewRegion(bound.to(dev)), bg=torch.zeros(3, device=dev), lpips=net)


def _timed(fn, replays, dev, load):
    import torch
    for i in range(20):
        load(i)
        fn()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(replays):
        load(i)
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / replays


def measure_captured(P, replays, lpips_precision="f32", lpips_reference=False, template_index=False, lbs_weights_precision="f32"):
    import torch
    from moss_amd.train import MossStep
    dev = torch.device("cuda:0")
    w = _world(P, dev, unified=True, lpips_precision=lpips_precision)
    kw, refs = {}, None
    if lpips_reference:                                      # one reference per frame (here of one ground truth: what is timed is the copy)
        from moss_amd import lpips as mlp
        refs, nbytes = mlp.reference_cache(w["lpips"], [w["gt"]] * 3, [w["region"]] * 3)
        kw["lpips_reference"] = mlp.LpipsReference.empty(w["lpips"], refs[0].crop, static=True).copy_(refs[0])
    if template_index:
        kw["template_index"] = True
    if lbs_weights_precision != "f32":                       # (left out for the control: a checkout without the argument serves)
        kw["lbs_weights_precision"] = lbs_weights_precision
    step = MossStep(w["pc"], w["cam"], w["gt"], w["bkgd"], w["region"], w["bg"], w["lpips"], {"auto_regression": LR_HEAD, "cross_attention_lbs": LR_NET},
                    **kw)
    step.capture(warmup=3)
    frames = [_frame(k, dev) for k in range(3)]

    def load(i):                                             # a new frame per replay: five small copies into the static inputs
        for key, v in frames[i % 3].items():
            w["cam"].smpl_param[key].copy_(v)
        if refs is not None:                                 # ... and the frame's reference: 122 floats per crop pixel
            step.lpips_reference.copy_(refs[i % 3])

    dt = _timed(step, replays, dev, load)
    step.check()
    out = step()
    torch.cuda.synchronize(dev)
    assert step.dropped_frames == 0 and float(out["render"].abs().max()) > 0 and bool(torch.isfinite(out["terms"]).all())
    return {"form": "captured", "P": P, "lpips_precision": lpips_precision, "lpips_reference": bool(lpips_reference),
            "template_index": bool(template_index), "lbs_weights_precision": lbs_weights_precision, "reference_bytes_per_camera": refs[0].nbytes if refs else 0, "replays": replays, "us_per_step": round(dt * 1e6, 1), "it_per_s": round(1.0 / dt, 1),
            "steps": list(step.step_counts()), "total_loss": float(out["terms"][-1])}


def measure_baseline(P, replays, lpips_precision="f32"):
    import torch
    from types import SimpleNamespace
    from moss_amd import lbs_weights as mlw
    from moss_amd import pose as mpose
    from moss_amd.diff_gaussian_rasterization import RasterContext
    from moss_amd.gaussian_renderer import render
    from moss_amd.loss import s3im_loss_roi_fused, training_loss_moss_fused
    from moss_amd.lpips import lpips_vgg_roi_fused
    from moss_amd.optim import AdamW
    dev = torch.device("cuda:0")
    w = _world(P, dev, unified=False, lpips_precision=lpips_precision)
    pc, cam = w["pc"], w["cam"]
    cx = RasterContext()
    cx.set_async(True)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raster_context=cx, **dict.fromkeys(FLAGS, True))
    # MOSS's eight groups (scene/gaussian_model.py:215-226); the networks' with every tensor of the module, as MOSS passes them
    groups = pc.param_groups() + [{"params": list(pc.auto_regression.parameters()), "lr": LR_HEAD, "name": "auto_regression"},
                                  {"params": list(pc.cross_attention_lbs.parameters()), "lr": LR_NET, "name": "cross_attention_lbs"}]
    assert len(groups) == 8
    opt = AdamW(groups, lr=0.0, eps=1e-15)
    frames = [_frame(k, dev) for k in range(3)]
    last = {}

    def load(i):
        for key, v in frames[i % 3].items():
            cam.smpl_param[key].copy_(v)

    def fn():
        opt.zero_grad(set_to_none=True)
        out = render(cam, pc, pipe, w["bg"])
        image = out["render"]
        loss = (training_loss_moss_fused(image, out["render_alpha"], w["gt"], w["bkgd"], w["region"], 0.2, 0.5)
                + 0.5 * lpips_vgg_roi_fused(w["lpips"], image, w["gt"], w["region"]).reshape(())
                + 0.06 * out["pose_out"]["nll"].mean() + 0.3 * s3im_loss_roi_fused(image, w["gt"], w["region"]))
        loss.backward()
        opt.step()
        last["loss"], last["image"] = loss.detach(), image.detach()

    dt = _timed(fn, replays, dev, load)
    cx.check_status()
    assert float(last["image"].abs().max()) > 0 and bool(torch.isfinite(last["loss"]))
    assert all(p.grad is not None for p in mpose.head_parameters(pc.auto_regression) + mlw.net_parameters(pc.cross_attention_lbs))
    return {"form": "baseline_eager_dropin_adamw", "P": P, "lpips_precision": lpips_precision, "replays": replays, "us_per_step": round(dt * 1e6, 1), "it_per_s": round(1.0 / dt, 1),
            "total_loss": float(last["loss"])}


def kernel_table(directory, top=25):
    """The per-kernel rows of rocprofv3's ``*kernel_stats.csv`` under ``directory``: (name, calls, total us, mean us, percent)."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                rows.append((r["Name"], int(r["Calls"]), float(r["TotalDurationNs"]) / 1e3, float(r["AverageNs"]) / 1e3, float(r["Percentage"])))
    rows.sort(key=lambda r: -r[2])
    return rows[:top]


def ab_comparison(a, key, worker_flag, names, P=45695):
    """The captured step with and without the option ``key`` of ``measure_captured`` (``worker_flag`` switches it on in the worker),
    LPIPS precisions f32 and bf16, each run a process of its own, the sequence twice.  ``names``: (without, with) for the table."""
    os.makedirs(a.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--package-root", os.path.abspath(a.package_root), "--replays", str(a.replays)]
    results = []
    for rep in (1, 2):
        for prec in ("f32", "bf16"):
            for on in (False, True):
                name = f"captured_{P}_{prec}_{names[on].replace('-', '_').replace(' ', '_')}_{rep}"
                cmd = (["timeout", "-k", "10", str(STEP_TIMEOUT)] + me + ["--lpips-precision", prec, "--worker", "captured", "--P", str(P)]
                       + ([worker_flag] if on else []))
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=os.path.abspath(a.package_root))
                with open(os.path.join(a.out, name + ".log"), "w") as f:
                    f.write(r.stdout)
                line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
                if r.returncode != 0 or line is None:
                    print(f"{name}: exit {r.returncode}; stopping (log: {os.path.join(a.out, name + '.log')})\n" + r.stdout[-3000:], flush=True)
                    raise SystemExit(1)
                res = dict(json.loads(line[7:]), job=name, repetition=rep)
                results.append(res)
                print(json.dumps(res), flush=True)
    nbytes = max(r["reference_bytes_per_camera"] for r in results)
    print(f"| LPIPS precision | {names[0]} us (1, 2) | spread | {names[1]} us (1, 2) | spread | {names[1]} / {names[0]} (1, 2) |"
          + (" bytes per camera |" if nbytes else "") + "\n|---|---|---|---|---|---|" + ("---|" if nbytes else ""))
    for prec in ("f32", "bf16"):
        t = {on: [r["us_per_step"] for r in results if r["lpips_precision"] == prec and r[key] == on] for on in (False, True)}
        spread = {on: abs(t[on][0] - t[on][1]) / (0.5 * sum(t[on])) for on in (False, True)}
        print(f"| {prec} | {t[False][0]:.1f}, {t[False][1]:.1f} | {100 * spread[False]:.2f} % | {t[True][0]:.1f}, {t[True][1]:.1f} | "
              f"{100 * spread[True]:.2f} % | {t[True][0] / t[False][0]:.4f}, {t[True][1] / t[False][1]:.4f} |" + (f" {nbytes} |" if nbytes else ""))
    with open(os.path.join(a.out, key + "_results.json"), "w") as f:
        json.dump(results, f, indent=1)


def lbs_weights_comparison(a, P=45695):
    """The captured step with MossStep(lbs_weights_precision=a.lbs_weights_precision) and without (f32, the control), at
    a.lpips_precision, with the template index in both if a.template_index; each run a process of its own, the sequence twice."""
    os.makedirs(a.out, exist_ok=True)
    me = ([sys.executable, os.path.abspath(__file__), "--package-root", os.path.abspath(a.package_root), "--replays", str(a.replays),
           "--lpips-precision", a.lpips_precision, "--worker", "captured", "--P", str(P)] + (["--with-template-index"] if a.template_index else []))
    modes = ("f32", a.lbs_weights_precision)
    results = []
    for rep in (1, 2):
        for mode in modes:
            name = f"captured_{P}_lbs_weights_{mode}_{rep}"
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT)] + me + ["--lbs-weights-precision", mode]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=os.path.abspath(a.package_root))
            with open(os.path.join(a.out, name + ".log"), "w") as f:
                f.write(r.stdout)
            line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
            if r.returncode != 0 or line is None:
                print(f"{name}: exit {r.returncode}; stopping (log: {os.path.join(a.out, name + '.log')})\n" + r.stdout[-3000:], flush=True)
                raise SystemExit(1)
            res = dict(json.loads(line[7:]), job=name, repetition=rep)
            results.append(res)
            print(json.dumps(res), flush=True)
    t = {m: [r["us_per_step"] for r in results if r["lbs_weights_precision"] == m] for m in modes}
    loss = {m: [r["total_loss"] for r in results if r["lbs_weights_precision"] == m] for m in modes}
    spread = {m: abs(t[m][0] - t[m][1]) / (0.5 * sum(t[m])) for m in modes}
    print(f"| LBS-weight network | us per step (1, 2) | spread | / f32 (1, 2) | total loss of the last step |\n|---|---|---|---|---|")
    for m in modes:
        print(f"| {m} | {t[m][0]:.1f}, {t[m][1]:.1f} | {100 * spread[m]:.2f} % | {t[m][0] / t['f32'][0]:.4f}, {t[m][1] / t['f32'][1]:.4f} | "
              f"{loss[m][0]:.6f} |")
    with open(os.path.join(a.out, "lbs_weights_precision_results.json"), "w") as f:
        json.dump(results, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=300)
    ap.add_argument("--sizes", default="6890,45695")
    ap.add_argument("--only", default="captured,baseline,profile")
    ap.add_argument("--out", default="moss_step_times_out")
    ap.add_argument("--lpips-precision", default="f32", choices=("f32", "bf16", "bf16x3"), help="the LPIPS net's operand precision (LpipsVGG(precision=))")
    ap.add_argument("--lbs-weights-precision", default="f32", choices=("f32", "bf16x3"),
                    help="bf16x3: the captured step at P = 45 695 with and without MossStep(lbs_weights_precision=\"bf16x3\"), alternated twice")
    ap.add_argument("--lpips-reference", action="store_true",
                    help="the captured step at P = 45 695 with and without MossStep(lpips_reference=), f32 and bf16, alternated twice")
    ap.add_argument("--with-reference", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--template-index", action="store_true",
                    help="the captured step at P = 45 695 with and without MossStep(template_index=True), f32 and bf16, alternated twice; "
                         "with --only profile: one rocprofv3 run of the step with the index")
    ap.add_argument("--with-template-index", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--package-root", default=os.path.dirname(HERE), help="the checkout whose moss_amd is measured")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--P", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    if a.worker:
        if a.replays < 200:
            raise SystemExit("at least 200 replays per measurement")
        extra = (a.with_reference, a.with_template_index, a.lbs_weights_precision) if a.worker == "captured" else ()
        print("RESULT " + json.dumps({"captured": measure_captured, "baseline": measure_baseline}[a.worker](a.P, a.replays, a.lpips_precision, *extra)), flush=True)
        return
    if a.lbs_weights_precision != "f32":
        return lbs_weights_comparison(a)
    if a.lpips_reference:
        return ab_comparison(a, "lpips_reference", "--with-reference", ("two-image", "reference"))
    if a.template_index and a.only != "profile":
        return ab_comparison(a, "template_index", "--with-template-index", ("grid", "template index"))
    os.makedirs(a.out, exist_ok=True)
    sizes = [int(x) for x in a.sizes.split(",")]
    only = a.only.split(",")
    me = [sys.executable, os.path.abspath(__file__), "--package-root", os.path.abspath(a.package_root), "--replays", str(a.replays),
          "--lpips-precision", a.lpips_precision]
    jobs = [(f"{form}_{P}", ["timeout", "-k", "10", str(STEP_TIMEOUT)] + me + ["--worker", form, "--P", str(P)])
            for form in ("captured", "baseline") if form in only for P in sizes]
    if "profile" in only:
        prof = os.path.join(os.path.abspath(a.out), "rocprof")
        jobs.append(("profile", ["timeout", "-k", "10", str(STEP_TIMEOUT), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv",
                                 "-d", prof, "-o", "moss_step", "--"] + me + ["--worker", "captured", "--P", str(max(sizes))]
                     + (["--with-template-index"] if a.template_index else [])))
    results = []
    for name, cmd in jobs:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=os.path.abspath(a.package_root))
        with open(os.path.join(a.out, name + ".log"), "w") as f:
            f.write(r.stdout)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            print(f"{name}: exit {r.returncode}; stopping (log: {os.path.join(a.out, name + '.log')})\n" + r.stdout[-3000:], flush=True)
            raise SystemExit(1)
        res = dict(json.loads(line[7:]), job=name)
        results.append(res)
        print(json.dumps(res), flush=True)
        if name == "profile":
            # (one process: capture warm-up, 20 + replays + 1 replayed steps; the eager warm-up steps' kernels are in the totals too)
            n = a.replays + 21
            print(f"| kernel | calls | total us | mean us | % | us / replayed step (calls / {n}) |\n|---|---|---|---|---|---|")
            for nm, calls, tot, mean, pct in kernel_table(prof):
                print(f"| `{nm[:90]}` | {calls} | {tot:.0f} | {mean:.1f} | {pct:.1f} | {tot / n:.1f} |")
    with open(os.path.join(a.out, "results.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
