#!/usr/bin/env python3
"""Generates tests/golden/densify_decision.npz by EXECUTING the reference's own ``GaussianModel.densify_and_prune``
(scene/gaussian_model.py:621-666) and the three phase functions it calls (``kl_densify_and_clone`` :495-526, ``kl_densify_and_split``
:528-571, ``kl_merge`` :573-619) from a MOSS checkout, on the CPU, in float32.

    python tests/golden/make_golden_densify.py <path of a MOSS checkout>

scene/gaussian_model.py is loaded as tests/golden/make_golden_lbs.py loads it (third-party modules stubbed).  The functions run on a
``GaussianModel`` made without its constructor that carries MOSS's six parameters in a ``torch.optim.AdamW(lr=0, eps=1e-15)`` with
the group names of ``training_setup`` (:215-226) and, after one step on zero learning rate, both moments of every parameter -- so that
``cat_tensors_to_optimizer`` and ``_prune_optimizer`` run as written.  Stand-ins, and what they are:

  "cuda" device arguments   mapped to the CPU by a TorchFunctionMode while the reference runs (``device="cuda"``, ``.cuda()``, ``.to('cuda')``)
  compute_normals_co3d /    replaced by a seeded mask: the surface-change test (open3d, :503-507) is an INPUT of the fused ops
  compute_angle_change_rate
  torch.normal(mean, std)   ``mean + std * eps`` with the recorded eps (rows of ``noise[phase]``, regenerated from the seed)
  knn / knn_near_2          exhaustive float64 searches over the float32 positions returning what moss_amd.knn_cuda returns:
                            Euclidean distances (1,Nq,k) float32, indices (1,Nq,k) int64
  matrix_to_quaternion      moss_amd.densify.matrix_to_quaternion_torch in float64: pytorch3d's convention, real part first, the
                            candidate of the largest component.  joint_F is a sum of rotations within 0.4 rad of the identity, so the
                            real part IS the largest and every pytorch3d release agrees, sign included.

Cases: P = 600 Gaussians, V = 256 vertices, 24 joints; ``screen_none`` (max_screen_size None) and ``screen_20`` (20); every phase
selects at least 16 and at most half of the rows (asserted).  ``guard``: 45 696 rows of trivial data, so that all three phases
return early (:496,530,574) and only the final prune acts -- with the max_radii2D the statistics hold; stored: the final row count and
the prune mask.

Margins.  The whole decision is repeated in FLOAT64 with moss_amd.densify's ``*_torch`` functions and it is asserted that no decision
quantity lies within a relative 1e-3 of its threshold: gradient vs max_grad, max scale vs percent_dense * extent and 0.1 * extent, KL
vs 0.4 and 0.1, sigmoid(opacity) vs min_opacity, vertex distance vs 0.05; and that no Gaussian's second and third nearest
neighbours (the first is itself) tie within a relative 1e-3.  The input generator moves gradients, scales and opacities that fall
into a margin away from it, and positions whose neighbours tie or whose vertex distance does; what depends on rows created on the
way (KL, distances, ties of new rows) is asserted, and a case whose seed fails
gets another seed.  With these margins the masks and index lists of the fixture are exact expectations.

Stored per case and phase: mask, index list, the six new tensors, the prune filter; the final parameter tensors; the seed and a
SHA-256 of the inputs (no inputs are stored).
"""
import hashlib
import importlib.machinery
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from torch.overrides import TorchFunctionMode

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from moss_amd import densify as D  # noqa: E402

P, V, J = 600, 256, 24
GUARD_P = 45696
CASES = {"screen_none": 134, "screen_20": 320}
SCREEN = {"screen_none": None, "screen_20": 20}
GUARD_SEED = 41
MAX_GRAD, MIN_OPACITY, EXTENT, PERCENT_DENSE, KL_THRESHOLD = 0.0002, 0.1, 1.0, 0.01, 0.4
MARGIN = 1e-3
PHASES = ("clone", "split", "merge")
ROW_NAMES = ("new_xyz", "new_features_dc", "new_features_rest", "new_opacities", "new_scaling", "new_rotation")
PARAMS = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")
INPUTS = PARAMS + ("accum", "denom", "max_radii2D", "joint_F", "lbs_weights", "t_vertices", "surface_mask", "noise_clone", "noise_split")


def _rodrigues(rng, n, angle):
    ax = rng.normal(size=(n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    th = rng.uniform(0.05, angle, size=(n, 1, 1))
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def _away(x, limit, step):
    """Move the entries of ``x`` within 2 MARGIN (relative) of ``limit`` to ``limit * (1 + step)``."""
    near = np.abs(x - limit) < 2 * MARGIN * limit
    return np.where(near, limit * (1 + step), x)


def golden_inputs(case, dtype=torch.float32, n=P):
    """The inputs of one case, regenerated from its seed (float32 values, handed out in ``dtype``): a dict of tensors named INPUTS."""
    rng = np.random.Generator(np.random.PCG64(CASES.get(case, GUARD_SEED)))
    f32 = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))        # noqa: E731
    tv = rng.uniform(-0.5, 0.5, size=(V, 3))
    xyz = tv[rng.integers(0, V, size=n)] + 0.015 * rng.normal(size=(n, 3))
    far = rng.random(n) < 0.06
    xyz[far] += 0.08 * np.sign(rng.normal(size=(int(far.sum()), 3)))
    scale = np.exp(np.log(PERCENT_DENSE * EXTENT) - 0.55 + 0.7 * rng.normal(size=(n, 3)))   # (the MAX of three straddles the limit)
    rot = rng.normal(size=(n, 4))
    # near-duplicates of an earlier Gaussian: the pairs kl_merge is after (KL < 0.1)
    twin = np.nonzero(rng.random(n) < 0.4)[0]
    twin = twin[twin > 0]
    src = (twin * rng.random(twin.shape[0])).astype(np.int64)
    scale[twin] = scale[src] * np.exp(0.05 * rng.normal(size=(twin.shape[0], 3)))
    rot[twin] = rot[src] + 0.02 * rng.normal(size=(twin.shape[0], 4))
    xyz[twin] = xyz[src] + 0.1 * scale[src] * rng.normal(size=(twin.shape[0], 3))
    for lim in (PERCENT_DENSE * EXTENT, 0.1 * EXTENT):
        scale = _away(scale, lim, 0.01)
    for _ in range(12):                                                   # neighbour ties and nearest-vertex distances out of their margins
        x32, v32 = xyz.astype(np.float32).astype(np.float64), tv.astype(np.float32).astype(np.float64)
        if n <= D.MAX_POINTS:                                             # (above it no phase runs and no neighbour is queried)
            dn = np.sort(((x32[:, None] - x32[None]) ** 2).sum(-1), axis=1)[:, 1:3] ** 0.5
            tie = (dn[:, 1] - dn[:, 0]) < 4 * MARGIN * dn[:, 1]
            xyz[tie] += 0.002 * rng.normal(size=(int(tie.sum()), 3))
            x32 = xyz.astype(np.float32).astype(np.float64)
        d2 = np.concatenate([((x32[a:a + 4096, None] - v32[None]) ** 2).sum(-1) for a in range(0, n, 4096)])
        near_v, dist = d2.argmin(1), np.sqrt(d2.min(1))
        bad = np.abs(dist - 0.05) < 4 * MARGIN * 0.05
        xyz[bad] += 0.01 * (x32[bad] - v32[near_v[bad]]) / dist[bad, None]
    opacity = 2.0 * rng.normal(size=(n, 1))
    sig = 1 / (1 + np.exp(-opacity))
    opacity = np.where(np.abs(sig - MIN_OPACITY) < 2 * MARGIN * MIN_OPACITY, opacity + 0.05, opacity)
    denom = rng.integers(0, 9, size=(n, 1)).astype(np.float64)
    denom[0] = 4.0
    grad = _away(rng.uniform(0, 2 * MAX_GRAD, size=(n, 1)), MAX_GRAD, 0.02)
    accum = (grad * denom).astype(np.float32)                             # (rows with denom 0: 0 / 0 = NaN -> 0, :642)
    g32 = accum / np.maximum(denom, 1).astype(np.float32)
    accum = np.where((np.abs(g32 - MAX_GRAD) < 2 * MARGIN * MAX_GRAD) & (denom > 0), accum * np.float32(1.02), accum)
    joint_F = np.stack([_rodrigues(rng, int(denom[0, 0]), 0.4).sum(0) for _ in range(J - 1)])
    logits = 2.0 * rng.normal(size=(n, J))
    w = np.exp(logits - logits.max(1, keepdims=True))
    lbs = denom[0, 0] * w / w.sum(1, keepdims=True)
    g = {"xyz": f32(xyz), "features_dc": f32(rng.normal(size=(n, 1, 3))), "features_rest": f32(0.1 * rng.normal(size=(n, 15, 3))),
         "opacity": f32(opacity), "scaling": f32(np.log(scale)), "rotation": f32(rot), "accum": f32(accum), "denom": f32(denom),
         "max_radii2D": f32(_away(rng.uniform(0, 40, size=(n,)), 20.0, 0.01)), "joint_F": f32(joint_F), "lbs_weights": f32(lbs)[None], "t_vertices": f32(tv),
         "surface_mask": torch.tensor(rng.random(n) < 0.85), "noise_clone": f32(rng.normal(size=(n, 3))),
         "noise_split": f32(rng.normal(size=(4 * n, 3)))}
    return {k: (v if v.dtype == torch.bool else v.to(dtype)) for k, v in g.items()}


def inputs_checksum(case, n=P):
    """SHA-256 over the float32 bytes of every input of ``case`` in the order of INPUTS."""
    g = golden_inputs(case, n=n)
    h = hashlib.sha256()
    for k in INPUTS:
        h.update(np.ascontiguousarray(g[k].numpy()).tobytes())
    return h.hexdigest()


def cpu_knn(ref, query, k):
    """What moss_amd.knn_cuda.knn returns, exhaustively: ref (1,Nr,3), query (1,Nq,3) -> Euclidean dist (1,Nq,k) float32, idx (1,Nq,k)."""
    r, q = ref[0].detach().double(), query[0].detach().double()
    dist = torch.empty((q.shape[0], k), dtype=torch.float64)
    idx = torch.empty((q.shape[0], k), dtype=torch.int64)
    for a in range(0, q.shape[0], 2048):                                  # (blocks: the guard case has 45 696 queries)
        d2 = ((q[a:a + 2048, None, :] - r[None, :, :]) ** 2).sum(-1)
        dd, ii = torch.topk(d2, k, dim=1, largest=False, sorted=True)
        dist[a:a + 2048], idx[a:a + 2048] = dd.sqrt(), ii
    return dist[None].to(ref.dtype), idx[None]


def neighbour_tie_margin(xyz):
    """The smallest relative gap between a Gaussian's second and third nearest neighbour (the first is itself), float64."""
    d, i = cpu_knn(xyz[None].double(), xyz[None].double(), 3)
    assert bool((i[0, :, 0] == torch.arange(xyz.shape[0])).all()), "a Gaussian is not its own nearest neighbour (duplicate positions)"
    return float(((d[0, :, 2] - d[0, :, 1]) / d[0, :, 2]).min())


def _load_reference(root):
    for name in ("open3d", "plyfile", "pytorch3d", "pytorch3d.transforms", "knn_cuda", "simple_knn", "simple_knn._C", "cv2",
                 "sklearn", "sklearn.neighbors"):
        sys.modules[name] = types.ModuleType(name)
        sys.modules[name].__spec__ = importlib.machinery.ModuleSpec(name, None)     # (torch's optimizers look the loaded modules up)
    sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = object
    sys.modules["pytorch3d.transforms"].matrix_to_quaternion = None
    sys.modules["knn_cuda"].KNN = object
    sys.modules["simple_knn._C"].distCUDA2 = None
    sys.modules["sklearn.neighbors"].KDTree = object
    sys.path.insert(0, root)
    spec = importlib.util.spec_from_file_location("moss_reference_gaussian_model", os.path.join(root, "scene", "gaussian_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Recorder(TorchFunctionMode):
    """Maps "cuda" to the CPU, answers torch.normal from the recorded noise and remembers the last boolean row mask used as an index."""

    def __init__(self, noise):
        super().__init__()
        self.noise, self.phase, self.last_mask, self.in_prune = noise, None, None, False

    def __torch_function__(self, func, types_, args=(), kwargs=None):
        kwargs = dict(kwargs or {})
        if isinstance(kwargs.get("device"), str) and kwargs["device"].startswith("cuda"):
            kwargs["device"] = "cpu"
        name = getattr(func, "__name__", "")
        if name == "cuda":
            return args[0]
        if name == "to":
            args = tuple("cpu" if isinstance(a, str) and a.startswith("cuda") else a for a in args)
        if func is torch.normal:
            std = kwargs["std"]
            return kwargs["mean"] + std * self.noise[self.phase][:std.shape[0]].to(std.dtype)
        if name == "__getitem__" and not self.in_prune and torch.is_tensor(args[1]) and args[1].dtype == torch.bool and args[1].dim() == 1:
            self.last_mask = args[1].clone()
        return func(*args, **kwargs)


def run_reference(mod, case, n=P, max_screen_size=None):
    """Runs the reference's densify_and_prune on the inputs of ``case``: {phase: {mask, index, rows..., prune_filter}}, final tensors."""
    g = golden_inputs(case, n=n)
    GM = mod.GaussianModel
    gm = GM.__new__(GM)
    gm.setup_functions()
    names = {"xyz": "_xyz", "features_dc": "_features_dc", "features_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
             "rotation": "_rotation"}
    for k, a in names.items():
        setattr(gm, a, torch.nn.Parameter(g[k].clone().requires_grad_(True)))
    gm.percent_dense = PERCENT_DENSE
    gm.xyz_gradient_accum, gm.denom, gm.max_radii2D = g["accum"].clone(), g["denom"].clone(), g["max_radii2D"].clone()
    groups = [{"params": [getattr(gm, a)], "lr": 0.0, "name": nm} for nm, a in
              (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"), ("scaling", "_scaling"),
               ("rotation", "_rotation"))]
    gm.optimizer = torch.optim.AdamW(groups, lr=0.0, eps=1e-15)          # (:226)
    for grp in groups:
        grp["params"][0].grad = torch.ones_like(grp["params"][0])
    gm.optimizer.step()                                                   # lr = 0: parameters unchanged, both moments now exist
    gm.knn = lambda ref, query: cpu_knn(ref, query, 1)
    gm.knn_near_2 = lambda ref, query: cpu_knn(ref, query, 2)
    gm.compute_normals_co3d = lambda *a, **k: None
    gm.compute_angle_change_rate = lambda *a, **k: g["surface_mask"].clone()
    mod.matrix_to_quaternion = lambda m: D.matrix_to_quaternion_torch(m.double()).to(m.dtype)
    rec = _Recorder({"clone": g["noise_clone"], "split": g["noise_split"]})
    phases = {}

    def phase_of(name, fn):
        def run(*a, **k):
            rec.phase = name
            fn(gm, *a, **k)
            rec.phase = None
        return run
    gm.kl_densify_and_clone = phase_of("clone", GM.kl_densify_and_clone)
    gm.kl_densify_and_split = phase_of("split", GM.kl_densify_and_split)
    gm.kl_merge = phase_of("merge", GM.kl_merge)

    def postfix(*rows):
        mask = rec.last_mask
        phases[rec.phase] = {"mask": mask.numpy().copy(), "index": torch.nonzero(mask).reshape(-1).numpy().astype(np.int32)}
        phases[rec.phase].update({k: r.detach().numpy().copy() for k, r in zip(ROW_NAMES, rows)})
        GM.densification_postfix(gm, *rows)

    def prune(mask):
        rec.in_prune = True
        phases.setdefault(rec.phase or "final", {})["prune_filter"] = mask.numpy().copy()
        GM.prune_points(gm, mask)
        rec.in_prune = False
    gm.densification_postfix, gm.prune_points = postfix, prune
    with torch.no_grad(), rec:
        GM.densify_and_prune(gm, MAX_GRAD, g["joint_F"], g["lbs_weights"], MIN_OPACITY, EXTENT, max_screen_size, KL_THRESHOLD,
                             t_vertices=g["t_vertices"])
    final = {k: getattr(gm, a).detach().numpy().copy() for k, a in names.items()}
    return phases, final


def float64_decision(case, n=P, max_screen_size=None):
    """The same decision with moss_amd.densify's ``*_torch`` functions in float64: the smallest relative margin of every decision
    quantity to its threshold, the neighbour tie margins, and the phases' index lists."""
    g = golden_inputs(case, torch.float64, n=n)
    cur = {k: g[k].clone() for k in PARAMS}
    accum, denom = g["accum"].reshape(-1), g["denom"].reshape(-1)
    table = D.joint_tables_torch(g["joint_F"], denom)
    margins, index = {}, {}

    def rel(name, x, limit):
        x = x[torch.isfinite(x)]
        margins[name] = min(margins.get(name, 1.0), float((x - limit).abs().min() / limit)) if x.numel() else margins.get(name, 1.0)

    def decision_margins(phase, kl_limit):
        grad = D._padded_grad(accum, denom, cur["xyz"].shape[0])
        rel("grad", grad, MAX_GRAD)
        rel("scale", torch.exp(cur["scaling"]).max(1).values, PERCENT_DENSE * EXTENT)
        ids = cpu_knn(cur["xyz"][None], cur["xyz"][None], 2)[1][0]
        rel(f"kl_{phase}", D.kl_div_torch(cur["xyz"], cur["rotation"], torch.exp(cur["scaling"]), ids), kl_limit)
        margins["tie"] = min(margins.get("tie", 1.0), neighbour_tie_margin(cur["xyz"]))
        return ids

    def append(rows):
        for k, r in zip(PARAMS, ROW_NAMES):
            cur[k] = torch.cat((cur[k], rows[r]), 0)

    def prune(mask):
        for k in PARAMS:
            cur[k] = cur[k][~mask]
    args = (cur["xyz"].shape[0] <= D.MAX_POINTS)
    radii = g["max_radii2D"]
    if args:
        ids = decision_margins("clone", KL_THRESHOLD)
        _, idx, _ = D.select_clone_torch(cur["xyz"], cur["rotation"], cur["scaling"], ids, accum, denom, MAX_GRAD, EXTENT, PERCENT_DENSE,
                                         KL_THRESHOLD, g["surface_mask"])
        index["clone"] = idx
        append(D.clone_rows_torch(idx, g["noise_clone"][:idx.numel()], *[cur[k] for k in PARAMS], g["lbs_weights"], denom, table))
        ids = decision_margins("split", KL_THRESHOLD)
        m, idx, _ = D.select_split_torch(cur["xyz"], cur["rotation"], cur["scaling"], ids, accum, denom, MAX_GRAD, EXTENT, PERCENT_DENSE, KL_THRESHOLD)
        index["split"] = idx
        append(D.split_rows_torch(idx, g["noise_split"][:2 * idx.numel()], *[cur[k] for k in PARAMS]))
        prune(torch.cat((m, torch.zeros(2 * idx.numel(), dtype=torch.bool))))
        ids = decision_margins("merge", 0.1)
        m, idx, _ = D.select_merge_torch(cur["xyz"], cur["rotation"], cur["scaling"], ids, accum, denom, MAX_GRAD, EXTENT, PERCENT_DENSE, 0.1)
        index["merge"] = idx
        if idx.numel():
            append(D.merge_rows_torch(idx, ids, m, *[cur[k] for k in PARAMS]))
            prune(torch.cat((m, torch.zeros(idx.numel(), dtype=torch.bool))))
        radii = torch.zeros(cur["xyz"].shape[0], dtype=torch.float64)
    rel("opacity", torch.sigmoid(cur["opacity"].reshape(-1)), MIN_OPACITY)
    dist = cpu_knn(g["t_vertices"][None], cur["xyz"][None], 1)[0].reshape(-1)
    rel("vertex_dist", dist, 0.05)
    if max_screen_size:
        rel("world_scale", torch.exp(cur["scaling"]).max(1).values, 0.1 * EXTENT)
        if radii.abs().max() > 0:
            rel("radii", radii, float(max_screen_size))
    index["final"] = torch.nonzero(D.prune_mask_torch(cur["opacity"], cur["scaling"], radii, dist, MIN_OPACITY, EXTENT, max_screen_size)).reshape(-1)
    return margins, index, cur


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    mod = _load_reference(os.path.abspath(sys.argv[1]))
    res = {}
    for case in CASES:
        margins, index64, _ = float64_decision(case, max_screen_size=SCREEN[case])
        print(case, "float64 margins:", {k: f"{v:.3g}" for k, v in margins.items()})
        assert min(margins.values()) > MARGIN, f"{case}: a decision quantity within {MARGIN} of its threshold; take another seed"
        phases, final = run_reference(mod, case, max_screen_size=SCREEN[case])
        rows = P
        for ph in PHASES:
            n_sel = int(phases[ph]["mask"].sum())
            assert 16 <= n_sel <= rows // 2, f"{case}/{ph}: {n_sel} of {rows} rows selected"
            assert np.array_equal(phases[ph]["index"], index64[ph].numpy()), f"{case}/{ph}: float64 and the reference select differently"
            rows = rows + phases[ph][ROW_NAMES[0]].shape[0] - (int(phases[ph]["prune_filter"].sum()) if "prune_filter" in phases[ph] else 0)
            for k, v in phases[ph].items():
                res[f"{case}_{ph}_{k}"] = v
        n_final = int(phases["final"]["prune_filter"].sum())
        assert 16 <= n_final <= rows // 2 and np.array_equal(np.nonzero(phases["final"]["prune_filter"])[0], index64["final"].numpy())
        res[f"{case}_final_prune_filter"] = phases["final"]["prune_filter"]
        for k, v in final.items():
            res[f"{case}_final_{k}"] = v
        res[f"{case}_seed"] = np.int64(CASES[case])
        res[f"{case}_inputs_sha256"] = np.array(inputs_checksum(case))
        print(case, {ph: int(phases[ph]["mask"].sum()) for ph in PHASES}, "final prune", n_final, "rows", final["xyz"].shape[0])
    margins, index64, _ = float64_decision("guard", n=GUARD_P, max_screen_size=20)
    assert min(margins.values()) > MARGIN, margins
    phases, final = run_reference(mod, "guard", n=GUARD_P, max_screen_size=20)
    assert set(phases) == {"final"} and np.array_equal(np.nonzero(phases["final"]["prune_filter"])[0], index64["final"].numpy())
    res["guard_final_prune_filter"] = np.packbits(phases["final"]["prune_filter"])
    res["guard_final_rows"] = np.int64(final["xyz"].shape[0])
    res["guard_seed"] = np.int64(GUARD_SEED)
    res["guard_inputs_sha256"] = np.array(inputs_checksum("guard", n=GUARD_P))
    print("guard: rows", GUARD_P, "->", final["xyz"].shape[0])
    path = os.path.join(OUT, "densify_decision.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
