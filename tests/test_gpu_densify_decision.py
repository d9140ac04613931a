"""The fused densify-and-prune decision on the GPU (moss_amd.densify: joint_tables, select_*, prune_mask, *_rows, densify_and_prune_fused)
against the reference's own run (tests/golden/densify_decision.npz) and, on random cases, against the float64 ``*_torch`` forms.

Rules (tests/test_densify_decision_cpu.py): masks and index lists exact; rows within 64 eps32 S_e (``row_bars``).  Random cases,
P in {1, 2, 63, 64, 65, 255, 257, 4097} (the wave, workgroup and multi-workgroup edges of the ordered compaction), V = 256: a mask
element may be left out of the comparison only if its float64 decision quantity lies within 64 eps32 S of its threshold (S: |grad|,
the max scale, the KL's sum of absolute terms, sigmoid(opacity), the distance); at most 0.5 % of P, none for P <= 65.  Both forms get
the SAME neighbour indices (an input of the functions), so ties do not enter.  Checked on the CPU with this generator, float32
``*_torch`` against float64: NO mask element differs at any size in any mode (selected, clone / split / merge: 0/0/0 at P = 1 and 2,
7/7/9 at 63, 8/8/7 at 64, 3/4/6 at 65, 27/27/17 at 255, 30/32/23 at 257, 444/467/368 at 4097); elements within the bar of a threshold
(those that MAY be left out): none up to 63, 1 (merge) at 64, 65 and 257, 3 (merge) at 255, 3/3/15 at 4097 -- under the cap of 20.
"""
import numpy as np
import pytest
import torch

from moss_amd import densify as D
from tests import test_densify_decision_cpu as cpu
from tests.golden import make_golden_densify as gold

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 257, 4097]
MODES = ["clone", "split", "merge"]
EPS32, K = cpu.EPS32, cpu.K
MAX_GRAD, EXTENT, PD = 0.0002, 1.0, 0.01


def random_case(P, seed=0, fill="mixed"):
    """float32 CPU tensors: gradients uniform in [0, 2 max_grad], log-scales with the scale limit mid-distribution of the MAX."""
    rng = np.random.Generator(np.random.PCG64(1000 * P + seed))
    f32 = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))        # noqa: E731
    tv = rng.uniform(-0.5, 0.5, size=(256, 3))
    xyz = tv[rng.integers(0, 256, size=P)] + 0.02 * rng.normal(size=(P, 3))
    scale = np.exp(np.log(PD * EXTENT) - 0.55 + 0.7 * rng.normal(size=(P, 3)))
    rot = rng.normal(size=(P, 4))
    twin = np.nonzero(rng.random(P) < 0.4)[0]                             # near-duplicates of an earlier Gaussian: what kl_merge selects
    twin = twin[twin > 0]
    src = (twin * rng.random(twin.shape[0])).astype(np.int64)
    scale[twin] = scale[src] * np.exp(0.05 * rng.normal(size=(twin.shape[0], 3)))
    rot[twin] = rot[src] + 0.02 * rng.normal(size=(twin.shape[0], 4))
    xyz[twin] = xyz[src] + 0.1 * scale[src] * rng.normal(size=(twin.shape[0], 3))
    denom = rng.integers(0, 6, size=(P, 1)).astype(np.float64)
    denom[0] = 3.0
    grad = rng.uniform(0, 2 * MAX_GRAD, size=(P, 1))
    if fill == "none":
        grad[:] = 0.0
    elif fill == "all":
        grad[:], denom[:] = 2 * MAX_GRAD, 3.0
    g = {"xyz": f32(xyz), "features_dc": f32(rng.normal(size=(P, 1, 3))), "features_rest": f32(rng.normal(size=(P, 15, 3))),
         "opacity": f32(2 * rng.normal(size=(P, 1))), "scaling": f32(np.log(scale)), "rotation": f32(rot),
         "accum": f32(grad * denom), "denom": f32(denom), "max_radii2D": f32(rng.uniform(0, 40, size=P)),
         "vertex_dist": f32(rng.uniform(0, 0.1, size=P)), "lbs_weights": f32(3.0 * rng.dirichlet(np.ones(24), size=P)),
         "joint_F": f32(np.stack([gold._rodrigues(rng, 3, 0.4).sum(0) for _ in range(23)])),
         "noise": f32(rng.normal(size=(2 * P, 3)))}
    return g


def force_limits(mode, fill):
    """(scale limit as extent, KL threshold): "all" / "none" are forced through the gradients; "all" also opens the other tests."""
    if fill != "all":
        return EXTENT, {"clone": 0.4, "split": 0.4, "merge": 0.1}[mode]
    return {"clone": 1e6, "split": 1e-9, "merge": 1e6}[mode], {"clone": -1e30, "split": -1e30, "merge": 1e30}[mode]


def kl_abs_sum(xyz, rotation, act, ids):
    """S of the KL: every product of kl_div in absolute value (float64)."""
    R0, R1 = cpu._rot_abs(rotation[ids[:, 0]]), cpu._rot_abs(rotation[ids[:, 1]])
    s0, s1 = act[ids[:, 0]], act[ids[:, 1]]
    dm = (xyz[ids[:, 1]] - xyz[ids[:, 0]]).abs()
    M = R1.transpose(1, 2) @ R0
    tr = ((M * s0[:, None, :] / s1[:, :, None]) ** 2).sum((1, 2))
    maha = (((R1.transpose(1, 2) @ dm[..., None]).squeeze(-1) / s1) ** 2).sum(1)
    return 0.5 * (tr + maha + torch.log((s1 / s0) ** 2).abs().sum(1) + 3)


def undecided(mode, g64, ids, extent, kl_thr):
    """Elements whose float64 decision quantity lies within 64 eps32 S of a threshold."""
    P = g64["xyz"].shape[0]
    grad = D._padded_grad(g64["accum"], g64["denom"], P)
    act = torch.exp(g64["scaling"])
    smax = act.max(1).values
    u = ((grad - MAX_GRAD).abs() <= K * EPS32 * grad.abs()) | ((smax - PD * extent).abs() <= K * EPS32 * smax)
    kl = D.kl_div_torch(g64["xyz"], g64["rotation"], act, ids)
    return u | ((kl - kl_thr).abs() <= K * EPS32 * kl_abs_sum(g64["xyz"], g64["rotation"], act, ids))


def neighbours(xyz):
    from moss_amd.knn_cuda import knn
    if xyz.shape[0] < 2:
        return torch.zeros((xyz.shape[0], 2), dtype=torch.int64, device=xyz.device)
    return knn(xyz[None], xyz[None], 2)[1][0]


SELECT = {"clone": (D.select_clone, D.select_clone_torch), "split": (D.select_split, D.select_split_torch), "merge": (D.select_merge, D.select_merge_torch)}
PARAMS = gold.PARAMS


def emit(mode, dev_g, index, ids, noise, table, mask=None):
    p = [dev_g[k] for k in PARAMS]
    if mode == "clone":
        return D.clone_rows(index, noise, *p, dev_g["lbs_weights"], dev_g["denom"], table)
    if mode == "split":
        return D.split_rows(index, noise, *p)
    return D.merge_rows(index, ids, mask, *p)


def emit_torch(mode, g, index, ids, noise, table, mask=None):
    p = [g[k] for k in PARAMS]
    if mode == "clone":
        return D.clone_rows_torch(index, noise, *p, g["lbs_weights"], g["denom"], table)
    if mode == "split":
        return D.split_rows_torch(index, noise, *p)
    return D.merge_rows_torch(index, ids, mask, *p)


@pytest.mark.parametrize("fill", ["mixed", "none", "all"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", SIZES)
def test_select_and_emit_against_float64(gpu, hip_lib, P, mode, fill):
    """One phase on a random case: mask / ascending index list / count against the float64 form, rows within the bar, the same bytes
    from a second call, kl_out bit for bit moss_neighbour_kl."""
    g = random_case(P, fill=fill)
    dg = {k: v.to(gpu) for k, v in g.items()}
    g64 = {k: v.double() for k, v in g.items()}
    ids_d = neighbours(dg["xyz"])
    ids = ids_d.cpu()
    extent, kl_thr = force_limits(mode, fill)
    fused, ref_fn = SELECT[mode]
    sentinel = torch.full((P,), -7, dtype=torch.int32, device=gpu)
    mask, index, n, kl = fused(dg["xyz"], dg["rotation"], dg["scaling"], ids_d, dg["accum"], dg["denom"], MAX_GRAD, extent, PD, kl_thr,
                               want_kl=True, index_out=sentinel)
    mask2, index2, n2, kl2 = fused(dg["xyz"], dg["rotation"], dg["scaling"], ids_d, dg["accum"], dg["denom"], MAX_GRAD, extent, PD, kl_thr,
                                   want_kl=True)
    assert n == n2 and torch.equal(mask, mask2) and torch.equal(index, index2) and torch.equal(kl.view(torch.int32), kl2.view(torch.int32)), "run-to-run bytes"
    from moss_amd.activations import activate_gaussians
    with torch.no_grad():                                                 # the scales as THIS library activates them (csrc/activations.hip)
        act = activate_gaussians(dg["xyz"], None, None, dg["opacity"], dg["scaling"], dg["rotation"])[3]
    assert torch.equal(kl.view(torch.int32), D.neighbour_kl(dg["xyz"], dg["rotation"], act, ids_d).view(torch.int32)), "kl_out vs neighbour_kl"
    assert int(mask.sum()) == n == index.numel() and bool((sentinel[n:] == -7).all()), "count / untouched tail of the index list"
    assert torch.equal(index.long(), torch.nonzero(mask).reshape(-1)), "ascending index order"
    rmask, rindex, rn = ref_fn(g64["xyz"], g64["rotation"], g64["scaling"], ids, g64["accum"], g64["denom"], MAX_GRAD, extent, PD, kl_thr)
    if fill == "none":
        assert n == 0 and rn == 0
    if fill == "all":
        assert n == P == rn
    left_out = undecided(mode, g64, ids, extent, kl_thr) if fill == "mixed" else torch.zeros(P, dtype=torch.bool)
    differ = mask.cpu() != rmask
    cap = 0 if P <= 65 else int(0.005 * P)
    print(f"\nP {P} {mode} {fill}: selected {n}, differing {int(differ.sum())}, undecided {int(left_out.sum())} (cap {cap})")
    assert not bool((differ & ~left_out).any()), f"{mode}: mask differs at {torch.nonzero(differ & ~left_out).reshape(-1).tolist()[:8]}"
    assert int((differ & left_out).sum()) <= cap, f"{mode}: more than {cap} undecided elements differ"
    # ---- the rows of this selection, against float64 on the fused form's own index list (so a left-out element shifts nothing)
    table = D.joint_tables(dg["joint_F"], dg["denom"])
    n_new = 2 * n if mode == "split" else n
    noise = dg["noise"][:n_new].contiguous()
    pm = mask.clone()
    rows = emit(mode, dg, index, ids_d, noise, table, pm)
    rows2 = emit(mode, dg, index, ids_d, noise, table, mask.clone())
    t64 = D.joint_tables_torch(g64["joint_F"], g64["denom"])
    pm64 = mask.cpu().clone()
    ref = emit_torch(mode, g64, index.cpu(), ids, g64["noise"][:n_new], t64, pm64)
    ref32 = emit_torch(mode, g, index.cpu(), ids, g["noise"][:n_new], t64.float(), mask.cpu().clone())
    bars = cpu.row_bars(mode, index.cpu(), g64["noise"][:n_new], *[g64[k] for k in PARAMS], ids=ids, lbs_weights=g64["lbs_weights"],
                        denom=g64["denom"], table=t64)
    assert torch.equal(rows["source"].cpu(), ref["source"]), "source"
    if mode == "merge":
        assert torch.equal(pm.cpu(), pm64), "merge: prune filter"
    worst, worst32 = {}, {}
    for name in gold.ROW_NAMES:
        assert tuple(rows[name].shape) == tuple(ref[name].shape), name
        assert torch.equal(rows[name].view(torch.int32), rows2[name].view(torch.int32)), f"{name}: run-to-run bytes"
        worst[name] = cpu.worst_ratio(rows[name].cpu(), ref[name], bars[name])
        worst32[name] = cpu.worst_ratio(ref32[name], ref[name], bars[name])
    if n:
        print("   rows, error / bar (fused | float32 torch): " + ", ".join(f"{k[4:]} {worst[k]:.3g} | {worst32[k]:.3g}" for k in worst))
    for name, v in worst.items():
        assert v < 1.0, (mode, name, v)


@pytest.mark.parametrize("screen", [None, 20])
@pytest.mark.parametrize("P", SIZES)
def test_prune_mask_against_float64(gpu, hip_lib, P, screen):
    g = random_case(P)
    dg = {k: v.to(gpu) for k, v in g.items()}
    g64 = {k: v.double() for k, v in g.items()}
    m = D.prune_mask(dg["opacity"], dg["scaling"], dg["max_radii2D"], dg["vertex_dist"], 0.1, EXTENT, screen)
    m2 = D.prune_mask(dg["opacity"], dg["scaling"], dg["max_radii2D"], dg["vertex_dist"], 0.1, EXTENT, screen)
    ref = D.prune_mask_torch(g64["opacity"], g64["scaling"], g64["max_radii2D"], g64["vertex_dist"], 0.1, EXTENT, screen)
    sig, smax = torch.sigmoid(g64["opacity"].reshape(-1)), torch.exp(g64["scaling"]).max(1).values
    left = ((sig - 0.1).abs() <= K * EPS32 * sig) | ((g64["vertex_dist"] - 0.05).abs() <= K * EPS32 * 0.05)
    if screen:
        left |= ((smax - 0.1 * EXTENT).abs() <= K * EPS32 * smax) | ((g64["max_radii2D"] - screen).abs() <= K * EPS32 * screen)
    differ = m.cpu() != ref
    assert torch.equal(m, m2) and not bool((differ & ~left).any()) and int(differ.sum()) <= (0 if P <= 65 else int(0.005 * P))


def test_joint_table_against_float64_svd(gpu, hip_lib):
    """rot = U V^T with the reference's sign rule and the sorted S against float64 torch.linalg.svd -- also for an F whose singular
    values lie within 1e-3 of each other (U and V are ill-determined there, U V^T is not) and for a reflection-like F (det < 0).
    The bar is the one tests/test_gpu_pose.py holds its SVD-derived rotation to: K = 8 times what the torch form loses when it runs in
    float32 on the same inputs.  U and V are never compared."""
    rng = np.random.Generator(np.random.PCG64(5))
    F = np.stack([gold._rodrigues(rng, 3, 0.4).sum(0) for _ in range(23)])
    close = gold._rodrigues(rng, 1, 0.4)[0]
    F[3] = close @ np.diag([3.0, 3.0 * (1 - 4e-4), 3.0 * (1 - 9e-4)]) @ gold._rodrigues(rng, 1, 0.4)[0]
    F[7] = gold._rodrigues(rng, 1, 0.4)[0] @ np.diag([3.0, 2.0, -1.0]) @ gold._rodrigues(rng, 1, 0.4)[0]   # det < 0, separated singular values (the flipped direction is then well determined)
    F32 = torch.tensor(F, dtype=torch.float32)
    denom = torch.tensor([3.0, 1.0], dtype=torch.float32)
    t = D.joint_tables(F32.to(gpu), denom.to(gpu)).cpu().double()
    ref = D.joint_tables_torch(F32.double(), denom.double())
    ref32 = D.joint_tables_torch(F32, denom).double()
    bar_rot = 8.0 * float((ref32[1:, :9] - ref[1:, :9]).abs().max())
    bar_S = 8.0 * float((ref32[1:, 9:] - ref[1:, 9:]).abs().max())
    err_rot, err_S = float((t[1:, :9] - ref[1:, :9]).abs().max()), float((t[1:, 9:] - ref[1:, 9:]).abs().max())
    print(f"\njoint table: rot error {err_rot:.3g} (bar {bar_rot:.3g}), S error {err_S:.3g} (bar {bar_S:.3g})")
    assert bool((t[0] == 1).all()) and err_rot < bar_rot and err_S < bar_S
    # denom[0] = 0: the torch form's non-finite pattern, and no fault
    bad = D.joint_tables(F32.to(gpu), torch.zeros(2, device=gpu)).cpu()
    ref_bad = D.joint_tables_torch(F32, torch.zeros(2))
    assert torch.equal(bad.isnan(), ref_bad.isnan()) and bool((bad[0] == 1).all()) and bool(bad[1:].isnan().all())


@pytest.mark.parametrize("mode", MODES)
def test_unified_feature_views_give_the_same_rows(gpu, hip_lib, mode):
    """features_dc / features_rest as views of ONE (P,16,3) tensor (row stride 48) against two separate tensors: equal bytes."""
    g = random_case(257)
    dg = {k: v.to(gpu) for k, v in g.items()}
    ids = neighbours(dg["xyz"])
    mask, index, n = SELECT[mode][0](dg["xyz"], dg["rotation"], dg["scaling"], ids, dg["accum"], dg["denom"], MAX_GRAD, EXTENT, PD)
    assert n > 0
    table = D.joint_tables(dg["joint_F"], dg["denom"])
    noise = dg["noise"][:2 * n if mode == "split" else n].contiguous()
    a = emit(mode, dg, index, ids, noise, table, mask.clone())
    uni = torch.cat((dg["features_dc"], dg["features_rest"]), dim=1).contiguous()
    du = dict(dg, features_dc=uni[:, :1, :], features_rest=uni[:, 1:, :])
    b = emit(mode, du, index, ids, noise, table, mask.clone())
    for name in gold.ROW_NAMES:
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name


def test_out_of_range_neighbour_unselects(gpu, hip_lib):
    g = random_case(65, fill="all")
    dg = {k: v.to(gpu) for k, v in g.items()}
    ids = neighbours(dg["xyz"])
    ids[3, 1], ids[40, 0] = 65, -1
    mask, index, n = D.select_clone(dg["xyz"], dg["rotation"], dg["scaling"], ids, dg["accum"], dg["denom"], MAX_GRAD, 1e6, PD, -1e30)
    assert n == 63 and not bool(mask[3]) and not bool(mask[40])


def test_bad_arguments_are_refused_without_a_launch(hip_lib):
    """NULL blocks, an unknown mode, n_grads > P, a missing workspace, n_new != n_sel: MOSS_ERR_INVALID_ARG (-1) and a message; nothing
    is launched (these calls never reach a kernel, so they need no GPU)."""
    import ctypes
    from moss_amd import _lib
    assert hip_lib.moss_densify_select(None, None) == -1 and b"moss_densify_select" in hip_lib.moss_last_error()
    assert hip_lib.moss_densify_emit(None, None) == -1 and hip_lib.moss_densify_joint_table(None, None, None, None) == -1
    a = _lib.DensifySelectArgs()
    a.mode, a.P = 7, 4
    assert hip_lib.moss_densify_select(ctypes.byref(a), None) == -1 and b"mode" in hip_lib.moss_last_error()
    a.mode, a.n_grads = 0, 5
    assert hip_lib.moss_densify_select(ctypes.byref(a), None) == -1 and b"n_grads" in hip_lib.moss_last_error()
    a.n_grads = 4
    assert hip_lib.moss_densify_select(ctypes.byref(a), None) == -1 and b"count" in hip_lib.moss_last_error()
    e = _lib.DensifyEmitArgs()
    e.mode, e.P, e.n_sel, e.n_new, e.rest_floats, e.dc_stride, e.rest_stride = 1, 8, 2, 2, 45, 3, 45
    assert hip_lib.moss_densify_emit(ctypes.byref(e), None) == -1 and b"n_new" in hip_lib.moss_last_error()
    e.n_new, e.rest_stride = 4, 44
    assert hip_lib.moss_densify_emit(ctypes.byref(e), None) == -1 and b"stride" in hip_lib.moss_last_error()
    e.rest_stride = 45
    assert hip_lib.moss_densify_emit(ctypes.byref(e), None) == -1 and b"null" in hip_lib.moss_last_error()


# ---- the fixture: the reference's own run -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(cpu.FIXTURE)


def _fused_sequence(case, gpu):
    """MOSS's sequence, every selection and every row from the fused functions on the fixture's inputs: ({phase: mask, index, rows,
    prune_filter, bars}, final prune mask, final parameters, their lineage (tests/test_densify_decision_cpu.py: Lineage))."""
    from moss_amd.knn_cuda import knn
    g = gold.golden_inputs(case)
    cur = {k: g[k].to(gpu) for k in PARAMS}
    accum, denom = g["accum"].to(gpu).reshape(-1), g["denom"].to(gpu).reshape(-1)
    table = D.joint_tables(g["joint_F"].to(gpu), denom)
    lbs = g["lbs_weights"].to(gpu).reshape(-1, 24)
    out, lin = {}, cpu.Lineage(gold.P)
    for ph in gold.PHASES:
        p = [cur[k] for k in PARAMS]
        ids = neighbours(cur["xyz"])
        p64 = [t.cpu().double() for t in p]
        if ph == "clone":
            mask, index, n = D.select_clone(cur["xyz"], cur["rotation"], cur["scaling"], ids, accum, denom, gold.MAX_GRAD, gold.EXTENT,
                                            gold.PERCENT_DENSE, gold.KL_THRESHOLD, surface_mask=g["surface_mask"].to(gpu))
            noise = g["noise_clone"][:n]
            rows = D.clone_rows(index, noise.to(gpu), *p, lbs, denom, table)
            bars = cpu.row_bars(ph, index.cpu(), noise.double(), *p64, lbs_weights=g["lbs_weights"].double(), denom=g["denom"].double(),
                                table=table.cpu().double())
            filt = None
        elif ph == "split":
            mask, index, n = D.select_split(cur["xyz"], cur["rotation"], cur["scaling"], ids, accum, denom, gold.MAX_GRAD, gold.EXTENT,
                                            gold.PERCENT_DENSE, gold.KL_THRESHOLD)
            noise = g["noise_split"][:2 * n]
            rows = D.split_rows(index, noise.to(gpu), *p)
            bars = cpu.row_bars(ph, index.cpu(), noise.double(), *p64)
            filt = torch.cat((mask, torch.zeros(2 * n, dtype=torch.bool, device=gpu)))
        else:
            mask, index, n = D.select_merge(cur["xyz"], cur["rotation"], cur["scaling"], ids, accum, denom, gold.MAX_GRAD, gold.EXTENT,
                                            gold.PERCENT_DENSE, 0.1)
            filt = mask.clone()
            rows = D.merge_rows(index, ids, filt, *p)
            bars = cpu.row_bars(ph, index.cpu(), None, *p64, ids=ids.cpu())
            filt = torch.cat((filt, torch.zeros(n, dtype=torch.bool, device=gpu)))
        bars = lin.append(ph, index.cpu(), ids.cpu(), bars)
        out[ph] = {"mask": mask, "index": index, "rows": rows, "prune_filter": filt, "bars": bars}
        for k, r in zip(PARAMS, gold.ROW_NAMES):
            cur[k] = torch.cat((cur[k], rows[r]), 0)
        if filt is not None:
            lin.prune(filt)
            for k in PARAMS:
                cur[k] = cur[k][~filt].contiguous()
    dist = knn(g["t_vertices"].to(gpu)[None], cur["xyz"][None], 1)[0].reshape(-1)
    final = D.prune_mask(cur["opacity"], cur["scaling"], torch.zeros_like(dist), dist, gold.MIN_OPACITY, gold.EXTENT, gold.SCREEN[case])
    lin.prune(final)
    return out, final, {k: cur[k][~final] for k in PARAMS}, lin


@pytest.mark.parametrize("case", list(gold.CASES))
def test_fused_functions_reproduce_the_reference(gpu, hip_lib, golden, case):
    """Every fused function against the reference's own run: masks, index lists and prune filters exactly, rows within the bar
    (printed beside the float32 torch form's), asserted per phase and per tensor."""
    out, final, params, lin = _fused_sequence(case, gpu)
    ref32 = cpu.replay(case, torch.float32)
    worst, worst32 = {}, {}
    for ph in gold.PHASES:
        o = out[ph]
        assert np.array_equal(o["mask"].cpu().numpy(), golden[f"{case}_{ph}_mask"]), f"{ph}: mask"
        assert np.array_equal(o["index"].cpu().numpy(), golden[f"{case}_{ph}_index"]), f"{ph}: index list"
        if o["prune_filter"] is not None:
            assert np.array_equal(o["prune_filter"].cpu().numpy(), golden[f"{case}_{ph}_prune_filter"]), f"{ph}: prune filter"
        for name in gold.ROW_NAMES:
            ref = golden[f"{case}_{ph}_{name}"]
            assert tuple(o["rows"][name].shape) == ref.shape, (ph, name)
            worst[f"{ph}.{name[4:]}"] = cpu.worst_ratio(o["rows"][name].cpu(), ref, o["bars"][name])
            worst32[f"{ph}.{name[4:]}"] = cpu.worst_ratio(ref32[ph]["rows"][name], ref, o["bars"][name])
    assert np.array_equal(final.cpu().numpy(), golden[f"{case}_final_prune_filter"]), "final prune mask"
    for k in PARAMS:
        assert tuple(params[k].shape) == golden[f"{case}_final_{k}"].shape, k
    final32 = cpu.final_ratios(ref32["final"]["params"], lin, golden, case, gold.golden_inputs(case))
    for k, v in cpu.final_ratios(params, lin, golden, case, gold.golden_inputs(case)).items():    # the final parameters, by value
        worst[f"final.{k}"], worst32[f"final.{k}"] = v, final32[k]
    print(f"\n{case}: worst error / bar (fused | float32 torch): " + ", ".join(f"{k} {v:.3g} | {worst32[k]:.3g}" for k, v in worst.items() if v > 0 or worst32[k] > 0))
    for k, v in worst.items():
        assert v < 1.0, (k, v)


def _scene_from(g):
    from types import SimpleNamespace
    return SimpleNamespace(P=int(g["xyz"].shape[0]), means3D=g["xyz"], shs=torch.cat((g["features_dc"], g["features_rest"]), 1),
                           scales=torch.exp(g["scaling"]), rotations=g["rotation"], opacities=torch.sigmoid(g["opacity"]))


def _driver_set(g, gpu):
    """A unified-feature GaussianSet + GradBucket + FlatAdamW holding exactly the fixture's raw parameters; every element of both
    moment buffers gets a value of its own (exact small numbers), so that a row's moments identify the row."""
    from moss_amd import dist as mdist
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.optim import FlatAdamW
    pc = GaussianSet(_scene_from(g), sh_degree=3, device=gpu, unified_features=True)
    bucket = mdist.GradBucket(list(pc.parameters()))
    opt = FlatAdamW(pc.param_groups(), bucket, eps=1e-15, capturable=True)
    with torch.no_grad():                                                 # (the constructor goes through activations: put the raw values back)
        pc._opacity.copy_(g["opacity"].to(gpu)); pc._scaling.copy_(g["scaling"].to(gpu))
        n = opt.exp_avg.numel()
        opt.exp_avg.copy_(torch.arange(n, device=gpu, dtype=torch.float32) + 1.0)
        opt.exp_avg_sq.copy_(torch.arange(n, device=gpu, dtype=torch.float32) + 0.5)
    return pc, bucket, opt


def _moments(pc, opt):
    """{parameter: (exp_avg, exp_avg_sq)} of the five parameters of a unified-feature set, cloned."""
    idx = {id(p): i for i, p in enumerate(opt.bucket.params)}
    return {k: tuple(t.clone() for t in opt._moments_of(idx[id(p)]))
            for k, p in (("xyz", pc._xyz), ("features", pc._features), ("opacity", pc._opacity), ("scaling", pc._scaling), ("rotation", pc._rotation))}


@pytest.mark.parametrize("case", list(gold.CASES))
def test_driver_reproduces_the_reference_on_a_gaussian_set(gpu, hip_lib, golden, case):
    """densify_and_prune_fused on GaussianSet + FlatAdamW + DensifyStats with the fixture's inputs: the final parameters are the
    fixture's BY VALUE (rows that descend from the inputs bit-equal, made rows within their bars); both optimizer moments of every
    surviving row are bit for bit that row's moments before, and both moments of every made row are exactly zero (the row map comes
    from the phases' masks and prune filters, which are exact); one host read per phase plus the prune; the statistics follow."""
    g = gold.golden_inputs(case)
    pc, bucket, opt = _driver_set(g, gpu)
    stats = D.DensifyStats(gold.P, device=gpu)
    stats.xyz_gradient_accum.copy_(g["accum"].to(gpu)); stats.denom.copy_(g["denom"].to(gpu)); stats.max_radii2D.copy_(g["max_radii2D"].to(gpu))
    m_before = _moments(pc, opt)
    noise = iter([g["noise_clone"], g["noise_split"]])
    rep = D.densify_and_prune_fused(pc, opt, stats, g["joint_F"].to(gpu), g["lbs_weights"].to(gpu), gold.MAX_GRAD, gold.MIN_OPACITY, gold.EXTENT,
                                    gold.SCREEN[case], g["t_vertices"].to(gpu), kl_threshold=gold.KL_THRESHOLD,
                                    surface_mask=g["surface_mask"].to(gpu), generator=lambda n: next(noise)[:n], percent_dense=gold.PERCENT_DENSE)
    print("\n", case, rep)
    assert rep["host_reads"] <= 4
    for ph, key in (("clone", "cloned"), ("split", "split"), ("merge", "merged")):
        assert rep[key] == int(golden[f"{case}_{ph}_mask"].sum()), ph
    assert rep["pruned"] == int(golden[f"{case}_final_prune_filter"].sum())
    assert rep["rows_after"] == golden[f"{case}_final_xyz"].shape[0] == pc._xyz.shape[0] == stats.denom.shape[0]
    lin = cpu.replay(case, torch.float64)["final"]["lineage"]            # (masks and filters are exact, so this is the driver's row map too)
    got = {"xyz": pc._xyz, "features_dc": pc._features_dc, "features_rest": pc._features_rest, "opacity": pc._opacity,
           "scaling": pc._scaling, "rotation": pc._rotation}
    ratios = cpu.final_ratios(got, lin, golden, case, g)
    print("   final parameters, worst error / bar:", {k: round(v, 4) for k, v in ratios.items()})
    for k, v in ratios.items():
        assert v < 1.0, (k, v)
    old, origin = (lin.origin >= 0).to(gpu), lin.origin.clamp_min(0).to(gpu)
    assert int(old.sum()) > 100 and int((~old).sum()) > 100
    for k, (m, v) in _moments(pc, opt).items():
        for name, after, before in (("exp_avg", m, m_before[k][0]), ("exp_avg_sq", v, m_before[k][1])):
            assert after.shape[0] == rep["rows_after"], (k, name)
            assert torch.equal(after[old], before[origin[old]]), f"{k}.{name}: a surviving row lost its moments"
            assert not bool(after[~old].any()), f"{k}.{name}: a new row has non-zero moments"
    assert bool((stats.xyz_gradient_accum == 0).all()) and bool((stats.max_radii2D == 0).all())


def test_driver_guard_case_only_prunes(gpu, hip_lib, golden):
    """45 696 rows: no phase runs, the prune uses the statistics' max_radii2D; the fixture's final row count and mask."""
    g = gold.golden_inputs("guard", n=gold.GUARD_P)
    pc, bucket, opt = _driver_set(g, gpu)
    stats = D.DensifyStats(gold.GUARD_P, device=gpu)
    stats.xyz_gradient_accum.copy_(g["accum"].to(gpu)); stats.denom.copy_(g["denom"].to(gpu)); stats.max_radii2D.copy_(g["max_radii2D"].to(gpu))
    before = pc._rotation.detach().clone()
    rep = D.densify_and_prune_fused(pc, opt, stats, g["joint_F"].to(gpu), g["lbs_weights"].to(gpu), gold.MAX_GRAD, gold.MIN_OPACITY, gold.EXTENT,
                                    20, g["t_vertices"].to(gpu), percent_dense=gold.PERCENT_DENSE)
    ref = torch.as_tensor(np.unpackbits(golden["guard_final_prune_filter"])[:gold.GUARD_P].astype(bool))
    assert rep["cloned"] == rep["split"] == rep["merged"] == 0 and rep["host_reads"] == 1
    assert rep["rows_after"] == int(golden["guard_final_rows"]) == pc._xyz.shape[0]
    assert torch.equal(pc._rotation.detach().cpu(), before.cpu()[~ref])


def test_event_with_rows_changed_recaptures_after_the_driver(gpu, hip_lib):
    """On the headline's objects (tests/test_gpu_surgery.py FormA): after a few captured steps, densify_and_prune_fused changes the rows,
    densification_event(rows_changed=True) re-learns the capacity and re-captures, and the next steps run.  (The moments are checked
    row by row in test_driver_reproduces_the_reference_on_a_gaussian_set.)"""
    from moss_amd import scenes
    from moss_amd.surgery import densification_event
    from tests import test_gpu_headline as thl
    from tests import test_gpu_surgery as sg
    scene = scenes.config2()
    gt, mask = sg._target(scenes.config2, gpu)
    A = sg.FormA(scene, gpu, gt, mask, thl.bench_transforms(scene.P))
    for _ in range(3):
        A.step()
    torch.cuda.synchronize(gpu)
    P0 = int(A.pc._xyz.shape[0])
    A.stats.xyz_gradient_accum.uniform_(0, 4 * MAX_GRAD); A.stats.denom.fill_(2.0)
    rng = torch.Generator(device=gpu); rng.manual_seed(3)
    extent = float((A.pc._xyz.detach().max(0).values - A.pc._xyz.detach().min(0).values).max())
    scale_mid = float(torch.exp(A.pc._scaling.detach()).max(1).values.median())
    rep = D.densify_and_prune_fused(A.pc, A.opt, A.stats, torch.eye(3, device=gpu).repeat(23, 1, 1) * 2.0, torch.full((P0, 24), 2.0 / 24, device=gpu),
                                    MAX_GRAD, 0.005, extent, None, A.pc._xyz.detach().clone(), generator=rng, percent_dense=scale_mid / extent)
    print("\n", rep)
    assert rep["cloned"] > 0 and rep["rows_after"] != P0 and rep["host_reads"] <= 4
    T = thl.bench_transforms(rep["rows_after"]).to(gpu).contiguous()
    A.T = T
    ev = densification_event(A.pc, A.opt, rows_changed=True, stats=A.stats, context=A.ctx, graphed=A.graphed, probe=A.probe)
    assert ev["recaptured"] and ev["rows_before"] == ev["rows_after"] == rep["rows_after"]
    for _ in range(2):
        A.step()
    torch.cuda.synchronize(gpu)
    A.graphed.check()
    assert A.graphed.dropped_frames == 0 and bool(torch.isfinite(A.opt.flat_params).all())
    # the default keeps today's behaviour: nothing appended, nothing pruned, rows_changed False -> no re-capture
    assert not densification_event(A.pc, A.opt, stats=A.stats, context=A.ctx, graphed=A.graphed, probe=A.probe)["recaptured"]
