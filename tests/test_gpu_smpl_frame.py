"""The fused per-frame SMPL op on the device (C ABI moss_smpl_frame_forward / _backward, moss_amd.lbs.smpl_frame_fused): the kernels
against float64 runs of moss_amd.lbs.smpl_joint_transforms / vertex_offsets, the drop-in ``coarse_deform_c2source(fused_frame=True)``
against the reference's own numbers (tests/golden/lbs_deform.npz), skewed ids, determinism and full writes, capture in a hipGraph with
a new frame per replay, and the renderer's ``pipe.smpl_frame_in_op``.

The bars.  Forward: an element of A_big, A_obs, D[ids] or rot_mats may be off by  64 eps32 s,  s the tensor's largest magnitude in
the case (float64) and 64 the constant tests/test_lbs_cpu.py uses for this chain.  Beside the fused op's ratio every test prints the
ratio of the float32 torch form (the parent's code on the same inputs) to the same bar.
Backward: element e of g_correct_Rs may be off by  64 eps32 S_e,  S_e = sum |terms|: the sum of the absolute values of the products
that make up the element.  The form chosen: the adjoint itself evaluated in float64 with every factor replaced by its absolute value
(:func:`abs_terms`) --
    |g_feat| = sum_i sum_c |posedirs[ids_i, c, :]| |g_d[i, c]|,
    |gGR_j| = |g_A_j[:3,:3]| + |g_A_j[:3,3]| |joints_j|^T,  |gGt_j| = |g_A_j[:3,3]|,  and for j = J-1 .. 1, p = parent[j]:
    |g_rot_j| = |G_p.R|^T |gGR_j|,  |gGR_p| += |gGR_j| |rot_j|^T + |gGt_j| |rel_j|^T,  |gGt_p| += |gGt_j|,
    S[q] = |rot_raw[q+1]|^T (|g_rot[q+1]| + |g_feat[9q .. 9q+8]|)
-- which is the definition, not an approximation of it.  (Float64 autograd of the torch chain on |g_A_obs|, |g_d| and |posedirs|
keeps the signs of the rotations and so lets terms cancel: an element of it can fall far below sum |terms|; it is printed beside the
ratio as ``S_autograd / S`` for the reader, not asserted on.)  Each test prints the worst ratio of error to bar it met.
"""
import ctypes
import gc
import time

import numpy as np
import pytest
import torch

from moss_amd import lbs as mlbs

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
SIZES = [1, 63, 64, 65, 6890, 45695, 100000]
V = 6890
_BODIES = {}


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    yield
    _BODIES.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch._C._cuda_clearCublasWorkspaces()
    torch.cuda.empty_cache()


def body_of(J, dev):
    if J not in _BODIES:
        _BODIES[J] = {k: v.to(dev) for k, v in mlbs.synthetic_body_model(V, J, seed=40 + J).items()}
    return _BODIES[J]


def f64(d):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in d.items()}


def make_case(P, J, seed, dev, with_cR=True, ids=None):
    body = body_of(J, dev)
    fr = {k: v.to(dev) for k, v in mlbs.synthetic_frame(seed, J).items()}
    big = {k: v.to(dev) for k, v in mlbs.synthetic_frame(0, J, big_pose=True).items()}
    g = torch.Generator().manual_seed(seed)
    if ids is None:
        ids = torch.randint(0, V, (P,), generator=g)
    cR = mlbs.batch_rodrigues(0.1 * torch.randn(J - 1, 3, generator=g)).to(dev).contiguous() if with_cR else None
    return body, fr, big, ids.to(dev), cR


def torch_form(body, fr, big, ids, cR):
    """The parent's torch per-frame part in the dtype of its inputs: A_big, A_obs, D[ids], rot_mats."""
    J = body["weights"].shape[-1]
    A_big = mlbs.smpl_joint_transforms(body, big)[0][0]
    rot = mlbs.batch_rodrigues(fr["poses"].reshape(-1, 3).to(body["v_template"])).reshape(J, 3, 3)
    if cR is not None:
        rot = torch.cat([rot[:1], rot[1:] @ cR], 0)
    A_obs = mlbs.smpl_joint_transforms(body, fr, rot_mats=rot)[0][0]
    D = mlbs.vertex_offsets(body, fr, big, rot)
    return A_big, A_obs, D[ids], rot


def abs_terms(body, fr, ids, cR, gA, gd):
    """S (J-1,3,3) of the module docstring, float64."""
    J = body["weights"].shape[-1]
    par = [int(v) for v in body["kintree_table"][0].tolist()]
    vs = body["v_template"] + (body["shapedirs"][..., :fr["shapes"].shape[-1]] * fr["shapes"][0]).sum(-1)
    jt = body["J_regressor"] @ vs
    raw = mlbs.batch_rodrigues(fr["poses"].reshape(-1, 3))
    rot = raw if cR is None else torch.cat([raw[:1], raw[1:] @ cR], 0)
    rel = jt.clone()
    GR = [rot[0]]
    for j in range(1, J):
        rel[j] = jt[j] - jt[par[j]]
        GR.append(GR[par[j]] @ rot[j])
    g_feat = torch.zeros(9 * (J - 1), dtype=torch.float64, device=gd.device)
    apd = body["posedirs"].abs()
    for lo in range(0, ids.shape[0], 8192):                       # (chunked: (P,3,F) float64 at once would be 1 GB)
        g_feat += torch.einsum("ick,ic->k", apd[ids[lo:lo + 8192]], gd[lo:lo + 8192].abs())
    gGR = [gA[j, :3, :3].abs() + gA[j, :3, 3].abs()[:, None] * jt[j].abs()[None, :] for j in range(J)]
    gGt = [gA[j, :3, 3].abs() for j in range(J)]
    gR = [None] * J
    for j in range(J - 1, 0, -1):
        p = par[j]
        gR[j] = GR[p].abs().T @ gGR[j]
        gGR[p] = gGR[p] + gGR[j] @ rot[j].abs().T + gGt[j][:, None] * rel[j].abs()[None, :]
        gGt[p] = gGt[p] + gGt[j]
    return torch.stack([raw[1 + q].abs().T @ (gR[1 + q] + g_feat[9 * q:9 * q + 9].reshape(3, 3)) for q in range(J - 1)])


def tensor_ratio(got, ref):
    return float((got.double() - ref).abs().max()) / (64.0 * EPS32 * max(float(ref.abs().max()), 1e-30))


@pytest.mark.parametrize("J", [24, 55])
@pytest.mark.parametrize("P", SIZES)
def test_forward_matches_float64(gpu, hip_lib, P, J):
    worst, worst_torch = 0.0, 0.0
    for with_cR in (True, False):
        body, fr, big, ids, cR = make_case(P, J, 100 + P % 97 + J, gpu, with_cR)
        got = mlbs.smpl_frame_fused(body, fr, big, ids, correct_Rs=cR)
        assert [tuple(t.shape) for t in got] == [(J, 4, 4), (J, 4, 4), (P, 3), (J, 3, 3)]
        ref = torch_form(f64(body), f64(fr), f64(big), ids, None if cR is None else cR.double())
        t32 = torch_form(body, fr, big, ids, cR)
        worst = max([worst] + [tensor_ratio(a, b) for a, b in zip(got, ref)])
        worst_torch = max([worst_torch] + [tensor_ratio(a, b) for a, b in zip(t32, ref)])
        assert torch.equal(got[0][:, 3], torch.tensor([0.0, 0, 0, 1], device=gpu).expand(J, 4))
    print(f"\nforward P={P} J={J}: worst error / bar: fused {worst:.3g}, float32 torch form {worst_torch:.3g}")
    assert worst < 1.0


def _backward_ratio(gpu, P, J, seed, ids=None):
    body, fr, big, ids, cR = make_case(P, J, seed, gpu, True, ids=ids)
    g = torch.Generator(device=gpu).manual_seed(P + J)
    gA = torch.randn(J, 4, 4, generator=g, device=gpu, dtype=torch.float64)
    gA[:, 3] = 0                                                  # (what moss_lbs_deform_backward hands back: row 3 is zero)
    gd = torch.randn(P, 3, generator=g, device=gpu, dtype=torch.float64)
    c32 = cR.clone().requires_grad_(True)
    _, A_obs, d, _ = mlbs.smpl_frame_fused(body, fr, big, ids, correct_Rs=c32)
    torch.autograd.backward([A_obs, d], [gA.float(), gd.float()])
    b64, fr64, big64 = f64(body), f64(fr), f64(big)
    c64 = cR.double().requires_grad_(True)
    _, A0, d0, _ = torch_form(b64, fr64, big64, ids, c64)
    ref, = torch.autograd.grad((A0 * gA).sum() + (d0 * gd).sum(), c64)
    S = abs_terms(b64, fr64, ids, cR.double(), gA, gd)
    # the float32 torch form, and the signed approximation of S (see the module docstring)
    t32 = cR.clone().requires_grad_(True)
    _, A1, d1, _ = torch_form(body, fr, big, ids, t32)
    g32, = torch.autograd.grad((A1 * gA.float()).sum() + (d1 * gd.float()).sum(), t32)
    ca = cR.double().requires_grad_(True)
    _, A2, d2, _ = torch_form({**b64, "posedirs": b64["posedirs"].abs()}, fr64, big64, ids, ca)
    Sa, = torch.autograd.grad((A2 * gA.abs()).sum() + (d2 * gd.abs()).sum(), ca)
    bar = 64.0 * EPS32 * S
    return (float(((c32.grad.double() - ref).abs() / bar).max()), float(((g32.double() - ref).abs() / bar).max()),
            float((Sa.abs() / S).min()))


@pytest.mark.parametrize("J", [24, 55])
@pytest.mark.parametrize("P", SIZES)
def test_backward_matches_float64_autograd(gpu, hip_lib, P, J):
    r, r32, sa = _backward_ratio(gpu, P, J, 200 + P % 89 + J)
    print(f"\nbackward P={P} J={J}: worst error / bar: fused {r:.3g}, float32 torch form {r32:.3g}; min S_autograd / S {sa:.3g}")
    assert r < 1.0


def _golden_model(g, dev):
    from moss_amd.knn_cuda import KNN
    from types import SimpleNamespace
    return SimpleNamespace(SMPL_NEUTRAL={k: v.to(dev) for k, v in g["body"].items()}, knn=KNN(k=1, transpose_mode=True))


@pytest.mark.parametrize("case", ["plain", "refined"])
def test_drop_in_with_fused_frame_reproduces_reference_golden(gpu, hip_lib, case):
    """coarse_deform_c2source(fused_frame=True) reproduces the reference's float32 outputs and gradients (query_pts, lbs_weights,
    correct_Rs) of tests/golden/lbs_deform.npz within the bars the flag-off drop-in is held to (tests/test_gpu_lbs.py: twice
    output_bar / grad_bar of tests/test_lbs_cpu.py, two float32 computations)."""
    from tests.golden import make_golden_lbs as gold
    from tests.test_lbs_cpu import FIXTURE, chain_torch, grad_bar, output_bar
    golden = np.load(FIXTURE)
    _, _, kappa, _ = chain_torch(case, requires_grad=False)
    g = gold.golden_inputs(case, device=gpu)
    model = _golden_model(g, gpu)
    q = g["query_pts"].clone().requires_grad_(True)
    L = None if g["lbs_weights"] is None else g["lbs_weights"].clone().requires_grad_(True)
    cR = None if g["correct_Rs"] is None else g["correct_Rs"].clone().requires_grad_(True)
    out = mlbs.coarse_deform_c2source(model, q, g["params"], g["t_params"], g["t_vertices"], lbs_weights=L, correct_Rs=cR,
                                      return_transl=True, fused_frame=True)
    out = dict(zip(gold.OUTPUTS, out))
    worst = {}
    for k in gold.OUTPUTS:
        ref = golden[f"{case}_{k}"]
        got = out[k].detach().cpu().numpy()
        assert got.shape == ref.shape, k
        worst[k] = float(np.abs(got - ref).max()) / (2 * output_bar(ref, kappa))
    loss = sum((out[k] * g["cotangents"][k]).sum() for k in gold.COTANGENT_OF)
    leaves = {k: v for k, v in {"query_pts": q, "lbs_weights": L, "correct_Rs": cR}.items() if v is not None}
    grads = torch.autograd.grad(loss, list(leaves.values()))
    for name, gr in zip(leaves, grads):
        ref = golden[f"{case}_grad_{name}"]
        worst["grad_" + name] = float(np.abs(gr.cpu().numpy() - ref).max()) / (2 * grad_bar(ref, kappa))
    print(f"\n{case}: GPU drop-in with fused_frame vs reference float32, fraction of the bar: "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) < 1.0, worst


@pytest.mark.parametrize("skew", ["all_equal", "half_in_one"])
def test_skewed_ids(gpu, hip_lib, skew):
    """Every Gaussian at one vertex, and half of them at one vertex: the backward stays within its bar and a forward + backward call
    (warm) ends within 5 s -- the reduction walks Gaussians, not vertices, so a crowded vertex costs what any other does."""
    P, J = 100000, 24
    ids = torch.full((P,), 1234, dtype=torch.int64)
    if skew == "half_in_one":
        ids[::2] = torch.randint(0, V, (P // 2,), generator=torch.Generator().manual_seed(1))
    _backward_ratio(gpu, 64, J, 5)                                # (warm-up of every kernel)
    torch.cuda.synchronize(gpu)
    body, fr, big, dids, cR = make_case(P, J, 6, gpu, True, ids=ids)
    t0 = time.perf_counter()
    c = cR.clone().requires_grad_(True)
    _, A_obs, d, _ = mlbs.smpl_frame_fused(body, fr, big, dids, correct_Rs=c)
    (A_obs.sum() + d.sum()).backward()
    torch.cuda.synchronize(gpu)
    dt = time.perf_counter() - t0
    r, r32, _ = _backward_ratio(gpu, P, J, 6, ids=ids)
    ref_d = torch_form(f64(body), f64(fr), f64(big), dids, cR.double())[2]
    rf = tensor_ratio(d.detach(), ref_d)
    print(f"\nskewed ids ({skew}): backward error / bar: fused {r:.3g}, float32 torch form {r32:.3g}; d error / bar {rf:.3g}; "
          f"forward + backward {dt * 1e3:.2f} ms")
    assert r < 1.0 and rf < 1.0 and dt < 5.0


def _run(body, fr, big, ids, c, gA, gd):
    c.grad = None
    out = mlbs.smpl_frame_fused(body, fr, big, ids, correct_Rs=c)
    torch.autograd.backward([out[1], out[2]], [gA, gd])
    return [t.detach() for t in out] + [c.grad]


def test_deterministic_and_fully_written(gpu, hip_lib):
    """Two calls on the same inputs are bit-identical, forward and backward; through the C ABI, outputs (and the workspace) that start
    as NaN come back without one; ids outside [0, V) give NaN rows of d and add nothing to the gradient."""
    from moss_amd._lib import SMPL_FRAME_SAVED_FLOATS_PER_JOINT, SmplFrameArgs, SmplFrameBackwardArgs, call, lib
    P, J = 100000, 24
    body, fr, big, ids, cR = make_case(P, J, 7, gpu)
    gA, gd = torch.randn(J, 4, 4, device=gpu), torch.randn(P, 3, device=gpu)
    c = cR.clone().requires_grad_(True)
    a = [t.clone() for t in _run(body, fr, big, ids, c, gA, gd)]
    b = _run(body, fr, big, ids, c, gA, gd)
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), i
    nan = lambda *s: torch.full(s, float("nan"), device=gpu)      # noqa: E731
    A_big, A_obs, d, rot, saved = nan(J, 4, 4), nan(J, 4, 4), nan(P, 3), nan(J, 3, 3), nan(SMPL_FRAME_SAVED_FLOATS_PER_JOINT * J)
    nbytes = int(lib().moss_smpl_frame_workspace_bytes(P, V, J))
    ws = torch.full((nbytes // 4,), float("nan"), device=gpu)
    par = [-1] + [int(v) for v in body["kintree_table"][0].tolist()][1:]
    f = SmplFrameArgs()
    f.P, f.V, f.J, f.num_betas_big, f.num_betas, f.shapedirs_stride = P, V, J, 10, 10, 10
    f.parents[:J] = par
    f.v_template, f.shapedirs, f.posedirs, f.J_regressor = (body[k].data_ptr() for k in ("v_template", "shapedirs", "posedirs", "J_regressor"))
    f.poses_big, f.shapes_big, f.poses, f.shapes = big["poses"].data_ptr(), big["shapes"].data_ptr(), fr["poses"].data_ptr(), fr["shapes"].data_ptr()
    f.correct_Rs, f.vert_ids = cR.data_ptr(), ids.data_ptr()
    f.A_big, f.A_obs, f.d, f.rot_mats, f.saved = A_big.data_ptr(), A_obs.data_ptr(), d.data_ptr(), rot.data_ptr(), saved.data_ptr()
    f.workspace, f.workspace_bytes = ws.data_ptr(), nbytes
    call("moss_smpl_frame_forward", gpu, ctypes.byref(f))
    for i, (u, v) in enumerate(zip((A_big, A_obs, d, rot), a)):
        assert torch.equal(u, v), i
    assert bool(torch.isfinite(saved).all())
    g = nan(J - 1, 3, 3)
    ws.fill_(float("nan"))
    k = SmplFrameBackwardArgs()
    k.P, k.V, k.J = P, V, J
    k.parents[:J] = par
    k.posedirs, k.vert_ids, k.saved = body["posedirs"].data_ptr(), ids.data_ptr(), saved.data_ptr()
    k.g_A_obs, k.g_d, k.g_correct_Rs = gA.data_ptr(), gd.data_ptr(), g.data_ptr()
    k.workspace, k.workspace_bytes = ws.data_ptr(), nbytes
    call("moss_smpl_frame_backward", gpu, ctypes.byref(k))
    assert torch.equal(g, a[4])
    # ids out of range
    bad = torch.tensor([0, 17, P - 1], device=gpu)
    ids2 = ids.clone()
    ids2[bad] = torch.tensor([-1, V, 1 << 40], device=gpu)
    gd2 = gd.clone()
    gd2[bad] = float("nan")                                       # (what lbs_deform's backward writes there)
    out = _run(body, fr, big, ids2, c, gA, gd2)
    ok = torch.ones(P, dtype=torch.bool, device=gpu)
    ok[bad] = False
    assert bool(torch.isnan(out[2][bad]).all()) and torch.equal(out[2][ok], a[2][ok]) and bool(torch.isfinite(out[4]).all())
    keep = gd.clone()
    keep[bad] = 0
    ids3 = ids.clone()
    ids3[bad] = 0
    assert torch.equal(_run(body, fr, big, ids3, c, gA, keep)[4], out[4])


def test_captured_replays_new_frames(gpu, hip_lib):
    """forward + backward captured once (moss_amd.graphs.GraphedStep: a host synchronisation would fail the capture), replayed over
    four frames whose poses and correct_Rs are copied into the static inputs: every replay equals the eager call bit for bit."""
    from moss_amd.graphs import GraphedStep
    P, J = 45695, 24
    body, fr, big, ids, cR = make_case(P, J, 300, gpu)
    frames = [make_case(P, J, 300 + k, gpu) for k in range(4)]
    gA, gd = torch.randn(J, 4, 4, device=gpu), torch.randn(P, 3, device=gpu)
    c = cR.clone().requires_grad_(True)

    def fn():
        return _run(body, fr, big, ids, c, gA, gd)

    fn()                                                          # (the parent table is read on the host here, outside the capture)
    step = GraphedStep(fn, warmup=2)
    first = None
    for k in range(4):
        with torch.no_grad():
            fr["poses"].copy_(frames[k][1]["poses"])
            c.copy_(frames[k][4])
        got = [v.clone() for v in step()]
        torch.cuda.synchronize(gpu)
        ref = [v.clone() for v in fn()]
        for i, (u, v) in enumerate(zip(got, ref)):
            assert torch.equal(u, v), (k, i)
        if first is None:
            first = got
        else:
            assert not torch.equal(got[1], first[1]) and not torch.equal(got[4], first[4])


def test_renderer_smpl_frame_in_op(gpu, hip_lib):
    """render() with lbs_in_op + pose_head_in_op + lbs_weights_in_op + smpl_frame_in_op against the same call with smpl_frame_in_op
    off: the image and the gradients of the pose head's parameters within the bars tests/test_gpu_pose.py's
    test_renderer_pose_head_in_op uses (image max 2 x 2e-3, mean 2 x 1e-5; parameter gradients, relative to the gradient's size,
    2 K x the pose fixture's largest float32 error)."""
    from moss_amd import lbs_weights as mlw
    from moss_amd import pose as mpose
    from moss_amd.gaussian_renderer import render
    from tests.test_gpu_lbs import _pipe, _scene
    from tests.test_gpu_pose import K
    from tests.test_lbs_weights_cpu import load_case
    from tests.test_pose_cpu import GOLDEN, HEAD_CASES, head_case
    g = np.load(GOLDEN)
    s, pc, cam, _ = _scene(gpu)
    params = head_case(g, "trained_small", dtype=torch.float32, device=gpu)[0]
    torch.manual_seed(3)
    poses = cam.smpl_param["poses"]
    cam.smpl_param["pose_rotmats"] = mlbs.batch_rodrigues(poses.reshape(24, 3)[1:] + 0.05 * torch.randn(23, 3, device=gpu))
    bg = torch.zeros(3, device=gpu)
    wimg = torch.rand(3, s.camera.H, s.camera.W, device=gpu)
    pc.auto_regression = mpose.head_module().to(gpu)
    pc.auto_regression.load_state_dict({k: v.float() for k, v in params.items()})
    pc.cross_attention_lbs = mlw.lbs_weight_module()
    pc.cross_attention_lbs.load_state_dict({k: v.float() for k, v in load_case("sharp", dtype=torch.float32, device=gpu)[1].items()})
    pc.cross_attention_lbs.to(gpu)
    pc.motion_offset_flag = True

    def run(pipe):
        for p in pc.auto_regression.parameters():
            p.grad = None
        out = render(cam, pc, pipe, bg)
        ((out["render"] * wimg).sum() + 0.06 * out["pose_out"]["nll"].mean()).backward()
        return out["render"].detach().clone(), [p.grad.clone() for p in mpose.head_parameters(pc.auto_regression)]

    flags = dict(lbs_in_op=True, pose_head_in_op=True, lbs_weights_in_op=True)
    img0, grads0 = run(_pipe(**flags))
    img, grads = run(_pipe(smpl_frame_in_op=True, **flags))
    assert float(img0.abs().sum()) > 0
    rel_bar = 2 * K * max(float(g[f"{c}_grad_err32"][i]) / float(np.abs(g[f"{c}_grad_{n}"]).max())
                          for c in HEAD_CASES for i, n in enumerate(mpose.PARAM_NAMES))
    worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(grads, grads0))
    print(f"\nrender with smpl_frame_in_op vs without: image max {float((img - img0).abs().max()):.3g} mean "
          f"{float((img - img0).abs().mean()):.3g}, worst relative parameter-gradient error {worst:.3g} (bar {rel_bar:.3g})")
    assert float((img - img0).abs().max()) < 2 * 2e-3 and float((img - img0).abs().mean()) < 2 * 1e-5
    assert worst < rel_bar


def test_step_with_smpl_frame_in_op_captured_over_frames(gpu, hip_lib):
    """tests/test_gpu_lbs.py's captured multi-frame step with pipe.smpl_frame_in_op on as well: captured once, replayed over four
    frames whose pose parameters are copied into the static inputs; each replay is bit-identical to the eager step of that frame."""
    import moss_amd.diff_gaussian_rasterization as dgr
    from moss_amd.gaussian_renderer import render
    from moss_amd.graphs import GraphedStep
    from moss_amd.loss import backward_from_loss, training_loss_fused
    from tests.test_gpu_lbs import _pipe, _scene, _small_frame
    s, pc, cam, _ = _scene(gpu)
    pipe = _pipe(lbs_in_op=True, transforms_in_op=True, pose_in_op=True, smpl_frame_in_op=True)
    bg = torch.zeros(3, device=gpu)
    gt_img = torch.rand(3, s.camera.H, s.camera.W, device=gpu)
    gt_mask = (torch.rand(1, s.camera.H, s.camera.W, device=gpu) > 0.5).float()
    params = list(pc.parameters())
    grads = [torch.zeros_like(p) for p in params]

    def fn():
        for p, g in zip(params, grads):
            g.zero_()
            p.grad = g
        out = render(cam, pc, pipe, bg)
        loss = training_loss_fused(out["render"], out["render_alpha"], gt_img, gt_mask)
        backward_from_loss(loss)
        return out["render"].detach(), loss.detach()

    ctx = dgr.RasterContext()
    pipe.raster_context = ctx
    ctx.set_async(True)
    try:
        fn()
        step = GraphedStep(fn, warmup=3, context=ctx)
        first = None
        for k in range(4):
            for key, v in _small_frame(k).items():
                cam.smpl_param[key].copy_(v)
            img_g, loss_g = (v.clone() for v in step())
            grads_g = [g.clone() for g in grads]
            torch.cuda.synchronize(gpu)
            img_e, loss_e = (v.clone() for v in fn())
            torch.cuda.synchronize(gpu)
            assert torch.equal(img_g, img_e) and torch.equal(loss_g, loss_e), k
            for i, (a, b) in enumerate(zip(grads_g, grads)):
                assert torch.equal(a, b), (k, i)
            if first is None:
                first = img_g
            else:
                assert not torch.equal(img_g, first)
        dgr.check_async_status(context=ctx)
    finally:
        ctx.set_async(False)
        step = None
