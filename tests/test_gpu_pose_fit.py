"""The pose fit on the device (moss_amd.posefit; C ABI moss_lbs_deform_backward_frame / moss_smpl_frame_backward_pose): the gradients
of ``posed_frame`` to ``poses``, ``R`` and ``Th`` against float64 autograd of ``posed_frame_torch``, an out-of-range id, full writes
and determinism, agreement with the old entry points, capture in a hipGraph, and ``PoseFitter`` end to end on a synthetic avatar.

The bar (the rule of tests/test_gpu_smpl_frame.py, extended):  |err_e| <= 64 eps32 S_e,  S_e the adjoint itself evaluated in float64
with every factor replaced by its absolute value (:func:`abs_terms`), from the cotangents to the element:
    gT' = |gT| + |gp| |x|^T,  gt' = |gt| + |gp|,
    S_Th = sum_i gt'_i,  S_R = sum_i (gT'_i |N_i|^T + gt'_i |n_i|^T),                     N = O3 Q,  n = O3 (d - Q b) + o
    |gM_i| = gT'_i |Q|^T + gt'_i |u|^T,  |gd_i| = |M|^T gt'_i,  |gA_j| = sum_i w_ij [ |R|^T |gM_i|  |  |R|^T gt'_i ],
    |g_feat|, |gGR|, |gGt| and the reverse walk as tests/test_gpu_smpl_frame.py's abs_terms, then
    |g_rot_0| = |gGR_0|,  |g_raw_0| = |g_rot_0|,  |g_raw_j| = (|g_rot_j| + |g_feat_j|) |correct_Rs[j-1]|^T,
    |g_s| = <|G|, |K|>,  |g_c| = <|G|, |K K|>,  |gK| = |sin a| |G| + |1 - cos a| (|G| |K|^T + |K|^T |G|),  |g_k| = sums of its entries,
    |g_a| = |g_s| |cos a| + |g_c| |sin a| + <|g_k|, |r|> / a^2,   S_poses = |g_k| / a + |g_a| |e| / a.
Every forward quantity (Q, M, u, N, n, the chain rotations, K) is the float64 value, taken by its absolute value where it is a factor.
Each test prints the worst ratio of error to bar, and beside it the ratio of the float32 torch form (``posed_frame_torch`` on the same
inputs) to the same bar.
"""
import ctypes
import gc
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from moss_amd import lbs as mlbs
from moss_amd import posefit

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
V = 6890
SIZES = [1, 63, 64, 65, 127, 128, 129, 6890]
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


def make_case(P, J, seed, dev, ids=None):
    """float32 inputs on ``dev``; joints 0 (the root) and 7 have r = 0 exactly, joint 11 has |r| = 3.0 (tests/test_pose_fit_cpu.py)."""
    body = body_of(J, dev)
    fr = mlbs.synthetic_frame(seed, J)
    poses = fr["poses"].reshape(J, 3).clone()
    poses[0] = 0
    poses[7] = 0
    poses[11] = poses[11] / poses[11].norm() * 3.0
    fr["poses"] = poses.reshape(1, 3 * J)
    fr = {k: v.to(dev) for k, v in fr.items()}
    big = {k: v.to(dev) for k, v in mlbs.synthetic_frame(0, J, big_pose=True).items()}
    g = torch.Generator().manual_seed(seed)
    if ids is None:
        ids = torch.randint(0, V, (P,), generator=g)
    x = body["v_template"][ids.clamp(0, V - 1).to(dev)] + 0.03 * torch.randn(P, 3, generator=g).to(dev)
    L = (0.7 * torch.randn(P, J, generator=g)).to(dev)
    cR = mlbs.batch_rodrigues(0.1 * torch.randn(J - 1, 3, generator=g)).to(dev).contiguous()
    cot = [torch.randn(*s, generator=g, dtype=torch.float64).to(dev) for s in ((P, 3, 3), (P, 3), (P, 3))]
    return SimpleNamespace(body=body, fr=fr, big=big, ids=ids.to(dev), x=x.contiguous(), L=L.contiguous(), cR=cR, cot=cot, J=J, P=P)


NAMES = ("poses", "R", "Th")


def grads_of(fn, c, dtype, L, cR, keep=None):
    """d <cot, fn(...)> / d (poses, R, Th) in ``dtype``; ``keep``: a mask of the Gaussians that enter (the others are dropped)."""
    dtype = torch.float32 if dtype is None else dtype
    conv = lambda t: t.to(dtype)                                                        # noqa: E731
    body = {k: (conv(v) if v.is_floating_point() else v) for k, v in c.body.items()}
    fr = {k: conv(v) for k, v in c.fr.items()}
    big = {k: conv(v) for k, v in c.big.items()}
    leaves = {k: fr[k].clone().requires_grad_(True) for k in NAMES}
    sel = slice(None) if keep is None else keep
    out = fn(body, body["weights"], {**fr, **leaves}, big, c.ids[sel], conv(c.x)[sel].contiguous(),
             lbs_offsets=None if L is None else conv(L)[sel].contiguous(), correct_Rs=None if cR is None else conv(cR))
    torch.autograd.backward(list(out), [conv(g)[sel].contiguous() for g in c.cot])
    return {k: leaves[k].grad.reshape(-1) for k in NAMES}


def abs_terms(c, L, cR, keep=None):
    """S of the module docstring, float64: {"poses" (3J), "R" (9), "Th" (3)}."""
    sel = slice(None) if keep is None else keep
    body, fr, big = f64(c.body), f64(c.fr), f64(c.big)
    ids, x = c.ids[sel], c.x.double()[sel]
    gT, gt, gp = (g[sel] for g in c.cot)
    J = c.J
    W = body["weights"]
    par = [int(v) for v in body["kintree_table"][0].tolist()]
    # the forward in float64
    raw = mlbs.batch_rodrigues(fr["poses"].reshape(-1, 3))
    rot = raw if cR is None else torch.cat([raw[:1], raw[1:] @ cR.double()], 0)
    A_big = mlbs.smpl_joint_transforms(body, big)[0][0]
    A_obs = mlbs.smpl_joint_transforms(body, fr, rot_mats=rot)[0][0]
    d = mlbs.vertex_offsets(body, fr, big, rot)[ids]
    w = W[ids]
    if L is not None:
        w = torch.softmax(torch.log(w + 1e-9) + L.double()[sel], -1)
    B = (w @ A_big.reshape(J, 16)).reshape(-1, 4, 4)
    O = (w @ A_obs.reshape(J, 16)).reshape(-1, 4, 4)
    R = fr["R"].reshape(3, 3)
    Q = torch.inverse(B[:, :3, :3])
    O3, o, b = O[:, :3, :3], O[:, :3, 3], B[:, :3, 3]
    M = R @ O3
    u = d - (Q @ b[..., None]).squeeze(-1)
    N = O3 @ Q
    n = (O3 @ u[..., None]).squeeze(-1) + o
    # the per-Gaussian adjoint, every factor by its absolute value
    gTp = gT.abs() + gp.abs()[:, :, None] * x.abs()[:, None, :]
    gtp = gt.abs() + gp.abs()
    S_Th = gtp.sum(0)
    S_R = (gTp @ N.abs().transpose(1, 2) + gtp[:, :, None] * n.abs()[:, None, :]).sum(0)
    gM = gTp @ Q.abs().transpose(1, 2) + gtp[:, :, None] * u.abs()[:, None, :]
    gd = (M.abs().transpose(1, 2) @ gtp[..., None]).squeeze(-1)
    gO = torch.cat([R.abs().T @ gM, (gtp @ R.abs())[..., None]], -1)                 # (P,3,4): [ |R|^T gM | |R|^T gt' ]
    gA = torch.einsum("ij,irc->jrc", w, gO)                                          # (J,3,4)
    # the frame's adjoint (tests/test_gpu_smpl_frame.py's abs_terms, with the root kept)
    vs = body["v_template"] + (body["shapedirs"][..., :fr["shapes"].shape[-1]] * fr["shapes"][0]).sum(-1)
    jt = body["J_regressor"] @ vs
    rel = jt.clone()
    GR = [rot[0]]
    for j in range(1, J):
        rel[j] = jt[j] - jt[par[j]]
        GR.append(GR[par[j]] @ rot[j])
    g_feat = torch.zeros(9 * (J - 1), dtype=torch.float64, device=gd.device)
    apd = body["posedirs"].abs()
    for lo in range(0, ids.shape[0], 4096):
        g_feat += torch.einsum("ick,ic->k", apd[ids[lo:lo + 4096]], gd[lo:lo + 4096])
    gGR = [gA[j, :, :3] + gA[j, :, 3][:, None] * jt[j].abs()[None, :] for j in range(J)]
    gGt = [gA[j, :, 3] for j in range(J)]
    g_rot = [None] * J
    for j in range(J - 1, 0, -1):
        p = par[j]
        g_rot[j] = GR[p].abs().T @ gGR[j] + g_feat[9 * (j - 1):9 * j].reshape(3, 3)
        gGR[p] = gGR[p] + gGR[j] @ rot[j].abs().T + gGt[j][:, None] * rel[j].abs()[None, :]
        gGt[p] = gGt[p] + gGt[j]
    g_rot[0] = gGR[0]
    G = torch.stack([g_rot[0]] + [g_rot[j] if cR is None else g_rot[j] @ cR.double()[j - 1].abs().T for j in range(1, J)])   # |g_raw|
    # the adjoint of Rodrigues
    r = fr["poses"].reshape(J, 3)
    e = r + 1e-8
    a = e.norm(dim=1)
    k = (r / a[:, None]).abs()
    z = torch.zeros_like(a)
    K = torch.stack([z, k[:, 2], k[:, 1], k[:, 2], z, k[:, 0], k[:, 1], k[:, 0], z], 1).reshape(J, 3, 3)                   # |K|
    kv = r / a[:, None]
    KK = (kv[:, :, None] * kv[:, None, :] - (kv * kv).sum(1)[:, None, None] * torch.eye(3, dtype=torch.float64, device=a.device)).abs()
    g_s, g_c = (G * K).sum((1, 2)), (G * KK).sum((1, 2))
    gK = torch.sin(a).abs()[:, None, None] * G + (1 - torch.cos(a)).abs()[:, None, None] * (G @ K.transpose(1, 2) + K.transpose(1, 2) @ G)
    g_k = torch.stack([gK[:, 2, 1] + gK[:, 1, 2], gK[:, 0, 2] + gK[:, 2, 0], gK[:, 1, 0] + gK[:, 0, 1]], 1)
    g_a = g_s * torch.cos(a).abs() + g_c * torch.sin(a).abs() + (g_k * r.abs()).sum(1) / (a * a)
    S_poses = g_k / a[:, None] + g_a[:, None] * e.abs() / a[:, None]
    return {"poses": S_poses.reshape(-1), "R": S_R.reshape(-1), "Th": S_Th}


def ratios(got, ref, S):
    return {k: float(((got[k].double() - ref[k]).abs() / (64.0 * EPS32 * S[k])).max()) for k in NAMES}


@pytest.mark.parametrize("J", [24, 55])
@pytest.mark.parametrize("P", SIZES)
def test_gradients_match_float64_autograd(gpu, hip_lib, P, J):
    """posed_frame's gradients of poses, R and Th against float64 autograd of posed_frame_torch under random cotangents g_T, g_t, g_p;
    with and without correct_Rs and lbs_offsets; the workgroup edges of both backward reductions (128 and 64 Gaussians)."""
    c = make_case(P, J, 400 + P % 83 + J, gpu)
    worst, worst32 = {}, {}
    for with_cR in (True, False):
        for with_L in (True, False):
            L, cR = (c.L if with_L else None), (c.cR if with_cR else None)
            got = grads_of(posefit.posed_frame, c, None, L, cR)
            ref = grads_of(posefit.posed_frame_torch, c, torch.float64, L, cR)
            t32 = grads_of(posefit.posed_frame_torch, c, None, L, cR)
            S = abs_terms(c, L, cR)
            for k, v in ratios(got, ref, S).items():
                worst[k] = max(worst.get(k, 0.0), v)
            for k, v in ratios(t32, ref, S).items():
                worst32[k] = max(worst32.get(k, 0.0), v)
            assert all(bool(torch.isfinite(got[k]).all()) for k in NAMES)
    print(f"\nP={P} J={J}: worst error / bar: fused " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items())
          + "; float32 torch form " + ", ".join(f"{k} {v:.3g}" for k, v in worst32.items()))
    assert max(worst.values()) < 1.0, worst


def test_out_of_range_id_adds_nothing(gpu, hip_lib):
    """P = 65 with one id = V: g_poses, g_R and g_Th are the float64 result with that row dropped, within the bar; no NaN."""
    P, J = 65, 24
    ids = torch.randint(0, V, (P,), generator=torch.Generator().manual_seed(3))
    ids[17] = V
    c = make_case(P, J, 431, gpu, ids=ids)
    keep = torch.ones(P, dtype=torch.bool, device=gpu)
    keep[17] = False
    got = grads_of(posefit.posed_frame, c, None, c.L, c.cR)
    ref = grads_of(posefit.posed_frame_torch, c, torch.float64, c.L, c.cR, keep=keep)
    r = ratios(got, ref, abs_terms(c, c.L, c.cR, keep=keep))
    print("\nout-of-range id: worst error / bar " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert all(bool(torch.isfinite(got[k]).all()) for k in NAMES) and max(r.values()) < 1.0, r
    fr = {**c.fr, **{k: c.fr[k].clone().requires_grad_(True) for k in NAMES}}
    T, t, p = posefit.posed_frame(c.body, c.body["weights"], fr, c.big, c.ids, c.x, lbs_offsets=c.L, correct_Rs=c.cR)
    assert bool(torch.isnan(T[17]).all()) and bool(torch.isfinite(T[keep]).all()) and bool(torch.isfinite(p[keep]).all())


# ---- through the C ABI ------------------------------------------------------------------------------------------------------------

def _parents_of(body):
    return [-1] + [int(v) for v in body["kintree_table"][0].tolist()][1:]


def c_forward(c, gpu):
    """Both forwards through the C ABI: A_big, A_obs, d, saved."""
    from moss_amd._lib import SMPL_FRAME_SAVED_FLOATS_PER_JOINT, SmplFrameArgs, call, lib
    J, P, body = c.J, c.P, c.body
    A_big, A_obs = torch.empty(J, 4, 4, device=gpu), torch.empty(J, 4, 4, device=gpu)
    d, rot, saved = torch.empty(P, 3, device=gpu), torch.empty(J, 3, 3, device=gpu), torch.empty(SMPL_FRAME_SAVED_FLOATS_PER_JOINT * J, device=gpu)
    nbytes = int(lib().moss_smpl_frame_workspace_bytes(P, V, J))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    f = SmplFrameArgs()
    f.P, f.V, f.J, f.num_betas_big, f.num_betas, f.shapedirs_stride = P, V, J, 10, 10, 10
    f.parents[:J] = _parents_of(body)
    f.v_template, f.shapedirs, f.posedirs, f.J_regressor = (body[k].data_ptr() for k in ("v_template", "shapedirs", "posedirs", "J_regressor"))
    f.poses_big, f.shapes_big, f.poses, f.shapes = (c.big["poses"].data_ptr(), c.big["shapes"].data_ptr(), c.fr["poses"].data_ptr(),
                                                    c.fr["shapes"].data_ptr())
    f.correct_Rs, f.vert_ids = c.cR.data_ptr(), c.ids.data_ptr()
    f.A_big, f.A_obs, f.d, f.rot_mats, f.saved = A_big.data_ptr(), A_obs.data_ptr(), d.data_ptr(), rot.data_ptr(), saved.data_ptr()
    f.workspace, f.workspace_bytes = ws.data_ptr(), nbytes
    call("moss_smpl_frame_forward", gpu, ctypes.byref(f))
    return A_big, A_obs, d, saved


def c_backward(c, gpu, fwd, new, fill=float("nan")):
    """The two backward entries through the C ABI (``new``: the frame / pose entries, else the old ones) on outputs and workspaces
    pre-filled with ``fill``: {name: tensor}."""
    from moss_amd import _lib
    lib, call = _lib.lib(), _lib.call
    J, P, body = c.J, c.P, c.body
    A_big, A_obs, d, saved = fwd
    full = lambda *s: torch.full(s, fill, device=gpu)                                   # noqa: E731
    out = {"g_L": full(P, J), "g_A_obs": full(J, 4, 4), "g_d": full(P, 3), "g_x": full(P, 3), "g_correct_Rs": full(J - 1, 3, 3)}
    gT, gt, gp = (g.float().contiguous() for g in c.cot)
    a = (_lib.LbsBackwardFrameArgs if new else _lib.LbsBackwardArgs)()
    a.P, a.J, a.V = P, J, V
    a.vert_ids, a.weights, a.lbs_offsets = c.ids.data_ptr(), body["weights"].data_ptr(), c.L.data_ptr()
    a.A_big, a.A_obs, a.d, a.R, a.Th, a.x = (A_big.data_ptr(), A_obs.data_ptr(), d.data_ptr(), c.fr["R"].data_ptr(), c.fr["Th"].data_ptr(),
                                             c.x.data_ptr())
    a.g_T, a.g_t, a.g_p = gT.data_ptr(), gt.data_ptr(), gp.data_ptr()
    a.g_L, a.g_A_obs, a.g_d, a.g_x = (out[k].data_ptr() for k in ("g_L", "g_A_obs", "g_d", "g_x"))
    nbytes = int((lib.moss_lbs_frame_workspace_bytes if new else lib.moss_lbs_workspace_bytes)(P, J))
    ws = torch.full((nbytes // 4,), fill, device=gpu)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    if new:
        out.update(g_R=full(3, 3), g_Th=full(3), g_poses=full(3 * J))
        a.g_R, a.g_Th = out["g_R"].data_ptr(), out["g_Th"].data_ptr()
    call("moss_lbs_deform_backward_frame" if new else "moss_lbs_deform_backward", gpu, ctypes.byref(a))
    b = (_lib.SmplFrameBackwardPoseArgs if new else _lib.SmplFrameBackwardArgs)()
    b.P, b.V, b.J = P, V, J
    b.parents[:J] = _parents_of(body)
    b.posedirs, b.vert_ids, b.saved = body["posedirs"].data_ptr(), c.ids.data_ptr(), saved.data_ptr()
    b.g_A_obs, b.g_d, b.g_correct_Rs = out["g_A_obs"].data_ptr(), out["g_d"].data_ptr(), out["g_correct_Rs"].data_ptr()
    nbytes2 = int(lib.moss_smpl_frame_workspace_bytes(P, V, J))
    ws2 = torch.full((nbytes2 // 4,), fill, device=gpu)
    b.workspace, b.workspace_bytes = ws2.data_ptr(), nbytes2
    if new:
        b.poses, b.correct_Rs, b.g_poses = c.fr["poses"].data_ptr(), c.cR.data_ptr(), out["g_poses"].data_ptr()
    call("moss_smpl_frame_backward_pose" if new else "moss_smpl_frame_backward", gpu, ctypes.byref(b))
    return out


@pytest.mark.parametrize("P", [129, 6890])
def test_every_element_written_and_deterministic(gpu, hip_lib, P):
    """Outputs and workspaces start as NaN bit patterns: every element of g_poses (3J), g_R and g_Th comes back written; a second run
    is bit-identical, and so is the autograd path."""
    c = make_case(P, 24, 440 + P % 7, gpu)
    fwd = c_forward(c, gpu)
    one = c_backward(c, gpu, fwd, new=True)
    two = c_backward(c, gpu, fwd, new=True)
    for k in ("g_poses", "g_R", "g_Th", "g_A_obs", "g_d", "g_correct_Rs"):
        assert bool(torch.isfinite(one[k]).all()), k
        assert torch.equal(one[k], two[k]), k
    assert tuple(one["g_poses"].shape) == (72,) and float(one["g_poses"].abs().min()) > 0
    got = grads_of(posefit.posed_frame, c, None, c.L, c.cR)
    assert torch.equal(got["poses"], one["g_poses"]) and torch.equal(got["R"], one["g_R"].reshape(-1)) and torch.equal(got["Th"], one["g_Th"])


def test_existing_outputs_equal_the_old_entries(gpu, hip_lib):
    """g_L, g_A_obs, g_d, g_x and g_correct_Rs requested through the new entries equal the old entries' bit for bit (P = 129, J = 24)."""
    c = make_case(129, 24, 450, gpu)
    fwd = c_forward(c, gpu)
    old, new = c_backward(c, gpu, fwd, new=False), c_backward(c, gpu, fwd, new=True)
    for k in ("g_L", "g_A_obs", "g_d", "g_x", "g_correct_Rs"):
        assert bool(torch.isfinite(old[k]).all()) and torch.equal(old[k], new[k]), k


def test_captured_replays_new_frames(gpu, hip_lib):
    """posed_frame forward + backward captured once, replayed three times, each after a copy_ of a new frame's poses, R (from a new
    Rh, in torch) and Th into the static leaves: every replay equals the eager call bit for bit."""
    from moss_amd.graphs import GraphedStep
    P, J = 6890, 24
    c = make_case(P, J, 460, gpu)
    leaves = {k: c.fr[k].clone().requires_grad_(True) for k in NAMES}
    cot = [g.float().contiguous() for g in c.cot]

    def fn():
        for v in leaves.values():
            v.grad = None
        out = posefit.posed_frame(c.body, c.body["weights"], {**c.fr, **leaves}, c.big, c.ids, c.x, lbs_offsets=c.L, correct_Rs=c.cR)
        torch.autograd.backward(list(out), cot)
        return [o.detach() for o in out] + [leaves[k].grad for k in NAMES]

    fn()                                                          # (the parent table is read on the host here, outside the capture)
    step = GraphedStep(fn, warmup=2)
    first = None
    for k in range(3):
        g = torch.Generator().manual_seed(470 + k)
        with torch.no_grad():
            leaves["poses"].copy_((0.3 * torch.randn(1, 3 * J, generator=g)).to(gpu))
            leaves["R"].copy_(mlbs.batch_rodrigues(torch.randn(1, 3, generator=g))[0].to(gpu))
            leaves["Th"].copy_(torch.randn(1, 3, generator=g).to(gpu))
        got = [v.clone() for v in step()]
        torch.cuda.synchronize(gpu)
        ref = [v.clone() for v in fn()]
        for i, (u, v) in enumerate(zip(got, ref)):
            assert torch.equal(u, v), (k, i)
        if first is None:
            first = got
        else:
            assert not torch.equal(got[0], first[0]) and not torch.equal(got[3], first[3])


# ---- end to end --------------------------------------------------------------------------------------------------------------------

def _avatar(gpu):
    """A small synthetic avatar built as tests/test_gpu_moss_step.py's ``world`` builds its model: body_scene Gaussians (P = 6 890), a
    synthetic body of V = 6 890 vertices, the fixture networks; one 128 x 128 camera."""
    from moss_amd import lbs_weights as mlw
    from moss_amd import pose as mpose
    from moss_amd import scenes
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import camera_view
    from moss_amd.knn_cuda import KNN
    from tests.test_gpu_lbs import _small_frame
    from tests.test_lbs_weights_cpu import load_case
    from tests.test_pose_cpu import GOLDEN, head_case
    s = scenes.body_scene(6890, 128, 128, 135.0, init_like=False, principal_offset=(3.0, -2.0), name="posefit")
    pc = GaussianSet(s, device=gpu, unified_features=True)
    body = mlbs.synthetic_body_model(V, 24, seed=21, device=gpu)
    pc.SMPL_NEUTRAL, pc.knn = body, KNN(k=1, transpose_mode=True)
    params = head_case(np.load(GOLDEN), "trained_small", dtype=torch.float32, device=gpu)[0]
    pc.auto_regression = mpose.head_module().to(gpu)
    pc.auto_regression.load_state_dict({k: v.float() for k, v in params.items()})
    pc.cross_attention_lbs = mlw.lbs_weight_module()
    pc.cross_attention_lbs.load_state_dict({k: v.float() for k, v in load_case("sharp", dtype=torch.float32, device=gpu)[1].items()})
    pc.cross_attention_lbs.to(gpu)
    pc.motion_offset_flag = True
    cam = camera_view(s.camera, gpu)
    cam.big_pose_smpl_param = {k: v.to(gpu) for k, v in mlbs.synthetic_frame(0, 24, big_pose=True).items()}
    cam.big_pose_world_vertex = body["v_template"].clone()
    truth = {k: v.to(gpu) for k, v in _small_frame(0).items()}
    truth["pose_rotmats"] = mlbs.batch_rodrigues(truth["poses"].reshape(24, 3))[1:].contiguous()
    cam.smpl_param = {k: v.clone() for k, v in truth.items()}
    return pc, cam, truth


def test_fit_descends_to_the_avatars_own_render(gpu, hip_lib):
    """The target is the avatar's own render at theta*, so the loss has its minimum, 0, at the truth.  Start: Th off by
    (0.02, -0.01, 0.015) m and three non-root joints off by 0.1 rad; 40 steps at lr 1e-3.  The loss after the last step is below the
    loss at step 0, |Th - Th*| is below its starting value, no model parameter's bits changed, and with capture=True the 40 losses
    equal the eager run's bit for bit.  Then player.frame(camera, fitted) renders the fitted pose."""
    from moss_amd.loss import ViewRegion
    from moss_amd.play import MossPlayer
    pc, cam, truth = _avatar(gpu)
    bg = torch.zeros(3, device=gpu)
    player = MossPlayer(pc, cam, bg)
    target = player.frame(cam, truth)
    gt, mask = target["render"].clone(), target["render_alpha"].clone()
    assert float(gt.abs().max()) > 0.1
    region = ViewRegion(torch.ones(1, 128, 128, device=gpu))
    start = {k: v.clone() for k, v in truth.items()}
    start["Th"] = truth["Th"] + torch.tensor([[0.02, -0.01, 0.015]], device=gpu)
    poses = truth["poses"].clone().reshape(24, 3)
    for j, axis in ((4, 0), (13, 1), (18, 2)):
        poses[j, axis] += 0.1
    start["poses"] = poses.reshape(1, 72)
    before = [p.detach().clone() for p in pc.parameters()]
    fitted, losses = posefit.PoseFitter(pc, cam, bg, lr=1e-3).fit(cam, (gt, mask), region, start, 40)
    fitted_g, losses_g = posefit.PoseFitter(pc, cam, bg, lr=1e-3, capture=True).fit(cam, (gt, mask), region, start, 40)
    losses, losses_g = losses.cpu(), losses_g.cpu()
    th0 = float((start["Th"] - truth["Th"]).norm())
    th1 = float((fitted["Th"] - truth["Th"]).norm())
    pose0 = float((start["poses"] - truth["poses"]).abs().max())
    pose1 = float((fitted["poses"] - truth["poses"]).abs().max())
    print(f"\nfit: loss {float(losses[0]):.6g} -> {float(losses[-1]):.6g} (ratio {float(losses[-1] / losses[0]):.3g}); |Th - Th*| {th0:.4g} -> "
          f"{th1:.4g} m; max |poses - poses*| {pose0:.4g} -> {pose1:.4g} rad")
    assert tuple(losses.shape) == (40,) and bool(torch.isfinite(losses).all())
    assert float(losses[-1]) < float(losses[0])
    assert th1 < th0
    for p, b in zip(pc.parameters(), before):
        assert torch.equal(p.detach(), b) and p.grad is None
    assert torch.equal(losses, losses_g)
    for k in ("poses", "Rh", "R", "Th"):
        assert torch.equal(fitted[k], fitted_g[k]), k
    again = player.frame(cam, fitted)["render"]
    assert bool(torch.isfinite(again).all()) and float(again.abs().max()) > 0.1
