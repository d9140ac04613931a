"""The keypoint fit on the device (moss_amd.keypoints; C ABI moss_smpl_vertices_backward / moss_keypoint_loss): the gradients of
``posed_vertices_fn`` to ``poses``, ``R`` and ``Th`` against float64 autograd of ``bounds.posed_vertices_torch``, the loss op against
``keypoint_loss_torch`` in float64, full writes, determinism, poisoned memory, capture, and ``PoseFitter`` with keypoints.

The bar is the rule of tests/test_gpu_pose_fit.py:  |err_e| <= 64 eps32 S_e,  S_e the adjoint itself evaluated in float64 with every
factor and term replaced by its absolute value.  That file's ``abs_terms`` is one function from the per-Gaussian cotangents to the
element, so what it offers apart is ``EPS32``, ``f64`` and ``_avatar``; the chain's reverse walk and the Rodrigues part are written
here as they are there (:func:`chain_abs`, :func:`rodrigues_abs`), and the vertex part the same way (:func:`abs_terms_vertices`):
    h'_v = |R|^T |g_v|,  S_Th = sum_v |g_v|,  S_R = sum_v |g_v| |y_v|^T,
    |gA_j| = sum_v w_vj h'_v [ |v_posed_v|^T  1 ],  |g_vposed_v| = |T_v[:3,:3]|^T h'_v,  |g_feat| = sum_v sum_c |posedirs[v,c,:]| |g_vposed_vc|,
    |gGR_j| = |gA_j[:3,:3]| + |gA_j[:3,3]| |joint_j|^T,  |gGt_j| = |gA_j[:3,3]|,  then the walk and Rodrigues with correct_Rs = I.
The loss (:func:`abs_terms_loss`): X'_k = sum_v |regressor_kv| |world_v|,  cam' = |RT[:, :3]| X' + |RT[:, 3]|,  uvw' = |K| cam',
u' = uvw'_xy / uvw_z (the divisor and the robustifier's denominators keep their float64 value: the cameras see every keypoint at
uvw_z >= 0.5),  d' = u' + |uv|  (u - uv counts as |u| + |uv|),  r2' = |d'|^2,  rho' = s^2 r2' / (s^2 + r2) (r2' without s),
S_loss = the loss of rho';  g_u' = 2 conf (d rho / d r2) d',  g_uvw' = (g_u'_x / z, g_u'_y / z, (g_u'_x u'_x + g_u'_y u'_y) / z),
g_X' = weight2d / (C Kp) sum_c |RT[:, :3]|^T |K|^T g_uvw' + weight3d / Kp 2 conf3 (d rho / d r2) (X' + |xyz|),
S_g = |regressor|^T g_X'.
Each test prints the worst ratio of error to bar, and beside it the ratio of the float32 torch form on the same inputs.
"""
import ctypes
import gc

import pytest
import torch

from moss_amd import bounds as mb
from moss_amd import keypoints as kp
from moss_amd import lbs as mlbs
from tests.test_gpu_poisoned_memory import under_fills
from tests.test_gpu_pose_fit import EPS32, _avatar, f64
from tests.test_keypoints_cpu import cameras, targets_for

pytestmark = pytest.mark.gpu

NAMES = ("poses", "R", "Th")
BAR = 64.0 * EPS32
_BODIES = {}


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    yield
    _BODIES.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch._C._cuda_clearCublasWorkspaces()
    torch.cuda.empty_cache()


def body_of(V, J, dev):
    if (V, J) not in _BODIES:
        _BODIES[(V, J)] = {k: v.to(dev) for k, v in mlbs.synthetic_body_model(V, J, seed=60 + J).items()}
    return _BODIES[(V, J)]


def frame_of(seed, J, dev):
    """A synthetic frame; with J >= 12 the root and joint 7 have r = 0 exactly and joint 11 has |r| = 3."""
    fr = mlbs.synthetic_frame(seed, J)
    if J >= 12:
        poses = fr["poses"].reshape(J, 3).clone()
        poses[0] = 0
        poses[7] = 0
        poses[11] = poses[11] / poses[11].norm() * 3.0
        fr["poses"] = poses.reshape(1, 3 * J)
    return {k: v.to(dev).contiguous() for k, v in fr.items()}


# ---- the bars ----------------------------------------------------------------------------------------------------------------------

def chain_abs(gA, g_feat, rot, jt, par):
    """|g_raw| (J,3,3) of |gA| (J,3,4) and |g_feat|: the reverse walk of tests/test_gpu_pose_fit.py's abs_terms, correct_Rs = I."""
    J = rot.shape[0]
    rel = jt.clone()
    GR = [rot[0]]
    for j in range(1, J):
        rel[j] = jt[j] - jt[par[j]]
        GR.append(GR[par[j]] @ rot[j])
    gGR = [gA[j, :, :3] + gA[j, :, 3][:, None] * jt[j].abs()[None, :] for j in range(J)]
    gGt = [gA[j, :, 3] for j in range(J)]
    g_rot = [None] * J
    for j in range(J - 1, 0, -1):
        p = par[j]
        g_rot[j] = GR[p].abs().T @ gGR[j] + g_feat[9 * (j - 1):9 * j].reshape(3, 3)
        gGR[p] = gGR[p] + gGR[j] @ rot[j].abs().T + gGt[j][:, None] * rel[j].abs()[None, :]
        gGt[p] = gGt[p] + gGt[j]
    g_rot[0] = gGR[0]
    return torch.stack(g_rot)


def rodrigues_abs(G, r):
    """S_poses (J,3) of |g_raw| (J,3,3) at the axis-angles r (J,3): the Rodrigues part of tests/test_gpu_pose_fit.py's abs_terms."""
    J = r.shape[0]
    e = r + 1e-8
    a = e.norm(dim=1)
    kv = r / a[:, None]
    k = kv.abs()
    z = torch.zeros_like(a)
    K = torch.stack([z, k[:, 2], k[:, 1], k[:, 2], z, k[:, 0], k[:, 1], k[:, 0], z], 1).reshape(J, 3, 3)
    KK = (kv[:, :, None] * kv[:, None, :] - (kv * kv).sum(1)[:, None, None] * torch.eye(3, dtype=r.dtype, device=r.device)).abs()
    g_s, g_c = (G * K).sum((1, 2)), (G * KK).sum((1, 2))
    gK = torch.sin(a).abs()[:, None, None] * G + (1 - torch.cos(a)).abs()[:, None, None] * (G @ K.transpose(1, 2) + K.transpose(1, 2) @ G)
    g_k = torch.stack([gK[:, 2, 1] + gK[:, 1, 2], gK[:, 0, 2] + gK[:, 2, 0], gK[:, 1, 0] + gK[:, 0, 1]], 1)
    g_a = g_s * torch.cos(a).abs() + g_c * torch.sin(a).abs() + (g_k * r.abs()).sum(1) / (a * a)
    return g_k / a[:, None] + g_a[:, None] * e.abs() / a[:, None]


def abs_terms_vertices(body, fr, g):
    """S of the module docstring for the vertex backward, float64: {"poses" (3J), "R" (9), "Th" (3)}."""
    body, fr, g = f64(body), f64(fr), g.double().abs()
    W = body["weights"]
    V, J = W.shape
    par = [int(v) for v in body["kintree_table"][0].tolist()]
    rot = mlbs.batch_rodrigues(fr["poses"].reshape(-1, 3))
    vs = body["v_template"] + (body["shapedirs"][..., :fr["shapes"].shape[-1]] * fr["shapes"][0]).sum(-1)
    jt = body["J_regressor"] @ vs
    vposed = vs
    if J > 1:
        feat = (rot[1:] - torch.eye(3, dtype=torch.float64, device=g.device)).reshape(-1)
        vposed = vs + (body["posedirs"].reshape(V * 3, -1) @ feat).reshape(V, 3)
    A = mlbs.smpl_joint_transforms(body, fr, rot_mats=rot)[0][0][:, :3, :]             # (J,3,4)
    T = (W @ A.reshape(J, 12)).reshape(V, 3, 4)
    y = (T[:, :, :3] @ vposed[..., None]).squeeze(-1) + T[:, :, 3]
    R = fr["R"].reshape(3, 3)
    h = g @ R.abs()                                                                    # |R|^T |g|
    S_Th = g.sum(0)
    S_R = (g[:, :, None] * y.abs()[:, None, :]).sum(0)
    gA = torch.einsum("vj,vr,vc->jrc", W, h, torch.cat([vposed.abs(), torch.ones(V, 1, dtype=torch.float64, device=g.device)], 1))
    gvp = torch.einsum("vrc,vr->vc", T[:, :, :3].abs(), h)
    g_feat = torch.einsum("vck,vc->k", body["posedirs"].abs(), gvp) if J > 1 else torch.zeros(0, dtype=torch.float64, device=g.device)
    G = chain_abs(gA, g_feat, rot, jt, par)
    return {"poses": rodrigues_abs(G, fr["poses"].reshape(J, 3)).reshape(-1), "R": S_R.reshape(-1), "Th": S_Th}


def _rho_terms(r2_abs, r2, sigma):
    """(rho', d rho / d r2) with the denominators at their float64 value."""
    if sigma <= 0:
        return r2_abs, torch.ones_like(r2)
    s2 = sigma * sigma
    return s2 * r2_abs / (s2 + r2), (s2 / (s2 + r2)) ** 2


def abs_terms_loss(world, tg, drop=None):
    """(S_loss, S_g (V,3)) of the module docstring, float64, on ``world``'s device.  ``drop`` (C,Kp) bool: 2D entries that are left out
    (behind their camera)."""
    w = world.double()
    d = lambda t: t.double().to(w.device)                                                # noqa: E731
    reg = d(tg.regressor)
    X, Xa = reg @ w, reg.abs() @ w.abs()
    S, gX = w.new_zeros(()), torch.zeros_like(X)
    if tg.C:
        K, RT, uv, conf = d(tg.K), d(tg.RT), d(tg.uv), d(tg.conf)
        u, z = kp.project_torch(X, K, RT)
        if drop is not None:
            conf, z = conf * ~drop, torch.where(drop, torch.ones_like(z), z)
        assert float(z.min()) >= 0.5
        cam_a = torch.einsum("crq,nq->cnr", RT[:, :, :3].abs(), Xa) + RT[:, None, :, 3].abs()
        uvw_a = torch.einsum("crq,cnq->cnr", K.abs(), cam_a)
        ua = uvw_a[..., :2] / z[..., None]
        da = ua + uv.abs()
        rho, drho = _rho_terms((da ** 2).sum(-1), ((u - uv) ** 2).sum(-1), tg.sigma)
        S = S + tg.weight2d / (tg.C * tg.Kp) * (conf * rho).sum()
        gu = 2 * (conf * drho)[..., None] * da
        guvw = torch.cat([gu / z[..., None], ((gu * ua).sum(-1) / z)[..., None]], -1)
        gcam = torch.einsum("crq,cnr->cnq", K.abs(), guvw)
        gX = gX + tg.weight2d / (tg.C * tg.Kp) * torch.einsum("crq,cnr->nq", RT[:, :, :3].abs(), gcam)
    if tg.has3d:
        xyz, conf3 = d(tg.xyz), d(tg.conf3)
        da = Xa + xyz.abs()
        rho, drho = _rho_terms((da ** 2).sum(-1), ((X - xyz) ** 2).sum(-1), tg.sigma3)
        S = S + tg.weight3d / tg.Kp * (conf3 * rho).sum()
        gX = gX + tg.weight3d / tg.Kp * 2 * (conf3 * drho)[:, None] * da
    return S, reg.abs().T @ gX


# ---- the vertex backward ---------------------------------------------------------------------------------------------------------------

def vertex_grads(fn, body, fr, g, dtype):
    conv = lambda t: t.to(dtype) if t.is_floating_point() else t                        # noqa: E731
    body, fr = {k: conv(v) for k, v in body.items()}, {k: conv(v) for k, v in fr.items()}
    leaves = {k: fr[k].clone().requires_grad_(True) for k in NAMES}
    world = fn(body, {**fr, **leaves})
    world.backward(conv(g))
    return {k: leaves[k].grad.reshape(-1) for k in NAMES}, world.detach()


def _torch_vertices(body, params):
    return mb.posed_vertices_torch(body, params, 0.0)[0]


def ratios(got, ref, S):
    return {k: float(((got[k].double() - ref[k]).abs() / (BAR * S[k])).max()) for k in NAMES}


@pytest.mark.parametrize("J", [1, 2, 24, 55])
@pytest.mark.parametrize("V", [1, 15, 17, 31, 33, 255, 257, 6890])
def test_vertex_gradients_match_float64_autograd(gpu, hip_lib, V, J):
    """g_poses, g_R and g_Th of a random g_world_vertex against float64 autograd of posed_vertices_torch; V at the edges of the three
    kernels' runs of vertices (16, 32, 256) and at SMPL's size; J = 1 (no posedirs), 2, SMPL's, SMPL-X's; r = 0 and |r| = 3 at J >= 12."""
    body, fr = body_of(V, J, gpu), frame_of(600 + V % 89 + J, J, gpu)
    g = torch.randn(V, 3, generator=torch.Generator().manual_seed(V + J)).to(gpu)
    got, world = vertex_grads(kp.posed_vertices_fn, body, fr, g, torch.float32)
    ref, _ = vertex_grads(_torch_vertices, body, fr, g, torch.float64)
    t32, _ = vertex_grads(_torch_vertices, body, fr, g, torch.float32)
    S = abs_terms_vertices(body, fr, g)
    if V == 1 and J == 1:                                           # (the vertex is its own joint: poses has no gradient, S_poses > 0 still)
        assert float(ref["poses"].abs().max()) < 1e-12
    r, r32 = ratios(got, ref, S), ratios(t32, ref, S)
    print(f"\nV={V} J={J}: worst error / bar: fused " + ", ".join(f"{k} {v:.3g}" for k, v in r.items())
          + "; float32 torch form " + ", ".join(f"{k} {v:.3g}" for k, v in r32.items()))
    assert all(bool(torch.isfinite(got[k]).all()) for k in NAMES)
    assert max(r.values()) < 1.0, r
    assert torch.equal(world, mb.posed_vertices(body, fr)[0])       # the forward is bounds.posed_vertices, bit for bit


def c_vertices_backward(body, fr, g, gpu, fill=float("nan")):
    """``moss_smpl_vertices_backward`` through the C ABI on outputs and a workspace pre-filled with ``fill``."""
    from moss_amd import _lib
    V, J = (int(s) for s in body["weights"].shape)
    out = {"g_poses": torch.full((3 * J,), fill, device=gpu), "g_R": torch.full((3, 3), fill, device=gpu), "g_Th": torch.full((3,), fill, device=gpu)}
    nbytes = int(_lib.lib().moss_smpl_vertices_backward_workspace_bytes(V, J))
    ws = torch.full((nbytes // 4,), fill, device=gpu)
    a = _lib.SmplVerticesBackwardArgs()
    a.V, a.J, a.num_betas, a.shapedirs_stride = V, J, 10, 10
    a.parents[:J] = [-1] + [int(v) for v in body["kintree_table"][0].tolist()][1:]
    for k in ("v_template", "shapedirs", "J_regressor", "weights"):
        setattr(a, k, body[k].data_ptr())
    a.posedirs = body["posedirs"].data_ptr() if J > 1 else None
    a.poses, a.shapes, a.R, a.Th = (fr[k].data_ptr() for k in ("poses", "shapes", "R", "Th"))
    a.g_world_vertex = g.data_ptr()
    a.g_poses, a.g_R, a.g_Th = (out[k].data_ptr() for k in ("g_poses", "g_R", "g_Th"))
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    _lib.call("moss_smpl_vertices_backward", gpu, ctypes.byref(a))
    return out


def c_keypoint_loss(world, tg, gpu, fill=float("nan"), keypoints=True):
    """``moss_keypoint_loss`` through the C ABI on outputs and a workspace pre-filled with ``fill`` (flags: -1)."""
    from moss_amd import _lib
    out = {"loss": torch.full((1,), fill, device=gpu), "g_world_vertex": torch.full((tg.V, 3), fill, device=gpu),
           "keypoints": torch.full((tg.Kp, 3), fill, device=gpu), "flags": torch.full((tg.C,), -1, dtype=torch.int32, device=gpu)}
    nbytes = int(_lib.lib().moss_keypoint_loss_workspace_bytes(tg.C, tg.Kp))
    ws = torch.full((nbytes // 4,), fill, device=gpu)
    a = _lib.KeypointLossArgs()
    a.V, a.Kp, a.C = tg.V, tg.Kp, tg.C
    a.world_vertex, a.regressor = world.data_ptr(), tg.regressor.data_ptr()
    a.K, a.RT, a.uv, a.conf, a.xyz, a.conf3 = (_lib.ptr(getattr(tg, k)) for k in ("K", "RT", "uv", "conf", "xyz", "conf3"))
    a.sigma, a.sigma3, a.weight2d, a.weight3d = tg.sigma, tg.sigma3, tg.weight2d, tg.weight3d
    a.loss, a.g_world_vertex = out["loss"].data_ptr(), out["g_world_vertex"].data_ptr()
    a.keypoints = out["keypoints"].data_ptr() if keypoints else None
    a.flags = out["flags"].data_ptr() if tg.C else None
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    _lib.call("moss_keypoint_loss", gpu, ctypes.byref(a))
    return out


def on(tg, dev):
    return kp.KeypointTargets(*(None if getattr(tg, k) is None else getattr(tg, k).to(dev) for k in tg.TENSORS),
                              **{k: getattr(tg, k) for k in tg.SCALARS})


@pytest.mark.parametrize("V,J", [(257, 24), (6890, 24), (33, 1)])
def test_vertex_backward_writes_every_element_and_is_deterministic(gpu, hip_lib, V, J):
    """Outputs and the workspace start as NaN bit patterns: every element comes back written; a second run and the autograd path are
    bit-identical; a zero g_world_vertex gives exact zeros."""
    body, fr = body_of(V, J, gpu), frame_of(700 + V, J, gpu)
    g = torch.randn(V, 3, generator=torch.Generator().manual_seed(V)).to(gpu)
    one, two = c_vertices_backward(body, fr, g, gpu), c_vertices_backward(body, fr, g, gpu)
    got, _ = vertex_grads(kp.posed_vertices_fn, body, fr, g, torch.float32)
    for k, name in (("g_poses", "poses"), ("g_R", "R"), ("g_Th", "Th")):
        assert bool(torch.isfinite(one[k]).all()), k
        assert torch.equal(one[k], two[k]) and torch.equal(one[k].reshape(-1), got[name]), k
    zero = c_vertices_backward(body, fr, torch.zeros_like(g), gpu)
    for k, v in zero.items():
        assert bool((v == 0).all()), k


# ---- the loss op --------------------------------------------------------------------------------------------------------------------

LOSS_CASES = [(V, C, Kp, parts, robust)
              for V, C, Kp in [(257, 1, 1), (257, 1, 25), (257, 1, 128), (257, 3, 1), (257, 3, 25), (255, 3, 128), (6890, 3, 25)]
              for parts in ("2d", "both") for robust in (True, False)] \
           + [(V, 0, Kp, "3d", robust) for V, Kp in [(257, 1), (256, 25), (6890, 128)] for robust in (True, False)]


def loss_and_grad(fn, world, tg, dtype):
    w = world.to(dtype).clone().requires_grad_(True)
    loss = fn(w, tg)
    loss.backward()
    return loss.detach(), w.grad


@pytest.mark.parametrize("V,C,Kp,parts,robust", LOSS_CASES)
def test_loss_matches_float64(gpu, hip_lib, V, C, Kp, parts, robust):
    """The value and g_world_vertex against keypoint_loss_torch in float64 on the same float32 inputs: 2D only, 3D only, both; with and
    without the robustifier; some conf = 0; V at the scatter kernel's block edge; every keypoint at uvw_z >= 0.5."""
    world = (0.5 * torch.randn(V, 3, generator=torch.Generator().manual_seed(V + Kp))).to(gpu)
    tg = on(targets_for(world.cpu(), Kp, C, 800 + V % 7 + Kp + C, parts=parts, sigma=30.0 if robust else 0.0,
                        sigma3=0.1 if robust else -1.0), gpu)
    got = loss_and_grad(kp.keypoint_loss, world, tg, torch.float32)
    ref = loss_and_grad(kp.keypoint_loss_torch, world, tg, torch.float64)
    t32 = loss_and_grad(kp.keypoint_loss_torch, world, tg, torch.float32)
    S_loss, S_g = abs_terms_loss(world, tg)
    rate = lambda a: (float((a[0].double() - ref[0]).abs() / (BAR * S_loss)),                                                   # noqa: E731
                      float(((a[1].double() - ref[1]).abs() / (BAR * S_g).clamp_min(1e-300)).max()))     # (S_g = 0: a vertex no keypoint reads)
    r, r32 = rate(got), rate(t32)
    print(f"\nV={V} C={C} Kp={Kp} {parts} robust={robust}: worst error / bar: fused loss {r[0]:.3g}, g {r[1]:.3g}; "
          f"float32 torch form loss {r32[0]:.3g}, g {r32[1]:.3g}")
    assert float(ref[0]) > 0 and bool(torch.isfinite(got[1]).all()) and max(r) < 1.0, r
    assert tg.flags.tolist() == [0] * C
    X = tg.regressor.double() @ world.double()
    assert float((tg.keypoints.double() - X).abs().max()) <= EPS32 * float((tg.regressor.double().abs() @ world.double().abs()).max())


def test_one_entry_behind_a_camera(gpu, hip_lib):
    """C = 2, Kp = 5, exactly one entry (camera 1, keypoint 3) at uvw_z <= 0: flags = [0, 1]; the value and every gradient equal the
    float64 statement, which drops the entry, within the bars; moving that entry's target leaves every bit unchanged."""
    V, Kp = 40, 5
    world = 0.3 * torch.randn(V, 3, generator=torch.Generator().manual_seed(5))
    reg = torch.zeros(Kp, V)
    reg[torch.arange(Kp), torch.arange(Kp) * 7] = 1.0
    world[21] = torch.tensor([0.1, -0.2, -9.5])                                          # keypoint 3
    K = torch.tensor([[500.0, 0.0, 100.0], [0.0, 500.0, 100.0], [0.0, 0.0, 1.0]]).repeat(2, 1, 1)
    RT = torch.tensor([[[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 12.0]], [[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4.0]]])
    g = torch.Generator().manual_seed(6)
    uv, conf = 100.0 + 30.0 * torch.randn(2, Kp, 2, generator=g), 0.5 + torch.rand(2, Kp, generator=g)
    tg = on(kp.KeypointTargets(reg, K=K, RT=RT, uv=uv, conf=conf, sigma=40.0), gpu)
    world = world.to(gpu)
    got = loss_and_grad(kp.keypoint_loss, world, tg, torch.float32)
    assert tg.flags.tolist() == [0, 1]
    ref = loss_and_grad(kp.keypoint_loss_torch, world, tg, torch.float64)
    assert tg.flags.tolist() == [0, 1]
    z = kp.project_torch(tg.regressor.double() @ world.double(), tg.K.double(), tg.RT.double())[1]
    assert (z <= 0).sum().item() == 1 and float(z[1, 3]) <= 0
    S_loss, S_g = abs_terms_loss(world, tg, drop=z <= 0)                                 # (the bars with that entry left out)
    assert float((got[0].double() - ref[0]).abs()) <= BAR * float(S_loss) and float(ref[0]) > 0
    assert bool(((got[1].double() - ref[1]).abs() <= BAR * S_g.clamp_min(1e-300)).all()) and bool((got[1][21] != 0).any())
    moved = tg.clone()
    moved.uv[1, 3] += 1000.0
    again = loss_and_grad(kp.keypoint_loss, world, moved, torch.float32)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


def test_loss_writes_every_element_and_is_deterministic(gpu, hip_lib):
    """Outputs and the workspace start as NaN bit patterns (flags: -1): everything comes back written, twice the same bits, the same as
    the autograd path; keypoints = NULL changes nothing else."""
    V, C, Kp = 6890, 3, 25
    world = (0.5 * torch.randn(V, 3, generator=torch.Generator().manual_seed(1))).to(gpu)
    tg = on(targets_for(world.cpu(), Kp, C, 820), gpu)
    one, two, none = c_keypoint_loss(world, tg, gpu), c_keypoint_loss(world, tg, gpu), c_keypoint_loss(world, tg, gpu, keypoints=False)
    got = loss_and_grad(kp.keypoint_loss, world, tg, torch.float32)
    for k in ("loss", "g_world_vertex", "keypoints"):
        assert bool(torch.isfinite(one[k]).all()) and torch.equal(one[k], two[k]), k
    assert one["flags"].tolist() == [0] * C
    assert torch.equal(one["loss"], none["loss"]) and torch.equal(one["g_world_vertex"], none["g_world_vertex"])
    assert torch.equal(got[0], one["loss"][0]) and torch.equal(got[1], one["g_world_vertex"]) and torch.equal(tg.keypoints, one["keypoints"])


def test_both_ops_on_poisoned_memory(gpu, hip_lib):
    """posed_vertices_fn and keypoint_loss, forward and backward, with every output and workspace from ``torch.empty``."""
    V, J, Kp, C = 257, 24, 25, 2
    body0, fr0 = mlbs.synthetic_body_model(V, J, seed=84), frame_of(840, J, "cpu")
    tg0 = targets_for(mb.posed_vertices_torch(body0, fr0, 0.0)[0], Kp, C, 841)

    def prepare():
        return dict(body={k: v.to(gpu) for k, v in body0.items()}, fr={k: v.to(gpu) for k, v in fr0.items()},
                    tensors=[None if getattr(tg0, k) is None else getattr(tg0, k).to(gpu) for k in tg0.TENSORS])

    def run(a):
        leaves = {k: a["fr"][k].clone().requires_grad_(True) for k in NAMES}
        tg = kp.KeypointTargets(*a["tensors"], **{k: getattr(tg0, k) for k in tg0.SCALARS})
        world = kp.posed_vertices_fn(a["body"], {**a["fr"], **leaves})
        loss = kp.keypoint_loss(world, tg)
        loss.backward()
        return dict(world_vertex=world.detach(), loss=loss.detach(), flags=tg.flags, keypoints=tg.keypoints,
                    **{"g_" + k: leaves[k].grad for k in NAMES}), []

    first = under_fills(gpu, prepare, run)
    assert float(first["loss"]) > 0 and all(bool(torch.isfinite(first["g_" + k]).all()) and bool(first["g_" + k].any()) for k in NAMES)


def test_captured_chain_replays_a_new_pose_and_new_targets(gpu, hip_lib):
    """posed_vertices_fn -> keypoint_loss -> backward captured once, replayed three times, each after a copy_ of a new pose and of new
    targets: every replay equals the eager call bit for bit."""
    from moss_amd.graphs import GraphedStep
    V, J, Kp, C = 6890, 24, 25, 2
    body, fr = body_of(V, J, gpu), frame_of(850, J, gpu)
    leaves = {k: fr[k].clone().requires_grad_(True) for k in NAMES}
    world0 = mb.posed_vertices(body, fr)[0]
    tg = on(targets_for(world0.cpu(), Kp, C, 851), gpu)

    def fn():
        for v in leaves.values():
            v.grad = None
        world = kp.posed_vertices_fn(body, {**fr, **leaves})
        loss = kp.keypoint_loss(world, tg)
        loss.backward()
        return [world.detach(), loss.detach(), tg.flags, tg.keypoints] + [leaves[k].grad for k in NAMES]

    fn()                                                          # (the parent table is read on the host here, outside the capture)
    step = GraphedStep(fn, warmup=2)
    first = None
    for k in range(3):
        new = frame_of(860 + k, J, gpu)
        with torch.no_grad():
            for name in NAMES:
                leaves[name].copy_(new[name])
        tg.copy_(on(targets_for(world0.cpu(), Kp, C, 870 + k), gpu))
        got = [v.clone() for v in step()]
        torch.cuda.synchronize(gpu)
        ref = [v.clone() for v in fn()]
        for i, (u, v) in enumerate(zip(got, ref)):
            assert torch.equal(u, v), (k, i)
        if first is None:
            first = got
        else:
            assert not torch.equal(got[0], first[0]) and not torch.equal(got[1], first[1]) and not torch.equal(got[4], first[4])


# ---- PoseFitter ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def avatar(gpu, hip_lib):
    """tests/test_gpu_pose_fit.py's small avatar with keypoint targets made from its true pose through the float64 statements (two
    cameras, Kp = 25 keypoints, each the weighted mean of the template's vertices around one of them, both parts): the loss at the truth
    is 0 up to the targets' rounding to float32.  The start: Th off by (0.02, -0.01, 0.015) m, three joints off by 0.1 rad."""
    pc, cam, truth = _avatar(gpu)
    body = pc.SMPL_NEUTRAL
    vt = body["v_template"].double()
    centre = vt[torch.arange(25, device=gpu) * 271 + 13]
    reg = torch.exp(-((vt[None] - centre[:, None]) ** 2).sum(-1) / (2 * 0.05 ** 2))
    reg = (reg / reg.sum(1, keepdim=True)).float().contiguous()
    world = mb.posed_vertices_torch(f64(body), f64(truth), 0.0)[0]
    K, RT = (t.to(gpu) for t in cameras(2, 90, distance=4.0))
    X = reg.double() @ world
    u, z = kp.project_torch(X, K.double(), RT.double())
    assert float(z.min()) >= 0.5
    tg = kp.KeypointTargets(reg, K=K, RT=RT, uv=u.float().contiguous(), conf=torch.ones(2, 25, device=gpu), xyz=X.float().contiguous(),
                            conf3=torch.ones(25, device=gpu), sigma=50.0, sigma3=0.2, weight2d=1e-3, weight3d=1.0)
    start = {k: v.clone() for k, v in truth.items()}
    start["Th"] = truth["Th"] + torch.tensor([[0.02, -0.01, 0.015]], device=gpu)
    poses = truth["poses"].clone().reshape(24, 3)
    for j, axis in ((4, 0), (13, 1), (18, 2)):
        poses[j, axis] += 0.1
    start["poses"] = poses.reshape(1, 72)
    yield pc, cam, truth, start, tg, world
    del pc, cam


def vertex_error(body, truth, fitted, world):
    """The pose error of a fit: the mean distance of the fitted pose's vertices to the true pose's, float64 (what the keypoints, which
    are means of vertices, can see of poses, R and Th together; a joint that moves no keypoint may drift without it mattering)."""
    params = {**truth, "poses": fitted["poses"], "R": fitted["R"], "Th": fitted["Th"]}
    return float((mb.posed_vertices_torch(f64(body), f64(params), 0.0)[0] - world).norm(dim=1).mean())


def test_keypoint_only_fit_descends_eager_and_captured(gpu, hip_lib, avatar):
    """photometric=False with cameras, images and regions None: 60 steps at lr 1e-3, eager and captured with equal bits; the last loss
    is below the first, the vertex error and |Th - Th*| below their start; the loss at the truth is ~0."""
    from moss_amd import posefit
    pc, cam, truth, start, tg, world = avatar
    bg = torch.zeros(3, device=gpu)
    before = [p.detach().clone() for p in pc.parameters()]
    at_truth = posefit.PoseFitter(pc, cam, bg, fit_R=False).fit(None, None, None, truth, 1, keypoints=tg, photometric=False)[1]
    fitted, losses = posefit.PoseFitter(pc, cam, bg, lr=1e-3).fit(None, None, None, start, 60, keypoints=tg, photometric=False)
    graphed = posefit.PoseFitter(pc, cam, bg, lr=1e-3, capture=True)
    fitted_g, losses_g = graphed.fit(None, None, None, start, 60, keypoints=tg, photometric=False)
    losses, losses_g = losses.cpu(), losses_g.cpu()
    e0, e1 = vertex_error(pc.SMPL_NEUTRAL, truth, start, world), vertex_error(pc.SMPL_NEUTRAL, truth, fitted, world)
    th0, th1 = float((start["Th"] - truth["Th"]).norm()), float((fitted["Th"] - truth["Th"]).norm())
    print(f"\nkeypoint-only fit: loss {float(losses[0]):.6g} -> {float(losses[-1]):.6g} (at the truth {float(at_truth[0]):.3g}); mean vertex error "
          f"{e0:.4g} -> {e1:.4g} m; |Th - Th*| {th0:.4g} -> {th1:.4g} m")
    assert tuple(losses.shape) == (60,) and bool(torch.isfinite(losses).all())
    assert float(at_truth[0]) < 1e-6 * float(losses[0])
    assert float(losses[-1]) < float(losses[0]) and e1 < e0 and th1 < th0
    assert torch.equal(losses, losses_g) and graphed.captures == 1
    for k in ("poses", "Rh", "R", "Th"):
        assert torch.equal(fitted[k], fitted_g[k]), k
    for p, b in zip(pc.parameters(), before):
        assert torch.equal(p.detach(), b) and p.grad is None
    # new targets of the same sizes arrive by copy_: no second capture, and the replays serve them
    other = tg.clone()
    other.xyz += 0.01
    again_g = graphed.fit(None, None, None, start, 3, keypoints=other, photometric=False)[1].cpu()
    again = posefit.PoseFitter(pc, cam, bg, lr=1e-3).fit(None, None, None, start, 3, keypoints=other, photometric=False)[1].cpu()
    assert graphed.captures == 1 and torch.equal(again, again_g) and not torch.equal(again[0], losses[0])


def test_combined_fit_and_unchanged_photometric_fit(gpu, hip_lib, avatar):
    """photometric=True with keypoints: the loss falls, and its first value is the photometric term plus the keypoint term, each computed
    apart.  Without keypoints ``fit`` returns what it returned before: the bits of the existing path composed here by hand from
    ``posed_frame``, ``render`` and the loss, also on a fitter that has just served a keypoint fit."""
    from moss_amd import posefit
    from moss_amd.gaussian_renderer import render
    from moss_amd.lbs_weights import cross_attention_lbs_fused
    from moss_amd.loss import ViewRegion, training_loss_moss_fused
    from moss_amd.play import MossPlayer
    from moss_amd.pose import pose_head_fused
    pc, cam, truth, start, tg, world = avatar
    bg = torch.zeros(3, device=gpu)
    target = MossPlayer(pc, cam, bg).frame(cam, truth)
    gt, mask = target["render"].clone(), target["render_alpha"].clone()
    region = ViewRegion(torch.ones(1, 128, 128, device=gpu))
    plain = posefit.PoseFitter(pc, cam, bg, lr=1e-3)
    fitted_p, losses_p = plain.fit(cam, (gt, mask), region, start, 5)
    both = posefit.PoseFitter(pc, cam, bg, lr=1e-3)
    fitted_c, losses_c = both.fit(cam, (gt, mask), region, start, 12, keypoints=tg)
    # the keypoint term apart, on the fitter's own start (R = Rodrigues(Rh))
    with torch.no_grad():
        R0 = mlbs.batch_rodrigues(posefit.rotation_to_axis_angle(start["R"].reshape(3, 3).float())[None])[0].contiguous()
        body = both.body
        lk = kp.keypoint_loss(kp.posed_vertices_fn(body, {"poses": start["poses"], "shapes": start["shapes"], "R": R0, "Th": start["Th"]}), tg)
    lp, lc = losses_p[0].double(), losses_c[0].double()
    print(f"\ncombined fit: loss {float(losses_c[0]):.6g} -> {float(losses_c[-1]):.6g}; first step: photometric {float(lp):.6g} + keypoints "
          f"{float(lk):.6g} = {float(lp + lk.double()):.6g}")
    assert bool(torch.isfinite(losses_c).all()) and float(losses_c[-1]) < float(losses_c[0])
    assert float((lc - (lp + lk.double())).abs()) <= BAR * float(lp.abs() + lk.double().abs())
    # without keypoints: the same bits from a fitter that served keypoints before ...
    fitted_a, losses_a = both.fit(cam, (gt, mask), region, start, 5)
    assert torch.equal(losses_a, losses_p) and all(torch.equal(fitted_a[k], fitted_p[k]) for k in ("poses", "Rh", "R", "Th"))
    # ... and of the existing path by hand: the networks as data, posed_frame, render, MOSS's loss on the region
    plain.fit(cam, (gt, mask), region, start, 0)
    J, v = plain.J, plain._views[0]
    frozen = plain._frozen_model()
    x = frozen.get_xyz.float().contiguous()
    with torch.no_grad():
        Rs = pose_head_fused(pc.auto_regression, plain.poses.detach(), plain.pose_rotmats)["Rs"].detach().reshape(J - 1, 3, 3)
        L = cross_attention_lbs_fused(pc.cross_attention_lbs, x[None], Rs, precision="f32").detach().reshape(x.shape[0], J)
    R = mlbs.batch_rodrigues(plain.Rh[None])[0]
    T, t, _ = posefit.posed_frame(plain.body, plain.body["weights"], {"poses": plain.poses, "shapes": plain.shapes, "R": R.contiguous(),
                                                                      "Th": plain.Th}, plain.big, plain.vert_ids, x, lbs_offsets=L, correct_Rs=Rs)
    out = render(v.camera, frozen, v.pipe, bg, transforms=T, translation=t)
    by_hand = training_loss_moss_fused(out["render"], out["render_alpha"], v.gt, v.mask, v.region, lambda_dssim=0.2, lambda_mask=0.5)
    assert torch.equal(by_hand.detach().reshape(()), losses_p[0])
