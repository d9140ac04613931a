"""CPU-only: the keypoint fit's host side (moss_amd.keypoints; C ABI moss_smpl_vertices_backward / moss_keypoint_loss).  The torch
statement of the loss against central differences, its camera convention against ``bounds.project_corners_numpy``, the robustifier,
``conf = 0``, a keypoint behind a camera, every refusal, and the ctypes mirrors against the header."""
import ctypes
import os
import threading

import numpy as np
import pytest
import torch

from moss_amd import bounds as mb
from moss_amd import keypoints as kp
from moss_amd import lbs as mlbs
from tests.helpers import c_layout, ctypes_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("moss_smpl_vertices_backward", "moss_smpl_vertices_backward_workspace_bytes", "moss_keypoint_loss",
         "moss_keypoint_loss_workspace_bytes")


def cameras(C, seed, distance=8.0):
    """``K`` (C,3,3), ``RT`` (C,3,4) float32: cameras ``distance`` in front of the origin, turned a little, 512 x 512 pixels."""
    g = torch.Generator().manual_seed(seed)
    K = torch.tensor([[700.0, 0.0, 256.0], [0.0, 720.0, 250.0], [0.0, 0.0, 1.0]]).repeat(C, 1, 1)
    K[:, 0, 0] += 20.0 * torch.arange(C)
    Rc = mlbs.batch_rodrigues(0.15 * torch.randn(C, 3, generator=g))
    t = torch.tensor([0.1, -0.2, distance]).repeat(C, 1) + 0.3 * torch.randn(C, 3, generator=g)
    return K.contiguous(), torch.cat([Rc, t[:, :, None]], 2).float().contiguous()


def regressor(Kp, V, seed):
    """(Kp,V) float32: rows of non-negative weights that sum to one, most of them tiny, a tenth exactly zero."""
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(Kp, V, generator=g) ** 8
    r[torch.rand(Kp, V, generator=g) < 0.1] = 0
    r[:, 0] += 1e-3
    return (r / r.sum(1, keepdim=True)).float().contiguous()


def targets_for(world, Kp, C, seed, parts="both", sigma=30.0, sigma3=0.1, zero_conf=True):
    """Targets near the keypoints of ``world`` (V,3): ``uv`` a few pixels and ``xyz`` a few centimetres off, some ``conf`` exactly 0."""
    g = torch.Generator().manual_seed(seed)
    V = world.shape[0]
    reg = regressor(Kp, V, seed + 1)
    a = {}
    if parts in ("2d", "both"):
        K, RT = cameras(C, seed + 2)
        u, z = kp.project_torch(reg.double() @ world.double().cpu(), K.double(), RT.double())
        assert float(z.min()) >= 0.5
        conf = torch.rand(C, Kp, generator=g)
        if zero_conf and C * Kp > 1:
            conf.view(-1)[::3] = 0
        a.update(K=K, RT=RT, uv=(u + 20.0 * torch.randn(C, Kp, 2, generator=g)).float().contiguous(), conf=conf.contiguous())
    if parts in ("3d", "both"):
        conf3 = torch.rand(Kp, generator=g)
        if zero_conf and Kp > 1:
            conf3[::4] = 0
        X = reg.double() @ world.double().cpu()
        a.update(xyz=(X + 0.05 * torch.randn(Kp, 3, generator=g)).float().contiguous(), conf3=conf3.contiguous())
    return kp.KeypointTargets(reg, sigma=sigma, sigma3=sigma3, weight2d=1.0, weight3d=50.0, **a)


def test_imports_without_a_gpu_and_symbols_declared(hip_lib):
    import moss_amd
    from moss_amd.posefit import PoseFitter
    assert {"keypoint_loss", "posed_vertices_fn", "KeypointTargets"} <= set(moss_amd.__all__)
    assert moss_amd.keypoint_loss is kp.keypoint_loss and moss_amd.KeypointTargets is kp.KeypointTargets
    assert "keypoints" in PoseFitter.fit.__code__.co_varnames and "photometric" in PoseFitter.fit.__code__.co_varnames
    text = open(os.path.join(ROOT, "include", "moss_raster.h")).read()
    for name in NAMES:
        assert name + "(" in text and hasattr(hip_lib, name)
    assert "#define MOSS_ABI_VERSION 7" in text and f"#define MOSS_KEYPOINTS_MAX {kp.KEYPOINTS_MAX}" in text
    assert hip_lib.moss_smpl_vertices_backward_workspace_bytes(6890, 24) > 0 and hip_lib.moss_keypoint_loss_workspace_bytes(4, 25) > 0
    for bad in ((0, 24), (10, 0), (10, 65)):
        assert hip_lib.moss_smpl_vertices_backward_workspace_bytes(*bad) == 0
    for bad in ((-1, 25), (65536, 25), (1, 0), (1, 129)):
        assert hip_lib.moss_keypoint_loss_workspace_bytes(*bad) == 0


@pytest.mark.parametrize("V,J", [(1, 1), (17, 2), (257, 24)])
def test_torch_statement_agrees_with_central_differences(V, J):
    """d loss / d (poses, R, Th) of ``keypoint_loss_torch(posed_vertices_torch(...))`` in float64, both parts, both robustifiers:
    autograd against central differences with h = 1e-5; the bar is 1e-6 max|g| per leaf."""
    body = {k: (v.double() if v.is_floating_point() else v) for k, v in mlbs.synthetic_body_model(V, J, seed=70 + J).items()}
    fr = {k: v.double() for k, v in mlbs.synthetic_frame(71 + J, J).items()}
    world0 = mb.posed_vertices_torch(body, fr, 0.0)[0]
    tg = targets_for(world0.float(), min(V, 5), 2, 72 + J)
    leaves = {k: fr[k].clone().requires_grad_(True) for k in ("poses", "R", "Th")}

    def f(p):
        return kp.keypoint_loss_torch(mb.posed_vertices_torch(body, {**fr, **p}, 0.0)[0], tg)

    f(leaves).backward()
    h = 1e-5
    for k, leaf in leaves.items():
        num = torch.zeros_like(leaf)
        with torch.no_grad():
            for i in range(leaf.numel()):
                d = torch.zeros_like(leaf)
                d.view(-1)[i] = h
                num.view(-1)[i] = (f({**leaves, k: leaf + d}) - f({**leaves, k: leaf - d})) / (2 * h)
        err, scale = float((num - leaf.grad).abs().max()), float(leaf.grad.abs().max())
        print(f"V={V} J={J} {k}: max |central difference - autograd| {err:.3g}, max|g| {scale:.3g}")
        assert err <= 1e-6 * scale, (k, err, scale)                # (V = J = 1: the vertex is its own joint, poses has no gradient)
        assert scale > 0 or (V, J, k) == (1, 1, "poses")


def test_projection_is_project_corners_numpy():
    """``project_torch`` of a box's eight corners equals ``bounds.project_corners_numpy(..., return_unrounded=True)``: one camera
    convention (``cam = RT [X, 1]``, ``uvw = K cam``)."""
    wb = torch.tensor([[-0.6, -0.9, -0.3], [0.5, 0.8, 0.4]])
    K, RT = cameras(3, 5)
    _, _, xy = mb.project_corners_numpy(wb, K, RT, return_unrounded=True)
    i = torch.arange(8)
    corners = torch.stack([wb[(i >> 2) & 1, 0], wb[(i >> 1) & 1, 1], wb[i & 1, 2]], 1).double()
    u, z = kp.project_torch(corners, K.double(), RT.double())
    assert float(z.min()) > 0 and np.abs(u.numpy() - xy).max() <= 1e-9 * np.abs(xy).max()


def _plain(world, tg, rho2, rho3):
    """The loss written out with numpy-like torch ops, entry by entry."""
    X = tg.regressor.double() @ world.double()
    total = 0.0
    for c in range(tg.C):
        for k in range(tg.Kp):
            cam = tg.RT[c].double() @ torch.cat([X[k], torch.ones(1, dtype=torch.float64)])
            uvw = tg.K[c].double() @ cam
            if float(uvw[2]) <= 0:
                continue
            r2 = float(((uvw[:2] / uvw[2] - tg.uv[c, k].double()) ** 2).sum())
            total += tg.weight2d / (tg.C * tg.Kp) * float(tg.conf[c, k]) * rho2(r2)
    if tg.has3d:
        for k in range(tg.Kp):
            total += tg.weight3d / tg.Kp * float(tg.conf3[k]) * rho3(float(((X[k] - tg.xyz[k].double()) ** 2).sum()))
    return total


def test_robustifier_and_plain_squares():
    """sigma > 0: rho = s^2 r2 / (s^2 + r2); sigma <= 0: r2 itself -- both parts, against the loss written out entry by entry."""
    world = 0.5 * torch.randn(40, 3, generator=torch.Generator().manual_seed(1))
    gm = lambda s: (lambda r2: s * s * r2 / (s * s + r2))                                # noqa: E731
    for sigma, sigma3 in ((30.0, 0.1), (0.0, -1.0)):
        tg = targets_for(world, 6, 2, 9, sigma=sigma, sigma3=sigma3)
        want = _plain(world, tg, gm(sigma) if sigma > 0 else (lambda r2: r2), gm(sigma3) if sigma3 > 0 else (lambda r2: r2))
        got = float(kp.keypoint_loss_torch(world.double(), tg))
        assert abs(got - want) <= 1e-12 * abs(want) and want > 0


def test_zero_confidence_removes_an_entry():
    world = 0.5 * torch.randn(40, 3, generator=torch.Generator().manual_seed(2))
    tg = targets_for(world, 6, 2, 11, zero_conf=False)
    tg.conf[1, 4] = 0
    tg.conf3[2] = 0
    moved = tg.clone()
    moved.uv[1, 4] += 500.0
    moved.xyz[2] += 3.0
    out = []
    for t in (tg, moved):
        w = world.double().requires_grad_(True)
        loss = kp.keypoint_loss_torch(w, t)
        loss.backward()
        out.append((loss.detach(), w.grad))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and float(out[0][0]) > 0


def test_a_keypoint_behind_a_camera_adds_nothing_and_sets_the_flag():
    world = torch.tensor([[0.0, 0.0, 0.0], [0.2, 0.1, -0.1], [0.1, -0.3, -9.5]])        # (the third lies behind camera 1 only)
    K = torch.tensor([[500.0, 0.0, 100.0], [0.0, 500.0, 100.0], [0.0, 0.0, 1.0]]).repeat(2, 1, 1)
    RT = torch.tensor([[[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 12.0]], [[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4.0]]])
    uv, conf = torch.full((2, 3, 2), 90.0), torch.ones(2, 3)
    tg = kp.KeypointTargets(torch.eye(3), K=K, RT=RT, uv=uv, conf=conf, sigma=0.0)
    w = world.double().requires_grad_(True)
    loss = kp.keypoint_loss_torch(w, tg)
    loss.backward()
    assert tg.flags.tolist() == [0, 1]
    assert abs(float(loss.detach()) - _plain(world, tg, lambda r2: r2, None)) <= 1e-12 * float(loss.detach())   # (_plain skips the entry)
    first = kp.KeypointTargets(torch.eye(3), K=K[:1].clone(), RT=RT[:1].clone(), uv=uv[:1].clone(), conf=conf[:1].clone(), sigma=0.0)
    w1 = world.double().requires_grad_(True)
    kp.keypoint_loss_torch(w1, first).backward()
    assert first.flags.tolist() == [0]
    # the vertex behind camera 1 has camera 0's gradient alone, at weight 1 / (2 Kp) instead of 1 / Kp
    assert torch.allclose(w.grad[2], 0.5 * w1.grad[2], rtol=1e-12, atol=0) and bool(torch.isfinite(w.grad).all())
    assert float(w.grad[2].abs().max()) > 0


def test_every_refusal_names_its_argument():
    reg, (K, RT) = regressor(4, 10, 3), cameras(2, 4)
    uv, conf, xyz, conf3 = torch.zeros(2, 4, 2), torch.ones(2, 4), torch.zeros(4, 3), torch.ones(4)
    T = kp.KeypointTargets
    with pytest.raises(ValueError, match="KeypointTargets: neither the 2D part .* nor the 3D part"):
        T(reg)
    with pytest.raises(ValueError, match=r"KeypointTargets: Kp = 129 keypoints .* 1\.\.128"):
        T(torch.zeros(129, 10), xyz=torch.zeros(129, 3), conf3=torch.ones(129))
    with pytest.raises(ValueError, match="KeypointTargets: Kp = 0"):
        T(torch.zeros(0, 10), xyz=torch.zeros(0, 3), conf3=torch.ones(0))
    with pytest.raises(ValueError, match="KeypointTargets: uv must have shape"):
        T(reg, K=K, RT=RT, uv=torch.zeros(2, 5, 2), conf=conf)
    with pytest.raises(ValueError, match="KeypointTargets: conf3 must have shape"):
        T(reg, xyz=xyz, conf3=torch.ones(5))
    with pytest.raises(ValueError, match="KeypointTargets: RT, conf missing"):
        T(reg, K=K, uv=uv)
    with pytest.raises(ValueError, match="KeypointTargets: xyz requires grad"):
        T(reg, xyz=xyz.clone().requires_grad_(True), conf3=conf3)
    with pytest.raises(ValueError, match="KeypointTargets: regressor requires grad"):
        T(reg.clone().requires_grad_(True), xyz=xyz, conf3=conf3)
    with pytest.raises(ValueError, match="KeypointTargets: conf must be torch.float32"):
        T(reg, K=K, RT=RT, uv=uv, conf=conf.double())
    tg = T(reg, K=K, RT=RT, uv=uv, conf=conf, xyz=xyz, conf3=conf3)
    with pytest.raises(ValueError, match=r"KeypointTargets.copy_: xyz must be of shape \(4, 3\), got none"):
        tg.copy_(T(reg, K=K, RT=RT, uv=uv, conf=conf))
    assert tg.copy_(tg.clone()) is tg and tg.key == tg.clone().key
    with pytest.raises(ValueError, match="keypoint_loss runs the HIP kernels of csrc/keypoints.hip: its tensors must be on a GPU"):
        kp.keypoint_loss(torch.zeros(10, 3), tg)
    with pytest.raises(ValueError, match="keypoint_loss: targets must be a KeypointTargets"):
        kp.keypoint_loss(torch.zeros(10, 3), None)
    body = mlbs.synthetic_body_model(10, 2, seed=1)
    fr = mlbs.synthetic_frame(1, 2)
    why = r"it is data of the fit \(the avatar is frozen: gradients go to params\['poses'\], params\['R'\] and params\['Th'\] only\); detach it"
    with pytest.raises(ValueError, match=r"posed_vertices_fn: params\['shapes'\] requires grad, but " + why):
        kp.posed_vertices_fn(body, {**fr, "shapes": fr["shapes"].clone().requires_grad_(True)})
    with pytest.raises(ValueError, match="posed_vertices_fn: posedirs requires grad, but " + why):
        kp.posed_vertices_fn({**body, "posedirs": body["posedirs"].clone().requires_grad_(True)}, fr)
    with pytest.raises(ValueError, match="posed_vertices_fn runs the HIP kernels of csrc/frame_bounds.hip: its tensors must be on a GPU"):
        kp.posed_vertices_fn(body, fr)


@pytest.mark.parametrize("cname,pyname", [("moss_smpl_vertices_backward_args", "SmplVerticesBackwardArgs"),
                                          ("moss_keypoint_loss_args", "KeypointLossArgs")])
def test_ctypes_blocks_match_the_c_layout(tmp_path, cname, pyname):
    from moss_amd import _lib
    cls = getattr(_lib, pyname)
    assert c_layout(tmp_path, cname, [f[0] for f in cls._fields_]) == ctypes_layout(cls)
    assert _lib.KEYPOINTS_MAX == kp.KEYPOINTS_MAX


def test_c_abi_refuses_bad_arguments_with_its_name(hip_lib):
    """Host-side validation needs no device.  (In a thread of its own: the error text is per thread.)"""
    failures = []

    def run():
        try:
            _refusals(hip_lib)
        except BaseException as e:                                # noqa: BLE001
            failures.append(e)

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if failures:
        raise failures[0]


def _refusals(lib):
    from moss_amd._lib import KeypointLossArgs, SmplVerticesBackwardArgs
    PTR = 256                                                     # (never dereferenced on the host)

    def refused(fn, a, *words):
        assert fn(ctypes.byref(a), None) == -1
        text = lib.moss_last_error()
        assert all(w in text for w in words), text

    vb, name = lib.moss_smpl_vertices_backward, b"moss_smpl_vertices_backward"
    assert vb(None, None) == -1 and name in lib.moss_last_error()
    a = SmplVerticesBackwardArgs()
    a.V, a.J, a.shapedirs_stride = 0, 2, 10
    refused(vb, a, name + b": V must be >= 1")
    a.V = 10
    for J in (0, 65):
        a.J = J
        refused(vb, a, name + b": J must be 1..64")
    a.J, a.num_betas = 2, 11
    refused(vb, a, name, b"num_betas")
    a.num_betas = 10
    a.v_template = a.shapedirs = a.J_regressor = a.weights = PTR
    refused(vb, a, name, b"posedirs")
    a.posedirs = PTR
    a.poses = a.R = a.Th = PTR
    refused(vb, a, name, b"shapes")
    a.shapes = PTR
    refused(vb, a, name, b"g_world_vertex")
    a.g_world_vertex = PTR
    a.g_poses = a.g_R = PTR
    refused(vb, a, name, b"g_Th")
    a.g_Th = PTR
    a.parents[1] = 1
    refused(vb, a, name + b": parents[j] must be in [0, j)")
    a.parents[1] = 0
    a.workspace, a.workspace_bytes = PTR, lib.moss_smpl_vertices_backward_workspace_bytes(10, 2) - 1
    refused(vb, a, name, b"workspace")
    a.J, a.posedirs, a.workspace, a.workspace_bytes = 1, None, None, 1 << 20      # (J = 1 passes without posedirs: the workspace is next)
    refused(vb, a, name, b"workspace")

    kl, name = lib.moss_keypoint_loss, b"moss_keypoint_loss"
    assert kl(None, None) == -1 and name in lib.moss_last_error()
    k = KeypointLossArgs()
    k.V, k.Kp, k.C = 0, 4, 1
    refused(kl, k, name + b": V must be >= 1")
    k.V = 10
    for Kp in (0, 129):
        k.Kp = Kp
        refused(kl, k, name + b": Kp must be 1..128")
    k.Kp, k.C = 4, -1
    refused(kl, k, name + b": C must be 0..65535")
    k.C = 0
    refused(kl, k, name, b"neither the 2D part", b"nor the 3D part")
    k.C = 1
    refused(kl, k, name, b"world_vertex", b"regressor")
    k.world_vertex = k.regressor = PTR
    k.K = k.RT = k.uv = PTR
    refused(kl, k, name, b"conf")
    k.conf, k.xyz = PTR, PTR
    refused(kl, k, name + b": xyz needs conf3")
    k.conf3 = PTR
    k.loss = k.g_world_vertex = PTR
    refused(kl, k, name, b"flags")
    k.flags = PTR
    k.workspace, k.workspace_bytes = PTR, lib.moss_keypoint_loss_workspace_bytes(1, 4) - 1
    refused(kl, k, name, b"workspace")
