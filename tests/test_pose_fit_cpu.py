"""CPU side of the pose fit (moss_amd.posefit; C ABI moss_lbs_deform_backward_frame / moss_smpl_frame_backward_pose): the symbols, their
declarations and refusals, the torch yardstick ``posed_frame_torch`` in float64 against the reference's own numbers and against
central finite differences, and the refusals of the Python surface (there is no CPU path)."""
import ctypes
import os
import re
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from moss_amd import lbs as mlbs
from moss_amd import posefit
from tests.helpers import c_layout, ctypes_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("moss_lbs_deform_backward_frame", "moss_lbs_frame_workspace_bytes", "moss_smpl_frame_backward_pose")


def test_symbols_exported_and_declared(hip_lib):
    import moss_amd
    text = open(os.path.join(ROOT, "include", "moss_raster.h")).read()
    assert re.search(r"#define\s+MOSS_ABI_VERSION\s+7\b", text) and hip_lib.moss_abi_version() == 7
    diag = re.search(r"#ifdef MOSS_DIAG\n(.*?)#endif", text, flags=re.S).group(0)
    public = re.sub(r"/\*.*?\*/", "", text.replace(diag, ""), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, public), name
        assert hasattr(hip_lib, name), name
    assert "} moss_lbs_backward_frame_args;" in public and "} moss_smpl_frame_backward_pose_args;" in public
    assert int(re.search(r"#define\s+MOSS_SMPL_FRAME_SAVED_FLOATS_PER_JOINT\s+(\d+)", text).group(1)) == 33
    assert moss_amd.PoseFitter is posefit.PoseFitter and moss_amd.posed_frame is posefit.posed_frame
    assert {"PoseFitter", "posed_frame"} <= set(moss_amd.__all__)
    ws, old = hip_lib.moss_lbs_frame_workspace_bytes, hip_lib.moss_lbs_workspace_bytes
    assert ws(0, 24) == 0 and ws(10, 0) == 0 and ws(10, 65) == 0
    prev = 0
    for P in (1, 127, 128, 129, 6890, 45695, 1000000):
        assert ws(P, 24) >= old(P, 24) + ((P + 127) // 128) * 12 * 8 and ws(P, 24) >= prev
        prev = ws(P, 24)


@pytest.mark.parametrize("cname,pyname", [("moss_lbs_backward_frame_args", "LbsBackwardFrameArgs"),
                                          ("moss_smpl_frame_backward_pose_args", "SmplFrameBackwardPoseArgs")])
def test_ctypes_blocks_match_the_c_layout(tmp_path, cname, pyname):
    """The ctypes mirrors have the header's size and field offsets (compiled against the header with the host compiler)."""
    from moss_amd import _lib
    cls = getattr(_lib, pyname)
    assert c_layout(tmp_path, cname, [f[0] for f in cls._fields_]) == ctypes_layout(cls)


def test_c_abi_refuses_bad_arguments_with_its_name(hip_lib):
    """Host-side validation needs no device.  (In a thread of its own: the error text is per thread, and tests/test_host_cpu.py
    expects the main thread's to be empty.)"""
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


def _refusals(hip_lib):
    from moss_amd._lib import LbsBackwardFrameArgs, SmplFrameBackwardPoseArgs
    PTR = 256                                                     # (never dereferenced on the host)
    pose, frame = hip_lib.moss_smpl_frame_backward_pose, hip_lib.moss_lbs_deform_backward_frame
    for J in (0, 65):
        b = SmplFrameBackwardPoseArgs()
        b.P, b.V, b.J = 1, 10, J
        b.saved = b.poses = b.g_poses = PTR
        assert pose(ctypes.byref(b), None) == -1
        assert b"moss_smpl_frame_backward_pose: J must be 1..64" in hip_lib.moss_last_error()
        a = LbsBackwardFrameArgs()
        a.P, a.J, a.V = 1, J, 10
        assert frame(ctypes.byref(a), None) == -1
        assert b"moss_lbs_deform_backward_frame: J must be 1..64" in hip_lib.moss_last_error()
    b = SmplFrameBackwardPoseArgs()
    b.P, b.V, b.J = 1, 10, 3
    b.saved = b.poses = PTR
    b.parents[1], b.parents[2] = 0, 1
    assert pose(ctypes.byref(b), None) == -1                      # NULL g_poses
    assert b"moss_smpl_frame_backward_pose" in hip_lib.moss_last_error() and b"g_poses" in hip_lib.moss_last_error()
    b.g_poses = PTR
    b.parents[2] = 2
    assert pose(ctypes.byref(b), None) == -1
    assert b"moss_smpl_frame_backward_pose: parents[j] must be in [0, j)" in hip_lib.moss_last_error()
    a = LbsBackwardFrameArgs()
    a.P, a.J, a.V = 129, 24, 10
    a.vert_ids = a.weights = a.A_big = a.A_obs = a.d = a.R = a.Th = PTR
    a.g_p = PTR                                                   # g_p without x
    assert frame(ctypes.byref(a), None) == -1
    assert b"moss_lbs_deform_backward_frame" in hip_lib.moss_last_error() and b"need x" in hip_lib.moss_last_error()
    a.g_p = None
    a.g_R = PTR                                                   # workspace too small with g_R requested
    a.workspace, a.workspace_bytes = PTR, hip_lib.moss_lbs_workspace_bytes(129, 24)     # (enough for g_A_obs alone: not for g_R)
    assert frame(ctypes.byref(a), None) == -1
    assert b"moss_lbs_deform_backward_frame" in hip_lib.moss_last_error() and b"workspace" in hip_lib.moss_last_error()
    a.workspace = None
    a.workspace_bytes = 1 << 30
    assert frame(ctypes.byref(a), None) == -1 and b"workspace" in hip_lib.moss_last_error()


def _golden_frame(case, dtype):
    from tests.golden import make_golden_lbs as gold
    g32, g = gold.golden_inputs(case), gold.golden_inputs(case, dtype)
    _, ids = gold.cpu_knn(g32["t_vertices"], g32["query_pts"])
    L = None if g["lbs_weights"] is None else g["lbs_weights"][0]
    cR = None if g["correct_Rs"] is None else g["correct_Rs"][0]
    return g, ids.reshape(-1), L, cR


@pytest.mark.parametrize("case", ["plain", "refined"])
def test_torch_form_float64_reproduces_reference_golden(case):
    """posed_frame_torch in float64 against the reference's own float32 transforms, translation and world_src_pts of
    tests/golden/lbs_deform.npz, within tests/test_lbs_cpu.py's bar for that fixture (64 kappa eps32 times the tensor's scale)."""
    from tests.test_lbs_cpu import FIXTURE, chain_torch, output_bar
    golden = np.load(FIXTURE)
    _, _, kappa, _ = chain_torch(case, requires_grad=False)
    g, ids, L, cR = _golden_frame(case, torch.float64)
    T, t, p = posefit.posed_frame_torch(g["body"], g["body"]["weights"], g["params"], g["t_params"], ids, g["query_pts"][0],
                                        lbs_offsets=L, correct_Rs=cR)
    worst = {}
    for name, got in (("transforms", T), ("translation", t), ("world_src_pts", p)):
        ref = golden[f"{case}_{name}"]
        assert got[None].shape == ref.shape, name
        worst[name] = float(np.abs(got[None].numpy() - ref).max()) / output_bar(ref, kappa)
    print(f"\n{case}: posed_frame_torch float64 vs reference float32, fraction of the bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) < 1.0, worst


def fd_case(J=24, P=65, V=200, seed=5, dtype=torch.float64, device="cpu"):
    """The case of the finite-difference test, shared with tests/test_gpu_pose_fit.py: joints 0 (the root) and 7 with r = 0 exactly,
    joint 11 with |r| = 3.0."""
    body = {k: (v.to(device) if k == "kintree_table" else v.to(dtype=dtype, device=device))
            for k, v in mlbs.synthetic_body_model(V, J, seed=60 + J).items()}
    conv = lambda d: {k: v.to(dtype=dtype, device=device) for k, v in d.items()}       # noqa: E731
    fr, big = conv(mlbs.synthetic_frame(seed, J)), conv(mlbs.synthetic_frame(0, J, big_pose=True))
    poses = fr["poses"].reshape(J, 3).clone()
    poses[0] = 0
    poses[7] = 0
    poses[11] = poses[11] / poses[11].norm() * 3.0
    fr["poses"] = poses.reshape(1, 3 * J)
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (P,), generator=g).to(device)
    x = (body["v_template"].cpu()[ids.cpu()] + 0.03 * torch.randn(P, 3, generator=g, dtype=torch.float64).to(dtype)).to(device)
    L = (0.7 * torch.randn(P, J, generator=g, dtype=torch.float64)).to(dtype=dtype, device=device)
    cR = mlbs.batch_rodrigues(0.1 * torch.randn(J - 1, 3, generator=g, dtype=torch.float64)).to(dtype=dtype, device=device)
    cot = [torch.randn(*s, generator=g, dtype=torch.float64).to(dtype=dtype, device=device) for s in ((P, 3, 3), (P, 3), (P, 3))]
    return body, fr, big, ids, x, L, cR, cot


def test_float64_autograd_agrees_with_central_differences():
    """d/d(poses, R, Th) of <cotangents, posed_frame_torch> in float64 against central differences, h = 1e-5: truncation ~ h^2 and
    rounding ~ eps64 / h are both far below the bar 1e-6 max|g| per tensor.  J = 24, P = 65; joints with r = 0 exactly (the root among
    them) and one with |r| = 3.0: this pins the yardstick, the +1e-8 shift of the norm included."""
    body, fr, big, ids, x, L, cR, cot = fd_case()
    names = ("poses", "R", "Th")

    def value(params):
        out = posefit.posed_frame_torch(body, body["weights"], params, big, ids, x, lbs_offsets=L, correct_Rs=cR)
        return sum((o * c).sum() for o, c in zip(out, cot))

    leaves = {**fr, **{k: fr[k].clone().requires_grad_(True) for k in names}}
    grads = dict(zip(names, torch.autograd.grad(value(leaves), [leaves[k] for k in names])))
    h = 1e-5
    for name in names:
        g, fd = grads[name], torch.zeros_like(grads[name])
        with torch.no_grad():
            for e in range(g.numel()):
                vals = []
                for sign in (1.0, -1.0):
                    moved = fr[name].clone()
                    moved.view(-1)[e] += sign * h
                    vals.append(value({**fr, name: moved}))
                fd.view(-1)[e] = (vals[0] - vals[1]) / (2 * h)
        err, bar = float((g - fd).abs().max()), 1e-6 * float(g.abs().max())
        print(f"\n{name}: max |autograd - central difference| {err:.3g}, bar {bar:.3g}")
        assert err <= bar, name
    assert float(grads["poses"].reshape(24, 3)[[0, 7]].abs().max()) > 0 and bool(torch.isfinite(grads["poses"]).all())


def test_refuses_cpu_tensors_and_data_that_requires_grad():
    body, fr, big, ids, x, L, cR, _ = fd_case(dtype=torch.float32)
    W = body["weights"]
    with pytest.raises(ValueError, match="must be on a GPU.*posed_frame_torch"):
        posefit.posed_frame(body, W, fr, big, ids, x, lbs_offsets=L, correct_Rs=cR)
    grad = lambda t: t.clone().requires_grad_(True)                                     # noqa: E731
    for name, kw in (("x", dict(x=grad(x))), ("lbs_offsets", dict(lbs_offsets=grad(L))), ("correct_Rs", dict(correct_Rs=grad(cR)))):
        args = {**dict(x=x, lbs_offsets=L, correct_Rs=cR), **kw}
        with pytest.raises(ValueError, match=name + " requires grad"):
            posefit.posed_frame(body, W, fr, big, ids, **args)
    with pytest.raises(ValueError, match=r"params\['shapes'\] requires grad"):
        posefit.posed_frame(body, W, {**fr, "shapes": grad(fr["shapes"])}, big, ids, x)
    with pytest.raises(ValueError, match="posedirs requires grad"):
        posefit.posed_frame({**body, "posedirs": grad(body["posedirs"])}, W, fr, big, ids, x)
    with pytest.raises(ValueError, match="W requires grad"):
        posefit.posed_frame(body, grad(W), fr, big, ids, x)
    # leaves that are the fit's variables are accepted up to the device check
    with pytest.raises(ValueError, match="must be on a GPU"):
        posefit.posed_frame(body, W, {**fr, "poses": grad(fr["poses"]), "R": grad(fr["R"]), "Th": grad(fr["Th"])}, big, ids, x)
    pc = SimpleNamespace(_xyz=x, motion_offset_flag=False, SMPL_NEUTRAL=body, knn=None)
    view = SimpleNamespace(big_pose_smpl_param=big, big_pose_world_vertex=body["v_template"])
    with pytest.raises(ValueError, match="must be on a GPU"):
        posefit.PoseFitter(pc, view, torch.zeros(3))
    with pytest.raises(ValueError, match="lacks"):
        posefit.PoseFitter(SimpleNamespace(_xyz=x, motion_offset_flag=True, SMPL_NEUTRAL=body, knn=None), view, torch.zeros(3))
