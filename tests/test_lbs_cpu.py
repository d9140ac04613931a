"""CPU side of the fused LBS deformation (moss_amd.lbs): the torch formulation -- smpl_joint_transforms, vertex_offsets, deform_torch --
in float64 against the reference's own float32 coarse_deform_c2source (tests/golden/lbs_deform.npz, tests/golden/make_golden_lbs.py).

The bar.  Everything the reference forms is O(1) products of O(1) factors, except the inverse of the blended big-pose block B3, whose
float32 error is ~ kappa(B3) eps relative (and its adjoint's ~ kappa^2 eps).  So an element of an output or gradient of scale s
(its largest magnitude in the case) may differ from exact by  c kappa eps32 s  with c a small multiple of the chain's depth (~20 rounded
operations from the joint chain to the output): c = 64 for the outputs, 64 kappa for the gradients.  The test records the measured
gap of the reference's float32 to our float64 as a fraction of that bar (printed; tests/test_gpu_lbs.py uses the same bar).
"""
import os

import numpy as np
import pytest
import torch

from moss_amd import lbs as mlbs
from tests.golden import make_golden_lbs as gold

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "lbs_deform.npz")
EPS32 = float(np.finfo(np.float32).eps)


def chain_torch(case, dtype=torch.float64, requires_grad=True):
    """The reference's coarse_deform_c2source rebuilt from moss_amd.lbs's torch pieces, in ``dtype`` on the CPU:
    (outputs {name: tensor}, leaves {name: tensor}, kappa (P,) of B3).  Nearest vertices from the float32 positions, as the reference's."""
    g32 = gold.golden_inputs(case)
    g = gold.golden_inputs(case, dtype)
    _, ids = gold.cpu_knn(g32["t_vertices"], g32["query_pts"])
    ids = ids.reshape(-1)
    body, params, t_params = g["body"], g["params"], g["t_params"]
    q = g["query_pts"].clone().requires_grad_(requires_grad)
    L = None if g["lbs_weights"] is None else g["lbs_weights"].clone().requires_grad_(requires_grad)
    cR = None if g["correct_Rs"] is None else g["correct_Rs"].clone().requires_grad_(requires_grad)
    J = body["weights"].shape[1]
    A_big = mlbs.smpl_joint_transforms(body, t_params)[0][0]
    rot = mlbs.batch_rodrigues(params["poses"].reshape(-1, 3))
    if cR is not None:
        rot = torch.cat([rot[:1], rot[1:] @ cR.reshape(J - 1, 3, 3)], 0)
    A_obs, R, Th = mlbs.smpl_joint_transforms(body, params, rot_mats=rot)
    D = mlbs.vertex_offsets(body, params, t_params, rot)
    R, Th = R.reshape(3, 3), Th.reshape(3)
    T, t, p, w = mlbs.deform_torch(ids, body["weights"], None if L is None else L[0], A_big, A_obs[0], D[ids], R, Th, x=q[0])
    B3 = (w @ A_big.reshape(J, 16)).reshape(-1, 4, 4)[:, :3, :3]
    kappa = torch.linalg.cond(B3.detach().double())
    out = {"smpl_src_pts": ((p - Th) @ R)[None], "world_src_pts": p[None], "bweights": w[None], "transforms": T[None],
           "translation": t[None]}
    leaves = {"query_pts": q, "lbs_weights": L, "correct_Rs": cR}
    return out, {k: v for k, v in leaves.items() if v is not None}, kappa, g["cotangents"]


def output_bar(ref, kappa):
    return 64.0 * float(kappa.max()) * EPS32 * max(float(np.abs(ref).max()), 1e-30)


def grad_bar(ref, kappa):
    return 64.0 * float(kappa.max()) ** 2 * EPS32 * max(float(np.abs(ref).max()), 1e-30)


@pytest.fixture(scope="module")
def golden():
    return np.load(FIXTURE)


@pytest.mark.parametrize("case", list(gold.CASES))
def test_golden_inputs_checksum(golden, case):
    """The inputs regenerated from the seeds are the ones the fixture was made from."""
    assert int(golden[f"{case}_seed"]) == gold.CASES[case]
    assert str(golden[f"{case}_inputs_sha256"]) == gold.inputs_checksum(case)


@pytest.mark.parametrize("case", list(gold.CASES))
def test_torch_chain_float64_reproduces_reference(golden, case):
    """smpl_joint_transforms + vertex_offsets + deform_torch in float64 reproduce the reference's float32 outputs and the gradients
    with respect to query_pts, lbs_weights and correct_Rs, within the kappa-scaled bar of the module docstring."""
    out, leaves, kappa, cot = chain_torch(case)
    worst = {}
    for k in gold.OUTPUTS:
        ref = golden[f"{case}_{k}"]
        got = out[k].detach().numpy()
        assert got.shape == ref.shape, k
        err = float(np.abs(got - ref).max())
        worst[k] = err / output_bar(ref, kappa)
    loss = sum((out[k] * cot[k]).sum() for k in gold.COTANGENT_OF)
    grads = torch.autograd.grad(loss, list(leaves.values()))
    for name, gr in zip(leaves, grads):
        ref = golden[f"{case}_grad_{name}"]
        assert gr.shape == ref.shape, name
        worst["grad_" + name] = float(np.abs(gr.numpy() - ref).max()) / grad_bar(ref, kappa)
    if case == "refined":
        assert {"grad_lbs_weights", "grad_correct_Rs"} <= set(worst)
    print(f"\n{case}: max kappa(B3) {float(kappa.max()):.3g}; reference float32 vs float64, fraction of the bar: "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) < 1.0, worst


def test_smpl_joint_transforms_rest_pose_is_identity():
    """Zero pose: every joint transform is the identity (the rest joints are subtracted), independent of the shape."""
    body = mlbs.synthetic_body_model(64, 24, seed=3)
    params = {"poses": torch.zeros(1, 72), "shapes": torch.randn(1, 10), "R": torch.eye(3), "Th": torch.zeros(1, 3)}
    A, _, _ = mlbs.smpl_joint_transforms(body, params)
    assert A.shape == (1, 24, 4, 4)
    torch.testing.assert_close(A[0], torch.eye(4).expand(24, 4, 4), atol=1e-6, rtol=0)


def test_synthetic_body_model_shape_and_seed():
    a = mlbs.synthetic_body_model(100, 24, seed=5)
    b = mlbs.synthetic_body_model(100, 24, seed=5)
    assert a["weights"].shape == (100, 24) and a["posedirs"].shape == (100, 3, 207) and a["J_regressor"].shape == (24, 100)
    torch.testing.assert_close(a["weights"].sum(1), torch.ones(100))
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert a["kintree_table"][0].tolist() == list(mlbs.SMPL_PARENTS)
    c = mlbs.synthetic_body_model(40, 55, seed=5)
    par = c["kintree_table"][0].tolist()
    assert all(0 <= par[j] < j for j in range(1, 55))


def test_lbs_deform_refuses_cpu_tensors():
    """No CPU path: lbs_deform is the HIP op (deform_torch is the torch form)."""
    W = torch.rand(8, 24)
    with pytest.raises(ValueError, match="GPU"):
        mlbs.lbs_deform(torch.zeros(4, dtype=torch.int64), W, None, torch.eye(4).repeat(24, 1, 1), torch.eye(4).repeat(24, 1, 1),
                        torch.zeros(4, 3), torch.eye(3), torch.zeros(3))
