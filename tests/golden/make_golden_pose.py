#!/usr/bin/env python3
"""Generates tests/golden/pose_head.npz by IMPORTING the reference's own ``Autoregression`` and ``matrix_fisher_nll`` from a MOSS
checkout and running them on the CPU in float64 (the other fixtures' generators are separate and unchanged).

    python tests/golden/make_golden_pose.py <path of a MOSS checkout>

Reference code exercised:
  nets/mlp_delta_body_pose.py   Autoregression (:6-82) and RodriguesModule (:258-284)
  utils/loss_utils.py           matrix_fisher_nll (:283-317), LogMFNormConstant (:222-280) and the quadrature under it (:98-219)

Head cases (``init``, ``trained_small``, ``trained_large``), each keyed <case>_...:
  param_<state_dict key> float32 -- the module's state; ``init`` is the module as constructed (fc_pose uniform +-1e-5, MOSS at
  iteration 1), the other two redraw the fc_pose weights uniform +-1e-2 / +-0.3 with biases a tenth of that
  poses (1,72) uniform +-0.6, target_R (23,3,3) random proper rotations, g_Rs (23,3,3) a cotangent of scale 1e-2 -- all float32,
  run as float64
  Rs (23,3,3), S (23,3) the PROPER singular values, nll (23,) float64; grad_<key> float32 -- the gradient of
  0.06 * nll.mean() + <Rs, g_Rs> w.r.t. every parameter (float64 autograd, rounded once)
General cases (``g1``, ``g5``, ``g20``) for the loss term alone: F (23,3,3) Gaussian of amplitude 1 / 5 / 20 with the last column of
every other matrix negated (both determinant signs), target_R random proper rotations (float32, run as float64); nll (23,) float64
and dF float64 = d nll.mean() / dF.
Beside every float64 result X there is X_err32: the largest absolute difference between the reference run in FLOAT32 on the same
inputs and its float64 run -- what the reference's own single-precision arithmetic loses (for the head gradients one number per
parameter, in PARAM order: <case>_grad_err32 (52,)).  <case>_inputs_sha256: SHA-256 over the float32 bytes of the case's inputs in
a fixed order.  U and V are not stored: they are not unique (Rs is within 1e-5 of a rotation).
"""
import hashlib
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
HEAD_CASES = {"init": (31, None), "trained_small": (32, 1e-2), "trained_large": (33, 0.3)}
GENERAL_CASES = {"g1": (41, 1.0), "g5": (42, 5.0), "g20": (43, 20.0)}
NJ = 23


def _rotations(rng, n):
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 2] *= np.linalg.det(q)[:, None]
    return torch.tensor(q, dtype=torch.float32)


def inputs_checksum(arrays):
    """SHA-256 over the float32 bytes of ``arrays`` (a list, in the order the generator lists them)."""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(np.asarray(a, dtype=np.float32)).tobytes())
    return h.hexdigest()


def _run_head(Autoregression, nll_fn, state, poses, target_R, g_Rs, dtype):
    net = Autoregression(device="cpu").to(dtype)
    net.load_state_dict({k: v.to(dtype) for k, v in state.items()})
    out = net(poses.to(dtype))
    nll = nll_fn(out["Rs"], out["pose_U"], out["pose_S"], out["pose_V"], target_R.to(dtype).contiguous())
    loss = 0.06 * nll.mean() + (out["Rs"] * g_Rs.to(dtype)).sum()
    names = list(state)
    grads = torch.autograd.grad(loss, [dict(net.named_parameters())[k] for k in names])
    with torch.no_grad():
        sign = torch.det(out["pose_U"] @ out["pose_V"].transpose(1, 2))
        S = out["pose_S"].clone()
        S[:, 2] *= sign
    return out["Rs"].detach(), S, nll.detach(), dict(zip(names, grads))


def _run_general(nll_fn, F, target_R, dtype):
    F = F.to(dtype).clone().requires_grad_(True)
    U, S, V = torch.svd(F)
    nll = nll_fn(F, U, S, V, target_R.to(dtype).contiguous())
    (dF,) = torch.autograd.grad(nll.mean(), F)
    return nll.detach(), dF


def _err(a32, a64):
    return np.float64((a32.double() - a64).abs().max().item())


def main(moss_root):
    sys.path.insert(0, moss_root)
    from nets.mlp_delta_body_pose import Autoregression
    from utils.loss_utils import matrix_fisher_nll
    res = {}
    torch.manual_seed(20261016)
    base = Autoregression(device="cpu")                                   # (the module as constructed: float32)
    for case, (seed, amp) in HEAD_CASES.items():
        rng = np.random.Generator(np.random.PCG64(seed))
        state = {k: v.detach().clone() for k, v in base.state_dict().items()}
        if amp is not None:
            for k in state:
                if k.startswith("fc_pose."):
                    a = amp if k.endswith("weight") else 0.1 * amp
                    state[k] = torch.tensor(rng.uniform(-a, a, size=tuple(state[k].shape)), dtype=torch.float32)
        poses = torch.tensor(rng.uniform(-0.6, 0.6, size=(1, 72)), dtype=torch.float32)
        target_R = _rotations(rng, NJ)
        g_Rs = torch.tensor(1e-2 * rng.normal(size=(NJ, 3, 3)), dtype=torch.float32)
        Rs, S, nll, grads = _run_head(Autoregression, matrix_fisher_nll, state, poses, target_R, g_Rs, torch.float64)
        Rs32, S32, nll32, grads32 = _run_head(Autoregression, matrix_fisher_nll, state, poses, target_R, g_Rs, torch.float32)
        for k, v in state.items():
            res[f"{case}_param_{k}"] = v.numpy()
            res[f"{case}_grad_{k}"] = grads[k].to(torch.float32).numpy()
        res[f"{case}_poses"], res[f"{case}_target_R"], res[f"{case}_g_Rs"] = poses.numpy(), target_R.numpy(), g_Rs.numpy()
        res[f"{case}_Rs"], res[f"{case}_S"], res[f"{case}_nll"] = Rs.numpy(), S.numpy(), nll.numpy()
        res[f"{case}_Rs_err32"], res[f"{case}_S_err32"], res[f"{case}_nll_err32"] = _err(Rs32, Rs), _err(S32, S), _err(nll32, nll)
        res[f"{case}_grad_err32"] = np.array([_err(grads32[k], grads[k]) for k in state])
        res[f"{case}_inputs_sha256"] = np.array(inputs_checksum([v.numpy() for v in state.values()] + [poses, target_R, g_Rs]))
        rel = max(float((grads32[k].double() - grads[k]).norm() / grads[k].norm()) for k in state)
        print(f"{case}: S in [{float(S.min()):.9f}, {float(S.max()):.9f}], nll err32 {res[f'{case}_nll_err32']:.3g}, "
              f"S err32 {res[f'{case}_S_err32']:.3g}, worst gradient relative L2 err32 {rel:.3g}")
    for case, (seed, amp) in GENERAL_CASES.items():
        rng = np.random.Generator(np.random.PCG64(seed))
        F = torch.tensor(amp * rng.normal(size=(NJ, 3, 3)), dtype=torch.float32)
        F[1::2, :, 2] *= -1
        target_R = _rotations(rng, NJ)
        nll, dF = _run_general(matrix_fisher_nll, F, target_R, torch.float64)
        nll32, dF32 = _run_general(matrix_fisher_nll, F, target_R, torch.float32)
        assert bool(torch.isfinite(nll).all() and torch.isfinite(dF).all())
        res[f"{case}_F"], res[f"{case}_target_R"] = F.numpy(), target_R.numpy()
        res[f"{case}_nll"], res[f"{case}_dF"] = nll.numpy(), dF.numpy()
        res[f"{case}_nll_err32"], res[f"{case}_dF_err32"] = _err(nll32, nll), _err(dF32, dF)
        res[f"{case}_inputs_sha256"] = np.array(inputs_checksum([F, target_R]))
        S = torch.linalg.svdvals(F.double())
        print(f"{case}: S up to {float(S.max()):.3g}, smallest gap {float((S[:, :2] - S[:, 1:]).min()):.3g}, "
              f"{int((torch.det(F.double()) < 0).sum())} negative determinants, nll {float(nll.min()):.3g} .. {float(nll.max()):.3g} "
              f"(err32 {res[f'{case}_nll_err32']:.3g}), dF err32 {res[f'{case}_dF_err32']:.3g}")
    path = os.path.join(OUT, "pose_head.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))
