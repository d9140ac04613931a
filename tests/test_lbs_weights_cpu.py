"""CPU tests of the LBS-weight network's torch form (moss_amd.lbs_weights.cross_attention_lbs_torch, the yardstick of the HIP kernels
of csrc/lbs_weight_net.hip) against the reference's own numbers (tests/golden/lbs_weights_*.npz, made by
tests/golden/make_golden_lbs_weights.py from MOSS's CrossAttention_lbs), of the refusals of the fused op, and of the new C ABI symbols."""
import hashlib
import os
import re

import numpy as np
import pytest
import torch

from moss_amd import lbs_weights as mlw
from tests import helpers as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
CASES = ["init", "sharp"]
GRAD_NAMES = ("x", "Rs") + mlw.PARAM_NAMES


def load_case(case, dtype=torch.float64, device="cpu"):
    """(g the case's npz, params {state_dict key: tensor} -- all 20, query.* / key.* scaled as the case says --, x (P,3), Rs (23,3,3),
    cotangent (1,P,24))."""
    g = np.load(os.path.join(GOLDEN_DIR, f"lbs_weights_{case}.npz"))
    stored = np.load(os.path.join(GOLDEN_DIR, "lbs_weights_params.npz"))
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype=dtype, device=device)          # noqa: E731
    scale = float(g["param_scale"])
    params = {k: t(stored[k] * np.float32(scale if k.split(".")[0] in ("query", "key") else 1.0)) for k in stored.files}
    return g, params, t(g["x"]), t(g["Rs"]), t(g["g"])


def _sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(np.asarray(a, dtype=np.float32)).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("case", CASES)
def test_torch_form_matches_the_reference_golden(case):
    """cross_attention_lbs_torch in float64 against the reference's CrossAttention_lbs in float64: out to 1e-12, the gradient of
    <out, g> w.r.t. x, Rs and each of the 16 parameters to float32 rounding of the stored value."""
    g, params, x, Rs, cot = load_case(case)
    assert _sha([g["x"], g["Rs"], g["g"]] + [params[k].numpy() for k in mlw.PARAM_NAMES]) == str(g["inputs_sha256"])
    assert len(params) == 20 and set(params) == set(mlw.PARAM_NAMES) | set(mlw.UNUSED_NAMES)
    P = x.shape[0]
    assert P in (797, 1100) and float(g["preact_err32"]) > 0
    leaves = [x.requires_grad_(True), Rs.requires_grad_(True)] + [params[k].requires_grad_(True) for k in mlw.PARAM_NAMES]
    out = mlw.cross_attention_lbs_torch(params, x[None], Rs)
    assert out.shape == (1, P, 24)
    assert float((out.detach() - torch.from_numpy(g["out"])).abs().max()) < 1e-12
    grads = torch.autograd.grad((out * cot).sum(), leaves)
    for k, gr in zip(GRAD_NAMES, grads):
        assert gr.shape == g[f"grad_{k}"].shape, k
        assert hp.rel_err(gr.numpy(), g[f"grad_{k}"]) < 1e-6, k
    # the sharp case is what its name says: the attention is no longer near-uniform
    spread = float(torch.from_numpy(g["out"]).std(1).max())
    assert spread > (0.03 if case == "sharp" else 0.001)


def test_torch_form_accepts_both_shapes_and_draws_nothing():
    """(P,3) / (1,P,3) and (23,3,3) / (1,23,3,3) give the same bits; the module's forward is the torch form on its own parameters; the
    default generator is left alone; moss_amd/lbs_weights.py holds no device-to-host read and no .cuda() call."""
    g, params, x, Rs, _ = load_case("init", dtype=torch.float32)
    state = torch.random.get_rng_state()
    a = mlw.cross_attention_lbs_torch(params, x, Rs)
    b = mlw.cross_attention_lbs_torch(params, x[None], Rs[None])
    assert torch.equal(state, torch.random.get_rng_state())
    assert a.shape == (1, x.shape[0], 24) and torch.equal(a, b)
    net = mlw.lbs_weight_module()
    assert set(net.state_dict()) == set(params)
    assert [tuple(v.shape) for v in net.state_dict().values()] == [tuple(params[k].shape) for k in net.state_dict()]
    net.load_state_dict(params)
    assert torch.equal(net(x[None], Rs), a)
    assert [tuple(p.shape[:2]) for p in mlw.net_parameters(net)] == list(mlw.PARAM_SHAPES)
    src = open(os.path.join(ROOT, "moss_amd", "lbs_weights.py")).read()
    assert not re.search(r"\.cpu\(|\.item\(|\.tolist\(|\.numpy\(|\.cuda\(", src)


def test_fused_op_refuses_cpu_tensors_and_other_layouts():
    """The product path has no CPU fallback: CPU tensors are refused with the tensor's name (the torch form is
    cross_attention_lbs_torch); a module of another layout is refused before anything else."""
    g, params, x, Rs, _ = load_case("init", dtype=torch.float32)
    net = mlw.lbs_weight_module()
    net.load_state_dict(params)
    with pytest.raises(RuntimeError, match="xyz must be a tensor on a GPU"):
        mlw.cross_attention_lbs_fused(net, x[None], Rs)
    with pytest.raises(ValueError, match="bw_linears.0.weight"):
        mlw.cross_attention_lbs_fused(torch.nn.Linear(3, 24), x[None], Rs)


def test_library_exports_the_lbs_weight_net_symbols(hip_lib):
    """The four entry points are exported, the ABI version is still 7, the two sizes are what the header says, and bad argument
    blocks come back as -1 through moss_last_error()."""
    import ctypes
    from moss_amd._lib import LbsWeightNetArgs, LbsWeightNetBackwardArgs
    for name in ("moss_lbs_weight_net_forward", "moss_lbs_weight_net_backward", "moss_lbs_weight_net_workspace_bytes",
                 "moss_lbs_weight_net_saved_bytes"):
        assert hasattr(hip_lib, name), name
    assert hip_lib.moss_abi_version() == 7
    assert hip_lib.moss_lbs_weight_net_saved_bytes(1000) == 1000 * 640 * 4
    assert hip_lib.moss_lbs_weight_net_saved_bytes(0) == 0 and hip_lib.moss_lbs_weight_net_workspace_bytes(-3) == 0
    assert hip_lib.moss_lbs_weight_net_workspace_bytes(2000) > hip_lib.moss_lbs_weight_net_workspace_bytes(1000) > 64 * 69488 * 4
    a = LbsWeightNetArgs()
    a.P = 5
    assert hip_lib.moss_lbs_weight_net_forward(ctypes.byref(a), None) == -1
    assert b"moss_lbs_weight_net_forward: null x" in hip_lib.moss_last_error()
    a.P = -1
    assert hip_lib.moss_lbs_weight_net_forward(ctypes.byref(a), None) == -1
    assert b"P must be >= 0" in hip_lib.moss_last_error()
    a.P = 0
    assert hip_lib.moss_lbs_weight_net_forward(ctypes.byref(a), None) == 0          # P = 0: a no-op
    b = LbsWeightNetBackwardArgs()
    b.P = 5
    assert hip_lib.moss_lbs_weight_net_backward(ctypes.byref(b), None) == -1
    assert b"moss_lbs_weight_net_backward" in hip_lib.moss_last_error()
    b.P = 0
    assert hip_lib.moss_lbs_weight_net_backward(ctypes.byref(b), None) == 0
    assert hip_lib.moss_lbs_weight_net_forward(None, None) == -1
