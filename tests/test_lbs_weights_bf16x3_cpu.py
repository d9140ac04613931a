"""CPU tests of the split-bf16 (three-product) mode of the LBS-weight network: the torch statement of its arithmetic
(moss_amd.lbs_weights.cross_attention_lbs_torch(operand_dtype=torch.bfloat16, operand_split=True)), the case builder the GPU tests
share (tests/test_gpu_lbs_weights_bf16x3.py), the refusals that need no GPU and the new C ABI symbols.

The cases.  The parameters are the fixtures' (tests/golden/lbs_weights_params.npz, query.* / key.* scaled as the case says); Rs and the
cotangent are drawn as tests/golden/make_golden_lbs_weights.py draws them, from a seed of this file.  2 P candidate points are drawn
uniform in [-1, 1]^3 and the first P are kept whose every pre-activation IN THE FLOAT64 SPLIT FORM is at least 16 x preact_err32_form
from zero, preact_err32_form being the worst pre-activation difference between the float32 and the float64 run of that form on the
candidates: a kernel within K = 8 of float32 accuracy then decides every ReLU as the form does.  Nothing is excluded later.  Beside
every float64 result X of the split form stands err32_form[X]: what the SAME form loses when it runs in float32 -- the bars of the GPU
tests are K times that.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from moss_amd import lbs_weights as mlw
from tests.test_lbs_weights_cpu import CASES, GRAD_NAMES, load_case

SIZES = {"init": (797, 21), "sharp": (1100, 22)}             # case -> (P, seed)
KINK_FACTOR = 16.0
SPLIT = dict(operand_dtype=torch.bfloat16, operand_split=True)
ROUNDED = dict(operand_dtype=torch.bfloat16)
QUANTITIES = ("out",) + GRAD_NAMES


def rotations(rng, n, scale):
    """Rotation matrices from axis-angles of the given scale (Rodrigues), as the fixtures' generator draws them."""
    r = rng.normal(size=(n, 3)) * scale
    th = np.linalg.norm(r, axis=1)[:, None, None]
    k = r / th[:, :, 0]
    Kx = np.zeros((n, 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return (np.eye(3)[None] + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx).astype(np.float32)


def run_form(params, x, Rs, cot, **form):
    """{quantity: tensor}: out and the gradients of <out, cot> w.r.t. x, Rs and the 16 parameters, of the torch form ``form`` in the
    dtype of the arguments (which are left alone)."""
    params = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    x, Rs = x.detach().clone().requires_grad_(True), Rs.detach().clone().requires_grad_(True)
    out = mlw.cross_attention_lbs_torch(params, x[None], Rs, **form)
    grads = torch.autograd.grad((out * cot).sum(), [x, Rs] + [params[k] for k in mlw.PARAM_NAMES])
    return dict(zip(QUANTITIES, [out.detach()] + list(grads)))


def form_on(case, x, Rs, cot):
    """(float64 split form, err32_form) on the given float32 inputs with the case's parameters: the reference of one GPU comparison."""
    p64 = load_case(case)[1]
    p32 = {k: v.float() for k, v in p64.items()}
    f64 = run_form(p64, x.double(), Rs.double(), cot.double(), **SPLIT)
    f32 = run_form(p32, x, Rs, cot, **SPLIT)
    return f64, {k: float((f32[k].double() - f64[k]).abs().max()) for k in QUANTITIES}


@functools.lru_cache(maxsize=None)
def build_case(case):
    """The built case, computed once per process and left unchanged: a dict with ``params`` (float64, all 20), ``x`` (P,3), ``Rs``
    (23,3,3), ``cot`` (1,P,24) as float32 CPU tensors, ``preact_err32_form``, ``rejected_share``, ``form64`` / ``form32`` (the split form's
    runs), ``err32_form`` per quantity, ``exact64`` and ``rounded64`` (the exact network and the rounded-bf16 form in float64)."""
    P, seed = SIZES[case]
    p64 = load_case(case)[1]
    p32 = {k: v.float() for k, v in p64.items()}
    rng = np.random.default_rng(seed)
    cand = torch.from_numpy(rng.uniform(-1, 1, size=(2 * P, 3)).astype(np.float32))
    with torch.no_grad():
        z64 = mlw.preactivations(p64, cand.double(), **SPLIT)
        z32 = mlw.preactivations(p32, cand, **SPLIT)
    preact_err32_form = float((z32.double() - z64).abs().max())
    keep = z64.abs().min(1).values >= KINK_FACTOR * preact_err32_form
    rejected = 1.0 - float(keep.float().mean())
    assert int(keep.sum()) >= P and rejected < 0.25, (case, int(keep.sum()), rejected)
    x = cand[keep][:P].contiguous()
    Rs = torch.from_numpy(rotations(rng, 23, 0.4))
    cot = torch.from_numpy(rng.normal(size=(1, P, 24)).astype(np.float32))
    x64, R64, c64 = x.double(), Rs.double(), cot.double()
    form64 = run_form(p64, x64, R64, c64, **SPLIT)
    form32 = run_form(p32, x, Rs, cot, **SPLIT)
    return {"params": p64, "x": x, "Rs": Rs, "cot": cot, "preact_err32_form": preact_err32_form, "rejected_share": rejected,
            "form64": form64, "form32": form32,
            "err32_form": {k: float((form32[k].double() - form64[k]).abs().max()) for k in QUANTITIES},
            "exact64": run_form(p64, x64, R64, c64), "rounded64": run_form(p64, x64, R64, c64, **ROUNDED)}


def _todays_torch_form(params, xyz, Rs):
    """cross_attention_lbs_torch as it stood before it had operand arguments, statement for statement."""
    x = xyz.reshape(-1, 3)
    e = mlw._embed(x)
    h = e
    for i in range(4):
        h = torch.relu(h @ mlw._matrix(params[f"bw_linears.{i}.weight"]).t() + params[f"bw_linears.{i}.bias"])
        if i == 2:
            h = torch.cat((e, h), -1)
    q0 = h @ mlw._matrix(params["bw_fc.weight"]).t() + params["bw_fc.bias"]
    M = torch.cat([torch.ones(1, 9, dtype=x.dtype, device=x.device), Rs.reshape(-1, 9)], 0)
    Q = q0 @ params["query.weight"].t() + params["query.bias"]
    K = M @ params["key.weight"].t() + params["key.bias"]
    V = M @ params["value.weight"].t() + params["value.bias"]
    att = torch.softmax((Q @ K) / (24 ** 0.5), -1)
    return (att @ V.t())[None]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_defaults_are_todays_function_bit_for_bit(case, dtype):
    """With the defaults (and with them spelled out) cross_attention_lbs_torch gives the bits of the function without the operand
    arguments, out and all 18 gradients, on both fixtures; operand_split without a dtype is refused."""
    g, params, x, Rs, cot = load_case(case, dtype=dtype)
    new = run_form(params, x, Rs, cot)
    spelled = run_form(params, x, Rs, cot, operand_dtype=None, operand_split=False)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    x0, R0 = x.clone().requires_grad_(True), Rs.clone().requires_grad_(True)
    out = _todays_torch_form(leaves, x0[None], R0)
    old = [out.detach()] + list(torch.autograd.grad((out * cot).sum(), [x0, R0] + [leaves[k] for k in mlw.PARAM_NAMES]))
    for k, v in zip(QUANTITIES, old):
        assert torch.equal(new[k], v) and torch.equal(spelled[k], v), k
    with pytest.raises(ValueError, match="operand_split needs operand_dtype"):
        mlw.cross_attention_lbs_torch(params, x, Rs, operand_split=True)


@pytest.mark.parametrize("case", CASES)
def test_case_builder_and_the_forms_own_float32_error(case):
    """The built case: P points off a multiple of 32, fewer than a quarter of the candidates rejected, every float64 split-form
    pre-activation at least 16 x preact_err32_form from zero; err32_form of out and of each of the 18 gradients is positive and finite;
    the float32 run of the split form flips no ReLU against its float64 run."""
    c = build_case(case)
    P = SIZES[case][0]
    assert c["x"].shape == (P, 3) and P % 32 != 0 and c["x"].dtype == torch.float32
    assert 0 < c["preact_err32_form"] < 1e-4 and c["rejected_share"] < 0.25
    p32 = {k: v.float() for k, v in c["params"].items()}
    with torch.no_grad():
        z64 = mlw.preactivations(c["params"], c["x"].double(), **SPLIT)
        z32 = mlw.preactivations(p32, c["x"], **SPLIT)
    assert z64.shape == (P, 512)
    assert float(z64.abs().min()) >= KINK_FACTOR * c["preact_err32_form"]
    assert bool(((z32 > 0) == (z64 > 0)).all())
    print(f"\n{case}: P {P}, preact_err32_form {c['preact_err32_form']:.3g}, rejected {c['rejected_share']:.3f}, err32_form: "
          + ", ".join(f"{k} {v:.3g}" for k, v in c["err32_form"].items()))
    assert set(c["err32_form"]) == set(QUANTITIES) and len(QUANTITIES) == 19
    for k, v in c["err32_form"].items():
        assert np.isfinite(v) and v > 0, k


@pytest.mark.parametrize("case", CASES)
def test_split_form_is_close_and_the_rounded_form_is_not(case):
    """Against the exact float64 network on the built case: the split form's out is at least 100 times closer than the rounded-bf16
    form's, and its ReLU decisions are the exact network's (the rounded form's flips are printed, not asserted)."""
    c = build_case(case)
    x64 = c["x"].double()
    with torch.no_grad():
        z = mlw.preactivations(c["params"], x64)
        zs = mlw.preactivations(c["params"], x64, **SPLIT)
        zr = mlw.preactivations(c["params"], x64, **ROUNDED)
    d_split = float((c["form64"]["out"] - c["exact64"]["out"]).abs().max())
    d_round = float((c["rounded64"]["out"] - c["exact64"]["out"]).abs().max())
    flips = int(((zr > 0) != (z > 0)).sum())
    print(f"\n{case}: out distance from exact float64: split {d_split:.3g}, rounded {d_round:.3g} ({d_round / d_split:.0f} x); "
          f"ReLU flips: split {int(((zs > 0) != (z > 0)).sum())}, rounded {flips}; worst pre-activation difference of the split form "
          f"{float((zs - z).abs().max()):.3g}")
    assert d_split > 0 and 100 * d_split <= d_round
    assert bool(((zs > 0) == (z > 0)).all())


def test_refusals_without_a_gpu():
    """An unknown precision raises ValueError before anything else is looked at (the module, the tensors); CPU tensors with
    precision="bf16x3" are refused with the message of the f32 mode."""
    g, params, x, Rs, _ = load_case("init", dtype=torch.float32)
    net = mlw.lbs_weight_module()
    net.load_state_dict(params)
    with pytest.raises(ValueError, match="precision must be one of"):
        mlw.cross_attention_lbs_fused(None, None, None, precision="bf16")
    with pytest.raises(ValueError, match="precision must be one of"):
        mlw.cross_attention_lbs_fused(net, x[None], Rs, precision="fp32")
    with pytest.raises(RuntimeError, match="xyz must be a tensor on a GPU"):
        mlw.cross_attention_lbs_fused(net, x[None], Rs, precision="bf16x3")
    assert mlw.PRECISIONS == ("f32", "bf16x3")


def test_library_exports_the_bf16x3_symbols(hip_lib):
    """The two entry points are exported, the ABI version is still 7, and bad argument blocks come back as -1 with the entry point's
    own name in moss_last_error(); P = 0 is a no-op."""
    from moss_amd._lib import LbsWeightNetArgs, LbsWeightNetBackwardArgs
    for name in ("moss_lbs_weight_net_forward_bf16x3", "moss_lbs_weight_net_backward_bf16x3"):
        assert hasattr(hip_lib, name), name
    assert hip_lib.moss_abi_version() == 7
    fwd, bwd = hip_lib.moss_lbs_weight_net_forward_bf16x3, hip_lib.moss_lbs_weight_net_backward_bf16x3
    a = LbsWeightNetArgs()
    a.P = 5
    assert fwd(ctypes.byref(a), None) == -1
    assert b"moss_lbs_weight_net_forward_bf16x3: null x" in hip_lib.moss_last_error()
    a.P = -1
    assert fwd(ctypes.byref(a), None) == -1
    assert b"moss_lbs_weight_net_forward_bf16x3: P must be >= 0" in hip_lib.moss_last_error()
    a.P = 0
    assert fwd(ctypes.byref(a), None) == 0
    assert fwd(None, None) == -1 and b"moss_lbs_weight_net_forward_bf16x3: null argument block" in hip_lib.moss_last_error()
    b = LbsWeightNetBackwardArgs()
    b.P = 5
    assert bwd(ctypes.byref(b), None) == -1
    assert b"moss_lbs_weight_net_backward_bf16x3: null Rs" in hip_lib.moss_last_error()
    b.P = -1
    assert bwd(ctypes.byref(b), None) == -1 and b"moss_lbs_weight_net_backward_bf16x3: P must be >= 0" in hip_lib.moss_last_error()
    b.P = 0
    assert bwd(ctypes.byref(b), None) == 0
    assert bwd(None, None) == -1 and b"moss_lbs_weight_net_backward_bf16x3: null argument block" in hip_lib.moss_last_error()
