"""CPU tests of the bf16-operand mode of the LPIPS term (``LpipsVGG(precision="bf16")``, C ABI ``moss_lpips_vgg_forward_bf16`` /
``_backward_bf16`` / ``_pack_weights_bf16``): the header and the Python wiring, the torch yardstick
``lpips_vgg_torch(..., operand_dtype=torch.bfloat16)``, and the yardstick's own float32 spread on the inputs the GPU bar of
tests/test_gpu_lpips_bf16.py is taken on.

The bf16-operand form rounds both operands of convolutions 2..13 to bf16 in the forward and in the data gradient and sums exactly in
the tensors' dtype: in float64 it is the exact statement of what the kernels compute.  Rounding turns a last-bit float32 difference
into a whole bf16 step, so the float32 runs of that form scatter more than those of the plain form, heavy-tailed on tiny images:
``bf16_err32`` measures four of them (contiguous / channels-last, one / four CPU threads -- the CPU convolutions split their sums by
team size) and the test below demands that no run is more than K = 8 from the largest of the other three, i.e. that err32 is a
number and not an accident of one run."""
import functools
import inspect
import os

import pytest
import torch

from moss_amd import lpips as mlp
from tests.test_lpips_cpu import ROOT, load_case, run_torch, weights

K = 8.0
BF16 = torch.bfloat16
MEASURES = ("value", "grad_max", "grad_l2")
GPU_INPUTS = ("odd", "person101x77", "person256x128")          # the inputs of the GPU bar
CAPACITY_INPUT = "rand29x37"                                   # and of the same bar under a capacity (uniform noise, 29 x 37)


def person_crop(H, W, seed=7):
    """``_person_crop`` of tests/test_gpu_lpips.py (a smooth figure on a black ground with fine texture; the render is the ground truth
    plus low-frequency error and noise), imported lazily: that module is marked ``gpu`` as a whole but the helper is plain numpy."""
    from tests.test_gpu_lpips import _person_crop
    return _person_crop(H, W, seed)


@functools.lru_cache(maxsize=None)
def images(name):
    """(x, y) float32 CPU tensors (3,H,W) of a named input."""
    if name.startswith("person"):
        H, W = (int(v) for v in name[len("person"):].split("x"))
        return person_crop(H, W)
    if name.startswith("rand"):
        H, W = (int(v) for v in name[len("rand"):].split("x"))
        gen = torch.Generator().manual_seed(11)
        return torch.rand(3, H, W, generator=gen), torch.rand(3, H, W, generator=gen)
    x, y, _ = load_case(name, dtype=torch.float32)
    return x, y


def run_bf16(params, x, y, channels_last=False):
    """``run_torch`` of tests/test_lpips_cpu.py for the bf16-operand form: (terms (5,), total (), dL/dx (3,H,W)), detached."""
    x, y = x.clone()[None], y.clone()[None]
    if channels_last:
        x, y = x.contiguous(memory_format=torch.channels_last), y.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    total, terms = mlp.lpips_vgg_torch(params, x, y, return_terms=True, operand_dtype=BF16)
    (grad,) = torch.autograd.grad(total.sum(), x)
    return terms.detach(), total.detach().reshape(()), grad[0].contiguous()


def errors(run, ref):
    """The file's three measures of (terms, total, grad) against a float64 (terms, total, grad)."""
    (t, v, g), (t64, v64, g64) = run, ref
    d = g.double() - g64
    return {"value": max(float((t.double() - t64).abs().max()), abs(float(v) - float(v64))), "grad_max": float(d.abs().max()),
            "grad_l2": float(d.norm())}


@functools.lru_cache(maxsize=None)
def bf16_reference(name):
    """The bf16-operand form in float64 on the CPU: (terms, total, grad).  Computed once per process, never modified."""
    x, y = images(name)
    return run_bf16(mlp.cast_params(weights(), torch.float64), x.double(), y.double())


@functools.lru_cache(maxsize=None)
def bf16_err32(name):
    """The four float32 runs of the bf16-operand form against its float64 run: a list of four {measure: error}."""
    x, y = images(name)
    ref, runs = bf16_reference(name), []
    threads = torch.get_num_threads()
    try:
        for n in (1, 4):
            torch.set_num_threads(n)
            for cl in (False, True):
                runs.append(errors(run_bf16(weights(), x, y, channels_last=cl), ref))
    finally:
        torch.set_num_threads(threads)
    return runs


def bf16_record(name):
    """The record tests/test_gpu_lpips.py's ``_ratios`` takes: the float64 bf16-operand run and err32 = the largest of the four."""
    t64, v64, g64 = bf16_reference(name)
    runs = bf16_err32(name)
    return {"terms": t64.numpy(), "total": float(v64), "grad": g64.numpy(), "value_err32": max(r["value"] for r in runs),
            "grad_err32_max": max(r["grad_max"] for r in runs), "grad_err32_l2": max(r["grad_l2"] for r in runs)}


# ---- header and wiring ---------------------------------------------------------------------------------------------------------------

def test_c_abi_declares_the_bf16_entry_points():
    text = open(os.path.join(ROOT, "include", "moss_raster.h")).read()
    for name in ("moss_lpips_vgg_forward_bf16", "moss_lpips_vgg_backward_bf16", "moss_lpips_vgg_pack_weights_bf16"):
        assert name + "(" in text, name
    assert "#define MOSS_ABI_VERSION 7" in text
    from moss_amd import _lib
    assert _lib.ABI_VERSION == 7
    src = inspect.getsource(_lib._declare)
    for name in ("moss_lpips_vgg_forward_bf16", "moss_lpips_vgg_backward_bf16", "moss_lpips_vgg_pack_weights_bf16"):
        assert f"lib.{name}.argtypes" in src, name


def test_signatures_default_to_float32():
    for fn in (mlp.LpipsVGG.__init__, mlp.LpipsVGG.from_tensors, mlp.LpipsVGG.from_module):
        assert inspect.signature(fn).parameters["precision"].default == "f32", fn
    assert inspect.signature(mlp.lpips_vgg_torch).parameters["operand_dtype"].default is None
    assert mlp.PRECISIONS == ("f32", "bf16")


def test_unknown_precision_is_refused():
    """Before the device check: the refusal needs no GPU."""
    p = weights()
    args = (p["conv_weights"], p["conv_biases"], p["lin_weights"], p["shift"], p["scale"])
    for bad in ("fp16", "BF16", None, 32):
        with pytest.raises(ValueError, match="precision must be one of"):
            mlp.LpipsVGG.from_tensors(*args, precision=bad)
        with pytest.raises(ValueError, match="precision must be one of"):
            mlp.LpipsVGG(*args, precision=bad)
    with pytest.raises(RuntimeError, match="must be on a GPU"):                     # a known one goes on to the device check
        mlp.LpipsVGG.from_tensors(*args, precision="bf16")


def test_evaluate_views_refuses_a_bf16_net():
    """A host-side check before any device call: nothing else of the arguments is looked at."""
    from moss_amd.metrics import evaluate_views
    net = object.__new__(mlp.LpipsVGG)
    net.precision = "bf16"
    with pytest.raises(ValueError, match="float32 term"):
        evaluate_views(None, [], [], None, None, lpips=net)


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------

def test_operand_dtype_none_is_the_present_function():
    x, y, _ = load_case("odd")
    p64 = mlp.cast_params(weights(), torch.float64)
    a = run_torch(p64, x, y)
    xx = x.clone()[None].requires_grad_(True)
    total, terms = mlp.lpips_vgg_torch(p64, xx, y[None], return_terms=True, operand_dtype=None)
    (grad,) = torch.autograd.grad(total.sum(), xx)
    assert torch.equal(terms, a[0]) and torch.equal(total.reshape(()), a[1]) and torch.equal(grad[0], a[2])
    assert torch.equal(mlp.lpips_vgg_torch(p64, x, y), total.detach())


def test_bf16_operands_in_float64():
    """Not the plain form (relative value difference between 1e-5 and 1e-1), bit-reproducible, and conv 1_1 untouched: rounding the
    images themselves to bf16 changes the result, so the first layer's operands are not rounded."""
    x, y, _ = load_case("odd")
    p64 = mlp.cast_params(weights(), torch.float64)
    plain = run_torch(p64, x, y)
    a, b = run_bf16(p64, x, y), run_bf16(p64, x, y)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    rel = abs(float(a[1]) - float(plain[1])) / float(plain[1])
    print(f"bf16 operands, odd: relative value difference {rel:.3g}, gradient relative L2 {float((a[2] - plain[2]).norm() / plain[2].norm()):.3g}")
    assert 1e-5 < rel < 1e-1
    assert not torch.equal(a[2], plain[2])
    assert a[0].dtype == torch.float64 and a[2].dtype == torch.float64


def test_bf16_operands_same_image_is_exactly_zero():
    x, _, _ = load_case("same")
    for dtype in (torch.float64, torch.float32):
        terms, total, grad = run_bf16(mlp.cast_params(weights(), dtype), x.to(dtype), x.to(dtype))
        assert float(total) == 0.0 and not terms.any() and not grad.any()


def test_rounded_conv_rounds_the_gradient_operands():
    """The backward of the rounded convolution is conv2d_input of the ROUNDED gradient with the ROUNDED weight (a plain ``.to(bfloat16)``
    would pass the gradient through unrounded)."""
    gen = torch.Generator().manual_seed(0)
    h = torch.randn(1, 4, 6, 5, generator=gen, dtype=torch.float64).requires_grad_(True)
    w, b = torch.randn(3, 4, 3, 3, generator=gen, dtype=torch.float64), torch.randn(3, generator=gen, dtype=torch.float64)
    g = torch.randn(1, 3, 6, 5, generator=gen, dtype=torch.float64)
    r = lambda t: t.to(BF16).double()                                                # noqa: E731
    out = mlp._RoundedOperandConv.apply(h, w, b, BF16)
    assert torch.equal(out, torch.nn.functional.conv2d(r(h.detach()), r(w), b, padding=1))
    (dh,) = torch.autograd.grad(out, h, g)
    assert torch.equal(dh, torch.nn.grad.conv2d_input(h.shape, r(w), r(g), padding=1))
    assert not torch.equal(dh, torch.nn.grad.conv2d_input(h.shape, r(w), g, padding=1))


# ---- the yardstick's own spread ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", GPU_INPUTS + (CAPACITY_INPUT,))
def test_float32_runs_of_the_bf16_form_agree(name):
    """Each of the four float32 runs within K of the largest of the other three, in each measure: the condition under which err32
    of this input can carry the GPU bar.  An input that fails it is replaced, K is not widened."""
    runs = bf16_err32(name)
    ref = bf16_reference(name)
    assert float(ref[1]) > 1e-6
    for m in MEASURES:
        vals = [r[m] for r in runs]
        assert min(vals) > 0, (name, m, vals)
        worst = max(v / max(vals[:i] + vals[i + 1:]) for i, v in enumerate(vals))
        print(f"bf16 yardstick {name} {m}: float32 runs {['%.3g' % v for v in vals]}, max / min {max(vals) / min(vals):.2f}, "
              f"worst run / largest of the others {worst:.2f}")
        assert worst <= K, (name, m, vals)
