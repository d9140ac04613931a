"""CPU tests of the split-bf16 (three-product) mode of the LPIPS term (``LpipsVGG(precision="bf16x3")``, C ABI
``moss_lpips_vgg_forward_bf16x3`` / ``_backward_bf16x3`` / ``_pack_weights_bf16x3`` / ``moss_lpips_vgg_conv3x3_bf16x3``): the header and the
Python wiring, the torch yardstick ``lpips_vgg_torch(..., operand_dtype=torch.bfloat16, operand_split=True)``, the derived per-element
bound of the split sum, and the references the GPU files (tests/test_gpu_lpips_bf16x3.py, tests/test_gpu_lpips_conv_layer_bf16x3.py)
judge the kernels by.

The split form: hi(a) = bf16(a), lo(a) = bf16(a - hi(a)), and every product a b of convolutions 2..13, forward and data gradient, is
lo(a) hi(b) + hi(a) lo(b) + hi(a) hi(b).  It equals ONE plain convolution over 3 Cin channels -- inputs [lo, hi, hi] against weights
[hi, lo, hi] -- which is how the per-layer float64 reference and its mass are built here.  The bar of the split sum against the
unsplit one is 2^-16 of mass = conv(|in|, |w|) + |bias| on every element.  (One product alone can be off by more: |lo| <= 2^-8 |a| and
|a - hi - lo| <= 2^-17 |a|, so a b loses at most 2 * 2^-17 + 2^-16 = 2^-15 |a b|; a sum of hundreds of products whose roundings are
not all at their worst stays well inside 2^-16 of its mass.  The bar is kept at 2^-16, the stricter figure.)"""
import ctypes
import functools
import inspect
import os

import pytest
import torch
import torch.nn.functional as F

from moss_amd import lpips as mlp
from tests.test_lpips_bf16_cpu import BF16, CAPACITY_INPUT, K, MEASURES, bf16_reference, errors, images
from tests.test_lpips_conv_layer_cpu import FAKE, SMALL, _block, _operands, sequential_float32
from tests.test_lpips_cpu import ROOT, load_case, run_torch, weights

GPU_INPUTS = ("odd", "person101x77")                       # the inputs of the GPU bar: every layer in the 32-row shape
NAMES = ("moss_lpips_vgg_forward_bf16x3", "moss_lpips_vgg_backward_bf16x3", "moss_lpips_vgg_pack_weights_bf16x3",
         "moss_lpips_vgg_conv3x3_bf16x3")
SPLIT_BOUND = 2.0 ** -16                                   # of the mass: see above, not a measured number


# ---- one layer: the split form as a plain convolution over 3 Cin channels -------------------------------------------------------------

def split(t):
    """(hi, lo) of a float32 tensor, as float32 (the subtraction is exact)."""
    hi = t.bfloat16().float()
    return hi, (t - hi).bfloat16().float()


def concatenated(mode, x, w):
    """(xcat (N,3C,H,W), wcat) float32: inputs [lo, hi, hi] against weights [hi, lo, hi].  ``w`` is the FORWARD layer's (cout_f,cin_f,3,3);
    a data gradient is conv_transpose2d, whose weight has the input channels first."""
    xh, xl = split(x)
    wh, wl = split(w)
    return torch.cat([xl, xh, xh], 1), torch.cat([wh, wl, wh], 1 if mode == "fwd" else 0)


def k_interleaved(mode, xcat, wcat):
    """The same operands with the 3 C channels reordered into the kernels' k order: per sixteen channels lo hi, hi lo, hi hi."""
    C = xcat.shape[1] // 3
    idx = torch.arange(3 * C).reshape(3, C // 16, 16).permute(1, 0, 2).reshape(-1)
    return xcat[:, idx], (wcat[:, idx] if mode == "fwd" else wcat[idx])


def _conv(mode, x, w, bias=None):
    return F.conv2d(x, w, bias, padding=1) if mode == "fwd" else F.conv_transpose2d(x, w, padding=1)


@functools.lru_cache(maxsize=None)
def split_layer_reference(mode, cin, cout, nimg, H, W):
    """``reference`` of tests/test_lpips_conv_layer_cpu.py for the split form, on that file's inputs: {x, w, bias float32, z64 the float64
    split result before any ReLU or mask, mass of the concatenated operands, e32}.  e32: the worst |z32 - z64| / mass of torch's
    float32 convolution of the concatenated operands, contiguous and channels-last, and, at 5 x 7, of one sequential float32 sum per
    element in the kernels' k-interleaved order (at other sizes the 5 x 7 figure of the same layer enters)."""
    x, _, _, w, bias = _operands(mode, cin, cout, nimg, H, W, False)
    b = bias if mode == "fwd" else None
    xcat, wcat = concatenated(mode, x, w)
    z64 = _conv(mode, xcat.double(), wcat.double(), None if b is None else b.double())
    mass = _conv(mode, xcat.double().abs(), wcat.double().abs(), None if b is None else b.double().abs())
    assert float(mass.min()) > 0.0
    e32 = 0.0
    for cl in (False, True):
        xi = xcat.contiguous(memory_format=torch.channels_last) if cl else xcat
        wi = wcat.contiguous(memory_format=torch.channels_last) if cl else wcat
        e32 = max(e32, float(((_conv(mode, xi, wi, b).double() - z64).abs() / mass).max()))
    if (H, W) == SMALL:
        xi, wi = k_interleaved(mode, xcat, wcat)
        w_corr = wi if mode == "fwd" else wi.flip(2, 3).transpose(0, 1).contiguous()
        e32 = max(e32, float(((sequential_float32(xi.contiguous(), w_corr, b).double() - z64).abs() / mass).max()))
    else:
        e32 = max(e32, split_layer_reference(mode, cin, cout, 2 if mode == "fwd" else 1, SMALL[0], SMALL[1])["e32"])
    assert e32 > 0.0
    return {"x": x, "w": w, "bias": bias, "z64": z64, "mass": mass, "e32": e32}


@pytest.mark.parametrize("cin, cout", [(64, 64), (512, 512)])
def test_split_layer_in_float64(cin, cout):
    """5 x 7, forward and data gradient: the yardstick's split convolution is the 3 Cin concatenated one (to float64 summation order:
    n 2^-53 of the mass, n = 27 Cin products), and it lies within 2^-16 x mass of the unsplit float64 convolution on every element."""
    H, W = SMALL
    x, _, _, w, bias = _operands("fwd", cin, cout, 2, H, W, False)
    g = _operands("bwd_plain", cout, cin, 2, H, W, False)[0]                # a gradient for the same layer: (2,cout,H,W)
    ref = split_layer_reference("fwd", cin, cout, 2, H, W)
    h = x.double().requires_grad_(True)
    out = mlp._SplitOperandConv.apply(h, w.double(), bias.double(), BF16)
    (dh,) = torch.autograd.grad(out, h, g.double())
    order64 = 27 * max(cin, cout) * 2.0 ** -53
    same = float(((out.detach() - ref["z64"]).abs() / ref["mass"]).max())
    gcat, wcat = concatenated("bwd_plain", g, w)
    dz64 = F.conv_transpose2d(gcat.double(), wcat.double(), padding=1)
    dmass = F.conv_transpose2d(gcat.double().abs(), wcat.double().abs(), padding=1)
    dsame = float(((dh - dz64).abs() / dmass).max())
    plain = F.conv2d(x.double(), w.double(), bias.double(), padding=1)
    pmass = F.conv2d(x.double().abs(), w.double().abs(), bias.double().abs(), padding=1)
    dplain = F.conv_transpose2d(g.double(), w.double(), padding=1)
    dpmass = F.conv_transpose2d(g.double().abs(), w.double().abs(), padding=1)
    fwd_err = float(((ref["z64"] - plain).abs() / pmass).max())
    bwd_err = float(((dz64 - dplain).abs() / dpmass).max())
    print(f"split conv {cin}->{cout}: against the concatenated form {same:.3g} / {dsame:.3g} of the mass (float64 order {order64:.3g}); against "
          f"the unsplit convolution {fwd_err / SPLIT_BOUND:.3f} / {bwd_err / SPLIT_BOUND:.3f} of 2^-16 mass; E32 "
          f"{ref['e32'] / 2.0 ** -24:.2f} roundoffs")
    assert same <= order64 and dsame <= order64
    assert 0 < fwd_err <= SPLIT_BOUND and 0 < bwd_err <= SPLIT_BOUND


def test_split_subtraction_is_exact():
    """a - hi(a) in float32 is the float64 difference, so lo is the rounding of the true remainder; |lo| <= 2^-8 |a| (half an ulp of
    eight bits) and hi + lo is within 2^-17 |a| (half an ulp of lo, whose exponent is at least nine below a's)."""
    gen = torch.Generator().manual_seed(5)
    a = torch.randn(100000, generator=gen) * torch.exp(8 * torch.randn(100000, generator=gen))
    hi, lo = split(a)
    assert torch.equal((a - hi).double(), a.double() - hi.double())
    assert bool((lo.double().abs() <= 2.0 ** -8 * a.double().abs()).all())
    assert bool(((a.double() - hi.double() - lo.double()).abs() <= 2.0 ** -17 * a.double().abs()).all())
    mh, ml = mlp.split_operand(a, BF16)
    assert torch.equal(mh, hi) and torch.equal(ml, lo)


# ---- the whole term: references shared with the GPU file -----------------------------------------------------------------------------

def run_split(params, x, y, channels_last=False):
    """``run_bf16`` of tests/test_lpips_bf16_cpu.py for the split form: (terms (5,), total (), dL/dx (3,H,W)), detached."""
    x, y = x.clone()[None], y.clone()[None]
    if channels_last:
        x, y = x.contiguous(memory_format=torch.channels_last), y.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    total, terms = mlp.lpips_vgg_torch(params, x, y, return_terms=True, operand_dtype=BF16, operand_split=True)
    (grad,) = torch.autograd.grad(total.sum(), x)
    return terms.detach(), total.detach().reshape(()), grad[0].contiguous()


@functools.lru_cache(maxsize=None)
def split_reference(name):
    """The split form in float64 on the CPU: (terms, total, grad).  Computed once per process, never modified."""
    x, y = images(name)
    return run_split(mlp.cast_params(weights(), torch.float64), x.double(), y.double())


@functools.lru_cache(maxsize=None)
def exact_reference(name):
    """The exact float64 term: (terms, total, grad), from the fixture where there is one."""
    if name.startswith("person") or name.startswith("rand"):
        x, y = images(name)
        return run_torch(mlp.cast_params(weights(), torch.float64), x.double(), y.double())
    rec = load_case(name)[2]
    return torch.from_numpy(rec["terms"]), torch.tensor(float(rec["total"]), dtype=torch.float64), torch.from_numpy(rec["grad"]).double()


@functools.lru_cache(maxsize=None)
def split_err32(name):
    """The four float32 runs of the split form (contiguous / channels-last, 1 / 4 threads) against its float64 run."""
    x, y = images(name)
    ref, runs = split_reference(name), []
    threads = torch.get_num_threads()
    try:
        for n in (1, 4):
            torch.set_num_threads(n)
            for cl in (False, True):
                runs.append(errors(run_split(weights(), x, y, channels_last=cl), ref))
    finally:
        torch.set_num_threads(threads)
    return runs


def split_record(name):
    """The record tests/test_gpu_lpips.py's ``_ratios`` takes: the float64 split run and err32 = the largest of the four."""
    t64, v64, g64 = split_reference(name)
    runs = split_err32(name)
    return {"terms": t64.numpy(), "total": float(v64), "grad": g64.numpy(), "value_err32": max(r["value"] for r in runs),
            "grad_err32_max": max(r["grad_max"] for r in runs), "grad_err32_l2": max(r["grad_l2"] for r in runs)}


# ---- header and wiring ---------------------------------------------------------------------------------------------------------------

def test_c_abi_declares_the_split_entry_points():
    text = open(os.path.join(ROOT, "include", "moss_raster.h")).read()
    for name in NAMES:
        assert name + "(" in text, name
        assert text.index(name + "(") < text.index("#ifdef MOSS_DIAG")
    assert "#define MOSS_ABI_VERSION 7" in text
    assert "hi(a) hi(b) + hi(a) lo(b) + lo(a) hi(b)" in text and "2^-126" in text        # the arithmetic and the flush are documented
    from moss_amd import _lib
    assert _lib.ABI_VERSION == 7
    src = inspect.getsource(_lib._declare)
    for name in NAMES:
        assert f"lib.{name}.argtypes" in src and f"lib.{name}.restype" in src, name


def test_precisions():
    assert mlp.PRECISIONS == ("f32", "bf16")
    assert mlp.ALL_PRECISIONS == ("f32", "bf16", "bf16x3")
    assert mlp._SUFFIX["bf16x3"] == "_bf16x3"
    sig = inspect.signature(mlp.lpips_vgg_torch).parameters
    assert sig["operand_split"].default is False and sig["operand_dtype"].default is None
    p = weights()
    args = (p["conv_weights"], p["conv_biases"], p["lin_weights"], p["shift"], p["scale"])
    for make in (mlp.LpipsVGG, mlp.LpipsVGG.from_tensors):
        with pytest.raises(RuntimeError, match="must be on a GPU"):                 # a known precision goes on to the device check
            make(*args, precision="bf16x3")
        for bad in ("fp16", "BF16x3"):
            with pytest.raises(ValueError, match="precision must be one of"):
                make(*args, precision=bad)


def test_evaluate_views_refuses_a_split_net():
    """(Passes without the split mode as well: the metric refuses every net that is not float32.  It records the decision.)"""
    from moss_amd.metrics import evaluate_views
    net = object.__new__(mlp.LpipsVGG)
    net.precision = "bf16x3"
    with pytest.raises(ValueError, match="float32 term"):
        evaluate_views(None, [], [], None, None, lpips=net)


def _refused(hip_lib, block, text):
    rc = hip_lib.moss_lpips_vgg_conv3x3_bf16x3(ctypes.byref(block) if block is not None else None, None)
    msg = hip_lib.moss_last_error().decode()
    assert rc == -1, (rc, msg, text)                                      # MOSS_ERR_INVALID_ARG
    assert msg.startswith("moss_lpips_vgg_conv3x3_bf16x3:") and text in msg, (msg, text)


def test_layer_entry_point_refusals(hip_lib):
    """The list of tests/test_lpips_conv_layer_cpu.py's test_refusals under the new name, and bf16 != 0; before any launch."""
    _refused(hip_lib, None, "null argument block")
    for field in ("in_", "weights", "out"):
        _refused(hip_lib, _block(**{field: None}), "null in, weights or out")
    _refused(hip_lib, _block(bias=None), "needs bias")
    _refused(hip_lib, _block(mode=1, mask_in=None), "needs mask_in")
    for field in ("cin", "cout"):
        for v in (0, -64, 32, 96, 65):
            _refused(hip_lib, _block(**{field: v}), "multiples of 64")
    for v in (-1, 3):
        _refused(hip_lib, _block(mode=v), "mode must be")
        _refused(hip_lib, _block(shape=v), "shape must be")
    for v in (-1, 1, 2):
        _refused(hip_lib, _block(bf16=v), "bf16 must be 0")
    for v in (0, 3, -1):
        _refused(hip_lib, _block(nimg=v), "nimg must be")
    for field in ("H", "W"):
        for v in (0, -5):
            _refused(hip_lib, _block(**{field: v}), ">= 1")
    _refused(hip_lib, _block(cap_H=48, cap_W=64), "needs rect")
    _refused(hip_lib, _block(cap_H=48, rect=FAKE), "both be set")
    _refused(hip_lib, _block(cap_W=64, rect=FAKE), "both be set")
    _refused(hip_lib, _block(cap_H=15, cap_W=64, rect=FAKE), "capacity must be >= 16")
    _refused(hip_lib, _block(cap_H=48, cap_W=64, rect=FAKE, level=5), "level must be")
    _refused(hip_lib, _block(cap_H=48, cap_W=64, rect=FAKE, level=-1), "level must be")
    assert hip_lib.moss_lpips_vgg_pack_weights_bf16x3(64, 64, None, None, None, None) == -1
    assert hip_lib.moss_last_error().decode().startswith("moss_lpips_vgg_pack_weights_bf16x3:")


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------

def test_operand_split_false_is_the_present_function():
    """Bit for bit, with and without rounded operands."""
    x, y, _ = load_case("odd")
    p64 = mlp.cast_params(weights(), torch.float64)
    for dtype, want in ((None, run_torch(p64, x, y)), (BF16, bf16_reference("odd"))):
        xx = x.double().clone()[None].requires_grad_(True)
        total, terms = mlp.lpips_vgg_torch(p64, xx, y.double()[None], return_terms=True, operand_dtype=dtype, operand_split=False)
        (grad,) = torch.autograd.grad(total.sum(), xx)
        assert torch.equal(terms, want[0]) and torch.equal(total.reshape(()), want[1]) and torch.equal(grad[0], want[2])
    with pytest.raises(ValueError, match="operand_split needs operand_dtype"):
        mlp.lpips_vgg_torch(p64, x, y, operand_split=True)


def test_split_same_image_is_exactly_zero():
    x, _, _ = load_case("same")
    for dtype in (torch.float64, torch.float32):
        terms, total, grad = run_split(mlp.cast_params(weights(), dtype), x.to(dtype), x.to(dtype))
        assert float(total) == 0.0 and not terms.any() and not grad.any()


@pytest.mark.parametrize("name", GPU_INPUTS)
def test_split_form_is_closer_to_float64_than_the_bf16_form(name):
    """In float64, against the exact term: the split form's value and gradient-L2 distances are smaller than the bf16-operand form's
    (measured with synthetic weights: 20x to 5 000x smaller)."""
    exact = exact_reference(name)
    s, b = errors(split_reference(name), exact), errors(bf16_reference(name), exact)
    print(f"split form {name}: distance from float64, split / bf16 form: " + ", ".join(f"{m} {s[m]:.3g} / {b[m]:.3g}" for m in MEASURES)
          + f"; relative: value {s['value'] / float(exact[1]):.3g}, gradient L2 {s['grad_l2'] / float(exact[2].norm()):.3g}")
    assert s["value"] < b["value"] and s["grad_l2"] < b["grad_l2"]


@pytest.mark.parametrize("name", GPU_INPUTS + (CAPACITY_INPUT,))
def test_float32_runs_of_the_split_form_agree(name):
    """Each of the four float32 runs within K of the largest of the other three, in each measure: the condition under which err32 of
    this input can carry the GPU bar."""
    runs = split_err32(name)
    assert float(split_reference(name)[1]) > 1e-6
    for m in MEASURES:
        vals = [r[m] for r in runs]
        assert min(vals) > 0, (name, m, vals)
        worst = max(v / max(vals[:i] + vals[i + 1:]) for i, v in enumerate(vals))
        print(f"split yardstick {name} {m}: float32 runs {['%.3g' % v for v in vals]}, worst run / largest of the others {worst:.2f}")
        assert worst <= K, (name, m, vals)
