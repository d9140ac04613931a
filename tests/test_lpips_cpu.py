"""CPU tests of the LPIPS term's torch form (moss_amd.lpips.lpips_vgg_torch, the yardstick of the HIP kernels of csrc/lpips.hip) against
the reference's own numbers (tests/golden/lpips_vgg.npz, made by tests/golden/make_golden_lpips.py from lpipsPyTorch's VGG16, LinLayers
and LPIPS.forward), of the weight discovery of LpipsVGG.from_module, and of the refusals of the fused op.

The weights are not stored: 14.7 M values from ``numpy.random.RandomState(seed)`` (moss_amd.lpips.synthetic_weights), rebuilt once per
session here; the fixture holds their SHA-256."""
import functools
import os

import numpy as np
import pytest
import torch
from torch import nn

from moss_amd import lpips as mlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lpips_vgg.npz")
CASES = ["min", "odd", "strip", "same"]
SIZES = {"min": (16, 16), "odd": (37, 53), "strip": (16, 40), "same": (20, 28)}


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(GOLDEN)


@functools.lru_cache(maxsize=None)
def weights():
    """The fixture's weights (float32, CPU), built once per process."""
    return mlp.synthetic_weights(int(golden()["seed"]))


def load_case(case, dtype=torch.float64, device="cpu"):
    """(x, y) of the case and its record {terms (5,) f64, total f64, grad (3,H,W) f32, value_err32, grad_err32_max, grad_err32_l2}."""
    g = golden()
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype=dtype, device=device)          # noqa: E731
    rec = {k: g[f"{case}_{k}"] for k in ("terms", "total", "grad", "value_err32", "grad_err32_max", "grad_err32_l2")}
    return t(g[f"{case}_x"]), t(g[f"{case}_y"]), rec


def run_torch(params, x, y, channels_last=False):
    """(terms (5,), total (), dL/dx (3,H,W)) of lpips_vgg_torch, detached."""
    x, y = x.clone()[None], y.clone()[None]
    if channels_last:
        x, y = x.contiguous(memory_format=torch.channels_last), y.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    total, terms = mlp.lpips_vgg_torch(params, x, y, return_terms=True)
    assert total.shape == (1, 1, 1, 1)
    (grad,) = torch.autograd.grad(total.sum(), x)
    return terms.detach(), total.detach().reshape(()), grad[0].contiguous()


def test_weight_hash():
    """The 14.7 M weights rebuilt from the seed are the ones the fixture was made with."""
    p = weights()
    assert [tuple(w.shape) for w in p["conv_weights"]] == list(mlp.CONV_SHAPES)
    assert sum(w.numel() for w in p["conv_weights"]) + sum(b.numel() for b in p["conv_biases"]) == 14714688
    assert mlp.weights_sha256(p) == str(golden()["weights_sha256"])


@pytest.mark.parametrize("case", CASES)
def test_torch_form_matches_the_reference_golden(case):
    """lpips_vgg_torch in float64 reproduces the reference's float64 run to round-off (terms and total to 1e-15 absolute -- they are
    ~1e-4 --, the gradient to the float32 rounding it was stored with), and in float32 stays within the reference's own float32
    error, in all three measures (on one CPU thread, as the generator measured it: the CPU convolutions split their sums by the size of
    the thread team)."""
    x, y, rec = load_case(case)
    assert tuple(x.shape[1:]) == SIZES[case]
    terms, total, grad = run_torch(mlp.cast_params(weights(), torch.float64), x, y)
    assert float((terms - torch.from_numpy(rec["terms"])).abs().max()) < 1e-15
    assert abs(float(total) - float(rec["total"])) < 1e-15
    ref_grad = torch.from_numpy(rec["grad"]).double()
    assert float((grad - ref_grad).abs().max()) <= 2.0 ** -24 * float(ref_grad.abs().max()) + 1e-300
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        t32, v32, g32 = run_torch(weights(), x.float(), y.float())
    finally:
        torch.set_num_threads(threads)
    if case == "same":
        assert float(rec["total"]) == 0.0 and float(v32) == 0.0 and not g32.any() and not grad.any()
        return
    assert float(rec["total"]) > 1e-4 and float(ref_grad.abs().max()) > 1e-6
    verr = max(float((t32.double() - terms).abs().max()), abs(float(v32) - float(total)))
    assert verr <= float(rec["value_err32"]), (verr, float(rec["value_err32"]))
    assert float((g32.double() - grad).abs().max()) <= float(rec["grad_err32_max"])
    assert float((g32.double() - grad).norm()) <= float(rec["grad_err32_l2"])


def test_fixture_is_small():
    assert os.path.getsize(GOLDEN) <= 700 * 1024


# ---- from_module ---------------------------------------------------------------------------------------------------------------------

def _features():
    layers, cin = [], 3
    for v in [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]:
        if v == "M":
            layers.append(nn.MaxPool2d(2, 2))
        else:
            layers += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return nn.Sequential(*layers)


def reference_layout_module():
    """A stand-in with the attribute layout of lpipsPyTorch.LPIPS(net_type='vgg'): .net.layers, .net.mean / .net.std, .lin[i][1]."""
    with torch.device("meta"):
        net = nn.Module()
        net.layers = _features()
        lin = nn.ModuleList([nn.Sequential(nn.Identity(), nn.Conv2d(c, 1, 1, 1, 0, bias=False)) for c in mlp.TAP_CHANNELS])
    net.register_buffer("mean", torch.tensor(mlp.SHIFT)[None, :, None, None])
    net.register_buffer("std", torch.tensor(mlp.SCALE)[None, :, None, None])
    m = nn.Module()
    m.net, m.lin = net, lin
    return m


def pip_layout_module():
    """A stand-in with the attribute names of the pip package's lpips.LPIPS(net='vgg'): .net.slice1..5, .scaling_layer, .lin0..4.model."""
    with torch.device("meta"):
        f = list(_features())
        net = nn.Module()
        for k, (a, b) in enumerate(((0, 4), (4, 9), (9, 16), (16, 23), (23, 30)), 1):
            setattr(net, f"slice{k}", nn.Sequential(*f[a:b]))
        m = nn.Module()
        m.net = net
        for k, c in enumerate(mlp.TAP_CHANNELS):
            lin = nn.Module()
            lin.model = nn.Sequential(nn.Dropout(), nn.Conv2d(c, 1, 1, 1, 0, bias=False))
            setattr(m, f"lin{k}", lin)
        m.lins = nn.ModuleList([getattr(m, f"lin{k}") for k in range(5)])
    m.scaling_layer = nn.Module()
    m.scaling_layer.register_buffer("shift", torch.tensor(mlp.SHIFT)[None, :, None, None])
    m.scaling_layer.register_buffer("scale", torch.tensor(mlp.SCALE)[None, :, None, None])
    return m


def test_from_module_finds_the_tensors_of_the_reference_layout():
    m = reference_layout_module()
    cw, cb, lw, shift, scale = mlp.LpipsVGG.find_tensors(m)
    convs = [l for l in m.net.layers if isinstance(l, nn.Conv2d)]
    assert len(cw) == 13 and all(a is c.weight for a, c in zip(cw, convs)) and all(a is c.bias for a, c in zip(cb, convs))
    assert len(lw) == 5 and all(a is s[1].weight for a, s in zip(lw, m.lin))
    assert shift is m.net.mean and scale is m.net.std
    assert [tuple(w.shape) for w in cw] == list(mlp.CONV_SHAPES)


def test_from_module_finds_the_tensors_of_the_pip_layout():
    m = pip_layout_module()
    cw, cb, lw, shift, scale = mlp.LpipsVGG.find_tensors(m)
    assert [tuple(w.shape) for w in cw] == list(mlp.CONV_SHAPES) and len(cb) == 13
    assert all(a is getattr(m, f"lin{k}").model[1].weight for k, a in enumerate(lw))          # (registered twice, found once)
    assert shift is m.scaling_layer.shift and scale is m.scaling_layer.scale


def test_from_module_refuses_other_layouts():
    m = reference_layout_module()
    m.net.layers = nn.Sequential(*list(m.net.layers)[:-3])                                   # 12 convolutions
    with pytest.raises(ValueError, match="exactly 13 and 5"):
        mlp.LpipsVGG.find_tensors(m)
    m = reference_layout_module()
    m.lin = nn.ModuleList(list(m.lin)[:4])
    with pytest.raises(ValueError, match="exactly 13 and 5"):
        mlp.LpipsVGG.find_tensors(m)
    m = reference_layout_module()
    del m.net.mean
    with pytest.raises(ValueError, match="mean"):
        mlp.LpipsVGG.find_tensors(m)
    with pytest.raises(ValueError, match="no .net"):
        mlp.LpipsVGG.find_tensors(nn.Linear(2, 2))
    # an AlexNet-shaped feature stack: the counts are wrong, and so are the shapes
    m = reference_layout_module()
    with torch.device("meta"):
        m.net.layers = nn.Sequential(*[nn.Conv2d(3 if i == 0 else 64, 64, 3, padding=1) for i in range(13)])
    with pytest.raises(ValueError, match="convolution 2 must have weight"):
        mlp.LpipsVGG(*mlp.LpipsVGG.find_tensors(m))


def test_cpu_tensors_are_refused():
    """The fused op and the packed weights have no CPU path."""
    p = weights()
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        mlp.LpipsVGG.from_tensors(p["conv_weights"], p["conv_biases"], p["lin_weights"], p["shift"], p["scale"])
    with pytest.raises(TypeError, match="must be an LpipsVGG"):
        mlp.lpips_vgg_fused(object(), torch.zeros(3, 16, 16), torch.zeros(3, 16, 16))


def test_c_abi_is_declared():
    """The five entry points are in the header; the ABI version did not move."""
    text = open(os.path.join(ROOT, "include", "moss_raster.h")).read()
    for name in ("moss_lpips_vgg_forward", "moss_lpips_vgg_backward", "moss_lpips_vgg_workspace_bytes", "moss_lpips_vgg_saved_bytes",
                 "moss_lpips_vgg_pack_weights"):
        assert name + "(" in text, name
    assert "#define MOSS_ABI_VERSION 7" in text
