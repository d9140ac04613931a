"""GPU parity over the two arguments of the rasterizer's call that every other test leaves at one value: `scale_modifier` (1.0 everywhere
else) and the number M of SH coefficients per Gaussian (16 everywhere else).

* `scale_modifier` enters cov3d_from_scale_rot in the forward (training and forward-only), scale_rot_backward (twice: m_k = mod s_k),
  the transforms branch (which rebuilds the covariance in front of the transform), the raw-parameter chain and the fused AdamW step
  that consumes those gradients.  The reference reports dL_dscales with respect to mod * s, WITHOUT a factor mod (backward.cu:322-325);
  the oracle restates that (tests/test_oracle_cpu.py pins it against float64 autograd / mod) and the kernels must follow it.
* The C ABI takes any M >= (D + 1)^2; a model allocated at SH degree 0 / 1 / 2 has M = 1 / 4 / 9.  For M != 16, and for an SH pointer
  that is not 16-byte aligned, the launchers (moss_amd/csrc/preprocess.hip) pick the UNSTAGED kernels -- preprocess_forward_kernel with
  stage_sh = 0 on an SH input, preprocess_backward_kernel<false, false, 0> -- which index `shs` and `dL_dsh` at a stride of 3 M floats;
  elsewhere those instantiations run with colours only (shs == NULL).

No comparison code and no tolerance of its own: the checkers and constants are those of tests/test_gpu_parity.py,
tests/test_gpu_parity_hardened.py and tests/helpers.py.  The scenes here are not BASELINE configurations as far as the single rule is
concerned (other arguments): they are held to helpers.RULE_K, the rule for arbitrary scenes.

Two scenes, so that both shapes of the per-Gaussian backward run: config1 (256 Gaussians: with M = 16 the launcher takes sixteen lanes
per Gaussian) and 9 000 body Gaussians at 192 x 192 (P > 8192: one Gaussian per lane; tile lists of up to 2 369 entries: heavy tiles).
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from moss_amd import scenes
from tests import helpers as hp
from tests import test_gpu_eval as te
from tests import test_gpu_parity as tp
from tests import test_gpu_parity_hardened as th

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "config1":
        return scenes.config1()
    return scenes.body_scene(9000, 192, 192, 200.0, init_like=False, name="body9000")


@functools.lru_cache(maxsize=None)
def _mean_tiles_at_modifier_one(name, mode):
    fw = hp.oracle_forward(hp.inputs_of(_scene(name), mode))
    return float(fw.tiles_touched[fw.radii > 0].mean())


def _inputs(name, mode, mod=1.0, M=16, degree=3):
    d = hp.inputs_of(_scene(name), mode, degree=degree)
    d.scale_modifier = mod
    if M != 16:
        d.shs = d.shs[:, :M].contiguous()
    return d


def _three_checkers(d, gpu, key):
    """The forward stage by stage, the backward on the HIP forward's state, and end to end against float32 and float64."""
    fw, t, e = tp._check_forward(d, gpu)
    g = tp._check_backward(d, gpu, fw, t, e)
    th._end_to_end(d, gpu, key, rule_k=hp.RULE_K)
    return fw, t, e, g


# ---- B1: scale_modifier ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod", [0.6, 1.7])
@pytest.mark.parametrize("name,mode", [("config1", "scale_rot"), ("config1", "lbs"), ("body9000", "scale_rot")])
def test_scale_modifier_forward_backward_end_to_end(gpu, hip_lib, name, mode, mod):
    d = _inputs(name, mode, mod=mod)
    fw, t, e, g = _three_checkers(d, gpu, f"{name}_{mode}_mod{mod}")
    if mod > 1.0:
        # the scene does what it claims: larger Gaussians reach more tiles (config1, scale_rot: 8.45 against 4.57)
        assert float(e.tiles_touched[e.radii > 0].mean()) > _mean_tiles_at_modifier_one(name, mode)
    if name == "body9000":
        # one Gaussian per lane, and tile lists far beyond the 32 entries from which a tile is blended as a heavy one
        assert d.P > 8192 and int((fw.ranges[:, 1].astype(np.int64) - fw.ranges[:, 0]).max()) > 320


# ---- B2: raw-parameter mode with a modifier ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sinks", [False, True])
def test_raw_parameters_with_a_scale_modifier(gpu, hip_lib, sinks):
    """logits / log-scales / unnormalised quaternions in, mod = 1.7: directly through the C ABI, and through render() with fused
    activations' pipeline flags and gradient sinks (which also asserts that render() and the direct call produce the same bits)."""
    th._raw_case(_scene("config1"), gpu, "cfg1_raw_mod1.7" + ("_sinks" if sinks else ""), sinks=sinks, scale_modifier=1.7)


# ---- B3: the forward-only path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["scale_rot", "lbs"])
def test_forward_only_equals_the_training_forward_with_a_scale_modifier(gpu, hip_lib, mode):
    te.forward_only_equals_the_training_forward(_inputs("config1", mode, mod=1.7), gpu, hip_lib)


# ---- B4: M != 16 -----------------------------------------------------------------------------------------------------------------------
def _check_sh_gradient(d, gpu, fw, t, g, M, degree):
    """Shape of dL_dsh, exact zeros above the active degree, run-to-run bits, exact zeros on culled Gaussians.  The last check is
    VACUOUS for config1 and the body scene, which cull nothing: test_culled_gaussians_with_a_short_sh_array is the one that runs it."""
    assert tuple(g.dL_dsh.shape) == (d.P, M, 3)
    assert not bool(g.dL_dsh[:, (degree + 1) ** 2:, :].any())                 # above the active degree: exactly zero
    culled = torch.from_numpy(fw.radii == 0)
    dc, dd, da = hp.image_grads(d.H, d.W)
    a = hp.hip_backward(d, t, dc, dd, da, gpu)
    b = hp.hip_backward(d, t, dc, dd, da, gpu)
    for k, v in vars(a).items():
        if torch.is_tensor(v) and v.numel() > 0:
            assert torch.equal(v, getattr(b, k)), k                           # run to run: the same bits
            if culled.any() and v.shape[0] == d.P:
                assert not bool(v.cpu()[culled].any()), k                     # a Gaussian that was not rendered: exactly zero
    assert tuple(a.dL_dsh.shape) == (d.P, M, 3) and not bool(a.dL_dsh[:, (degree + 1) ** 2:, :].any())


@pytest.mark.parametrize("M,degree", [(1, 0), (4, 1), (9, 2), (9, 1)])
@pytest.mark.parametrize("mode", ["scale_rot", "precomp"])
def test_sh_arrays_of_fewer_than_16_coefficients(gpu, hip_lib, mode, M, degree):
    d = _inputs("config1", mode, M=M, degree=degree)
    fw, t, e, g = _three_checkers(d, gpu, f"config1_{mode}_M{M}_D{degree}")
    _check_sh_gradient(d, gpu, fw, t, g, M, degree)


def test_sh_array_of_4_coefficients_with_a_scale_modifier_one_gaussian_per_lane(gpu, hip_lib):
    d = _inputs("body9000", "scale_rot", mod=1.7, M=4, degree=1)
    fw, t, e, g = _three_checkers(d, gpu, "body9000_scale_rot_mod1.7_M4_D1")
    _check_sh_gradient(d, gpu, fw, t, g, 4, 1)


def test_culled_gaussians_with_a_short_sh_array(gpu, hip_lib):
    """Neither scene above culls a Gaussian.  Here every eighth Gaussian of config1 sits behind the camera (radii == 0): with M = 4 the
    unstaged kernel must leave their rows of dL_dsh, and every other gradient of theirs, exactly zero."""
    import copy
    s = copy.copy(_scene("config1"))
    s.means3D = s.means3D.clone()
    s.means3D[::8, 2] = -3.5                                                  # the camera looks along +z from z = -3: view depth -0.5
    d = hp.inputs_of(s, "scale_rot", degree=1)
    d.shs = d.shs[:, :4].contiguous()
    d.scale_modifier = 1.7
    fw, t, e, g = _three_checkers(d, gpu, "config1_culled_scale_rot_mod1.7_M4_D1")
    assert int((fw.radii == 0).sum()) == d.P // 8
    _check_sh_gradient(d, gpu, fw, t, g, 4, 1)


def test_sh_array_that_is_not_16_byte_aligned(gpu, hip_lib):
    """M = 16, degree 3, but the (P, 16, 3) tensor is a contiguous view that starts 4 bytes into its storage: the staging kernels' 16-byte
    loads cannot take it and the launchers fall to the unstaged kernels.  Same checkers; whether the results equal the aligned run's
    bit for bit is printed, not asserted (two kernels, the same arithmetic on paper)."""
    d = _inputs("config1", "scale_rot")
    aligned = d.shs
    store = torch.zeros(d.P * 48 + 1, device=gpu)
    store[1:].copy_(aligned.reshape(-1).to(gpu))
    d.shs = store[1:].view(d.P, 16, 3)                                        # (helpers: .to(device) of a device tensor is the tensor itself)
    assert d.shs.is_contiguous() and d.shs.data_ptr() % 16 != 0 and d.shs.data_ptr() % 4 == 0
    fw, t, e, g = _three_checkers(d, gpu, "config1_scale_rot_sh_misaligned")
    assert t.args["sh"].data_ptr() == d.shs.data_ptr()                        # the op did see the misaligned pointer
    _check_sh_gradient(d, gpu, fw, t, g, 16, 3)
    d0 = _inputs("config1", "scale_rot")
    dc, dd, da = hp.image_grads(d.H, d.W)
    t0 = hp.hip_forward(d0, gpu)
    g0, g1 = hp.hip_backward(d0, t0, dc, dd, da, gpu), hp.hip_backward(d, hp.hip_forward(d, gpu), dc, dd, da, gpu)
    same = {k: bool(torch.equal(v, getattr(g1, k))) for k, v in vars(g0).items() if torch.is_tensor(v) and v.numel() > 0}
    same["color"] = bool(torch.equal(t0.color, t.color))
    print("misaligned SH against the aligned run, bit for bit:", same)
    th._note("config1_scale_rot_sh_misaligned_equals_aligned_bitwise", same)


# ---- B5: the fused AdamW step in the unstaged kernel (preprocess_backward_kernel<false, true, 0>) -----------------------------------------
@pytest.mark.parametrize("mod", [1.0, 1.7])
def test_backward_kernel_takes_the_adamw_step_without_sh(gpu, hip_lib, mod):
    """Colours given (override_color: shs == NULL in the op), position / opacity / scaling / rotation fused into the backward.  The
    launcher stages the SH rows only when `shs != nullptr` (launch_preprocess_backward), and a fused call without staging is
    preprocess_backward_kernel<false, true, 0>: the unstaged kernel takes the step.  Against the two-kernel form (backward -> gradients in the bucket -> flat AdamW) on an identical
    model, like tests/test_gpu_ops.py::test_backward_kernel_takes_the_adamw_step: parameters, both moments and the step count are
    bit-identical after each of three steps -- at scale_modifier 1.7 too.

    What this cannot see: both sides consume the SAME kernel's gradients, so a wrong factor `mod` in the scale gradient itself passes
    here.  That is guarded by the comparisons with the oracle above (test_scale_modifier_..., test_raw_parameters_...); this test is
    about the step the unstaged kernel takes with them."""
    from moss_amd.diff_gaussian_rasterization import _C
    from moss_amd.dist import GradBucket
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import camera_view, render
    from moss_amd.optim import FlatAdamW
    s = scenes.config2()
    cam = camera_view(s.camera, gpu)
    bg = torch.zeros(3, device=gpu)
    gen = torch.Generator().manual_seed(5)
    w = torch.rand(3, s.camera.H, s.camera.W, generator=gen).to(gpu)
    colors = torch.rand(s.P, 3, generator=gen).to(gpu)

    def make(fused):
        pc = GaussianSet(s, sh_degree=3, device=gpu, unified_features=True)
        cx = _C.RasterContext()
        cx.set_async(True, capacity=4_000_000)
        pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raster_context=cx, raw_parameters_in_op=True)
        groups = [g for g in pc.param_groups() if g["name"] != "features"]    # (the features receive no gradient from this render)
        bucket = GradBucket([p for g in groups for p in g["params"]])
        opt = FlatAdamW(groups, bucket, eps=1e-15, weight_decay=0.01, capturable=True)
        if fused:
            opt.fuse_into_backward(cx, means3D=pc._xyz, opacity=pc._opacity, scales=pc._scaling, rotations=pc._rotation)

        def step():
            if not fused:
                bucket.attach()
            out = render(cam, pc, pipe, bg, scaling_modifier=mod, override_color=colors)
            ((out["render"] * w).sum() + out["render_alpha"].sum()).backward()
            if fused:
                assert all(p.grad is None for p in pc.parameters())           # the gradients never left the kernel
            opt.step(skip_word=None if fused else _C.frame_status_word(cx.last_img_buffer))
            return out["render"].detach()
        return SimpleNamespace(pc=pc, opt=opt, step=step)

    a, b = make(False), make(True)
    start = a.opt.flat_params.clone()
    for it in range(3):
        ia, ib = a.step(), b.step()
        torch.cuda.synchronize(gpu)
        assert torch.equal(ia, ib) and float(ia.abs().max()) > 0
        for name in ("flat_params", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(a.opt, name), getattr(b.opt, name)), f"{name} differs after step {it + 1}"
        assert a.opt.step_count() == b.opt.step_count() == it + 1
    assert not torch.equal(start, b.opt.flat_params)
    assert torch.equal(a.pc._features.data, b.pc._features.data) and a.pc._features.grad is None
