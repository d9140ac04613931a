"""The forward-only (evaluation) path: MOSS_FORWARD_ONLY at the C ABI (VERDICT r5 "next round" 3).

MOSS renders novel views with `render(view, gaussians, pipeline, background)` under torch.no_grad() (render_ZJU.py:56-72).  The glue
tells the library that no backward follows; the library then produces none of the state only a backward reads (depth-segment cuts,
per-block tails, gradient-record cells, validity bits) and asks for a binning buffer of 62 B per instance instead of ~370.  What must
NOT change is any output: images, radii, sorted lists, final_T and n_contrib are the training forward's bit for bit."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from moss_amd import scenes
from tests import helpers as hp

pytestmark = pytest.mark.gpu

FORWARD_ONLY = 16


def _forward(d, gpu, debug):
    t = hp.hip_forward(d, gpu, debug=debug)
    return t, hp.hip_export(d, t, gpu)


@pytest.mark.parametrize("cfg,mode", [("config1", "precomp"), ("config1", "scale_rot"), ("config1", "lbs"), ("config2", "scale_rot"),
                                      ("config3", "scale_rot"), ("config3", "precomp"), ("config5", "scale_rot")])
def test_forward_only_outputs_equal_the_training_forward_bit_for_bit(gpu, hip_lib, cfg, mode):
    scene = getattr(scenes, cfg)()
    forward_only_equals_the_training_forward(hp.inputs_of(scene, mode), gpu, hip_lib)


def forward_only_equals_the_training_forward(d, gpu, hip_lib):
    """(also called by tests/test_gpu_raster_arguments.py with a scale_modifier other than 1)"""
    t0, e0 = _forward(d, gpu, 0)
    t1, e1 = _forward(d, gpu, FORWARD_ONLY)
    assert t0.R == t1.R > 0
    for name in ("color", "depth", "alpha", "radii", "final_T", "n_contrib", "point_list", "point_list_keys", "ranges"):
        assert np.array_equal(getattr(e0, name), getattr(e1, name)), name
    # the buffer: ids + block masks + records + keys, nothing else
    want = hip_lib.moss_raster_binning_bytes_forward_only(t1.R)
    assert t1.binning.numel() == want and want <= 64 * t1.R + 4096, (t1.binning.numel(), want, t1.R)
    assert t0.binning.numel() == hip_lib.moss_raster_binning_bytes(t1.R) or t0.binning.numel() > 3 * want
    assert want / t1.R <= 100.0 or t1.R < 200
    # status flag: the image buffer says what kind of forward filled it
    assert int(t1.img.view(torch.int32)[2].item()) & 4 and not int(t0.img.view(torch.int32)[2].item()) & 4


def test_backward_over_forward_only_buffers_is_a_no_op_with_zero_gradients(gpu, hip_lib):
    """include/moss_raster.h: a backward call over MOSS_FORWARD_ONLY buffers must never read the record pool the buffer does not have: the
    kernels check the frame's flag on the device and return zero gradients."""
    scene = scenes.config2()
    d = hp.inputs_of(scene, "scale_rot")
    t, _ = _forward(d, gpu, FORWARD_ONLY)
    dc, dd, da = hp.image_grads(d.H, d.W)
    g = hp.hip_backward(d, t, dc, dd, da, gpu)
    torch.cuda.synchronize(gpu)
    for name in ("dL_dmeans2D", "dL_dopacity", "dL_dmeans3D", "dL_dsh", "dL_dscales", "dL_drotations"):
        v = getattr(g, name)
        assert v is not None and not bool(v.any()), name


def test_render_under_no_grad_takes_the_forward_only_path(gpu, hip_lib):
    """render() is the reference's signature; the decision is the glue's: grad mode off -> plain tensors, the small buffer (seen through
    the context's last image buffer: its flag word), the same image as the differentiable call -- synchronous and capacity-bounded."""
    from moss_amd import diff_gaussian_rasterization as dgr
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import camera_view, render
    from moss_amd.graphs import GraphedStep
    scene = scenes.config2()
    pc = GaussianSet(scene, sh_degree=3, device=gpu, unified_features=True)
    cam, bg = camera_view(scene.camera, gpu), torch.zeros(3, device=gpu)
    P = scene.P
    T = (torch.eye(3) + 0.05 * torch.randn(P, 3, 3, generator=torch.Generator().manual_seed(1234))).to(gpu)
    tl = (0.01 * torch.randn(P, 3, generator=torch.Generator().manual_seed(3))).to(gpu)
    cx = dgr.RasterContext()
    cx.set_async(True)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, fused_activations=False, transforms_in_op=True,
                           pose_in_op=True, raw_parameters_in_op=True, raster_context=cx)
    ref = render(cam, pc, pipe, bg, transforms=T, translation=tl)            # differentiable, synchronous (learns the capacity)
    assert ref["render"].grad_fn is not None
    with torch.no_grad():
        out = render(cam, pc, pipe, bg, transforms=T, translation=tl)         # forward only, asynchronous
    assert out["render"].grad_fn is None and not out["render"].requires_grad
    cx.check_status()
    assert int(dgr._C.frame_status_word(cx.last_img_buffer).item()) & 4
    for k in ("render", "render_depth", "render_alpha", "radii"):
        assert torch.equal(out[k], ref[k].detach()), k
    # ... and replayed as a hipGraph: the same image again
    def eval_render():
        with torch.no_grad():
            return render(cam, pc, pipe, bg, transforms=T, translation=tl)["render"]
    g = GraphedStep(eval_render, warmup=2, device=gpu, context=cx)
    img = g()
    torch.cuda.synchronize(gpu)
    assert torch.equal(img, ref["render"].detach())
    g.check()
    assert g.dropped_frames == 0
    # a differentiable render on the same context afterwards still trains (the flag is per call)
    again = render(cam, pc, pipe, bg, transforms=T, translation=tl)
    again["render"].sum().backward()
    assert float(pc._xyz.grad.abs().max()) > 0 and torch.equal(again["render"].detach(), ref["render"].detach())


def test_forward_only_probe_reports_the_capacity_a_training_forward_needs(gpu, hip_lib):
    """Status word [3] of a forward-only frame is still what a TRAINING forward of the frame needs (instances, and the gradient-record
    cells a training buffer would hold): moss_amd.surgery sizes a re-captured training step from such a probe."""
    from moss_amd.diff_gaussian_rasterization import _C, RasterContext
    scene = scenes.config2()
    d = hp.inputs_of(scene, "scale_rot")
    words = {}
    for debug in (0, FORWARD_ONLY):
        t = hp.hip_forward(d, gpu, debug=debug)
        cx = RasterContext()
        cx._request_status(t.img, gpu)
        st, ev = cx.pending
        ev.synchronize()
        words[debug] = [int(x) for x in st]
    assert words[0][3] == words[FORWARD_ONLY][3] >= words[0][6] == words[FORWARD_ONLY][6] > 0
