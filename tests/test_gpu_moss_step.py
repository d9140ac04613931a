"""``moss_amd.train.MossStep``: MOSS's whole training iteration -- all six loss terms, all eight parameter groups -- as one step and
from one hipGraph.  tests/test_gpu_lbs.py's body scene (P = 6 890, 512 x 512), the two networks loaded from the fixtures the renderer
tests use, synthetic LPIPS weights, a fixed 192 x 256 region.  Everything is compared bit for bit: the class adds no mathematics."""
import copy
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LRS = {"auto_regression": 2.5e-4, "cross_attention_lbs": 1e-4}          # MOSS's rates for its two networks
FLAGS = dict(lbs_in_op=True, pose_head_in_op=True, lbs_weights_in_op=True, smpl_frame_in_op=True, transforms_in_op=True, pose_in_op=True,
             raw_parameters_in_op=True)


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    """Leave the device as the module found it (later tests bound their peak allocation): a MossStep and its GraphedStep refer to
    each other, so the captured graphs' pools are freed by a collection; the capture streams leave a BLAS workspace each."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch._C._cuda_clearCublasWorkspaces()
    torch.cuda.empty_cache()


def _frame(k, gpu):
    """tests/test_gpu_lbs.py's frame k and the target rotations of its pose term (the frame's own rotations, perturbed)."""
    from moss_amd import lbs as mlbs
    from tests.test_gpu_lbs import _small_frame
    f = _small_frame(k)
    g = torch.Generator().manual_seed(700 + k)
    f["pose_rotmats"] = mlbs.batch_rodrigues(f["poses"].reshape(24, 3)[1:] + 0.05 * torch.randn(23, 3, generator=g))
    return {key: v.to(gpu) for key, v in f.items()}


def _load(cam, k, gpu):
    for key, v in _frame(k, gpu).items():
        cam.smpl_param[key].copy_(v)


@pytest.fixture(scope="module")
def world(gpu, hip_lib):
    """What every test shares and none changes: the scene's images and region, the LPIPS network, one pristine model to copy."""
    from moss_amd import lbs_weights as mlw
    from moss_amd import lpips as mlp
    from moss_amd import pose as mpose
    from moss_amd.loss import ViewRegion
    from tests.test_gpu_lbs import _scene
    from tests.test_lbs_weights_cpu import load_case
    from tests.test_pose_cpu import GOLDEN, head_case
    s, pc0, cam, _ = _scene(gpu)
    pc = type(pc0)(s, device=gpu, unified_features=True)                 # (the same model with the SH coefficients as one tensor)
    pc.SMPL_NEUTRAL, pc.knn = pc0.SMPL_NEUTRAL, pc0.knn
    params = head_case(np.load(GOLDEN), "trained_small", dtype=torch.float32, device=gpu)[0]
    pc.auto_regression = mpose.head_module().to(gpu)
    pc.auto_regression.load_state_dict({k: v.float() for k, v in params.items()})
    pc.cross_attention_lbs = mlw.lbs_weight_module()
    pc.cross_attention_lbs.load_state_dict({k: v.float() for k, v in load_case("sharp", dtype=torch.float32, device=gpu)[1].items()})
    pc.cross_attention_lbs.to(gpu)
    pc.motion_offset_flag = True
    cam.smpl_param = _frame(0, gpu)
    H, W = s.camera.H, s.camera.W
    g = torch.Generator().manual_seed(77)
    bound = torch.zeros(1, H, W)
    bound[:, 128:384, 160:352] = 1                                       # 192 wide, 256 high
    lp = mlp.cast_params(mlp.synthetic_weights(), device=gpu)
    return {"pc": pc, "cam": cam, "H": H, "W": W, "gt": torch.rand(3, H, W, generator=g).to(gpu),
            "bkgd": (torch.rand(1, H, W, generator=g) > 0.5).float().to(gpu), "region": ViewRegion(bound.to(gpu)),
            "bg": torch.zeros(3, device=gpu),
            "lpips": mlp.LpipsVGG.from_tensors(lp["conv_weights"], lp["conv_biases"], lp["lin_weights"], lp["shift"], lp["scale"])}


def _fresh(world, stats=False):
    """A deep copy of the pristine model with a camera (static frame inputs) of its own."""
    from moss_amd.densify import DensifyStats
    pc, cam = copy.deepcopy(world["pc"]), copy.deepcopy(world["cam"])
    return pc, cam, (DensifyStats(int(pc._xyz.shape[0]), pc._xyz.device) if stats else None)


def _step(world, pc, cam, stats=None):
    from moss_amd.train import MossStep
    return MossStep(pc, cam, world["gt"], world["bkgd"], world["region"], world["bg"], world["lpips"], LRS, stats=stats)


def _gaussians(pc):
    return {"xyz": pc._xyz, "features": pc._features, "opacity": pc._opacity, "scaling": pc._scaling, "rotation": pc._rotation}


def _state(step):
    out = []
    for o in step.optimizers:
        out += [o.flat_params.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), o.step_state[:1].clone()]
    return out


def test_wiring_equals_the_step_composed_by_hand(gpu, hip_lib, world):
    """compute() against the same step written out here from the public ops: render with the same flags but no sinks and no update
    inside the backward, the six terms with MOSS's weights as literals, a plain backward(), three un-fused FlatAdamW.step() calls."""
    from types import SimpleNamespace
    from moss_amd import lbs_weights as mlw
    from moss_amd import pose as mpose
    from moss_amd.diff_gaussian_rasterization import RasterContext
    from moss_amd.dist import GradBucket
    from moss_amd.gaussian_renderer import render
    from moss_amd.loss import s3im_loss_roi_fused, training_loss_moss_fused
    from moss_amd.lpips import lpips_vgg_roi_fused
    from moss_amd.optim import FlatAdamW
    from moss_amd.train import TERM_NAMES
    assert TERM_NAMES == ("l1", "ssim", "mask_l2", "lpips", "nll", "s3im", "total")
    # --- the class
    pc, cam, _ = _fresh(world)
    unused0 = {n: p.detach().clone() for n, p in pc.cross_attention_lbs.named_parameters() if n in mlw.UNUSED_NAMES}
    step = _step(world, pc, cam)
    on = step.opt_networks
    assert on.nseg == 2 and len(on.bucket.params) == 68 and abs(on.seg_lr[0] - 2.5e-4) < 1e-10 and abs(on.seg_lr[1] - 1e-4) < 1e-10
    for o in step.optimizers:
        assert o.step_state is not None and o.eps == 1e-15 and o.weight_decay == 0.01
    assert step.opt_gaussians.fused is not None and [id(p) for p in step.opt_xyz.bucket.params] == [id(pc._xyz)]
    out = step.compute()
    torch.cuda.synchronize(gpu)
    step.context.check_status()
    assert float(out["render"].abs().max()) > 0.1
    # --- by hand
    pc2, cam2, _ = _fresh(world)
    cx = RasterContext()
    cx.set_async(True)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raster_context=cx, **FLAGS)
    kw = dict(capturable=True, eps=1e-15, weight_decay=0.01)
    groups = {g["name"]: g for g in pc2.param_groups()}
    four = ("features", "opacity", "scaling", "rotation")
    ba = GradBucket([groups[n]["params"][0] for n in four])
    oa = FlatAdamW([groups[n] for n in four], ba, **kw)
    bb = GradBucket([pc2._xyz])
    ob = FlatAdamW([groups["xyz"]], bb, **kw)
    head, net = mpose.head_parameters(pc2.auto_regression), mlw.net_parameters(pc2.cross_attention_lbs)
    bc = GradBucket(head + net)
    oc = FlatAdamW([{"params": head, "lr": 2.5e-4}, {"params": net, "lr": 1e-4}], bc, **kw)
    for b in (ba, bb, bc):
        b.detach_grads()
    r = render(cam2, pc2, pipe, world["bg"])
    image = r["render"]
    four_terms = torch.zeros(4, device=gpu)
    photometric = training_loss_moss_fused(image, r["render_alpha"], world["gt"], world["bkgd"], world["region"], 0.2, 0.5, terms_out=four_terms)
    lpips = lpips_vgg_roi_fused(world["lpips"], image, world["gt"], world["region"]).reshape(())
    nll = r["pose_out"]["nll"].mean()
    s3im = s3im_loss_roi_fused(image, world["gt"], world["region"])
    loss = photometric + 0.5 * lpips + 0.06 * nll + 0.3 * s3im
    loss.backward()
    for b in (ba, bb, bc):
        b.collect()
    assert cx.last_img_buffer is None                                    # (the first forward of a context is the synchronous one)
    for o in (oa, ob, oc):
        o.step()
    torch.cuda.synchronize(gpu)
    cx.check_status()
    # --- the same bits
    assert torch.equal(out["render"], image.detach())
    by_hand = torch.stack((four_terms[1], four_terms[2], four_terms[3], lpips.detach(), nll.detach(), s3im.detach(), loss.detach()))
    print("\nterms " + ", ".join(f"{n} {float(v):.6g}" for n, v in zip(TERM_NAMES, step.terms)))
    assert torch.equal(step.terms, by_hand) and torch.equal(out["terms"], by_hand)
    assert all(float(v) != 0 for v in by_hand)
    # photometric = l1 + 0.5 mask_l2 + 0.2 (1 - ssim): the three terms are MOSS's, with its weights
    l1, ssim, mask = (float(v) for v in by_hand[:3])
    assert abs(float(four_terms[0]) - (l1 + 0.5 * mask + 0.2 * (1 - ssim))) <= 1e-6 * abs(float(four_terms[0]))
    mine = mpose.head_parameters(pc.auto_regression) + mlw.net_parameters(pc.cross_attention_lbs)
    for i, (p, q) in enumerate(zip(mine, head + net)):
        assert p.grad is not None and torch.equal(p.grad, q.grad), f"gradient of network tensor {i}"
        assert p.grad.data_ptr() == step.bucket_networks.flat[step.bucket_networks.offsets[i]:].data_ptr()      # written through its sink
        assert bool(torch.isfinite(p.grad).all()), i
        assert torch.equal(p, q), f"network tensor {i} after the step"
    assert sum(float(p.grad.abs().sum()) for p in mine[:52]) > 0 and sum(float(p.grad.abs().sum()) for p in mine[52:]) > 0
    assert not torch.equal(mine[0], world["pc"].auto_regression.block_mlps[0].weight)                            # both networks moved
    assert not torch.equal(mine[52], world["pc"].cross_attention_lbs.bw_linears[0].weight)
    assert torch.equal(pc._xyz.grad, pc2._xyz.grad)
    for (n, p), q in zip(_gaussians(pc).items(), _gaussians(pc2).values()):
        assert torch.equal(p, q), n
        assert not torch.equal(p, _gaussians(world["pc"])[n]), n          # ... and every group moved
    for mo, ho in zip(step.optimizers, (oa, ob, oc)):
        assert torch.equal(mo.exp_avg, ho.exp_avg) and torch.equal(mo.exp_avg_sq, ho.exp_avg_sq)
        assert mo.step_count() == ho.step_count() == 1
    # out_layer / gate_proj: no gradient in MOSS, so no optimizer state and not even weight decay
    for m in (pc, pc2):
        for n, p in m.cross_attention_lbs.named_parameters():
            if n in mlw.UNUSED_NAMES:
                assert p.grad is None and torch.equal(p, unused0[n]), n
    assert len(unused0) == 4


def test_six_replays_of_one_capture_equal_six_eager_steps(gpu, hip_lib, world):
    """Two deep copies of the model; one stepped eagerly six times, one by six replays of one capture, over three frames copied
    into the static inputs.  (capture() undoes the steps its warm-up takes.)"""
    pe, ce, se = _fresh(world, stats=True)
    pg, cg, sg = _fresh(world, stats=True)
    eager, graphed = _step(world, pe, ce, se), _step(world, pg, cg, sg)
    start = _state(graphed)
    graphed.capture(warmup=3)
    for a, b in zip(start, _state(graphed)):
        assert torch.equal(a, b)                                         # the capture left the model where it found it
    assert not bool(sg.denom.any()) and not bool(graphed.joint_F_sum.any())
    images = []
    for i in range(6):
        k = i % 3
        _load(ce, k, gpu)
        _load(cg, k, gpu)
        out_e = eager.compute()
        te, ie = out_e["terms"].clone(), out_e["render"].clone()
        out_g = graphed()
        tg, ig = out_g["terms"].clone(), out_g["render"].clone()
        torch.cuda.synchronize(gpu)
        assert torch.equal(te, tg), (i, te.tolist(), tg.tolist())
        assert torch.equal(ie, ig), i
        images.append(ig)
    graphed.check()                                                      # (may capture again: the other frames need a little more room)
    assert graphed.dropped_frames == 0
    eager.context.check_status()
    for j, (a, b) in enumerate(zip(_state(eager), _state(graphed))):
        assert torch.equal(a, b), f"optimizer state {j} (parameters, exp_avg, exp_avg_sq, step counter per optimizer)"
    assert eager.step_counts() == graphed.step_counts() == (6, 6, 6)
    for a, b in ((se.xyz_gradient_accum, sg.xyz_gradient_accum), (se.denom, sg.denom), (se.max_radii2D, sg.max_radii2D),
                 (eager.joint_F_sum, graphed.joint_F_sum), (eager.lbs_weights_sum, graphed.lbs_weights_sum)):
        assert torch.equal(a, b) and float(a.abs().max()) > 0
    assert float(sg.denom.max()) == 6.0
    assert not torch.equal(images[0], images[1]) and not torch.equal(images[1], images[2]) and not torch.equal(images[0], images[2])
    assert not torch.equal(images[0], images[3])                         # the same frame again, three steps later: the model has moved


def test_a_dropped_frame_is_a_step_for_none_of_the_three_optimizers(gpu, hip_lib, world):
    """Captured with the capacity of a frame of shrunken Gaussians, then replayed on Gaussians that need far more: the frame
    overflows and renders nothing.  Parameters, moments and the three step counters stay bit for bit -- the pose term alone would
    have moved the pose head -- and check() counts the frame; the re-captured step then steps."""
    pc, cam, st = _fresh(world, stats=True)
    step = _step(world, pc, cam, st)
    original = pc._scaling.detach().clone()
    with torch.no_grad():
        pc._scaling.copy_(original - 5.0)
    step.capture(warmup=2)
    with torch.no_grad():
        pc._scaling.copy_(original + 2.0)
    before = _state(step)
    out = step()
    torch.cuda.synchronize(gpu)
    assert not bool(out["render"].any())                                 # rendered nothing
    for j, (a, b) in enumerate(zip(before, _state(step))):
        assert torch.equal(a, b), f"optimizer state {j} changed across a dropped frame"
    assert step.step_counts() == (0, 0, 0)
    assert not bool(st.denom.any()) and not bool(step.joint_F_sum.any()) and not bool(step.lbs_weights_sum.any())
    # (the frame itself was not empty for the pose term: its gradients are in the bucket, and the guard kept them from being applied)
    assert float(step.bucket_networks.flat[:step.bucket_networks.n_params].abs().max()) > 0
    assert step.check() and step.dropped_frames >= 1                     # counted, and captured again with the capacity that fits
    dropped = step.dropped_frames
    out = step()
    torch.cuda.synchronize(gpu)
    assert float(out["render"].abs().max()) > 0 and step.step_counts() == (1, 1, 1)
    assert not step.check() and step.dropped_frames == dropped


def test_the_step_reads_nothing_back(gpu, hip_lib, world):
    pc, cam, st = _fresh(world, stats=True)
    step = _step(world, pc, cam, st)
    for _ in range(2):
        step.compute()                                                   # (the first forward of a context is synchronous by design)
    step.set_learning_rates({"xyz": 1e-4, "auto_regression": 2e-4})      # (each entry goes to the optimizer that holds the group)
    torch.cuda.synchronize(gpu)
    torch.cuda.set_sync_debug_mode("error")
    try:
        step.compute()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize(gpu)
    assert step.step_counts() == (3, 3, 3)
    assert abs(step.opt_networks.seg_lr[0] - 2e-4) < 1e-10 and abs(step.opt_xyz.seg_lr[0] - 1e-4) < 1e-10
