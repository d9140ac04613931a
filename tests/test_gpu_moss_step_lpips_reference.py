"""``MossStep(lpips_reference=)``: the training step with the ground truth's half of LPIPS computed once per camera.  The set-up is
tests/test_gpu_moss_step.py's (P = 6 890, 512 x 512) with regions of at most 96 x 72, so that every wide LPIPS convolution takes the
same kernel shape with one image as with two (a device with more than 122 CUs) and everything is compared bit for bit: the keyword
adds no mathematics."""
import pytest
import torch

from moss_amd import lpips as mlp
from tests.test_gpu_moss_step import LRS, _fresh, _load, _release_device_memory, _state, world  # noqa: F401  (fixtures of that module, by import)

pytestmark = pytest.mark.gpu

RECTS = ((220, 200, 72, 96), (231, 189, 61, 83))                         # (x, y, w, h): two crops that differ in size, on the body


@pytest.fixture(autouse=True)
def _same_shapes(gpu):
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    if cus <= 122:
        pytest.skip(f"{cus} CUs: the one-image and two-image LPIPS calls take the same kernel shapes at 96 x 72 only above 122 CUs")


def _regions(world, gpu):
    from moss_amd.loss import ViewRegion
    out = []
    for x0, y0, w, h in RECTS:
        bound = torch.zeros(1, world["H"], world["W"])
        bound[:, y0:y0 + h, x0:x0 + w] = 1
        out.append(ViewRegion(bound.to(gpu)))
    assert [r.xywh for r in out] == list(RECTS)
    return out


def _truths(world, gpu):
    gen = torch.Generator().manual_seed(78)
    return [world["gt"], torch.rand(3, world["H"], world["W"], generator=gen).to(gpu)]


def _moss_step(world, gpu, capacity, reference):
    """A step with static inputs of its own (ground truth and region: the tests rewrite them), on view 0."""
    from moss_amd.train import MossStep
    pc, cam, _ = _fresh(world)
    step = MossStep(pc, cam, world["gt"].clone(), world["bkgd"], _regions(world, gpu)[0], world["bg"], world["lpips"], LRS,
                    lpips_capacity=capacity, lpips_reference=reference)
    return step, cam


def test_one_eager_step_is_the_step_without_a_reference(gpu, hip_lib, world):
    """One compute() with a reference of the crop's size (no capacity) and one without, from the same state: the seven terms, every
    parameter and every optimizer moment are the same bits."""
    net, regions, truths = world["lpips"], _regions(world, gpu), _truths(world, gpu)
    ref = mlp.lpips_vgg_roi_reference(net, truths[0], regions[0])
    (plain, _), (cached, _) = _moss_step(world, gpu, None, None), _moss_step(world, gpu, None, ref)
    assert plain.lpips_reference is None and cached.lpips_reference is ref
    a, b = plain.compute(), cached.compute()
    torch.cuda.synchronize(gpu)
    assert torch.equal(a["terms"], b["terms"]) and torch.equal(a["render"], b["render"]) and float(b["terms"][3]) > 0
    for j, (u, v) in enumerate(zip(_state(plain), _state(cached))):
        assert torch.equal(u, v), f"optimizer state {j} (parameters, exp_avg, exp_avg_sq, step counter per optimizer)"
    assert plain.step_counts() == cached.step_counts() == (1, 1, 1)
    with pytest.raises(ValueError, match="laid out for capacity"):
        _moss_step(world, gpu, (96, 72), ref)
    with pytest.raises(TypeError, match="LpipsReference"):
        _moss_step(world, gpu, None, truths[0])


def test_captured_replay_over_frames_whose_crops_differ(gpu, hip_lib, world):
    """One capture with a capacity and a static reference, replayed over two frames whose crops differ in size, each loaded by the
    input copies, region.copy_ and lpips_reference.copy_(refs[k]); against the eager compute() of a second step WITHOUT references
    fed the same frames.  Then check(): it passes, and raises once a region is loaded without its reference."""
    net, regions, truths = world["lpips"], _regions(world, gpu), _truths(world, gpu)
    cap = mlp.crop_capacity(regions)
    assert cap == (96, 72)
    refs, nbytes = mlp.reference_cache(net, truths, regions, cap)
    assert nbytes == 2 * mlp.reference_bytes(*cap)
    static = mlp.LpipsReference.empty(net, cap).copy_(refs[0])
    (eager, ce), (graphed, cg) = _moss_step(world, gpu, cap, None), _moss_step(world, gpu, cap, static)
    graphed.capture(warmup=3)
    lpips_terms = []
    for i in (1, 0, 1, 0):
        for step, cam in ((eager, ce), (graphed, cg)):
            _load(cam, i, gpu)
            step.gt_image.copy_(truths[i])
            step.region.copy_(regions[i])
        graphed.lpips_reference.copy_(refs[i])
        out_e = eager.compute()
        te, ie = out_e["terms"].clone(), out_e["render"].clone()
        out_g = graphed()
        tg, ig = out_g["terms"].clone(), out_g["render"].clone()
        torch.cuda.synchronize(gpu)
        assert torch.equal(te, tg), (i, te.tolist(), tg.tolist())
        assert torch.equal(ie, ig), i
        lpips_terms.append(float(tg[3]))
    assert len(set(lpips_terms)) == 4 and all(v > 0 for v in lpips_terms)
    graphed.check()
    assert graphed.dropped_frames == 0
    eager.context.check_status()
    for j, (u, v) in enumerate(zip(_state(eager), _state(graphed))):
        assert torch.equal(u, v), f"optimizer state {j}"
    assert eager.step_counts() == graphed.step_counts() == (4, 4, 4)
    graphed.region.copy_(regions[1])                                     # ... and the reference of view 0 stays loaded
    graphed()
    torch.cuda.synchronize(gpu)
    with pytest.raises(RuntimeError, match=r"lpips_reference holds a crop of \(96, 72\) and the region's is 83x61"):
        graphed.check()
