"""The evaluation metrics on the device (C ABI moss_eval_metrics, moss_amd.metrics.QualityReport / evaluate_views): the reference's
per-view numbers (tests/golden/eval_metrics.npz), its float64 accumulation, a float64 torch cross-check on random cases, the clamped and
filled image, determinism, batching, graph capture next to MultiViewRender, and the split driver."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from moss_amd import scenes

pytestmark = pytest.mark.gpu

GOLDEN = "tests/golden/eval_metrics.npz"


def _grid(z, key):
    """The fixture's images: stored as uint8 grid indices q, the float32 values are exactly q / 128 - 0.25 (tests/golden/make_golden_eval.py)."""
    return z[key + "_q"].astype(np.float32) / np.float32(128) - np.float32(0.25)


def _golden_views(z, s, gpu):
    from moss_amd.loss import ViewRegion
    views = []
    for i in range(len(z[f"{s}_l1"])):
        region = ViewRegion(torch.from_numpy(z[f"{s}_bound"][i]).to(gpu)) if z[f"{s}_has_bound"][i] else None
        views.append((torch.from_numpy(_grid(z, f"{s}_image")[i]).to(gpu).contiguous(), torch.from_numpy(_grid(z, f"{s}_gt")[i]).to(gpu).contiguous(), region))
    return views


@pytest.mark.parametrize("s", ["a", "b", "c"])
def test_kernel_matches_the_reference_numbers_per_view(gpu, hip_lib, s):
    from moss_amd.metrics import QualityReport
    z = np.load(GOLDEN)
    views = _golden_views(z, s, gpu)
    C, H, W = views[0][0].shape
    rep = QualityReport(gpu, C, H, W, torch.from_numpy(z[f"{s}_bg"]).to(gpu), per_view_capacity=len(views))
    rep.add_many(views)
    pv = rep.per_view().numpy()
    assert pv.shape == (len(views), 3)
    # SSIM: the loss fixtures' bar, 2e-6, on the black background.  On the WHITE one the render is filled with 1 and sigma^2 = E[x^2] - mu^2
    # cancels around 1, where float32 resolves 6e-8 against C2 = 9e-4: the reference's own float32 value is 1.5e-6 from its float64 value
    # there (view b1, the all-zero mask: the whole render is 1) and this kernel's summation order lands 3.5e-6 from the reference's
    ssim_bar = 2e-6 if float(z[f"{s}_bg"].sum()) == 0 else 6e-6
    for i in range(len(views)):
        assert abs(pv[i, 0] - z[f"{s}_l1"][i]) < 2e-6, (s, i, pv[i, 0], z[f"{s}_l1"][i])
        assert abs(pv[i, 2] - z[f"{s}_ssim"][i]) < ssim_bar, (s, i, pv[i, 2], z[f"{s}_ssim"][i])
        want = float(z[f"{s}_psnr"][i])
        if math.isinf(want):
            assert math.isinf(pv[i, 1]) and pv[i, 1] > 0, (s, i, pv[i, 1])
        else:
            assert abs(pv[i, 1] - want) < 1e-4, (s, i, pv[i, 1], want)


@pytest.mark.parametrize("s", ["a", "b", "c"])
def test_set_means_are_the_reference_double_accumulation(gpu, hip_lib, s):
    """means() = ((0.0 + double(v0)) + double(v1) + ...) / n over the kernel's own float32 per-view values -- the reference's
    `x_test += metric.mean().double()` then `/= len(cameras)` -- bit for bit; and the reference's means within the per-view bars."""
    from moss_amd.metrics import QualityReport
    z = np.load(GOLDEN)
    views = _golden_views(z, s, gpu)
    C, H, W = views[0][0].shape
    rep = QualityReport(gpu, C, H, W, torch.from_numpy(z[f"{s}_bg"]).to(gpu), per_view_capacity=16)
    for v in views:
        rep.add(*v)
    m, pv = rep.means(), rep.per_view()
    n = len(views)
    assert m["n"] == n
    for k, name in enumerate(("l1", "psnr", "ssim")):
        acc = 0.0
        for i in range(n):
            acc += torch.tensor(float(pv[i, k]), dtype=torch.float32).double().item()
        assert m[name] == acc / n, (name, m[name], acc / n)
        want = float(z[f"{s}_mean_{name}"])
        assert (math.isinf(want) and m[name] == want) or abs(m[name] - want) < (1e-4 if name == "psnr" else 2e-6), (name, m[name], want)


def _random_case(seed, gpu):
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda n: int(torch.randint(n, (1,), generator=g))
    sizes = [(1024, 1024, 3), (1024, 1024, 1), (512, 512, 3), (97, 131, 3), (33, 31, 1), (1, 1, 3), (5, 300, 3), (300, 7, 3), (64, 48, 1),
             (255, 257, 3), (2048, 96, 3), (96, 2048, 1)]
    H, W, C = sizes[seed % len(sizes)]
    B = 1 + r(8)
    bg = torch.zeros(3) if r(2) else torch.ones(3)
    views = []
    for _ in range(B):
        gt = torch.rand(C, H, W, generator=g) * 1.4 - 0.2
        image = gt + 0.2 * torch.randn(C, H, W, generator=g) if r(4) else gt.clone()
        kind = r(3)
        mask = None if kind == 0 else (torch.zeros(H, W) if kind == 1 else (torch.rand(H, W, generator=g) < 0.6).float())
        views.append((image, gt, mask))
    return C, H, W, bg, views


@pytest.mark.parametrize("seed", range(20))
def test_random_cases_agree_with_float64_torch(gpu, hip_lib, seed):
    from moss_amd.loss import ViewRegion
    from moss_amd.metrics import QualityReport, quality_torch
    C, H, W, bg, views = _random_case(seed, gpu)
    rep = QualityReport(gpu, C, H, W, bg.to(gpu), per_view_capacity=len(views))
    rep.add_many([(im.to(gpu), gt.to(gpu), None if m is None else ViewRegion(m.to(gpu))) for im, gt, m in views])
    pv = rep.per_view().double()
    for i, (im, gt, m) in enumerate(views):
        l1, p, s = (float(v) for v in quality_torch(im.double(), gt.double(), m, bg))
        assert abs(pv[i, 0].item() - l1) < 1e-6, (seed, i, pv[i, 0].item(), l1)
        assert abs(pv[i, 2].item() - s) < 2e-5, (seed, i, pv[i, 2].item(), s)
        if math.isinf(p):
            assert math.isinf(pv[i, 1].item()), (seed, i)
        else:
            assert abs(pv[i, 1].item() - p) < 1e-3, (seed, i, pv[i, 1].item(), p)


@pytest.mark.parametrize("bg", [0.0, 1.0])
def test_out_image_is_torch_clamp_and_fill_bit_for_bit(gpu, hip_lib, bg):
    from moss_amd.loss import ViewRegion
    from moss_amd.metrics import QualityReport
    g = torch.Generator().manual_seed(77)
    C, H, W = 3, 133, 70
    image = (torch.rand(C, H, W, generator=g) * 1.6 - 0.3).to(gpu)
    image[0, 3, 4] = float("nan")
    gt = torch.rand(C, H, W, generator=g).to(gpu)
    mask = (torch.rand(1, H, W, generator=g) < 0.5).float().to(gpu)
    rep = QualityReport(gpu, C, H, W, torch.full((3,), bg, device=gpu))
    out = torch.full((C, H, W), 7.0, device=gpu)
    rep.add(image, gt, ViewRegion(mask), out_image=out)
    want = torch.clamp(image, 0.0, 1.0)
    want.permute(1, 2, 0)[mask[0] == 0] = bg
    torch.cuda.synchronize(gpu)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    out2 = torch.empty_like(out)
    rep.add(image, gt, None, out_image=out2)                  # no region: clamp only
    assert torch.equal(out2.view(torch.int32), torch.clamp(image, 0.0, 1.0).view(torch.int32))


def test_runs_are_bitwise_identical_and_add_many_equals_single_adds(gpu, hip_lib):
    from moss_amd.loss import ViewRegion
    from moss_amd.metrics import QualityReport
    g = torch.Generator().manual_seed(9)
    C, H, W = 3, 300, 257
    views = []
    for i in range(8):
        gt = torch.rand(C, H, W, generator=g).to(gpu)
        image = (gt.cpu() + 0.1 * torch.randn(C, H, W, generator=g)).to(gpu)
        views.append((image, gt, ViewRegion((torch.rand(H, W, generator=g) < 0.7).float().to(gpu)) if i % 3 else None))
    states = []
    for mode in ("many", "many", "single"):
        rep = QualityReport(gpu, C, H, W, torch.ones(3, device=gpu), per_view_capacity=8)
        if mode == "many":
            rep.add_many(views)
        else:
            for v in views:
                rep.add(*v)
        torch.cuda.synchronize(gpu)
        states.append((rep.state.clone(), rep.per_view()))
    for st, pv in states[1:]:
        assert torch.equal(st, states[0][0]) and torch.equal(pv.view(torch.int32), states[0][1].view(torch.int32))
    assert states[0][1].shape == (8, 3) and int(states[0][0].view(torch.int64)[3]) == 8
    rep = QualityReport(gpu, C, H, W, torch.ones(3, device=gpu), per_view_capacity=8)
    rep.add_many(views + views[:3])                            # eleven views: two launches, the per-view buffer keeps the first eight
    assert rep.means()["n"] == 11 and torch.equal(rep.per_view(), states[0][1])


def test_multiview_render_and_report_in_one_captured_graph(gpu, hip_lib):
    """B = 4 forward-only renders (MultiViewRender, four streams) + report.add_many, captured in ONE GraphedStep: one replay adds the four
    views, two replays add exactly twice the sums (x + x is exact), no allocation between replays; the values equal an eager report."""
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.graphs import GraphedStep
    from moss_amd.loss import ViewRegion
    from moss_amd.metrics import QualityReport
    from moss_amd.multiview import MultiViewRender
    from tests.test_gpu_multiview import _setup
    scene, cams, gts, bg, T = _setup(gpu, 4)
    pc = GaussianSet(scene, sh_degree=3, device=gpu, unified_features=True)
    tl = (0.01 * torch.randn(scene.P, 3, generator=torch.Generator().manual_seed(3))).to(gpu)
    mr = MultiViewRender(pc, cams, bg, transforms=T, translation=tl)
    regions = [ViewRegion(m) for _, m in gts]
    C, H, W = gts[0][0].shape
    rep = QualityReport(gpu, C, H, W, bg, per_view_capacity=8)

    def fn():
        outs = mr.compute()
        rep.add_many([(outs[b][0], gts[b][0], regions[b]) for b in range(4)])
        return outs

    mr.compute()
    torch.cuda.synchronize(gpu)
    step = GraphedStep(fn, warmup=1, device=gpu, context=mr.views[0].ctx, extra_contexts=[v.ctx for v in mr.views[1:]])
    rep.reset()
    torch.cuda.synchronize(gpu)
    step()
    torch.cuda.synchronize(gpu)
    s1 = rep.state.clone()
    mem = torch.cuda.memory_allocated(gpu)
    outs = step()
    torch.cuda.synchronize(gpu)
    assert torch.cuda.memory_allocated(gpu) == mem
    s2 = rep.state.clone()
    mr.check()
    f1, f2 = s1.view(torch.float64), s2.view(torch.float64)
    assert int(s1.view(torch.int64)[3]) == 4 and int(s2.view(torch.int64)[3]) == 8
    for k in range(3):
        assert f2[k].item() == 2 * f1[k].item(), k
    eager = QualityReport(gpu, C, H, W, bg, per_view_capacity=4)
    eager.add_many([(outs[b][0].clone(), gts[b][0], regions[b]) for b in range(4)])
    assert torch.equal(eager.state[:32], s1[:32])
    assert torch.equal(eager.per_view(), rep.per_view()[:4]) and torch.equal(rep.per_view()[:4], rep.per_view()[4:])
    assert 0.0 < f1[2].item() / 4 < 1.0


def test_evaluate_views_matches_quality_torch_of_render(gpu, hip_lib):
    from moss_amd.diff_gaussian_rasterization import RasterContext
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import camera_view, render
    from moss_amd.loss import ViewRegion
    from moss_amd.metrics import evaluate_views, quality_torch
    scene = scenes.config2()
    c0 = scene.camera
    cams = [camera_view(scenes.make_camera(c0.W, c0.H, float(c0.K[0, 0]), float(c0.K[1, 1]), float(c0.K[0, 2]), float(c0.K[1, 2]), R, t), gpu)
            for R, t in scenes.look_at_ring(8)]
    pc = GaussianSet(scene, sh_degree=3, device=gpu, unified_features=True)
    T = (torch.eye(3) + 0.05 * torch.randn(scene.P, 3, 3, generator=torch.Generator().manual_seed(1234))).to(gpu)
    tl = (0.01 * torch.randn(scene.P, 3, generator=torch.Generator().manual_seed(3))).to(gpu)
    bg = torch.ones(3, device=gpu)
    g = torch.Generator().manual_seed(11)
    gts, masks = [], []
    for i in range(8):
        gts.append((torch.rand(3, c0.H, c0.W, generator=g) * 1.2 - 0.1).to(gpu).contiguous())
        m = torch.zeros(1, c0.H, c0.W)
        y0, x0 = 40 + 10 * i, 60 + 5 * i
        m[:, y0:y0 + 300, x0:x0 + 250] = 1
        masks.append(m.to(gpu))
    regions = [ViewRegion(m) if i != 3 else None for i, m in enumerate(masks)]
    lpips_fn = lambda a, b: (a - b).abs().mean()              # a stand-in with a known value: the L1 of the image it is handed
    got = evaluate_views(pc, cams, gts, regions, bg, transforms=T, translation=tl, lpips_fn=lpips_fn)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, fused_activations=False, transforms_in_op=True,
                           pose_in_op=True, raw_parameters_in_op=True, raster_context=RasterContext())
    acc = [0.0, 0.0, 0.0]
    for i, cam in enumerate(cams):
        with torch.no_grad():
            image = render(cam, pc, pipe, bg, transforms=T, translation=tl)["render"]
        vals = quality_torch(image.double().cpu(), gts[i].double().cpu(), None if regions[i] is None else masks[i].cpu(), bg.cpu())
        for k in range(3):
            acc[k] += float(vals[k])
    assert got["n"] == 8
    assert abs(got["l1"] - acc[0] / 8) < 1e-6, (got["l1"], acc[0] / 8)
    assert abs(got["psnr"] - acc[1] / 8) < 1e-4, (got["psnr"], acc[1] / 8)
    assert abs(got["ssim"] - acc[2] / 8) < 1e-5, (got["ssim"], acc[2] / 8)
    assert abs(got["lpips"] - got["l1"]) < 1e-6, (got["lpips"], got["l1"])
