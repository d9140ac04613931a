"""The S3IM term on the device (C ABI moss_s3im_loss, csrc/s3im.hip; moss_amd.loss.s3im_fused / s3im_loss_roi_fused): against the
reference's own numbers (tests/golden/s3im.npz) and the float64 torch restatement, R = 1 against the SSIM kernels, MOSS's call pattern,
determinism, no host synchronisation, capture in a hipGraph with a change of view, and the refusals.

The bars are those of the fused SSIM loss (test_gpu_ops.py::test_fused_moss_loss_matches_reference_golden): values within 2e-6, gradients
within 2e-5 of their largest element.
"""
import os

import numpy as np
import pytest
import torch

from moss_amd.graphs import capturing
from moss_amd.loss import ViewRegion, s3im, s3im_fused, s3im_loss_roi_fused, ssim_fused
from tests import helpers as hp

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "s3im.npz")


def _region(H, W, rect, device):
    x, y, w, h = rect
    m = torch.zeros(1, H, W, dtype=torch.uint8)
    m[0, max(y, 0):y + h, max(x, 0):x + w] = 1
    return ViewRegion(m.to(device), rect=rect)


def _embed(crop, H, W, x, y, g):
    """A (C,H,W) frame of noise with ``crop`` at (x, y): what lies outside the rectangle must not matter."""
    f = torch.rand(crop.shape[0], H, W, generator=g, dtype=crop.dtype)
    f[:, y:y + crop.shape[1], x:x + crop.shape[2]] = crop
    return f


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
@pytest.mark.parametrize("R", [10, 3])
def test_s3im_fused_matches_reference_golden(gpu, hip_lib, name, R):
    """s3im_fused on the crops and s3im_loss_roi_fused on a frame holding them, against the reference's own s3im_fun."""
    g = np.load(GOLDEN)
    src = torch.from_numpy(g[f"{name}_src_q"]).float() / 128.0
    tar = torch.from_numpy(g[f"{name}_tar_q"]).float() / 128.0
    ref_v, ref_g = float(g[f"{name}_value_r{R}"]), g[f"{name}_grad_r{R}"]
    rows = g["e_grad_rows"] if name == "e" else slice(None)
    a = src.to(gpu).unsqueeze(0).requires_grad_(True)
    v = s3im_fused(a, tar.to(gpu).unsqueeze(0), repeat_time=R)
    v.backward()
    assert abs(float(v.detach()) - ref_v) < 2e-6
    assert hp.rel_err(a.grad[0].cpu().numpy()[:, rows], ref_g) < 2e-5
    # the same crop inside a frame, at an offset that is no multiple of any tile edge
    gen = torch.Generator().manual_seed(3)
    C, h, w = src.shape
    H, W, x, y = h + 19, w + 37, 29, 11
    frame, gt_frame = _embed(src, H, W, x, y, gen), _embed(tar, H, W, x, y, gen)
    region = _region(H, W, (x, y, w, h), gpu)
    X = frame.to(gpu).requires_grad_(True)
    v2 = s3im_loss_roi_fused(X, gt_frame.to(gpu), region, repeat_time=R)
    v2.backward()
    gx = X.grad.cpu().numpy()
    assert abs(float(v2.detach()) - ref_v) < 2e-6
    assert hp.rel_err(gx[:, y:y + h, x:x + w][:, rows], ref_g) < 2e-5
    off = np.ones((H, W), bool); off[y:y + h, x:x + w] = False
    assert float(np.abs(gx[:, off]).max(initial=0.0)) == 0.0


CASES = [
    # (C, H, W), rect (x, y, w, h) as the device words say it (may stick out of the frame), R
    ((3, 512, 512), (170, 44, 172, 424), 10),         # MOSS's person rectangle at 512^2
    ((3, 1024, 1024), (301, 97, 345, 848), 10),       # ... at 1024^2
    ((3, 97, 131), (0, 0, 131, 97), 10),              # the whole odd-sized frame
    ((3, 70, 90), (0, 23, 41, 47), 7),                # touching the left edge
    ((3, 70, 90), (55, 0, 35, 33), 10),               # touching the top and right edges
    ((3, 70, 90), (13, 40, 60, 30), 4),               # touching the bottom edge
    ((3, 70, 90), (61, 50, 100, 100), 10),            # sticking out to the right / bottom
    ((3, 70, 90), (-9, -5, 39, 25), 2),               # sticking out to the left / top
    ((1, 33, 65), (5, 3, 3, 2), 16),                  # narrower than the window
    ((2, 41, 29), (3, 4, 17, 30), 1),
    ((3, 64, 64), (7, 9, 31, 33), 5),
]


@pytest.mark.parametrize("shape,rect,R", CASES)
def test_s3im_roi_matches_float64_torch(gpu, hip_lib, shape, rect, R):
    """Random frames and rectangles against moss_amd.loss.s3im in float64 on the clipped crop; the gradient is exactly zero off it."""
    C, H, W = shape
    x, y, w, h = rect
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
    g = torch.Generator().manual_seed(H * 1000 + W + R)
    img = torch.rand(C, H, W, generator=g); gt = torch.rand(C, H, W, generator=g) * (torch.rand(1, H, W, generator=g) > 0.3)
    a = img[:, y0:y1, x0:x1].double().unsqueeze(0).requires_grad_(True)
    ref = s3im(a, gt[:, y0:y1, x0:x1].double().unsqueeze(0), repeat_time=R)
    ref.backward()
    region = _region(H, W, (x0, y0, x1 - x0, y1 - y0), gpu)
    region.rect[:4] = torch.tensor(rect, dtype=torch.int32, device=gpu)      # (the kernel clips what the device words say)
    X = img.to(gpu).requires_grad_(True)
    v = s3im_loss_roi_fused(X, gt.to(gpu), region, repeat_time=R)
    (v * 1.0).backward()
    gx = X.grad.cpu()
    err_v, err_g = abs(float(v.detach()) - float(ref.detach())), hp.rel_err(gx[:, y0:y1, x0:x1].numpy(), a.grad[0].numpy())
    print(f"{shape} {rect} R={R}: value {err_v:.2e}, gradient {err_g:.2e}")
    assert err_v < 2e-6 and err_g < 2e-5
    off = torch.ones(H, W, dtype=torch.bool); off[y0:y1, x0:x1] = False
    assert float(gx[:, off].abs().sum()) == 0.0


@pytest.mark.parametrize("shape", [(3, 97, 131), (3, 424, 172), (1, 5, 3)])
def test_s3im_with_repeat_one_is_the_ssim_kernels(gpu, hip_lib, shape):
    """R = 1 is plain SSIM: s3im_fused(x, y, 1) == 1 - ssim_fused(x, y) within the SSIM bars, value and gradient."""
    g = torch.Generator().manual_seed(sum(shape))
    img = torch.rand(*shape, generator=g).to(gpu); gt = torch.rand(*shape, generator=g).to(gpu)
    a = img.clone().requires_grad_(True); b = img.clone().requires_grad_(True)
    v = s3im_fused(a.unsqueeze(0), gt.unsqueeze(0), repeat_time=1)
    s = 1.0 - ssim_fused(b.unsqueeze(0), gt.unsqueeze(0))
    v.backward(); s.backward()
    assert abs(float(v.detach()) - float(s.detach())) < 2e-6
    assert hp.rel_err(a.grad.cpu().numpy(), b.grad.cpu().numpy()) < 2e-5


def test_s3im_fused_is_a_drop_in_for_the_reference_s3im(gpu, hip_lib):
    """Called as train_ZJU.py:123,131 call it: two (1,3,h,w) crops of the rendered and the true frame, 0.3 * s3im beside other terms,
    against autograd through the torch form.  A batch > 1 goes to the torch form (which fails as the reference's reshape does, after
    drawing the same permutations); CPU tensors are refused."""
    g = torch.Generator().manual_seed(17)
    image0 = torch.rand(3, 200, 160, generator=g).to(gpu); gt_image = torch.rand(3, 200, 160, generator=g).to(gpu)
    x, y, w, h = 23, 17, 101, 160
    res = []
    for fn, dt in ((s3im_fused, torch.float32), (s3im, torch.float64)):       # (the torch form in float64: the yardstick)
        image = image0.to(dt).clone().requires_grad_(True)
        img_pred = image[:, y:y + h, x:x + w].unsqueeze(0)
        img_gt = gt_image.to(dt)[:, y:y + h, x:x + w].unsqueeze(0)
        s3im_loss = fn(img_pred, img_gt)
        loss = 0.8 * (img_pred - img_gt).abs().mean() + 0.3 * s3im_loss
        loss.backward()
        res.append((float(s3im_loss.detach()), image.grad.clone()))
    assert abs(res[0][0] - res[1][0]) < 2e-6
    assert hp.rel_err(res[0][1].cpu().numpy(), res[1][1].cpu().numpy()) < 2e-5
    two = torch.rand(2, 3, 8, 9, device=gpu)
    torch.manual_seed(1)
    with pytest.raises(RuntimeError):
        s3im(two, two)
    state = torch.random.get_rng_state()
    torch.manual_seed(1)
    with pytest.raises(RuntimeError):
        s3im_fused(two, two)
    assert torch.equal(torch.random.get_rng_state(), state)
    with pytest.raises(RuntimeError):
        s3im_fused(image0.cpu().unsqueeze(0), gt_image.cpu().unsqueeze(0))


def test_s3im_is_bitwise_deterministic(gpu, hip_lib):
    """Two calls on the same inputs give the same bits (fixed-order sums, no atomics)."""
    g = torch.Generator().manual_seed(4)
    img = torch.rand(3, 512, 512, generator=g).to(gpu); gt = torch.rand(3, 512, 512, generator=g).to(gpu)
    region = _region(512, 512, (170, 44, 172, 424), gpu)
    out = []
    for _ in range(2):
        X = img.clone().requires_grad_(True)
        v = s3im_loss_roi_fused(X, gt, region)
        v.backward()
        out.append((v.detach().clone(), X.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_s3im_does_not_synchronise(gpu, hip_lib):
    """One eager forward + backward of each form runs clean under torch.cuda.set_sync_debug_mode("error")."""
    from moss_amd.loss import backward_from_loss
    g = torch.Generator().manual_seed(8)
    img = torch.rand(3, 256, 256, generator=g).to(gpu); gt = torch.rand(3, 256, 256, generator=g).to(gpu)
    region = _region(256, 256, (40, 10, 90, 230), gpu)
    X = img.clone().requires_grad_(True)
    torch.cuda.synchronize(gpu)
    torch.cuda.set_sync_debug_mode("error")
    try:
        backward_from_loss(s3im_loss_roi_fused(X, gt, region))
        (0.3 * s3im_fused(X[:, 10:240, 40:130].unsqueeze(0), gt[:, 10:240, 40:130].unsqueeze(0))).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize(gpu)
    assert bool(torch.isfinite(X.grad).all())


def test_s3im_changes_view_inside_a_captured_graph(gpu, hip_lib):
    """s3im_loss_roi_fused + its backward captured once: ``ViewRegion.copy_`` switches the view, and every replay equals the eager
    evaluation on that view bit for bit."""
    from moss_amd.loss import backward_from_loss
    H = W = 256
    g = torch.Generator().manual_seed(5)
    img = torch.rand(3, H, W, generator=g).to(gpu); gt = torch.rand(3, H, W, generator=g).to(gpu)
    views = [_region(H, W, (20, 30, 100, 180), gpu), _region(H, W, (131, 7, 90, 240), gpu)]

    def run(region):
        X = img.clone().requires_grad_(True)
        v = s3im_loss_roi_fused(X, gt, region)
        backward_from_loss(v)
        return v.detach().clone(), X.grad.clone()

    eager = [run(v) for v in views]
    live = _region(H, W, (20, 30, 100, 180), gpu).copy_(views[0])
    X = img.clone().requires_grad_(True)
    val = torch.zeros((), device=gpu); gimg = torch.zeros_like(img)

    def body():
        X.grad = None
        v = s3im_loss_roi_fused(X, gt, live)
        backward_from_loss(v)
        val.copy_(v.detach()); gimg.copy_(X.grad)

    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    with capturing(graph, stream=side):
        body()
    for k in (1, 0, 1):
        live.copy_(views[k])
        graph.replay()
        torch.cuda.synchronize(gpu)
        assert torch.equal(val, eager[k][0]) and torch.equal(gimg, eager[k][1])
    assert not torch.equal(eager[0][1], eager[1][1])


def test_s3im_refusals_and_empty_region(gpu, hip_lib):
    """An empty rectangle: the value is NaN (a mean over nothing), every gradient element zero or NaN.  repeat outside 1..16, a short
    workspace, sizes <= 0 and missing outputs are refused with an error code and a message, nothing is launched."""
    from moss_amd._lib import lib
    L = lib()
    H, W = 40, 56
    g = torch.Generator().manual_seed(2)
    img = torch.rand(3, H, W, generator=g).to(gpu); gt = torch.rand(3, H, W, generator=g).to(gpu)
    empty = ViewRegion(torch.zeros(1, H, W, dtype=torch.uint8, device=gpu))
    X = img.clone().requires_grad_(True)
    v = s3im_loss_roi_fused(X, gt, empty)
    (v * 1.0).backward()
    assert bool(torch.isnan(v.detach()))
    assert bool(((X.grad == 0) | torch.isnan(X.grad)).all())
    for R in (0, 17, -3):
        with pytest.raises(RuntimeError):
            s3im_fused(img.unsqueeze(0), gt.unsqueeze(0), repeat_time=R)
    nbytes = int(L.moss_s3im_workspace_bytes(3, H, W))
    assert nbytes > 0 and int(L.moss_s3im_workspace_bytes(3, -1, W)) == 0
    out = torch.full((2,), 7.0, device=gpu); d = torch.full_like(img, 7.0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    stream = torch.cuda.current_stream(gpu).cuda_stream

    def call(C=3, h=H, w=W, R=10, nb=nbytes, out_p=None):
        return L.moss_s3im_loss(C, h, w, img.data_ptr(), gt.data_ptr(), None, R, out.data_ptr() if out_p is None else out_p,
                                d.data_ptr(), ws.data_ptr(), nb, stream)

    assert call(R=0) < 0 and b"repeat" in L.moss_last_error()
    assert call(R=17) < 0 and b"repeat" in L.moss_last_error()
    assert call(nb=nbytes - 1) < 0 and b"workspace" in L.moss_last_error()
    assert call(h=-1) < 0 and call(C=0) < 0 and b"positive" in L.moss_last_error()
    assert call(out_p=0) < 0 and b"NULL" in L.moss_last_error()
    torch.cuda.synchronize(gpu)
    assert bool((out == 7.0).all()) and bool((d == 7.0).all())           # (nothing was launched)
    assert call() == 0
    torch.cuda.synchronize(gpu)
    ref = s3im(img.double().unsqueeze(0).cpu(), gt.double().unsqueeze(0).cpu())
    assert abs(float(out[0]) - float(ref)) < 2e-6 and abs(float(out[0] + out[1]) - 1.0) < 1e-6
