"""GPU tests of the remaining entry points and of the edge cases the domain offers."""
import numpy as np
import pytest
import torch

from moss_amd import scenes
from moss_amd.graphs import capturing
from oracle import oracle
from tests import helpers as hp

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- fused loss
@pytest.mark.parametrize("shape", [(3, 128, 128), (3, 70, 100), (3, 512, 512)])
def test_fused_loss_matches_torch_reference(gpu, hip_lib, shape):
    """Tolerance: loss value 1e-6 absolute (fp32 sums of <= 786k terms), gradients 2e-5 of their max."""
    from moss_amd.loss import training_loss, training_loss_fused
    C, H, W = shape
    g = torch.Generator().manual_seed(3)
    img = torch.rand(C, H, W, generator=g); gt = scenes.synthetic_target(H, W)
    alpha = torch.rand(1, H, W, generator=g); mask = (torch.rand(1, H, W, generator=g) > 0.5).float()
    a = img.double().requires_grad_(True); b = alpha.double().requires_grad_(True)
    ref = training_loss(a, b, gt.double(), mask.double())           # float64 torch reference on the CPU
    ref.backward()
    x = img.to(gpu).requires_grad_(True); al = alpha.to(gpu).requires_grad_(True)
    out = training_loss_fused(x, al, gt.to(gpu), mask.to(gpu))
    (out * 1.0).backward()
    assert abs(float(out) - float(ref)) < 1e-6
    assert hp.rel_err(x.grad.cpu().numpy(), a.grad.numpy()) < 2e-5
    assert hp.rel_err(al.grad.cpu().numpy(), b.grad.numpy()) < 2e-5


# (the last three: more than 768 workgroups -- three per CU -- so the launcher picks the instantiations that skip the filters of empty
#  tiles, loss.hip "EMPTY TILES"; the others run the plain ones)
@pytest.mark.parametrize("shape,blobs", [((3, 160, 200), 2), ((3, 512, 512), 1), ((3, 96, 96), 0),
                                         ((3, 1024, 1024), 2), ((3, 700, 900), 2), ((3, 544, 544), 0)])
def test_fused_loss_on_masked_frames_with_empty_tiles(gpu, hip_lib, shape, blobs):
    """MOSS's frames are masked people on black: most 32x32 tiles of a frame are exactly zero in BOTH images.  The loss kernels skip
    the filters there (loss.hip, "EMPTY TILES") -- the values they leave must be the general path's: checked against the float64 torch
    reference at the tolerances of the dense test, the gradient is exactly +0 wherever a tile and its neighbours are empty, and a frame
    with NO content at all (blobs = 0) gives SSIM = 1 to rounding, L1 = 0 and a zero image gradient."""
    from moss_amd.loss import training_loss, training_loss_fused
    C, H, W = shape
    g = torch.Generator().manual_seed(9)
    yy, xx = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    m = torch.zeros(H, W)
    for k in range(blobs):                                   # irregular blobs that cross tile borders at odd offsets
        cx, cy, r = (0.3 + 0.37 * k) * W, (0.45 + 0.2 * k) * H, 0.17 * min(H, W)
        m = torch.maximum(m, ((xx - cx) ** 2 + ((yy - cy) * 0.8) ** 2 < r * r).float())
    img = torch.rand(C, H, W, generator=g) * m
    gt = torch.rand(C, H, W, generator=g) * torch.roll(m, shifts=(3, -5), dims=(0, 1))       # the target's silhouette is not the render's
    alpha = torch.rand(1, H, W, generator=g) * m; mask = m[None].clone()
    a = img.double().requires_grad_(True); b = alpha.double().requires_grad_(True)
    ref = training_loss(a, b, gt.double(), mask.double())
    ref.backward()
    x = img.to(gpu).requires_grad_(True); al = alpha.to(gpu).requires_grad_(True)
    terms = torch.zeros(4, device=gpu)
    out = training_loss_fused(x, al, gt.to(gpu), mask.to(gpu), terms_out=terms)
    (out * 1.0).backward()
    assert abs(float(out) - float(ref)) < 1e-6
    gx = x.grad.cpu()
    assert hp.rel_err(gx.numpy(), a.grad.numpy()) < 2e-5 or (blobs == 0 and float(gx.abs().max()) == 0.0)
    assert hp.rel_err(al.grad.cpu().numpy(), b.grad.numpy()) < 2e-5 or float(b.grad.abs().max()) == 0.0
    # exactly +0 (not a tiny number, not -0) where nothing is within a tile + its neighbours of content
    content = ((img.abs().sum(0) + gt.abs().sum(0)) > 0).float()[None, None]
    near = torch.nn.functional.max_pool2d(content, kernel_size=2 * 64 + 1, stride=1, padding=64)[0, 0] > 0
    far = ~near
    if far.any():
        vals = gx[:, far]
        assert float(vals.abs().max()) == 0.0 and not bool(torch.signbit(vals).any())
    if blobs == 0:
        assert abs(float(terms[2]) - 1.0) < 1e-6 and float(terms[1]) == 0.0


@pytest.mark.parametrize("i", [0, 1])
def test_fused_loss_matches_reference_golden(gpu, hip_lib, i):
    """The HIP loss kernels against the REFERENCE'S OWN numbers, no restatement in between: tests/golden/loss.npz
    holds l1_loss / ssim values, total = l1 + 0.2 (1 - ssim) and its autograd gradient as computed by the reference's
    utils/loss_utils.py:41-87 (imported in the build container by tests/golden/make_golden.py, float64 inputs) on two random image
    pairs (48x40: ragged against the kernels' 32x32 tiles; 64x64).  lambda_mask = 0 switches the mask term off, as the fixture has
    none.  Tolerances: values 2e-6 absolute (float32 kernels, sums of <= 12k terms; the reference's own float32 evaluation of ssim
    differs from its float64 one by up to 1e-7), gradient 2e-5 of its largest element."""
    import os
    from moss_amd.loss import training_loss_fused
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss.npz"))
    a = torch.from_numpy(g[f"l{i}_a"]).float().to(gpu).requires_grad_(True)
    b = torch.from_numpy(g[f"l{i}_b"]).float().to(gpu)
    _, H, W = a.shape
    alpha = torch.zeros(1, H, W, device=gpu, requires_grad=True); mask = torch.zeros(1, H, W, device=gpu)
    terms = torch.zeros(4, device=gpu)
    out = training_loss_fused(a, alpha, b, mask, lambda_dssim=0.2, lambda_mask=0.0, terms_out=terms)
    (out * 1.0).backward()
    total, l1, ssim_v, _ = [float(x) for x in terms.cpu()]
    assert abs(l1 - float(g[f"l{i}_l1"])) < 2e-6
    assert abs(ssim_v - float(g[f"l{i}_ssim"])) < 2e-6
    assert abs(total - float(g[f"l{i}_total"])) < 2e-6 and float(out) == total
    assert hp.rel_err(a.grad.cpu().numpy(), g[f"l{i}_grad"]) < 2e-5
    assert float(alpha.grad.abs().max()) == 0.0               # lambda_mask = 0: no gradient reaches alpha


@pytest.mark.parametrize("i", [0, 1])
def test_ssim_fused_is_a_drop_in_for_the_reference_ssim(gpu, hip_lib, i):
    """moss_amd.loss.ssim_fused -- what patches/train_ZJU.diff binds to MOSS's name `ssim` -- against the REFERENCE'S OWN ssim values
    (tests/golden/loss.npz, utils/loss_utils.py:47-87) and, for the gradient, against autograd through the torch restatement: called
    the way train_ZJU.py:119 calls it, on (1,3,h,w) tensors, inside a larger torch expression."""
    import os
    from moss_amd.loss import ssim, ssim_fused
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss.npz"))
    a0 = torch.from_numpy(g[f"l{i}_a"]).float().to(gpu)
    b = torch.from_numpy(g[f"l{i}_b"]).float().to(gpu)
    res = []
    for fn in (ssim_fused, ssim):
        a = a0.clone().requires_grad_(True)
        v = fn((a * 1.0).unsqueeze(0), b.unsqueeze(0))
        (0.2 * (1.0 - v) + 0.1 * a.mean()).backward()          # MOSS's 0.2 * (1 - ssim) beside another term
        res.append((float(v), a.grad.clone()))
    assert abs(res[0][0] - float(g[f"l{i}_ssim"])) < 2e-6 and abs(res[0][0] - res[1][0]) < 2e-6
    assert hp.rel_err(res[0][1].cpu().numpy(), res[1][1].cpu().numpy()) < 2e-5
    # other windows / batches fall back to the torch expressions; CPU tensors are refused (no CPU path)
    assert abs(float(ssim_fused(a0.unsqueeze(0), b.unsqueeze(0), window_size=7)) - float(ssim(a0.unsqueeze(0), b.unsqueeze(0), window_size=7))) < 1e-7
    with pytest.raises(RuntimeError):
        ssim_fused(a0.cpu(), b.cpu())


@pytest.mark.parametrize("i", [0, 1, 2])
def test_fused_moss_loss_matches_reference_golden(gpu, hip_lib, i):
    """C ABI moss_photometric_loss_roi against the REFERENCE'S OWN numbers for MOSS's own loss expression (tests/golden/loss_moss.npz:
    train_ZJU.py:108-119,131 composed from utils/loss_utils.py by make_golden.py -- L1 and mask L2 over bound_mask, SSIM on its
    bounding rectangle).  Tolerances as for the full-frame kernel: values 2e-6, gradients 2e-5 of their largest element; and the
    gradients are exactly zero off the rectangle (image) / off the mask (alpha)."""
    import os
    from moss_amd.loss import ViewRegion, training_loss_moss_fused
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_moss.npz"))
    img = torch.from_numpy(g[f"m{i}_image"]).to(gpu).requires_grad_(True); gt = torch.from_numpy(g[f"m{i}_gt"]).to(gpu)
    alpha = torch.from_numpy(g[f"m{i}_alpha"]).to(gpu).requires_grad_(True); bk = torch.from_numpy(g[f"m{i}_bkgd_mask"]).float().to(gpu)
    bound = torch.from_numpy(g[f"m{i}_bound_mask"]).to(gpu)
    region = ViewRegion(bound)
    assert region.xywh == tuple(int(v) for v in g[f"m{i}_rect"]) and int(region.rect[4]) == int(g[f"m{i}_bound_mask"].sum())
    terms = torch.zeros(4, device=gpu)
    out = training_loss_moss_fused(img, alpha, gt, bk, region, terms_out=terms)
    (out * 1.0).backward()
    total, l1, ssim_v, mk = [float(x) for x in terms.cpu()]
    assert abs(l1 - float(g[f"m{i}_l1"])) < 2e-6 and abs(ssim_v - float(g[f"m{i}_ssim"])) < 2e-6 and abs(mk - float(g[f"m{i}_mask"])) < 2e-6
    assert abs(total - float(g[f"m{i}_total"])) < 2e-6 and float(out) == total
    gi, ga = img.grad.cpu().numpy(), alpha.grad.cpu().numpy()
    assert hp.rel_err(gi, g[f"m{i}_grad_image"]) < 2e-5
    assert hp.rel_err(ga, g[f"m{i}_grad_alpha"]) < 2e-5
    x, y, w, h = region.xywh
    off = np.ones(gi.shape[1:], bool); off[y:y + h, x:x + w] = False
    assert float(np.abs(gi[:, off]).max(initial=0.0)) == 0.0
    assert float(np.abs(ga[0][g[f"m{i}_bound_mask"][0] == 0]).max(initial=0.0)) == 0.0


@pytest.mark.parametrize("shape,rect", [((3, 512, 512), (150, 40, 210, 430)), ((3, 1024, 1024), (301, 97, 417, 803)), ((3, 200, 330), (0, 0, 330, 200)),
                                        ((3, 96, 96), (37, 41, 11, 9)), ((3, 130, 70), (64, 32, 6, 98))])
def test_fused_moss_loss_matches_torch_expression(gpu, hip_lib, shape, rect):
    """The same at MOSS's frame sizes (a person's bounding region in a 512^2 / 1024^2 frame; rectangles at odd offsets against the 32 x 32
    tiles; a rectangle smaller than the SSIM window; the whole frame), against the float64 torch restatement of the expression
    (``training_loss_moss``, itself pinned by the golden file).  The mask: an ellipse inside the rectangle minus a few holes."""
    from moss_amd.loss import ViewRegion, training_loss_moss, training_loss_moss_fused
    C, H, W = shape
    x, y, w, h = rect
    g = torch.Generator().manual_seed(11)
    yy, xx = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    bound = ((((xx - (x + (w - 1) / 2)) / (w / 2)) ** 2 + ((yy - (y + (h - 1) / 2)) / (h / 2)) ** 2) <= 1.0)
    bound &= torch.rand(H, W, generator=g) > 0.02
    bound[y, x:x + w] = True; bound[y + h - 1, x:x + w] = True; bound[y:y + h, x] = True; bound[y:y + h, x + w - 1] = True   # (the box is tight)
    bound = bound[None].to(torch.uint8)
    img = torch.rand(C, H, W, generator=g); gt = torch.rand(C, H, W, generator=g) * (torch.rand(1, H, W, generator=g) > 0.3)
    alpha = torch.rand(1, H, W, generator=g); bk = (torch.rand(1, H, W, generator=g) > 0.5).float()
    a = img.double().requires_grad_(True); b = alpha.double().requires_grad_(True)
    ref = training_loss_moss(a, b, gt.double(), bk.double(), bound)
    ref.backward()
    region = ViewRegion(bound.to(gpu))
    assert region.xywh == rect
    X = img.to(gpu).requires_grad_(True); A = alpha.to(gpu).requires_grad_(True)
    out = training_loss_moss_fused(X, A, gt.to(gpu), bk.to(gpu), region)
    (out * 1.0).backward()
    assert abs(float(out) - float(ref)) < 2e-6
    assert hp.rel_err(X.grad.cpu().numpy(), a.grad.numpy()) < 2e-5
    assert hp.rel_err(A.grad.cpu().numpy(), b.grad.numpy()) < 2e-5
    off = torch.ones(H, W, dtype=torch.bool); off[y:y + h, x:x + w] = False
    assert float(X.grad.cpu()[:, off].abs().sum()) == 0.0 and float(A.grad.cpu()[0][bound[0] == 0].abs().sum()) == 0.0


def test_fused_moss_loss_edge_cases(gpu, hip_lib):
    """An EMPTY bound_mask: the means over an empty selection are NaN (torch.mean of nothing) and so are the kernels' L1 / mask terms,
    while no gradient element is written as anything but NaN or zero.  A rectangle handed in by the caller that sticks out of the frame is
    clipped to it (the C ABI's contract): same value and gradients as the clipped rectangle.  A mask pixel OUTSIDE the caller's rectangle
    counts for nothing."""
    from moss_amd.loss import ViewRegion, training_loss_moss, training_loss_moss_fused
    H, W = 80, 96
    g = torch.Generator().manual_seed(21)
    img = torch.rand(3, H, W, generator=g).to(gpu); gt = torch.rand(3, H, W, generator=g).to(gpu)
    alpha = torch.rand(1, H, W, generator=g).to(gpu); bk = (torch.rand(1, H, W, generator=g) > 0.5).float().to(gpu)
    # (1) empty mask
    empty = ViewRegion(torch.zeros(1, H, W, dtype=torch.uint8, device=gpu))
    assert empty.xywh == (0, 0, 0, 0) and int(empty.rect[4]) == 0
    terms = torch.zeros(4, device=gpu)
    X = img.clone().requires_grad_(True); A = alpha.clone().requires_grad_(True)
    out = training_loss_moss_fused(X, A, gt, bk, empty, terms_out=terms)
    (out * 1.0).backward()
    assert bool(torch.isnan(terms[1])) and bool(torch.isnan(terms[3])) and bool(torch.isnan(out))
    # (MOSS's own expression does not get that far: ssim() of the 0 x 0 crop raises inside conv2d)
    with pytest.raises(RuntimeError):
        training_loss_moss(img.cpu().double(), alpha.cpu().double(), gt.cpu().double(), bk.cpu().double(), torch.zeros(1, H, W, dtype=torch.uint8))
    gx = X.grad.cpu()
    assert bool(((gx == 0) | torch.isnan(gx)).all())
    # (2) a rectangle that sticks out of the frame == the clipped rectangle
    m = torch.zeros(1, H, W, dtype=torch.uint8); m[0, 50:, 60:] = 1; m[0, 55, 70] = 0
    res = []
    for rect in ((60, 50, 100, 100), (60, 50, W - 60, H - 50)):              # (sticking out to the right / bottom)
        region = ViewRegion(m.to(gpu), rect=rect)
        X = img.clone().requires_grad_(True); A = alpha.clone().requires_grad_(True)
        out = training_loss_moss_fused(X, A, gt, bk, region)
        (out * 1.0).backward()
        res.append((out.detach().clone(), X.grad.clone(), A.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    ref = training_loss_moss(img.cpu().double(), alpha.cpu().double(), gt.cpu().double(), bk.cpu().double(), m)
    assert abs(float(res[1][0]) - float(ref)) < 2e-6
    # (... and to the left / top: a negative corner is clipped at 0, the far edge stays where it was)
    m3 = torch.zeros(1, H, W, dtype=torch.uint8); m3[0, :20, :30] = 1; m3[0, 4, 7] = 0
    res3 = []
    for rect in ((-9, -5, 39, 25), (0, 0, 30, 20)):
        region = ViewRegion(m3.to(gpu), rect=rect) if rect[0] >= 0 else ViewRegion(m3.to(gpu), rect=(0, 0, 30, 20))
        if rect[0] < 0:
            region.rect[:4] = torch.tensor(rect, dtype=torch.int32, device=gpu)      # (the C ABI takes what the device words say)
        X = img.clone().requires_grad_(True); A = alpha.clone().requires_grad_(True)
        out = training_loss_moss_fused(X, A, gt, bk, region)
        (out * 1.0).backward()
        res3.append((out.detach().clone(), X.grad.clone(), A.grad.clone()))
    assert torch.equal(res3[0][0], res3[1][0]) and torch.equal(res3[0][1], res3[1][1]) and torch.equal(res3[0][2], res3[1][2])
    # (3) mask pixels outside the caller's rectangle count for nothing: the same as the mask cut to the rectangle
    m2 = m.clone(); m2[0, 3:9, 4:30] = 1
    r2 = ViewRegion(m2.to(gpu), rect=(60, 50, W - 60, H - 50))
    assert int(r2.rect[4]) == int(m.sum())
    X = img.clone().requires_grad_(True); A = alpha.clone().requires_grad_(True)
    out = training_loss_moss_fused(X, A, gt, bk, r2)
    (out * 1.0).backward()
    assert torch.equal(out.detach(), res[1][0]) and torch.equal(X.grad, res[1][1]) and torch.equal(A.grad, res[1][2])


def test_fused_moss_loss_changes_view_inside_a_captured_graph(gpu, hip_lib):
    """The rectangle, the mask and its pixel count live in device memory: a captured loss changes view by ``ViewRegion.copy_`` --
    the replay then equals an eager evaluation on the new view, bit for bit."""
    from moss_amd.loss import ViewRegion, training_loss_moss_fused
    H = W = 256
    g = torch.Generator().manual_seed(5)
    img = torch.rand(3, H, W, generator=g).to(gpu); gt = torch.rand(3, H, W, generator=g).to(gpu)
    alpha = torch.rand(1, H, W, generator=g).to(gpu); bk = (torch.rand(1, H, W, generator=g) > 0.5).float().to(gpu)
    def region_of(x, y, w, h):
        m = torch.zeros(1, H, W, dtype=torch.uint8); m[0, y:y + h, x:x + w] = (torch.rand(h, w, generator=g) > 0.2).to(torch.uint8)
        m[0, y, x] = 1; m[0, y + h - 1, x + w - 1] = 1
        return ViewRegion(m.to(gpu), rect=(x, y, w, h))
    views = [region_of(20, 30, 100, 180), region_of(131, 7, 90, 240)]
    def run(region):
        X = img.clone().requires_grad_(True); A = alpha.clone().requires_grad_(True)
        out = training_loss_moss_fused(X, A, gt, bk, region)
        (out * 1.0).backward()
        return out.detach().clone(), X.grad.clone(), A.grad.clone()
    eager = [run(v) for v in views]
    live = region_of(20, 30, 100, 180).copy_(views[0])
    X = img.clone().requires_grad_(True); A = alpha.clone().requires_grad_(True)
    terms = torch.zeros(4, device=gpu); gimg = torch.zeros_like(img); galpha = torch.zeros_like(alpha)
    def body():
        X.grad = None; A.grad = None
        out = training_loss_moss_fused(X, A, gt, bk, live, terms_out=terms)
        (out * 1.0).backward()
        gimg.copy_(X.grad); galpha.copy_(A.grad)
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
        assert torch.equal(terms[0], eager[k][0]) and torch.equal(gimg, eager[k][1]) and torch.equal(galpha, eager[k][2])
    assert not torch.equal(eager[0][1], eager[1][1])


# ---------------------------------------------------------------- distCUDA2
@pytest.mark.parametrize("P", [1, 3, 4, 5, 1000, 6890, 20000])
def test_dist2_bit_exact_vs_bruteforce_oracle(gpu, hip_lib, P):
    from moss_amd.simple_knn._C import distCUDA2
    g = torch.Generator().manual_seed(P)
    pts = scenes.body_points(P, g) if P >= 1000 else torch.randn(P, 3, generator=g)
    if P >= 1000:
        pts[7] = pts[3]                       # exact duplicates -> distance 0 counted
    got = distCUDA2(pts.to(gpu)).cpu().numpy()
    ref = oracle.dist2(pts.numpy())
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("P", [2049, 150_000, 1_000_003])
def test_dist2_at_the_sizes_the_rasterizer_is_tested_at(gpu, hip_lib, P):
    """distCUDA2 sorted its Morton keys in ONE workgroup -- fine at 6 890 points, a cliff at 100k - 1M.  The sort is
    now device-wide (knn.hip: launch_sort_keys; 2049 points = the first size with a cross-tile step, the others not powers of two).
    The C oracle is O(P^2) on one host thread, so up to 150k points the reference here is the same exhaustive search in float32 torch
    on the GPU, in the kernel's operation order ((dx dx + dy dy) + dz dz, each operation rounded; three smallest summed ascending, / 3):
    BIT-EXACT.  At a million points the exhaustive search is out of reach (10^12 pairs): the three nearest other points then come from
    the exact grid k-NN of this library, which ranks by the ROUNDED Euclidean distance -- where two candidates tie after the square
    root it may name the other one as third neighbour, so there: equal within 1e-6 relative, bit-equal for > 99.9 % of the points."""
    from moss_amd.simple_knn._C import distCUDA2
    g = torch.Generator().manual_seed(P)
    pts = scenes.body_points(P, g).to(gpu)
    got = distCUDA2(pts)
    assert float(got.min()) > 0.0
    if P <= 150_000:
        best = torch.empty(P, 3, device=gpu)
        x, y, z = pts[:, 0].contiguous(), pts[:, 1].contiguous(), pts[:, 2].contiguous()
        for r0 in range(0, P, 4096):
            r1 = min(P, r0 + 4096)
            dx = x[None, :] - x[r0:r1, None]; d2 = dx * dx
            dy = y[None, :] - y[r0:r1, None]; d2 = d2 + dy * dy
            dz = z[None, :] - z[r0:r1, None]; d2 = d2 + dz * dz
            d2[torch.arange(r1 - r0, device=gpu), torch.arange(r0, r1, device=gpu)] = float("inf")
            best[r0:r1] = torch.topk(d2, 3, dim=1, largest=False, sorted=True).values
            del dx, dy, dz, d2
        # (the sum and the division by 3 in numpy float32: torch divides by a scalar through a reciprocal multiplication on the GPU)
        b = best.cpu().numpy()
        want = ((b[:, 0] + b[:, 1]) + b[:, 2]) / np.float32(3.0)
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
        return
    from moss_amd.knn_cuda import KnnGrid
    _, idx = KnnGrid(pts).query(pts, 4)                      # the query point itself comes first (distance 0, lowest index on ties)
    d = pts[idx[:, 1:]] - pts[:, None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    b = torch.sort(d2, dim=1).values.cpu().numpy()
    want = ((b[:, 0] + b[:, 1]) + b[:, 2]) / np.float32(3.0)
    got = got.cpu().numpy()
    assert float((np.abs(got - want) / want).max()) < 1e-6
    assert float((got.view(np.uint32) == want.view(np.uint32)).mean()) > 0.999


def test_dist2_empty(gpu, hip_lib):
    from moss_amd.simple_knn._C import distCUDA2
    assert distCUDA2(torch.zeros(0, 3, device=gpu)).shape == (0,)


# ---------------------------------------------------------------- markVisible
def test_mark_visible(gpu, hip_lib):
    from moss_amd.diff_gaussian_rasterization import GaussianRasterizer, GaussianRasterizationSettings
    s = scenes.config1()
    c = s.camera
    pts = s.means3D.clone(); pts[::3, 2] -= 3.0              # push a third behind the near plane
    rs = GaussianRasterizationSettings(c.H, c.W, c.tanfovx, c.tanfovy, s.bg.to(gpu), 1.0, c.viewmatrix.to(gpu),
                                       c.projmatrix.to(gpu), 3, c.campos.to(gpu), False, False)
    vis = GaussianRasterizer(rs).markVisible(pts.to(gpu)).cpu().numpy()
    ref = oracle.mark_visible(pts.numpy(), c.viewmatrix.numpy(), c.projmatrix.numpy())
    np.testing.assert_array_equal(vis, ref)
    assert 0 < vis.sum() < len(vis)


# ---------------------------------------------------------------- edge cases
def test_zero_gaussians(gpu, hip_lib):
    """P == 0 short-circuits both directions with zero-filled outputs (rasterize_points.cu:83,168)."""
    from moss_amd.diff_gaussian_rasterization import _C
    c = scenes.config1().camera
    z = lambda *s: torch.zeros(*s, device=gpu)
    R, color, depth, alpha, radii, gb, bb, ib = _C.rasterize_gaussians(
        torch.tensor([0.2, 0.3, 0.4], device=gpu), z(0, 3), torch.Tensor([]), z(0, 1), z(0, 3), z(0, 4), 1.0, torch.Tensor([]),
        c.viewmatrix.to(gpu), c.projmatrix.to(gpu), c.tanfovx, c.tanfovy, c.H, c.W, z(0, 16, 3), 3, c.campos.to(gpu), False, False)
    assert R == 0 and float(color.abs().sum()) == 0 and float(alpha.abs().sum()) == 0 and radii.numel() == 0
    grads = _C.rasterize_gaussians_backward(
        torch.zeros(3, device=gpu), z(0, 3), radii, torch.Tensor([]), z(0, 3), z(0, 4), 1.0, torch.Tensor([]), c.viewmatrix.to(gpu),
        c.projmatrix.to(gpu), c.tanfovx, c.tanfovy, z(3, c.H, c.W), z(1, c.H, c.W), z(1, c.H, c.W), z(0, 16, 3), 3,
        c.campos.to(gpu), gb, R, bb, ib, alpha, False)
    assert all(g.shape[0] == 0 for g in grads)


def test_everything_culled_gives_background(gpu, hip_lib):
    s = scenes.config1()
    s.means3D[:, 2] -= 10.0                                   # all behind the camera
    d = hp.inputs_of(s, "scale_rot", bg=[0.1, 0.5, 0.9])
    fw = hp.oracle_forward(d)
    t = hp.hip_forward(d, gpu)
    assert t.R == 0 == fw.num_rendered
    np.testing.assert_array_equal(t.color.cpu().numpy(), fw.color)
    np.testing.assert_array_equal(t.radii.cpu().numpy(), 0)
    dc, dd, da = hp.image_grads(d.H, d.W)
    g = hp.hip_backward(d, t, dc, dd, da, gpu)
    for name in ("dL_dmeans3D", "dL_dsh", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dmeans2D"):
        assert float(getattr(g, name).abs().sum()) == 0.0


def _stacked_scene(P, W=64, H=64, spread=0.02, scale=0.15, seed=0, equal_depth_every=0):
    """P big Gaussians piled onto a few tiles: long per-tile lists (sort classes, multi-batch blend)."""
    g = torch.Generator().manual_seed(seed)
    s = scenes.config1(P=P, W=W, H=H)
    s.means3D = torch.randn(P, 3, generator=g) * spread
    if equal_depth_every:
        s.means3D[::equal_depth_every, 2] = 0.0               # identical depths: order must fall back to the index
    s.scales = torch.full((P, 3), scale) * torch.exp(0.2 * torch.randn(P, 3, generator=g))
    s.opacities = torch.sigmoid(torch.randn(P, 1, generator=g) - 3.0)   # faint, so pixels do not saturate early
    s.cov3D_precomp = scenes.covariance_precomp(s.scales, s.rotations)
    s.camera = scenes.make_camera(W, H, 70.0, 70.0, W / 2, H / 2, np.eye(3), np.array([0.0, 0.0, 3.0]))
    return s


@pytest.mark.parametrize("P,ties", [(700, 0), (3000, 0), (3000, 7), (9500, 0)])
def test_long_tile_lists_and_depth_ties(gpu, hip_lib, P, ties):
    """3000 > 2048 and 9500 > 8192 entries per tile exercise the larger sort paths (LDS and global-memory network);
    equal depths must keep ascending Gaussian index (stability of the reference's radix sort)."""
    from tests.test_gpu_parity import _check_forward, _check_backward
    d = hp.inputs_of(_stacked_scene(P, equal_depth_every=ties), "precomp")
    # thousands of faint entries per pixel put many alphas within rounding of 1/255: allow more excluded pixels here
    fw, t, e = _check_forward(d, gpu, max_fragile=3e-2)
    assert (fw.ranges[:, 1] - fw.ranges[:, 0]).max() >= P * 0.9
    _check_backward(d, gpu, fw, t, e)


def test_image_covering_gaussians(gpu, hip_lib):
    """A few Gaussians grown to cover every tile of the image (what an optimiser does to a background splat) among ordinary ones:
    their tile rectangles (up to gx*gy instances each) take the wave-cooperative paths of the histogram, the scatter and the
    per-Gaussian gradient gather.  Results must still match the oracle."""
    from tests.test_gpu_parity import _check_forward, _check_backward
    W, H, P = 200, 136, 1500
    g = torch.Generator().manual_seed(3)
    s = scenes.config1(P=P, W=W, H=H)
    s.means3D = torch.randn(P, 3, generator=g) * torch.tensor([0.9, 0.6, 0.3])
    s.scales = torch.full((P, 3), 0.03) * torch.exp(0.3 * torch.randn(P, 3, generator=g))
    big = torch.arange(0, P, 97)                                  # spread over many waves; 16 of them
    s.scales[big] = torch.tensor([4.0, 3.0, 0.05]) * torch.exp(0.3 * torch.randn(len(big), 3, generator=g))
    s.opacities = torch.sigmoid(torch.randn(P, 1, generator=g))
    s.opacities[big] = 0.05
    s.cov3D_precomp = scenes.covariance_precomp(s.scales, s.rotations)
    s.camera = scenes.make_camera(W, H, 120.0, 120.0, W / 2, H / 2, np.eye(3), np.array([0.0, 0.0, 3.0]))
    d = hp.inputs_of(s, "precomp")
    fw, t, e = _check_forward(d, gpu, max_fragile=1e-2)
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    assert int((fw.tiles_touched == tiles).sum()) >= 8             # really image-covering
    _check_backward(d, gpu, fw, t, e)


def test_heavy_tiles_on_a_ragged_image(gpu, hip_lib):
    """Heavy tiles (lists of 32 entries or more: block-mask scan + LDS-DMA path, 16 wave items per tile; here hundreds of entries)
    on an image whose size is not a multiple of the tile: partial tiles on the right and bottom edge, pixels outside the image
    inside 4x4 blocks."""
    from tests.test_gpu_parity import _check_forward, _check_backward
    s = _stacked_scene(2500, W=70, H=50, spread=0.25, scale=0.12, seed=7)
    d = hp.inputs_of(s, "precomp")
    fw, t, e = _check_forward(d, gpu, max_fragile=3e-2)
    n = fw.ranges[:, 1] - fw.ranges[:, 0]
    assert (n >= 128).sum() >= 6 and n.max() < 2500            # several heavy tiles, including edge ones
    _check_backward(d, gpu, fw, t, e)


@pytest.mark.parametrize("seed", [11, 12])
def test_lists_on_both_sides_of_the_light_heavy_threshold(gpu, hip_lib, seed):
    """Tiles with fewer than 32 entries are blended one pixel per lane (light path, 4 quadrant items), longer ones by wave pairs per
    4x4 block (heavy path, 16 block items).  A blob that thins out towards the image border gives lists of every length from a few
    entries to a few hundred in one frame -- including the 32..127 class that was light until the threshold moved -- so the class
    boundary of the scan block (binning.hip: header[7]) and both blend paths are checked against the oracle together."""
    from tests.test_gpu_parity import _check_forward, _check_backward
    s = _stacked_scene(900, W=112, H=80, spread=0.55, scale=0.04, seed=seed)
    d = hp.inputs_of(s, "precomp")
    fw, t, e = _check_forward(d, gpu, max_fragile=3e-2)
    n = np.asarray(fw.ranges[:, 1] - fw.ranges[:, 0])
    assert ((n > 0) & (n < 32)).sum() >= 3 and ((n >= 32) & (n < 128)).sum() >= 3 and (n >= 128).sum() >= 1, sorted(n.tolist())
    _check_backward(d, gpu, fw, t, e)


def test_more_tiles_than_the_lds_histogram_holds(gpu, hip_lib):
    """2200 x 1504 pixels = 138 x 94 = 12 972 tiles > 8192: the tile histogram and the scatter's slot reservation fall back from LDS
    to global atomics, the scan / tile order / empty-tile fill run over a long tile table."""
    from tests.test_gpu_parity import _check_forward, _check_backward
    W, H, P = 2200, 1504, 3000
    g = torch.Generator().manual_seed(21)
    s = scenes.config1(P=P, W=W, H=H)
    s.means3D = (torch.rand(P, 3, generator=g) - 0.5) * torch.tensor([4.0, 2.7, 0.6])
    s.scales = torch.full((P, 3), 0.02) * torch.exp(0.4 * torch.randn(P, 3, generator=g))
    s.cov3D_precomp = scenes.covariance_precomp(s.scales, s.rotations)
    s.camera = scenes.make_camera(W, H, 1500.0, 1500.0, W / 2, H / 2, np.eye(3), np.array([0.0, 0.0, 3.0]))
    d = hp.inputs_of(s, "scale_rot")
    fw, t, e = _check_forward(d, gpu)
    assert fw.ranges.shape[0] == 138 * 94 and int((fw.ranges[:, 1] > fw.ranges[:, 0]).sum()) > 2000
    _check_backward(d, gpu, fw, t, e)


def test_prefiltered_trap_is_reported(gpu, hip_lib):
    s = scenes.config1()
    s.means3D[0, 2] = -10.0
    d = hp.inputs_of(s, "scale_rot")
    with pytest.raises(RuntimeError, match="prefiltered"):
        hp.hip_forward(d, gpu, prefiltered=True)


def test_debug_mode_runs_stage_checks(gpu, hip_lib):
    d = hp.inputs_of(scenes.config1(), "scale_rot")
    t = hp.hip_forward(d, gpu, debug=True)
    assert t.R > 0


# ---------------------------------------------------------------- Python surface, end to end
def test_render_binding_and_autograd(gpu, hip_lib):
    """render() (gaussian_renderer counterpart) -> autograd.Function -> .backward(): gradients land on the raw parameters and
    on the zero means2D sink (viewspace_points.grad, consumed by MOSS's densification, scene/gaussian_model.py:816-818)."""
    from types import SimpleNamespace
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import render, camera_view
    s = scenes.config1()
    pc = GaussianSet(s, device=gpu)
    cam = camera_view(s.camera, gpu)
    outs = {}
    for cov_py in (True, False):
        pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=cov_py, debug=False)
        pc.zero_grad()
        out = render(cam, pc, pipe, torch.zeros(3, device=gpu))
        assert all(k in out for k in ["render", "render_depth", "render_alpha", "viewspace_points", "visibility_filter", "radii"])
        assert out.get("visibility_filter") is not None and "visibility_filter" in set(out)       # computed on first use, then a plain entry
        loss = out["render"].sum() + out["render_alpha"].sum()
        loss.backward()
        assert out["viewspace_points"].grad is not None and out["viewspace_points"].grad.abs().sum() > 0
        assert out["visibility_filter"].dtype == torch.bool
        outs[cov_py] = (out["render"].detach().cpu(), pc._xyz.grad.clone().cpu(), pc._scaling.grad.clone().cpu())
    # the two covariance input modes (Python-precomputed vs in-kernel) must agree (gaussian_renderer/__init__.py:88-93)
    assert hp.rel_err(outs[True][0].numpy(), outs[False][0].numpy()) < 1e-4
    assert hp.rel_err(outs[True][1].numpy(), outs[False][1].numpy()) < 1e-3
    assert hp.rel_err(outs[True][2].numpy(), outs[False][2].numpy()) < 1e-3


def test_convert_shs_python_matches_native(gpu, hip_lib):
    """pipe.convert_SHs_python (SH->RGB in torch, gaussian_renderer/__init__.py:100-105) vs the in-kernel SH path."""
    from types import SimpleNamespace
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import render, camera_view
    s = scenes.config1()
    pc = GaussianSet(s, device=gpu)
    cam = camera_view(s.camera, gpu)
    imgs = []
    for sh_py in (True, False):
        pipe = SimpleNamespace(convert_SHs_python=sh_py, compute_cov3D_python=False, debug=False)
        with torch.no_grad():
            imgs.append(render(cam, pc, pipe, torch.zeros(3, device=gpu))["render"].cpu().numpy())
    assert hp.rel_err(imgs[0], imgs[1]) < 1e-5


def test_argument_validation(gpu, hip_lib):
    from moss_amd.diff_gaussian_rasterization import GaussianRasterizer, GaussianRasterizationSettings
    s = scenes.config1(); c = s.camera
    rs = GaussianRasterizationSettings(c.H, c.W, c.tanfovx, c.tanfovy, s.bg.to(gpu), 1.0, c.viewmatrix.to(gpu),
                                       c.projmatrix.to(gpu), 3, c.campos.to(gpu), False, False)
    r = GaussianRasterizer(rs)
    m, m2, o = s.means3D.to(gpu), torch.zeros_like(s.means3D).to(gpu), s.opacities.to(gpu)
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(m, m2, o, shs=None, colors_precomp=None, scales=s.scales.to(gpu), rotations=s.rotations.to(gpu))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(m, m2, o, shs=s.shs.to(gpu), scales=s.scales.to(gpu), rotations=s.rotations.to(gpu), cov3D_precomp=s.cov3D_precomp.to(gpu))
    with pytest.raises(RuntimeError, match="num_points, 3"):
        r(m[:, :2], m2, o, shs=s.shs.to(gpu), scales=s.scales.to(gpu), rotations=s.rotations.to(gpu))


# ---------------------------------------------------------------- flat fused AdamW
def test_flat_adamw_matches_torch_adamw(gpu, hip_lib):
    """Three steps of the flat HIP AdamW vs torch.optim.AdamW on the same gradients: parameters agree to 1e-6 relative."""
    from moss_amd.dist import GradBucket
    from moss_amd.optim import FlatAdamW
    torch.manual_seed(0)
    shapes, lrs = [(1001, 3), (1001, 15, 3), (1001, 1), (1001, 4)], [0.00016, 0.000125, 0.05, 0.001]
    init = [torch.randn(*s) for s in shapes]
    pa = [torch.nn.Parameter(t.clone().to(gpu)) for t in init]
    pb = [torch.nn.Parameter(t.clone().to(gpu)) for t in init]
    ref = torch.optim.AdamW([{"params": [p], "lr": lr} for p, lr in zip(pb, lrs)], lr=0.0, eps=1e-15)
    bucket = GradBucket(pa)
    opt = FlatAdamW([{"params": [p], "lr": lr} for p, lr in zip(pa, lrs)], bucket, eps=1e-15)
    for it in range(3):
        bucket.attach()
        grads = [torch.randn(*s, device=gpu) * (it + 1) for s in shapes]
        for p, q, g in zip(pa, pb, grads):
            p.grad.copy_(g); q.grad = g.clone()
        opt.step(); ref.step()
    for p, q in zip(pa, pb):
        assert hp.rel_err(p.detach().cpu().numpy(), q.detach().cpu().numpy()) < 1e-6


# ---------------------------------------------------------------- asynchronous forward / hipGraph capture
def _train_like_step(pc, cam, pipe, bg, weights):
    from moss_amd.gaussian_renderer import render
    pc.zero_grad()
    out = render(cam, pc, pipe, bg)
    loss = (out["render"] * weights).sum() + 0.5 * out["render_alpha"].sum() + 0.1 * out["render_depth"].sum()
    loss.backward()
    grads = [p.grad.detach().clone() for p in pc.parameters()]
    return out["render"].detach().clone(), out["render_alpha"].detach().clone(), out["radii"].clone(), grads


@pytest.fixture
def async_mode():
    import moss_amd.diff_gaussian_rasterization as dgr
    yield dgr
    dgr.set_async(False)


@pytest.mark.parametrize("raw", [False, True])
def test_async_forward_equals_sync_forward(gpu, hip_lib, async_mode, raw):
    """The asynchronous forward (moss_raster_forward_ex with a capacity > 0: no host read-back, capacity-bounded) runs the same kernels
    on the same data: image, alpha, radii and every parameter gradient are BIT-IDENTICAL to the synchronous call (also with raw
    parameters).  A capacity of 0 is neither: the library refuses it before it launches anything."""
    from types import SimpleNamespace
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import camera_view
    s = scenes.config2()
    pc = GaussianSet(s, device=gpu)
    cam = camera_view(s.camera, gpu)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raw_parameters_in_op=raw)
    bg = torch.tensor([0.1, 0.2, 0.3], device=gpu)
    w = torch.rand(3, s.camera.H, s.camera.W, device=gpu)
    ref = _train_like_step(pc, cam, pipe, bg, w)
    async_mode.set_async(True)
    first = _train_like_step(pc, cam, pipe, bg, w)            # synchronous: learns the capacity
    assert async_mode._C.ASYNC.capacity > 0
    for _ in range(2):
        got = _train_like_step(pc, cam, pipe, bg, w)          # asynchronous
    async_mode.check_async_status()
    # the context's frame state (per-frame counters of the asynchronous forward, the `frame_state` ARGUMENT of the C ABI since version
    # 2) was used -- no clear kernel ran -- and is all-zero again
    fs = async_mode._C.ASYNC.frame_state
    assert fs is not None and int(fs.count_nonzero()) == 0
    for a, b, c in zip(ref[:3], first[:3], got[:3]):
        assert torch.equal(a, b) and torch.equal(a, c)
    for a, c in zip(ref[3], got[3]):
        assert torch.equal(a, c)
    # capacity 0 (an extension caller's; the context policy never passes it): refused, nothing launched
    from moss_amd._lib import ext
    d = hp.inputs_of(scenes.config1(), "scale_rot")
    a = hp.hip_forward(d, gpu).args
    c = d.cam
    with pytest.raises(RuntimeError, match="capacity 0"):
        ext().rasterize_gaussians(
            a["bg"], a["means3D"], a["colors"], a["opacity"], a["scales"], a["rotations"], d.scale_modifier, a["cov3D"], a["view"],
            a["proj"], c.tanfovx, c.tanfovy, c.H, c.W, a["sh"], d.degree, a["campos"], False, 0, raw_flags=7 if raw else 0, capacity=0)


@pytest.mark.parametrize("size", [1024, 2048])
def test_async_forward_equals_sync_forward_beyond_one_tile_per_sort_thread(gpu, hip_lib, async_mode, size):
    """The asynchronous forward has three shapes by the number of tiles T: T <= 1024 (the bench frame: keys bucketed by the preprocess
    kernel, one tile per thread of the sort workgroups' self-scan), T <= 8192 (the same with up to 8 tiles per thread: 1024 x 1024), and
    beyond that -- the tile histogram no longer fits the LDS -- the scan -> scatter chain of rounds 2-4 with global histogram atomics
    (2048 x 2048: 16 384 tiles).  Each must give the synchronous forward's frame bit for bit, gradients included."""
    from types import SimpleNamespace
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import camera_view
    s = scenes.body_scene(40_000, size, size, 540.0 * size / 512, init_like=False, name=f"body{size}")
    pc = GaussianSet(s, device=gpu)
    cam = camera_view(s.camera, gpu)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raw_parameters_in_op=True)
    bg = torch.tensor([0.1, 0.2, 0.3], device=gpu)
    w = torch.rand(3, size, size, device=gpu)
    ref = _train_like_step(pc, cam, pipe, bg, w)
    async_mode.set_async(True)
    _train_like_step(pc, cam, pipe, bg, w)                    # synchronous: learns the capacity
    for _ in range(2):
        got = _train_like_step(pc, cam, pipe, bg, w)          # asynchronous
    async_mode.check_async_status()
    assert int(async_mode._C.ASYNC.frame_state.count_nonzero()) == 0
    assert float(ref[1].sum()) > 1000.0                       # something was rendered
    for a, c in zip(ref[:3], got[:3]):
        assert torch.equal(a, c)
    for a, c in zip(ref[3], got[3]):
        assert torch.equal(a, c)


def test_async_overflow_renders_nothing_and_is_reported(gpu, hip_lib, async_mode):
    """A frame that needs more (Gaussian, tile) instances than the capacity: background image, zero alpha, zero gradients (never
    an out-of-bounds write), the overflow flag raised at the next status check, and the capacity grown from the needed size."""
    from types import SimpleNamespace
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import camera_view
    s = scenes.config2()
    pc = GaussianSet(s, device=gpu)
    cam = camera_view(s.camera, gpu)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    bg = torch.tensor([0.1, 0.2, 0.3], device=gpu)
    w = torch.rand(3, s.camera.H, s.camera.W, device=gpu)
    ref = _train_like_step(pc, cam, pipe, bg, w)
    async_mode.set_async(True, capacity=2048)                  # far below what config2 needs
    img, alpha, radii, grads = _train_like_step(pc, cam, pipe, bg, w)
    assert torch.equal(img, bg[:, None, None].expand_as(img))
    assert float(alpha.abs().max()) == 0.0
    assert torch.equal(radii, ref[2])                          # preprocess still ran
    for g in grads:
        assert float(g.abs().max()) == 0.0
    with pytest.raises(async_mode.CapacityOverflow, match="needed") as exc:
        async_mode.check_async_status()
    assert isinstance(exc.value, RuntimeError) and exc.value.needed > 2048
    # the library's STICKY dropped-frame counter (frame state word MOSS_FRAME_STATE_DROPPED_WORD) saw exactly that frame -- which was
    # RAISED to the caller just now, so it does not count as a frame a replay dropped silently; reading resets the word,
    # and then the overflowed frame has left every other counter clean too
    cx = async_mode._C.ASYNC
    assert int(cx.frame_state.view(torch.int32)[async_mode._C.FRAME_STATE_DROPPED_WORD]) == 1
    assert cx.read_dropped_frames(reset=False) == 0 and cx.read_dropped_frames() == 0
    assert int(async_mode._C.ASYNC.frame_state.count_nonzero()) == 0
    assert async_mode._C.ASYNC.capacity > 2048
    got = _train_like_step(pc, cam, pipe, bg, w)               # the grown capacity fits
    async_mode.check_async_status()
    assert torch.equal(got[0], ref[0])
    for a, c in zip(ref[3], got[3]):
        assert torch.equal(a, c)


def test_async_record_pool_overflow_and_the_learned_capacity(gpu, hip_lib):
    """The binning buffer of an asynchronous forward holds a gradient-record pool of 6 cells per instance of CAPACITY (body scenes use
    3.7-5.5 per instance of the frame); a frame of wide Gaussians -- every instance covers its whole tile: 16 cells -- asks for more
    than `2 R` gives.  Such a frame is dropped like one with too many instances (status word [3] = the capacity that holds it), the
    capacity grows from that word, and a context that learns its capacity from a first synchronous call gets it right at once: the
    asynchronous frame then equals the synchronous one bit for bit, gradients included."""
    from moss_amd.diff_gaussian_rasterization import _C
    g = torch.Generator().manual_seed(11)
    P, H, W = 300, 256, 256
    s = scenes.config1()
    cam = s.camera
    # wide, fairly opaque Gaussians in front of config1's camera: boxes of many tiles each
    d0 = hp.inputs_of(s, "scale_rot")
    means = d0.means3D[:1].repeat(P, 1) + 0.15 * torch.randn(P, 3, generator=g)
    scales_ = torch.full((P, 3), 1.5) * (0.5 + torch.rand(P, 3, generator=g))          # (the camera is ~3 away: every one covers the image)
    rot = torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=1)
    opa = torch.full((P, 1), 0.9)
    sh = 0.3 * torch.randn(P, d0.shs.shape[1], 3, generator=g)
    a = dict(bg=d0.bg.to(gpu), means3D=means.to(gpu), opacity=opa.to(gpu), scales=scales_.to(gpu), rotations=rot.to(gpu),
             view=cam.viewmatrix.to(gpu), proj=cam.projmatrix.to(gpu), sh=sh.to(gpu), campos=cam.campos.to(gpu))
    E = torch.empty(0, device=gpu)                             # (no precomputed colours / covariances)

    def forward(cx, debug=0):
        return _C.rasterize_gaussians(a["bg"], a["means3D"], E, a["opacity"], a["scales"], a["rotations"], 1.0, E, a["view"], a["proj"],
                                      cam.tanfovx, cam.tanfovy, cam.H, cam.W, a["sh"], d0.degree, a["campos"], False, debug, None, 0, cx)

    def backward(cx, r, dc):
        z = torch.zeros(1, cam.H, cam.W, device=gpu)
        return _C.rasterize_gaussians_backward(a["bg"], a["means3D"], r[4], E, a["scales"], a["rotations"], 1.0, E, a["view"], a["proj"],
                                               cam.tanfovx, cam.tanfovy, dc, z, z, a["sh"], d0.degree, a["campos"], r[5], r[0], r[6], r[7], r[3], 0,
                                               None, 0, None, cx)
    ref = forward(_C.RasterContext())                          # synchronous
    R = int(ref[0])
    assert R > 1000
    dc = torch.rand(3, cam.H, cam.W, device=gpu)
    gref = backward(_C.RasterContext(), ref, dc)
    # (1) capacity 2 R + 1024 as in rounds 2-4: enough instances, too few record cells -> dropped, reported, grown
    cx = _C.RasterContext(); cx.set_async(True, capacity=2 * R + 1024)
    r1 = forward(cx)
    with pytest.raises(_C.CapacityOverflow) as exc:
        cx.check_status()
    assert exc.value.needed > 2 * R + 1024 and cx.last_needed == R, (exc.value.needed, R)
    assert float(r1[3].abs().max()) == 0.0                     # rendered nothing
    assert cx.capacity >= 2 * exc.value.needed
    r2 = forward(cx); cx.check_status()                        # the grown capacity fits
    for u, v in zip(r2[1:5], ref[1:5]):
        assert torch.equal(u, v)
    # (2) a context that learns from its first, synchronous call
    cx = _C.RasterContext(); cx.set_async(True)
    forward(cx)
    assert cx.capacity > 2 * R + 1024
    r3 = forward(cx); cx.check_status()
    assert cx.last_needed == R
    for u, v in zip(r3[1:5], ref[1:5]):
        assert torch.equal(u, v)
    for u, v in zip(backward(cx, r3, dc), gref):
        assert torch.equal(u, v)


def test_dropped_frame_is_not_an_optimizer_step(gpu, hip_lib, async_mode):
    """A frame that overflows its capacity renders nothing; a step captured in a hipGraph cannot skip its optimizer on the host.  With
    the frame's status word as the guard (FlatAdamW.step(skip_word=...), C ABI moss_adamw_flat_guarded) the update kernel turns itself
    into a no-op ON THE DEVICE: parameters, both moments and the step counter stay bit for bit across the dropped frame -- under graph
    replay -- while a frame that fits steps as usual."""
    from types import SimpleNamespace
    from moss_amd.dist import GradBucket
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import render, camera_view
    from moss_amd.optim import FlatAdamW
    from moss_amd.diff_gaussian_rasterization import _C
    s = scenes.config2()
    pc = GaussianSet(s, device=gpu)
    cam = camera_view(s.camera, gpu)
    cx = _C.RasterContext()
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raster_context=cx)
    bg = torch.zeros(3, device=gpu)
    w = torch.rand(3, s.camera.H, s.camera.W, device=gpu)
    params = list(pc.parameters())
    bucket = GradBucket(params)
    opt = FlatAdamW([{"params": params, "lr": 1e-3}], bucket, capturable=True)

    def compute():
        bucket.attach()
        out = render(cam, pc, pipe, bg)
        ((out["render"] * w).sum() + out["render_alpha"].sum()).backward()
        opt.step(skip_word=_C.frame_status_word(cx.last_img_buffer))
        return out["render"].detach()

    def state():
        return [opt.flat_params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_state.clone()]

    for capacity, dropped in ((2048, True), (4_000_000, False)):          # far below / above what config2 needs
        cx.set_async(True, capacity=capacity)
        side = torch.cuda.Stream(gpu)
        side.wait_stream(torch.cuda.current_stream(gpu))
        with torch.cuda.stream(side):
            compute()
        torch.cuda.current_stream(gpu).wait_stream(side)
        torch.cuda.synchronize(gpu)
        cx.pending = None                                                  # (the eager frame's status: not what this test is about)
        graph = torch.cuda.CUDAGraph()
        with capturing(graph, stream=side):
            img = compute()
        before = state()
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize(gpu)
        after = state()
        if dropped:
            assert torch.equal(img, torch.zeros_like(img))
            for a, b in zip(before, after):
                assert torch.equal(a, b)
            assert cx.read_dropped_frames() >= 3
        else:
            assert float(img.abs().max()) > 0
            assert int(after[3][0]) == int(before[3][0]) + 3
            assert not torch.equal(before[0], after[0]) and not torch.equal(before[1], after[1])
            assert cx.read_dropped_frames() == 0
    # a retired frame-state block that serves again is not counted twice
    cx2 = _C.RasterContext()
    a = cx2._frame_state(gpu, 64, 64); b = cx2._frame_state(gpu, 512, 512); c = cx2._frame_state(gpu, 64, 64)
    assert c is b and len(cx2._retired_frame_states) == 1 and cx2._retired_frame_states[0] is a
    b.view(torch.int32)[_C.FRAME_STATE_DROPPED_WORD] = 2
    assert cx2.read_dropped_frames(reset=False) == 2 and cx2.read_dropped_frames() == 2 and cx2.read_dropped_frames() == 0


@pytest.mark.parametrize("mode", ["scale_rot", "lbs", "scale_rot_spatial_hint"])
def test_backward_kernel_takes_the_adamw_step(gpu, hip_lib, async_mode, mode):
    """FlatAdamW.fuse_into_backward (C ABI moss_raster_backward_raw_adamw): the per-Gaussian backward kernel applies the AdamW update of
    the parameters it has just differentiated.  Against the two-kernel form (backward -> gradients in the bucket -> flat AdamW) on
    identical models: parameters, both moments and the step count agree BIT FOR BIT after every step; a frame that overflows its
    capacity takes no step; inputs that are not the parameters themselves are refused."""
    from types import SimpleNamespace
    from moss_amd.dist import GradBucket
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import render, camera_view
    from moss_amd.optim import FlatAdamW
    from moss_amd.diff_gaussian_rasterization import _C
    s = scenes.config2()
    cam = camera_view(s.camera, gpu)
    bg = torch.zeros(3, device=gpu)
    gen = torch.Generator(device="cpu").manual_seed(5)
    w = torch.rand(3, s.camera.H, s.camera.W, generator=gen).to(gpu)
    T = None
    if mode == "lbs":                                        # a per-Gaussian transform close to the identity + a translation
        T = (torch.eye(3)[None] + 0.05 * torch.randn(s.P, 3, 3, generator=gen)).to(gpu)
        tl = (0.01 * torch.randn(s.P, 3, generator=gen)).to(gpu)

    def make(fused):
        pc = GaussianSet(s, sh_degree=3, device=gpu, unified_features=True)
        # (MOSS_HINT_SPATIAL_ORDER: a block's rows are then groups of 16 Gaussians from four places of the index range)
        pc.spatially_ordered = mode == "scale_rot_spatial_hint"
        cx = _C.RasterContext()
        cx.set_async(True, capacity=4_000_000)
        pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raster_context=cx,
                               raw_parameters_in_op=True, transforms_in_op=T is not None, pose_in_op=T is not None)
        bucket = GradBucket(list(pc.parameters()))
        opt = FlatAdamW(pc.param_groups(), bucket, eps=1e-15, weight_decay=0.01, capturable=True)
        if fused:
            opt.fuse_into_backward(cx, means3D=pc._xyz, sh=pc._features, opacity=pc._opacity, scales=pc._scaling, rotations=pc._rotation)

        def step():
            if not fused:
                bucket.attach()
            out = render(cam, pc, pipe, bg, **({} if T is None else {"transforms": T, "translation": tl}))
            ((out["render"] * w).sum() + out["render_alpha"].sum()).backward()
            if fused:
                assert all(p.grad is None for p in pc.parameters())         # the gradients never left the kernel
            opt.step(skip_word=None if fused else _C.frame_status_word(cx.last_img_buffer))
            return out["render"].detach()
        return SimpleNamespace(pc=pc, cx=cx, opt=opt, step=step, pipe=pipe)

    a, b = make(False), make(True)
    for it in range(3):
        ia, ib = a.step(), b.step()
        torch.cuda.synchronize(gpu)
        assert torch.equal(ia, ib) and float(ia.abs().max()) > 0
        for name in ("flat_params", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(a.opt, name), getattr(b.opt, name)), f"{name} differs after step {it + 1}"
        assert a.opt.step_count() == b.opt.step_count() == it + 1
    # a dropped frame takes no step
    b.cx.pending = None
    b.cx.set_async(True, capacity=2048)
    before = [b.opt.flat_params.clone(), b.opt.exp_avg.clone(), b.opt.exp_avg_sq.clone(), b.opt.step_state.clone()]
    img = b.step()
    torch.cuda.synchronize(gpu)
    assert torch.equal(img, torch.zeros_like(img))
    for x, y in zip(before, [b.opt.flat_params, b.opt.exp_avg, b.opt.exp_avg_sq, b.opt.step_state]):
        assert torch.equal(x, y)
    b.cx.pending = None
    b.cx.set_async(True, capacity=4_000_000)
    # activated copies are not the parameters: refused, nothing updated
    b.pipe.raw_parameters_in_op = False
    with pytest.raises(RuntimeError, match="raw parameters|not the parameter"):
        b.step()
    b.pipe.raw_parameters_in_op = True
    assert b.opt.step_count() == 3


def test_adamw_drop_in_matches_torch_optim_adamw(gpu, hip_lib):
    """moss_amd.optim.AdamW -- what patches/gaussian_model.diff puts in place of ``torch.optim.AdamW(l, lr=0.0, eps=1e-15)``
    (scene/gaussian_model.py:226) -- against torch's own optimizer: MOSS's group structure (one tensor per group, a name, a per-group
    lr rewritten between steps), five steps, then the densification surgery MOSS performs on the state (prune by mask, as
    ``_prune_optimizer`` does, scene/gaussian_model.py:377-392) and three more steps.  Parameters and moments agree to 2e-6 of their
    largest value (the kernel's square root and reciprocal are the hardware's, ~1 ulp)."""
    from moss_amd.optim import AdamW
    gen = torch.Generator().manual_seed(3)
    shapes = {"xyz": (1237, 3), "f_dc": (1237, 1, 3), "f_rest": (1237, 15, 3), "opacity": (1237, 1), "scaling": (1237, 3), "rotation": (1237, 4)}
    lrs = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3}
    init = {k: torch.randn(s, generator=gen) for k, s in shapes.items()}

    net_init = [torch.randn(s_, generator=gen) for s_ in [(64, 32), (64,), (32, 64), (32,), (16, 32), (16,), (3, 16)]]

    def make(cls):
        groups = [{"params": [torch.nn.Parameter(init[k].clone().to(gpu))], "lr": lrs[k], "name": k} for k in shapes]
        # MOSS's network groups (scene/gaussian_model.py:222-223): MANY small tensors in one group
        groups.append({"params": [torch.nn.Parameter(t.clone().to(gpu)) for t in net_init], "lr": 1e-4, "name": "auto_regression"})
        return cls(groups, lr=0.0, eps=1e-15)

    def close(a, b):
        return float((a - b).abs().max()) <= 2e-6 * max(float(b.abs().max()), 1e-30)

    ours, ref = make(AdamW), make(torch.optim.AdamW)
    for it in range(8):
        if it == 5:                                          # MOSS's _prune_optimizer, on both
            mask = (torch.rand(1237, generator=gen) > 0.3).to(gpu)
            for opt in (ours, ref):
                for group in opt.param_groups:
                    if group["name"] == "auto_regression":
                        continue
                    st = opt.state.get(group["params"][0], None)
                    st["exp_avg"] = st["exp_avg"][mask]; st["exp_avg_sq"] = st["exp_avg_sq"][mask]
                    del opt.state[group["params"][0]]
                    group["params"][0] = torch.nn.Parameter(group["params"][0][mask].requires_grad_(True))
                    opt.state[group["params"][0]] = st
        for go, gr in zip(ours.param_groups, ref.param_groups):
            if go["name"] == "xyz":
                go["lr"] = gr["lr"] = lrs["xyz"] * (0.9 ** it)  # update_learning_rate (scene/gaussian_model.py:263-268)
            for po, pr in zip(go["params"], gr["params"]):
                g = torch.randn(po.shape, generator=gen).to(gpu) * (0.0 if (it == 2 and go["name"] == "opacity") else 1.0)
                po.grad = g.clone(); pr.grad = g.clone()
        ours.step(); ref.step()
        for go, gr in zip(ours.param_groups, ref.param_groups):
            for po, pr in zip(go["params"], gr["params"]):
                assert close(po.data, pr.data), (it, go["name"])
                assert close(ours.state[po]["exp_avg"], ref.state[pr]["exp_avg"]) and close(ours.state[po]["exp_avg_sq"], ref.state[pr]["exp_avg_sq"])
    # a parameter the kernel cannot take (float64) goes through torch's expressions
    p64 = torch.nn.Parameter(torch.randn(17, dtype=torch.float64, device=gpu))
    r64 = torch.nn.Parameter(p64.detach().clone())
    oa, ob = AdamW([p64], lr=1e-2), torch.optim.AdamW([r64], lr=1e-2)
    for _ in range(3):
        g = torch.randn(17, dtype=torch.float64, device=gpu)
        p64.grad = g.clone(); r64.grad = g.clone()
        oa.step(); ob.step()
    assert float((p64 - r64).abs().max()) < 1e-12


def test_adamw_multi_is_bit_identical_to_one_flat_ex_call_per_tensor(gpu, hip_lib):
    """C ABI moss_adamw_multi (several tensors with buffers and step counts of their own, one launch) against moss_adamw_flat_ex (one
    segment, host-side step) called once per tensor: the same bits in every parameter and moment -- ragged sizes (not multiples of 4, one element, empty), different learning
    rates and DIFFERENT step counts (MOSS's surgery keeps the step per tensor), two steps."""
    import ctypes as C
    from moss_amd import _lib
    L = _lib.lib()
    gen = torch.Generator().manual_seed(17)
    sizes = [3711, 1237 * 45, 1, 1237 * 4, 0, 1237 * 3 + 2, 262147]
    lrs = [1.6e-4, 1.25e-4, 0.05, 1e-3, 0.3, 5e-3, 2.5e-3]
    steps0 = [1, 7, 1, 300, 1, 2, 41]
    def fresh():
        g = torch.Generator().manual_seed(99)
        return [[torch.randn(max(n, 0), generator=g).to(gpu) for n in sizes] for _ in range(2)] + \
               [[(torch.rand(max(n, 0), generator=g) * 1e-3).to(gpu) for n in sizes]]
    (pa, ma, va), (pb, mb, vb) = fresh(), fresh()
    stream = torch.cuda.current_stream(gpu).cuda_stream
    for it in range(2):
        grads = [torch.randn(max(n, 0), generator=gen).to(gpu) for n in sizes]
        a = _lib.AdamWMultiArgs()
        a.num_tensors = len(sizes)
        a.beta1, a.beta2, a.eps, a.weight_decay = 0.9, 0.999, 1e-15, 0.01
        for k, n in enumerate(sizes):
            a.numel[k], a.lr[k], a.step[k] = n, lrs[k], steps0[k] + it
            a.params[k], a.grads[k], a.exp_avg[k], a.exp_avg_sq[k] = pa[k].data_ptr(), grads[k].data_ptr(), ma[k].data_ptr(), va[k].data_ptr()
        assert L.moss_adamw_multi(C.addressof(a), stream) == 0
        for k, n in enumerate(sizes):
            if n == 0:
                continue
            one, lr = (C.c_longlong * 1)(n), (C.c_float * 1)(lrs[k])
            f = _lib.AdamWFlatArgs()
            f.first, f.count, f.num_segments, f.segment_end, f.segment_lr = 0, n, 1, C.addressof(one), C.addressof(lr)
            f.params, f.grads, f.exp_avg, f.exp_avg_sq = pb[k].data_ptr(), grads[k].data_ptr(), mb[k].data_ptr(), vb[k].data_ptr()
            f.beta1, f.beta2, f.eps, f.weight_decay, f.step = 0.9, 0.999, 1e-15, 0.01, steps0[k] + it
            assert L.moss_adamw_flat_ex(C.addressof(f), stream) == 0
        torch.cuda.synchronize(gpu)
        for k in range(len(sizes)):
            assert torch.equal(pa[k], pb[k]) and torch.equal(ma[k], mb[k]) and torch.equal(va[k], vb[k]), (it, k)
    # refused: nine tensors, a misaligned pointer, a step count of zero
    a.num_tensors = 9
    assert L.moss_adamw_multi(C.addressof(a), stream) != 0
    a.num_tensors = 1; a.numel[0] = 8; a.params[0] = pa[1].data_ptr() + 4
    assert L.moss_adamw_multi(C.addressof(a), stream) != 0
    a.params[0] = pa[1].data_ptr(); a.step[0] = 0
    assert L.moss_adamw_multi(C.addressof(a), stream) != 0


def test_partial_fusion_position_in_an_optimizer_of_its_own(gpu, hip_lib, async_mode):
    """The configuration INTEGRATION.md recommends for MOSS: features, opacity, scaling and rotation take their AdamW step inside the
    backward kernel; the POSITION -- whose gradient MOSS also feeds from its LBS network -- keeps its gradient (written by the op) and
    an optimizer of its own.  Against one flat AdamW over all five tensors: bit-identical parameters and moments after every step."""
    from types import SimpleNamespace
    from moss_amd.dist import GradBucket
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import render, camera_view
    from moss_amd.optim import FlatAdamW
    from moss_amd.diff_gaussian_rasterization import _C
    s = scenes.config2()
    cam = camera_view(s.camera, gpu)
    bg = torch.zeros(3, device=gpu)
    w = torch.rand(3, s.camera.H, s.camera.W, generator=torch.Generator().manual_seed(3)).to(gpu)

    def model():
        pc = GaussianSet(s, sh_degree=3, device=gpu, unified_features=True)
        cx = _C.RasterContext()
        cx.set_async(True, capacity=4_000_000)
        pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raster_context=cx, raw_parameters_in_op=True)
        return pc, cx, pipe

    def loss_of(out):
        return (out["render"] * w).sum() + out["render_alpha"].sum()

    # reference: one flat optimizer over everything
    pa, cxa, pipea = model()
    ba = GradBucket(list(pa.parameters()))
    oa = FlatAdamW(pa.param_groups(), ba, eps=1e-15, capturable=True)
    # partial fusion: [features, opacity, scaling, rotation] fused; xyz in a second optimizer over its own bucket
    pb, cxb, pipeb = model()
    groups = pb.param_groups()
    g_xyz = [g for g in groups if g["name"] == "xyz"]
    g_rest = [g for g in groups if g["name"] != "xyz"]
    b_rest = GradBucket([p for g in g_rest for p in g["params"]])
    b_xyz = GradBucket([pb._xyz])
    o_rest = FlatAdamW(g_rest, b_rest, eps=1e-15, capturable=True)
    o_xyz = FlatAdamW(g_xyz, b_xyz, eps=1e-15, capturable=True)
    o_rest.fuse_into_backward(cxb, sh=pb._features, opacity=pb._opacity, scales=pb._scaling, rotations=pb._rotation)
    for it in range(3):
        ba.attach()
        loss_of(render(cam, pa, pipea, bg)).backward()
        oa.step()
        b_xyz.attach()
        loss_of(render(cam, pb, pipeb, bg)).backward()
        assert pb._features.grad is None and pb._xyz.grad is not None       # only the position's gradient left the kernel
        o_xyz.step()
        o_rest.step()                                                       # (a no-op: the backward took it)
        torch.cuda.synchronize(gpu)
        for name in ("_xyz", "_features", "_opacity", "_scaling", "_rotation"):
            assert torch.equal(getattr(pa, name).data, getattr(pb, name).data), f"{name} differs after step {it + 1}"
    assert oa.step_count() == o_rest.step_count() == o_xyz.step_count() == 3


def test_identical_trainings_end_bit_identical_on_the_bench_frame(gpu, hip_lib, async_mode):
    """150 training steps on the bench frame (config3: 100k Gaussians, depth segments active), twice with the flat AdamW kernel and once
    with the step inside the backward kernel, each queued without host synchronisation: parameters and moments must be equal bit for
    bit.  (Round 3's forward made the cut after a list's k x 64-th hit depend on whether the scanner's "list complete" flag had arrived
    yet: the same frame was now and then partitioned differently -- a handful of last-bit differences every ~20 steps, found in round 4
    by exactly this comparison.  The single-frame reproducibility test never saw it.)"""
    from types import SimpleNamespace
    from moss_amd.dist import GradBucket
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import render, camera_view
    from moss_amd.loss import training_loss_fused, backward_from_loss
    from moss_amd.optim import FlatAdamW
    from moss_amd.diff_gaussian_rasterization import _C
    s = scenes.config3()
    cam = camera_view(s.camera, gpu)
    bg = torch.zeros(3, device=gpu)
    with torch.no_grad():
        o = render(cam, GaussianSet(scenes.config3(seed=scenes.SEED + 7), sh_degree=3, device=gpu),
                   SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False), bg)
    gt = o["render"].detach().clamp(0, 1).contiguous()
    gt_mask = (o["render_alpha"].detach() > 0.5).float().contiguous()

    def run(fused, steps=150):
        pc = GaussianSet(s, sh_degree=3, device=gpu, unified_features=True)
        bucket = GradBucket(list(pc.parameters()))
        cx = _C.RasterContext()
        cx.set_async(True, capacity=480_000)                  # (2 x the frame's instances: what the capacity policy would pick)
        pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raw_parameters_in_op=True,
                               grad_bucket=bucket, raster_context=cx)
        opt = FlatAdamW(pc.param_groups(), bucket, eps=1e-15, capturable=True)
        if fused:
            opt.fuse_into_backward(cx, means3D=pc._xyz, sh=pc._features, opacity=pc._opacity, scales=pc._scaling, rotations=pc._rotation)
        else:
            cx.set_grad_sink(sh=lambda: bucket.sink_for(pc._features), means3D=lambda: bucket.sink_for(pc._xyz),
                             opacity=lambda: bucket.sink_for(pc._opacity), scales=lambda: bucket.sink_for(pc._scaling),
                             rotations=lambda: bucket.sink_for(pc._rotation))
        for _ in range(steps):
            bucket.detach_grads()
            out = render(cam, pc, pipe, bg)
            backward_from_loss(training_loss_fused(out["render"], out["render_alpha"], gt, gt_mask, terms_out=bucket.loss_terms))
            if not fused:
                bucket.collect()
                opt.step(skip_word=_C.frame_status_word(cx.last_img_buffer))
        torch.cuda.synchronize(gpu)
        cx.check_status()
        assert cx.read_dropped_frames() == 0
        return opt.flat_params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_count()

    a, b, c = run(False), run(False), run(True)
    assert a[3] == b[3] == c[3] == 150
    for x, y, z, name in zip(a[:3], b[:3], c[:3], ("parameters", "exp_avg", "exp_avg_sq")):
        assert torch.equal(x, y), f"{name}: two identical trainings differ"
        assert torch.equal(x, z), f"{name}: the step inside the backward kernel differs from the flat kernel"


def test_learning_rate_schedule_without_recapture(gpu, hip_lib, async_mode):
    """MOSS changes the position learning rate every iteration (scene/gaussian_model.py:263-268).  FlatAdamW.set_learning_rates puts the
    rates into the optimizer's device-side state block, where the update kernels read them: a captured step follows the schedule
    without being captured again -- the fused form (the rasterizer backward takes the step) and the flat kernel alike, and both
    equal eager steps that were given the rates as launch arguments."""
    from types import SimpleNamespace
    from moss_amd.dist import GradBucket
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import render, camera_view
    from moss_amd.optim import FlatAdamW
    from moss_amd.diff_gaussian_rasterization import _C
    s = scenes.config2()
    cam = camera_view(s.camera, gpu)
    bg = torch.zeros(3, device=gpu)
    w = torch.rand(3, s.camera.H, s.camera.W, generator=torch.Generator().manual_seed(9)).to(gpu)
    schedule = [1.6e-4, 1.1e-4, 7e-5, 3e-5]                   # the position rate, step by step; the SH pair changes too

    def make(fused, device_table):
        pc = GaussianSet(s, sh_degree=3, device=gpu, unified_features=True)
        cx = _C.RasterContext()
        cx.set_async(True, capacity=4_000_000)
        pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raster_context=cx, raw_parameters_in_op=True)
        bucket = GradBucket(list(pc.parameters()))
        opt = FlatAdamW(pc.param_groups(), bucket, eps=1e-15, capturable=device_table)
        if fused:
            opt.fuse_into_backward(cx, means3D=pc._xyz, sh=pc._features, opacity=pc._opacity, scales=pc._scaling, rotations=pc._rotation)

        def step():
            if not fused:
                bucket.attach()
            out = render(cam, pc, pipe, bg)
            ((out["render"] * w).sum() + out["render_alpha"].sum()).backward()
            opt.step()
            return out["render"].detach()
        return SimpleNamespace(pc=pc, opt=opt, step=step)

    def rates(m, k):
        return {m.pc._xyz: schedule[k], m.pc._features: (0.0025 * (1 + k), 0.0025 / 20.0 * (1 + k))}

    # reference: eager steps of the flat kernel with the rates as LAUNCH ARGUMENTS (the host tables, no device table)
    ref = make(False, True)
    index = {id(p): i for i, p in enumerate(ref.opt.bucket.params)}
    for k in range(len(schedule)):
        for prm, val in rates(ref, k).items():
            i = index[id(prm)]
            ref.opt.seg_lr[i] = val[0] if isinstance(val, tuple) else val
            if isinstance(val, tuple):
                ref.opt.seg_lr2[i] = val[1]
        ref.step()
    assert int(ref.opt.step_state[12]) == 0
    torch.cuda.synchronize(gpu)
    for fused in (False, True):
        m = make(fused, True)
        m.opt.set_learning_rates(rates(m, 0))
        side = torch.cuda.Stream(gpu)
        side.wait_stream(torch.cuda.current_stream(gpu))
        with torch.cuda.stream(side):
            snap = m.opt.snapshot()
            m.step()                                           # warm-up (allocator), then rewind
            m.opt.restore(snap)
        torch.cuda.current_stream(gpu).wait_stream(side)
        torch.cuda.synchronize(gpu)
        graph = torch.cuda.CUDAGraph()
        with capturing(graph, stream=side):
            m.step()
        m.opt.restore(snap)                                    # the capture itself ran nothing, but keep the state explicit
        torch.cuda.synchronize(gpu)
        for k in range(len(schedule)):
            m.opt.set_learning_rates(rates(m, k))              # between replays: a 80-byte copy, no re-capture
            graph.replay()
        torch.cuda.synchronize(gpu)
        assert m.opt.step_count() == len(schedule)
        for name in ("flat_params", "exp_avg", "exp_avg_sq"):
            a, b = getattr(ref.opt, name), getattr(m.opt, name)
            assert torch.equal(a, b), f"{name} (fused={fused}): max difference {float((a - b).abs().max())}"


def test_step_captured_in_hipgraph_replays_with_new_parameters(gpu, hip_lib, async_mode):
    """With the asynchronous forward nothing in render+backward talks to the host, so the step is capturable in a hipGraph.
    Replays must track the CURRENT parameter values (not the captured ones) and agree bit-for-bit with eager launches."""
    from types import SimpleNamespace
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import render, camera_view
    s = scenes.config2()
    pc = GaussianSet(s, device=gpu)
    cam = camera_view(s.camera, gpu)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    bg = torch.zeros(3, device=gpu)
    w = torch.rand(3, s.camera.H, s.camera.W, device=gpu)
    params = list(pc.parameters())
    grads = [torch.zeros_like(p) for p in params]

    def compute():
        for p, g in zip(params, grads):
            g.zero_(); p.grad = g
        out = render(cam, pc, pipe, bg)
        ((out["render"] * w).sum() + out["render_alpha"].sum()).backward()
        return out["render"].detach()          # no grad_fn kept: the autograd graph (and its AccumulateGrad nodes) dies here

    async_mode.set_async(True)
    compute()                                                  # synchronous: learns the capacity
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        compute()
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    with capturing(graph, stream=side):
        g_img = compute()
    for trial in range(2):
        with torch.no_grad():
            pc._xyz.add_(0.01 * (trial + 1))
            pc._opacity.mul_(0.9)
        graph.replay()
        torch.cuda.synchronize(gpu)
        img_g = g_img.clone(); grads_g = [g.clone() for g in grads]
        img_e = compute().clone()
        torch.cuda.synchronize(gpu)
        assert torch.equal(img_g, img_e)
        for a, b in zip(grads_g, grads):
            assert torch.equal(a, b)
    async_mode.check_async_status()


def test_flat_adamw_device_step_counter(gpu, hip_lib):
    """moss_adamw_flat_devstep keeps the step count (bias correction) on the device: five steps equal torch.optim.AdamW."""
    from moss_amd.dist import GradBucket
    from moss_amd.optim import FlatAdamW
    torch.manual_seed(1)
    shapes, lrs = [(513, 3), (513, 4)], [0.01, 0.002]
    init = [torch.randn(*s) for s in shapes]
    pa = [torch.nn.Parameter(t.clone().to(gpu)) for t in init]
    pb = [torch.nn.Parameter(t.clone().to(gpu)) for t in init]
    ref = torch.optim.AdamW([{"params": [p], "lr": lr} for p, lr in zip(pb, lrs)], lr=0.0, eps=1e-15)
    bucket = GradBucket(pa)
    opt = FlatAdamW([{"params": [p], "lr": lr} for p, lr in zip(pa, lrs)], bucket, eps=1e-15, capturable=True)
    for it in range(5):
        bucket.attach()
        for p, q, s_ in zip(pa, pb, shapes):
            g = torch.randn(*s_, device=gpu)
            p.grad.copy_(g); q.grad = g.clone()
        opt.step(); ref.step()
    assert int(opt.step_state[0]) == 5
    for p, q in zip(pa, pb):
        assert hp.rel_err(p.detach().cpu().numpy(), q.detach().cpu().numpy()) < 1e-6


def test_sharded_flat_adamw_equals_the_full_update(gpu, hip_lib):
    """moss_adamw_flat_range (FlatAdamW(shard=(r, w))): the w shards of the update, each with the moments of its own elements only,
    give bit for bit the parameters of the full update -- learning-rate segments, the periodic SH pattern and shard boundaries that
    fall inside a segment included; device-side and host-side step counters."""
    from moss_amd.dist import GradBucket
    from moss_amd.optim import FlatAdamW
    torch.manual_seed(3)
    shapes = [(301, 3), (301, 16, 3), (301, 1), (301, 4)]
    world = 4

    def groups(ps):
        return [{"params": [ps[0]], "lr": 0.01}, {"params": [ps[1]], "lr": 0.0025, "lr_pattern": (48, 3, 0.0025 / 20)},
                {"params": [ps[2]], "lr": 0.05}, {"params": [ps[3]], "lr": 0.001}]
    init = [torch.randn(*s) for s in shapes]
    for capturable in (False, True):
        pf = [torch.nn.Parameter(t.clone().to(gpu)) for t in init]
        bf = GradBucket(pf)
        full = FlatAdamW(groups(pf), bf, eps=1e-15, capturable=capturable)
        shards = []
        for r in range(world):
            ps = [torch.nn.Parameter(t.clone().to(gpu)) for t in init]
            b = GradBucket(ps, world=world)
            shards.append((b, FlatAdamW(groups(ps), b, eps=1e-15, capturable=capturable, shard=(r, world))))
        n = bf.n_params
        assert sum(o.count for _, o in shards) == n and all(o.exp_avg.numel() == max(o.count, 1) for _, o in shards)
        for it in range(4):
            g = torch.randn(n, device=gpu)
            bf.flat[:n] = g
            full.step()
            for r, (b, o) in enumerate(shards):
                per = b.shard_len
                o.grad_shard.zero_()
                o.grad_shard[:o.count] = g[o.first:o.first + o.count]          # what the reduce-scatter would have left here
                o.step()
            # "all-gather": every rank's shard of the parameters
            got = torch.cat([o.flat_params[o.first:o.first + o.count] for _, o in shards])
            assert torch.equal(got, full.flat_params[:n]), (capturable, it)
            for b, o in shards:                                               # ... copied into every replica for the next step
                o.flat_params[:n] = got


def test_spatial_order_hint_changes_no_result(gpu, hip_lib):
    """GaussianSet.reorder_spatially(): the rendered image is the same image, the gradients are the same gradients in the new order,
    and the MOSS_HINT_SPATIAL_ORDER bit render() then passes (per-Gaussian backward: rows dealt in groups of 16) changes nothing but the
    order of some float32 sums."""
    from types import SimpleNamespace
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import render, camera_view
    s = scenes.config1(P=3000, W=160, H=96)
    cam = camera_view(s.camera, gpu)
    bg = torch.zeros(3, device=gpu)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raw_parameters_in_op=True)
    w = torch.rand(3, 96, 160, generator=torch.Generator().manual_seed(5)).to(gpu)

    def grads(pc):
        for p in pc.parameters():
            p.grad = None
        out = render(cam, pc, pipe, bg)
        ((out["render"] * w).sum() + 0.3 * out["render_alpha"].sum()).backward()
        return out["render"].detach().clone(), {n: p.grad.detach().clone() for n, p in pc.named_parameters()}

    pc = GaussianSet(s, sh_degree=3, device=gpu, unified_features=True)
    img0, g0 = grads(pc)
    perm = pc.reorder_spatially()
    assert pc.spatially_ordered and sorted(perm.tolist()) == list(range(3000))
    img1, g1 = grads(pc)                                      # hinted
    pc.spatially_ordered = False
    img2, g2 = grads(pc)                                      # same order, no hint
    # (not bit for bit: the wave-balanced gather adds a Gaussian's records in an order that depends on its wave-mates, and the hint
    # changes who they are)
    assert torch.equal(img1, img2)
    for n in g1:
        assert hp.rel_err(g1[n].cpu().numpy(), g2[n].cpu().numpy()) < 2e-6, n
    assert float((img1 - img0).abs().max()) <= 2e-6           # (depth ties are broken by the index: none in this scene; sums re-ordered)
    for n in g0:
        assert hp.rel_err(g1[n].cpu().numpy(), g0[n][perm].cpu().numpy()) < 2e-5, n


def test_flat_adamw_rows_can_be_reindexed(gpu, hip_lib):
    """densify.spatial_order + FlatAdamW.permute_rows: training on the re-indexed set is the same training (the parameters and both
    moments move together), checked against an optimizer that never saw the permutation."""
    from moss_amd.dist import GradBucket
    from moss_amd.optim import FlatAdamW
    from moss_amd.densify import spatial_order
    torch.manual_seed(2)
    P = 777
    shapes, lrs = [(P, 3), (P, 15, 3), (P, 4)], [0.01, 0.002, 0.003]
    init = [torch.randn(*s) for s in shapes]
    pa = [torch.nn.Parameter(t.clone().to(gpu)) for t in init]
    pb = [torch.nn.Parameter(t.clone().to(gpu)) for t in init]
    ba, bb = GradBucket(pa), GradBucket(pb)
    oa = FlatAdamW([{"params": [p], "lr": lr} for p, lr in zip(pa, lrs)], ba, eps=1e-15)
    ob = FlatAdamW([{"params": [p], "lr": lr} for p, lr in zip(pb, lrs)], bb, eps=1e-15)
    perm = None
    for it in range(4):
        if it == 2:
            perm = spatial_order(pa[0].detach())
            assert sorted(perm.tolist()) == list(range(P))
            oa.permute_rows(perm)
        ba.attach(); bb.attach()
        for p, q, s_ in zip(pa, pb, shapes):
            g = torch.randn(*s_, device=gpu)
            q.grad.copy_(g)
            p.grad.copy_(g if perm is None else g[perm])
        oa.step(); ob.step()
    for p, q in zip(pa, pb):
        assert torch.equal(p.detach(), q.detach()[perm])
    # the curve keeps index neighbours close: mean distance between consecutive Gaussians well under that of a random order
    step_len = lambda x: float((x[1:] - x[:-1]).norm(dim=1).mean())
    assert step_len(pa[0].detach()) < 0.5 * step_len(pb[0].detach())


# ---------------------------------------------------------------- fused parameter activations
def _raw_params(P, K, gpu, seed=0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.nn.Parameter(torch.randn(*s, generator=g).to(gpu))
    return dict(xyz=mk(P, 3), dc=mk(P, 1, 3), rest=mk(P, K - 1, 3), opa=mk(P, 1), scl=mk(P, 3), rot=mk(P, 4))


@pytest.mark.parametrize("P,K", [(1, 16), (5, 16), (1000, 16), (6890, 4), (4097, 1)])
def test_fused_activations_match_torch_getters(gpu, hip_lib, P, K):
    """moss_gaussian_activate_forward/backward vs the torch ops of scene/gaussian_model.py:46-53,134-166 (exp, sigmoid,
    F.normalize, cat): values to 1e-6 relative, gradients to 1e-5."""
    from moss_amd.activations import activate_gaussians
    a = _raw_params(P, K, gpu)
    b = {k: torch.nn.Parameter(v.detach().clone()) for k, v in a.items()}
    outs = activate_gaussians(a["xyz"], a["dc"], a["rest"], a["opa"], a["scl"], a["rot"])
    refs = (b["xyz"] * 1.0, torch.cat((b["dc"], b["rest"]), dim=1), torch.sigmoid(b["opa"]), torch.exp(b["scl"]),
            torch.nn.functional.normalize(b["rot"]))
    g = torch.Generator().manual_seed(9)
    ws = [torch.randn(*o.shape, generator=g).to(gpu) for o in outs]
    for o, r in zip(outs, refs):
        assert o.shape == r.shape
        assert hp.rel_err(o.detach().cpu().numpy(), r.detach().cpu().numpy()) < 1e-6
    sum((o * w).sum() for o, w in zip(outs, ws)).backward()
    sum((r * w).sum() for r, w in zip(refs, ws)).backward()
    for k in a:
        if a[k].numel():
            assert hp.rel_err(a[k].grad.cpu().numpy(), b[k].grad.cpu().numpy()) < 1e-5, k


def _ulp32(x):
    """The float32 unit in the last place at the magnitude of the float64 values ``x``: 2^(floor(log2 |x|) - 23)."""
    return np.ldexp(1.0, np.frexp(np.abs(x))[1] - 24)


@pytest.mark.parametrize("P,K", [(150001, 16), (1000001, 1)])
def test_fused_activations_match_torch_getters_in_the_second_grid_turn(gpu, hip_lib, P, K):
    """activations.hip caps its grid at 8192 x 256 threads and walks the remaining float4 cells with a grid stride: at these sizes the
    loop body runs twice.  (150001, 16): 2 212 516 cells, the turn falls in the quaternion section; (1000001, 1): 3 500 005 cells, it
    falls inside the scaling section and all of the rotation section runs in the second turn.  Every ELEMENT against the float64 torch
    getters and float64 autograd on the same float32 inputs (randn), not against a max-normalised error:
      xyz, features and their gradients   bit-exact
      sigmoid, exp, normalize             within 4 float32 ulps of the float64 value
      d opacity                           8 * 2^-24 * |g|                (absolute: 1 - s cancels)
      d scaling                           4 ulps
      d rotation                          8 * 2^-24 * |g|_2 / |q|        (absolute: g - y (y.g) cancels)
    with g the incoming gradient: one expf, sqrtf or reciprocal at <= 1-2 ulp each plus the two to four roundings around it.
    The bounds are derived, not measured.  Measured on an MI355X, worst error / bound over all elements (the test prints them):
      (150001, 16)   sigmoid 0.536  exp 0.204  normalize 0.651  d_scaling 0.413  d_opacity 0.162  d_rotation 0.613
      (1000001, 1)   sigmoid 0.536  exp 0.211  normalize 0.706  d_scaling 0.434  d_opacity 0.164  d_rotation 0.665"""
    from moss_amd.activations import activate_gaussians
    a = _raw_params(P, K, gpu)
    outs = activate_gaussians(a["xyz"], a["dc"], a["rest"], a["opa"], a["scl"], a["rot"])
    g = torch.Generator().manual_seed(9)
    ws = [torch.randn(*o.shape, generator=g) for o in outs]
    sum((o * w.to(gpu)).sum() for o, w in zip(outs, ws)).backward()
    b = {k: v.detach().cpu().double().requires_grad_(True) for k, v in a.items()}
    refs = (b["xyz"] * 1.0, torch.cat((b["dc"], b["rest"]), dim=1), torch.sigmoid(b["opa"]), torch.exp(b["scl"]),
            torch.nn.functional.normalize(b["rot"]))
    sum((r * w.double()).sum() for r, w in zip(refs, ws)).backward()
    got = [o.detach().cpu() for o in outs]
    # copies: bit-exact
    assert torch.equal(got[0], a["xyz"].detach().cpu()) and torch.equal(got[1], torch.cat((a["dc"], a["rest"]), dim=1).detach().cpu())
    assert torch.equal(a["xyz"].grad.cpu(), ws[0]) and torch.equal(a["dc"].grad.cpu(), ws[1][:, :1])
    if K > 1:
        assert torch.equal(a["rest"].grad.cpu(), ws[1][:, 1:])
    worst = {}

    def within(name, x, ref, bound):
        x, ref = x.double().numpy(), ref.detach().numpy()
        ratio = np.abs(x - ref) / bound
        k = int(np.argmax(ratio))
        worst[name] = float(ratio.reshape(-1)[k])
        return worst[name] <= 1.0, (name, k, worst[name])

    checks = []
    for name, x, ref in (("sigmoid", got[2], refs[2]), ("exp", got[3], refs[3]), ("normalize", got[4], refs[4]),
                         ("d_scaling", a["scl"].grad.cpu(), b["scl"].grad)):
        checks.append(within(name, x, ref, 4.0 * _ulp32(ref.detach().numpy())))
    checks.append(within("d_opacity", a["opa"].grad.cpu(), b["opa"].grad, 8.0 * hp.U32 * np.abs(ws[2].double().numpy())))
    row = (ws[4].double().norm(dim=1, keepdim=True) / b["rot"].detach().norm(dim=1, keepdim=True)).numpy()
    checks.append(within("d_rotation", a["rot"].grad.cpu(), b["rot"].grad, 8.0 * hp.U32 * np.broadcast_to(row, (P, 4))))
    print(f"\nP={P} K={K}: worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for ok, what in checks:
        assert ok, what


def test_fused_activations_write_into_the_bucket_without_copies(gpu, hip_lib):
    """With a GradBucket as sink the backward kernel writes the raw-parameter gradients into the flat bucket and autograd adopts
    those views as .grad (same storage, no accumulate kernel); an unused output (NULL incoming gradient) yields zeros even
    though the bucket is never zero-filled."""
    from moss_amd.activations import activate_gaussians
    from moss_amd.dist import GradBucket
    P, K = 777, 16
    a = _raw_params(P, K, gpu, seed=4)
    params = [a[k] for k in ("xyz", "dc", "rest", "opa", "scl", "rot")]
    bucket = GradBucket(params)
    bucket.flat.fill_(float("nan"))                          # stale contents must be overwritten, never accumulated into
    bucket.detach_grads()
    xyz, feat, opa, scl, rot = activate_gaussians(*params, bucket=bucket)
    w = torch.randn(P, K, 3, device=gpu)
    ((feat * w).sum() + (opa * 2.0).sum() + xyz.sum()).backward()       # scaling and rotation outputs unused
    for p, v in zip(params, bucket.views):
        assert p.grad is not None and p.grad.data_ptr() == v.data_ptr()
    bucket.collect()
    assert not any(bool(torch.isnan(v).any()) for v in bucket.views)      # (the <= 3-float alignment gaps between tensors are nobody's)
    assert torch.equal(a["rest"].grad, w[:, 1:, :]) and torch.equal(a["dc"].grad, w[:, :1, :])
    assert float(a["scl"].grad.abs().max()) == 0.0 and float(a["rot"].grad.abs().max()) == 0.0
    s = torch.sigmoid(a["opa"].detach())
    assert hp.rel_err(a["opa"].grad.cpu().numpy(), (2.0 * s * (1 - s)).cpu().numpy()) < 1e-6
    assert torch.equal(a["xyz"].grad, torch.ones_like(a["xyz"]))


def test_render_with_fused_activations_equals_torch_getters(gpu, hip_lib):
    """render() with pipe.fused_activations: same image, same raw-parameter gradients as the five torch getters."""
    from types import SimpleNamespace
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import render, camera_view
    s = scenes.config2()
    pc = GaussianSet(s, device=gpu)
    cam = camera_view(s.camera, gpu)
    bg = torch.tensor([0.2, 0.1, 0.0], device=gpu)
    w = torch.rand(3, s.camera.H, s.camera.W, device=gpu)
    res = {}
    for fused in (False, True):
        for cov_py in (False, True):
            pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=cov_py, debug=False, fused_activations=fused)
            pc.zero_grad()
            out = render(cam, pc, pipe, bg)
            ((out["render"] * w).sum() + out["render_alpha"].sum()).backward()      # render_depth unused: None gradient path
            res[(fused, cov_py)] = (out["render"].detach().clone(), [p.grad.detach().clone() for p in pc.parameters()],
                                    out["viewspace_points"].grad.detach().clone())
    for cov_py in (False, True):
        a, b = res[(False, cov_py)], res[(True, cov_py)]
        assert hp.rel_err(a[0].cpu().numpy(), b[0].cpu().numpy()) < 1e-5
        assert hp.rel_err(a[2].cpu().numpy(), b[2].cpu().numpy()) < 1e-4
        for ga, gb in zip(a[1], b[1]):
            assert hp.rel_err(ga.cpu().numpy(), gb.cpu().numpy()) < 1e-4


def test_backward_from_loss_equals_loss_backward(gpu, hip_lib):
    """backward_from_loss() (cached unit gradient, no ones_like fill, no multiply-by-one kernel) gives bit-identical gradients."""
    from moss_amd.loss import training_loss_fused, backward_from_loss
    torch.manual_seed(2)
    img = torch.rand(3, 96, 80, device=gpu); alpha = torch.rand(1, 96, 80, device=gpu)
    gt = torch.rand(3, 96, 80, device=gpu); mask = (torch.rand(1, 96, 80, device=gpu) > 0.5).float()
    res = []
    for fn in (lambda l: l.backward(), backward_from_loss, lambda l: (2.0 * l).backward()):
        a = img.clone().requires_grad_(True); b = alpha.clone().requires_grad_(True)
        fn(training_loss_fused(a, b, gt, mask))
        res.append((a.grad.clone(), b.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.allclose(res[2][0], 2.0 * res[0][0], rtol=1e-6, atol=0) and torch.allclose(res[2][1], 2.0 * res[0][1], rtol=1e-6, atol=0)


def test_flat_adamw_periodic_learning_rates(gpu, hip_lib):
    """One (P,16,3) SH parameter with the dc rate on the first 3 of every 48 floats and the rest rate elsewhere == torch.optim.AdamW
    over separate f_dc / f_rest tensors (the reference's two parameter groups, scene/gaussian_model.py:215-226)."""
    from moss_amd.dist import GradBucket
    from moss_amd.optim import FlatAdamW
    torch.manual_seed(5)
    P = 333
    init = torch.randn(P, 16, 3)
    xyz0 = torch.randn(P, 3)
    uni = torch.nn.Parameter(init.clone().to(gpu)); xa = torch.nn.Parameter(xyz0.clone().to(gpu))
    dc = torch.nn.Parameter(init[:, :1].clone().to(gpu)); rest = torch.nn.Parameter(init[:, 1:].clone().to(gpu)); xb = torch.nn.Parameter(xyz0.clone().to(gpu))
    ref = torch.optim.AdamW([{"params": [xb], "lr": 0.01}, {"params": [dc], "lr": 0.0025}, {"params": [rest], "lr": 0.0025 / 20}], lr=0.0, eps=1e-15)
    bucket = GradBucket([xa, uni])
    opt = FlatAdamW([{"params": [xa], "lr": 0.01}, {"params": [uni], "lr": 0.0025, "lr_pattern": (48, 3, 0.0025 / 20)}], bucket, eps=1e-15,
                    capturable=True)
    for it in range(4):
        bucket.attach()
        g = torch.randn(P, 16, 3, device=gpu); gx = torch.randn(P, 3, device=gpu)
        uni.grad.copy_(g); xa.grad.copy_(gx)
        dc.grad = g[:, :1].clone(); rest.grad = g[:, 1:].clone(); xb.grad = gx.clone()
        opt.step(); ref.step()
    assert hp.rel_err(uni[:, :1].detach().cpu().numpy(), dc.detach().cpu().numpy()) < 1e-6
    assert hp.rel_err(uni[:, 1:].detach().cpu().numpy(), rest.detach().cpu().numpy()) < 1e-6
    assert hp.rel_err(xa.detach().cpu().numpy(), xb.detach().cpu().numpy()) < 1e-6


def test_unified_features_step_equals_separate_features(gpu, hip_lib):
    """GaussianSet(unified_features=True): render() + backward with the dL_dsh sink gives the same image and the same gradients as
    the reference's separate _features_dc / _features_rest parameters (and writes them into the bucket without a copy)."""
    from types import SimpleNamespace
    from moss_amd.dist import GradBucket
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import render, camera_view
    import moss_amd.diff_gaussian_rasterization as dgr
    s = scenes.config2()
    cam = camera_view(s.camera, gpu)
    bg = torch.tensor([0.1, 0.0, 0.2], device=gpu)
    w = torch.rand(3, s.camera.H, s.camera.W, device=gpu)
    out = {}
    try:
        for uni in (False, True):
            pc = GaussianSet(s, device=gpu, unified_features=uni)
            bucket = GradBucket(list(pc.parameters()))
            pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, fused_activations=True,
                                   grad_bucket=bucket)
            dgr.set_grad_sink(sh=(lambda: bucket.sink_for(pc._features)) if uni else None)
            bucket.flat.fill_(float("nan"))
            bucket.detach_grads()
            r = render(cam, pc, pipe, bg)
            ((r["render"] * w).sum() + r["render_alpha"].sum()).backward()
            if uni:
                off = bucket._offset[id(pc._features)]
                assert pc._features.grad.data_ptr() == bucket.flat[off:off + 1].data_ptr()      # adopted, not copied
                assert bucket.sink_for(pc._features) is None                                   # single use per step (re-armed by detach_grads)
            bucket.collect()
            assert not any(bool(torch.isnan(v).any()) for v in bucket.views)      # (the <= 3-float alignment gaps between tensors are nobody's)
            feat_grad = pc._features.grad if uni else torch.cat((pc._features_dc.grad, pc._features_rest.grad), dim=1)
            out[uni] = (r["render"].detach().clone(), feat_grad.clone(), pc._xyz.grad.clone(), pc._opacity.grad.clone(),
                        pc._scaling.grad.clone(), pc._rotation.grad.clone())
    finally:
        dgr.set_grad_sink(sh=None)
    for a, b in zip(out[False], out[True]):
        assert torch.equal(a, b)


def test_transforms_inside_the_op_equal_python_covariance(gpu, hip_lib):
    """n2 extension: rasterizer(scales, rotations, transforms=T) == rasterizer(cov3D_precomp = get_covariance(.., T)) -- MOSS's shipped
    path (gaussian_renderer/__init__.py:88-91, scene/gaussian_model.py:37-44) -- in image and in the gradients of scales, rotations
    and T; asynchronous mode included."""
    import moss_amd.diff_gaussian_rasterization as dgr
    from moss_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    s = scenes.config1(P=400, W=96, H=80)
    c = s.camera
    rs = GaussianRasterizationSettings(image_height=c.H, image_width=c.W, tanfovx=c.tanfovx, tanfovy=c.tanfovy,
                                       bg=torch.tensor([0.1, 0.2, 0.3], device=gpu), scale_modifier=1.0, viewmatrix=c.viewmatrix.to(gpu),
                                       projmatrix=c.projmatrix.to(gpu), sh_degree=3, campos=c.campos.to(gpu), prefiltered=False, debug=False)
    rast = GaussianRasterizer(rs)
    w = torch.rand(3, c.H, c.W, device=gpu)
    leaf = lambda t: t.clone().to(gpu).requires_grad_(True)
    res = []
    try:
        for variant in ("python", "in_op", "in_op_async"):
            dgr.set_async(variant == "in_op_async")
            reps = 2 if variant == "in_op_async" else 1           # first call of an async session is synchronous
            for _ in range(reps):
                means, opa, shs = leaf(s.means3D), leaf(s.opacities), leaf(s.shs)
                scl, rot, T = leaf(s.scales), leaf(s.rotations), leaf(s.transforms)
                m2d = torch.zeros_like(means, requires_grad=True)
                if variant == "python":
                    cov = scenes.covariance_precomp(scl, rot, 1.0, T)
                    img, radii, depth, alpha = rast(means3D=means, means2D=m2d, opacities=opa, shs=shs, cov3D_precomp=cov)
                else:
                    img, radii, depth, alpha = rast(means3D=means, means2D=m2d, opacities=opa, shs=shs, scales=scl, rotations=rot,
                                                    transforms=T)
                ((img * w).sum() + alpha.sum() + 0.1 * depth.sum()).backward()
            res.append((img.detach(), radii, scl.grad, rot.grad, T.grad, means.grad, opa.grad, shs.grad))
    finally:
        dgr.set_async(False)
    py, op, op_async = res
    assert torch.equal(py[1], op[1])
    assert hp.rel_err(py[0].cpu().numpy(), op[0].cpu().numpy()) < 1e-5
    # scene.rotations are unit quaternions; covariance_precomp normalises, the kernel uses them as given: the rotation gradients
    # differ by the normalisation's projection, so compare its tangential part
    q = s.rotations.to(gpu)
    tang = lambda g: g - q * (g * q).sum(1, keepdim=True)
    for k in (2, 4, 5, 6, 7):
        assert hp.rel_err(py[k].cpu().numpy(), op[k].cpu().numpy()) < 2e-4, k
    assert hp.rel_err(tang(py[3]).cpu().numpy(), tang(op[3]).cpu().numpy()) < 2e-4
    for a, b in zip(op, op_async):
        assert torch.equal(a, b)                                  # asynchronous == synchronous, bit for bit
    with pytest.raises(Exception):
        rast(means3D=means, means2D=m2d, opacities=opa, shs=shs, cov3D_precomp=cov, transforms=T)


def test_means_posed_inside_the_op_equal_the_torch_posing(gpu, hip_lib):
    """MOSS_RAW_POSE: rasterizer(means3D = canonical x, transforms = T, translation = t, raw_flags |= RAW_POSE) is the reference caller's
    `means3D = torch.matmul(transforms, means3D[..., None]).squeeze(-1) + translation` (gaussian_renderer/__init__.py:74-77) followed
    by the op, without the torch kernels:
      * every integer stage (radii, sorted keys, ranges) is BIT-EXACT against the CPU oracle run on means posed with the kernel's
        expression (rows of T times x summed left to right, then t: float32, one rounding per operation);
      * the gradients of x, T and t equal those autograd sends back through the torch posing."""
    means_posed_inside_the_op_equal_the_torch_posing(scenes.config1(P=500, W=112, H=96), gpu)


def means_posed_inside_the_op_equal_the_torch_posing(s, gpu):
    """The body of the test above for a scene `s` (also called by tests/test_gpu_cameras.py under a general camera)."""
    import moss_amd.diff_gaussian_rasterization as dgr
    from moss_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C
    c = s.camera
    g = torch.Generator().manual_seed(21)
    T = (torch.eye(3) + 0.1 * torch.randn(s.P, 3, 3, generator=g)).float()
    t = (0.05 * torch.randn(s.P, 3, generator=g)).float()
    x = s.means3D.float()
    Tn, xn, tn = T.numpy(), x.numpy(), t.numpy()
    posed = np.empty_like(xn)
    for r in range(3):
        posed[:, r] = ((Tn[:, r, 0] * xn[:, 0] + Tn[:, r, 1] * xn[:, 1]) + Tn[:, r, 2] * xn[:, 2]) + tn[:, r]
    assert posed.dtype == np.float32
    # ---- integer stages against the oracle on the posed means (through the raw C-level entry: hp.hip_forward has no pose argument)
    d = hp.inputs_of(s, "lbs")
    d.transforms = T
    d_oracle = hp.inputs_of(s, "lbs"); d_oracle.transforms = T; d_oracle.means3D = torch.from_numpy(posed)
    fw = hp.oracle_forward(d_oracle)
    a = dict(bg=d.bg.to(gpu), means3D=x.to(gpu), opacity=d.opacities.to(gpu), scales=d.scales.to(gpu), rotations=d.rotations.to(gpu),
             view=c.viewmatrix.to(gpu), proj=c.projmatrix.to(gpu), sh=d.shs.to(gpu), campos=c.campos.to(gpu))
    empty = torch.Tensor([])
    from types import SimpleNamespace
    tt = SimpleNamespace()
    (tt.R, tt.color, tt.depth, tt.alpha, tt.radii, tt.geom, tt.binning, tt.img) = _C.rasterize_gaussians(
        a["bg"], a["means3D"], empty, a["opacity"], a["scales"], a["rotations"], 1.0, empty, a["view"], a["proj"], c.tanfovx, c.tanfovy,
        c.H, c.W, a["sh"], d.degree, a["campos"], False, False, transforms=T.to(gpu), raw_flags=_C.RAW_POSE, translation=t.to(gpu))
    e = hp.hip_export(d, tt, gpu)
    assert np.array_equal(e.radii, fw.radii) and tt.R == fw.num_rendered
    assert np.array_equal(e.point_list_keys, fw.point_list_keys) and np.array_equal(e.point_list, fw.point_list)
    assert np.array_equal(e.ranges, fw.ranges) and np.array_equal(e.n_contrib, fw.n_contrib)
    assert hp.rel_err(e.color, fw.color) < 2e-5 and hp.rel_err(e.alpha, fw.alpha) < 2e-5
    # ---- gradients against the torch posing
    rs = GaussianRasterizationSettings(image_height=c.H, image_width=c.W, tanfovx=c.tanfovx, tanfovy=c.tanfovy,
                                       bg=torch.tensor([0.1, 0.2, 0.3], device=gpu), scale_modifier=1.0, viewmatrix=c.viewmatrix.to(gpu),
                                       projmatrix=c.projmatrix.to(gpu), sh_degree=3, campos=c.campos.to(gpu), prefiltered=False, debug=False)
    rast = GaussianRasterizer(rs)
    w = torch.rand(3, c.H, c.W, device=gpu)
    leaf = lambda v: v.clone().to(gpu).requires_grad_(True)
    res = []
    for variant in ("torch", "in_op", "in_op_no_translation"):
        xs, opa, shs, scl, rot, Tl, tl = leaf(x), leaf(s.opacities), leaf(s.shs), leaf(s.scales), leaf(s.rotations), leaf(T), leaf(t)
        m2d = torch.zeros_like(xs, requires_grad=True)
        if variant == "torch":
            means = (Tl * xs[:, None, :]).sum(-1) + tl
            img, radii, depth, alpha = rast(means3D=means, means2D=m2d, opacities=opa, shs=shs, scales=scl, rotations=rot, transforms=Tl)
        elif variant == "in_op":
            img, radii, depth, alpha = rast(means3D=xs, means2D=m2d, opacities=opa, shs=shs, scales=scl, rotations=rot, transforms=Tl,
                                            raw_flags=_C.RAW_POSE, translation=tl)
        else:
            img, radii, depth, alpha = rast(means3D=xs, means2D=m2d, opacities=opa, shs=shs, scales=scl, rotations=rot, transforms=Tl,
                                            raw_flags=_C.RAW_POSE)
        ((img * w).sum() + alpha.sum() + 0.1 * depth.sum()).backward()
        res.append((img.detach(), radii, xs.grad, Tl.grad, tl.grad, scl.grad, rot.grad, opa.grad, shs.grad, m2d.grad))
    ref, op, op0 = res
    assert hp.rel_err(ref[0].cpu().numpy(), op[0].cpu().numpy()) < 1e-5
    assert float((ref[1] != op[1]).float().mean()) < 0.01       # (torch may sum the three products in another order: a radius can move by one)
    for k in range(2, 10):
        assert hp.rel_err(op[k].cpu().numpy(), ref[k].cpu().numpy()) < 2e-4, k
    assert op0[4] is None and float((op0[0] - op[0]).abs().max()) > 1e-3      # without a translation: another image, no translation gradient
    with pytest.raises(Exception):
        rast(means3D=xs, means2D=m2d, opacities=opa, shs=shs, scales=scl, rotations=rot, raw_flags=_C.RAW_POSE)      # no transforms


# ---------------------------------------------------------------- k-NN query (replacement for the knn_cuda wheel, row n3)
@pytest.mark.parametrize("Nr,Nq,k", [(6890, 20000, 1), (3000, 3000, 2), (5, 17, 4), (1025, 300, 3)])
def test_knn_query_matches_exhaustive_search(gpu, hip_lib, Nr, Nq, k):
    """KNN(k, transpose_mode=True)(ref, query) as MOSS calls it (scene/gaussian_model.py:85-86,586,657,827): indices and Euclidean
    distances equal an exhaustive float64 search (random points: no ties)."""
    from knn_cuda import KNN
    g = torch.Generator().manual_seed(Nr + k)
    ref = torch.randn(1, Nr, 3, generator=g)
    query = ref.clone() if Nr == Nq else torch.randn(1, Nq, 3, generator=g)
    dist, idx = KNN(k=k, transpose_mode=True)(ref.to(gpu), query.to(gpu))
    assert dist.shape == (1, Nq, k) and idx.shape == (1, Nq, k) and idx.dtype == torch.int64
    d_ref = torch.cdist(query.double(), ref.double())[0]
    want_d, want_i = d_ref.topk(k, dim=1, largest=False)
    assert torch.equal(idx[0].cpu(), want_i)
    assert hp.rel_err(dist[0].cpu().numpy(), want_d.float().numpy()) < 1e-5 or float((dist[0].cpu() - want_d.float()).abs().max()) < 1e-6
    if Nr == Nq:                                                  # self query: the point itself comes first at distance 0
        assert torch.equal(idx[0, :, 0].cpu(), torch.arange(Nq)) and float(dist[0, :, 0].abs().max()) == 0.0


def test_knn_dimension_major_mode_and_ties(gpu, hip_lib):
    from knn_cuda import KNN
    ref = torch.tensor([[[0.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [5.0, 0, 0]]], device=gpu)        # two identical references
    query = torch.tensor([[[0.9, 0, 0]]], device=gpu)
    d, i = KNN(k=3, transpose_mode=True)(ref, query)
    assert i[0, 0].tolist() == [1, 2, 0]                           # equal distances: the lower index first
    d2, i2 = KNN(k=3, transpose_mode=False)(ref.transpose(1, 2).contiguous(), query.transpose(1, 2).contiguous())
    assert d2.shape == (1, 3, 1) and torch.equal(i2[0, :, 0], i[0, 0]) and torch.equal(d2[0, :, 0], d[0, 0])
    with pytest.raises(RuntimeError):
        KNN(k=1, transpose_mode=True)(ref.cpu(), query.cpu())


# ---------------------------------------------------------------- cell-grid k-NN, densification statistics, neighbour KL (rows n3/n4)
def _body_points(n, seed, spread=0.02):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(n, generator=g) * 1.7
    ang = torch.rand(n, generator=g) * 6.2831853
    rad = 0.1 + 0.1 * torch.rand(n, generator=g)
    pts = torch.stack([rad * torch.cos(ang), t, rad * torch.sin(ang)], 1) + spread * torch.randn(n, 3, generator=g)
    return pts.float()


@pytest.mark.parametrize("Nr,Nq,k", [(1, 5, 1), (7, 100, 4), (3000, 2500, 1), (6890, 20000, 1), (20000, 20000, 2), (50000, 3000, 3)])
def test_knn_grid_is_identical_to_brute_force(gpu, hip_lib, Nr, Nq, k):
    from knn_cuda import knn
    ref = _body_points(Nr, 1).cuda()
    query = (ref if Nr == Nq else _body_points(Nq, 2)).cuda()
    d0, i0 = knn(ref[None], query[None], k, "brute")
    d1, i1 = knn(ref[None], query[None], k, "grid")
    torch.cuda.synchronize()
    assert torch.equal(i0, i1)
    assert torch.equal(d0, d1)


def test_knn_grid_ties_outliers_and_degenerate_boxes(gpu, hip_lib):
    from knn_cuda import knn, KnnGrid
    # duplicates (ties broken by index), coplanar references (a degenerate bounding box), queries far outside the box
    g = torch.Generator().manual_seed(5)
    base = torch.rand(1500, 3, generator=g)
    base[:, 2] = 0.25
    ref = torch.cat([base, base[:700]]).cuda()
    query = torch.cat([base[:900], torch.tensor([[5.0, -3.0, 2.0], [-40.0, 0.5, 0.25], [0.5, 0.5, 1e4]])]).cuda()
    d0, i0 = knn(ref[None], query[None], 4, "brute")
    d1, i1 = knn(ref[None], query[None], 4, "grid")
    assert torch.equal(i0, i1) and torch.equal(d0, d1)
    # all references identical: one cell
    same = torch.full((3000, 3), 0.5).cuda()
    d0, i0 = knn(same[None], query[None], 3, "brute")
    d1, i1 = knn(same[None], query[None], 3, "grid")
    assert torch.equal(i0, i1) and torch.equal(d0, d1)
    # a kept grid answers several queries and ignores later changes of the reference tensor
    grid = KnnGrid(ref)
    ref.zero_()
    d2, i2 = grid.query(query, 2)
    d3, i3 = knn(torch.cat([base, base[:700]]).cuda()[None], query[None], 2, "brute")
    assert torch.equal(i2, i3[0]) and torch.equal(d2, d3[0])


def test_knn_grid_matches_the_exhaustive_oracle(gpu, hip_lib):
    from knn_cuda import KNN
    from oracle import oracle
    ref = _body_points(5000, 3)
    query = _body_points(4000, 4)
    d, i = KNN(2, transpose_mode=True, impl="grid")(ref.cuda()[None], query.cuda()[None])
    d_ref, i_ref = oracle.knn_exhaustive(ref.numpy(), query.numpy(), 2)
    assert np.array_equal(i[0].cpu().numpy(), i_ref)
    np.testing.assert_array_equal(d[0].cpu().numpy(), d_ref)


def test_densify_stats_match_the_reference_expressions(gpu, hip_lib):
    from moss_amd.densify import DensifyStats
    from oracle import oracle
    P = 5000
    g = torch.Generator().manual_seed(11)
    stats = DensifyStats(P)
    acc, den, mr = np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(P, np.float32)
    for it in range(3):
        radii = (torch.randint(-2, 40, (P,), generator=g) * (torch.rand(P, generator=g) > 0.3)).int()
        grad = torch.randn(P, 3, generator=g)
        stats.add(radii.cuda(), grad.cuda())
        acc, den, mr = oracle.densify_stats(radii.numpy(), grad.numpy(), acc, den, mr)
    np.testing.assert_array_equal(stats.denom.cpu().numpy().ravel(), den)
    np.testing.assert_array_equal(stats.max_radii2D.cpu().numpy(), mr)
    np.testing.assert_allclose(stats.xyz_gradient_accum.cpu().numpy().ravel(), acc, rtol=3e-7, atol=0)   # sqrt rounding only
    # the reference's own torch expressions on the GPU
    t_acc = torch.zeros(P, 1).cuda(); t_den = torch.zeros(P, 1).cuda(); t_mr = torch.zeros(P).cuda()
    s2 = DensifyStats(P)
    radii = torch.randint(0, 30, (P,), generator=g).int().cuda(); grad = torch.randn(P, 3, generator=g).cuda()
    vis = radii > 0
    t_mr[vis] = torch.max(t_mr[vis], radii[vis].float())
    t_acc[vis] += torch.norm(grad[vis, :2], dim=-1, keepdim=True); t_den[vis] += 1
    s2.add(radii, grad)
    assert torch.equal(s2.denom, t_den) and torch.equal(s2.max_radii2D, t_mr)
    torch.testing.assert_close(s2.xyz_gradient_accum, t_acc, rtol=1e-6, atol=0)
    g_mean = s2.mean_grads()
    assert not g_mean.isnan().any() and (g_mean[~vis] == 0).all()


def test_neighbour_kl_matches_the_float64_oracle(gpu, hip_lib):
    from moss_amd.densify import neighbour_kl, cal_kl
    from oracle import oracle
    P = 20000
    g = torch.Generator().manual_seed(12)
    xyz = _body_points(P, 6)
    rot = torch.randn(P, 4, generator=g)
    scaling = torch.exp(torch.randn(P, 3, generator=g) * 0.5 + np.log(0.01)).float()
    kl, ids = cal_kl(xyz.cuda(), rot.cuda(), scaling.cuda())
    ids_np = ids.cpu().numpy()
    assert (ids_np[:, 0] == np.arange(P)).all()                      # distinct points: the nearest is the point itself
    want, mag = oracle.kl_div(xyz.numpy()[ids_np[:, 0]], rot.numpy()[ids_np[:, 0]], scaling.numpy()[ids_np[:, 0]],
                              xyz.numpy()[ids_np[:, 1]], rot.numpy()[ids_np[:, 1]], scaling.numpy()[ids_np[:, 1]])
    err = np.abs(kl.cpu().numpy().astype(np.float64) - want)
    assert (err <= 2e-5 * mag).all(), float((err / mag).max())       # fp32 evaluation vs float64, relative to the terms' magnitude
    # explicit pairs, including a Gaussian against itself (KL = 0 up to rounding) and an invalid index (NaN, no fault)
    pairs = torch.tensor([[0, 0], [5, 9], [9, 5], [3, P]], dtype=torch.int64).cuda()
    out = neighbour_kl(xyz.cuda(), rot.cuda(), scaling.cuda(), pairs).cpu().numpy()
    assert abs(out[0]) < 1e-5 and np.isnan(out[3]) and out[1] != out[2]


def test_scale_beyond_the_largest_baseline_config(gpu, hip_lib):
    """1M Gaussians at 2048x2048 (3.8M instances; BASELINE's largest is 300k at 1024^2): forward + backward run, are finite, and
    are bit-identical across two runs (the gradient reduction has a fixed order).  scripts/stress_large.py takes it to 4M / 4096^2."""
    from moss_amd import scenes
    sc = scenes.body_scene(1_000_000, 2048, 2048, 540.0 * 4, init_like=False, name="stress")
    d = hp.inputs_of(sc, "scale_rot")
    runs = []
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    for _ in range(2):
        t = hp.hip_forward(d, gpu)
        dc, dd, da = hp.image_grads(2048, 2048, seed=5)
        g = hp.hip_backward(d, t, dc, dd, da, gpu)
        runs.append((t.R, t.color.clone(), g.dL_dmeans3D.clone(), g.dL_dsh.clone(), g.dL_dscales.clone()))
    assert runs[0][0] == runs[1][0] > 3_000_000
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    # Scratch: the binning buffer of this frame (the synchronous forward sizes the gradient-record pool for the frame's cells exactly)
    # and the whole test's peak (inputs, two runs' outputs and gradients, scratch): rounds 1-4 held 16 record slabs per instance --
    # 834 B per instance, 3.2 GB for this frame; review item 7 of round 4 asked for <= 400 B per instance and <= 4 GiB peak here.
    R = runs[0][0]
    per_instance = t.binning.numel() / R
    assert per_instance <= 400, per_instance
    assert hip_lib.moss_raster_binning_bytes(R) <= 400 * R
    assert torch.cuda.max_memory_allocated() <= 4 << 30, torch.cuda.max_memory_allocated() / 2**30
    print(f"1M Gaussians: R = {R}, binning buffer {t.binning.numel() / 2**20:.0f} MiB = {per_instance:.0f} B per instance, "
          f"peak allocated {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB")


@pytest.mark.parametrize("with_transforms", [False, True])
def test_raw_parameters_inside_the_op_equal_the_torch_getters(gpu, hip_lib, with_transforms):
    """moss_raster_forward_raw / _backward_raw: sigmoid / exp / normalize of the raw GaussianModel parameters inside preprocess give
    the image and the raw-parameter gradients of the torch getters + the plain op (also together with in-op transforms, with
    unnormalised quaternions, and through the gradient sinks that write straight into a bucket)."""
    from types import SimpleNamespace
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import render, camera_view
    from moss_amd import diff_gaussian_rasterization as dgr
    from moss_amd.dist import GradBucket
    s = scenes.config2()
    cam = camera_view(s.camera, gpu)
    bg = torch.tensor([0.1, 0.2, 0.3], device=gpu)
    g = torch.Generator().manual_seed(4)
    T = (torch.eye(3) + 0.05 * torch.randn(s.means3D.shape[0], 3, 3, generator=g)).to(gpu) if with_transforms else None
    w = torch.rand(3, s.camera.H, s.camera.W, device=gpu)
    res = {}
    for raw in (False, True):
        pc = GaussianSet(s, device=gpu, unified_features=True)
        with torch.no_grad():
            pc._rotation.mul_(torch.rand(pc._rotation.shape[0], 1, device=gpu) * 3 + 0.2)      # far from unit length
        pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, fused_activations=False,
                               transforms_in_op=with_transforms, raw_parameters_in_op=raw)
        out = render(cam, pc, pipe, bg, transforms=T)
        ((out["render"] * w).sum() + (out["render_alpha"] ** 2).sum() + out["render_depth"].sum()).backward()
        res[raw] = (out["render"].detach().cpu().numpy(), {n: p.grad.detach().cpu().numpy() for n, p in pc.named_parameters()},
                    out["viewspace_points"].grad.detach().cpu().numpy())
    assert hp.rel_err(res[False][0], res[True][0]) < 1e-5
    assert hp.rel_err(res[False][2], res[True][2]) < 1e-4
    for n in res[False][1]:
        assert hp.rel_err(res[False][1][n], res[True][1][n]) < 2e-4, n
    if with_transforms:
        return
    # sinks: the raw-parameter gradients land in the bucket without a copy
    pc = GaussianSet(s, device=gpu, unified_features=True)
    bucket = GradBucket(list(pc.parameters()))
    dgr.set_grad_sink(sh=lambda: bucket.sink_for(pc._features), means3D=lambda: bucket.sink_for(pc._xyz),
                      opacity=lambda: bucket.sink_for(pc._opacity), scales=lambda: bucket.sink_for(pc._scaling),
                      rotations=lambda: bucket.sink_for(pc._rotation))
    try:
        bucket.flat.fill_(float("nan"))
        bucket.detach_grads()
        pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raw_parameters_in_op=True)
        out = render(cam, pc, pipe, bg)
        ((out["render"] * w).sum() + (out["render_alpha"] ** 2).sum() + out["render_depth"].sum()).backward()
        for p, v in zip(bucket.params, bucket.views):
            assert p.grad.data_ptr() == v.data_ptr()                 # adopted, not copied
        assert not any(bool(torch.isnan(v).any()) for v in bucket.views)      # (the <= 3-float alignment gaps between tensors are nobody's)
    finally:
        dgr.set_grad_sink()


def test_block_mask_culling_never_changes_a_result(gpu, hip_lib):
    """The per-instance block masks only SKIP (entry, block) pairs that cannot reach alpha >= 1/255 in that block.  With the masks
    switched off (``debug = MOSS_DEBUG_NO_BLOCK_CULL`` on the forward and the backward call -- an argument since ABI 2, a process-wide
    switch before; since ABI 3 on EVERY entry point, also the in-op transform / raw-parameter ones the bench and MOSS's data flow use:
    every entry is blended against every block) the DECISIONS must be the same:
    final_T and n_contrib bit-identical; colour / depth / alpha equal up to fp32 summation order (a pixel's sums are kept as four
    per-slot partial sums, and which slot an entry lands in depends on how many entries were skipped before it); every gradient equal
    up to rounding -- since round 2 the forward cuts a block's list every 64 HITS into depth segments, the unculled run cuts elsewhere,
    and a segment starts its suffix state from the stored sums instead of from the recurrence (1e-5 of the largest value).  Checked on
    the body scene, on anisotropic random Gaussians with a precomputed (transformed) covariance, and with Gaussians that cover the
    whole image and opacities around the 1/255 threshold."""
    NO_BLOCK_CULL = 2                                                        # include/moss_raster.h MOSS_DEBUG_NO_BLOCK_CULL
    cases = [hp.inputs_of(scenes.config2(), "scale_rot"), hp.inputs_of(scenes.config1(), "precomp"), hp.inputs_of(scenes.config1(), "lbs")]
    big = scenes.config1(P=600, W=200, H=136, seed=77)
    big.scales[:12] *= 40.0
    big.opacities[:200] = torch.linspace(0.0, 0.02, 200)[:, None]            # around the 1/255 threshold
    cases.append(hp.inputs_of(big, "scale_rot"))
    for d in cases:
        outs = []
        for dbg in (0, NO_BLOCK_CULL):
            t = hp.hip_forward(d, gpu, debug=dbg)
            e = hp.hip_export(d, t, gpu)
            dc, dd, da = hp.image_grads(d.H, d.W, seed=3)
            g = hp.hip_backward(d, t, dc, dd, da, gpu, debug=dbg)
            outs.append(([t.color.cpu(), t.depth.cpu(), t.alpha.cpu()],
                         [torch.from_numpy(e.final_T), torch.from_numpy(e.n_contrib.astype(np.int64))],
                         [v.cpu() for v in vars(g).values() if v is not None]))
        for a, b in zip(outs[0][0], outs[1][0]):
            assert float((a - b).abs().max()) <= 2e-6 * max(1.0, float(b.abs().max()))
        for a, b in zip(outs[0][1], outs[1][1]):
            assert torch.equal(a, b)
        for a, b in zip(outs[0][2], outs[1][2]):
            assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-30


def test_two_renders_into_one_backward_with_gradient_sinks(gpu, hip_lib):
    """a gradient sink is OVERWRITTEN by the backward kernel, so when a parameter receives gradients from two rasterizer
    calls in one autograd pass (two views before one loss.backward()) the second call must not be handed the slice .grad already
    aliases.  GradBucket.sink_for is single-use per step: the result is the SUM of both views' gradients, as without sinks.
    Also: two RasterContexts in one process keep separate sinks and asynchronous-forward state."""
    from types import SimpleNamespace
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import render, camera_view
    from moss_amd import diff_gaussian_rasterization as dgr
    from moss_amd.dist import GradBucket
    s = scenes.config2()
    poses = scenes.look_at_ring(8)
    cams = []
    for R_, t_ in (poses[0], poses[1]):
        c0 = s.camera
        cams.append(camera_view(scenes.make_camera(c0.W, c0.H, float(c0.K[0, 0]), float(c0.K[1, 1]), float(c0.K[0, 2]), float(c0.K[1, 2]), R_, t_), gpu))
    bg = torch.zeros(3, device=gpu)
    w = torch.rand(3, s.camera.H, s.camera.W, device=gpu)

    def two_view_loss(pc, pipe):
        tot = 0.0
        for cam in cams:
            out = render(cam, pc, pipe, bg)
            tot = tot + (out["render"] * w).sum() + out["render_alpha"].sum()
        return tot

    # reference: no sinks, autograd accumulates
    pc0 = GaussianSet(s, device=gpu, unified_features=True)
    pipe0 = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raw_parameters_in_op=True)
    two_view_loss(pc0, pipe0).backward()
    want = {n: p.grad.detach().clone() for n, p in pc0.named_parameters()}
    # with sinks, in a context of its own
    ctx = dgr.RasterContext()
    pc = GaussianSet(s, device=gpu, unified_features=True)
    bucket = GradBucket(list(pc.parameters()))
    ctx.set_grad_sink(sh=lambda: bucket.sink_for(pc._features), means3D=lambda: bucket.sink_for(pc._xyz),
                      opacity=lambda: bucket.sink_for(pc._opacity), scales=lambda: bucket.sink_for(pc._scaling),
                      rotations=lambda: bucket.sink_for(pc._rotation))
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raw_parameters_in_op=True, raster_context=ctx)
    for _ in range(2):                                       # twice: detach_grads() re-arms the slices for the next step
        bucket.detach_grads()
        two_view_loss(pc, pipe).backward()
        bucket.collect()
        for n, p in pc.named_parameters():
            assert hp.rel_err(p.grad.cpu().numpy(), want[n].cpu().numpy()) < 1e-6, n
    assert all(v is None for v in dgr._C.DEFAULT.sinks.values())          # the default context never saw these sinks
    # asynchronous-forward state is per context too
    ctx.set_async(True)
    try:
        render(cams[0], pc, pipe, bg)
        assert ctx.capacity > 0 and dgr._C.DEFAULT.capacity == 0 and not dgr._C.DEFAULT.enabled
    finally:
        ctx.set_async(False)
