"""The fused LBS deformation on the device (C ABI moss_lbs_deform_forward / _backward, moss_amd.lbs): the kernels against float64
autograd of moss_amd.lbs.deform_torch, the drop-in coarse_deform_c2source against the reference's own numbers
(tests/golden/lbs_deform.npz), determinism, no host synchronisation, capture in a hipGraph with a new frame per replay, the renderer's
``pipe.lbs_in_op`` path and the refusals.

The bars.  Per Gaussian the kernel forms O(1) float32 products of O(1) factors -- except Q = B3^-1, whose error is ~ kappa(B3) eps
relative.  With the row scales (Frobenius norms, float64)
    s_T = |M| |Q|,   s_t = s_T |b| + |M| |d| + |o| + |Th|,   s_p = s_T |x| + s_t
an element of row i of T / t / p may be off by  c kappa_i eps32 s_i,  c = 64 zeta,  zeta = 1 + max |L| (the softmax's exponent:
an error of eps |z| in z is a relative error of the weight, and every blended entry inherits it).  The weights: c eps32 absolute.
Backward: every adjoint term is a product of the incoming gradient G_i = |gT| + |gt| + |gp| (1 + |x|) with at most three of
(|Q| + |u| + 1), (|M| + 1), (|Q| + |b| + 1) and one entry of A; inverting once more (gB3 = -Q^T gQ Q^T) multiplies the relative
error by kappa once more, so a row of gL / gd / gx may be off by  c kappa_i^2 eps32 G_i S_i  (S_i that product of norms, times
max |A|), and element j of gA_obs, a sum over the Gaussians, by the sum of its terms' bars:  c eps32 sum_i w_ij kappa_i^2 G_i S_i.
Each test prints the worst ratio of error to bar it met.
"""
from types import SimpleNamespace

import gc

import numpy as np
import pytest
import torch

from moss_amd import lbs as mlbs

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
SIZES = [1, 63, 64, 65, 6890, 45695, 100000]


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    """Leave the device as the module found it.  Later tests bound their peak allocation (test_gpu_ops.py's 1M-Gaussian test), and
    this module's matmuls and inverses on the side streams of its captures leave a BLAS workspace per stream in torch's allocator
    (~600 MiB measured in all): they, and whatever a collection frees, are released here."""
    yield
    before = torch.cuda.memory_allocated()
    gc.collect()
    torch.cuda.synchronize()
    torch._C._cuda_clearCublasWorkspaces()
    torch.cuda.empty_cache()
    print(f"\ntest_gpu_lbs: {before / 2**20:.0f} MiB allocated at the end, {torch.cuda.memory_allocated() / 2**20:.0f} MiB after a collection")


def make_case(P, J, seed, dev, V=256):
    """float64 inputs on ``dev``: ids, W, L, A_big, A_obs, d, R, Th, x of a synthetic body and frame."""
    body = mlbs.synthetic_body_model(V, J, seed=seed)
    A_big = mlbs.smpl_joint_transforms(body, mlbs.synthetic_frame(0, J, big_pose=True))[0][0]
    fr = mlbs.synthetic_frame(seed, J)
    A_obs, R, Th = mlbs.smpl_joint_transforms(body, fr)
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (P,), generator=g)
    f64 = lambda t: t.to(dtype=torch.float64, device=dev)                          # noqa: E731
    return {"ids": ids.to(dev), "W": f64(body["weights"]), "L": f64(0.7 * torch.randn(P, J, generator=g)), "A_big": f64(A_big),
            "A_obs": f64(A_obs[0]), "d": f64(0.01 * torch.randn(P, 3, generator=g)), "R": f64(R.reshape(3, 3)),
            "Th": f64(Th.reshape(3)), "x": f64(body["v_template"][ids] + 0.03 * torch.randn(P, 3, generator=g))}


def f32(c):
    return {k: (v if k == "ids" else v.float().contiguous()) for k, v in c.items()}


def row_scales(c, L):
    """kappa (P,), the forward row scales s_T, s_t, s_p and the backward product S (float64)."""
    J = c["W"].shape[1]
    w = c["W"][c["ids"]]
    if L is not None:
        w = torch.softmax(torch.log(w + 1e-9) + L, -1)
    B = (w @ c["A_big"].reshape(J, 16)).reshape(-1, 4, 4)
    O = (w @ c["A_obs"].reshape(J, 16)).reshape(-1, 4, 4)
    Q = torch.inverse(B[:, :3, :3])
    M = c["R"] @ O[:, :3, :3]
    n = lambda t: t.flatten(1).norm(dim=1)                                          # noqa: E731
    kappa = torch.linalg.cond(B[:, :3, :3])
    b, o = B[:, :3, 3], O[:, :3, 3]
    u = c["d"] - (Q @ b[..., None]).squeeze(-1)
    sT = n(M) * n(Q)
    st = sT * b.norm(dim=1) + n(M) * c["d"].norm(dim=1) + o.norm(dim=1) + c["Th"].norm()
    sp = sT * c["x"].norm(dim=1) + st
    amax = max(float(c["A_big"].abs().max()), float(c["A_obs"].abs().max()))
    S = (n(Q) + u.norm(dim=1) + 1) * (n(M) + 1) * (n(Q) + b.norm(dim=1) + 1) * amax
    return kappa, sT, st, sp, S, w


def zeta(L):
    return 1.0 + (0.0 if L is None else float(L.abs().max()))


def ratio(err, bar):
    """max over rows of (max abs error in the row) / bar of the row."""
    err = err.reshape(err.shape[0], -1).abs().amax(1) if err.dim() > 1 else err.abs()
    return float((err / bar).max())


@pytest.mark.parametrize("J", [24, 55])
@pytest.mark.parametrize("P", SIZES)
def test_forward_matches_float64(gpu, hip_lib, P, J):
    c = make_case(P, J, 100 + P % 97 + J, gpu)
    c32 = f32(c)
    worst = 0.0
    for with_L in (True, False):
        for with_x in (True, False):
            for want_w in (True, False):
                L, L32 = (c["L"], c32["L"]) if with_L else (None, None)
                x, x32 = (c["x"], c32["x"]) if with_x else (None, None)
                T, t, p, w = mlbs.lbs_deform(c32["ids"], c32["W"], L32, c32["A_big"], c32["A_obs"], c32["d"], c32["R"], c32["Th"],
                                             x=x32, want_weights=want_w)
                T0, t0, p0, w0 = mlbs.deform_torch(c["ids"], c["W"], L, c["A_big"], c["A_obs"], c["d"], c["R"], c["Th"], x=x)
                kappa, sT, st, sp, _, _ = row_scales(c, L)
                k = 64.0 * zeta(L) * EPS32 * kappa
                assert T.shape == (P, 3, 3) and t.shape == (P, 3)
                r = [ratio(T.double() - T0, k * sT), ratio(t.double() - t0, k * st)]
                if with_x:
                    r.append(ratio(p.double() - p0, k * sp))
                else:
                    assert p is None
                if want_w:
                    assert w.shape == (P, J) and not w.requires_grad
                    r.append(float((w.double() - w0).abs().max()) / (64.0 * zeta(L) * EPS32))
                else:
                    assert w is None
                worst = max(worst, *r)
    print(f"\nforward P={P} J={J}: worst error / bar {worst:.3g}")
    assert worst < 1.0


@pytest.mark.parametrize("J", [24, 55])
@pytest.mark.parametrize("P", SIZES)
def test_backward_matches_float64_autograd(gpu, hip_lib, P, J):
    c = make_case(P, J, 200 + P % 89 + J, gpu)
    g = torch.Generator(device=gpu).manual_seed(P + J)
    gT = torch.randn(P, 3, 3, generator=g, device=gpu, dtype=torch.float64)
    gt = torch.randn(P, 3, generator=g, device=gpu, dtype=torch.float64)
    gp = torch.randn(P, 3, generator=g, device=gpu, dtype=torch.float64)
    worst = 0.0
    for with_L in (True, False):
        leaves64 = {k: c[k].clone().requires_grad_(True) for k in ("A_obs", "d", "x")}
        leaves32 = {k: c[k].float().clone().requires_grad_(True) for k in ("A_obs", "d", "x")}
        if with_L:
            leaves64["L"] = c["L"].clone().requires_grad_(True)
            leaves32["L"] = c["L"].float().clone().requires_grad_(True)
        c32 = f32(c)
        T, t, p, _ = mlbs.lbs_deform(c32["ids"], c32["W"], leaves32.get("L"), c32["A_big"], leaves32["A_obs"], leaves32["d"],
                                     c32["R"], c32["Th"], x=leaves32["x"])
        torch.autograd.backward([T, t, p], [gT.float(), gt.float(), gp.float()])
        T0, t0, p0, _ = mlbs.deform_torch(c["ids"], c["W"], leaves64.get("L"), c["A_big"], leaves64["A_obs"], leaves64["d"],
                                          c["R"], c["Th"], x=leaves64["x"])
        torch.autograd.backward([T0, t0, p0], [gT, gt, gp])
        kappa, _, _, _, S, w = row_scales(c, c["L"] if with_L else None)
        G = gT.flatten(1).norm(dim=1) + gt.norm(dim=1) + gp.norm(dim=1) * (1 + c["x"].norm(dim=1))
        rowbar = 64.0 * zeta(c["L"] if with_L else None) * EPS32 * kappa ** 2 * G * S
        for k in leaves32:
            assert leaves32[k].grad is not None, k
            err = leaves32[k].grad.double() - leaves64[k].grad
            if k == "A_obs":
                bar = (w * rowbar[:, None]).sum(0)                                  # (J,)
                assert torch.all(leaves32[k].grad[:, 3, :] == 0)
                r = float((err.reshape(J, -1).abs().amax(1) / bar).max())
            else:
                r = ratio(err, rowbar)
            worst = max(worst, r)
    print(f"\nbackward P={P} J={J}: worst error / bar {worst:.3g}")
    assert worst < 1.0


def _golden_model(g, dev):
    from moss_amd.knn_cuda import KNN
    body = {k: v.to(dev) for k, v in g["body"].items()}
    return SimpleNamespace(SMPL_NEUTRAL=body, knn=KNN(k=1, transpose_mode=True))


@pytest.mark.parametrize("case", ["plain", "refined"])
def test_drop_in_reproduces_reference_golden(gpu, hip_lib, case):
    """moss_amd.lbs.coarse_deform_c2source on the GPU reproduces the reference's float32 outputs and gradients (query_pts,
    lbs_weights, correct_Rs) of tests/golden/lbs_deform.npz, within twice the bar of tests/test_lbs_cpu.py (two float32 computations)."""
    from tests.golden import make_golden_lbs as gold
    from tests.test_lbs_cpu import FIXTURE, chain_torch, grad_bar, output_bar
    golden = np.load(FIXTURE)
    _, _, kappa, _ = chain_torch(case, requires_grad=False)
    g = gold.golden_inputs(case, device=gpu)
    model = _golden_model(g, gpu)
    q = g["query_pts"].clone().requires_grad_(True)
    L = None if g["lbs_weights"] is None else g["lbs_weights"].clone().requires_grad_(True)
    cR = None if g["correct_Rs"] is None else g["correct_Rs"].clone().requires_grad_(True)
    out = mlbs.coarse_deform_c2source(model, q, g["params"], g["t_params"], g["t_vertices"], lbs_weights=L, correct_Rs=cR,
                                      return_transl=True)
    out = dict(zip(gold.OUTPUTS, out))
    worst = {}
    for k in gold.OUTPUTS:
        ref = golden[f"{case}_{k}"]
        got = out[k].detach().cpu().numpy()
        assert got.shape == ref.shape, k
        worst[k] = float(np.abs(got - ref).max()) / (2 * output_bar(ref, kappa))
    loss = sum((out[k] * g["cotangents"][k]).sum() for k in gold.COTANGENT_OF)
    leaves = {"query_pts": q, "lbs_weights": L, "correct_Rs": cR}
    leaves = {k: v for k, v in leaves.items() if v is not None}
    grads = torch.autograd.grad(loss, list(leaves.values()))
    for name, gr in zip(leaves, grads):
        ref = golden[f"{case}_grad_{name}"]
        worst["grad_" + name] = float(np.abs(gr.cpu().numpy() - ref).max()) / (2 * grad_bar(ref, kappa))
    print(f"\n{case}: GPU drop-in vs reference float32, fraction of the bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) < 1.0, worst
    assert mlbs.coarse_deform_c2source(model, q.detach(), g["params"], g["t_params"], g["t_vertices"])[4] is None


def _run_all(c32, leaves, gT, gt, gp):
    for v in leaves.values():
        v.grad = None
    T, t, p, w = mlbs.lbs_deform(c32["ids"], c32["W"], leaves["L"], c32["A_big"], leaves["A_obs"], leaves["d"], c32["R"], c32["Th"],
                                 x=leaves["x"], want_weights=True)
    torch.autograd.backward([T, t, p], [gT, gt, gp])
    return [T.detach(), t.detach(), p.detach(), w] + [leaves[k].grad for k in ("L", "A_obs", "d", "x")]


def _leaves(c):
    return {k: c[k].float().clone().requires_grad_(True) for k in ("L", "A_obs", "d", "x")}


def test_deterministic(gpu, hip_lib):
    """Two calls on the same inputs: bit-identical T, t, p, w, gL, gA_obs, gd, gx (no atomics; fixed reduction order)."""
    P, J = 100000, 24
    c = make_case(P, J, 7, gpu)
    c32 = f32(c)
    gT, gt, gp = (torch.randn(P, *s, device=gpu) for s in ((3, 3), (3,), (3,)))
    leaves = _leaves(c)
    a = [v.clone() for v in _run_all(c32, leaves, gT, gt, gp)]
    b = _run_all(c32, leaves, gT, gt, gp)
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), i


def test_no_host_sync(gpu, hip_lib):
    """One eager forward + backward runs clean under torch.cuda.set_sync_debug_mode("error")."""
    P, J = 6890, 24
    c = make_case(P, J, 8, gpu)
    c32 = f32(c)
    gT, gt, gp = (torch.randn(P, *s, device=gpu) for s in ((3, 3), (3,), (3,)))
    leaves = _leaves(c)
    _run_all(c32, leaves, gT, gt, gp)                  # (allocator warm-up outside the checked window)
    torch.cuda.synchronize(gpu)
    torch.cuda.set_sync_debug_mode("error")
    try:
        _run_all(c32, leaves, gT, gt, gp)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize(gpu)


def test_op_captured_replays_new_frames(gpu, hip_lib):
    """forward + backward of lbs_deform captured once, replayed over four frames whose A_obs, L, d and R are copied into the static
    inputs: every replay is bit-identical to the eager call on that frame (outputs, gL, gA_obs, gd, gx)."""
    from moss_amd.graphs import GraphedStep
    P, J = 45695, 24
    frames = [make_case(P, J, 300 + k, gpu) for k in range(4)]
    c32 = f32(frames[0])
    leaves = _leaves(frames[0])
    gT, gt, gp = (torch.randn(P, *s, device=gpu) for s in ((3, 3), (3,), (3,)))

    def load(k):
        with torch.no_grad():
            for name in ("L", "A_obs", "d", "x"):
                leaves[name].copy_(frames[k][name])
            for name in ("R", "Th", "A_big"):
                c32[name].copy_(frames[k][name])

    def fn():
        return [v.detach() for v in _run_all(c32, leaves, gT, gt, gp)]

    step = GraphedStep(fn, warmup=2)
    for k in range(4):
        load(k)
        got = [v.clone() for v in step()]
        torch.cuda.synchronize(gpu)
        ref = fn()
        for i, (u, v) in enumerate(zip(got, ref)):
            assert torch.equal(u, v), (k, i)
        if k > 0:
            assert not torch.equal(got[0], first)
        else:
            first = got[0]


def _scene(gpu, P=6890):
    from moss_amd import scenes
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import camera_view
    from moss_amd.knn_cuda import KNN
    s = scenes.config2()
    calls = []

    class DeformableSet(GaussianSet):
        """GaussianSet + what MOSS's GaussianModel gives the LBS branch: SMPL_NEUTRAL, knn and a torch coarse_deform_c2source."""

        def coarse_deform_c2source(self, query_pts, params, t_params, t_vertices, lbs_weights=None, correct_Rs=None, return_transl=False):
            calls.append(1)
            body = self.SMPL_NEUTRAL
            _, ids = self.knn(t_vertices.float(), query_pts.float())
            ids = ids.reshape(-1)
            A_big = mlbs.smpl_joint_transforms(body, t_params)[0][0]
            rot = mlbs.batch_rodrigues(params["poses"].reshape(-1, 3))
            A_obs, R, Th = mlbs.smpl_joint_transforms(body, params, rot_mats=rot)
            D = mlbs.vertex_offsets(body, params, t_params, rot)
            R, Th = R.reshape(3, 3), Th.reshape(3)
            T, t, p, w = mlbs.deform_torch(ids, body["weights"], None, A_big, A_obs[0], D[ids], R, Th, x=query_pts[0])
            return ((p - Th) @ R)[None], p[None], w[None], T[None], (t[None] if return_transl else None)

    pc = DeformableSet(s, device=gpu)
    V = 256
    body = mlbs.synthetic_body_model(V, 24, seed=21, device=gpu)
    pc.SMPL_NEUTRAL = body
    pc.knn = KNN(k=1, transpose_mode=True)
    cam = camera_view(s.camera, gpu)
    cam.big_pose_smpl_param = {k: v.to(gpu) for k, v in mlbs.synthetic_frame(0, 24, big_pose=True).items()}
    cam.big_pose_world_vertex = body["v_template"].clone()
    cam.smpl_param = {k: v.to(gpu) for k, v in _small_frame(0).items()}
    return s, pc, cam, calls


def _small_frame(k):
    """A frame that keeps the body in view: small joint rotations, R a small rotation, Th small."""
    g = torch.Generator().manual_seed(500 + k)
    axis = torch.randn(1, 3, generator=g)
    return {"poses": 0.15 * torch.randn(1, 72, generator=g), "shapes": 0.3 * torch.randn(1, 10, generator=g),
            "R": mlbs.batch_rodrigues(0.3 * axis / axis.norm())[0], "Th": 0.05 * torch.randn(1, 3, generator=g)}


def _pipe(**kw):
    return SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, **kw)


def test_renderer_lbs_in_op_matches_torch_path(gpu, hip_lib):
    """pipe.lbs_in_op: the image matches the flag-off path (pc.coarse_deform_c2source, the torch chain) and the position gradients
    are close; with the flag off pc.coarse_deform_c2source is what render() calls."""
    from moss_amd.gaussian_renderer import render
    s, pc, cam, calls = _scene(gpu)
    bg = torch.zeros(3, device=gpu)
    wimg = torch.rand(3, s.camera.H, s.camera.W, device=gpu)
    res = {}
    for name, pipe in (("off", _pipe()), ("on", _pipe(lbs_in_op=True)),
                       ("on_pose", _pipe(lbs_in_op=True, transforms_in_op=True, pose_in_op=True)),
                       ("off_tio", _pipe(transforms_in_op=True))):
        pc._xyz.grad = None
        n = len(calls)
        out = render(cam, pc, pipe, bg)
        (out["render"] * wimg).sum().backward()
        assert len(calls) == n + (0 if name.startswith("on") else 1), name
        res[name] = (out["render"].detach().clone(), pc._xyz.grad.clone())
    # lbs_in_op alone hands the rasterizer posed means (as the flag-off path); with transforms_in_op + pose_in_op the op also
    # transforms the covariances, as the flag-off path with transforms_in_op does
    for name, base in (("on", "off"), ("on_pose", "off_tio")):
        img, gx = res[name]
        img0, gx0 = res[base]
        assert float(img0.abs().sum()) > 0
        print(f"\n{name} vs {base}: image max {float((img - img0).abs().max()):.3g} mean {float((img - img0).abs().mean()):.3g}; "
              f"position gradient relative {float((gx - gx0).norm() / gx0.norm()):.3g}")
        assert float((img - img0).abs().max()) < 2e-3, name
        assert float((img - img0).abs().mean()) < 1e-5, name
        assert float((gx - gx0).norm() / gx0.norm()) < 1e-2, name


def test_step_with_lbs_in_op_captured_over_frames(gpu, hip_lib):
    """The frame-varying MOSS-shaped step -- render with pipe.lbs_in_op + transforms_in_op + pose_in_op (the deformation, the
    covariance transform and the pose inside the ops), the fused loss, the backward -- captured ONCE with GraphedStep and replayed
    over four frames whose pose parameters are copied into the static inputs: each replay is bit-identical to the eager step of that
    frame (image, loss, every Gaussian-parameter gradient).  Nothing in it synchronises with the host."""
    import moss_amd.diff_gaussian_rasterization as dgr
    from moss_amd.gaussian_renderer import render
    from moss_amd.graphs import GraphedStep
    from moss_amd.loss import backward_from_loss, training_loss_fused
    s, pc, cam, _ = _scene(gpu)
    pipe = _pipe(lbs_in_op=True, transforms_in_op=True, pose_in_op=True)
    bg = torch.zeros(3, device=gpu)
    gt_img = torch.rand(3, s.camera.H, s.camera.W, device=gpu)
    gt_mask = (torch.rand(1, s.camera.H, s.camera.W, device=gpu) > 0.5).float()
    params = list(pc.parameters())
    grads = [torch.zeros_like(p) for p in params]

    def fn():
        for p, g in zip(params, grads):
            g.zero_()
            p.grad = g
        out = render(cam, pc, pipe, bg)
        loss = training_loss_fused(out["render"], out["render_alpha"], gt_img, gt_mask)
        backward_from_loss(loss)
        return out["render"].detach(), loss.detach()

    def load(k):
        for key, v in _small_frame(k).items():
            cam.smpl_param[key].copy_(v)

    ctx = dgr.RasterContext()                                 # a context of its own: its buffers go with the test
    pipe.raster_context = ctx
    ctx.set_async(True)
    try:
        fn()                                                    # synchronous first forward: learns the capacity
        step = GraphedStep(fn, warmup=3, context=ctx)
        first = None
        for k in range(4):
            load(k)
            img_g, loss_g = (v.clone() for v in step())
            grads_g = [g.clone() for g in grads]
            torch.cuda.synchronize(gpu)
            img_e, loss_e = (v.clone() for v in fn())
            torch.cuda.synchronize(gpu)
            assert torch.equal(img_g, img_e), k
            assert torch.equal(loss_g, loss_e), k
            for i, (a, b) in enumerate(zip(grads_g, grads)):
                assert torch.equal(a, b), (k, i)
            if first is None:
                first = img_g
            else:
                assert not torch.equal(img_g, first)
        dgr.check_async_status(context=ctx)
    finally:
        ctx.set_async(False)
        step = None


def test_edges(gpu, hip_lib):
    """P = 0; out-of-range ids give NaN rows and nothing else; J > 64, non-contiguous inputs, wrong dtypes or devices and constants
    that require grad are refused."""
    c = f32(make_case(200, 24, 9, gpu))
    args = lambda **kw: {**{k: c[k] for k in ("W", "A_big", "A_obs", "R", "Th")}, **kw}   # noqa: E731
    # P = 0
    e = torch.zeros(0, dtype=torch.int64, device=gpu)
    A_obs = c["A_obs"].clone().requires_grad_(True)
    T, t, p, w = mlbs.lbs_deform(e, c["W"], None, c["A_big"], A_obs, torch.zeros(0, 3, device=gpu), c["R"], c["Th"],
                                 x=torch.zeros(0, 3, device=gpu), want_weights=True)
    assert T.shape == (0, 3, 3) and t.shape == (0, 3) and p.shape == (0, 3) and w.shape == (0, 24)
    (T.sum() + t.sum()).backward()
    assert torch.equal(A_obs.grad, torch.zeros_like(A_obs))
    # out-of-range ids
    ids = c["ids"].clone()
    bad = torch.tensor([0, 17, 199], device=gpu)
    ids[bad] = torch.tensor([-1, 256, 1 << 40], device=gpu)
    L = c["L"].clone().requires_grad_(True)
    A_obs = c["A_obs"].clone().requires_grad_(True)
    T, t, p, w = mlbs.lbs_deform(ids, c["W"], L, c["A_big"], A_obs, c["d"], c["R"], c["Th"], x=c["x"], want_weights=True)
    ok = torch.ones(200, dtype=torch.bool, device=gpu)
    ok[bad] = False
    for o in (T.reshape(200, -1), t, p, w):
        assert torch.isnan(o[bad]).all() and torch.isfinite(o[ok]).all()
    (T.sum() + t.sum() + p.sum()).backward()
    assert torch.isnan(L.grad[bad]).all() and torch.isfinite(L.grad[ok]).all()
    assert torch.isfinite(A_obs.grad).all()
    keep = ids.clone()
    keep[bad] = 0
    A2 = c["A_obs"].clone().requires_grad_(True)
    T2, t2, p2, _ = mlbs.lbs_deform(keep, c["W"], L.detach(), c["A_big"], A2, c["d"], c["R"], c["Th"], x=c["x"])
    torch.testing.assert_close(T2[ok], T[ok], rtol=0, atol=0)
    # refusals
    base = dict(vert_ids=c["ids"], lbs_offsets=c["L"], d=c["d"], x=c["x"])
    with pytest.raises(ValueError, match="1..64"):
        W65 = torch.rand(256, 65, device=gpu)
        mlbs.lbs_deform(c["ids"], W65, None, torch.eye(4, device=gpu).repeat(65, 1, 1), torch.eye(4, device=gpu).repeat(65, 1, 1),
                        c["d"], c["R"], c["Th"])
    with pytest.raises(ValueError, match="contiguous"):
        mlbs.lbs_deform(**args(**{**base, "d": torch.zeros(3, 200, device=gpu).t()}))
    with pytest.raises(ValueError, match="float32"):
        mlbs.lbs_deform(**args(**{**base, "d": c["d"].double()}))
    with pytest.raises(ValueError, match="int64"):
        mlbs.lbs_deform(**args(**{**base, "vert_ids": c["ids"].int()}))
    with pytest.raises(ValueError, match="must be on"):
        mlbs.lbs_deform(**args(**{**base, "d": c["d"].cpu()}))
    for name in ("W", "A_big", "R", "Th"):
        kw = args(**base)
        kw[name] = kw[name].clone().requires_grad_(True)
        with pytest.raises(ValueError, match="requires grad"):
            mlbs.lbs_deform(**kw)
    # the C ABI itself refuses a bad J with a message
    from moss_amd._lib import LbsForwardArgs, lib
    import ctypes
    a = LbsForwardArgs()
    a.P, a.J, a.V = 1, 65, 1
    assert lib().moss_lbs_deform_forward(ctypes.byref(a), None) == -1
    assert b"J must be 1..64" in lib().moss_last_error()
    a.J = 24
    assert lib().moss_lbs_deform_forward(ctypes.byref(a), None) == -1
    assert b"null" in lib().moss_last_error()
    assert lib().moss_lbs_workspace_bytes(0, 24) == 0 and lib().moss_lbs_workspace_bytes(129, 24) >= 2 * 24 * 12 * 4
