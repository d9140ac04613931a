"""CPU-only tests of the host side: the C-ABI library loads and exports every declared symbol (no compute without a GPU),
the op fails loudly instead of falling back, the Python surface validates arguments like the reference, scene generators
are deterministic, and the frame-parallel gradient exchange is correct under a 2-process gloo group."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from moss_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(moss_[a-z0-9_]+)\s*\(", text)) - {"moss_alloc_fn"}


def test_library_exports_exactly_the_declared_symbols(hip_lib):
    """The PRODUCT library exports everything the header declares outside its ``#ifdef MOSS_DIAG`` block -- and nothing of that block
    (diagnostics do not ship) -- and, the other way round, every ``moss_*`` symbol it exports is declared there (no
    stale entry point left behind when one is removed from the ABI)."""
    import subprocess
    from moss_amd import _lib
    text = open(os.path.join(ROOT, "include", "moss_raster.h")).read()
    diag_block = re.search(r"#ifdef MOSS_DIAG\n(.*?)#endif", text, flags=re.S)
    assert diag_block
    diag_names = _declared(diag_block.group(1))
    names = _declared(text.replace(diag_block.group(0), ""))
    assert len(names) >= 15 and diag_names == {"moss_raster_debug_set_stamps", "moss_raster_debug_set_bwd_stamps"}
    for n in sorted(names):
        assert hasattr(hip_lib, n), f"{n} is declared in include/moss_raster.h but not exported"
    for n in sorted(diag_names):
        assert not hasattr(hip_lib, n), f"{n} is a diagnostic entry point and must not be in the product build"
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\s(moss_[A-Za-z0-9_]+)$", syms, flags=re.M))
    assert len(exported) >= 15 and exported <= names, f"exported but not declared in include/moss_raster.h: {sorted(exported - names)}"
    assert hip_lib.moss_build_has_diagnostics() == 0
    assert re.search(r"#define\s+MOSS_ABI_VERSION\s+7\b", text) and hip_lib.moss_abi_version() == 7
    assert hip_lib.moss_last_error() == b""
    assert hip_lib.moss_adamw_state_bytes() == int(re.search(r"#define\s+MOSS_ADAMW_STATE_BYTES\s+(\d+)", text).group(1))


def test_product_build_reads_no_environment_variable():
    """No translation unit under moss_amd/csrc/ mentions getenv, and the built product library does not import it (the knobs of the
    A/B scripts exist only in the -DMOSS_DIAG build, whose getenv lives in scripts/diag/knobs.cpp)."""
    import subprocess
    for f in os.listdir(os.path.join(ROOT, "moss_amd", "csrc")):
        assert "getenv" not in open(os.path.join(ROOT, "moss_amd", "csrc", f)).read(), f
    from moss_amd import _lib
    syms = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert syms and "getenv" not in syms


def test_extension_reports_its_compile_time_abi_version(monkeypatch):
    """`_moss_C.abi_version()` used to call the library, so `_lib.ext()` compared the library with itself.  It now returns
    the MOSS_ABI_VERSION of the header the extension was COMPILED against, and a library of another version refuses to load."""
    from moss_amd import _lib
    src = open(os.path.join(ROOT, "moss_amd", "csrc", "torch_binding.cpp")).read()
    assert re.search(r'm\.def\("abi_version",\s*\[\]\(\)\s*\{\s*return\s*\(int\)MOSS_ABI_VERSION;', src)
    assert _lib.ext().abi_version() == _lib.ABI_VERSION == _lib.lib().moss_abi_version()
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "ABI_VERSION", 1)
    with pytest.raises(ImportError, match="ABI version"):
        _lib.lib()


def test_frame_state_blocks_are_never_freed_by_a_context():
    """a RasterContext must keep every frame-state block it has handed out (a captured hipGraph holds its address)."""
    from moss_amd.diff_gaussian_rasterization import RasterContext
    cx = RasterContext()
    dev = torch.device("cpu")                              # (allocation policy only: no kernel runs)
    a = cx._frame_state(dev, 512, 512)
    assert cx._frame_state(dev, 256, 256) is a             # a smaller image is served by the same block
    b = cx._frame_state(dev, 2048, 2048)                   # a larger one by a new block ...
    assert b is not a and any(t is a for t in cx._retired_frame_states)      # ... while the old one stays alive
    assert cx._frame_state(dev, 512, 512) is b
    assert int(a.count_nonzero()) == 0 and int(b.count_nonzero()) == 0


def test_reorder_spatially_moves_torch_optimizer_state_too():
    """with a torch.optim optimizer the moments must be permuted with the parameters; an unknown optimizer type raises."""
    from moss_amd.gaussian_model import GaussianSet
    s = scenes.config1()
    pc = GaussianSet(s, device="cpu")
    opt = torch.optim.AdamW(pc.param_groups(), lr=0.0, eps=1e-15)
    for p in pc.parameters():
        p.grad = torch.arange(p.numel(), dtype=torch.float32).reshape(p.shape) / p.numel()
    opt.step()
    before = {id(p): (p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in pc.parameters()}
    perm = pc.reorder_spatially(opt)
    assert sorted(perm.tolist()) == list(range(s.P)) and not torch.equal(perm, torch.arange(s.P))
    for p in pc.parameters():
        p0, m0, v0 = before[id(p)]
        assert torch.equal(p.detach(), p0[perm]) and torch.equal(opt.state[p]["exp_avg"], m0[perm]) and torch.equal(opt.state[p]["exp_avg_sq"], v0[perm])
    with pytest.raises(TypeError, match="cannot permute the state"):
        pc.reorder_spatially(object())


def test_scratch_size_functions_are_host_only_and_monotonic(hip_lib):
    g = [hip_lib.moss_raster_geometry_bytes(p) for p in (1, 1000, 100000)]
    assert g[0] < g[1] < g[2] and g[2] < 100000 * 120           # ~ 100 B per Gaussian
    b = [hip_lib.moss_raster_binning_bytes(r) for r in (0, 1000, 1000000)]
    assert b[0] <= b[1] < b[2]
    # the binning buffer: ~66 B of per-instance tables + a record pool of 6 cells x 48 B per instance (rounds 1-4: 16 slabs, 834 B)
    assert b[2] <= 400 * 1000000 and b[0] < (16 << 20)              # (the constant: the blend kernels' segment queues)
    assert hip_lib.moss_raster_image_bytes(512, 512) >= 512 * 512 * 8
    assert hip_lib.moss_knn_workspace_bytes(6890) >= 6890 * 24
    assert hip_lib.moss_loss_workspace_bytes(3, 512, 512) >= 3 * 3 * 512 * 512 * 4


def test_refused_loss_calls_say_which_entry_point_and_why(hip_lib):
    """Every refusal of the three photometric-loss entry points sets the text of moss_last_error(): it names the entry point, and it
    is not what an earlier refused call of another op left behind.  All of these calls are refused before anything is dereferenced
    or launched (the non-null pointers are dummy addresses)."""
    INVALID = -1                                               # MOSS_ERR_INVALID_ARG
    p = 0x1000                                                 # a pointer that only has to be non-null
    C, H, W = 3, 64, 48
    need = hip_lib.moss_loss_workspace_bytes(C, H, W)

    def plain(C=C, image=p, alpha=p, mask=p, nbytes=need):
        return hip_lib.moss_photometric_loss(C, H, W, image, p, alpha, mask, 0.2, 0.5, p, p, p, p, nbytes, None)

    def weighted(C=C, image=p, alpha=p, mask=p, nbytes=need):
        return hip_lib.moss_photometric_loss_weighted(C, H, W, image, p, alpha, mask, 1.0, 0.2, 0.5, p, p, p, p, nbytes, None)

    def roi(C=C, image=p, alpha=p, mask=p, nbytes=need, rect=p):
        return hip_lib.moss_photometric_loss_roi(C, H, W, image, p, alpha, mask, p, rect, 1.0, 0.2, 0.5, p, p, p, p, nbytes, None)

    refusals = [dict(C=0), dict(image=None), dict(mask=None), dict(nbytes=need - 1)]
    for name, fn, cases in (("moss_photometric_loss", plain, refusals), ("moss_photometric_loss_weighted", weighted, refusals),
                            ("moss_photometric_loss_roi", roi, refusals + [dict(rect=None)])):
        texts = []
        for kw in cases:
            assert hip_lib.moss_s3im_loss(0, H, W, p, p, None, 10, p, p, p, 0, None) == INVALID      # refused at its first check
            sentinel = hip_lib.moss_last_error()
            assert b"moss_s3im_loss" in sentinel
            assert fn(**kw) == INVALID, (name, kw)
            text = hip_lib.moss_last_error()
            assert text != sentinel and text.split(b":")[0] == name.encode(), (name, kw, text)
            texts.append(text)
        assert len(set(texts)) == len(texts), texts           # a text per condition


def test_missing_library_is_an_import_error_not_a_fallback(monkeypatch):
    from moss_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libmoss_raster.so")
    with pytest.raises(ImportError, match="no CPU/PyTorch fallback"):
        _lib.lib()


def test_no_product_module_imports_the_oracle():
    """The oracle is test infrastructure: nothing under moss_amd/ (nor the root alias packages) may import it."""
    for base in ("moss_amd", "diff_gaussian_rasterization", "simple_knn"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith(".py"):
                    src = open(os.path.join(dirpath, f)).read()
                    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), os.path.join(dirpath, f)
    for dirpath, _, files in os.walk(os.path.join(ROOT, "moss_amd", "csrc")):
        for f in files:
            assert "#include \"../../oracle" not in open(os.path.join(dirpath, f)).read()


def test_python_surface_validation_without_gpu(hip_lib):
    import diff_gaussian_rasterization as dgr                      # the root alias MOSS imports
    from moss_amd.diff_gaussian_rasterization import GaussianRasterizer as GR2
    assert dgr.GaussianRasterizer is GR2
    assert dgr.GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "sh_degree", "campos", "prefiltered", "debug")
    s = scenes.config1(); c = s.camera
    rs = dgr.GaussianRasterizationSettings(c.H, c.W, c.tanfovx, c.tanfovy, s.bg, 1.0, c.viewmatrix, c.projmatrix, 3, c.campos,
                                           False, False)
    r = dgr.GaussianRasterizer(rs)
    m2 = torch.zeros_like(s.means3D)
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(s.means3D, m2, s.opacities, shs=s.shs, colors_precomp=torch.rand(256, 3), scales=s.scales, rotations=s.rotations)
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(s.means3D, m2, s.opacities, shs=s.shs)
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(s.means3D, m2, s.opacities, shs=s.shs, scales=s.scales)          # rotations missing
    # CPU tensors are refused loudly (the reference would dereference host pointers on the device)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r(s.means3D, m2, s.opacities, shs=s.shs, scales=s.scales, rotations=s.rotations)
    from simple_knn._C import distCUDA2
    with pytest.raises(RuntimeError, match="no CPU path"):
        distCUDA2(s.means3D)


def test_cpu_deep_copy_tuple():
    from moss_amd.diff_gaussian_rasterization import cpu_deep_copy_tuple
    t = torch.arange(4.0)
    out = cpu_deep_copy_tuple((t, 3, "x"))
    assert out[1:] == (3, "x") and torch.equal(out[0], t) and out[0].data_ptr() != t.data_ptr()


def test_scene_generators_are_deterministic():
    a, b = scenes.config2(), scenes.config2()
    assert torch.equal(a.means3D, b.means3D) and torch.equal(a.scales, b.scales) and torch.equal(a.shs, b.shs)
    assert a.means3D.shape == (6890, 3) and a.camera.W == 512
    ring = scenes.look_at_ring(8)
    R0, t0 = ring[0]
    np.testing.assert_allclose(R0, np.eye(3), atol=1e-12); np.testing.assert_allclose(t0, [0, 0, 3.0], atol=1e-12)
    for R, t in ring:
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
        assert abs(np.linalg.det(R) - 1) < 1e-12
        np.testing.assert_allclose(np.linalg.norm(-R.T @ t), 3.0, atol=1e-12)       # camera centre on the ring


def test_spatial_order_is_a_permutation_along_a_curve():
    """densify.spatial_order (pure torch, any device): a permutation of the indices; consecutive Gaussians of the re-indexed set are
    close in space (a Morton curve), which is all the rasterizer's memory traffic asks of it; deterministic; degenerate inputs
    (all points equal, a single point) do not divide by zero."""
    from moss_amd.densify import spatial_order
    s = scenes.config2()
    x = s.means3D
    perm = spatial_order(x)
    assert perm.dtype == torch.int64 and sorted(perm.tolist()) == list(range(x.shape[0]))
    assert torch.equal(perm, spatial_order(x))
    step = lambda y: float((y[1:] - y[:-1]).norm(dim=1).mean())
    assert step(x[perm]) < 0.25 * step(x)                      # the generator's own order is uncorrelated with position
    assert sorted(spatial_order(torch.zeros(5, 3)).tolist()) == [0, 1, 2, 3, 4]
    assert spatial_order(torch.tensor([[1.0, 2.0, 3.0]])).tolist() == [0]


def test_header_declares_the_spatial_order_hint():
    """MOSS_HINT_SPATIAL_ORDER of include/moss_raster.h and its Python mirror are the same bit, distinct from the raw-parameter bits."""
    from moss_amd.diff_gaussian_rasterization import _C
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "moss_raster.h")).read()
    m = re.search(r"#define\s+MOSS_HINT_SPATIAL_ORDER\s+(\d+)", text)
    assert m and int(m.group(1)) == _C.HINT_SPATIAL_ORDER == 8
    assert _C.HINT_SPATIAL_ORDER & (_C.RAW_OPACITY | _C.RAW_SCALE | _C.RAW_ROTATION) == 0


def test_shard_views():
    from moss_amd.dist import shard_views
    parts = [shard_views(10, r, 4) for r in range(4)]
    assert sorted(sum(parts, [])) == list(range(10)) and parts[1] == [1, 5, 9]


def test_bucket_shard_layout():
    """GradBucket(params, world): equal 4-aligned shards that cover gradients + loss block; the loss block never straddles two."""
    from moss_amd.dist import GradBucket, shard_layout
    for sizes, world in (((5, 3), 2), ((1001, 7, 16), 8), ((100000 * 59,), 8), ((3,), 4)):
        params = [torch.nn.Parameter(torch.zeros(n)) for n in sizes]
        b = GradBucket(params, world=world)
        per, padded = shard_layout(b.n_exchange, world)
        assert b.shard_len == per and b.flat.numel() == padded == per * world and per % 4 == 0
        assert b.tail % 4 == 0 and b.tail >= sum(sizes) and b.tail // per == (b.tail + 3) // per
        assert b.loss_terms.data_ptr() == b.flat[b.tail:].data_ptr()
    b1 = GradBucket([torch.nn.Parameter(torch.zeros(10))])
    assert b1.flat.numel() == 12 + 4 and b1.world == 1


def _rank_main(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from moss_amd import dist as mdist
    r, w, _ = mdist.init_from_env(backend="gloo")
    assert (r, w) == (rank, world)
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.zeros(5, 3)), torch.nn.Parameter(torch.zeros(7))]
    bucket = mdist.GradBucket(params)
    bucket.attach()
    # each rank produces a different "view" gradient through autograd, accumulating straight into the bucket
    loss = ((params[0] + 1.0) * (rank + 1)).sum() + (params[1] * float(10 * (rank + 1))).sum()
    loss.backward()
    assert params[0].grad.data_ptr() == bucket.views[0].data_ptr()          # no pack copy
    got_loss = bucket.all_reduce_mean(loss, world).clone()
    # numpy, not tensors: a tensor crosses a multiprocessing queue as a file descriptor served by THIS process, which may have
    # exited by the time the parent unpickles it
    q.put((rank, params[0].grad.numpy().copy(), params[1].grad.numpy().copy(), got_loss.numpy().copy()))
    dist.barrier()
    dist.destroy_process_group()


def test_frame_parallel_gradient_bucket_gloo_world2():
    """N>1 path on CPU: two processes, gloo backend, ONE all-reduce of the flat bucket averages every gradient and the loss."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, g0, g1, loss in res:
        g0, g1, loss = torch.from_numpy(g0), torch.from_numpy(g1), torch.from_numpy(loss)
        assert torch.allclose(g0, torch.full((5, 3), 1.5))                  # mean of 1 and 2
        assert torch.allclose(g1, torch.full((7,), 15.0))                   # mean of 10 and 20
        assert torch.allclose(loss, torch.tensor([(15.0 + 30.0) / 2]))      # mean of the two ranks' losses


class _TorchAdamWShard:
    """torch restatement of FlatAdamW(shard=...) for the CPU test of the exchange (the HIP kernel needs a GPU): AdamW on
    flat_params[first : first + count] with the gradients in grad_shard."""
    def __init__(self, bucket, params0, rank, lr=0.01, betas=(0.9, 0.999), eps=1e-15, wd=0.01):
        per = bucket.shard_len
        self.flat_params = torch.zeros(bucket.flat.numel())
        self.flat_params[:bucket.n_params] = params0
        self.grad_shard = torch.zeros(per)
        self.first = min(rank * per, bucket.n_params)
        self.count = min(self.first + per, bucket.n_params) - self.first
        self.m, self.v, self.t = torch.zeros(self.count), torch.zeros(self.count), 0
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, wd

    def step(self):
        self.t += 1
        _adamw_update(self.flat_params[self.first:self.first + self.count], self.grad_shard[:self.count], self.m, self.v, self.t,
                      self.lr, self.betas, self.eps, self.wd)


def _adamw_update(p, g, m, v, t, lr, betas, eps, wd):
    p.mul_(1 - lr * wd)
    m.mul_(betas[0]).add_(g, alpha=1 - betas[0]); v.mul_(betas[1]).addcmul_(g, g, value=1 - betas[1])
    p.addcdiv_(m / (1 - betas[0] ** t), (v.sqrt() / (1 - betas[1] ** t) ** 0.5).add_(eps), value=-lr)


def _exchange_rank_main(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from moss_amd import dist as mdist
    mdist.init_from_env(backend="gloo")
    g = torch.Generator().manual_seed(5)
    shapes = [(37, 3), (37, 16, 3), (37, 1)]                                  # 111 + 1776 + 37 parameters, every tensor 16-byte aligned: 1925 floats (+ pad + the 4-float loss block = 1932): two shards of 968
    init = [torch.randn(s, generator=g) for s in shapes]
    out = {}
    for kind in ("allreduce", "sharded"):
        params = [torch.nn.Parameter(x.clone()) for x in init]
        bucket = mdist.GradBucket(params, world=world if kind == "sharded" else 1)
        n = bucket.n_params
        p0 = bucket.pack(init)                                # (every tensor 16-byte aligned in the flat buffers)
        if kind == "sharded":
            opt = _TorchAdamWShard(bucket, p0, rank)
            ex = mdist.ShardedStep(bucket, opt, rank, world)
        else:
            flat, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
        gr = torch.Generator().manual_seed(100 + rank)                        # every rank its own "view"
        for t in range(1, 4):
            bucket.flat[:n] = torch.randn(n, generator=gr)
            bucket.loss_terms[:] = torch.tensor([1.0, 2.0, 3.0, 4.0]) * (rank + 1) * t
            if kind == "sharded":
                loss = ex.step()
                terms = ex.loss_terms.clone()
            else:
                loss = bucket.all_reduce_mean(None, world)
                terms = bucket.loss_terms.clone()
                _adamw_update(flat, bucket.flat[:n], m, v, t, 0.01, (0.9, 0.999), 1e-15, 0.01)
            assert torch.allclose(terms, torch.tensor([1.0, 2.0, 3.0, 4.0]) * t * (world + 1) / 2) and float(loss) == float(terms[0])
        out[kind] = (opt.flat_params[:n] if kind == "sharded" else flat).numpy().copy()
        if kind == "sharded":
            assert opt.count == (968 if rank == 0 else 957) and opt.m.numel() == opt.count     # ceil(1932 / 2) rounded up to 4 = 968 per shard, 1925 of them parameters; moments for the shard only
    q.put((rank, out["allreduce"], out["sharded"]))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_optimizer_exchange_equals_allreduce_gloo_world2():
    """reduce-scatter -> AdamW on the rank's shard -> all-gather (moss_amd.dist.ShardedStep) leaves the SAME
    parameters on every rank as all-reduce -> full AdamW, and both replicas agree; the averaged loss block reaches every rank."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_exchange_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(2)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, a0, s0), (_, a1, s1) = res
    assert np.array_equal(a0, a1) and np.array_equal(s0, s1)                  # replicas identical, either path
    np.testing.assert_allclose(s0, a0, rtol=0, atol=1e-7)                     # and the two paths agree
    assert np.abs(a0).max() > 0.1


def _loss_only_rank_main(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from moss_amd import dist as mdist
    mdist.init_from_env(backend="gloo")
    params = [torch.nn.Parameter(torch.zeros(37, 3)), torch.nn.Parameter(torch.zeros(37, 16, 3))]
    bucket = mdist.GradBucket(params)
    n = bucket.n_params
    bucket.flat[:n] = float(rank + 1)                                          # this rank's own gradients
    bucket.loss_terms[:] = torch.tensor([1.0, 2.0, 3.0, 4.0]) * (rank + 1)
    loss = bucket.all_reduce_loss_only(world)
    q.put((rank, bucket.flat[:n].numpy().copy(), bucket.loss_terms.numpy().copy(), float(loss)))
    dist.barrier()
    dist.destroy_process_group()


def test_loss_only_exchange_gloo_world2():
    """BASELINE configs[3] as written ("frames sharded across the GPUs, RCCL loss all-reduce"): every rank keeps its own model and
    gradients; only the 4-float loss block is averaged over the ranks (GradBucket.all_reduce_loss_only, bench.py --exchange loss_only)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_loss_only_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(2)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, grads, terms, loss in res:
        assert np.all(grads == float(rank + 1))                                # the gradients never travelled
        np.testing.assert_allclose(terms, np.array([1.0, 2.0, 3.0, 4.0]) * 1.5) and loss == 1.5


def _stats_rank_main(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from moss_amd import dist as mdist
    from moss_amd.densify import DensifyStats
    mdist.init_from_env(backend="gloo")
    stats = DensifyStats(6, device="cpu")
    # what two steps of moss_densify_stats would have left on this rank (the kernel itself needs a GPU)
    stats.xyz_gradient_accum[:, 0] = torch.tensor([1.0, 0.0, 2.0, 0.0, 0.5, 0.0]) * (rank + 1)
    stats.denom[:, 0] = torch.tensor([2.0, 0.0, 1.0, 0.0, 1.0, 0.0]) + rank
    stats.max_radii2D[:] = torch.tensor([3.0, 0.0, 9.0, 0.0, 1.0, 0.0]) if rank == 0 else torch.tensor([4.0, 7.0, 2.0, 0.0, 1.0, 0.0])
    stats.sync()
    q.put((rank, stats.xyz_gradient_accum.numpy().copy(), stats.denom.numpy().copy(), stats.max_radii2D.numpy().copy(), stats.mean_grads().numpy().copy()))
    dist.barrier()
    dist.destroy_process_group()


def test_densification_statistics_sync_gloo_world2():
    """Frame-parallel replicas must take the same densification decision: sum / sum / max of the per-rank statistics."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_stats_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, acc, den, mr, mean in res:
        acc, den, mr, mean = (torch.from_numpy(x) for x in (acc, den, mr, mean))
        assert torch.equal(acc[:, 0], torch.tensor([3.0, 0.0, 6.0, 0.0, 1.5, 0.0]))
        assert torch.equal(den[:, 0], torch.tensor([5.0, 1.0, 3.0, 1.0, 3.0, 1.0]))
        assert torch.equal(mr, torch.tensor([4.0, 7.0, 9.0, 0.0, 1.0, 0.0]))
        assert torch.equal(mean[:, 0], torch.tensor([0.6, 0.0, 2.0, 0.0, 0.5, 0.0]))


def test_densify_ops_refuse_cpu_tensors(hip_lib):
    from moss_amd.densify import DensifyStats, neighbour_kl
    from knn_cuda import KnnGrid
    s = DensifyStats(4, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        s.add(torch.ones(4, dtype=torch.int32), torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        neighbour_kl(torch.zeros(4, 3), torch.ones(4, 4), torch.ones(4, 3), torch.zeros(4, 2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        KnnGrid(torch.zeros(4, 3))
    assert hip_lib.moss_knn_grid_workspace_bytes(100000) > 100000 * 24
    assert hip_lib.moss_knn_grid_build(0, None, None, 0, None) != 0          # argument validation happens before any launch
    assert hip_lib.moss_neighbour_kl(-1, 0, None, None, None, None, None, None) != 0


def _run_bench_dry(extra, timeout=300):
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["MOSS_DIST_BACKEND"] = "gloo"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "1"] + list(extra),
                       env=env, capture_output=True, text=True, timeout=timeout)
    return p, [ln for ln in p.stdout.splitlines() if ln.strip()], json


def test_bench_starts_its_own_ranks_and_reports_the_collective(tmp_path):
    """`python bench.py --gpus 2` WITHOUT a torchrun environment must start two ranks itself (it used to run one GPU
    silently and print n_gpus: 1), relay rank 0's single JSON line, and carry rccl_ranks / allreduce_ms / adamw_ms /
    replicas_identical.  --dry-run-cpu swaps the GPU step for a host-side gradient bucket so the launcher, the rendezvous, the
    all-reduce (gloo) and the max-over-ranks timing run on a machine without GPUs.

    Round 5: `value` of an N > 1 line is the DATA-PARALLEL gradient all-reduce (the form that exercises
    RCCL) unless --exchange says otherwise, and every form of the step is at top level -- value_<kind>, ms_per_step_<kind>,
    replicas_identical_<kind> -- whichever one `value` is; config.parallelism says which."""
    p, lines, json = _run_bench_dry(["--dry-run-cpu", "--full"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["rccl_ranks"] == 2 and res["steps"] == 5 and res["scaling"] == "weak"
    assert res["replicas_identical"] is True and res["backend"] == "gloo"            # (of the two gradient exchanges measured beside)
    assert res["allreduce_ms"] >= 0.0 and "adamw_ms" in res and res["value"] > 0
    ev = res["exchange_variants"]
    assert set(ev) == {"allreduce", "sharded", "loss_only"}
    assert res["exchange"] == "allreduce" and res["value"] == ev["allreduce"]["value"] == res["value_allreduce"]
    assert "allreduce" in res["config"]["parallelism"]
    for kind in ("allreduce", "sharded", "loss_only"):
        assert res[f"value_{kind}"] == ev[kind]["value"] > 0 and res[f"ms_per_step_{kind}"] == ev[kind]["ms_per_step"] > 0
        assert res[f"replicas_identical_{kind}"] is ev[kind]["replicas_identical"]
    assert res["replicas_identical_allreduce"] is True and res["replicas_identical_sharded"] is True
    assert ev["allreduce"]["checksum"] == ev["sharded"]["checksum"]
    # BASELINE configs[3] as written: independent models, only the loss block travels (asserted inside the ranks: every rank kept its
    # own gradients and saw the mean loss); nothing to compare between replicas
    assert res["replicas_identical_loss_only"] is None and ev["loss_only"]["checksum"] != ev["allreduce"]["checksum"]
    # a rank that fails takes the launcher down with a non-zero exit code and no JSON line
    p, lines, _ = _run_bench_dry([])                                                 # no GPU here: every rank asserts
    assert p.returncode != 0 and not [ln for ln in lines if ln.strip().startswith("{")]


@pytest.mark.parametrize("kind", ["allreduce", "sharded", "loss_only"])
def test_bench_dry_run_every_exchange_as_the_headline(kind):
    """`bench.py --gpus 2 --dry-run-cpu --exchange <kind>` -- each of the three forms as `value`, two ranks in the
    group that ran the collectives, replicas identical for the two gradient exchanges."""
    p, lines, json = _run_bench_dry(["--dry-run-cpu", "--full", "--exchange", kind])
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(lines[-1])
    assert res["rccl_ranks"] == 2 and res["n_gpus"] == 2 and res["exchange"] == kind
    assert res["value"] == res[f"value_{kind}"] and kind in res["config"]["parallelism"]
    assert res["replicas_identical"] is True                       # over the variants that HAVE replicas (all-reduce, sharded)
    assert res[f"replicas_identical_{kind}"] is (None if kind == "loss_only" else True)


@pytest.mark.parametrize("kind", ["allreduce", "loss_only"])
def test_bench_plain_run_reports_the_headline_alone(kind):
    """Without --full a run measures its headline and nothing beside it: one exchange timed, no replica check, no other exchange's
    fields (the dry run reports as the GPU path does)."""
    p, lines, json = _run_bench_dry(["--dry-run-cpu", "--exchange", kind])
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["rccl_ranks"] == 2 and res["steps"] == 5 and res["exchange"] == kind
    assert res["value"] > 0 and res["ms_per_step"] > 0 and res["unit"] == "iters/s" and res["higher_is_better"] is True
    assert res["dtype"] == "f32" and kind in res["config"]["parallelism"]
    assert "exchange_variants" not in res and "replicas_identical" not in res
    assert not [k for k in res if k.startswith(("value_", "ms_per_step_", "replicas_identical_"))], sorted(res)


def test_bench_full_is_off_by_default_and_gates_the_side_options():
    import bench
    assert bench.parse_args([]).full is False and bench.parse_args(["--full"]).full is True
    a = bench.parse_args(["--full", "--no-callers", "--no-cpu-baseline", "--callers-only", "eval"])
    assert a.no_callers and a.no_cpu_baseline and a.callers_only == "eval"
    assert not bench.parse_args(["--no-callers", "--no-cpu-baseline"]).full      # (narrowing --full: harmless without it)
    with pytest.raises(SystemExit):
        bench.parse_args(["--callers-only", "eval"])                               # measuring callers needs --full: an error, not a no-op

def _avg_order_rank_main(rank, world, port, q):
    """Records, in program order, every collective this rank issues and every avg_supported() decision."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from moss_amd import dist as mdist
    mdist.init_from_env(backend="gloo")
    log = []
    real_all_reduce, real_avg = dist.all_reduce, mdist.avg_supported
    mdist._AVG_OK.clear()

    def all_reduce(t, *a, **k):
        log.append(("all_reduce", int(t.numel())))
        return real_all_reduce(t, *a, **k)

    def avg(device=None):
        decided_before = dist.get_backend() in mdist._AVG_OK
        r = real_avg(device)
        if not decided_before:
            log.append(("avg_decided", bool(r)))
        return r
    dist.all_reduce = all_reduce
    mdist.avg_supported = avg
    params = [torch.nn.Parameter(torch.zeros(64, 3)), torch.nn.Parameter(torch.zeros(64, 16, 3))]
    bucket = mdist.GradBucket(params)                            # <- the decision is taken HERE, on every rank alike
    after_ctor = list(log)
    bucket.flat.fill_(float(rank + 1))
    if rank == 1:
        bucket.all_reduce_loss_only(world)                       # ranks may reach their first exchange through different entry points ...
    else:
        bucket.all_reduce_loss_only(world)
    bucket.all_reduce_mean(None, world, sh_param=params[1], active_sh_degree=1)
    q.put((rank, after_ctor, log))
    dist.barrier()
    dist.destroy_process_group()


def test_avg_reduce_op_is_decided_before_the_first_data_collective_gloo_world2():
    """VERDICT r4 item 8 / ADVICE r4: whether ReduceOp.AVG is used is decided ONCE, when the bucket is built (outside any graph capture,
    at the same program point on every rank), never at the first exchange -- so no rank can take a different collective sequence from
    its peers.  Both ranks: the decision is the first entry of their logs, identical, and every data collective comes after it."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_avg_order_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, ctor0, log0), (_, ctor1, log1) = res
    assert ctor0 == ctor1 == [("avg_decided", False)]            # gloo: sum + divide; decided in the constructor, no collective yet
    assert log0 == log1                                          # the same collective sequence on both ranks
    assert [e for e in log0 if e[0] == "avg_decided"] == [("avg_decided", False)]
    assert log0[1][0] == "all_reduce" and len(log0) >= 5         # loss block, then the three pieces of the active-degree exchange


def _fuse_guard_rank_main(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from moss_amd import dist as mdist
    from moss_amd.diff_gaussian_rasterization import RasterContext
    from moss_amd.optim import FlatAdamW
    mdist.init_from_env(backend="gloo")
    P = 8
    names = ("means3D", "sh", "opacity", "scales", "rotations")
    shapes = ((P, 3), (P, 16, 3), (P, 1), (P, 3), (P, 4))
    params = [torch.nn.Parameter(torch.zeros(*sh)) for sh in shapes]
    bucket = mdist.GradBucket(params)
    opt = FlatAdamW([{"params": [p_], "lr": 1e-3} for p_ in params], bucket, capturable=True)
    cx = RasterContext()
    kw = dict(zip(names, params))
    refused = False
    try:
        opt.fuse_into_backward(cx, **kw)
    except RuntimeError as e:
        refused = "local_only" in str(e)
    still_clean = opt.fused is None and cx.fused_adamw is None
    opt.fuse_into_backward(cx, local_only=True, **kw)            # every rank its own model: allowed when said so
    q.put((rank, refused, still_clean, cx.fused_adamw is opt.fused and opt.fused is not None))
    dist.barrier()
    dist.destroy_process_group()


def test_fused_optimizer_is_refused_in_a_data_parallel_group_gloo_world2(hip_lib):
    """fuse_into_backward on an unsharded optimizer in a group of > 1 ranks used to be accepted -- the fused
    gradients never reach the bucket, no all-reduce averages them, replicas diverge silently.  Now refused unless local_only=True."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_fuse_guard_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, refused, still_clean, fused_ok in res:
        assert refused and still_clean and fused_ok, (rank, refused, still_clean, fused_ok)


def test_unfuse_rearms_the_flat_step(hip_lib):
    """step() returned early whenever the optimizer had EVER been fused; clearing context.fused_adamw by hand (what
    round 4's error message suggested) then froze the parameters without a word.  Now: step() is a no-op only while the context still
    carries this optimizer's fused update; a context cleared by hand makes step() raise; unfuse() clears both sides."""
    from moss_amd.diff_gaussian_rasterization import RasterContext
    from moss_amd.dist import GradBucket
    from moss_amd.optim import FlatAdamW
    P = 4
    names = ("means3D", "sh", "opacity", "scales", "rotations")
    params = [torch.nn.Parameter(torch.zeros(*sh)) for sh in ((P, 3), (P, 16, 3), (P, 1), (P, 3), (P, 4))]
    bucket = GradBucket(params)
    opt = FlatAdamW([{"params": [p_], "lr": 1e-3} for p_ in params], bucket, capturable=True)
    cx = RasterContext()
    opt.fuse_into_backward(cx, **dict(zip(names, params)))
    assert cx.fused_adamw is opt.fused is not None
    assert opt.step() is None                                    # the backward kernel takes the step: nothing is launched (no GPU here)
    cx.fused_adamw = None                                        # the stale advice
    with pytest.raises(RuntimeError, match="unfuse"):
        opt.step()
    opt.unfuse()
    assert opt.fused is None and cx.fused_adamw is None
    opt.fuse_into_backward(cx, **dict(zip(names, params)))       # and it can be fused again
    opt.unfuse(cx)
    assert opt.fused is None and cx.fused_adamw is None
    # a guarded step on a sharded optimizer is refused (one rank would skip its shard while its peers step theirs)
    b2 = GradBucket([torch.nn.Parameter(torch.zeros(16))], world=2)
    o2 = FlatAdamW([{"params": b2.params, "lr": 1e-3}], b2, capturable=True, shard=(0, 2))
    with pytest.raises(RuntimeError, match="SHARDED"):
        o2.step(skip_word=torch.zeros(1, dtype=torch.int32))


def _diff_hunks(path):
    """(target file, [(old_start, old_lines, new_start, new_lines), ...]) of a unified diff.  Lines keep their CR: the target files
    have CRLF line endings and the diffs carry them."""
    lines = open(path, "rb").read().decode().split("\n")
    target, hunks, i = None, [], 0
    while i < len(lines):
        if lines[i].startswith("+++ b/"):
            target = lines[i][6:].rstrip("\r")
        m = re.match(r"@@ -(\d+),(\d+) \+(\d+),(\d+) @@", lines[i])
        i += 1
        if not m:
            continue
        o0, on, n0, nn = map(int, m.groups())
        old, new = [], []
        while len(old) < on or len(new) < nn:
            tag, s = lines[i][:1], lines[i][1:]
            assert tag in (" ", "-", "+"), f"{os.path.basename(path)}:{i + 1}: {lines[i]!r}"
            if tag != "+":
                old.append(s)
            if tag != "-":
                new.append(s)
            i += 1
        assert (len(old), len(new)) == (on, nn), f"{os.path.basename(path)}: hunk at -{o0} miscounted"
        hunks.append((o0, old, n0, new))
    assert target and hunks, path
    return target, hunks


def _apply_exactly(text, hunks):
    """``text``: the lines of a file, None where no hunk has shown the line yet.  Each hunk must sit exactly where its header says --
    no offset, no fuzz: the new-side start is the old-side start plus what the hunks before it added -- and its context and removed
    lines must be the lines found there (a line still unknown is taken from the hunk).  Returns the patched lines."""
    text, out, pos, delta = list(text), [], 0, 0
    for o0, old, n0, new in hunks:
        assert n0 == o0 + delta, (o0, n0, delta)
        start = o0 - 1 if old else o0
        assert start >= pos, "hunks overlap or are out of order"
        text += [None] * (start + len(old) - len(text))
        for j, s in enumerate(old):
            if text[start + j] is None:
                text[start + j] = s
            assert text[start + j] == s, f"line {start + j + 1}: {text[start + j]!r} != {s!r}"
        out += text[pos:start] + new
        pos = start + len(old)
        delta += len(new) - len(old)
    return out + text[pos:]


def test_moss_side_patches_apply(hip_lib):
    """patches/*.diff (the MOSS-side edits of INTEGRATION.md section 3) are well-formed and apply in their documented order -- the
    three, then train_ZJU_one_call_loss.diff on top of train_ZJU.diff -- each hunk exactly at its line (no offset, no fuzz).  The lines
    of the MOSS files come from the diffs themselves (context and removed lines): where two diffs touch the same lines, the later one
    must find what the earlier one left.  The patched lines say what the integration needs, and what they call exists."""
    files = {}
    for name in ("gaussian_renderer.diff", "train_ZJU.diff", "gaussian_model.diff", "train_ZJU_one_call_loss.diff"):
        target, hunks = _diff_hunks(os.path.join(ROOT, "patches", name))
        try:
            files[target] = _apply_exactly(files.get(target, []), hunks)
        except AssertionError as e:
            raise AssertionError(f"{name} does not apply to {target}: {e}") from None
    assert set(files) == {"gaussian_renderer/__init__.py", "train_ZJU.py", "scene/gaussian_model.py"}
    files = {k: "\n".join(s for s in v if s is not None) for k, v in files.items()}
    for rel in ("gaussian_renderer/__init__.py", "train_ZJU.py"):
        src = files[rel]
        assert "transforms_in_op" in src
        assert "raw_parameters_in_op" in src               # set by the train_ZJU patch AND read by the renderer patch
    assert "pc._opacity, pc._scaling, pc._rotation, 7" in files["gaussian_renderer/__init__.py"]
    src = files["scene/gaussian_model.py"]
    assert "from moss_amd.optim import AdamW as _AdamW" in src and "torch.optim.AdamW(l, lr=0.0, eps=1e-15)" not in src
    src = files["train_ZJU.py"]
    assert "ssim_fused as ssim" in src
    # the optional fourth diff (on top of train_ZJU.diff): lines 111-119 and the first three terms of :131 as ONE call
    assert "training_loss_moss_fused(image, alpha, gt_image, bkgd_mask, viewpoint_cam.moss_region, terms_out=raster_terms)" in src
    assert "loss = raster_loss +" in src and "cv2.boundingRect" not in src
    from moss_amd import optim as moptim
    import torch as _t
    assert issubclass(moptim.AdamW, _t.optim.Optimizer)
    # what the patched lines call exists with the argument names they use
    import inspect
    from moss_amd import densify
    from moss_amd.diff_gaussian_rasterization import GaussianRasterizer
    assert "context" in inspect.signature(GaussianRasterizer.__init__).parameters
    assert "transforms" in inspect.signature(GaussianRasterizer.forward).parameters
    assert list(inspect.signature(densify.densify_stats_update).parameters) == ["max_radii2D", "xyz_gradient_accum", "denom", "radii", "viewspace_grad"]
    from moss_amd import loss as mloss
    assert list(inspect.signature(mloss.training_loss_moss_fused).parameters)[:5] == ["image", "alpha", "gt_image", "bkgd_mask", "region"]
    assert "terms_out" in inspect.signature(mloss.training_loss_moss_fused).parameters and hasattr(mloss.ViewRegion, "copy_")


def test_graft_entry_build_passes(hip_lib):
    """__graft_entry__.build() is what the driver runs as its "does it build" check: it must succeed on a tree whose libraries are
    current (it re-checks the three ABI numbers -- library, compiled glue, Python binding -- against each other, never against a literal:
    the literal survived two ABI bumps unnoticed in round 4)."""
    import importlib
    import re
    ge = importlib.import_module("__graft_entry__")
    ge.build()
    src = open(ge.__file__).read()
    assert not re.search(r"abi_version\(\)\s*==\s*\d", src)


def test_gradient_bucket_tensors_are_16_byte_aligned():
    """Every tensor of the flat gradient / parameter / moment buffers starts at a multiple of 4 floats whatever the sizes (P is
    arbitrary after a densification): the kernels that read and write those slices work on float4, and with P % 4 != 0 the SH slice of
    rounds 1-3's packed layout was misaligned (the staged paths silently fell back to per-lane loads)."""
    from moss_amd.dist import GradBucket
    P = 1237
    params = [torch.nn.Parameter(torch.randn(P, 3)), torch.nn.Parameter(torch.randn(P, 16, 3)), torch.nn.Parameter(torch.randn(P, 1)),
              torch.nn.Parameter(torch.randn(P, 3)), torch.nn.Parameter(torch.randn(P, 4))]
    b = GradBucket(params)
    assert all(off % 4 == 0 for off in b.offsets) and b.offsets[0] == 0
    assert all(b.offsets[i] + b.sizes[i] <= b.offsets[i + 1] < b.offsets[i] + b.sizes[i] + 4 for i in range(4))
    assert b.n_params == b.offsets[-1] + b.sizes[-1] and b.tail % 4 == 0 and b.tail >= b.n_params
    for v, p in zip(b.views, params):
        assert v.shape == p.shape and v.data_ptr() % 16 == b.flat.data_ptr() % 16
    flat = b.pack([p.data for p in params])
    for p, n, off in zip(params, b.sizes, b.offsets):
        assert torch.equal(flat[off:off + n], p.data.reshape(-1))
    gaps = torch.ones(b.n_params, dtype=torch.bool)
    for n, off in zip(b.sizes, b.offsets):
        gaps[off:off + n] = False
    assert float(flat[gaps].abs().sum()) == 0.0 and int(gaps.sum()) == b.n_params - sum(b.sizes)


def test_per_gaussian_backward_keeps_two_waves_per_simd():
    """The per-Gaussian backward kernels sit close to the register budget of two waves per SIMD (its 1 563 single-wave workgroups need
    six per CU to be resident together): the fused form was measured at 38 us with 254 VGPRs and at 52 us with 260 -- one wave per SIMD --
    when a block of scalar loads was placed where its registers stay live across the gather (profiles/r04_notes.md section 8).  The
    compiler's own resource report for gfx950 must say 2 waves per SIMD and no more scratch than the 128 bytes per lane of rounds 2-4."""
    import re
    import shutil
    import subprocess
    import tempfile
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    from moss_amd import build as hip_build
    src = os.path.join(ROOT, "moss_amd", "csrc", "preprocess.hip")
    with tempfile.TemporaryDirectory(dir=os.path.join(ROOT, "moss_amd", "lib")) as tmp:
        cmd = [hipcc] + [a for a in hip_build.COMMON if a != "-Wall"] + hip_build.SOURCES["preprocess.hip"] + \
              ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "pp.o")]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    found = {}
    blocks = re.split(r"remark: Function Name: ", p.stderr)
    for b in blocks[1:]:
        name = b.split()[0]
        m = re.search(r"preprocess_backward_kernelILb(\d)ELb(\d)ELi(\d)E", name)
        if not m:
            continue
        vg = int(re.search(r"VGPRs: (\d+)", b).group(1)); ag = int(re.search(r"AGPRs: (\d+)", b).group(1))
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)); scr = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        found[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = (vg, ag, occ, scr)
    # (third parameter: log2 of the lanes per Gaussian -- the small-P instantiation, 4, exists for the staged-SH kernels only)
    assert set(found) == {(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0), (1, 0, 4), (1, 1, 4)}, found
    for key, (vg, ag, occ, scr) in found.items():
        assert occ >= 2 and vg + ag <= 256 and scr <= 128, f"preprocess_backward_kernel<STAGE_SH={key[0]}, FUSED={key[1]}, LPG_L2={key[2]}>: {vg} VGPRs + {ag} AGPRs, {occ} waves per SIMD, {scr} B scratch"


def test_sort_kernel_keeps_two_workgroups_per_cu():
    """chunk_sort_kernel runs 1024-thread workgroups -- four waves per SIMD each -- and its whole grid (the frame's chunks + the scan
    block that rides along on the asynchronous path) must be resident at once: two workgroups per CU = 8 waves per SIMD = at most 64
    VGPRs.  Round 5 measured what 70 cost (a 64-bit division in the scan block's overflow hint, values held across its third block
    scan): 12.9 -> 16.7 us, late workgroups starting 8 us into the kernel (scripts/sort_stamps.py)."""
    import re
    import shutil
    import subprocess
    import tempfile
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    from moss_amd import build as hip_build
    src = os.path.join(ROOT, "moss_amd", "csrc", "binning.hip")
    with tempfile.TemporaryDirectory(dir=os.path.join(ROOT, "moss_amd", "lib")) as tmp:
        cmd = [hipcc] + [a for a in hip_build.COMMON if a != "-Wall"] + hip_build.SOURCES["binning.hip"] + \
              ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "bn.o")]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    found = {}
    for b in re.split(r"remark: Function Name: ", p.stderr)[1:]:
        m = re.search(r"chunk_sort_kernelILi(\d)E", b.split()[0])
        if m:
            found[int(m.group(1))] = (int(re.search(r"VGPRs: (\d+)", b).group(1)), int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)))
    assert set(found) == {1, 8}, found
    for k, (vg, occ) in found.items():
        assert vg <= 64 and occ >= 8, f"chunk_sort_kernel<{k}>: {vg} VGPRs, {occ} waves per SIMD"


def _active_sh_rank_main(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from moss_amd import dist as mdist
    mdist.init_from_env(backend="gloo")
    g = torch.Generator().manual_seed(40 + rank)
    P = 37
    out = {}
    for degree in (0, 1, 2, 3):
        res = []
        for active in (None, degree):
            xyz, sh, opa = (torch.nn.Parameter(torch.zeros(P, 3)), torch.nn.Parameter(torch.zeros(P, 16, 3)), torch.nn.Parameter(torch.zeros(P, 1)))
            b = mdist.GradBucket([xyz, sh, opa])
            gg = torch.Generator().manual_seed(100 * degree + rank)
            b.attach()
            xyz.grad.copy_(torch.randn(P, 3, generator=gg)); opa.grad.copy_(torch.randn(P, 1, generator=gg))
            k = (degree + 1) ** 2
            sh.grad[:, :k, :] = torch.randn(P, k, 3, generator=gg)               # the backward writes exact zeros above the active degree
            b.loss_terms[:] = torch.tensor([1.0, 2.0, 3.0, 4.0]) * (rank + 1)
            loss = b.all_reduce_mean(None, world, sh_param=sh if active is not None else None, active_sh_degree=active)
            res.append((b.flat.clone(), float(loss)))
        out[degree] = bool(torch.equal(res[0][0], res[1][0])) and res[0][1] == res[1][1] == 1.5
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_active_degree_sh_exchange_equals_the_full_all_reduce_gloo_world2():
    """GradBucket.all_reduce_mean(sh_param=, active_sh_degree=): only the first 3 (d+1)^2 of every 48 SH floats travel (packed; the
    rest of the bucket in two more pieces) -- round 3's review item 6.  The bucket afterwards is BIT-identical to the full all-reduce at
    every degree (the coefficients above the active degree are exact zeros on every rank: their mean is zero), the loss block included."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_active_sh_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, out in res:
        assert out == {0: True, 1: True, 2: True, 3: True}, (rank, out)


_TEARDOWN_RANK = r"""
import os, sys, time
sys.path.insert(0, sys.argv[2])
import torch, torch.distributed as dist
from moss_amd import dist as mdist
rank, world, _ = mdist.init_from_env(backend="gloo")
t = torch.ones(4); dist.all_reduce(t); assert float(t[0]) == 2.0
if sys.argv[1] == "peer_dies":
    if rank == 1:
        os._exit(3)                      # dies without any teardown
    time.sleep(0.5)
    try:
        dist.all_reduce(t)
    except RuntimeError:
        sys.exit(5)                      # leaves on the error, through the teardown
    sys.exit(6)
"""


@pytest.mark.parametrize("mode,want", [("clean", [0, 0]), ("peer_dies", [5, 3])])
def test_a_gloo_rank_leaves_through_the_group_teardown(mode, want):
    """A rank that leaves the interpreter with its gloo group alive aborts now and then while the static destructors run ("terminate
    called without an active exception": 2 of 48 two-rank dry runs of bench.py with six running at once, after the result line was
    printed, so the launcher reports a failed job; 0 of 96 with the teardown).  init_from_env therefore registers
    destroy_process_group at exit for gloo.  Two real ranks: both leave cleanly with 0; and a rank whose peer DIED without any
    teardown sees its next collective fail and still leaves at once with its own exit code -- the teardown waits for nobody."""
    import socket
    import subprocess
    import sys
    import time
    from moss_amd import dist as mdist
    assert mdist._destroy_group_at_exit() is None                                # without a group: nothing to do
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0)); port = so.getsockname()[1]
    ps = []
    for r in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r))
        ps.append(subprocess.Popen([sys.executable, "-c", _TEARDOWN_RANK, mode, ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    t0 = time.time()
    outs = [p.communicate(timeout=120)[0] for p in ps]
    assert [p.returncode for p in ps] == want, outs
    assert time.time() - t0 < 60
