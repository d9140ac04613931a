"""``moss_amd.play`` on the GPU: the 8-bit kernel against its torch statement, and ``MossPlayer`` / ``evaluate_split`` against the
renderer, the training step and ``metrics.evaluate_views``.  The world is tests/test_gpu_moss_step.py's (P = 6 890, 512 x 512, the
fixture networks); a second camera has another focal length and pose.  Everything is compared bit for bit: the player adds no
mathematics, and the kernel's float32 operations are each rounded on their own like torch's."""
import copy
import gc
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_gpu_moss_step import FLAGS, _frame, _fresh, _load, _step, world   # noqa: F401  (``world``: the module fixture, shared)
from tests.test_player_cpu import as_image, boundary_values

pytestmark = pytest.mark.gpu

KEYS = ("render", "render_depth", "render_alpha", "radii")


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    """Leave the device as the module found it: players and their graphs refer to each other, so the pools go with a collection."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch._C._cuda_clearCublasWorkspaces()
    torch.cuda.empty_cache()


def _second_camera(cam, gpu):
    """The world's view seen by another camera: another focal length (so another tanfov), principal point and pose."""
    from moss_amd import scenes
    from moss_amd.gaussian_renderer import camera_view
    R, t = scenes.look_at_ring(8, radius=3.4, height=-0.2)[1]
    c = camera_view(scenes.make_camera(512, 512, 640.0, 610.0, 250.0, 262.0, R, t), gpu)
    c.smpl_param, c.big_pose_smpl_param, c.big_pose_world_vertex = cam.smpl_param, cam.big_pose_smpl_param, cam.big_pose_world_vertex
    return c


def _eager(pc, cam, bg, precision="f32", flags=FLAGS):
    """``gaussian_renderer.render`` eagerly under ``no_grad`` with the seven in-op flags, on a synchronous context of its own."""
    from moss_amd.diff_gaussian_rasterization import RasterContext
    from moss_amd.gaussian_renderer import render
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raster_context=RasterContext(),
                           lbs_weights_precision=precision, **flags)
    with torch.no_grad():
        out = render(cam, pc, pipe, bg)
    got = {k: out[k].clone() for k in KEYS}
    got["transforms"], got["translation"] = out["transforms"][0].clone(), out["translation"][0].clone()
    return got


def _same(a, b, keys=KEYS, what=""):
    for k in keys:
        assert torch.equal(a[k], b[k]), f"{what}: {k}"


@pytest.fixture(scope="module")
def scene(gpu, world):
    """One model and two cameras that no test changes, with the eager renders of 4 frames x 2 cameras."""
    pc, cam, _ = _fresh(world)
    cams = [cam, _second_camera(cam, gpu)]
    ref = {}
    for k in range(4):
        _load(cam, k, gpu)
        for c in range(2):
            ref[k, c] = _eager(pc, cams[c], world["bg"])
    assert float(ref[0, 0]["render"].abs().max()) > 0.1 and float(ref[0, 1]["render"].abs().max()) > 0.1
    assert not torch.equal(ref[0, 0]["render"], ref[0, 1]["render"]) and not torch.equal(ref[0, 0]["render"], ref[1, 0]["render"])
    _load(cam, 0, gpu)
    return SimpleNamespace(pc=pc, cams=cams, ref=ref, bg=world["bg"])


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (17, 33), (48, 64), (512, 512)])
def test_frames_to_u8_equals_its_torch_statement(gpu, hip_lib, shape):
    """1, 3 and 8 views per call, RGB and RGBA, both roundings, with and without masks; view 0 is the boundary set of the CPU test
    tiled into the image; one output starts 1 byte into its buffer, and the bytes around every output stay as they were."""
    from moss_amd.play import frames_to_u8, frames_to_u8_torch
    H, W = shape
    g = torch.Generator().manual_seed(H * 1000 + W)
    values = boundary_values()
    images = [as_image(values, H, W)] + [torch.rand(3, H, W, generator=g) * 1.5 - 0.25 for _ in range(7)]
    images[1].view(-1)[::5] = float("nan")
    images = [t.to(gpu) for t in images]
    alphas = [as_image(values.flip(0), H, W)[0].contiguous().to(gpu)] + [torch.rand(1, H, W, generator=g).to(gpu) for _ in range(7)]
    bounds = [(torch.rand(H, W, generator=g) > 0.3).to(torch.uint8).to(gpu) for _ in range(8)]
    bounds[2].view(-1)[::3] = 2                                       # (anything but 1 is outside)
    for n in (1, 3, 8):
        for C in (3, 4):
            for rounding in ("nearest", "truncate"):
                for masked in (False, True):
                    kw = dict(alphas=alphas[:n] if C == 4 else None, regions=bounds[:n] if masked else None, fill=1.0 if masked else 0.0,
                              rounding=rounding)
                    want = frames_to_u8_torch(images[:n], **kw)
                    got = frames_to_u8(images[:n], **kw)
                    for b in range(n):
                        assert got[b].dtype == torch.uint8 and tuple(got[b].shape) == (H, W, C)
                        assert torch.equal(got[b], want[b]), (n, C, rounding, masked, b)
    # outputs at byte offsets 1 (no packed store is possible there), 4 and 6, guard bytes on both sides
    for C in (3, 4):
        nb = H * W * C
        buffers = [torch.full((nb + 16,), 0xAB, dtype=torch.uint8, device=gpu) for _ in range(3)]
        outs = [buf[o:o + nb].view(H, W, C) for buf, o in zip(buffers, (1, 4, 6))]
        assert outs[0].data_ptr() % 4 == 1 and outs[1].data_ptr() % 4 == 0
        kw = dict(alphas=alphas[:3] if C == 4 else None, regions=bounds[:3], fill=1.0)
        back = frames_to_u8(images[:3], out=outs, **kw)
        want = frames_to_u8_torch(images[:3], **kw)
        for b, (buf, o) in enumerate(zip(buffers, (1, 4, 6))):
            assert back[b] is outs[b] and torch.equal(outs[b], want[b]), (C, b)
            assert bool((buf[:o] == 0xAB).all()) and bool((buf[o + nb:] == 0xAB).all()), (C, b)
    # an unaligned INPUT (a view 4 bytes into its storage) takes the element-wise loads
    shifted = torch.zeros(3 * H * W + 1, device=gpu)
    shifted[1:].copy_(images[0].view(-1))
    assert torch.equal(frames_to_u8(shifted[1:].view(3, H, W)), frames_to_u8_torch(images[0]))


def test_frames_to_u8_is_capturable(gpu, hip_lib):
    from moss_amd.graphs import capturing
    from moss_amd.play import frames_to_u8, frames_to_u8_torch
    H, W = 48, 64
    g = torch.Generator().manual_seed(9)
    image, alpha = torch.rand(3, H, W, generator=g).to(gpu), torch.rand(1, H, W, generator=g).to(gpu)
    out = torch.zeros(H, W, 4, dtype=torch.uint8, device=gpu)
    frames_to_u8(image, alphas=alpha, out=out)                       # (an eager run first)
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    with capturing(graph, collect=True):
        frames_to_u8(image, alphas=alpha, out=out, rounding="truncate")
    for seed in (10, 11):
        g = torch.Generator().manual_seed(seed)
        image.copy_((torch.rand(3, H, W, generator=g) * 1.4 - 0.2).to(gpu))
        alpha.copy_(torch.rand(1, H, W, generator=g).to(gpu))
        out.zero_()
        graph.replay()
        assert torch.equal(out, frames_to_u8_torch(image, alphas=alpha, rounding="truncate")) and bool(out.any())
    with pytest.raises(ValueError, match="alphas"):
        frames_to_u8([image, image], alphas=[alpha, None])
    with pytest.raises(ValueError, match="contiguous"):
        frames_to_u8(image.permute(0, 2, 1))


# ---- the player --------------------------------------------------------------------------------------------------------------------
def test_the_player_adds_no_mathematics(gpu, hip_lib, scene):
    """frame() eager, frame() replayed and pose() + render() against the eager render, over 4 frames and 2 cameras; the graphs are
    counted: 1 pose graph + 1 render graph per camera, and none more when a camera comes back."""
    from moss_amd.play import MossPlayer
    pc, cams, ref = scene.pc, scene.cams, scene.ref
    before = [p.detach().clone() for p in (pc._xyz, pc._features, pc._opacity, pc._scaling, pc._rotation)]
    player = MossPlayer(pc, cams[0], scene.bg)
    tables = ("transforms", "translation")
    for k in range(4):                                               # eager
        for c in range(2):
            out = player.frame(cams[c], _frame(k, gpu))
            _same(out, ref[k, c], what=f"eager frame {k} camera {c}")
            _same(player.tables(), ref[k, c], tables, f"eager tables {k}")
    assert player.captures == 0 and player.poses == 8 and player.pose_replays == 0
    player.capture(warmup=2)
    assert player.captures == 2
    for k in range(4):                                               # replayed
        for c in range(2):
            out = player.frame(cams[c], _frame(k, gpu))
            _same(out, ref[k, c], what=f"replayed frame {k} camera {c}")
            _same(player.tables(), ref[k, c], tables, f"replayed tables {k}")
        assert player.captures == 3                                  # the first camera came back: nothing new
    assert player.live_render_graphs == 2 and player.pose_replays >= 8
    for k in (2, 0):                                                 # pose once, render from both cameras
        posed = player.pose(_frame(k, gpu))
        assert tuple(posed["transforms"].shape) == (6890, 3, 3) and tuple(posed["translation"].shape) == (6890, 3)
        assert tuple(posed["Rs"].shape) == (23, 3, 3) and tuple(posed["lbs_weights"].shape) == (6890, 24)
        for c in (1, 0):
            _same(player.render(cams[c]), ref[k, c], what=f"pose + render {k} camera {c}")
    assert player.captures == 3 and not player.check() and player.dropped_frames == 0
    # an LRU of one: the cameras evict each other, the results stay
    small = MossPlayer(pc, cams[0], scene.bg, max_render_graphs=1).capture()
    assert small.captures == 2
    for i, c in enumerate((1, 0, 1)):
        _same(small.frame(cams[c], _frame(1, gpu)), ref[1, c], what=f"LRU of one, camera {c}")
        assert small.captures == 3 + i and small.live_render_graphs == 1
    for p, q in zip((pc._xyz, pc._features, pc._opacity, pc._scaling, pc._rotation), before):
        assert torch.equal(p, q)                                     # the player writes no parameter


@pytest.mark.parametrize("precision,template_index", [("f32", False), ("f32", True), ("bf16x3", True)])
def test_the_player_shows_what_the_step_trains_on(gpu, hip_lib, world, precision, template_index):
    from moss_amd.play import MossPlayer
    from moss_amd.train import MossStep
    pp, cp, _ = _fresh(world)
    ps, cs, _ = _fresh(world)
    _load(cp, 2, gpu)
    _load(cs, 2, gpu)
    player = MossPlayer(pp, cp, world["bg"], template_index=template_index, lbs_weights_precision=precision)
    step = MossStep(ps, cs, world["gt"], world["bkgd"], world["region"], world["bg"], world["lpips"],
                    {"auto_regression": 2.5e-4, "cross_attention_lbs": 1e-4}, template_index=template_index, lbs_weights_precision=precision)
    shown = player.frame()["render"].clone()
    trained = step.compute()["render"]
    assert torch.equal(shown, trained) and float(shown.abs().max()) > 0.1
    assert not hasattr(pp, "template_index")                         # (the player's index is its own: the model is not touched)


def test_render_from_explicit_tables(gpu, hip_lib, scene):
    """render_ZJU.py's branch: the tables of a pose, cloned, rendered later from both cameras."""
    from moss_amd.play import MossPlayer
    player = MossPlayer(scene.pc, scene.cams[0], scene.bg).capture()
    made = player.frame(scene.cams[0], _frame(3, gpu))
    _same(made, scene.ref[3, 0], what="the frame that made the tables")
    kept = {k: v.clone() for k, v in player.tables().items() if k in ("transforms", "translation")}
    player.frame(scene.cams[1], _frame(1, gpu))                      # (another pose in between)
    for c in (0, 1):
        out = player.render(scene.cams[c], transforms=kept["transforms"][None], translation=kept["translation"])
        _same(out, scene.ref[3, c], what=f"from tables, camera {c}")
    with pytest.raises(ValueError, match="together"):
        player.render(transforms=kept["transforms"])


def test_a_model_without_motion_offsets_is_posed_by_the_smpl_weights(gpu, hip_lib, world):
    """``motion_offset_flag=False``: ``render()``'s ``lbs_in_op`` branch alone -- neither network runs (the model has none here) -- with
    the frame, pose and parameter flags the player's render graphs always use."""
    from moss_amd.play import MossPlayer
    pc, cam, _ = _fresh(world)
    pc.motion_offset_flag = False
    del pc.auto_regression, pc.cross_attention_lbs
    _load(cam, 1, gpu)
    want = _eager(pc, cam, world["bg"])
    player = MossPlayer(pc, cam, world["bg"])
    _same(player.frame(), want, what="eager")
    assert player.tables()["Rs"] is None
    _same(player.capture().frame(), want, what="replayed")
    _same(player.tables(), want, ("transforms", "translation"), "tables")
    pm, cm, _ = _fresh(world)
    _load(cm, 1, gpu)
    assert not torch.equal(_eager(pm, cm, world["bg"])["render"], want["render"])      # (the networks do move the avatar)


def test_a_frame_reads_nothing_back(gpu, hip_lib, scene):
    from moss_amd.play import MossPlayer
    for captured in (False, True):
        player = MossPlayer(scene.pc, scene.cams[0], scene.bg)
        if captured:
            player.capture(warmup=2)
        for k in range(2):
            player.frame(scene.cams[0], _frame(k, gpu))              # (the first forward of a context is synchronous by design)
        frames = [_frame(k, gpu) for k in (2, 3)]
        torch.cuda.synchronize(gpu)
        torch.cuda.set_sync_debug_mode("error")
        try:
            for f in frames:
                out = player.frame(scene.cams[0], f)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize(gpu)
        _same(out, scene.ref[3, 0], what=f"captured={captured}")


def test_a_view_that_overflows_is_counted_and_its_graph_captured_again(gpu, hip_lib, world):
    """Captured on shrunken Gaussians, replayed on grown ones (as the step's dropped-frame test): the view is empty, check() counts it
    and captures that graph again, and the next frame is the eager one."""
    from moss_amd.play import MossPlayer
    pc, cam, _ = _fresh(world)
    original = pc._scaling.detach().clone()
    with torch.no_grad():
        pc._scaling.copy_(original - 5.0)
    player = MossPlayer(pc, cam, world["bg"]).capture(warmup=2)
    with torch.no_grad():
        pc._scaling.copy_(original + 2.0)
    out = player.frame()
    torch.cuda.synchronize(gpu)
    assert not bool(out["render"].any())                             # rendered nothing
    assert player.check() and player.dropped_frames >= 1 and player.recaptures == 1
    dropped, captures = player.dropped_frames, player.captures
    out = player.frame()
    _same(out, _eager(pc, cam, world["bg"]), what="after the re-capture")
    assert float(out["render"].abs().max()) > 0
    assert not player.check() and player.dropped_frames == dropped and player.captures == captures


def test_a_stale_player_raises_until_it_is_refreshed(gpu, hip_lib, world):
    from moss_amd.checkpoint import assign_rows
    from moss_amd.play import MossPlayer
    pc, cam, _ = _fresh(world)
    player = MossPlayer(pc, cam, world["bg"]).capture()
    _same(player.frame(), _eager(pc, cam, world["bg"]), what="before")
    rows = slice(0, 5000)
    values = {"xyz": pc._xyz, "features": pc._features, "opacity": pc._opacity, "scaling": pc._scaling, "rotation": pc._rotation}
    assign_rows(pc, {k: v.detach()[rows].clone() for k, v in values.items()})
    assert int(pc._xyz.shape[0]) == 5000
    for call in (player.frame, player.pose, player.render, player.check):
        with pytest.raises(RuntimeError, match="refresh"):
            call()
    player.refresh()
    want = _eager(pc, cam, world["bg"])
    out = player.frame()
    assert tuple(out["radii"].shape) == (5000,) and tuple(player.tables()["transforms"].shape) == (5000, 3, 3)
    _same(out, want, what="after refresh")
    pc.active_sh_degree -= 1                                         # the degree is a launch argument too
    with pytest.raises(RuntimeError, match="refresh"):
        player.frame()
    player.refresh()
    _same(player.frame(), _eager(pc, cam, world["bg"]), what="another degree")


def test_evaluate_split(gpu, hip_lib, world, scene, tmp_path, monkeypatch):
    """3 poses x 2 cameras.  The grouped split equals ``metrics.evaluate_views`` given the returned tables and equals the split with
    every ``pose_id`` removed, as Python floats; the pose graph runs 3 and 6 times; with ``out_dir`` the PNGs hold the clamped, filled
    render, and the per-view loop reads nothing back."""
    from moss_amd import metrics
    from moss_amd.play import MossPlayer, evaluate_split, frames_to_u8_torch, read_png
    pc, cams = scene.pc, scene.cams
    views = []
    for k in range(3):
        for c in range(2):
            v = copy.copy(cams[c])
            v.smpl_param, v.pose_id = _frame(k, gpu), 10 + k
            views.append(v)
    g = torch.Generator().manual_seed(31)
    gts = [(torch.rand(3, 512, 512, generator=g) * 1.1 - 0.05).to(gpu) for _ in range(6)]
    regions = [world["region"]] * 5 + [None]
    lp = world["lpips"]
    player = MossPlayer(pc, cams[0], scene.bg).capture()
    at = player.pose_replays
    grouped = evaluate_split(player, views, gts, regions, lpips=lp)
    assert player.pose_replays - at == 3 and grouped["n"] == 6
    tables = grouped["tables"]
    assert list(tables) == [10, 11, 12]
    for k in range(3):
        assert tuple(tables[10 + k]["transforms"].shape) == (1, 6890, 3, 3) and tuple(tables[10 + k]["translation"].shape) == (1, 6890, 3)
        assert torch.equal(tables[10 + k]["transforms"][0], scene.ref[k, 0]["transforms"])
    by_hand = metrics.evaluate_views(pc, views, gts, regions, scene.bg, transforms=[tables[v.pose_id]["transforms"] for v in views],
                                     translation=[tables[v.pose_id]["translation"] for v in views], lpips=lp)
    print("\nsplit " + ", ".join(f"{k} {grouped[k]!r}" for k in ("l1", "psnr", "ssim", "lpips", "n")))
    for k in ("l1", "psnr", "ssim", "lpips", "n"):
        assert grouped[k] == by_hand[k], (k, grouped[k], by_hand[k])
    assert 0 < grouped["l1"] < 1 and grouped["lpips"] > 0
    loose = [copy.copy(v) for v in views]
    for v in loose:
        del v.pose_id
    at = player.pose_replays
    ungrouped = evaluate_split(player, loose, gts, regions, lpips=lp, keep_tables=False)
    assert player.pose_replays - at == 6 and ungrouped["tables"] is None
    for k in ("l1", "psnr", "ssim", "lpips", "n"):
        assert ungrouped[k] == grouped[k], k
    # poses that come back later in the order are not posed again
    at = player.pose_replays
    shuffled = [0, 2, 4, 1, 3, 5]
    mixed = evaluate_split(player, [views[i] for i in shuffled], [gts[i] for i in shuffled], [regions[i] for i in shuffled])
    assert player.pose_replays - at == 3 and mixed["lpips"] is None and mixed["n"] == 6
    # the files; error mode is on from the report's reset to its read, which is the per-view loop
    reset, sums = metrics.QualityReport.reset, metrics.QualityReport.sums

    def reset_then_watch(self):
        reset(self)
        torch.cuda.synchronize(gpu)
        torch.cuda.set_sync_debug_mode("error")

    def unwatch_then_read(self):
        torch.cuda.set_sync_debug_mode("default")
        return sums(self)
    monkeypatch.setattr(metrics.QualityReport, "reset", reset_then_watch)
    monkeypatch.setattr(metrics.QualityReport, "sums", unwatch_then_read)
    try:
        written = evaluate_split(player, views, gts, regions, lpips=lp, out_dir=str(tmp_path), name="test", iteration=3000)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for k in ("l1", "psnr", "ssim", "lpips", "n"):
        assert written[k] == grouped[k], k
    base = tmp_path / "test" / "ours_3000"
    names = [f"{i:05d}.png" for i in range(6)]
    assert sorted(os.listdir(base)) == ["gt", "renders"]
    assert sorted(os.listdir(base / "renders")) == names and sorted(os.listdir(base / "gt")) == names
    filled = torch.clamp(scene.ref[0, 0]["render"], 0.0, 1.0)
    filled.permute(1, 2, 0)[world["region"].bound != 1] = 0.0        # (a black background: the fill is 0)
    assert np.array_equal(read_png(str(base / "renders" / "00000.png")), frames_to_u8_torch(filled).cpu().numpy())
    assert np.array_equal(read_png(str(base / "gt" / "00005.png")), frames_to_u8_torch(torch.clamp(gts[5], 0, 1)).cpu().numpy())
    last = torch.clamp(scene.ref[2, 1]["render"], 0.0, 1.0)          # (view 5 has no region: no fill)
    assert np.array_equal(read_png(str(base / "renders" / "00005.png")), frames_to_u8_torch(last).cpu().numpy())
    with pytest.raises(ValueError, match="float32 term"):
        evaluate_split(player, views, gts, regions, lpips=SimpleNamespace(precision="bf16"))
