"""The frame-bounds ops on the device (C ABI moss_smpl_vertices / moss_bound_mask, moss_amd.bounds): the vertex kernels against a
float64 run of ``posed_vertices_torch`` and the reference's own numbers (tests/golden/frame_bounds.npz), the world bound bit for bit,
the projected corners against ``project_corners_numpy`` and the fixture, the masks bit for bit against ``bound_mask_numpy``, full
writes and determinism, capture with a new pose per replay, and ``MossPlayer(bounds=...)`` / ``evaluate_split(regions="pose")``.

The vertex bar: an element may be off by 64 eps32 s, s the tensor's largest magnitude in the case (float64) and 64 the constant
tests/test_lbs_cpu.py and tests/test_gpu_smpl_frame.py use for this chain.  Beside the op's ratio every case prints the ratio of the
float32 torch form (the same math as the parent would run it) to the same bar."""
import copy
import gc
import os

import numpy as np
import pytest
import torch

from moss_amd import bounds as mb
from moss_amd import lbs as mlbs
from tests.test_frame_bounds_cpu import box_corners, gen
from tests.test_gpu_moss_step import _frame, _fresh, world   # noqa: F401  (``world``: the module fixture, shared)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = float(np.finfo(np.float32).eps)
_BODIES = {}


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    yield
    _BODIES.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch._C._cuda_clearCublasWorkspaces()
    torch.cuda.empty_cache()


def body_of(V, J, dev):
    if (V, J) not in _BODIES:
        _BODIES[V, J] = {k: v.to(dev) for k, v in mlbs.synthetic_body_model(V, J, seed=60 + J).items()}
    return _BODIES[V, J]


def f64(d):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in d.items()}


def frame_of(seed, J, dev):
    return {k: v.to(dev).contiguous() for k, v in mlbs.synthetic_frame(seed, J).items()}


@pytest.fixture(scope="module")
def golden(gpu):
    z = np.load(os.path.join(ROOT, "tests", "golden", "frame_bounds.npz"))
    assert str(z["body_sha256"]) == gen.body_sha256()
    return z


def within_bar(name, got, ref64, plain32=None):
    bar = 64 * EPS32 * float(ref64.abs().max())
    ratio = float((got.double() - ref64).abs().max()) / bar
    other = "" if plain32 is None else f", float32 torch {float((plain32.double() - ref64).abs().max()) / bar:.4f}"
    print(f"{name}: error / bar = {ratio:.4f}{other}")
    assert ratio <= 1.0, (name, ratio)


# ---- vertices ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [1, 2, 24])
@pytest.mark.parametrize("V", [1, 15, 16, 17, 257, 6890])
@pytest.mark.parametrize("joints", [False, True])
def test_vertices_against_float64(gpu, hip_lib, V, J, joints):
    body, fr = body_of(V, J, gpu), frame_of(100 + V + J, J, gpu)
    out = mb.posed_vertices(body, fr, pad=0.1, joints=joints)
    assert len(out) == (3 if joints else 2) and out[0].dtype == torch.float32 and tuple(out[0].shape) == (V, 3)
    ref = mb.posed_vertices_torch(f64(body), f64(fr), 0.1)
    plain = mb.posed_vertices_torch(body, fr, 0.1)
    print()
    within_bar(f"V={V} J={J} world_vertex", out[0], ref[0], plain[0])
    if joints:
        within_bar(f"V={V} J={J} joints", out[2], ref[2], plain[2])
    # the bound: bit-equal to torch's min / max -+ pad on the op's OWN vertices, in float32
    pad = torch.tensor(0.1, dtype=torch.float32, device=gpu)
    expect = torch.stack([out[0].min(0).values - pad, out[0].max(0).values + pad], 0)
    assert torch.equal(out[1].view(torch.int32), expect.view(torch.int32)), (out[1], expect)


def test_vertices_and_bound_against_the_reference(gpu, hip_lib, golden):
    body = gen.golden_body(device=gpu)
    print()
    for f in range(len(gen.FRAME_SEEDS)):
        frame, pad = gen.golden_frame(f)
        fr = {k: v.to(gpu) for k, v in frame.items()}
        wv, wb, jt = mb.posed_vertices(body, fr, pad=pad, joints=True)
        within_bar(f"frame {f} world_vertex", wv, torch.tensor(golden["vertices"][f], device=gpu).double())
        within_bar(f"frame {f} joints", jt, torch.tensor(golden["joints"][f], device=gpu))
        within_bar(f"frame {f} world_bound", wb, torch.tensor(golden["world_bound"][f], device=gpu).double())
        p32 = torch.tensor(pad, dtype=torch.float32, device=gpu)
        assert torch.equal(wb, torch.stack([wv.min(0).values - p32, wv.max(0).values + p32], 0))
        # corners: against the CPU statement on the op's own bound (exactly), and against the reference's rounded corners, all of them
        K, RT = torch.tensor(golden["K"][f], device=gpu), torch.tensor(golden["RT"][f], device=gpu)
        H, W = int(golden["H"]), int(golden["W"])
        bound, rect, corners, flags = mb.bound_masks(wb, K, RT, H, W)
        expect, eflags, xy = mb.project_corners_numpy(wb.cpu().numpy(), golden["K"][f], golden["RT"][f], return_unrounded=True)
        assert float(np.abs(xy - np.floor(xy) - 0.5).min()) >= 1e-6
        np.testing.assert_array_equal(corners.cpu().numpy(), expect)
        np.testing.assert_array_equal(flags.cpu().numpy(), eflags)
        np.testing.assert_array_equal(corners.cpu().numpy(), golden["corners"][f])
        for c in range(K.shape[0]):
            eb, er = mb.bound_mask_numpy(expect[c], H, W)
            np.testing.assert_array_equal(bound[c].cpu().numpy(), eb)
            np.testing.assert_array_equal(rect[c].cpu().numpy(), er)
        assert int(rect[2, 0]) + int(rect[2, 2]) == W and int(rect[2, 1]) + int(rect[2, 3]) == H      # offside: cut on two sides


# ---- masks -----------------------------------------------------------------------------------------------------------------------------
def pixel_camera(x0, y0, x1, y1, skew=(0, 0)):
    """(world_bound, K, RT) whose eight projected corners are ``box_corners(x0, y0, x1, y1, skew)``: the box is given in pixels (a
    quarter pixel off the integers), its z spans 0..1 and moves the far face by ``skew``; w = 1."""
    wb = np.array([[x0 + 0.25, y0 + 0.25, 0.0], [x1 + 0.25, y1 + 0.25, 1.0]], dtype=np.float32)
    RT = np.array([[1, 0, skew[0], 0], [0, 1, skew[1], 0], [0, 0, 0, 1]], dtype=np.float32)
    return wb, np.eye(3, dtype=np.float32), RT


def mask_cameras(H, W):
    """name -> (world_bound, K, RT, corners expected or None, flagged): the cases of tests/test_frame_bounds_cpu.py, a perspective
    camera, and a corner behind the camera."""
    boxes = {
        "inside": (W // 4, H // 4, W // 2, H // 2, (W // 5, H // 6)),
        "left": (-W // 3 - 1, H // 4, W // 3, H // 2, (2, 1)),
        "right": (W // 2, H // 4, W + W // 3, H // 2, (1, 2)),
        "top": (W // 4, -H // 2 - 1, W // 2, H // 3, (2, -1)),
        "bottom": (W // 4, H // 2, W // 2, H + H // 2, (-2, 1)),
        "outside": (W + 3, H + 2, W + 9, H + 7, (2, 2)),
        "segment": (1, 1, 1, H - 2, (W - 3, 0)),
        "pixel": (W // 2, H // 2, W // 2, H // 2, (0, 0)),
    }
    cases = {name: pixel_camera(*b) + (box_corners(*b), False) for name, b in boxes.items()}
    wb = np.array([[-0.5, -0.9, -0.3], [0.5, 0.9, 0.3]], dtype=np.float32)
    K, RT = gen.look_at("near", np.zeros(3), 7)
    K = np.array([[min(H, W), 0, W / 2], [0, min(H, W), H / 2 + 0.25], [0, 0, 1]], dtype=np.float32)
    cases["perspective"] = (wb, K, RT, None, False)
    behind = pixel_camera(W // 4, H // 4, W // 2, H // 2)
    behind[2][2] = (0, 0, 1, -0.4)                               # w = z - 0.4: the near face is behind the camera
    cases["behind"] = behind + (None, True)
    return cases


@pytest.mark.parametrize("H,W", [(1, 1), (17, 23), (64, 64), (130, 70)])
@pytest.mark.parametrize("C", [1, 3])
def test_masks_bit_equal_to_the_cpu_statement(gpu, hip_lib, H, W, C):
    cases = mask_cameras(H, W)
    names = list(cases)
    # C = 3: consecutive triples that share a world_bound cannot be formed from different boxes, so a call serves ONE box seen by three
    # cameras: its own, the flagged one ("behind"'s K / RT), and a shifted one
    for name in names:
        wb, K, RT, expect_corners, flagged = cases[name]
        Ks, RTs = [K], [RT]
        if C == 3:
            shifted = RT.copy()
            shifted[0, 3] += 3.0
            shifted[1, 3] -= 2.0
            Ks, RTs = [K, cases["behind"][1], K], [RT, cases["behind"][2], shifted]
        Ks, RTs = np.stack(Ks), np.stack(RTs)
        out = mb.bound_masks(torch.tensor(wb, device=gpu), torch.tensor(Ks, device=gpu), torch.tensor(RTs, device=gpu), H, W)
        bound, rect, corners, flags = (t.cpu().numpy() for t in out)
        ecorners, eflags, xy = mb.project_corners_numpy(wb, Ks, RTs, return_unrounded=True)
        ok = np.isfinite(xy)
        assert float(np.abs(xy[ok] - np.floor(xy[ok]) - 0.5).min()) >= 1e-6, name
        np.testing.assert_array_equal(corners, ecorners, err_msg=name)
        np.testing.assert_array_equal(flags, eflags, err_msg=name)
        if expect_corners is not None:
            np.testing.assert_array_equal(corners[0], expect_corners, err_msg=name)
        assert bool(flags[0] & 1) == flagged, name
        if C == 3:
            assert flags[1] == 1 and (flags[2] == 0 or flagged), name
        for c in range(C):
            eb, er = mb.bound_mask_numpy(corners[c], H, W, flagged=bool(flags[c] & 1))
            np.testing.assert_array_equal(bound[c], eb, err_msg=f"{name} camera {c}")
            np.testing.assert_array_equal(rect[c], er, err_msg=f"{name} camera {c}")
            if flags[c] & 1:
                assert tuple(rect[c]) == (0, 0, W, H, W * H) and bound[c].all()
        if name == "outside":
            assert tuple(rect[0]) == (0, 0, 0, 0, 0) and not bound[0].any()
        if name == "pixel" and (H, W) != (1, 1):
            assert tuple(rect[0]) == (W // 2, H // 2, 1, 1, 1)


def test_every_byte_is_written_and_runs_repeat(gpu, hip_lib):
    V, J, C, H, W = 257, 24, 3, 130, 70
    body, fr = body_of(V, J, gpu), frame_of(5, J, gpu)
    cases = mask_cameras(H, W)
    Ks = torch.tensor(np.stack([cases[n][1] for n in ("perspective", "behind", "inside")]), device=gpu)
    RTs = torch.tensor(np.stack([cases[n][2] for n in ("perspective", "behind", "inside")]), device=gpu)
    results = []
    for fill in (0xAB, 0xAB, 0x00):
        v_out = [torch.empty(s, dtype=torch.float32, device=gpu) for s in ((V, 3), (2, 3), (J, 3))]
        m_out = [torch.empty((C, H, W), dtype=torch.uint8, device=gpu), torch.empty((C, 5), dtype=torch.int32, device=gpu),
                 torch.empty((C, 8, 2), dtype=torch.int32, device=gpu), torch.empty(C, dtype=torch.int32, device=gpu)]
        for t in v_out + m_out:
            t.view(torch.uint8).fill_(fill)
        got = mb.posed_vertices(body, fr, pad=0.1, out=v_out, joints=True)
        assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, v_out))
        wb = torch.tensor(cases["perspective"][0], device=gpu)
        mb.bound_masks(wb, Ks, RTs, H, W, out=m_out)
        results.append([t.view(torch.uint8).clone() for t in v_out + m_out])
    for a, b, c in zip(*results):
        assert torch.equal(a, b) and torch.equal(a, c)             # the same bytes twice, and whatever the buffers held before
    assert int(results[0][3].max()) == 1


# ---- capture -----------------------------------------------------------------------------------------------------------------------------
def test_frame_bounds_captured_serves_a_new_pose_per_replay(gpu, hip_lib):
    V, J, H, W = 6890, 24, 130, 70
    body = body_of(V, J, gpu)
    cases = mask_cameras(H, W)
    wb0 = np.array([[-1.2, -1.2, -1.2], [1.2, 1.2, 1.2]])

    def cameras(k):
        out = []
        for seed in (3, 4, 5):
            K, RT = gen.look_at("near", wb0.mean(0), seed)
            out.append((cases["perspective"][1], RT))
        return out
    fb, eager = mb.FrameBounds(body, cameras(0), H, W), mb.FrameBounds(body, cameras(0), H, W)
    frames = [frame_of(30 + k, J, gpu) for k in range(4)]
    fb.update(frames[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fb.update()                                              # (a host read in here would fail the capture)
    addresses = [(r.bound.data_ptr(), r.rect.data_ptr()) for r in fb.regions]
    seen = []
    for k in (1, 2, 3):
        fb.load(frames[k])
        graph.replay()
        eager.update(frames[k])
        for name in ("world_vertex", "world_bound", "joints", "bound", "rect", "corners", "flags"):
            assert torch.equal(getattr(fb, name), getattr(eager, name)), (k, name)
        assert [(r.bound.data_ptr(), r.rect.data_ptr()) for r in fb.regions] == addresses
        assert all(r.xywh is None for r in fb.regions)
        seen.append(fb.world_bound.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    region = fb.regions[1].read()
    assert region.xywh == tuple(int(v) for v in fb.rect[1, :4].tolist()) and int(fb.rect[1, 4]) == int(fb.bound[1].sum()) > 0


def test_dataset_regions_reads_the_host_once(gpu, hip_lib):
    V, J, H, W = 257, 24, 64, 64
    body = body_of(V, J, gpu)
    cases = mask_cameras(H, W)
    cams = [[(cases["perspective"][1], gen.look_at("near", np.zeros(3), 10 * p + c)[1]) for c in range(2 + p % 2)] for p in range(3)]
    cams[1][0] = (cases["behind"][1], cases["behind"][2])
    frames = [{k: v.cpu().numpy() for k, v in frame_of(40 + p, J, "cpu").items()} for p in range(3)]
    torch.cuda.synchronize()
    out = mb.dataset_regions(body, frames, cams, H, W)
    assert [len(v) for v in out["regions"]] == [2, 3, 2] and (1, 0) in out["flagged"]
    for p in range(3):
        fb = mb.FrameBounds(body, cams[p], H, W).update({k: torch.tensor(v) for k, v in frames[p].items()})
        assert torch.equal(out["world_vertex"][p], fb.world_vertex) and torch.equal(out["world_bound"][p], fb.world_bound)
        for c, region in enumerate(out["regions"][p]):
            assert torch.equal(region.bound, fb.bound[c]) and torch.equal(region.rect, fb.rect[c])
            assert region.xywh == tuple(fb.rect[c, :4].tolist())
    assert out["regions"][1][0].xywh == (0, 0, W, H)


# ---- the player --------------------------------------------------------------------------------------------------------------------------
def _with_krt(cam):
    """A copy of the test camera with the ``K``, ``R`` (stored transposed) and ``T`` a MOSS Camera carries."""
    import math
    c = copy.copy(cam)
    RT = cam.world_view_transform.t()[:3].cpu().numpy()
    H, W = int(cam.image_height), int(cam.image_width)
    c.K = np.array([[W / (2 * math.tan(cam.FoVx / 2)), 0, W / 2], [0, H / (2 * math.tan(cam.FoVy / 2)), H / 2], [0, 0, 1]], dtype=np.float32)
    c.R, c.T = RT[:, :3].T.copy(), RT[:, 3].copy()
    return c


def test_player_regions_and_split(gpu, hip_lib, world):
    from moss_amd.loss import ViewRegion
    from moss_amd.play import MossPlayer, evaluate_split
    from tests.test_gpu_player import _second_camera
    pc, cam, _ = _fresh(world)
    cams = [_with_krt(cam), _with_krt(_second_camera(cam, gpu))]
    H, W = world["H"], world["W"]
    plain = MossPlayer(pc, cams[0], world["bg"])
    base = {k: v.clone() for k, v in plain.frame(cams[1], _frame(1, gpu)).items()}
    assert "region" not in base
    player = MossPlayer(pc, cams[0], world["bg"], bounds=cams)
    alone = mb.FrameBounds(pc.SMPL_NEUTRAL, cams, H, W)
    for captured in (False, True):
        if captured:
            player.capture()
        for k in (1, 2):
            out = player.frame(cams[1], _frame(k, gpu))
            alone.update(_frame(k, gpu))
            region = out["region"]
            assert region.xywh is None and region is player.region_of(cams[1])
            assert torch.equal(region.bound, alone.bound[1]) and torch.equal(region.rect, alone.rect[1])
            assert torch.equal(player.region_of(cams[0]).bound, alone.bound[0])
            assert 0 < int(region.rect[4]) < H * W
            if k == 1:
                for key, v in base.items():
                    assert torch.equal(out[key], v), (captured, key)     # the render is what it was without bounds
    with pytest.raises(RuntimeError, match="without bounds"):
        plain.region_of(cams[0])
    # a split whose regions come from the player equals the split given those regions
    views, explicit = [], []
    for k in range(2):
        for c in range(2):
            v = copy.copy(cams[c])
            v.smpl_param, v.pose_id = _frame(k, gpu), 20 + k
            views.append(v)
            alone.update(v.smpl_param)
            explicit.append(ViewRegion.from_device(alone.bound[c].clone(), alone.rect[c].clone()))
    g = torch.Generator().manual_seed(32)
    gts = [torch.rand(3, H, W, generator=g).to(gpu) for _ in views]
    a = evaluate_split(player, views, gts, "pose", keep_tables=False)
    b = evaluate_split(player, views, gts, explicit, keep_tables=False)
    c = evaluate_split(player, views, gts, None, keep_tables=False)
    print("\nsplit by pose regions " + ", ".join(f"{k} {a[k]!r}" for k in ("l1", "psnr", "ssim", "n")))
    for k in ("l1", "psnr", "ssim", "n"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert a["l1"] != c["l1"]
    with pytest.raises(RuntimeError, match="without bounds"):
        evaluate_split(plain, views, gts, "pose")
