"""CPU-only tests of the frame-bounds ops (C ABI moss_smpl_vertices / moss_bound_mask, moss_amd.bounds): the CPU statements against
the reference's own numbers (tests/golden/frame_bounds.npz) and against a brute-force per-pixel evaluation of the mask rules, the
symbols, declarations and ctypes blocks, the refusals of both entry points, and ``ViewRegion.from_device``.

The vertex bar is the project's for this chain (tests/test_lbs_cpu.py): 64 eps32 s, s the tensor's largest magnitude."""
import ctypes
import os
import re
import sys
import threading

import numpy as np
import pytest
import torch

from moss_amd import bounds as mb
from moss_amd.loss import ViewRegion, bounding_rect
from tests.helpers import c_layout, ctypes_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_frame_bounds as gen  # noqa: E402

EPS32 = float(np.finfo(np.float32).eps)
NAMES = ("moss_smpl_vertices", "moss_smpl_vertices_workspace_bytes", "moss_bound_mask", "moss_bound_mask_workspace_bytes")


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "frame_bounds.npz"))
    assert str(z["body_sha256"]) == gen.body_sha256(), "synthetic_body_model no longer makes the body the fixture was generated from"
    return z


def test_float64_torch_form_against_the_reference(golden):
    body = gen.golden_body(torch.float64)
    for f in range(len(gen.FRAME_SEEDS)):
        frame, pad = gen.golden_frame(f)
        for k in ("poses", "shapes", "R", "Th"):
            np.testing.assert_array_equal(frame[k].numpy(), golden[k][f])
        wv, wb, jt = mb.posed_vertices_torch(body, {k: v.double() for k, v in frame.items()}, pad)
        for name, got, ref in (("vertices", wv, golden["vertices"][f]), ("joints", jt, golden["joints"][f]),
                               ("world_bound", wb, golden["world_bound"][f])):
            bar = 64 * EPS32 * float(np.abs(ref).max())
            err = float(np.abs(got.numpy() - ref).max())
            print(f"frame {f} {name}: error / bar = {err / bar:.4f}")
            assert err <= bar, (f, name, err, bar)


def test_projected_corners_equal_the_reference_all_of_them(golden):
    assert float(np.abs(golden["corners_unrounded"] - np.floor(golden["corners_unrounded"]) - 0.5).min()) >= 0.05
    for f in range(len(gen.FRAME_SEEDS)):
        corners, flags, xy = mb.project_corners_numpy(golden["world_bound"][f], golden["K"][f], golden["RT"][f], return_unrounded=True)
        np.testing.assert_array_equal(corners, golden["corners"][f])
        np.testing.assert_array_equal(flags, 0)
        assert float(np.abs(xy - golden["corners_unrounded"][f]).max()) < 1e-9
        one, flag = mb.project_corners_numpy(golden["world_bound"][f], golden["K"][f, 1], golden["RT"][f, 1])
        np.testing.assert_array_equal(one, golden["corners"][f, 1])
        assert flag == 0


def test_flags_and_clamp_of_the_projection():
    wb = np.array([[-1, -1, -1], [1, 1, 1]], dtype=np.float32)
    K = np.array([[500, 0, 32], [0, 500, 32], [0, 0, 1]], dtype=np.float32)
    RT = np.concatenate([np.eye(3), [[0], [0], [0.5]]], 1).astype(np.float32)             # the camera sits inside the box
    corners, flag = mb.project_corners_numpy(wb, K, RT)
    assert flag == 1 and np.abs(corners).max() <= mb.CORNER_LIMIT
    RT[2, 3] = 1.0                                                                          # corners at depth 0: a division by zero
    corners, flag = mb.project_corners_numpy(wb, K, RT)
    assert flag == 1 and np.abs(corners).max() == mb.CORNER_LIMIT
    RT[2, 3] = 1.0 + 1e-4                                                                   # in front, but 5e6 pixels out
    corners, flag = mb.project_corners_numpy(wb, K, RT)
    assert flag == 1 and np.abs(corners).max() == mb.CORNER_LIMIT
    RT[2, 3] = 5.0
    assert mb.project_corners_numpy(wb, K, RT)[1] == 0


def brute_force_mask(corners, H, W):
    """Rules (a) and (b) of include/moss_raster.h, pixel by pixel, in Python integers."""
    q = [(int(x), int(y)) for x, y in np.asarray(corners).reshape(8, 2)]
    out = np.zeros((H, W), dtype=np.uint8)
    for y in range(H):
        for x in range(W):
            for face in mb.FACES:
                f = [q[i] for i in face]
                xs, ys = [p[0] for p in f], [p[1] for p in f]
                if not (min(xs) <= x <= max(xs) and min(ys) <= y <= max(ys)):
                    continue
                crosses, edge = [], False
                for k in range(4):
                    (x0, y0), (x1, y1) = f[k], f[(k + 1) % 4]
                    dx, dy = x1 - x0, y1 - y0
                    cr = dx * (y - y0) - dy * (x - x0)
                    crosses.append(cr)
                    if min(x0, x1) <= x <= max(x0, x1) and min(y0, y1) <= y <= max(y0, y1) and abs(2 * cr) <= max(abs(dx), abs(dy)):
                        edge = True
                if all(c >= 0 for c in crosses) or all(c <= 0 for c in crosses) or edge:
                    out[y, x] = 1
                    break
    return out


def box_corners(x0, y0, x1, y1, skew=(0, 0)):
    """Eight 2D corners of a box-like solid: the front face (x0..x1, y0..y1) and a back face moved by ``skew``, in
    get_bound_corners' order (x <- bit 2, y <- bit 1, z <- bit 0)."""
    c = np.zeros((8, 2), dtype=np.int64)
    for i in range(8):
        c[i] = ((x1 if i & 4 else x0) + (skew[0] if i & 1 else 0), (y1 if i & 2 else y0) + (skew[1] if i & 1 else 0))
    return c


def mask_cases(H, W):
    """name -> corners: a box inside, one crossing each border, one outside, a face collapsed to a segment, a single-pixel box."""
    cases = {
        "inside": box_corners(W // 4, H // 4, W // 2, H // 2, (W // 5, H // 6)),
        "left": box_corners(-W // 3, H // 4, W // 3, H // 2, (2, 1)),
        "right": box_corners(W // 2, H // 4, W + W // 3, H // 2, (1, 2)),
        "top": box_corners(W // 4, -H // 2, W // 2, H // 3, (2, -1)),
        "bottom": box_corners(W // 4, H // 2, W // 2, H + H // 2, (-2, 1)),
        "outside": box_corners(W + 3, H + 2, W + 9, H + 7, (2, 2)),
        "segment": box_corners(1, 1, 1, H - 2, (W - 3, 0)),          # the faces x = min / max collapse to segments
        "pixel": box_corners(W // 2, H // 2, W // 2, H // 2),
        "slanted": np.array([[1, 2], [W - 2, 0], [0, H - 3], [W - 3, H - 1], [3, 3], [W - 4, 2], [2, H - 4], [W - 5, H - 2]], dtype=np.int64),
    }
    return cases


@pytest.mark.parametrize("H,W", [(7, 9), (20, 33)])
def test_mask_against_brute_force(H, W):
    for name, corners in mask_cases(H, W).items():
        bound, rect = mb.bound_mask_numpy(corners, H, W)
        ref = brute_force_mask(corners, H, W)
        np.testing.assert_array_equal(bound, ref, err_msg=name)
        x, y, w, h = bounding_rect(torch.tensor(bound))
        assert tuple(rect[:4]) == (x, y, w, h), name
        assert rect[4] == bound.sum(), name
        for cx, cy in corners:
            if 0 <= cx < W and 0 <= cy < H:
                assert bound[cy, cx] == 1, (name, cx, cy)
        if name == "outside":
            assert tuple(rect) == (0, 0, 0, 0, 0)
        if name == "pixel":
            assert tuple(rect) == (W // 2, H // 2, 1, 1, 1)
        if name == "segment":
            assert bound.sum() > 0
    full, rect = mb.bound_mask_numpy(mask_cases(H, W)["outside"], H, W, flagged=True)
    assert full.all() and tuple(rect) == (0, 0, W, H, W * H)


def test_pil_polygons_printed_not_asserted():
    """The symmetric difference against PIL's ImageDraw.polygon fills (another rasteriser's convention, not cv2's): printed."""
    try:
        from PIL import Image, ImageDraw
    except ImportError:
        print("PIL is not importable: nothing to print")
        return
    H, W = 20, 33
    for name, corners in mask_cases(H, W).items():
        img = Image.new("L", (W, H), 0)
        draw = ImageDraw.Draw(img)
        for face in mb.FACES:
            draw.polygon([tuple(int(v) for v in corners[i]) for i in face], fill=1, outline=1)
        pil = np.asarray(img, dtype=np.uint8)
        ours = mb.bound_mask_numpy(corners, H, W)[0]
        print(f"{name}: ours {int(ours.sum())} px, PIL {int(pil.sum())} px, ours only {int((ours & ~pil & 1).sum())}, "
              f"PIL only {int((pil & ~ours & 1).sum())}")


def test_symbols_exported_and_declared(hip_lib):
    text = open(os.path.join(ROOT, "include", "moss_raster.h")).read()
    assert re.search(r"#define\s+MOSS_ABI_VERSION\s+7\b", text)
    from moss_amd import _lib
    assert _lib.ABI_VERSION == 7 and hip_lib.moss_abi_version() == 7
    diag = re.search(r"#ifdef MOSS_DIAG\n(.*?)#endif", text, flags=re.S).group(0)
    public = re.sub(r"/\*.*?\*/", "", text.replace(diag, ""), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, public), name
        assert hasattr(hip_lib, name), name
        assert getattr(hip_lib, name).argtypes is not None, name
    assert "} moss_smpl_vertices_args;" in public and "} moss_bound_mask_args;" in public
    for cite in ("smpl/smpl_numpy.py:46-98", "scene/dataset_readers.py:428-436", ":331-339", "scene/dataset_readers.py:1034-1045",
                 ":1008-1021", ":1023-1032", "train_ZJU.py:115"):
        assert cite in text, cite
    assert "frame_bounds.hip" in open(os.path.join(ROOT, "moss_amd", "build.py")).read()


@pytest.mark.parametrize("cname,pyname", [("moss_smpl_vertices_args", "SmplVerticesArgs"), ("moss_bound_mask_args", "BoundMaskArgs")])
def test_ctypes_blocks_match_the_c_layout(tmp_path, cname, pyname):
    from moss_amd import _lib
    cls = getattr(_lib, pyname)
    assert c_layout(tmp_path, cname, [f[0] for f in cls._fields_]) == ctypes_layout(cls)


def test_workspace_sizes_are_monotonic_host_functions(hip_lib):
    wv, wm = hip_lib.moss_smpl_vertices_workspace_bytes, hip_lib.moss_bound_mask_workspace_bytes
    for bad in ((0, 24), (-1, 24), (6890, 0), (6890, 65)):
        assert wv(*bad) == 0, bad
    assert wv(6890, 24) >= 6890 * 3 * 8 and wv(6890, 24) % 256 == 0
    assert wv(1, 1) > 0 and wv(100, 24) <= wv(6890, 24) <= wv(20000, 24) and wv(6890, 2) <= wv(6890, 24) <= wv(6890, 64)
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (65536, 8, 8), (1, 65536, 32768)):
        assert wm(*bad) == 0, bad
    assert wm(1, 1, 1) > 0 and wm(1, 512, 512) <= wm(4, 512, 512) <= wm(4, 1024, 1024)
    assert wm(3, 130, 70) >= 3 * (2 * 17) * 5 * 4                    # 5 words per 64 x 8 tile (2 across 70, 17 down 130) and camera


def test_c_abi_refuses_bad_arguments_naming_the_field(hip_lib):
    """Host-side validation needs no device (in a thread of its own: the error text is per thread)."""
    failures = []

    def run():
        try:
            _refusals(hip_lib)
        except BaseException as e:                                # noqa: BLE001
            failures.append(e)

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if failures:
        raise failures[0]


def _refusals(lib):
    from moss_amd._lib import BoundMaskArgs, SmplVerticesArgs
    err = lib.moss_last_error
    assert lib.moss_smpl_vertices(None, None) == -1 and b"moss_smpl_vertices: null argument block" in err()
    a = SmplVerticesArgs()
    a.V, a.J = 0, 24
    assert lib.moss_smpl_vertices(ctypes.byref(a), None) == -1 and b"moss_smpl_vertices: V must be >= 1" in err()
    a.V = 10
    for J in (0, 65):
        a.J = J
        assert lib.moss_smpl_vertices(ctypes.byref(a), None) == -1 and b"moss_smpl_vertices: J must be 1..64" in err()
    a.J, a.num_betas, a.shapedirs_stride = 3, 11, 10
    assert lib.moss_smpl_vertices(ctypes.byref(a), None) == -1 and b"num_betas" in err()
    a.num_betas = 10
    assert lib.moss_smpl_vertices(ctypes.byref(a), None) == -1 and b"null body-model array" in err() and b"weights" in err()
    a.v_template = a.shapedirs = a.posedirs = a.J_regressor = a.weights = 256          # (never dereferenced on the host)
    assert lib.moss_smpl_vertices(ctypes.byref(a), None) == -1 and b"null frame input" in err() and b"pad" in err()
    a.poses = a.shapes = a.R = a.Th = a.pad = 256
    assert lib.moss_smpl_vertices(ctypes.byref(a), None) == -1 and b"null output (world_vertex, world_bound)" in err()
    a.world_vertex = a.world_bound = 256
    a.parents[1], a.parents[2] = 0, 2
    assert lib.moss_smpl_vertices(ctypes.byref(a), None) == -1 and b"parents[j] must be in [0, j)" in err()
    a.parents[2] = 1
    assert lib.moss_smpl_vertices(ctypes.byref(a), None) == -1 and b"moss_smpl_vertices_workspace_bytes" in err()
    assert lib.moss_bound_mask(None, None) == -1 and b"moss_bound_mask: null argument block" in err()
    b = BoundMaskArgs()
    b.C, b.H, b.W = 0, 8, 8
    assert lib.moss_bound_mask(ctypes.byref(b), None) == -1 and b"moss_bound_mask: C must be 1..65535" in err()
    b.C = 1
    for H, W in ((0, 8), (8, 0), (65536, 32768)):
        b.H, b.W = H, W
        assert lib.moss_bound_mask(ctypes.byref(b), None) == -1 and b"H and W must be >= 1 with H * W < 2^31" in err()
    b.H, b.W = 8, 8
    assert lib.moss_bound_mask(ctypes.byref(b), None) == -1 and b"null input (world_bound, K, RT)" in err()
    b.world_bound = b.K = b.RT = 256
    assert lib.moss_bound_mask(ctypes.byref(b), None) == -1 and b"null output (bound, rect, corners, flags)" in err()
    b.bound = b.rect = b.corners = b.flags = 256
    assert lib.moss_bound_mask(ctypes.byref(b), None) == -1 and b"moss_bound_mask_workspace_bytes" in err()


def test_python_surface_refuses_cpu_tensors_and_bad_inputs(hip_lib):
    from moss_amd import lbs as mlbs
    body = mlbs.synthetic_body_model(32, 24, seed=3)
    fr = mlbs.synthetic_frame(1, 24)
    with pytest.raises(ValueError, match="must be on a GPU.*posed_vertices_torch"):
        mb.posed_vertices(body, fr)
    with pytest.raises(ValueError, match="float32"):
        mb.posed_vertices({**body, "posedirs": body["posedirs"].double()}, fr)
    with pytest.raises(ValueError, match="contiguous"):
        mb.posed_vertices({**body, "J_regressor": body["J_regressor"].t().contiguous().t()}, fr)
    with pytest.raises(ValueError, match="requires grad"):
        mb.posed_vertices({**body, "weights": body["weights"].clone().requires_grad_(True)}, fr)
    with pytest.raises(ValueError, match="1..64"):
        mb.posed_vertices(mlbs.synthetic_body_model(70, 65, seed=3), mlbs.synthetic_frame(1, 65))
    with pytest.raises(ValueError, match="must be on a GPU.*bound_mask_numpy"):
        mb.bound_masks(torch.zeros(2, 3), torch.zeros(1, 3, 3), torch.zeros(1, 3, 4), 8, 8)


def test_camera_krt_undoes_the_stored_transpose():
    from types import SimpleNamespace
    rng = np.random.Generator(np.random.PCG64(5))
    w2c = rng.normal(size=(3, 4))
    cam = SimpleNamespace(K=rng.normal(size=(3, 3)), R=np.transpose(w2c[:, :3]), T=w2c[:, 3])     # dataset_readers.py:396-397
    K, RT = mb.camera_KRT(cam)
    assert K.dtype == RT.dtype == torch.float32 and tuple(K.shape) == (3, 3) and tuple(RT.shape) == (3, 4)
    np.testing.assert_array_equal(RT.numpy(), w2c.astype(np.float32))
    np.testing.assert_array_equal(K.numpy(), cam.K.astype(np.float32))


def test_view_region_from_device_and_read():
    bound = torch.zeros((6, 8), dtype=torch.uint8)
    bound[2:5, 1:4] = 1
    rect = torch.tensor([1, 2, 3, 3, 9], dtype=torch.int32)
    region = ViewRegion.from_device(bound, rect)
    assert region.bound.data_ptr() == bound.data_ptr() and region.rect.data_ptr() == rect.data_ptr() and region.xywh is None
    from moss_amd.loss import region_xywh
    from moss_amd.lpips import crop_capacity
    with pytest.raises(RuntimeError, match=r"has not been read on the host.*region\.read\(\)"):
        crop_capacity([region])
    with pytest.raises(RuntimeError, match=r"MossStep.*region\.read\(\)"):
        region_xywh(region, "MossStep")
    assert region.read() is region and region.xywh == (1, 2, 3, 3)
    assert crop_capacity([region]) == (3, 3)
    same = ViewRegion(bound)
    assert same.xywh == region.xywh and torch.equal(same.rect, region.rect) and torch.equal(same.bound, region.bound)
    other = ViewRegion.from_device(bound.clone(), rect.clone()).read([4, 5, 6, 7, 42])
    assert other.xywh == (4, 5, 6, 7)
    with pytest.raises(ValueError, match="uint8"):
        ViewRegion.from_device(bound.float(), rect)
    with pytest.raises(ValueError, match="int32"):
        ViewRegion.from_device(bound, rect.long())
