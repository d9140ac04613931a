"""``moss_amd.play`` and the pose-table file of ``moss_amd.checkpoint`` without a GPU: the 8-bit quantisation in torch against the two
expressions it stands for, at every rounding boundary; the PNG writer and reader; the pose tables' two file forms."""
import os
import pickle

import numpy as np
import pytest
import torch


def boundary_values():
    """The float32 inputs at which an 8-bit quantisation can go wrong: for every k in 0..255 the floats nearest k/255 and (k+0.5)/255
    with their two neighbours on either side; -0.0, a subnormal, -1, 2, +-inf, NaN; 4 096 random values around [0, 1]."""
    k = np.arange(256, dtype=np.float64)
    centres = np.concatenate((k / 255.0, (k + 0.5) / 255.0)).astype(np.float32)
    vals = [centres]
    for direction in (-np.inf, np.inf):
        step = centres
        for _ in range(2):
            step = np.nextafter(step, np.float32(direction), dtype=np.float32)
            vals.append(step)
    special = np.array([-0.0, 1e-42, -1.0, 2.0, np.inf, -np.inf, np.nan], dtype=np.float32)
    rng = np.random.default_rng(5)
    vals += [special, rng.uniform(-0.25, 1.25, 4096).astype(np.float32)]
    return torch.from_numpy(np.concatenate(vals))


def expected_u8(x, rounding):
    """The two torch expressions of the issue, element for element; NaN (whose conversion to uint8 torch leaves undefined) gives 0."""
    if rounding == "nearest":
        q = x.clone().mul(255).add_(0.5).clamp_(0, 255)              # torchvision.utils.save_image
    else:
        q = torch.clamp(x, 0, 1) * 255                               # train_ZJU.py:75
    q[torch.isnan(x)] = 0
    return q.to(torch.uint8)


def as_image(values, H, W):
    """``values`` tiled into a (3,H,W) image (each channel starts at another offset)."""
    n = H * W
    idx = (torch.arange(3 * n) * 7 + 3) % values.numel()
    return values[idx].reshape(3, H, W).contiguous()


@pytest.mark.parametrize("rounding", ["nearest", "truncate"])
def test_quantisation_equals_the_torch_expression_at_every_boundary(rounding):
    from moss_amd.play import frames_to_u8_torch
    v = boundary_values()
    assert v.numel() == 512 * 5 + 7 + 4096 and int(torch.isnan(v).sum()) == 1
    W = v.numel()
    image = torch.stack((v, v.flip(0), v.roll(17))).reshape(3, 1, W)
    got = frames_to_u8_torch(image, rounding=rounding)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, W, 3)
    assert torch.equal(got, expected_u8(image, rounding).permute(1, 2, 0))
    # what the boundaries are: k/255 maps to k in both; (k+0.5)/255 goes up for nearest at or above the tie only
    k = torch.arange(256, dtype=torch.float64)
    exact = (k / 255).to(torch.float32).reshape(1, 1, 256).expand(3, 1, 256).contiguous()
    assert torch.equal(frames_to_u8_torch(exact, rounding="nearest")[0, :, 0].long(), k.long())
    special = frames_to_u8_torch(torch.tensor([-0.0, 1e-42, -1.0, 2.0, float("inf"), float("-inf"), float("nan")]).reshape(1, 1, 7)
                                 .expand(3, 1, 7).contiguous(), rounding=rounding)
    assert special[0, :, 1].tolist() == [0, 0, 0, 255, 255, 0, 0]


def test_fill_by_a_mask_and_the_rgba_layout():
    from moss_amd.play import frames_to_u8_torch
    g = torch.Generator().manual_seed(3)
    H, W = 5, 7
    image, alpha = torch.rand(3, H, W, generator=g) * 1.2 - 0.1, torch.rand(1, H, W, generator=g)
    bound = (torch.rand(H, W, generator=g) > 0.4).to(torch.uint8)
    bound[0, 0], bound[0, 1] = 0, 2                                   # (anything but 1 is outside, as moss_eval_metrics)
    for fill in (0.0, 1.0):
        for rounding in ("nearest", "truncate"):
            rgb = frames_to_u8_torch(image, regions=bound, fill=fill, rounding=rounding)
            want = expected_u8(image, rounding).permute(1, 2, 0).clone()
            want[bound != 1] = 255 if fill else 0
            assert torch.equal(rgb, want)
            rgba = frames_to_u8_torch([image], alphas=[alpha], regions=[bound], fill=fill, rounding=rounding)[0]
            assert tuple(rgba.shape) == (H, W, 4) and torch.equal(rgba[..., :3], want)
            assert torch.equal(rgba[..., 3], expected_u8(alpha[0], rounding))      # alpha: quantised alike, never filled
    out = torch.zeros(H, W, 3, dtype=torch.uint8)
    assert frames_to_u8_torch(image, out=out) is out and torch.equal(out, expected_u8(image, "nearest").permute(1, 2, 0))
    with pytest.raises(ValueError, match="rounding"):
        frames_to_u8_torch(image, rounding="floor")


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (33, 17)])
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_png_round_trip(tmp_path, shape, channels):
    from moss_amd.play import read_png, save_png
    rng = np.random.default_rng(shape[0] * 10 + channels)
    a = rng.integers(0, 256, shape + ((channels,) if channels > 1 else ()), dtype=np.uint8)
    path = str(tmp_path / "sub" / "a.png")
    save_png(path, a)
    back = read_png(path)
    assert back.dtype == np.uint8 and back.shape == a.shape and np.array_equal(back, a)
    save_png(path, torch.from_numpy(a))                               # a CPU tensor, over the existing file
    assert np.array_equal(read_png(path), a)
    assert os.listdir(os.path.dirname(path)) == ["a.png"]


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_pil_decodes_the_same_pixels(tmp_path, channels):
    Image = pytest.importorskip("PIL.Image")
    from moss_amd.play import save_png
    for shape in ((1, 1), (5, 7), (33, 17)):
        a = np.random.default_rng(channels).integers(0, 256, shape + ((channels,) if channels > 1 else ()), dtype=np.uint8)
        path = save_png(str(tmp_path / f"{shape[0]}.png"), a)
        with Image.open(path) as im:
            assert im.mode == {1: "L", 3: "RGB", 4: "RGBA"}[channels] and np.array_equal(np.asarray(im), a)


def test_png_reader_refuses_what_the_writer_does_not_write(tmp_path):
    from moss_amd.play import read_png, save_png
    with pytest.raises(ValueError, match="uint8"):
        save_png(str(tmp_path / "f.png"), np.zeros((4, 4, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="uint8"):
        save_png(str(tmp_path / "f.png"), np.zeros((4, 4, 2), dtype=np.uint8))
    path = str(tmp_path / "not.png")
    open(path, "wb").write(b"ply\n")
    with pytest.raises(ValueError, match="no PNG"):
        read_png(path)
    good = str(tmp_path / "good.png")
    rng = np.random.default_rng(1)
    save_png(good, rng.integers(0, 256, (9, 11, 3), dtype=np.uint8))
    data = open(good, "rb").read()
    open(path, "wb").write(data[:-20])
    with pytest.raises(ValueError):
        read_png(path)
    # a valid PNG of another kind, made by hand: 2 x 2 greyscale whose second scanline uses filter type 1 (Sub)
    import struct
    import zlib

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)

    def png(header, scanlines):
        return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", header) + chunk(b"IDAT", zlib.compress(scanlines)) + chunk(b"IEND", b"")
    open(path, "wb").write(png(struct.pack(">IIBBBBB", 2, 2, 8, 0, 0, 0, 0), bytes([0, 10, 20, 0, 30, 40])))
    assert read_png(path).tolist() == [[10, 20], [30, 40]]
    open(path, "wb").write(png(struct.pack(">IIBBBBB", 2, 2, 8, 0, 0, 0, 0), bytes([0, 10, 20, 1, 30, 10])))
    with pytest.raises(ValueError, match="filter"):
        read_png(path)
    open(path, "wb").write(png(struct.pack(">IIBBBBB", 2, 2, 8, 0, 0, 0, 1), bytes([0, 10, 20, 0, 30, 40])))
    with pytest.raises(ValueError, match="interlaced"):
        read_png(path)
    open(path, "wb").write(png(struct.pack(">IIBBBBB", 2, 2, 16, 0, 0, 0, 0), bytes([0, 0, 10, 0, 20, 0, 0, 30, 0, 40])))
    with pytest.raises(ValueError, match="bit depth"):
        read_png(path)


def test_png_reader_refuses_a_foreign_encoder(tmp_path):
    """PIL's default encoder picks adaptive scanline filters for a smooth picture; its palette and 16-bit forms are other kinds."""
    from moss_amd.play import read_png
    Image = pytest.importorskip("PIL.Image")
    yy, xx = np.mgrid[0:40, 0:48]
    smooth = np.stack((yy * 3 + xx, yy + xx * 2, 255 - yy * 2 - xx), -1).astype(np.uint8)
    foreign = str(tmp_path / "foreign.png")
    Image.fromarray(smooth).save(foreign)
    with pytest.raises(ValueError, match="filter"):
        read_png(foreign)
    Image.fromarray(smooth).convert("P").save(foreign)
    with pytest.raises(ValueError, match="palette|colour type"):
        read_png(foreign)
    Image.fromarray(smooth[..., 0].astype(np.uint16) * 257).save(foreign)
    with pytest.raises(ValueError, match="bit depth"):
        read_png(foreign)


def test_a_png_writer_that_dies_leaves_no_half_file(tmp_path, monkeypatch):
    from moss_amd import play
    path = str(tmp_path / "x.png")
    play.save_png(path, np.full((3, 3), 7, dtype=np.uint8))
    before = open(path, "rb").read()

    def dies(*a, **k):
        raise OSError("disk full")
    monkeypatch.setattr(play.zlib, "compress", dies)
    with pytest.raises(OSError):
        play.save_png(path, np.zeros((3, 3), dtype=np.uint8))
    with pytest.raises(OSError):
        play.save_png(str(tmp_path / "y.png"), np.zeros((3, 3), dtype=np.uint8))
    assert open(path, "rb").read() == before and not os.path.exists(str(tmp_path / "y.png"))


def _tables(P, seed):
    g = torch.Generator().manual_seed(seed)
    return {pid: {"transforms": torch.randn(1, P, 3, 3, generator=g), "translation": torch.randn(1, P, 3, generator=g)}
            for pid in (0, 30, 7)}


def test_pose_tables_round_trip(tmp_path):
    from moss_amd.checkpoint import load_pose_tables, save_pose_tables
    model = str(tmp_path / "model")
    by_split = {"train": _tables(11, 1), "test": _tables(11, 2)}
    pth, pkl = save_pose_tables(model, 2500, by_split)
    assert pth == os.path.join(model, "smpl_rot", "iteration_2500", "pose_tables.pth") and pkl is None
    raw = torch.load(pth, map_location="cpu", weights_only=True)      # plain containers and tensors only
    assert set(raw["tables"]) == {"train", "test"}
    save_pose_tables(model, 300, {"test": _tables(11, 3)})
    back = load_pose_tables(model)                                    # iteration=-1: the largest
    assert set(back) == {"train", "test"}
    for split in by_split:
        assert list(back[split]) == [0, 30, 7]
        for pid, e in by_split[split].items():
            assert tuple(back[split][pid]["transforms"].shape) == (1, 11, 3, 3) and tuple(back[split][pid]["translation"].shape) == (1, 11, 3)
            assert torch.equal(back[split][pid]["transforms"], e["transforms"]) and torch.equal(back[split][pid]["translation"], e["translation"])
    assert set(load_pose_tables(model, iteration=300)) == {"test"}
    assert torch.equal(load_pose_tables(pth)["test"][7]["translation"], by_split["test"][7]["translation"])
    with pytest.raises(ValueError, match=r"\(1,P,3,3\)"):
        save_pose_tables(model, 1, {"test": {0: {"transforms": torch.zeros(11, 3, 3), "translation": torch.zeros(11, 3)}}})


def test_moss_pickle_is_written_as_moss_writes_it_and_not_read_untrusted(tmp_path):
    from moss_amd.checkpoint import load_pose_tables, save_pose_tables
    model = str(tmp_path / "model")
    by_split = {"train": _tables(5, 4), "test": _tables(5, 5)}
    pth, pkl = save_pose_tables(model, 3000, by_split, moss_pickle=True)
    assert pkl == os.path.join(model, "smpl_rot", "iteration_3000", "smpl_rot.pickle") and os.path.exists(pth)
    with open(pkl, "rb") as f:                                        # render_ZJU.py:42-47
        smpl_rot = pickle.load(f)
    assert set(smpl_rot) == {"train", "test"}
    for split in by_split:
        for pid, e in by_split[split].items():
            assert set(smpl_rot[split][pid]) == {"transforms", "translation"}
            assert torch.equal(smpl_rot[split][pid]["transforms"], e["transforms"])
            assert smpl_rot[split][pid]["translation"].device == e["translation"].device
    with pytest.raises(ValueError, match="trust_pickle"):
        load_pose_tables(pkl)
    assert torch.equal(load_pose_tables(pkl, trust_pickle=True)["test"][30]["transforms"], by_split["test"][30]["transforms"])
    os.remove(pth)                                                    # a directory that holds MOSS's file alone
    with pytest.raises(ValueError, match="trust_pickle"):
        load_pose_tables(model)


def test_the_header_declares_the_frame_kernel_and_the_binding_knows_it(hip_lib):
    from moss_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "moss_raster.h")).read()
    assert "int moss_frames_to_u8(const moss_frames_to_u8_args* args, void* stream);" in text
    assert hasattr(hip_lib, "moss_frames_to_u8") and hip_lib.moss_frames_to_u8.argtypes is not None
    import ctypes
    assert ctypes.sizeof(_lib.FramesToU8Args) == 24 + 3 * 64 + 8 + 64
