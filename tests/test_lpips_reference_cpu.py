"""The LPIPS reference (the ground truth's tapped activations, computed once: ``moss_lpips_vgg_reference`` / ``_forward_ref`` of the C
ABI, ``LpipsReference`` of moss_amd.lpips), without a GPU: the ctypes mirrors of the two new argument blocks against the header as a C
compiler lays them out, the block's size, the host-side refusals of the six entry points (before any launch, so no device is needed),
and the new keywords."""
import ctypes
import inspect
import os

import pytest

from moss_amd import lpips as mlp
from tests.helpers import c_layout, ctypes_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUFFIXES = ("", "_bf16", "_bf16x3")
FAKE = 0x1000                                                            # a non-NULL pointer no refused call ever follows


@pytest.mark.parametrize("cname, pyname", [("moss_lpips_vgg_reference_args", "LpipsVggReferenceArgs"),
                                           ("moss_lpips_vgg_forward_ref_args", "LpipsVggForwardRefArgs")])
def test_argument_blocks_mirror_the_header(tmp_path, cname, pyname):
    """sizeof and every offsetof as gcc sees the header; the two-image blocks and the ABI version did not move."""
    import moss_amd._lib as L
    cls = getattr(L, pyname)
    fields = [f[0] for f in cls._fields_]
    assert "reference" in fields and "reference_bytes" in fields and fields[-2:] == ["cap_H", "cap_W"]
    assert c_layout(tmp_path, cname, fields) == ctypes_layout(cls)
    text = open(os.path.join(ROOT, "include", "moss_raster.h")).read()
    assert "#define MOSS_ABI_VERSION 7" in text
    assert cls().cap_H == 0 and cls().cap_W == 0
    assert [f[0] for f in L.LpipsVggArgs._fields_][:2] == ["x", "y"]


def test_the_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "moss_raster.h")).read()
    assert "size_t moss_lpips_vgg_reference_bytes(int H, int W);" in text
    for s in SUFFIXES:
        assert f"int moss_lpips_vgg_reference{s}(const moss_lpips_vgg_reference_args* args, void* stream);" in text
        assert f"int moss_lpips_vgg_forward_ref{s}(const moss_lpips_vgg_forward_ref_args* args, void* stream);" in text


def test_reference_bytes(hip_lib):
    """Five regions, each (H >> l)(W >> l) C_l floats rounded up to 256 bytes; 0 for a size the calls refuse."""
    align = lambda n: (n + 255) // 256 * 256                             # noqa: E731
    for H, W in ((16, 16), (37, 53), (101, 77), (256, 176)):
        want = sum(align((H >> l) * (W >> l) * c * 4) for l, c in enumerate(mlp.TAP_CHANNELS))
        assert hip_lib.moss_lpips_vgg_reference_bytes(H, W) == want == mlp.reference_bytes(H, W), (H, W)
    assert mlp.reference_bytes(256, 176) == 21987328                     # 22 MB: 122 floats per pixel
    for H, W in ((15, 16), (16, 15), (4096, 4096), (1 << 16, 16), (16, 1 << 17)):
        assert hip_lib.moss_lpips_vgg_reference_bytes(H, W) == 0, (H, W)


def _block(kind, **change):
    """A block every check accepts (fake non-NULL pointers: a refused call follows none; an accepted one is never made here)."""
    from moss_amd._lib import LpipsVggForwardRefArgs, LpipsVggReferenceArgs
    from moss_amd._lib import lib
    L = lib()
    a = LpipsVggReferenceArgs() if kind == "reference" else LpipsVggForwardRefArgs()
    a.H, a.W = 37, 53
    for i in range(13):
        a.weights[i], a.biases[i] = FAKE, FAKE
    a.shift = a.scale = FAKE
    a.reference, a.reference_bytes = FAKE, L.moss_lpips_vgg_reference_bytes(37, 53)
    a.workspace, a.workspace_bytes = FAKE, L.moss_lpips_vgg_workspace_bytes(37, 53)
    if kind == "reference":
        a.y = FAKE
    else:
        a.x = a.out = FAKE
        for i in range(5):
            a.lin[i] = FAKE
    for k, v in change.items():
        if "[" in k:
            name, i = k[:-1].split("[")
            getattr(a, name)[int(i)] = v
        else:
            setattr(a, k, v)
    return a


@pytest.mark.parametrize("suffix", SUFFIXES)
@pytest.mark.parametrize("kind", ["reference", "forward_ref"])
def test_host_refusals(hip_lib, kind, suffix):
    """MOSS_ERR_INVALID_ARG with the field named, before any launch: no device is touched (this test runs without one)."""
    name = f"moss_lpips_vgg_{kind}{suffix}"
    fn = getattr(hip_lib, name)

    def refused(block, text):
        rc = fn(ctypes.byref(block) if block is not None else None, None)
        msg = hip_lib.moss_last_error().decode()
        assert rc == -1, (rc, msg, text)                                 # MOSS_ERR_INVALID_ARG
        assert msg.startswith(name + ":") and text in msg, (msg, text)

    refused(None, "null argument block")
    image = "y" if kind == "reference" else "x"
    refused(_block(kind, **{image: None}), "null " + image)
    if kind == "forward_ref":
        refused(_block(kind, out=None), "null out")
        for i in (0, 4):
            refused(_block(kind, **{f"lin[{i}]": None}), "null lin")
    refused(_block(kind, shift=None), "shift")
    refused(_block(kind, scale=None), "scale")
    for i in (0, 7, 12):
        refused(_block(kind, **{f"weights[{i}]": None}), "null weight or bias")
        refused(_block(kind, **{f"biases[{i}]": None}), "null weight or bias")
    good = _block(kind)
    refused(_block(kind, reference=None), "reference")
    refused(_block(kind, reference_bytes=good.reference_bytes - 1), "reference_bytes")
    refused(_block(kind, workspace=None), "workspace")
    refused(_block(kind, workspace_bytes=good.workspace_bytes - 1), "workspace")
    refused(_block(kind, cap_H=48, cap_W=64, frame_H=64, frame_W=64), "needs rect")
    refused(_block(kind, cap_H=48, rect=FAKE), "both be set")
    # a reference that would do for the crop but not for the capacity; and the size refusals of the two-image call
    refused(_block(kind, cap_H=48, cap_W=64, frame_H=64, frame_W=64, rect=FAKE, workspace_bytes=1 << 30), "reference_bytes")
    refused(_block(kind, H=15), ">= 16")
    refused(_block(kind, frame_H=36, frame_W=53), "frame is smaller")
    refused(_block(kind, cap_H=65, cap_W=64, frame_H=64, frame_W=64, rect=FAKE), "larger than the frame")


def test_signatures():
    from moss_amd.metrics import evaluate_views
    from moss_amd.train import MossStep
    assert inspect.signature(MossStep.__init__).parameters["lpips_reference"].default is None
    assert inspect.signature(evaluate_views).parameters["lpips_references"].default is None
    assert inspect.signature(mlp.lpips_vgg_roi_reference).parameters["capacity"].default is None
    for name in ("LpipsReference", "lpips_vgg_reference", "lpips_vgg_roi_reference", "reference_bytes", "reference_cache"):
        assert name in mlp.__all__ and hasattr(mlp, name)
    for method in ("empty", "copy_", "nbytes"):
        assert hasattr(mlp.LpipsReference, method)


def test_evaluate_views_refuses_references_that_are_not_float32():
    """Before anything is rendered, as a net that is not float32 is."""
    from moss_amd.metrics import evaluate_views
    net = object.__new__(mlp.LpipsVGG)
    net.precision = "f32"
    ref = mlp.LpipsReference(None, (16, 16), None, "bf16", 0)
    with pytest.raises(ValueError, match="float32 term"):
        evaluate_views(None, [], [], None, None, lpips=net, lpips_references=[ref])
    with pytest.raises(ValueError, match="needs lpips="):
        evaluate_views(None, [], [], None, None, lpips_references=[])
