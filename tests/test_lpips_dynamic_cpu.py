"""The LPIPS call whose crop size is read from the device (``capacity=``; ``cap_H``, ``cap_W`` of the C ABI), without a GPU: the ctypes
mirrors of the two argument blocks against the header as a C compiler lays them out, ``crop_capacity``, and the host-side refusals
of ``lpips_vgg_roi_fused(capacity=)``."""
import os

import pytest
import torch

from moss_amd import lpips as mlp
from tests.helpers import c_layout, ctypes_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _region(h, w, x=0, y=0, frame=(64, 64)):
    from moss_amd.loss import ViewRegion
    mask = torch.zeros(1, *frame)
    mask[:, y:y + h, x:x + w] = 1
    return ViewRegion(mask, rect=(x, y, w, h))


@pytest.mark.parametrize("cname, pyname", [("moss_lpips_vgg_args", "LpipsVggArgs"),
                                           ("moss_lpips_vgg_backward_args", "LpipsVggBackwardArgs")])
def test_argument_blocks_mirror_the_header(tmp_path, cname, pyname):
    """sizeof and every offsetof as gcc sees the header; cap_H, cap_W are the LAST two fields (an addition to ABI 7)."""
    import moss_amd._lib as L
    cls = getattr(L, pyname)
    fields = [f[0] for f in cls._fields_]
    assert fields[-2:] == ["cap_H", "cap_W"] and fields[-3] == "workspace_bytes"
    assert c_layout(tmp_path, cname, fields) == ctypes_layout(cls)
    text = open(os.path.join(ROOT, "include", "moss_raster.h")).read()
    assert "#define MOSS_ABI_VERSION 7" in text                          # the version did not move
    assert cls().cap_H == 0 and cls().cap_W == 0                          # a caller who sets neither makes the static call


def test_crop_capacity_is_the_per_axis_maximum():
    regions = [_region(37, 29), _region(16, 48, x=3), _region(20, 20, y=40)]
    assert mlp.crop_capacity(regions) == (37, 48)
    assert mlp.crop_capacity(iter(regions[:1])) == (37, 29)
    assert mlp.crop_capacity([_region(64, 64)]) == (64, 64)
    with pytest.raises(ValueError, match="no regions"):
        mlp.crop_capacity([])


def test_capacity_refusals_on_the_host():
    """A region larger than the capacity, capacities the kernels do not take, and CPU tensors (the op has no CPU path)."""
    x, y = torch.zeros(3, 64, 64), torch.zeros(3, 64, 64)
    for region, cap in ((_region(37, 29), (36, 48)), (_region(37, 29), (48, 28)), (_region(64, 64), (64, 48))):
        with pytest.raises(ValueError, match="exceeds the capacity"):
            mlp.lpips_vgg_roi_fused(object(), x, y, region, capacity=cap)
    for cap in ((15, 48), (48, 15), (65, 48), (48, 65), "whole"):
        with pytest.raises(ValueError, match="capacity must be"):
            mlp.lpips_vgg_roi_fused(object(), x, y, _region(20, 20), capacity=cap)
    net = object.__new__(mlp.LpipsVGG)                                    # (no weights: the images are refused before they are read)
    net.device = torch.device("cpu")
    for cap in ((48, 48), "frame"):
        with pytest.raises(RuntimeError, match="on a GPU"):
            mlp.lpips_vgg_roi_fused(net, x, y, _region(37, 29), capacity=cap)
    with pytest.raises(TypeError, match="must be an LpipsVGG"):
        mlp.lpips_vgg_roi_fused(object(), x, y, _region(37, 29), capacity="frame")


def test_moss_step_takes_a_capacity():
    import inspect
    from moss_amd.train import MossStep
    assert inspect.signature(MossStep.__init__).parameters["lpips_capacity"].default is None
    assert inspect.signature(mlp.lpips_vgg_roi_fused).parameters["capacity"].default is None
