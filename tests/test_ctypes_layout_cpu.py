"""Every ``ctypes.Structure`` of moss_amd/_lib.py against include/moss_raster.h as a host C compiler lays it out: the size and the
offset of every field.  The blocks that the test file of their op already checks this way are left to it; this file takes all the
others, so a new mirror is checked from the day it is added.  The C name is the one the class's docstring gives first."""
import ctypes
import inspect
import re

import pytest

from moss_amd import _lib
from tests.helpers import c_layout, ctypes_layout

CHECKED_BY_THEIR_OP = {                                       # (tests/test_<file>_cpu.py)
    "SmplFrameArgs": "smpl_frame", "SmplFrameBackwardArgs": "smpl_frame", "LbsBackwardFrameArgs": "pose_fit",
    "SmplFrameBackwardPoseArgs": "pose_fit", "ViewImagesPrepareArgs": "view_images", "ViewImagesLoadArgs": "view_images",
    "SmplVerticesArgs": "frame_bounds", "BoundMaskArgs": "frame_bounds", "LpipsVggArgs": "lpips_dynamic",
    "LpipsVggBackwardArgs": "lpips_dynamic", "LpipsVggReferenceArgs": "lpips_reference", "LpipsVggForwardRefArgs": "lpips_reference",
    "LpipsConv3x3Args": "lpips_conv_layer", "EvalMetricsArgs": "metrics",
}
STRUCTS = {name: cls for name, cls in vars(_lib).items()
           if inspect.isclass(cls) and issubclass(cls, ctypes.Structure) and cls.__module__ == _lib.__name__}
HERE = sorted(set(STRUCTS) - set(CHECKED_BY_THEIR_OP))


def test_every_mirror_is_checked_somewhere():
    assert set(CHECKED_BY_THEIR_OP) <= set(STRUCTS)
    for name in ("LbsForwardArgs", "LbsBackwardArgs", "PoseHeadArgs", "PoseHeadBackwardArgs", "LbsWeightNetArgs", "LbsWeightNetBackwardArgs",
                 "DensifySelectArgs", "DensifyEmitArgs", "FusedAdamWStruct", "AdamWFlatArgs", "AdamWMultiArgs", "FramesToU8Args",
                 "RowsTensor", "RowsRelayoutArgs"):
        assert name in HERE, name


@pytest.mark.parametrize("pyname", HERE)
def test_mirror_has_the_headers_size_and_offsets(tmp_path, pyname):
    cls = STRUCTS[pyname]
    cname = re.match(r"\s*``(moss_\w+)``", cls.__doc__ or "")
    assert cname, f"the docstring of _lib.{pyname} must begin with the C struct's name in double backquotes"
    assert c_layout(tmp_path, cname.group(1), [f[0] for f in cls._fields_]) == ctypes_layout(cls)
