"""CPU-only tests of the fused per-frame SMPL op (C ABI moss_smpl_frame_forward / _backward, moss_amd.lbs.smpl_frame_fused): the
symbols and their declarations, the ctypes blocks against the header's layout, the workspace size function, the refusals of the
Python surface (there is no CPU path), and the two switches (``fused_frame``, ``pipe.smpl_frame_in_op``)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from moss_amd import lbs as mlbs
from tests.helpers import c_layout, ctypes_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("moss_smpl_frame_forward", "moss_smpl_frame_backward", "moss_smpl_frame_workspace_bytes")


def test_symbols_exported_and_declared(hip_lib):
    text = open(os.path.join(ROOT, "include", "moss_raster.h")).read()
    assert re.search(r"#define\s+MOSS_ABI_VERSION\s+7\b", text)
    diag = re.search(r"#ifdef MOSS_DIAG\n(.*?)#endif", text, flags=re.S).group(0)
    public = re.sub(r"/\*.*?\*/", "", text.replace(diag, ""), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, public), name
        assert hasattr(hip_lib, name), name
    assert "} moss_smpl_frame_args;" in public and "} moss_smpl_frame_backward_args;" in public
    # the declarations cite the reference lines they replace
    block = text[text.index("The per-frame, per-subject part of MOSS's coarse_deform_c2source"):text.index("size_t moss_smpl_frame_workspace_bytes")]
    for cite in ("scene/gaussian_model.py:835-901", ":965-1031", ":945-963", ":885-901"):
        assert cite in block, cite
    from moss_amd import _lib
    assert int(re.search(r"#define\s+MOSS_SMPL_FRAME_MAX_JOINTS\s+(\d+)", text).group(1)) == _lib.SMPL_FRAME_MAX_JOINTS == mlbs.MAX_JOINTS
    assert int(re.search(r"#define\s+MOSS_SMPL_FRAME_SAVED_FLOATS_PER_JOINT\s+(\d+)", text).group(1)) == _lib.SMPL_FRAME_SAVED_FLOATS_PER_JOINT


@pytest.mark.parametrize("cname,pyname", [("moss_smpl_frame_args", "SmplFrameArgs"),
                                          ("moss_smpl_frame_backward_args", "SmplFrameBackwardArgs")])
def test_ctypes_blocks_match_the_c_layout(tmp_path, cname, pyname):
    """The ctypes mirrors have the header's size and field offsets (compiled against the header with the host compiler)."""
    from moss_amd import _lib
    cls = getattr(_lib, pyname)
    assert c_layout(tmp_path, cname, [f[0] for f in cls._fields_]) == ctypes_layout(cls)


def test_workspace_bytes_is_a_monotonic_host_function(hip_lib):
    ws = hip_lib.moss_smpl_frame_workspace_bytes
    for bad in ((0, 6890, 24), (-1, 6890, 24), (100, 0, 24), (100, -5, 24), (100, 6890, 0), (100, 6890, -1), (100, 6890, 65)):
        assert ws(*bad) == 0, bad
    base = ws(45695, 6890, 24)
    assert base >= 6890 * 3 * 4 and base % 256 == 0
    assert base >= ((45695 + 63) // 64) * 207 * 8               # one float64 vector of 9 (J - 1) features per 64 Gaussians
    prev = 0
    for P in (1, 63, 64, 65, 6890, 45695, 100000, 1000000):
        cur = ws(P, 6890, 24)
        assert cur >= prev > -1
        prev = cur
    assert ws(100, 100, 24) <= ws(100, 6890, 24) <= ws(100, 20000, 24)
    assert ws(100000, 6890, 2) <= ws(100000, 6890, 24) <= ws(100000, 6890, 55) <= ws(100000, 6890, 64)


def _case(J=24, V=64, P=10):
    body = mlbs.synthetic_body_model(V, J, seed=3)
    return body, mlbs.synthetic_frame(1, J), mlbs.synthetic_frame(0, J, big_pose=True), torch.arange(P) % V


def test_refuses_cpu_tensors_naming_the_torch_form(hip_lib):
    body, fr, big, ids = _case()
    with pytest.raises(ValueError, match="must be on a GPU.*smpl_joint_transforms"):
        mlbs.smpl_frame_fused(body, fr, big, ids)
    with pytest.raises(ValueError, match="must be on a GPU"):
        mlbs.smpl_frame_fused(body, fr, big, ids, correct_Rs=torch.eye(3).repeat(23, 1, 1))


def test_refuses_bad_inputs(hip_lib):
    body, fr, big, ids = _case()
    with pytest.raises(ValueError, match="contiguous"):
        mlbs.smpl_frame_fused({**body, "J_regressor": body["J_regressor"].t().contiguous().t()}, fr, big, ids)
    with pytest.raises(ValueError, match="contiguous"):
        mlbs.smpl_frame_fused(body, fr, big, ids, correct_Rs=torch.eye(3).repeat(23, 1, 1).transpose(1, 2))
    with pytest.raises(ValueError, match="float32"):
        mlbs.smpl_frame_fused({**body, "posedirs": body["posedirs"].double()}, fr, big, ids)
    with pytest.raises(ValueError, match="float32"):
        mlbs.smpl_frame_fused(body, {**fr, "poses": fr["poses"].double()}, big, ids)
    with pytest.raises(ValueError, match="int64"):
        mlbs.smpl_frame_fused(body, fr, big, ids.int())
    with pytest.raises(ValueError, match="shape"):
        mlbs.smpl_frame_fused(body, fr, big, ids, correct_Rs=torch.eye(3).repeat(24, 1, 1))
    with pytest.raises(ValueError, match="elements"):
        mlbs.smpl_frame_fused(body, {**fr, "poses": fr["poses"][:, :69]}, big, ids)
    body65, fr65, big65, ids65 = _case(J=65)
    with pytest.raises(ValueError, match="1..64"):
        mlbs.smpl_frame_fused(body65, fr65, big65, ids65)
    for who, key in (("params", "poses"), ("params", "shapes"), ("t_params", "poses"), ("t_params", "shapes")):
        p = {"params": dict(fr), "t_params": dict(big)}
        p[who][key] = p[who][key].clone().requires_grad_(True)
        with pytest.raises(ValueError, match="requires grad"):
            mlbs.smpl_frame_fused(body, p["params"], p["t_params"], ids)
    with pytest.raises(ValueError, match="requires grad"):
        mlbs.smpl_frame_fused({**body, "posedirs": body["posedirs"].clone().requires_grad_(True)}, fr, big, ids)


def test_the_switches_exist():
    sig = inspect.signature(mlbs.coarse_deform_c2source)
    assert "fused_frame" in sig.parameters and sig.parameters["fused_frame"].default is False
    assert list(sig.parameters)[:8] == ["model", "query_pts", "params", "t_params", "t_vertices", "lbs_weights", "correct_Rs", "return_transl"]
    assert "smpl_frame_fused" in mlbs.__all__
    src = open(os.path.join(ROOT, "moss_amd", "gaussian_renderer.py")).read()
    assert "smpl_frame_in_op" in src and "fused_frame" in src


def test_c_abi_refuses_bad_arguments_with_its_name(hip_lib):
    """Host-side validation needs no device: a bad J, null inputs and a bad parent table come back as -1 with the entry point's name.
    (In a thread of its own: the error text is per thread, and tests/test_host_cpu.py expects the main thread's to be empty.)"""
    import threading
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


def _refusals(hip_lib):
    from moss_amd._lib import SmplFrameArgs, SmplFrameBackwardArgs
    a = SmplFrameArgs()
    a.P, a.V, a.J = 1, 10, 65
    assert hip_lib.moss_smpl_frame_forward(ctypes.byref(a), None) == -1
    assert b"moss_smpl_frame_forward: J must be 1..64" in hip_lib.moss_last_error()
    a.J = 24
    assert hip_lib.moss_smpl_frame_forward(ctypes.byref(a), None) == -1
    assert b"moss_smpl_frame_forward" in hip_lib.moss_last_error() and b"null" in hip_lib.moss_last_error()
    b = SmplFrameBackwardArgs()
    b.P, b.V, b.J = 1, 10, 0
    assert hip_lib.moss_smpl_frame_backward(ctypes.byref(b), None) == -1
    assert b"moss_smpl_frame_backward: J must be 1..64" in hip_lib.moss_last_error()
    b.J = 3
    b.saved = b.g_correct_Rs = 256                               # (never dereferenced on the host)
    b.parents[1], b.parents[2] = 0, 2
    assert hip_lib.moss_smpl_frame_backward(ctypes.byref(b), None) == -1
    assert b"parents[j] must be in [0, j)" in hip_lib.moss_last_error()
