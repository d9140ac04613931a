"""CPU-only: every refusal of the eight C entry points of the SMPL / LBS family (lbs.hip, smpl_frame.hip, frame_bounds.hip), word
for word.  The library loads without a GPU and every refusal returns before any launch, so each case below provokes ``invalid_arg``
with ONE fault in an otherwise valid block (pointers are the never-dereferenced address 256) and compares the WHOLE text of
``moss_last_error()``.  The two-fault cases pin the ORDER of the checks: the text is that of the check that comes first.  The cases
that return 0 are the early returns that come before a later check (nothing is launched there either).

The old LBS entries say ``lbs`` / ``lbs forward`` / ``lbs backward``; the newer ones say their full name."""
import ctypes

import pytest

from moss_amd import _lib

PTR = 256
INVALID = -1                                              # MOSS_ERR_INVALID_ARG
BIG = 1 << 30

LBS_REQUIRED = ("vert_ids", "weights", "A_big", "A_obs", "d", "R", "Th")
LBS_NULL = "null required input (vert_ids, weights, A_big, A_obs, d, R, Th)"
PARENTS = "parents[j] must be in [0, j) for every j >= 1"


def block(cls, ints, parents=None, null=()):
    """A valid block of ``cls``: every pointer field 256 but those in ``null``, ``workspace_bytes`` large, the ints as given."""
    a = cls()
    for name, ctype in cls._fields_:
        if ctype is ctypes.c_void_p and name not in null:
            setattr(a, name, PTR)
    if hasattr(a, "workspace_bytes"):
        a.workspace_bytes = BIG
    for k, v in ints.items():
        setattr(a, k, v)
    for j, p in enumerate(parents or ()):
        a.parents[j] = p
    return a


def refused(lib, entry, cls, ints, cases, parents=None):
    """Every case ``(faults, text)``: ``faults`` maps a field to its bad value (``("parents", j)`` to a bad parent); ``text`` is the
    whole error text, or 0 for a call that returns 0 before the faulty field is looked at."""
    fn = getattr(lib, entry)
    assert fn(None, None) == INVALID
    first = lib.moss_last_error()
    for faults, text in cases:
        a = block(cls, ints, parents)
        for k, v in faults.items():
            if isinstance(k, tuple):
                a.parents[k[1]] = v
            else:
                setattr(a, k, v)
        rc = fn(ctypes.byref(a), None)
        if text == 0:
            assert rc == 0, (entry, faults)
        else:
            assert rc == INVALID, (entry, faults)
            assert lib.moss_last_error() == text.encode(), (entry, faults)
    return first


def lbs_common_cases(who):
    cases = [({"P": -1}, f"{who}: P must be >= 0"), ({"J": 0}, f"{who}: J must be 1..64"), ({"J": 65}, f"{who}: J must be 1..64"),
             ({"V": 0}, f"{who}: V must be >= 1")]
    cases += [({k: None}, f"{who}: {LBS_NULL}") for k in LBS_REQUIRED]
    # the order: P, J, V, the pointers
    cases += [({"P": -1, "J": 0}, f"{who}: P must be >= 0"), ({"J": 65, "V": 0}, f"{who}: J must be 1..64"),
              ({"J": 65, "vert_ids": None}, f"{who}: J must be 1..64"), ({"V": 0, "Th": None}, f"{who}: V must be >= 1")]
    return cases


LBS_INTS = {"P": 5, "J": 24, "V": 10}


def test_lbs_deform_forward(hip_lib):
    cases = lbs_common_cases("lbs") + [
        ({"T": None}, "lbs forward: null T or t"), ({"t": None}, "lbs forward: null T or t"),
        ({"x": None}, "lbs forward: p needs x"),
        ({"d": None, "T": None}, f"lbs: {LBS_NULL}"), ({"T": None, "x": None}, "lbs forward: null T or t"),
        ({"P": 0, "x": None}, "lbs forward: p needs x"),
        ({"P": 0}, 0), ({"P": 0, "x": None, "p": None, "w": None, "lbs_offsets": None}, 0),
    ]
    assert refused(hip_lib, "moss_lbs_deform_forward", _lib.LbsForwardArgs, LBS_INTS, cases) == b"lbs: null argument block"


def lbs_backward_cases(who_common, who):
    return lbs_common_cases(who_common) + [
        ({"x": None}, f"{who}: g_p and g_x need x"), ({"x": None, "g_p": None}, f"{who}: g_p and g_x need x"),
        ({"x": None, "g_x": None}, f"{who}: g_p and g_x need x"),
        ({"lbs_offsets": None}, f"{who}: g_L needs lbs_offsets"),
        ({"R": None, "x": None}, f"{who_common}: {LBS_NULL}"),
        ({"x": None, "lbs_offsets": None}, f"{who}: g_p and g_x need x"),
        ({"P": 0, "x": None}, f"{who}: g_p and g_x need x"), ({"P": 0, "lbs_offsets": None}, f"{who}: g_L needs lbs_offsets"),
    ]


def test_lbs_deform_backward(hip_lib):
    text = "lbs backward: g_A_obs needs moss_lbs_workspace_bytes(P, J) bytes of workspace"
    need = hip_lib.moss_lbs_workspace_bytes(5, 24)
    assert need > 0
    cases = lbs_backward_cases("lbs", "lbs backward") + [
        ({"workspace": None}, text), ({"workspace_bytes": need - 1}, text), ({"workspace_bytes": 0}, text),
        ({"lbs_offsets": None, "workspace": None}, "lbs backward: g_L needs lbs_offsets"),
        # P = 0 returns before the workspace is looked at
        ({"P": 0}, 0), ({"P": 0, "workspace": None, "workspace_bytes": 0}, 0),
    ]
    assert refused(hip_lib, "moss_lbs_deform_backward", _lib.LbsBackwardArgs, LBS_INTS, cases) == b"lbs: null argument block"


def test_lbs_deform_backward_frame(hip_lib):
    who = "moss_lbs_deform_backward_frame"
    text = f"{who}: g_A_obs, g_R and g_Th need moss_lbs_frame_workspace_bytes(P, J) bytes of workspace"
    need, plain = hip_lib.moss_lbs_frame_workspace_bytes(5, 24), hip_lib.moss_lbs_workspace_bytes(5, 24)
    assert need > plain > 0
    cases = lbs_backward_cases(who, who) + [
        ({"workspace": None}, text), ({"workspace_bytes": need - 1}, text), ({"workspace_bytes": plain}, text),
        ({"workspace": None, "g_R": None, "g_Th": None}, text), ({"workspace": None, "g_A_obs": None, "g_Th": None}, text),
        ({"workspace": None, "g_A_obs": None, "g_R": None}, text),
        ({"lbs_offsets": None, "workspace": None}, f"{who}: g_L needs lbs_offsets"),
    ]
    assert refused(hip_lib, who, _lib.LbsBackwardFrameArgs, LBS_INTS, cases) == f"{who}: null argument block".encode()


SF_INTS = {"P": 5, "V": 10, "J": 3}
SF_PARENTS = (0, 0, 1)


def size_cases(who):
    """The checks the three smpl_frame entries open with: P, V, J in that order."""
    return [({"P": -1}, f"{who}: P must be >= 0"), ({"V": 0}, f"{who}: V must be >= 1"), ({"J": 0}, f"{who}: J must be 1..64"),
            ({"J": 65}, f"{who}: J must be 1..64"), ({"P": -1, "V": 0}, f"{who}: P must be >= 0"),
            ({"V": 0, "J": 0}, f"{who}: V must be >= 1")]


def test_smpl_frame_forward(hip_lib):
    who = "moss_smpl_frame_forward"
    betas = f"{who}: num_betas and num_betas_big must be 0..shapedirs_stride"
    req = f"{who}: null required input (v_template, shapedirs, posedirs, J_regressor, poses_big, poses)"
    out = f"{who}: null output (A_big, A_obs, rot_mats)"
    ws = f"{who}: needs moss_smpl_frame_workspace_bytes(max(P, 1), V, J) bytes of workspace"
    need = hip_lib.moss_smpl_frame_workspace_bytes(5, 10, 3)
    assert need == 512                                               # (D and the shares: one 256-byte unit each)
    cases = size_cases(who) + [({"num_betas_big": -1}, betas), ({"num_betas": -1}, betas), ({"num_betas_big": 11}, betas),
                               ({"num_betas": 11}, betas)]
    cases += [({k: None}, req) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "poses_big", "poses")]
    cases += [
        ({"shapes_big": None}, f"{who}: null shapes"), ({"shapes": None}, f"{who}: null shapes"),
        ({"vert_ids": None}, f"{who}: null vert_ids or d"), ({"d": None}, f"{who}: null vert_ids or d"),
        ({"A_big": None}, out), ({"A_obs": None}, out), ({"rot_mats": None}, out),
        ({("parents", 2): 2}, f"{who}: {PARENTS}"), ({("parents", 1): -1}, f"{who}: {PARENTS}"), ({("parents", 1): 1}, f"{who}: {PARENTS}"),
        ({"workspace": None}, ws), ({"workspace_bytes": need - 1}, ws),
        # the order, and what a check lets through
        ({"J": 65, "v_template": None}, f"{who}: J must be 1..64"), ({"J": 65, "num_betas": 11}, f"{who}: J must be 1..64"),
        ({"num_betas": 11, "poses": None}, betas), ({"poses": None, "shapes": None}, req),
        ({"shapes": None, "d": None}, f"{who}: null shapes"), ({"d": None, "A_big": None}, f"{who}: null vert_ids or d"),
        ({"rot_mats": None, ("parents", 2): 2}, out), ({("parents", 2): 2, "workspace": None}, f"{who}: {PARENTS}"),
        ({"J": 1, "posedirs": None, "A_big": None}, out),          # J = 1 needs no posedirs
        ({"num_betas_big": 0, "shapes_big": None, "num_betas": 0, "shapes": None, "A_obs": None}, out),
        ({"P": 0, "vert_ids": None, "d": None, "rot_mats": None}, out),
        ({"saved": None, "correct_Rs": None, "workspace": None}, ws),
    ]
    first = refused(hip_lib, who, _lib.SmplFrameArgs, dict(SF_INTS, num_betas_big=10, num_betas=10, shapedirs_stride=10), cases, SF_PARENTS)
    assert first == f"{who}: null argument block".encode()


def smpl_backward_tail(who):
    gd = f"{who}: g_d needs vert_ids and posedirs"
    ws = f"{who}: g_d needs moss_smpl_frame_workspace_bytes(P, V, J) bytes of workspace"
    return [
        ({("parents", 2): 2}, f"{who}: {PARENTS}"), ({("parents", 1): -1}, f"{who}: {PARENTS}"),
        ({"vert_ids": None}, gd), ({"posedirs": None}, gd), ({"workspace": None}, ws), ({"workspace_bytes": 511}, ws),
        ({("parents", 2): 2, "vert_ids": None}, f"{who}: {PARENTS}"), ({"posedirs": None, "workspace": None}, gd),
    ]


def test_smpl_frame_backward(hip_lib):
    who = "moss_smpl_frame_backward"
    null = f"{who}: null saved or g_correct_Rs"
    cases = size_cases(who) + [
        ({"saved": None}, null), ({"g_correct_Rs": None}, null), ({"saved": None, ("parents", 2): 2}, null),
        ({"J": 65, "saved": None}, f"{who}: J must be 1..64"),
        # J = 1 returns before any pointer is looked at
        ({"J": 1}, 0), ({"J": 1, "saved": None, "g_correct_Rs": None, "workspace": None}, 0), ({"J": 1, "V": 0}, f"{who}: V must be >= 1"),
    ] + smpl_backward_tail(who)
    assert hip_lib.moss_smpl_frame_workspace_bytes(5, 10, 3) == 512
    assert refused(hip_lib, who, _lib.SmplFrameBackwardArgs, SF_INTS, cases, SF_PARENTS) == f"{who}: null argument block".encode()


def test_smpl_frame_backward_pose(hip_lib):
    who = "moss_smpl_frame_backward_pose"
    null = f"{who}: null saved or poses"
    cases = size_cases(who) + [
        ({"g_poses": None}, f"{who}: null g_poses"), ({"saved": None}, null), ({"poses": None}, null),
        ({"g_poses": None, "saved": None}, f"{who}: null g_poses"), ({"poses": None, ("parents", 2): 2}, null),
        ({"J": 65, "g_poses": None}, f"{who}: J must be 1..64"),
        # J = 1 is no early return here: the root's pose still gets its gradient
        ({"J": 1, "saved": None}, null), ({"J": 1, "g_poses": None}, f"{who}: null g_poses"),
        ({"g_correct_Rs": None, "correct_Rs": None, "workspace": None},
         f"{who}: g_d needs moss_smpl_frame_workspace_bytes(P, V, J) bytes of workspace"),
    ] + smpl_backward_tail(who)
    assert refused(hip_lib, who, _lib.SmplFrameBackwardPoseArgs, SF_INTS, cases, SF_PARENTS) == f"{who}: null argument block".encode()


def test_smpl_vertices(hip_lib):
    who = "moss_smpl_vertices"
    body = f"{who}: null body-model array (v_template, shapedirs, posedirs, J_regressor, weights)"
    frame = f"{who}: null frame input (poses, shapes, R, Th, pad)"
    out = f"{who}: null output (world_vertex, world_bound)"
    ws = f"{who}: needs moss_smpl_vertices_workspace_bytes(V, J) bytes of workspace"
    need = hip_lib.moss_smpl_vertices_workspace_bytes(10, 3)
    assert need > 0
    cases = [({"V": 0}, f"{who}: V must be >= 1"), ({"J": 0}, f"{who}: J must be 1..64"), ({"J": 65}, f"{who}: J must be 1..64"),
             ({"num_betas": -1}, f"{who}: num_betas must be 0..shapedirs_stride"), ({"num_betas": 11}, f"{who}: num_betas must be 0..shapedirs_stride")]
    cases += [({k: None}, body) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")]
    cases += [({k: None}, frame) for k in ("poses", "shapes", "R", "Th", "pad")]
    cases += [
        ({"world_vertex": None}, out), ({"world_bound": None}, out),
        ({("parents", 2): 2}, f"{who}: {PARENTS}"), ({("parents", 1): -1}, f"{who}: {PARENTS}"),
        ({"workspace": None}, ws), ({"workspace_bytes": need - 1}, ws),
        ({"V": 0, "J": 65}, f"{who}: V must be >= 1"), ({"J": 65, "weights": None}, f"{who}: J must be 1..64"),
        ({"num_betas": 11, "weights": None}, f"{who}: num_betas must be 0..shapedirs_stride"), ({"weights": None, "pad": None}, body),
        ({"pad": None, "world_bound": None}, frame), ({"world_bound": None, ("parents", 2): 2}, out),
        ({("parents", 2): 2, "workspace": None}, f"{who}: {PARENTS}"),
        ({"J": 1, "posedirs": None, "poses": None}, frame), ({"num_betas": 0, "shapes": None, "world_vertex": None}, out),
        ({"joints": None, "workspace": None}, ws),
    ]
    first = refused(hip_lib, who, _lib.SmplVerticesArgs, {"V": 10, "J": 3, "num_betas": 10, "shapedirs_stride": 10}, cases, SF_PARENTS)
    assert first == f"{who}: null argument block".encode()


def test_bound_mask(hip_lib):
    who = "moss_bound_mask"
    size = f"{who}: H and W must be >= 1 with H * W < 2^31"
    inp, out = f"{who}: null input (world_bound, K, RT)", f"{who}: null output (bound, rect, corners, flags)"
    ws = f"{who}: needs moss_bound_mask_workspace_bytes(C, H, W) bytes of workspace"
    need = hip_lib.moss_bound_mask_workspace_bytes(3, 17, 23)
    assert need > 0
    cases = [({"C": 0}, f"{who}: C must be 1..65535"), ({"C": 65536}, f"{who}: C must be 1..65535"), ({"H": 0}, size), ({"W": 0}, size),
             ({"H": 65536, "W": 32768}, size)]
    cases += [({k: None}, inp) for k in ("world_bound", "K", "RT")] + [({k: None}, out) for k in ("bound", "rect", "corners", "flags")]
    cases += [({"workspace": None}, ws), ({"workspace_bytes": need - 1}, ws),
              ({"C": 0, "H": 0}, f"{who}: C must be 1..65535"), ({"H": 0, "K": None}, size), ({"RT": None, "rect": None}, inp),
              ({"flags": None, "workspace": None}, out)]
    assert refused(hip_lib, who, _lib.BoundMaskArgs, {"C": 3, "H": 17, "W": 23}, cases) == f"{who}: null argument block".encode()


@pytest.mark.parametrize("name,bad", [
    ("moss_lbs_workspace_bytes", [(0, 24), (-1, 24), (5, 0), (5, -3), (5, 65), (0, 0)]),
    ("moss_lbs_frame_workspace_bytes", [(0, 24), (-1, 24), (5, 0), (5, -3), (5, 65), (0, 0)]),
    ("moss_smpl_frame_workspace_bytes", [(0, 10, 24), (-1, 10, 24), (5, 0, 24), (5, -1, 24), (5, 10, 0), (5, 10, 65), (5, 10, -1)]),
    ("moss_smpl_vertices_workspace_bytes", [(0, 24), (-1, 24), (10, 0), (10, 65), (10, -1)]),
    ("moss_bound_mask_workspace_bytes", [(0, 8, 8), (-1, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, -1, 8), (1, 65536, 32768)]),
])
def test_workspace_bytes_are_zero_for_what_the_calls_refuse(hip_lib, name, bad):
    fn = getattr(hip_lib, name)
    for args in bad:
        assert fn(*args) == 0, (name, args)
    good = {"moss_lbs_workspace_bytes": (5, 24), "moss_lbs_frame_workspace_bytes": (5, 24), "moss_smpl_frame_workspace_bytes": (5, 10, 3),
            "moss_smpl_vertices_workspace_bytes": (10, 3), "moss_bound_mask_workspace_bytes": (3, 17, 23)}[name]
    assert fn(*good) > 0 and fn(*good) % 256 == 0
