"""A frame's posed SMPL vertices, their world bound, and per camera the bound mask and its rectangle -- on the device.

MOSS makes these in its dataset reader, on the CPU, per (pose, camera) (``scene/dataset_readers.py:428-439`` with numpy SMPL,
``get_bound_corners``, ``project`` and six ``cv2.fillPoly``, ``:1008-1045``; the big pose at ``:331-339``).  Here they are two fused HIP
ops (C ABI ``moss_smpl_vertices`` / ``moss_bound_mask``, csrc/frame_bounds.hip; the formulas are restated in include/moss_raster.h):

* :func:`posed_vertices` -- ``world_vertex`` (V,3), ``world_bound`` (2,3) and optionally the posed joints of one ``smpl_param``;
* :func:`bound_masks` -- ``bound`` (C,H,W), ``rect`` (C,5), ``corners`` (C,8,2), ``flags`` (C) of one ``world_bound`` for C cameras;
* :class:`FrameBounds` -- both on buffers of its own: capturable, and its ``regions`` are ``ViewRegion``s at stable addresses;
* :func:`dataset_regions` -- every view of a dataset, one host read at the end;
* :func:`camera_KRT` -- ``K`` and ``RT`` of a MOSS ``Camera``.

The CPU statements -- :func:`posed_vertices_torch` (any dtype: a float64 run is the yardstick), :func:`project_corners_numpy` and
:func:`bound_mask_numpy` (int64) -- are what the kernels are tested against.  The mask is NOT verified against ``cv2.fillPoly`` (see
INTEGRATION.md): rule (b)'s tie pixels and lines cv2 clips at the image border may differ by single pixels on the outline.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._checks import body_arrays, frame_params, need, need_gpu, no_grad
from .lbs import batch_rodrigues

__all__ = ["posed_vertices", "posed_vertices_torch", "bound_masks", "bound_mask_numpy", "project_corners_numpy", "camera_KRT",
           "FrameBounds", "dataset_regions", "FACES", "CORNER_LIMIT"]

FACES = ((0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5))    # dataset_readers.py:1039-1044
CORNER_LIMIT = 1 << 20


# ---- the CPU statements ------------------------------------------------------------------------------------------------------------------
def posed_vertices_torch(body, params, pad):
    """``(world_vertex (V,3), world_bound (2,3), joints (J,3))`` in torch ops, in the dtype and on the device of the inputs: the
    reference's ``SMPL.__call__`` (smpl/smpl_numpy.py:46-98), ``xyz @ R^T + Th`` and the padded min / max
    (dataset_readers.py:428-436), with the project's Rodrigues.  ``joints`` are the posed joints ``SMPL.__call__`` returns second."""
    vt, W = body["v_template"], body["weights"]
    J, V = W.shape[-1], vt.shape[0]
    betas = params["shapes"].reshape(-1).to(vt)
    v_shaped = vt + (body["shapedirs"][..., :betas.shape[0]] * betas).sum(-1)
    joints = body["J_regressor"] @ v_shaped
    rot = batch_rodrigues(params["poses"].reshape(-1, 3).to(vt)).reshape(J, 3, 3)
    v_posed = v_shaped
    if J > 1:
        feat = (rot[1:] - torch.eye(3, dtype=vt.dtype, device=vt.device)).reshape(-1)
        v_posed = v_shaped + (body["posedirs"].reshape(V * 3, -1) @ feat).reshape(V, 3)
    par = [int(v) for v in body["kintree_table"][0].tolist()]
    G = []
    for j in range(J):
        rel = joints[j] if j == 0 else joints[j] - joints[par[j]]
        local = torch.cat([torch.cat([rot[j], rel[:, None]], 1), torch.tensor([[0, 0, 0, 1]], dtype=vt.dtype, device=vt.device)], 0)
        G.append(local if j == 0 else G[par[j]] @ local)
    G = torch.stack(G, 0)
    A = G.clone()
    A[:, :3, 3] = G[:, :3, 3] - (G[:, :3, :3] @ joints[..., None]).squeeze(-1)
    T = (W @ A.reshape(J, 16)).reshape(V, 4, 4)
    v = (T[:, :3, :3] @ v_posed[..., None]).squeeze(-1) + T[:, :3, 3]
    world = v @ params["R"].reshape(3, 3).to(vt).t() + params["Th"].reshape(1, 3).to(vt)
    p = torch.as_tensor(pad, dtype=vt.dtype, device=vt.device).reshape(())
    bound = torch.stack([world.min(0).values - p, world.max(0).values + p], 0)
    return world, bound, G[:, :3, 3]


def project_corners_numpy(world_bound, K, RT, return_unrounded=False):
    """``(corners (C,8,2) int64, flags (C) int64)`` of a float32 ``world_bound`` (2,3) seen by ``K`` (C,3,3) / ``RT`` (C,3,4) (or one
    camera: (3,3) / (3,4), then (8,2) and a scalar): ``get_bound_corners`` and ``project`` (dataset_readers.py:1008-1032) in float64,
    every operation rounded on its own in the order include/moss_raster.h states, ``np.round``, the flag (a corner with
    ``uvw[2] <= 0`` or a rounded coordinate beyond 2^20) and the clamp to +-2^20.  ``return_unrounded``: also ``xy`` (C,8,2) float64."""
    wb = np.asarray(world_bound, dtype=np.float32).reshape(2, 3).astype(np.float64)
    K = np.asarray(K, dtype=np.float32).astype(np.float64)
    RT = np.asarray(RT, dtype=np.float32).astype(np.float64)
    single = K.ndim == 2
    K, RT = K.reshape(-1, 3, 3), RT.reshape(-1, 3, 4)
    i = np.arange(8)
    c = np.stack([wb[(i >> 2) & 1, 0], wb[(i >> 1) & 1, 1], wb[i & 1, 2]], 1)                  # (8,3)
    with np.errstate(all="ignore"):
        cam = [((c[None, :, 0] * RT[:, r, 0, None] + c[None, :, 1] * RT[:, r, 1, None]) + c[None, :, 2] * RT[:, r, 2, None])
               + RT[:, r, 3, None] for r in range(3)]
        uvw = [(cam[0] * K[:, r, 0, None] + cam[1] * K[:, r, 1, None]) + cam[2] * K[:, r, 2, None] for r in range(3)]
        xy = np.stack([uvw[0] / uvw[2], uvw[1] / uvw[2]], -1)                                   # (C,8,2)
        q = np.round(xy)
        flags = ((uvw[2] <= 0).any(1) | (~(np.abs(q) <= CORNER_LIMIT)).any((1, 2))).astype(np.int64)
        q = np.where(q >= -CORNER_LIMIT, q, -float(CORNER_LIMIT))
        q = np.where(q > CORNER_LIMIT, float(CORNER_LIMIT), q)
    corners = q.astype(np.int64)
    out = (corners[0], flags[0]) if single else (corners, flags)
    return out + ((xy[0] if single else xy),) if return_unrounded else out


def bound_mask_numpy(corners, H, W, flagged=False):
    """``(bound (H,W) uint8, rect (5,) int64)`` of one camera's rounded ``corners`` (8,2): the union of the six faces by rules (a) closed
    quad and (b) drawn edge of include/moss_raster.h, in int64; ``rect`` = (x, y, w, h, count) with ``bounding_rect``'s rectangle
    ((0,0,0,0) when empty).  ``flagged``: the whole frame."""
    q = np.asarray(corners, dtype=np.int64).reshape(8, 2)
    H, W = int(H), int(W)
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    bound = np.ones((H, W), dtype=bool) if flagged else np.zeros((H, W), dtype=bool)
    for face in () if flagged else FACES:
        f = q[list(face)]
        inbox = (x >= f[:, 0].min()) & (x <= f[:, 0].max()) & (y >= f[:, 1].min()) & (y <= f[:, 1].max())
        ge, le, edge = inbox.copy(), inbox.copy(), np.zeros((H, W), dtype=bool)
        for k in range(4):
            q0, q1 = f[k], f[(k + 1) % 4]
            dx, dy = q1[0] - q0[0], q1[1] - q0[1]
            cr = dx * (y - q0[1]) - dy * (x - q0[0])
            ge &= cr >= 0
            le &= cr <= 0
            ebox = (x >= min(q0[0], q1[0])) & (x <= max(q0[0], q1[0])) & (y >= min(q0[1], q1[1])) & (y <= max(q0[1], q1[1]))
            edge |= ebox & (np.abs(2 * cr) <= max(abs(dx), abs(dy)))
        bound |= ge | le | edge
    ys, xs = np.nonzero(bound.any(1))[0], np.nonzero(bound.any(0))[0]
    rect = np.zeros(5, dtype=np.int64)
    if ys.size:
        rect[:] = (xs[0], ys[0], xs[-1] - xs[0] + 1, ys[-1] - ys[0] + 1, int(bound.sum()))
    return bound.astype(np.uint8), rect


def camera_KRT(camera):
    """``(K (3,3), RT (3,4))`` float32 CPU tensors of a MOSS ``Camera``: its ``K``, and ``[R^T | T]`` -- the camera stores ``R``
    transposed (dataset_readers.py:396) -- which is the ``w2c[:3]`` that ``get_bound_2d_mask`` is given (:439)."""
    as32 = lambda v: torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v), dtype=torch.float32)  # noqa: E731
    missing = [k for k in ("K", "R", "T") if not hasattr(camera, k)]
    if missing:
        raise ValueError(f"camera_KRT: the camera has no {missing} (a MOSS Camera carries K, R -- stored transposed -- and T)")
    K, R, T = as32(camera.K).reshape(3, 3), as32(camera.R).reshape(3, 3), as32(camera.T).reshape(3)
    return K.contiguous(), torch.cat([R.t(), T[:, None]], 1).contiguous()


# ---- the fused ops -------------------------------------------------------------------------------------------------------------------------
_WHY = "no gradient is formed for it"


def _data(who, t, name, shape=None, dtype=torch.float32, numel=None, device=None):
    """``need`` of a tensor that must not require grad."""
    no_grad(who, ((name, need(who, t, name, shape, dtype, numel, device)),), _WHY)
    return t


def _body_arrays(who, body):
    return body_arrays(who, body, _WHY, "kernels of csrc/frame_bounds.hip", "posed_vertices_torch is the torch form", check_weights=True)


def _frame_inputs(who, params, J, body, dev):
    flat = frame_params(who, params, ("poses", "shapes", "R", "Th"), J, int(body["shapedirs"].shape[2]), dev)
    no_grad(who, [(f"params['{k}']", t) for k, t in flat.items()], _WHY)
    return flat


def _launch_vertices(body, V, J, par, poses, shapes, R, Th, pad, world_vertex, world_bound, joints, ws):
    from ._lib import SmplVerticesArgs, call, ptr
    a = SmplVerticesArgs()
    a.V, a.J, a.num_betas, a.shapedirs_stride = V, J, int(shapes.numel()), int(body["shapedirs"].shape[2])
    a.parents[:J] = par
    a.v_template, a.shapedirs, a.posedirs = body["v_template"].data_ptr(), body["shapedirs"].data_ptr(), body["posedirs"].data_ptr()
    a.J_regressor, a.weights = body["J_regressor"].data_ptr(), body["weights"].data_ptr()
    a.poses, a.shapes, a.R, a.Th, a.pad = poses.data_ptr(), shapes.data_ptr(), R.data_ptr(), Th.data_ptr(), pad.data_ptr()
    a.world_vertex, a.world_bound, a.joints = world_vertex.data_ptr(), world_bound.data_ptr(), ptr(joints)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    call("moss_smpl_vertices", world_vertex.device, ctypes.byref(a))


def posed_vertices(body, params, pad=0.1, out=None, joints=False):
    """``(world_vertex (V,3), world_bound (2,3)[, joints (J,3)])`` of one frame on the device (C ABI ``moss_smpl_vertices``, three
    launches): what dataset_readers.py:428-436 computes with numpy SMPL on the CPU; a subject's ``big_pose_world_vertex`` /
    ``big_pose_world_bound`` (:331-339) is this of the big pose with ``pad=0.05``.

    ``body``: the dict ``smpl_frame_fused`` takes (``weights`` (V,J) enters here).  ``params``: ``poses`` (3J elements), ``shapes`` (at
    most B), ``R`` (3,3), ``Th`` (3 elements).  ``pad``: a float, or one float32 on the device.  ``out``: the tensors to write into,
    in the order returned.  All float32, contiguous, on one GPU; one that requires grad raises ValueError.  No host read: capturable
    when ``out`` and a tensor ``pad`` are given (the workspace is then the caller's to keep alive: use :class:`FrameBounds`).  There is
    no CPU path; :func:`posed_vertices_torch` is the torch form."""
    from ._lib import lib
    who = "posed_vertices"
    V, J, par, dev = _body_arrays(who, body)
    flat = _frame_inputs(who, params, J, body, dev)
    if isinstance(pad, torch.Tensor):
        pad_t = _data(who, pad, "pad", numel=1, device=dev)
    else:
        pad_t = torch.full((1,), float(pad), dtype=torch.float32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    shapes = [(V, 3), (2, 3)] + ([(J, 3)] if joints else [])
    if out is None:
        out = [torch.empty(s, **f32) for s in shapes]
    else:
        out = list(out)
        if len(out) != len(shapes):
            raise ValueError(f"{who}: out must hold {len(shapes)} tensors")
        for t, s, name in zip(out, shapes, ("world_vertex", "world_bound", "joints")):
            _data(who, t, f"out {name}", s, device=dev)
    ws = torch.empty(int(lib().moss_smpl_vertices_workspace_bytes(V, J)), dtype=torch.uint8, device=dev)
    _launch_vertices(body, V, J, par, flat["poses"], flat["shapes"], flat["R"], flat["Th"], pad_t, out[0], out[1],
                     out[2] if joints else None, ws)
    return tuple(out)


def _launch_masks(world_bound, K, RT, H, W, bound, rect, corners, flags, ws):
    from ._lib import BoundMaskArgs, call
    a = BoundMaskArgs()
    a.C, a.H, a.W = int(K.shape[0]), int(H), int(W)
    a.world_bound, a.K, a.RT = world_bound.data_ptr(), K.data_ptr(), RT.data_ptr()
    a.bound, a.rect, a.corners, a.flags = bound.data_ptr(), rect.data_ptr(), corners.data_ptr(), flags.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    call("moss_bound_mask", bound.device, ctypes.byref(a))


def _mask_workspace(C, H, W, dev):
    from ._lib import lib
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W >= 2 ** 31 or not 1 <= C <= 65535:
        raise ValueError(f"bound_masks: C must be 1..65535 and H, W >= 1 with H * W < 2^31, got C = {C}, {H} x {W}")
    return torch.empty(int(lib().moss_bound_mask_workspace_bytes(C, H, W)), dtype=torch.uint8, device=dev)


def bound_masks(world_bound, K, RT, H, W, out=None):
    """``(bound (C,H,W) uint8, rect (C,5) int32, corners (C,8,2) int32, flags (C) int32)`` of one ``world_bound`` (2,3) for the C cameras
    ``K`` (C,3,3) / ``RT`` (C,3,4) (C ABI ``moss_bound_mask``, two launches whatever C is): ``get_bound_2d_mask``
    (dataset_readers.py:1034-1045) and ``cv2.boundingRect`` of it, by the rules restated in include/moss_raster.h.  ``rect[c]`` is laid
    out as ``ViewRegion.rect``; ``flags[c] & 1``: a corner behind the camera or beyond 2^20 pixels -- the mask is then the whole frame.
    float32 contiguous GPU tensors; ``out``: the four tensors to write into.  No host read."""
    who = "bound_masks"
    if not isinstance(K, torch.Tensor) or K.dim() != 3:
        raise ValueError(f"{who}: K must be a (C,3,3) tensor")
    C = int(K.shape[0])
    dev = K.device
    need_gpu(who, dev, "kernels of csrc/frame_bounds.hip", "project_corners_numpy and bound_mask_numpy are the CPU form")
    _data(who, world_bound, "world_bound", (2, 3), device=dev)
    _data(who, K, "K", (C, 3, 3))
    _data(who, RT, "RT", (C, 3, 4), device=dev)
    ws = _mask_workspace(C, H, W, dev)
    specs = [((C, int(H), int(W)), torch.uint8), ((C, 5), torch.int32), ((C, 8, 2), torch.int32), ((C,), torch.int32)]
    if out is None:
        out = [torch.empty(s, dtype=d, device=dev) for s, d in specs]
    else:
        out = list(out)
        if len(out) != 4:
            raise ValueError(f"{who}: out must hold bound, rect, corners, flags")
        for t, (s, d), name in zip(out, specs, ("bound", "rect", "corners", "flags")):
            _data(who, t, f"out {name}", s, d, device=dev)
    _launch_masks(world_bound, K, RT, H, W, *out, ws)
    return tuple(out)


def _cameras_KRT(cameras, dev):
    """(K (C,3,3), RT (C,3,4)) on ``dev`` of a list of MOSS cameras or (K, RT) pairs."""
    pairs = [c if isinstance(c, (tuple, list)) else camera_KRT(c) for c in cameras]
    if not pairs:
        raise ValueError("bounds: at least one camera")
    f32 = lambda t: torch.as_tensor(t, dtype=torch.float32).detach()                           # noqa: E731
    K = torch.stack([f32(k).reshape(3, 3).cpu() for k, _ in pairs], 0).contiguous()
    RT = torch.stack([f32(rt).reshape(3, 4).cpu() for _, rt in pairs], 0).contiguous()
    return K.to(dev), RT.to(dev)


class FrameBounds:
    """``fb = FrameBounds(body, cameras, H, W)``; ``fb.update(smpl_param)`` queues the five launches of one pose for all cameras.

    It owns the static inputs (``smpl_param``: ``poses``, ``shapes``, ``R``, ``Th``; ``pad``; ``K`` (C,3,3), ``RT`` (C,3,4)), the outputs
    (``world_vertex`` (V,3), ``world_bound`` (2,3), ``joints`` (J,3), ``bound`` (C,H,W), ``rect`` (C,5), ``corners`` (C,8,2), ``flags``
    (C)) and the workspaces; ``regions[c]`` is a ``ViewRegion.from_device`` over ``bound[c]`` / ``rect[c]``: stable addresses, so a
    captured consumer sees the new frame.  ``update(smpl_param)`` copies the given keys into the static inputs first (``load``);
    ``update()`` alone only launches -- the form to capture: a replay serves a new pose after ``load``.  Nothing reads the host;
    ``regions[c].read()`` is the one read a host consumer needs.  ``cameras``: MOSS ``Camera`` objects or ``(K, RT)`` pairs;
    ``set_cameras`` rewrites them in place.  ``num_betas``: how many shape coefficients ``smpl_param['shapes']`` carries (default: all
    that ``shapedirs`` stores); ``smpl_param``: the caller's static tensors to read instead of tensors of its own (``MossPlayer``'s)."""

    def __init__(self, body, cameras, H, W, pad=0.1, num_betas=None, smpl_param=None):
        from ._lib import lib
        from .loss import ViewRegion
        who = "FrameBounds"
        self.body = body
        self.V, self.J, self._par, dev = _body_arrays(who, body)
        self.device, self.H, self.W = dev, int(H), int(W)
        B = int(body["shapedirs"].shape[2])
        nb = B if num_betas is None else int(num_betas)
        if not 0 <= nb <= B:
            raise ValueError(f"{who}: num_betas must be 0..{B}")
        f32 = dict(dtype=torch.float32, device=dev)
        if smpl_param is None:
            self.smpl_param = {"poses": torch.zeros(1, 3 * self.J, **f32), "shapes": torch.zeros(1, nb, **f32), "R": torch.eye(3, **f32),
                               "Th": torch.zeros(1, 3, **f32)}
        else:                                                    # (the caller's static tensors are the inputs themselves)
            _frame_inputs(who, smpl_param, self.J, body, dev)
            self.smpl_param = {k: smpl_param[k] for k in ("poses", "shapes", "R", "Th")}
        self.pad = torch.full((1,), float(pad), **f32)
        self.K, self.RT = _cameras_KRT(cameras, dev)
        C = self.C = int(self.K.shape[0])
        self.world_vertex, self.world_bound, self.joints = torch.zeros(self.V, 3, **f32), torch.zeros(2, 3, **f32), torch.zeros(self.J, 3, **f32)
        self.bound = torch.zeros((C, self.H, self.W), dtype=torch.uint8, device=dev)
        self.rect, self.corners = torch.zeros((C, 5), dtype=torch.int32, device=dev), torch.zeros((C, 8, 2), dtype=torch.int32, device=dev)
        self.flags = torch.zeros(C, dtype=torch.int32, device=dev)
        self._ws_v = torch.empty(int(lib().moss_smpl_vertices_workspace_bytes(self.V, self.J)), dtype=torch.uint8, device=dev)
        self._ws_m = _mask_workspace(C, self.H, self.W, dev)
        self.regions = [ViewRegion.from_device(self.bound[c], self.rect[c]) for c in range(C)]

    def set_cameras(self, cameras):
        K, RT = _cameras_KRT(cameras, self.device)
        if K.shape != self.K.shape:
            raise ValueError(f"FrameBounds.set_cameras: built for {self.C} cameras, got {int(K.shape[0])}")
        self.K.copy_(K)
        self.RT.copy_(RT)

    def load(self, smpl_param):
        """Copy ``poses``, ``shapes``, ``R``, ``Th`` (those given) into the static inputs."""
        with torch.no_grad():
            for k, dst in self.smpl_param.items():
                if k in smpl_param and smpl_param[k] is not dst:
                    src = torch.as_tensor(smpl_param[k])
                    if src.numel() != dst.numel():
                        raise ValueError(f"FrameBounds.load: smpl_param['{k}'] must have {dst.numel()} elements, got {src.numel()}")
                    dst.copy_(src.reshape(dst.shape))
        return self

    def update(self, smpl_param=None):
        if smpl_param is not None:
            self.load(smpl_param)
        s = self.smpl_param
        _launch_vertices(self.body, self.V, self.J, self._par, s["poses"], s["shapes"], s["R"], s["Th"], self.pad, self.world_vertex,
                         self.world_bound, self.joints, self._ws_v)
        _launch_masks(self.world_bound, self.K, self.RT, self.H, self.W, self.bound, self.rect, self.corners, self.flags, self._ws_m)
        return self


def dataset_regions(body, smpl_params_by_pose, cameras_by_pose, H, W, pad=0.1):
    """The regions of a whole dataset -- what replaces dataset_readers.py:428-439 for a loader.  ``smpl_params_by_pose``: one
    ``smpl_param`` dict per pose (``poses``, ``shapes``, ``R``, ``Th``: tensors or arrays, any device); ``cameras_by_pose``: per pose the
    list of its cameras (MOSS ``Camera`` objects or ``(K, RT)`` pairs).  Returns ``{"regions": [[ViewRegion per camera] per pose],
    "world_vertex": [(V,3) per pose], "world_bound": [(2,3) per pose], "flagged": [(pose, camera) ...]}``.  Every pose gets buffers of
    its own (its views' ``bound`` / ``rect`` are rows of them and keep them alive); five launches per pose; all rectangles and flags
    come to the host in ONE read at the end, which also sets every region's ``xywh``."""
    from ._lib import lib
    from .loss import ViewRegion
    who = "dataset_regions"
    V, J, par, dev = _body_arrays(who, body)
    if len(smpl_params_by_pose) != len(cameras_by_pose) or not len(smpl_params_by_pose):
        raise ValueError(f"{who}: one camera list per pose, at least one pose")
    f32 = dict(dtype=torch.float32, device=dev)
    pad_t = torch.full((1,), float(pad), **f32)
    ws_v = torch.empty(int(lib().moss_smpl_vertices_workspace_bytes(V, J)), dtype=torch.uint8, device=dev)
    ws_m = {}
    regions, vertices, bounds, words = [], [], [], []
    for params, cameras in zip(smpl_params_by_pose, cameras_by_pose):
        frame = {k: torch.as_tensor(params[k]).detach().to(**f32).reshape(-1).contiguous() for k in ("poses", "shapes", "R", "Th")}
        flat = _frame_inputs(who, frame, J, body, dev)
        K, RT = _cameras_KRT(cameras, dev)
        C = int(K.shape[0])
        if C not in ws_m:
            ws_m[C] = _mask_workspace(C, H, W, dev)
        wv, wb = torch.empty(V, 3, **f32), torch.empty(2, 3, **f32)
        bound = torch.empty((C, int(H), int(W)), dtype=torch.uint8, device=dev)
        rect_flags = torch.empty((C, 6), dtype=torch.int32, device=dev)                        # (rect and flag side by side: one read)
        rect, corners = torch.empty((C, 5), dtype=torch.int32, device=dev), torch.empty((C, 8, 2), dtype=torch.int32, device=dev)
        flags = torch.empty(C, dtype=torch.int32, device=dev)
        _launch_vertices(body, V, J, par, flat["poses"], flat["shapes"], flat["R"], flat["Th"], pad_t, wv, wb, None, ws_v)
        _launch_masks(wb, K, RT, H, W, bound, rect, corners, flags, ws_m[C])
        rect_flags[:, :5] = rect
        rect_flags[:, 5] = flags
        words.append(rect_flags)
        regions.append([ViewRegion.from_device(bound[c], rect[c]) for c in range(C)])
        vertices.append(wv)
        bounds.append(wb)
    host = torch.cat(words, 0).cpu().tolist()                                                   # the one host read
    flagged, at = [], 0
    for p, views in enumerate(regions):
        for c, region in enumerate(views):
            region.read(host[at][:5])
            if host[at][5] & 1:
                flagged.append((p, c))
            at += 1
    return {"regions": regions, "world_vertex": vertices, "world_bound": bounds, "flagged": flagged}
