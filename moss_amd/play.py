"""Using a trained avatar: pose it, render it, score it and write the frames -- without a training step.

:class:`MossPlayer` is the forward half of ``moss_amd.train.MossStep`` as an object of its own: the pose pipeline of
``gaussian_renderer.render`` (pose head -> LBS-weight network -> SMPL frame -> LBS deformation) and the rasterizer, under
``torch.no_grad()``, with no loss, no backward and no optimizer.  It is a composition and a capture; it has no mathematics of its own.
It serves MOSS's evaluation (``train_ZJU.py:242-264`` ``training_report``, ``render_ZJU.py:42-94``) and novel-pose driving: one pose in,
one frame out, nothing trained.

Two kinds of captured graphs, because the two halves change at different rates:

    pose graph (one)        static ``smpl_param`` tensors -> the static tables ``transforms (P,3,3)``, ``translation (P,3)``, ``Rs``
                            ``(23,3,3)``, ``lbs_weights (P,24)``.  Depends on the model and the pose, not on the camera.
    render graphs (LRU)     one per distinct ``(H, W, tanfovx, tanfovy, active_sh_degree, P)`` -- the host scalars a capture bakes
                            in -- each a forward-only ``render()`` from the static tables on a ``RasterContext`` of its own.  The
                            camera's three tensors are static and copied into in place.

MOSS's test split is 17 poses seen by 22 cameras of different intrinsics: each pose is posed once, and each camera's intrinsics are
captured once.  :func:`evaluate_split` is that loop with the device-side metrics of ``moss_amd.metrics``; :func:`frames_to_u8` (C ABI
``moss_frames_to_u8``, csrc/present.hip) and :func:`save_png` write the frames without torchvision, PIL or cv2.

Everything here imports without a GPU; :func:`frames_to_u8_torch`, :func:`save_png` and :func:`read_png` run without one.
"""
from __future__ import annotations

import collections
import ctypes
import math
import os
import struct
import zlib
from types import SimpleNamespace

import numpy as np
import torch

__all__ = ["MossPlayer", "evaluate_split", "frames_to_u8", "frames_to_u8_torch", "save_png", "read_png", "ROUNDINGS",
           "MAX_FRAMES_PER_LAUNCH"]

ROUNDINGS = ("nearest", "truncate")
MAX_FRAMES_PER_LAUNCH = 8
_RENDER_KEYS = ("render", "render_depth", "render_alpha", "radii")
_SMPL_KEYS = ("poses", "shapes", "R", "Th", "pose_rotmats")


# ---- float32 frames -> 8-bit pixels ---------------------------------------------------------------------------------------------------
def _as_list(v, n, what):
    if v is None:
        return [None] * n
    v = list(v) if isinstance(v, (list, tuple)) else [v]
    if len(v) != n:
        raise ValueError(f"frames_to_u8: {len(v)} {what} for {n} images")
    return v


def _bound_of(region):
    return None if region is None else getattr(region, "bound", region)


def _quantise_torch(x, rounding):
    if rounding == "nearest":
        q = x.mul(255).add_(0.5).clamp_(0, 255)                  # torchvision.utils.save_image
    else:
        q = torch.clamp(x, 0.0, 1.0) * 255                       # train_ZJU.py:75
    return torch.where(torch.isnan(q), torch.zeros_like(q), q).to(torch.uint8)   # (NaN -> 0: a float NaN has no uint8 to convert to)


def frames_to_u8_torch(images, alphas=None, regions=None, fill=0.0, rounding="nearest", out=None):
    """:func:`frames_to_u8` in torch ops, on any device: the readable statement of the semantics and the CPU cross-check.

    Per element, in float32, every operation rounded on its own: ``nearest`` is ``x.mul(255).add_(0.5).clamp_(0, 255).to(uint8)``
    (``torchvision.utils.save_image``), ``truncate`` is ``(clamp(x, 0, 1) * 255).byte()`` (``train_ZJU.py:75``); NaN gives 0.  Where a
    region's ``bound`` is not 1 the colour is ``fill`` before it is quantised; alpha becomes the fourth byte, by the same rule, never
    filled."""
    if rounding not in ROUNDINGS:
        raise ValueError(f"frames_to_u8: rounding must be one of {ROUNDINGS}, got {rounding!r}")
    single = not isinstance(images, (list, tuple))
    images = [images] if single else list(images)
    n = len(images)
    alphas, regions, outs = _as_list(alphas, n, "alphas"), _as_list(regions, n, "regions"), _as_list(out, n, "outputs")
    result = []
    for image, alpha, region, o in zip(images, alphas, regions, outs):
        H, W = int(image.shape[-2]), int(image.shape[-1])
        x = image.reshape(3, H, W).to(torch.float32).clone()
        bound = _bound_of(region)
        if bound is not None:
            x.permute(1, 2, 0)[bound.reshape(H, W) != 1] = float(fill)
        planes = [x] if alpha is None else [x, alpha.reshape(1, H, W).to(torch.float32)]
        q = _quantise_torch(torch.cat(planes, 0), rounding).permute(1, 2, 0).contiguous()
        result.append(q if o is None else o.copy_(q))
    return result[0] if single else result


def frames_to_u8(images, alphas=None, regions=None, fill=0.0, rounding="nearest", out=None):
    """(3,H,W) float32 GPU frames -> (H,W,3) uint8, or (H,W,4) with ``alphas`` ((H,W) or (1,H,W) float32): the HIP kernel of
    csrc/present.hip, eight frames of one size per launch (C ABI ``moss_frames_to_u8``).  ``images``: one tensor or a list (then a
    list is returned); ``regions``: per frame a ``loss.ViewRegion`` (or its (H,W) uint8 ``bound``) or None -- where the bound is not 1
    the colour is ``fill``; ``rounding``: ``"nearest"`` (``save_image``) or ``"truncate"`` (``train_ZJU.py:75``); ``out``: contiguous
    uint8 tensors to write into, at any byte address (every byte is written, none beside them).  No host read, no workspace:
    capturable.  :func:`frames_to_u8_torch` states the semantics; the two agree bit for bit."""
    from ._lib import FramesToU8Args, call
    if rounding not in ROUNDINGS:
        raise ValueError(f"frames_to_u8: rounding must be one of {ROUNDINGS}, got {rounding!r}")
    single = not isinstance(images, (list, tuple))
    images = [images] if single else list(images)
    n = len(images)
    if n == 0:
        return []
    alphas, regions, outs = _as_list(alphas, n, "alphas"), _as_list(regions, n, "regions"), _as_list(out, n, "outputs")
    dev = images[0].device
    if dev.type != "cuda":
        raise RuntimeError("frames_to_u8 runs the HIP kernel: it needs GPU tensors (frames_to_u8_torch is the torch form)")
    H, W = int(images[0].shape[-2]), int(images[0].shape[-1])
    C = 4 if alphas[0] is not None else 3

    def need(t, what, dtype, numel):
        if t.dtype != dtype or t.numel() != numel or t.device != dev or not t.is_contiguous():
            raise ValueError(f"frames_to_u8: {what} must be a contiguous {dtype} tensor of {numel} elements on {dev}, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
        return t
    keep, result = [], []
    for i in range(n):
        need(images[i], "an image", torch.float32, 3 * H * W)
        if (alphas[i] is not None) != (C == 4):
            raise ValueError("frames_to_u8: alphas for all frames or for none")
        if alphas[i] is not None:
            need(alphas[i], "an alpha", torch.float32, H * W)
        bound = _bound_of(regions[i])
        if bound is not None:
            need(bound, "a region's bound", torch.uint8, H * W)
        keep.append(bound)
        o = outs[i]
        result.append(torch.empty((H, W, C), dtype=torch.uint8, device=dev) if o is None else need(o, "an output", torch.uint8, H * W * C))
    for k in range(0, n, MAX_FRAMES_PER_LAUNCH):
        a = FramesToU8Args()
        m = min(MAX_FRAMES_PER_LAUNCH, n - k)
        a.num_views, a.H, a.W, a.channels_out, a.rounding, a.fill = m, H, W, C, ROUNDINGS.index(rounding), float(fill)
        for b in range(m):
            a.image[b] = images[k + b].data_ptr()
            a.alpha[b] = None if alphas[k + b] is None else alphas[k + b].data_ptr()
            a.bound[b] = None if keep[k + b] is None else keep[k + b].data_ptr()
            a.out[b] = result[k + b].data_ptr()
        call("moss_frames_to_u8", dev, ctypes.byref(a))
    return result[0] if single else result


# ---- PNG, from the standard library -------------------------------------------------------------------------------------------------
_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_PNG_COLOUR_TYPE = {1: 0, 3: 2, 4: 6}                            # channels -> greyscale, truecolour, truecolour with alpha


def _pixels(array):
    a = array.detach().cpu().numpy() if isinstance(array, torch.Tensor) else np.asarray(array)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (3, 4)) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"save_png: an (H,W), (H,W,3) or (H,W,4) uint8 array is written, got {a.dtype} {tuple(a.shape)}")
    return np.ascontiguousarray(a)


def save_png(path, array):
    """Write an (H,W), (H,W,3) or (H,W,4) uint8 numpy array or CPU tensor as a non-interlaced 8-bit PNG (greyscale, RGB, RGBA), from
    the standard library alone: every scanline with filter type 0, one zlib stream, one IDAT chunk.  The file takes its place whole
    (``checkpoint._replace``): a reader never finds half of one.  What ``torchvision.utils.save_image`` leaves on disk holds the same
    pixels (its encoder may choose other filters)."""
    from .checkpoint import _replace
    a = _pixels(array)
    H, W = a.shape[:2]
    channels = 1 if a.ndim == 2 else a.shape[2]
    rows = np.zeros((H, 1 + W * channels), dtype=np.uint8)       # (column 0: the filter type of the scanline, 0 = None)
    rows[:, 1:] = a.reshape(H, W * channels)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)
    body = (_PNG_SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, _PNG_COLOUR_TYPE[channels], 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))
    _replace(path, lambda f: f.write(body))
    return path


def read_png(path):
    """What :func:`save_png` wrote, as an (H,W) or (H,W,3|4) uint8 numpy array.  It reads that form and nothing else: another bit
    depth, a palette or greyscale-with-alpha image, an interlaced one, a scanline with a filter type other than 0, a bad checksum or
    a truncated file raise ``ValueError`` naming what was found (there is no second decoder to fall back on)."""
    with open(path, "rb") as f:
        data = f.read()
    if not data.startswith(_PNG_SIGNATURE):
        raise ValueError(f"read_png: {path} is no PNG file (it starts with {data[:8]!r})")
    at, header, idat, ended = len(_PNG_SIGNATURE), None, [], False
    while at + 12 <= len(data) and not ended:
        (length,), kind = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        body, crc = data[at + 8:at + 8 + length], data[at + 8 + length:at + 12 + length]
        if len(body) != length or len(crc) != 4:
            raise ValueError(f"read_png: {path}: chunk {kind!r} is truncated")
        if struct.unpack(">I", crc)[0] != (zlib.crc32(kind + body) & 0xffffffff):
            raise ValueError(f"read_png: {path}: chunk {kind!r} fails its checksum")
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            ended = True
        elif kind == b"PLTE":
            raise ValueError(f"read_png: {path} has a palette; only greyscale, RGB and RGBA are read")
        at += 12 + length
    if header is None or not ended or not idat:
        raise ValueError(f"read_png: {path} lacks its IHDR, IDAT or IEND chunk (truncated?)")
    W, H, depth, colour, compression, filtering, interlace = header
    channels = {v: k for k, v in _PNG_COLOUR_TYPE.items()}.get(colour)
    if depth != 8:
        raise ValueError(f"read_png: {path} has bit depth {depth}; only 8 is read")
    if channels is None:
        raise ValueError(f"read_png: {path} has colour type {colour}; only 0 (greyscale), 2 (RGB) and 6 (RGBA) are read")
    if interlace != 0 or compression != 0 or filtering != 0:
        raise ValueError(f"read_png: {path} is interlaced or uses an unknown compression / filter method ({compression}, {filtering}, {interlace})")
    raw = zlib.decompress(b"".join(idat))
    if len(raw) != H * (1 + W * channels):
        raise ValueError(f"read_png: {path} holds {len(raw)} bytes of scanlines where {H * (1 + W * channels)} are expected")
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(H, 1 + W * channels)
    if rows[:, 0].any():
        raise ValueError(f"read_png: {path} uses scanline filters {sorted(set(rows[:, 0].tolist()))}; only filter type 0 is read")
    out = rows[:, 1:].reshape((H, W) if channels == 1 else (H, W, channels))
    return np.array(out)


# ---- the player ------------------------------------------------------------------------------------------------------------------------
class MossPlayer:
    """``player = MossPlayer(pc, view, bg)``; ``player.frame(camera, smpl_param)`` poses the avatar and renders it.

    ``pc``, ``view``: what ``MossStep`` takes -- a ``GaussianSet(unified_features=True)`` with ``auto_regression``,
    ``cross_attention_lbs``, ``SMPL_NEUTRAL``, ``knn`` and ``motion_offset_flag=True``; a camera with ``smpl_param``,
    ``big_pose_smpl_param`` and ``big_pose_world_vertex``.  A model with ``motion_offset_flag=False`` is accepted too: it is posed by
    the SMPL weights alone (``render()``'s ``lbs_in_op`` branch without the two networks; ``Rs`` is then None).  The player owns no
    parameter and never writes one; everything runs under ``torch.no_grad()`` (the rasterizer's forward-only path).

    STATIC: ``view.smpl_param``'s ``poses``, ``shapes``, ``R``, ``Th`` (and ``pose_rotmats``; without one the player keeps
    ``batch_rodrigues(poses)[1:]`` of the frame loaded at construction -- it only feeds the NLL, which is dropped) are the pose
    graph's inputs: change pose by ``copy_`` into them or by ``pose(smpl_param)``.  The four tables, and the camera's
    ``world_view_transform``, ``full_proj_transform`` and ``camera_center``, are tensors of the player: ``render(camera)`` copies a
    camera's three into them.  ``FoVx``, ``FoVy``, ``image_height`` and ``image_width`` are host scalars: they select the render graph.

    ``template_index=True``: the nearest-vertex query goes through a ``knn_cuda.TemplateIndex`` built here, once, from
    ``view.big_pose_world_vertex`` (as in ``MossStep``; the model is not touched).  ``lbs_weights_precision``: ``"f32"`` or
    ``"bf16x3"``, handed to ``cross_attention_lbs_fused``.  ``max_render_graphs``: the size of the LRU; an evicted graph frees its pool.

    ``bounds``: a list of cameras (MOSS ``Camera`` objects with ``K``, ``R``, ``T``, or ``(K, RT)`` pairs; ``True``: ``view`` alone), all
    of ``view``'s frame size.  The player then owns a ``moss_amd.bounds.FrameBounds`` over its static ``smpl_param`` whose five launches
    are part of the pose half: every ``pose()`` also writes the bound masks and rectangles of that pose's RAW ``poses`` for these
    cameras (``bounds_pad``: the box's padding, MOSS's 0.1 m), ``frame()`` returns ``"region"`` beside the render, :meth:`region_of`
    gives any camera's, and ``evaluate_split(..., regions="pose")`` uses them.  Default: no bounds, and nothing changes.

    Before :meth:`capture` everything runs eagerly, with the same results.  After it the pose is one replay and a render is one
    replay; a camera with intrinsics not seen before is captured on first use.  After the warm-up ``frame()`` reads nothing on the
    host.  Call :meth:`check` now and then (it synchronises) and :meth:`refresh` after the model's row count, SH degree or parameter
    storage changed (``load_scene``, a densification event): a stale player raises instead of replaying graphs that hold old
    addresses.

    Counters: ``captures`` (graphs captured: the pose graph and every render graph, evicted ones included), ``recaptures`` (by
    ``check()``), ``poses`` (runs of the pose pipeline), ``pose_replays`` (those that were replays), ``dropped_frames``."""

    def __init__(self, pc, view, bg, template_index=False, lbs_weights_precision="f32", max_render_graphs=32, bounds=False,
                 bounds_pad=0.1):
        from .lbs_weights import PRECISIONS
        if not getattr(pc, "unified_features", False):
            raise ValueError("MossPlayer needs GaussianSet(unified_features=True)")
        self.motion = bool(getattr(pc, "motion_offset_flag", False))
        needs = ("SMPL_NEUTRAL", "knn") + (("auto_regression", "cross_attention_lbs") if self.motion else ())
        missing = [a for a in needs if not hasattr(pc, a)]
        if missing:
            raise ValueError(f"MossPlayer: the model lacks {missing}")
        for a in ("smpl_param", "big_pose_smpl_param", "big_pose_world_vertex"):
            if not hasattr(view, a):
                raise ValueError(f"MossPlayer: the view has no {a}")
        if lbs_weights_precision not in PRECISIONS:
            raise ValueError(f"MossPlayer: lbs_weights_precision must be one of {PRECISIONS}, got {lbs_weights_precision!r}")
        if int(max_render_graphs) < 1:
            raise ValueError("MossPlayer: max_render_graphs must be at least 1")
        self.pc, self.view, self.bg = pc, view, bg
        self.lbs_weights_precision = lbs_weights_precision
        self.max_render_graphs = int(max_render_graphs)
        self.device = dev = pc._xyz.device
        with torch.no_grad():
            from .lbs import batch_rodrigues
            self.smpl_param = dict(view.smpl_param)              # (the caller's tensors themselves: they are the static inputs)
            if "pose_rotmats" not in self.smpl_param:
                self.smpl_param["pose_rotmats"] = batch_rodrigues(self.smpl_param["poses"].reshape(24, 3).float())[1:].contiguous()
            self.template_index = None
            if template_index:
                from .knn_cuda import TemplateIndex
                self.template_index = TemplateIndex(view.big_pose_world_vertex)
            # the three camera tensors every render graph reads
            self._camera = {k: torch.empty_like(getattr(view, k)) for k in ("world_view_transform", "full_proj_transform", "camera_center")}
            for k, t in self._camera.items():
                t.copy_(getattr(view, k))
            self.bounds, self._bounds_index = None, {}
            if bounds:
                from .bounds import FrameBounds, camera_KRT
                cameras = [view] if bounds is True else list(bounds)
                pairs = [c if isinstance(c, (tuple, list)) else camera_KRT(c) for c in cameras]
                self.bounds = FrameBounds(pc.SMPL_NEUTRAL, pairs, int(view.image_height), int(view.image_width), pad=bounds_pad,
                                          smpl_param=self.smpl_param)
                self._bounds_index = {self._camera_key(pair): i for i, pair in reversed(list(enumerate(pairs)))}
        from .gaussian_renderer import intrinsics_of
        self._intrinsics = intrinsics_of(view)
        self.captures = self.poses = self.pose_replays = 0
        self._dropped = self._recaptured = 0
        self._captured = False
        self._last_camera = None
        self._warmup = 2
        self._renders = collections.OrderedDict()                # key -> SimpleNamespace(camera, context, pipe, graphed)
        self._pose_graph = None
        self._tables = None
        # the Parameter objects whose storage the graphs hold by address (an optimizer that re-homes one changes its data_ptr)
        self._held = [pc._xyz, pc._features, pc._opacity, pc._scaling, pc._rotation]
        if self.motion:
            from .train import network_parameters
            head, net = network_parameters(pc)
            self._held += head + net
        self.refresh()

    # ---- what a capture bakes in -----------------------------------------------------------------------------------------------------
    def _signature(self):
        pc = self.pc
        return (int(pc._xyz.shape[0]), int(pc.active_sh_degree), tuple(t.data_ptr() for t in self._held))

    def _fresh(self, who):
        if self._signature() != self._signed:
            P, degree, _ = self._signed
            raise RuntimeError(f"MossPlayer.{who}: the model has changed since the player was built or refreshed (then {P} rows at SH "
                               f"degree {degree}, now {int(self.pc._xyz.shape[0])} at {int(self.pc.active_sh_degree)}, or its parameters "
                               "have moved): its tables and graphs hold the old sizes and addresses; call refresh()")

    def refresh(self):
        """Drop every graph (their pools are freed) and size the static tables for the model as it is now.  A captured player stays
        one: the pose graph and the render graphs are captured again on their next use."""
        dev = self.device
        if self._pose_graph is not None or any(e.graphed is not None for e in self._renders.values()):
            torch.cuda.synchronize(dev)
        for e in self._renders.values():
            self._retire(e)
        self._renders.clear()
        self._pose_graph = None
        self._signed = self._signature()
        P = self._signed[0]
        J = int(self.pc.SMPL_NEUTRAL["weights"].shape[-1])
        self._tables = {"transforms": torch.zeros(1, P, 3, 3, device=dev), "translation": torch.zeros(1, P, 3, device=dev),
                        "Rs": torch.zeros(J - 1, 3, 3, device=dev) if self.motion else None, "lbs_weights": torch.zeros(1, P, J, device=dev)}
        self._posed = False

    # ---- the pose half ---------------------------------------------------------------------------------------------------------------
    def _pose_compute(self):
        """``gaussian_renderer.render``'s ``lbs_in_op`` branch with ``pose_head_in_op``, ``lbs_weights_in_op`` and ``smpl_frame_in_op``,
        call for call, without gradient sinks; the results are copied into the static tables."""
        from .lbs import coarse_deform_c2source
        pc, view, smpl = self.pc, self.view, self.smpl_param
        with torch.no_grad():
            means3D = pc.get_xyz
            extra, Rs = {}, None
            if self.motion:
                from .lbs_weights import cross_attention_lbs_fused
                from .pose import pose_head_fused
                pose_out = pose_head_fused(pc.auto_regression, smpl["poses"], smpl["pose_rotmats"])
                Rs = pose_out["Rs"]
                lbs_weights = cross_attention_lbs_fused(pc.cross_attention_lbs, means3D[None], Rs, precision=self.lbs_weights_precision)
                extra = {"lbs_weights": lbs_weights, "correct_Rs": Rs.reshape(1, 23, 3, 3)}
            model = pc if self.template_index is None else SimpleNamespace(SMPL_NEUTRAL=pc.SMPL_NEUTRAL, knn=pc.knn,
                                                                           template_index=self.template_index)
            _, _, bweights, transforms, translation = coarse_deform_c2source(
                model, means3D[None], smpl, view.big_pose_smpl_param, view.big_pose_world_vertex[None], return_transl=True,
                fused_frame=True, **extra)
            t = self._tables
            t["transforms"].copy_(transforms)
            t["translation"].copy_(translation)
            t["lbs_weights"].copy_(bweights)
            if Rs is not None:
                t["Rs"].copy_(Rs)
            if self.bounds is not None:
                self.bounds.update()                             # (the region of the RAW poses, as the reference's: not of Rs)
        return None

    def pose(self, smpl_param=None):
        """Run the pose pipeline on the static inputs (``smpl_param``: copied into them first; keys it lacks keep their values) and
        return ``{"transforms" (P,3,3), "translation" (P,3), "Rs" (23,3,3), "lbs_weights" (P,24)}`` -- views of the static tables:
        valid until the next ``pose()`` or ``render(transforms=...)``; clone to keep."""
        self._fresh("pose")
        if smpl_param is not None and smpl_param is not self.smpl_param:
            with torch.no_grad():
                for k in _SMPL_KEYS:
                    if k in smpl_param and smpl_param[k] is not self.smpl_param[k]:
                        self.smpl_param[k].copy_(smpl_param[k].reshape(self.smpl_param[k].shape))
        if self._captured:
            if self._pose_graph is None:
                from .diff_gaussian_rasterization import RasterContext
                from .graphs import GraphedStep
                # (a context of its own that no forward ever uses: the pose half has no binning capacity to bake in)
                self._pose_graph = GraphedStep(self._pose_compute, warmup=self._warmup, device=self.device, context=RasterContext())
                self.captures += 1
            self._pose_graph()
            self.pose_replays += 1
        else:
            self._pose_compute()
        self.poses += 1
        self._posed = True
        return self.tables()

    def tables(self):
        t = self._tables
        return {"transforms": t["transforms"][0], "translation": t["translation"][0], "Rs": t["Rs"], "lbs_weights": t["lbs_weights"][0]}

    # ---- the camera half -------------------------------------------------------------------------------------------------------------
    def _entry(self, intrinsics):
        """The render graph (before ``capture()``: the eager render) of these intrinsics at the model's size and degree, most recently
        used last; the least recently used one goes when there are more than ``max_render_graphs``."""
        from .gaussian_renderer import static_view
        H, W, fovx, fovy = intrinsics
        key = (H, W, math.tan(fovx * 0.5), math.tan(fovy * 0.5), self._signed[1], self._signed[0])
        e = self._renders.get(key)
        if e is not None:
            self._renders.move_to_end(key)
            return e
        while len(self._renders) >= self.max_render_graphs:
            _, old = self._renders.popitem(last=False)
            if old.graphed is not None:
                torch.cuda.synchronize(self.device)              # (its last replay has ended before its pool goes)
            self._retire(old)
        camera, cx, pipe = static_view(intrinsics, self._camera)
        e = self._renders[key] = SimpleNamespace(camera=camera, context=cx, pipe=pipe, graphed=None, outputs=None)
        return e

    def _retire(self, e):
        """An entry leaves: what its replays dropped since the last check stays counted; its graph and pool are freed with it."""
        if e.graphed is not None:
            self._dropped += e.graphed.dropped_frames
            self._recaptured += e.graphed.recaptures
            e.graphed = None
        e.outputs = None

    def _render_compute(self, e):
        from .gaussian_renderer import render
        t = self._tables
        with torch.no_grad():
            out = render(e.camera, self.pc, e.pipe, self.bg, transforms=t["transforms"][0], translation=t["translation"][0])
        return {k: out[k].detach() for k in _RENDER_KEYS}

    def render(self, camera=None, transforms=None, translation=None):
        """Render the last pose from ``camera`` (None: the last camera; at first the player's ``view``).  Returns ``{"render" (3,H,W),
        "render_depth", "render_alpha" (1,H,W), "radii" (P,)}`` -- after ``capture()`` the static outputs of this camera's graph, valid
        until its next render.  ``transforms`` (P,3,3) / ``translation`` (P,3) (a leading 1 allowed), both: copied into the static
        tables and rendered from (``render_ZJU.py:56-72`` with the tables of a pose file)."""
        self._fresh("render")
        if (transforms is None) != (translation is None):
            raise ValueError("MossPlayer.render: give transforms and translation together")
        with torch.no_grad():
            if transforms is not None:
                self._tables["transforms"].copy_(transforms.reshape(self._tables["transforms"].shape))
                self._tables["translation"].copy_(translation.reshape(self._tables["translation"].shape))
                self._posed = True
            if camera is not None:
                self._last_camera = camera
                for k, t in self._camera.items():
                    src = getattr(camera, k)
                    if src is not t:
                        t.copy_(src)
                from .gaussian_renderer import intrinsics_of
                self._intrinsics = intrinsics_of(camera)
        if not self._posed:
            raise RuntimeError("MossPlayer.render: nothing is posed yet (pose() or frame() first, or give transforms and translation)")
        e = self._entry(self._intrinsics)
        if not self._captured:
            return self._render_compute(e)
        if e.graphed is None:
            from .graphs import GraphedStep
            e.graphed = GraphedStep(lambda: self._render_compute(e), warmup=self._warmup, device=self.device, context=e.context)
            self.captures += 1
        return e.graphed()

    def frame(self, camera=None, smpl_param=None):
        """``pose(smpl_param)`` then ``render(camera)``; returns the render's dict -- with ``bounds``, a copy of it that also holds
        ``"region"``: :meth:`region_of` the camera."""
        self.pose(smpl_param)
        out = self.render(camera)
        if self.bounds is None:
            return out
        return dict(out, region=self.region_of(camera))

    # ---- the bound masks ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _camera_key(pair):
        K, RT = pair
        return (torch.as_tensor(K, dtype=torch.float32).cpu().numpy().tobytes(), torch.as_tensor(RT, dtype=torch.float32).cpu().numpy().tobytes())

    def bounds_index(self, camera=None):
        """Which of the cameras given as ``bounds=`` ``camera`` is (None: the last one rendered): matched by the values of its ``K``,
        ``R`` and ``T`` -- host arithmetic when those are host arrays, as a MOSS ``Camera``'s are."""
        if self.bounds is None:
            raise RuntimeError("MossPlayer: built without bounds= (MossPlayer(..., bounds=True) or bounds=[cameras])")
        if camera is None:
            camera = self._last_camera if self._last_camera is not None else self.view
        from .bounds import camera_KRT
        i = self._bounds_index.get(self._camera_key(camera if isinstance(camera, (tuple, list)) else camera_KRT(camera)))
        if i is None:
            raise ValueError("MossPlayer: this camera is not among the cameras the player's bounds were built for")
        return i

    def region_of(self, camera=None):
        """The ``ViewRegion`` of the last pose seen by ``camera``: device buffers of the player's ``FrameBounds``, rewritten by the next
        ``pose()``; ``xywh`` is None until ``read()``."""
        i = self.bounds_index(camera)                            # (raises for a player without bounds)
        return self.bounds.regions[i]

    # ---- capture, check ---------------------------------------------------------------------------------------------------------------
    def capture(self, warmup=2):
        """From here on the pose and every render are replays of captured graphs: the pose graph and the render graph of the current
        camera are captured now (``warmup`` eager runs each, which also size the binning capacity), others on first use.  Returns
        ``self``."""
        self._fresh("capture")
        self._captured, self._warmup = True, max(int(warmup), 1)
        self.frame()
        return self

    def check(self) -> bool:
        """Synchronises.  Every live render context is verified as ``GraphedStep.check`` does: a view that overflowed the binning
        capacity baked into its graph rendered nothing -- it is counted in ``dropped_frames`` and that graph is captured again with
        the grown capacity (an eager player's context grows it by itself).  Returns True if anything was captured again."""
        from .diff_gaussian_rasterization._C import CapacityOverflow
        self._fresh("check")
        again = False
        for e in list(self._renders.values()):
            if e.graphed is not None:
                again |= e.graphed.check()
            else:
                try:
                    e.context.check_status()
                except CapacityOverflow:
                    self._dropped += 1
                self._dropped += e.context.read_dropped_frames()
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        return again

    @property
    def dropped_frames(self) -> int:
        return self._dropped + sum(e.graphed.dropped_frames for e in self._renders.values() if e.graphed is not None)

    @property
    def recaptures(self) -> int:
        return self._recaptured + sum(e.graphed.recaptures for e in self._renders.values() if e.graphed is not None)

    @property
    def live_render_graphs(self) -> int:
        return len(self._renders)


# ---- a split: MOSS's training_report body and render_set ---------------------------------------------------------------------------
def evaluate_split(player, views, gts, regions, lpips=None, lpips_references=None, keep_tables=True, out_dir=None, name="test",
                   iteration=0):
    """MOSS's ``training_report`` body for one split (``train_ZJU.py:242-264``) and ``render_ZJU.py``'s ``render_set`` on a
    :class:`MossPlayer`.  ``views``: cameras with ``smpl_param``; those that carry a ``pose_id`` are grouped -- each pose is posed ONCE
    (its tables are kept on the device and copied back in when a pose returns later in the order) -- views without one are posed per
    view.  ``regions``: one ``ViewRegion`` (or None) per view, or ``"pose"``: every view's region comes from the player's bounds
    (``MossPlayer(..., bounds=cameras)``; a pose's masks are kept on the device like its tables).  Per view, in the given order, exactly what ``metrics.evaluate_views`` runs: ``QualityReport.add(image, gt, region,
    out_image)`` and, with ``lpips`` (a float32 ``LpipsVGG``; others are refused as there), ``lpips_vgg_fused`` on ``out_image``
    against the clamped ground truth or its ``LpipsReference``, summed in float64 on the device.  One host read at the end; when
    ``check()`` finds a dropped view the whole split is run again, at most 3 times, then ``RuntimeError``.

    Returns ``{"l1", "psnr", "ssim", "lpips", "n", "tables"}``; ``tables = {pose_id: {"transforms" (1,P,3,3), "translation" (1,P,3)}}``
    -- MOSS's ``smpl_rot`` layout, cloned device tensors, keyed ``("view", i)`` for view i without a ``pose_id`` -- or None with
    ``keep_tables=False``.

    ``out_dir``: also writes ``out_dir/name/ours_{iteration}/renders/{i:05d}.png`` (the clamped, filled render) and ``.../gt/{i:05d}.png``
    (the clamped ground truth), ``render_ZJU.py:32-39,83-84``: both through :func:`frames_to_u8` (``save_image``'s rounding) in one
    launch per view, a non-blocking copy into pinned memory, and :func:`save_png` on a pool of at most 16 threads after the loop.
    Nothing reads the device inside the loop."""
    from .metrics import QualityReport
    who = "evaluate_split"
    if lpips is not None and getattr(lpips, "precision", "f32") != "f32":
        raise ValueError(f"{who}: reported LPIPS is the float32 term; the net given has precision={lpips.precision!r} "
                         "(build a second LpipsVGG with precision='f32' for evaluation)")
    if lpips_references is not None:
        lpips_references = list(lpips_references)
        if lpips is None:
            raise ValueError(f"{who}: lpips_references needs lpips= (the LpipsVGG that made them)")
        for r in lpips_references:
            if getattr(r, "precision", None) != "f32":
                raise ValueError(f"{who}: reported LPIPS is the float32 term; a reference given has precision="
                                 f"{getattr(r, 'precision', None)!r}")
    views, gts = list(views), list(gts)
    n = len(views)
    from_pose = isinstance(regions, str)
    if from_pose:
        if regions != "pose":
            raise ValueError(f"{who}: regions must be a list, None or 'pose', got {regions!r}")
        index = [player.bounds_index(v) for v in views]          # (raises for a player without bounds or a camera it does not know)
        regions = [None] * n
    else:
        regions = list(regions) if regions is not None else [None] * n
    if len(gts) != n or len(regions) != n or n == 0:
        raise ValueError(f"{who}: one ground truth and one region (or None) per view")
    if lpips_references is not None and len(lpips_references) != n:
        raise ValueError(f"{who}: one LPIPS reference per view")
    if lpips is not None:
        from .lpips import lpips_vgg_fused
    dev = player.device
    C, H, W = gts[0].shape
    report = QualityReport(dev, C, H, W, player.bg)
    want_image = lpips is not None or out_dir is not None
    out_image = torch.empty((C, H, W), dtype=torch.float32, device=dev) if want_image else None
    if out_dir is not None:
        staged = torch.empty((2, H, W, 3), dtype=torch.uint8, device=dev)
        landed = torch.empty((n, 2, H, W, 3), dtype=torch.uint8).pin_memory()
    keys = [getattr(v, "pose_id", None) for v in views]
    from .diff_gaussian_rasterization._C import CapacityOverflow

    def region_at(i, key, masks):
        """regions='pose': view i's region over the clones of its pose's masks (a pose's masks are kept like its tables)."""
        from .loss import ViewRegion
        bound, rect = masks[("view", i) if key is None else key]
        return ViewRegion.from_device(bound[index[i]], rect[index[i]])

    def one_pass():
        tables, loaded, masks = {}, object(), {}
        with torch.no_grad():
            for i, view in enumerate(views):
                key = keys[i]
                if key is None or key not in tables:
                    t = player.pose(view.smpl_param)
                    loaded = key if key is not None else object()
                    if from_pose:
                        masks[("view", i) if key is None else key] = (player.bounds.bound.clone(), player.bounds.rect.clone())
                    if key is not None or keep_tables:
                        tables[("view", i) if key is None else key] = {"transforms": t["transforms"][None].clone(),
                                                                       "translation": t["translation"][None].clone()}
                    image = player.render(view)["render"]
                elif key == loaded:
                    image = player.render(view)["render"]
                else:                                            # a pose that was posed earlier in the order: its tables come back
                    image = player.render(view, tables[key]["transforms"], tables[key]["translation"])["render"]
                    loaded = key
                report.add(image, gts[i], region_at(i, key, masks) if from_pose else regions[i], out_image)
                if lpips is not None:
                    truth = torch.clamp(gts[i], 0.0, 1.0) if lpips_references is None else lpips_references[i]
                    report.extra += lpips_vgg_fused(lpips, out_image, truth).mean().double()
                if out_dir is not None:
                    # (save_image's rounding of the ground truth as it is equals that of the clamped one: the rule clamps)
                    frames_to_u8([out_image, gts[i]], out=[staged[0], staged[1]])
                    landed[i].copy_(staged, non_blocking=True)
        return tables, report.sums()                             # the one host read (it synchronises: the pinned copies have landed)

    for attempt in range(3):
        report.reset()
        dropped = player.dropped_frames
        try:
            tables, s = one_pass()
            player.check()
        except CapacityOverflow:                                 # (an eager player's context raises a dropped view itself, a frame late)
            dropped = -1
            player.check()
        if player.dropped_frames == dropped:
            break
        if attempt == 2:
            raise RuntimeError(f"{who}: views kept overflowing the rasterizer's binning capacity")
    if out_dir is not None:
        from concurrent.futures import ThreadPoolExecutor
        from .host import cpu_quota
        base = os.path.join(out_dir, name, f"ours_{int(iteration)}")
        pixels = landed.numpy()
        jobs = [(os.path.join(base, folder, f"{i:05d}.png"), pixels[i, k]) for i in range(n) for k, folder in enumerate(("renders", "gt"))]
        with ThreadPoolExecutor(max_workers=max(1, min(16, cpu_quota()))) as pool:
            list(pool.map(lambda job: save_png(*job), jobs))
    return {"l1": s["l1"] / n, "psnr": s["psnr"] / n, "ssim": s["ssim"] / n, "lpips": s["extra"] / n if lpips is not None else None,
            "n": s["n"], "tables": tables if keep_tables else None}
