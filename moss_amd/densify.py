"""Densification bookkeeping either side of the rasterizer.

Mirrors the three statistics MOSS keeps on ``GaussianModel`` and what it does with them every step
(train_ZJU.py:171-174, scene/gaussian_model.py:815-817), plus the KL test of its KL-guided densify
(scene/gaussian_model.py:586-598, :758-813), plus the DECISION MOSS takes at every densification event -- which Gaussians to clone,
split, merge and prune, and the rows that result (``GaussianModel.densify_and_prune``, :621-666, with ``kl_densify_and_clone`` :495-526,
``kl_densify_and_split`` :528-571, ``kl_merge`` :573-619) -- as fused ops (csrc/densify_decision.hip): ``joint_tables``, ``select_clone /
_split / _merge``, ``prune_mask``, ``clone_rows / split_rows / merge_rows`` and the driver ``densify_and_prune_fused``.  Each phase
costs ONE host read, the count of selected Gaussians (a caller needs it to allocate the new rows).  The surface-change test of the
clone (:503-507, open3d normals) is not rebuilt: it is the optional input ``surface_mask``.  The ``*_torch`` functions restate the
same lines in torch, in the dtype of their inputs, on any device: what the tests compare with.
HIP only (csrc/densify.hip, csrc/densify_decision.hip through the C ABI); the ops have no CPU path.

Frame-parallel training: every rank accumulates the statistics of ITS views locally; ``sync()`` -- called once,
right before a densification decision -- sums ``xyz_gradient_accum`` and ``denom`` and takes the maximum of ``max_radii2D``
over the ranks, so every replica takes the same decision on the same numbers.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import call

__all__ = ["DensifyStats", "densify_stats_update", "neighbour_kl", "cal_kl",
           "joint_tables", "select_clone", "select_split", "select_merge", "prune_mask", "clone_rows", "split_rows", "merge_rows",
           "densify_and_prune_fused", "host_reads",
           "joint_tables_torch", "kl_div_torch", "select_clone_torch", "select_split_torch", "select_merge_torch", "prune_mask_torch",
           "clone_rows_torch", "split_rows_torch", "merge_rows_torch", "matrix_to_quaternion_torch", "build_rotation_torch"]


class DensifyStats:
    """``xyz_gradient_accum (P,1)``, ``denom (P,1)``, ``max_radii2D (P)`` as in GaussianModel.training_setup
    (scene/gaussian_model.py:204-205) / create_from_pcd (:198)."""

    def __init__(self, P: int, device="cuda"):
        self.xyz_gradient_accum = torch.zeros((P, 1), device=device)
        self.denom = torch.zeros((P, 1), device=device)
        self.max_radii2D = torch.zeros((P,), device=device)

    def add(self, radii: torch.Tensor, viewspace_grad: torch.Tensor) -> None:
        """One step's update: ``max_radii2D[vis] = max(.., radii[vis])`` and ``add_densification_stats(viewspace_points, vis)``
        with ``vis = radii > 0``.  ``viewspace_grad`` is ``viewspace_point_tensor.grad`` (P, >= 2 columns)."""
        P = self.denom.shape[0]
        if not radii.is_cuda or not viewspace_grad.is_cuda:
            raise RuntimeError("DensifyStats.add needs GPU tensors; this op has no CPU path")
        if radii.shape != (P,) or radii.dtype != torch.int32 or viewspace_grad.dim() != 2 or viewspace_grad.shape[0] != P \
                or viewspace_grad.shape[1] < 2 or viewspace_grad.dtype != torch.float32:
            raise RuntimeError("DensifyStats.add: expected radii (P) int32 and viewspace_grad (P, >=2) float32")
        if viewspace_grad.stride(1) != 1:
            viewspace_grad = viewspace_grad.contiguous()
        call("moss_densify_stats", radii.device, P, radii.contiguous().data_ptr(), viewspace_grad.data_ptr(), viewspace_grad.stride(0),
             self.xyz_gradient_accum.data_ptr(), self.denom.data_ptr(), self.max_radii2D.data_ptr())

    def sync(self, group=None) -> None:
        """Combine the ranks' locally accumulated statistics (sum, sum, max).  No-op without an initialised process group."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return
        sums = torch.cat([self.xyz_gradient_accum.view(-1), self.denom.view(-1)])
        dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)
        P = self.denom.shape[0]
        self.xyz_gradient_accum.copy_(sums[:P].view(P, 1))
        self.denom.copy_(sums[P:].view(P, 1))
        dist.all_reduce(self.max_radii2D, op=dist.ReduceOp.MAX, group=group)

    def mean_grads(self) -> torch.Tensor:
        """``grads = xyz_gradient_accum / denom; grads[grads.isnan()] = 0`` (scene/gaussian_model.py:721-722)."""
        g = self.xyz_gradient_accum / self.denom
        g[g.isnan()] = 0.0
        return g

    def reset(self, P: int = None) -> None:
        """All three back to zero -- for ``P`` Gaussians if given: ``densification_postfix`` re-creates them at the new size
        (scene/gaussian_model.py:451-454)."""
        if P is not None and int(P) != self.denom.shape[0]:
            dev = self.denom.device
            self.xyz_gradient_accum = torch.zeros((int(P), 1), device=dev)
            self.denom = torch.zeros((int(P), 1), device=dev)
            self.max_radii2D = torch.zeros((int(P),), device=dev)
        else:
            self.xyz_gradient_accum.zero_(); self.denom.zero_(); self.max_radii2D.zero_()

    def prune(self, keep_mask: torch.Tensor) -> None:
        """``prune_points`` keeps the surviving rows of the three statistics (scene/gaussian_model.py:406-410)."""
        keep = keep_mask.to(self.denom.device).bool()
        self.xyz_gradient_accum = self.xyz_gradient_accum[keep].contiguous()
        self.denom = self.denom[keep].contiguous()
        self.max_radii2D = self.max_radii2D[keep].contiguous()


def densify_stats_update(max_radii2D: torch.Tensor, xyz_gradient_accum: torch.Tensor, denom: torch.Tensor,
                         radii: torch.Tensor, viewspace_grad: torch.Tensor) -> None:
    """The per-step bookkeeping of train_ZJU.py:171-174 on the CALLER's tensors (MOSS's ``gaussians.max_radii2D (P)``,
    ``gaussians.xyz_gradient_accum (P,1)``, ``gaussians.denom (P,1)``), in place, in one launch and without the mask -> index host
    synchronisation: what ``patches/train_ZJU.diff`` puts in the place of those two lines."""
    st = DensifyStats.__new__(DensifyStats)
    st.max_radii2D, st.xyz_gradient_accum, st.denom = max_radii2D, xyz_gradient_accum, denom
    for t in (max_radii2D, xyz_gradient_accum, denom):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("densify_stats_update: the statistics must be contiguous float32 GPU tensors")
    st.add(radii, viewspace_grad)


def neighbour_kl(xyz: torch.Tensor, rotation: torch.Tensor, scaling: torch.Tensor, pair_idx: torch.Tensor) -> torch.Tensor:
    """``kl_div`` (scene/gaussian_model.py:773-813) of Gaussian ``pair_idx[:,0]`` against Gaussian ``pair_idx[:,1]``, gather
    fused in.  ``rotation``: raw quaternions; ``scaling``: activated scales.  Returns (P,) float32."""
    if not xyz.is_cuda:
        raise RuntimeError("neighbour_kl needs GPU tensors; this op has no CPU path")
    N = xyz.shape[0]
    if xyz.shape != (N, 3) or rotation.shape != (N, 4) or scaling.shape != (N, 3) or pair_idx.dim() != 2 or pair_idx.shape[1] != 2 \
            or pair_idx.dtype != torch.int64:
        raise RuntimeError("neighbour_kl: expected xyz (N,3), rotation (N,4), scaling (N,3), pair_idx (P,2) int64")
    P = pair_idx.shape[0]
    out = torch.empty((P,), dtype=torch.float32, device=xyz.device)
    x, r, s = (t.detach().float().contiguous() for t in (xyz, rotation, scaling))
    call("moss_neighbour_kl", xyz.device, P, N, x.data_ptr(), r.data_ptr(), s.data_ptr(), pair_idx.contiguous().data_ptr(), out.data_ptr())
    return out


def cal_kl(xyz: torch.Tensor, rotation: torch.Tensor, scaling: torch.Tensor, knn_impl: str = None):
    """The KL of every Gaussian against its nearest other Gaussian: the k = 2 self-query (``knn_near_2``) followed by ``kl_div``,
    as in GaussianModel.cal_kl (scene/gaussian_model.py:758-771) and densify_and_clone/split (:586-598).  Returns
    ``(kl (P,), point_ids (P,2))``; the caller compares with its threshold (``> kl_threshold`` in cal_kl, ``<`` at :598)."""
    from .knn_cuda import knn
    _, ids = knn(xyz.detach()[None], xyz.detach()[None], 2, knn_impl)
    return neighbour_kl(xyz, rotation, scaling, ids[0]), ids[0]


def spatial_order(xyz: torch.Tensor, bits: int = 10) -> torch.Tensor:
    """A permutation that lists the Gaussians along a 3-D Morton (Z-order) curve of their positions (`bits` per axis).

    Nothing in the rasterizer depends on the index order of the Gaussians (ties in depth are broken by the index, as in the
    reference's radix sort of (tile | depth) keys, rasterizer_impl.cu:330-337), but its memory traffic does: a block of 256
    consecutive Gaussians adds to the histogram of every tile it touches (preprocess.hip), reserves a run in each of those tiles
    (binning.hip: scatter) and its instances' records are gathered by Gaussian index (merge_gather, per-Gaussian backward).  MOSS
    starts from the SMPL vertices in mesh order and appends clones and splits next to nothing in particular
    (scene/gaussian_model.py: densification_postfix); re-indexing the set along a space-filling curve whenever it is rebuilt anyway
    (densify / prune, every few hundred iterations) keeps index neighbours spatial neighbours.  Apply the returned permutation to
    every per-Gaussian tensor AND to the optimizer state (`FlatAdamW.permute_rows`; `GaussianSet.reorder_spatially` does both)."""
    with torch.no_grad():
        p = xyz.detach().float()
        lo = p.min(dim=0).values
        span = (p.max(dim=0).values - lo).clamp_min(1e-12)
        q = ((p - lo) / span * (2 ** bits - 1)).round().to(torch.int64).clamp_(0, 2 ** bits - 1)
        code = torch.zeros(p.shape[0], dtype=torch.int64, device=p.device)
        for b in range(bits):
            for a in range(3):
                code |= ((q[:, a] >> b) & 1) << (3 * b + a)
        return torch.argsort(code, stable=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# The densify-and-prune DECISION (scene/gaussian_model.py:621-666 and :495-619) -- fused ops
# ---------------------------------------------------------------------------------------------------------------------------------
MAX_POINTS = 45695               # "Control the Gaussians num." (:496, :530, :574): a phase returns early above this many rows
JOINTS = 24
_host_reads = 0
_pinned = {}


def host_reads() -> int:
    """How many times the fused decision OPS have made the host wait for the device in this process: one per selection, its count.
    The ops' own reads only -- what a caller does around them (``FlatAdamW.prune_rows`` indexes with a boolean mask, which
    synchronises too) is not counted here."""
    return _host_reads


def _need_gpu(what, *tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{what} needs GPU tensors; this op has no CPU path (the torch form is {what}_torch)")


def _f32(t):
    return t.detach().float().contiguous()


def joint_tables(joint_F_sum: torch.Tensor, denom: torch.Tensor) -> torch.Tensor:
    """``joint_F / denom[0]`` -> SVD -> ``U[:,2] *= det U, V[:,2] *= det V`` -> ``U V^T`` (:624-635) as the (24,12) table
    ``[rot (9) | S (3)]`` whose row 0 is ones (:637,640).  ``joint_F_sum`` (23,3,3); ``denom``: the statistics' ``denom``, of which
    element 0 is read ON THE DEVICE.  One launch."""
    _need_gpu("joint_tables", joint_F_sum, denom)
    if joint_F_sum.numel() != 23 * 9 or denom.numel() < 1:
        raise RuntimeError("joint_tables: expected joint_F_sum (23,3,3) and a non-empty denom")
    table = torch.empty((JOINTS, 12), dtype=torch.float32, device=joint_F_sum.device)
    F, d = _f32(joint_F_sum), _f32(denom)
    call("moss_densify_joint_table", F.device, F.data_ptr(), d.data_ptr(), table.data_ptr())
    return table


def _select(mode, P, dev, *, xyz=None, rotation=None, scaling=None, opacity=None, ids=None, accum=None, denom=None, n_grads=0,
            surface_mask=None, max_radii2D=None, vertex_dist=None, max_grad=0.0, scale_limit=0.0, kl_threshold=0.0, min_opacity=0.0,
            max_screen_size=None, world_scale_limit=0.0, want_kl=False, index_out=None, read_count=True):
    """One ``moss_densify_select`` call: (mask bool (P,), index int32 (count,), count, kl or None)."""
    global _host_reads
    mask = torch.empty((P,), dtype=torch.uint8, device=dev)
    index = index_out if index_out is not None else torch.empty((max(P, 1),), dtype=torch.int32, device=dev)
    if index.dtype != torch.int32 or index.numel() < P or not index.is_contiguous() or index.device != mask.device:
        raise RuntimeError("select: index_out must be a contiguous int32 tensor of at least P entries on the inputs' device")
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    kl = torch.empty((P,), dtype=torch.float32, device=dev) if want_kl else None
    nbytes = 4 * max((P + 255) // 256, 1) if mode == "prune" else int(_lib.lib().moss_densify_select_workspace_bytes(P))   # (PRUNE: the totals alone)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    host = None
    if read_count:
        host = _pinned.get(dev)
        if host is None:
            host = _pinned[dev] = torch.zeros((1,), dtype=torch.int32).pin_memory()
    keep = [None if t is None else _f32(t) for t in (accum, denom, xyz, rotation, scaling, opacity, max_radii2D, vertex_dist)]
    ids_c = None if ids is None else ids.contiguous()
    surf = None if surface_mask is None else surface_mask.to(torch.uint8).contiguous()
    a = _lib.DensifySelectArgs()
    a.mode, a.P, a.n_grads = _lib.DENSIFY_MODES[mode], P, int(n_grads)
    (a.xyz_gradient_accum, a.denom, a.xyz, a.rotation, a.scaling, a.opacity, a.max_radii2D, a.vertex_dist) = [_lib.ptr(t) for t in keep]
    a.ids, a.surface_mask = _lib.ptr(ids_c), _lib.ptr(surf)
    a.max_grad, a.scale_limit, a.kl_threshold, a.min_opacity = float(max_grad), float(scale_limit), float(kl_threshold), float(min_opacity)
    a.max_screen_size, a.use_screen_size = float(max_screen_size or 0.0), int(bool(max_screen_size))
    a.world_scale_limit, a.vertex_dist_limit = float(world_scale_limit), 0.05
    a.mask, a.index, a.count, a.count_host, a.kl_out = mask.data_ptr(), index.data_ptr(), count.data_ptr(), _lib.ptr(host), _lib.ptr(kl)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    call("moss_densify_select", dev, ctypes.byref(a))
    n = None
    if read_count:
        torch.cuda.current_stream(dev).synchronize()          # THE host read of the phase
        _host_reads += 1
        n = int(host[0])
    return mask.view(torch.bool), (index[:n] if n is not None else index), n, kl


def _check_gaussians(what, xyz, rotation, scaling, ids):
    _need_gpu(what, xyz, rotation, scaling, ids)
    P = xyz.shape[0]
    if xyz.shape != (P, 3) or rotation.shape != (P, 4) or scaling.shape != (P, 3) or ids.shape != (P, 2) or ids.dtype != torch.int64:
        raise RuntimeError(f"{what}: expected xyz (P,3), rotation (P,4), scaling (P,3) raw, ids (P,2) int64")
    return P


def _select_phase(mode, what, xyz, rotation, scaling, ids, xyz_gradient_accum, denom, max_grad, extent, percent_dense, kl_threshold,
                  surface_mask, want_kl, index_out):
    P = _check_gaussians(what, xyz, rotation, scaling, ids)
    n_grads = int(xyz_gradient_accum.numel())
    if int(denom.numel()) != n_grads or n_grads > P:
        raise RuntimeError(f"{what}: xyz_gradient_accum and denom must have the same number of rows, at most P")
    if surface_mask is not None and int(surface_mask.numel()) != P:
        raise RuntimeError(f"{what}: surface_mask must have P entries")
    mask, index, n, kl = _select(mode, P, xyz.device, xyz=xyz, rotation=rotation, scaling=scaling, ids=ids, accum=xyz_gradient_accum,
                                 denom=denom, n_grads=n_grads, surface_mask=surface_mask, max_grad=max_grad,
                                 scale_limit=percent_dense * extent, kl_threshold=kl_threshold, want_kl=want_kl, index_out=index_out)
    return (mask, index, n, kl) if want_kl else (mask, index, n)


def select_clone(xyz, rotation, scaling, ids, xyz_gradient_accum, denom, max_grad, extent, percent_dense=0.01, kl_threshold=0.4,
                 surface_mask=None, want_kl=False, index_out=None):
    """The selection of ``kl_densify_and_clone`` (:499-509): ``|grad| >= max_grad``, ``max(exp(scaling)) <= percent_dense * extent``,
    ``KL > kl_threshold`` and ``surface_mask`` (None = all True).  ``scaling`` is the RAW parameter; ``ids (P,2)`` the k = 2 self
    query; ``xyz_gradient_accum`` / ``denom`` the statistics (n_grads <= P rows; rows beyond have gradient 0).  Returns
    ``(mask (P,) bool, index (count,) int32 ascending, count)`` -- and the KL (P,) with ``want_kl``.  One host read: the count."""
    return _select_phase("clone", "select_clone", xyz, rotation, scaling, ids, xyz_gradient_accum, denom, max_grad, extent, percent_dense,
                         kl_threshold, surface_mask, want_kl, index_out)


def select_split(xyz, rotation, scaling, ids, xyz_gradient_accum, denom, max_grad, extent, percent_dense=0.01, kl_threshold=0.4,
                 want_kl=False, index_out=None):
    """The selection of ``kl_densify_and_split`` (:540-549): the zero-padded gradient ``>= max_grad``, ``max scale > percent_dense *
    extent`` and ``KL > kl_threshold``.  Arguments and result as :func:`select_clone`."""
    return _select_phase("split", "select_split", xyz, rotation, scaling, ids, xyz_gradient_accum, denom, max_grad, extent, percent_dense,
                         kl_threshold, None, want_kl, index_out)


def select_merge(xyz, rotation, scaling, ids, xyz_gradient_accum, denom, max_grad, extent, percent_dense=0.01, kl_threshold=0.1,
                 want_kl=False, index_out=None):
    """The selection of ``kl_merge`` (:579-602): gradient test, ``max scale <= percent_dense * extent`` and ``KL < kl_threshold``."""
    return _select_phase("merge", "select_merge", xyz, rotation, scaling, ids, xyz_gradient_accum, denom, max_grad, extent, percent_dense,
                         kl_threshold, None, want_kl, index_out)


def _prune_select(opacity, scaling, max_radii2D, vertex_dist, min_opacity, extent, max_screen_size, read_count):
    _need_gpu("prune_mask", opacity, scaling, max_radii2D, vertex_dist)
    P = scaling.shape[0]
    if scaling.shape != (P, 3) or opacity.numel() != P or vertex_dist.numel() != P or (max_screen_size and max_radii2D.numel() != P):
        raise RuntimeError("prune_mask: expected opacity (P,1), scaling (P,3), max_radii2D (P), vertex_dist (P)")
    return _select("prune", P, scaling.device, scaling=scaling, opacity=opacity, max_radii2D=max_radii2D if max_screen_size else None,
                   vertex_dist=vertex_dist, min_opacity=min_opacity, max_screen_size=max_screen_size, world_scale_limit=0.1 * extent,
                   read_count=read_count)


def prune_mask(opacity, scaling, max_radii2D, vertex_dist, min_opacity, extent, max_screen_size=None):
    """The final prune mask (:650-662): ``sigmoid(opacity) < min_opacity``, OR -- when ``max_screen_size`` is given -- ``max_radii2D >
    max_screen_size`` or ``max scale > 0.1 extent``, OR ``vertex_dist > 0.05`` (the k = 1 distances to the SMPL vertices, from
    ``knn``).  RAW opacity and scaling.  Returns the (P,) bool mask; queued work, no host read."""
    return _prune_select(opacity, scaling, max_radii2D, vertex_dist, min_opacity, extent, max_screen_size, False)[0]


def _emit(mode, what, index, xyz, features_dc, features_rest, opacity, scaling, rotation, *, noise=None, ids=None, lbs_weights=None,
          denom=None, table=None, prune=None):
    _need_gpu(what, index, xyz, features_dc, features_rest, opacity, scaling, rotation, noise, ids, lbs_weights, denom, table, prune)
    P, n_sel = int(xyz.shape[0]), int(index.numel())
    n_new = 2 * n_sel if mode == "split" else n_sel
    dev = xyz.device
    rest = int(features_rest[0].numel()) if P else int(features_rest.shape[1] * features_rest.shape[2])
    if index.dtype != torch.int32 or xyz.shape != (P, 3) or scaling.shape != (P, 3) or rotation.shape != (P, 4) or opacity.numel() != P \
            or features_dc.shape[0] != P or features_rest.shape[0] != P or int(features_dc[0].numel() if P else 3) != 3:
        raise RuntimeError(f"{what}: expected index int32, xyz (P,3), features_dc (P,1,3), features_rest (P,K-1,3), opacity (P,1), "
                           "scaling (P,3), rotation (P,4)")
    if noise is not None and (tuple(noise.shape) != (n_new, 3)):
        raise RuntimeError(f"{what}: noise must be ({n_new},3): one standard normal draw per new row")

    def rows_of(t, width):
        """A float32 view whose rows are ``width`` contiguous floats: (tensor kept alive, row stride in floats)."""
        t = t.detach()
        if t.dtype != torch.float32 or (P and (t[0].numel() != width or not t[0].is_contiguous())):
            t = t.float().contiguous()
        return t, (int(t.stride(0)) if P > 1 else width)
    dc, dc_stride = rows_of(features_dc, 3)
    fr, rest_stride = rows_of(features_rest, rest)
    out = {"new_xyz": torch.empty((n_new, 3), device=dev), "new_features_dc": torch.empty((n_new,) + tuple(features_dc.shape[1:]), device=dev),
           "new_features_rest": torch.empty((n_new,) + tuple(features_rest.shape[1:]), device=dev),
           "new_opacities": torch.empty((n_new, 1), device=dev), "new_scaling": torch.empty((n_new, 3), device=dev),
           "new_rotation": torch.empty((n_new, 4), device=dev)}
    keep = [_f32(t) for t in (xyz, opacity, scaling, rotation)]
    extra = [None if t is None else _f32(t) for t in (lbs_weights, denom, table, noise)]
    index_c, ids_c = index.contiguous(), None if ids is None else ids.contiguous()
    if lbs_weights is not None and extra[0].numel() != P * JOINTS:
        raise RuntimeError(f"{what}: lbs_weights must be (P,{JOINTS})")
    if prune is not None and (prune.dtype != torch.bool or prune.numel() != P or not prune.is_contiguous()):
        raise RuntimeError(f"{what}: the prune mask must be a contiguous (P,) bool tensor")
    a = _lib.DensifyEmitArgs()
    a.mode, a.P, a.n_sel, a.n_new, a.rest_floats, a.dc_stride, a.rest_stride = _lib.DENSIFY_MODES[mode], P, n_sel, n_new, rest, dc_stride, rest_stride
    a.index, a.ids = index_c.data_ptr(), _lib.ptr(ids_c)
    a.xyz, a.opacity, a.scaling, a.rotation = [t.data_ptr() for t in keep]
    a.features_dc, a.features_rest = dc.data_ptr(), fr.data_ptr()
    a.lbs_weights, a.denom, a.table, a.noise = [_lib.ptr(t) for t in extra]
    a.new_xyz, a.new_features_dc, a.new_features_rest = out["new_xyz"].data_ptr(), out["new_features_dc"].data_ptr(), out["new_features_rest"].data_ptr()
    a.new_opacity, a.new_scaling, a.new_rotation = out["new_opacities"].data_ptr(), out["new_scaling"].data_ptr(), out["new_rotation"].data_ptr()
    a.prune_mask = _lib.ptr(prune)
    call("moss_densify_emit", dev, ctypes.byref(a))
    return out


def clone_rows(index, noise, xyz, features_dc, features_rest, opacity, scaling, rotation, lbs_weights, denom, table):
    """The new rows of ``kl_densify_and_clone`` (:511-524) for the selected ``index``: per Gaussian ``rot_joint = w . table[:, :9]``,
    ``scl_joint = w . table[:, 9:]`` with ``w = lbs_weights[i] / denom[0]`` (the ACCUMULATED weights (P,24); :625,638,641), then
    ``std = scl_joint exp(scaling)``, ``new_xyz = (rot_joint R(q)) (std noise) + xyz``, ``new_scaling = log(exp(scaling) scl_joint)``,
    ``new_rotation = matrix_to_quaternion(rot_joint) * rotation`` (elementwise, as the reference).  ``noise (n,3)``: standard normal
    draws.  Returns the dict ``surgery.densification_event`` takes as ``append`` (with ``source``)."""
    out = _emit("clone", "clone_rows", index, xyz, features_dc, features_rest, opacity, scaling, rotation, noise=noise,
                lbs_weights=lbs_weights, denom=denom, table=table)
    out["source"] = index.long()
    return out


def split_rows(index, noise, xyz, features_dc, features_rest, opacity, scaling, rotation):
    """The 2 n new rows of ``kl_densify_and_split`` (:551-566), N = 2: rows r and n + r derive from ``index[r]`` (``repeat(N,1)``);
    ``new_xyz = R(q)(exp(scaling) noise) + xyz``, ``new_scaling = log(exp(scaling) / 1.6)``, the rest copied.  ``noise (2n,3)``."""
    out = _emit("split", "split_rows", index, xyz, features_dc, features_rest, opacity, scaling, rotation, noise=noise)
    out["source"] = index.long().repeat(2)
    return out


def merge_rows(index, ids, mask, xyz, features_dc, features_rest, opacity, scaling, rotation):
    """The n new rows of ``kl_merge`` (:606-612): means over the pair ``ids[i]`` of xyz, features and raw opacity, ``log(exp(scaling[a])
    / 0.8)`` and ``rotation[a]`` of the pair's first member -- and ``mask[ids[i,1]] = True`` IN PLACE (:616): ``mask`` (the
    selection) becomes the prune filter of the old rows."""
    out = _emit("merge", "merge_rows", index, xyz, features_dc, features_rest, opacity, scaling, rotation, ids=ids, prune=mask)
    out["source"] = ids[index.long(), 0]
    return out


def densify_and_prune_fused(pc, optimizer, stats, joint_F, lbs_weights, max_grad, min_opacity, extent, max_screen_size, t_vertices,
                            kl_threshold=0.4, surface_mask=None, generator=None, percent_dense=0.01, one_pass=False,
                            template_index=None):
    """``GaussianModel.densify_and_prune`` (:621-666) on a ``GaussianSet`` + ``FlatAdamW`` (or an ``optim.FlatAdamWRows`` over several:
    ``MossStep.rows``) + ``DensifyStats``, in MOSS's order:
    clone-append; split-append and its prune; merge-append and its prune; the final prune -- every selection and every new row from
    the fused ops, every append / prune through ``pc.densification_postfix`` / ``pc.prune_points``.

    As the reference: ``grads``, ``joint_F / denom[0]`` and ``lbs_weights / denom[0]`` are those of the statistics AT THE CALL (the
    appends re-zero the statistics; the gradients stay row-indexed as they were, :540-541, :579-580, also after the split's prune has
    moved the rows); each phase is skipped above ``MAX_POINTS`` rows, on the row count it finds (:496,530,574); the neighbours are
    queried again before each phase; ``max_radii2D`` is the CURRENT statistic in the final prune, i.e. zero unless every phase was
    skipped.  ``joint_F`` (23,3,3) and ``lbs_weights`` (P,24) or (1,P,24) are the accumulated sums; ``t_vertices`` (V,3) or (1,V,3);
    ``surface_mask`` (P,) bool or None: the clone's surface-change test (:503-507), computed by the caller.  ``generator``: a
    ``torch.Generator`` of the device for the noise, or a callable ``n -> (n,3)`` standard normal draws.

    ``one_pass=True``: every append and the prune that follows it are carried out by ONE gather pass over the optimizer's flat
    buffers (``GaussianSet.relayout_points``, C ABI ``moss_rows_relayout``) instead of a torch pass per tensor and step -- the clone
    is one re-layout, the split-append with its prune one, the merge-append with its prune one, the final prune one; same bits.  The
    report then carries ``relayouts`` (at most 4), and ``host_reads`` includes the read of a row map's length where the phase's
    count does not already give it (the merge, whose mask ``merge_rows`` extends on the device).

    ``template_index``: a ``knn_cuda.TemplateIndex`` over ``t_vertices``; the final prune's vertex distance (:657) then comes from it
    (the same distances, no grid build).

    Follow it with ``surgery.densification_event(pc, optimizer, rows_changed=True, context=..., graphed=..., probe=...)``.
    Returns a report: rows per phase and ``host_reads``, the reads of the decision ops themselves (one count per phase and the
    prune's: at most 4) -- NOT those of the appends and prunes it then carries out (``prune_points`` synchronises on its mask), nor
    of the event's tail."""
    from .knn_cuda import knn
    dev = pc._xyz.device
    _need_gpu("densify_and_prune_fused", pc._xyz)
    reads0 = host_reads()
    with torch.no_grad():
        accum, denom = stats.xyz_gradient_accum.detach().reshape(-1).clone(), stats.denom.detach().reshape(-1).clone()
        table = joint_tables(joint_F, denom)
        lbs_w = lbs_weights.detach().reshape(-1, JOINTS)
        report = {"rows_before": int(pc._xyz.shape[0]), "cloned": 0, "split": 0, "merged": 0, "pruned": 0}
        if one_pass:
            report["relayouts"] = 0

        def draw(n):
            if callable(generator):
                return generator(n).to(dev).float()
            return torch.randn((n, 3), generator=generator, device=dev, dtype=torch.float32)

        def gaussians():
            return (pc._xyz.detach(), pc._features_dc.detach(), pc._features_rest.detach(), pc._opacity.detach(), pc._scaling.detach(),
                    pc._rotation.detach())

        def neighbours(xyz):
            return knn(xyz[None], xyz[None], 2)[1][0]

        def relayout(rows, remove, rows_new=None):
            pc.relayout_points(optimizer, remove_mask=remove, new_rows=rows, stats=stats, rows_new=rows_new)
            report["relayouts"] += 1

        def append(rows):
            pc.densification_postfix(rows["new_xyz"], rows["new_features_dc"], rows["new_features_rest"], rows["new_opacities"],
                                     rows["new_scaling"], rows["new_rotation"], optimizer, stats=stats)

        def tail(n):
            return torch.zeros((n,), dtype=torch.bool, device=dev)
        args = dict(max_grad=max_grad, extent=extent, percent_dense=percent_dense)
        # ---- kl_densify_and_clone (:495-526)
        if int(pc._xyz.shape[0]) <= MAX_POINTS:
            xyz, fdc, frest, opa, scl, rot = gaussians()
            mask, index, n = select_clone(xyz, rot, scl, neighbours(xyz), accum, denom, kl_threshold=kl_threshold, surface_mask=surface_mask, **args)
            if n and one_pass:
                relayout(clone_rows(index, draw(n), xyz, fdc, frest, opa, scl, rot, lbs_w, denom, table), None)
            elif n:
                append(clone_rows(index, draw(n), xyz, fdc, frest, opa, scl, rot, lbs_w, denom, table))
            elif stats is not None:
                stats.reset()                                 # (densification_postfix re-zeroes the statistics for zero new rows too, :452-454)
            report["cloned"] = n
        # ---- kl_densify_and_split (:528-571)
        if int(pc._xyz.shape[0]) <= MAX_POINTS:
            xyz, fdc, frest, opa, scl, rot = gaussians()
            mask, index, n = select_split(xyz, rot, scl, neighbours(xyz), accum, denom, kl_threshold=kl_threshold, **args)
            if n and one_pass:                                # (the mask has exactly n rows set: the new row count needs no read)
                relayout(split_rows(index, draw(2 * n), xyz, fdc, frest, opa, scl, rot), mask, int(xyz.shape[0]) + n)
            elif n:
                append(split_rows(index, draw(2 * n), xyz, fdc, frest, opa, scl, rot))
                pc.prune_points(torch.cat((mask, tail(2 * n))), optimizer, stats=stats)
            elif stats is not None:
                stats.reset()
            report["split"] = n
        # ---- kl_merge (:573-619)
        if int(pc._xyz.shape[0]) <= MAX_POINTS:
            xyz, fdc, frest, opa, scl, rot = gaussians()
            ids = neighbours(xyz)
            mask, index, n = select_merge(xyz, rot, scl, ids, accum, denom, kl_threshold=0.1, **args)
            if n >= 1:
                mask = mask.clone()
                rows = merge_rows(index, ids, mask, xyz, fdc, frest, opa, scl, rot)
                if one_pass:                                 # (merge_rows added the pairs' second members to the mask: its count is read)
                    relayout(rows, mask)
                else:
                    append(rows)
                    pc.prune_points(torch.cat((mask, tail(n))), optimizer, stats=stats)
            report["merged"] = n
        # ---- the final prune (:650-664)
        xyz, _, _, opa, scl, _ = gaussians()
        if template_index is not None:
            dist = template_index.query(xyz, want_dist=True)[1]
        else:
            tv = t_vertices.detach().reshape(1, -1, 3).to(dev).float()
            dist = knn(tv, xyz[None], 1)[0].reshape(-1)
        max_radii = stats.max_radii2D if stats is not None else torch.zeros((xyz.shape[0],), device=dev)
        mask, _, n, _ = _prune_select(opa, scl, max_radii, dist, min_opacity, extent, max_screen_size, True)
        if n and one_pass:
            relayout(None, mask, int(xyz.shape[0]) - n)
        elif n:
            pc.prune_points(mask, optimizer, stats=stats)
        report["pruned"] = n
    report["rows_after"] = int(pc._xyz.shape[0])
    report["host_reads"] = host_reads() - reads0
    return report


# ---------------------------------------------------------------------------------------------------------------------------------
# The same lines restated in torch, in the dtype and on the device of the inputs (float64-capable): what the tests compare with
# ---------------------------------------------------------------------------------------------------------------------------------
def build_rotation_torch(r):
    """utils/general_utils.py:79-100."""
    q = r / torch.sqrt((r * r).sum(1))[:, None]
    a, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - a * z), 2 * (x * z + a * y),
                        2 * (x * y + a * z), 1 - 2 * (x * x + z * z), 2 * (y * z - a * x),
                        2 * (x * z - a * y), 2 * (y * z + a * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def matrix_to_quaternion_torch(m):
    """pytorch3d.transforms.matrix_to_quaternion (m (...,3,3) -> (...,4), real part first): ``q_abs = sqrt(max(0, 1 +- m00 +- m11 +-
    m22))``, the candidate built around the largest ``q_abs``, divided by ``2 max(q_abs, 0.1)``; no sign standardisation (with the
    real part largest, as MOSS's joint rotations give it, every release agrees)."""
    m = m.reshape(-1, 9)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m.unbind(1)
    t = torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], dim=1)
    q_abs = torch.where(t > 0, torch.sqrt(t.clamp_min(0)), torch.zeros_like(t))
    cand = torch.stack([torch.stack([q_abs[:, 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=1),
                        torch.stack([m21 - m12, q_abs[:, 1] ** 2, m10 + m01, m02 + m20], dim=1),
                        torch.stack([m02 - m20, m10 + m01, q_abs[:, 2] ** 2, m12 + m21], dim=1),
                        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[:, 3] ** 2], dim=1)], dim=1)
    cand = cand / (2.0 * q_abs[:, :, None].clamp_min(0.1))
    best = q_abs.argmax(dim=1)
    return cand[torch.arange(m.shape[0], device=m.device), best]


def joint_tables_torch(joint_F_sum, denom):
    """:624-640 as the (24,12) table of :func:`joint_tables`; a joint whose ``F`` is not finite gives a row of NaN."""
    F = joint_F_sum.reshape(23, 3, 3) / denom.reshape(-1)[0]
    ok = torch.isfinite(F).reshape(23, 9).all(1)
    U, S, Vh = torch.linalg.svd(torch.where(ok[:, None, None], F, torch.eye(3, dtype=F.dtype, device=F.device).expand(23, 3, 3)))
    U, V = U.clone(), Vh.transpose(1, 2).clone()
    U[:, :, 2] *= torch.linalg.det(U)[:, None]
    V[:, :, 2] *= torch.linalg.det(V)[:, None]
    rot = U @ V.transpose(1, 2)
    rows = torch.cat([rot.reshape(23, 9), S], dim=1)
    rows = torch.where(ok[:, None], rows, torch.full_like(rows, float("nan")))
    return torch.cat([torch.ones((1, 12), dtype=F.dtype, device=F.device), rows], dim=0)


def kl_div_torch(xyz, rotation, scaling, ids):
    """``kl_div`` (:776-814) of Gaussian ``ids[:,0]`` against ``ids[:,1]`` as ``cal_kl`` (:758-772) gathers them; ``scaling`` ACTIVATED."""
    mu0, mu1 = xyz[ids[:, 0]], xyz[ids[:, 1]]
    s0, s1 = scaling[ids[:, 0]], scaling[ids[:, 1]]
    L0 = build_rotation_torch(rotation[ids[:, 0]]) @ torch.diag_embed(s0)
    cov0 = L0 @ L0.transpose(1, 2)
    L1i = build_rotation_torch(rotation[ids[:, 1]]) @ torch.diag_embed(1 / s1)
    cov1i = L1i @ L1i.transpose(1, 2)
    d = mu1 - mu0
    k0 = torch.diagonal(cov1i @ cov0, dim1=-2, dim2=-1).sum(-1)
    k1 = (d[:, None] @ cov1i @ d[..., None]).reshape(-1)
    k2 = torch.log(torch.prod((s1 / s0) ** 2, dim=1))
    return 0.5 * (k0 + k1 + k2 - 3)


def _padded_grad(xyz_gradient_accum, denom, P):
    g = (xyz_gradient_accum.reshape(-1) / denom.reshape(-1))
    g = torch.where(g.isnan(), torch.zeros_like(g), g)
    out = torch.zeros((P,), dtype=g.dtype, device=g.device)
    out[:g.shape[0]] = g
    return out


def _select_torch(mode, xyz, rotation, scaling, ids, xyz_gradient_accum, denom, max_grad, extent, percent_dense, kl_threshold, surface_mask):
    P = xyz.shape[0]
    g = _padded_grad(xyz_gradient_accum, denom, P)
    if mode == "clone":
        g = g.abs()
    act = torch.exp(scaling)
    smax = act.max(dim=1).values
    ok = ((ids >= 0) & (ids < P)).all(1)
    kl = torch.full((P,), float("nan"), dtype=xyz.dtype, device=xyz.device)
    kl[ok] = kl_div_torch(xyz, rotation, act, ids[ok])
    sel = (g >= max_grad) & ((smax > percent_dense * extent) if mode == "split" else (smax <= percent_dense * extent))
    sel = sel & ((kl < kl_threshold) if mode == "merge" else (kl > kl_threshold))
    if mode == "clone" and surface_mask is not None:
        sel = sel & surface_mask.bool()
    index = torch.nonzero(sel).reshape(-1)
    return sel, index, int(index.numel())


def select_clone_torch(xyz, rotation, scaling, ids, xyz_gradient_accum, denom, max_grad, extent, percent_dense=0.01, kl_threshold=0.4,
                       surface_mask=None):
    """:499-509 in torch: ``(mask, index int64, count)``."""
    return _select_torch("clone", xyz, rotation, scaling, ids, xyz_gradient_accum, denom, max_grad, extent, percent_dense, kl_threshold, surface_mask)


def select_split_torch(xyz, rotation, scaling, ids, xyz_gradient_accum, denom, max_grad, extent, percent_dense=0.01, kl_threshold=0.4):
    """:540-549 in torch."""
    return _select_torch("split", xyz, rotation, scaling, ids, xyz_gradient_accum, denom, max_grad, extent, percent_dense, kl_threshold, None)


def select_merge_torch(xyz, rotation, scaling, ids, xyz_gradient_accum, denom, max_grad, extent, percent_dense=0.01, kl_threshold=0.1):
    """:579-602 in torch."""
    return _select_torch("merge", xyz, rotation, scaling, ids, xyz_gradient_accum, denom, max_grad, extent, percent_dense, kl_threshold, None)


def prune_mask_torch(opacity, scaling, max_radii2D, vertex_dist, min_opacity, extent, max_screen_size=None):
    """:650-662 in torch."""
    m = torch.sigmoid(opacity.reshape(-1)) < min_opacity
    if max_screen_size:
        m = m | (max_radii2D.reshape(-1) > max_screen_size) | (torch.exp(scaling).max(dim=1).values > 0.1 * extent)
    return m | (vertex_dist.reshape(-1) > 0.05)


def clone_rows_torch(index, noise, xyz, features_dc, features_rest, opacity, scaling, rotation, lbs_weights, denom, table):
    """:511-524 in torch (with :625,638,641 for the selected rows)."""
    i = index.long()
    w = lbs_weights.reshape(-1, JOINTS)[i] / denom.reshape(-1)[0]
    rot_joint, scl_joint = (w @ table[:, :9]).reshape(-1, 3, 3), w @ table[:, 9:]
    act = torch.exp(scaling[i])
    samples = (scl_joint * act) * noise
    rots = rot_joint @ build_rotation_torch(rotation[i])
    return {"new_xyz": (rots @ samples[..., None]).squeeze(-1) + xyz[i], "new_features_dc": features_dc[i], "new_features_rest": features_rest[i],
            "new_opacities": opacity[i], "new_scaling": torch.log(act * scl_joint),
            "new_rotation": matrix_to_quaternion_torch(rot_joint) * rotation[i], "source": i}


def split_rows_torch(index, noise, xyz, features_dc, features_rest, opacity, scaling, rotation, N=2):
    """:551-566 in torch."""
    i = index.long().repeat(N)
    act = torch.exp(scaling[i])
    return {"new_xyz": (build_rotation_torch(rotation[i]) @ (act * noise)[..., None]).squeeze(-1) + xyz[i], "new_features_dc": features_dc[i],
            "new_features_rest": features_rest[i], "new_opacities": opacity[i], "new_scaling": torch.log(act / (0.8 * N)),
            "new_rotation": rotation[i], "source": i}


def merge_rows_torch(index, ids, mask, xyz, features_dc, features_rest, opacity, scaling, rotation):
    """:606-616 in torch; ``mask`` is updated in place like the fused form."""
    pair = ids[index.long()]
    out = {"new_xyz": xyz[pair].mean(1), "new_features_dc": features_dc[pair].mean(1), "new_features_rest": features_rest[pair].mean(1),
           "new_opacities": opacity[pair].mean(1), "new_scaling": torch.log(torch.exp(scaling[pair][:, 0]) / 0.8),
           "new_rotation": rotation[pair][:, 0], "source": pair[:, 0]}
    mask[pair[:, 1]] = True
    return out
