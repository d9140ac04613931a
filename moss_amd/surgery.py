"""One densification EVENT on the step that produces the headline number.

MOSS adds and removes Gaussians every 100 iterations between iterations 400 and 2000 and resets the opacities
(``train_ZJU.py:171-186``): ``densify_and_prune`` -> ``densification_postfix`` (``cat_tensors_to_optimizer``) / ``prune_points``
(``_prune_optimizer``), ``reset_opacity`` (``replace_tensor_to_optimizer``) -- ``scene/gaussian_model.py:314-317, 362-454``.  Which
Gaussians it clones, splits, merges or drops is decided by ``moss_amd.densify.densify_and_prune_fused`` (MOSS's rule, ``:495-666``, as
fused ops) or by the caller; THIS module carries out a decision on the objects of the fast step, in the order MOSS does, with one call
per event and outside graph capture -- or, with ``rows_changed=True``, finishes an event whose appends and prunes were already made:

    parameters + both AdamW moments   ``FlatAdamW.append_rows`` / ``prune_rows`` / ``reset_rows`` (new rows: zero moments; reset: zero moments)
    gradient bucket                   ``GradBucket.relayout`` (new offsets, the loss block moves with the tail)
    fused optimizer step              re-armed on the new moment addresses (``FlatAdamW.fuse_into_backward`` again, same names)
    densification statistics          ``DensifyStats.reset(P)`` after an append (densification_postfix :451-454), ``.prune`` after a prune
    binning capacity                  ``RasterContext.relearn_capacity()``: the next forward is synchronous and sizes it for the new set
    captured step                     ``GraphedStep.recapture(probe)``: parameter, moment, bucket and scratch addresses are baked into a graph

A ``reset_opacity`` alone changes no shape and no address: it is applied in place and the captured graph stays valid.
"""
from __future__ import annotations

import gc
import time

import torch

__all__ = ["densification_event", "rows_map", "rows_map_torch", "relayout_rows_torch"]


def reserve_workspace(nbytes, device):
    """Make torch's caching allocator hold ONE free segment of ``nbytes`` (allocate it, release it -- call after the first graph capture,
    which empties the cache).  A densification event builds new flat parameter / gradient / moment buffers and their gathered sources
    (seven tensors of 236 B per Gaussian) a little larger than the ones it frees, so none of them fits a cached block and every one
    is a hipMalloc (a few hundred microseconds each).  Blocks split off a large cached segment cost nothing and merge back when they
    are freed.  3 KB per Gaussian of the LARGEST set expected is ample; an MI355X has 288 GB."""
    t = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    del t


def rows_map(remove_mask, rows_app=0, rows_old=None, count=None):
    """The row map of "drop the rows where ``remove_mask`` is True, then keep ``rows_app`` appended rows" (C ABI
    ``moss_rows_keep_map``): the ascending indices of the surviving old rows followed by ``rows_old .. rows_old + rows_app - 1`` -- what
    ``FlatAdamW.relayout_rows`` takes.  ``remove_mask``: (rows_old,) bool / uint8 on the GPU, or None (every row stays; give
    ``rows_old``).  Returns ``(map int32 (count,), count)``.  The count is read from the device (one host read, counted by
    ``densify.host_reads()``) unless the caller knows it and passes ``count``.  CPU tensors: :func:`rows_map_torch`."""
    import ctypes as C
    from . import _lib, densify
    if remove_mask is None:
        if rows_old is None:
            raise ValueError("rows_map: rows_old is needed when there is no mask")
        return torch.arange(int(rows_old) + int(rows_app), dtype=torch.int32), int(rows_old) + int(rows_app)
    if not remove_mask.is_cuda:
        return rows_map_torch(remove_mask, rows_app)
    dev = remove_mask.device
    mask = remove_mask.reshape(-1)
    mask = (mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0).contiguous()
    rows_old, rows_app = int(mask.numel()), int(rows_app)
    out = torch.empty((max(rows_old + rows_app, 1),), dtype=torch.int32, device=dev)
    n_dev = torch.empty((1,), dtype=torch.int32, device=dev)
    nbytes = int(_lib.lib().moss_rows_map_workspace_bytes(rows_old))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    _lib.call("moss_rows_keep_map", dev, rows_old, mask.data_ptr(), rows_app, out.data_ptr(), n_dev.data_ptr(), ws.data_ptr(), C.c_size_t(nbytes))
    if count is None:
        count = int(n_dev.item())                            # THE host read of the map: its length
        densify._host_reads += 1
    return out[:int(count)], int(count)


def rows_map_torch(remove_mask, rows_app=0):
    """:func:`rows_map` restated in torch (``nonzero`` of the kept rows, then the appended rows' indices)."""
    mask = remove_mask.reshape(-1) != 0
    rows_old = int(mask.numel())
    kept = torch.nonzero(~mask).reshape(-1).to(torch.int32)
    m = torch.cat((kept, torch.arange(rows_old, rows_old + int(rows_app), dtype=torch.int32, device=mask.device)))
    return m, int(m.numel())


def relayout_rows_torch(optimizer, row_map, appended=None, rows_old=None):
    """``FlatAdamW.relayout_rows`` restated with plain torch indexing on the optimizer's own tensors (any device): ``cat`` the appended
    rows (zero moments), index parameters and moments with the map, rebuild the flat buffers by copy.  What the tests compare the
    one-pass kernel with."""
    index = {id(p): i for i, p in enumerate(optimizer.bucket.params)}
    dev = optimizer.flat_params.device
    ext = {(k if isinstance(k, int) else index[id(k)]): t.detach().to(device=dev, dtype=torch.float32) for k, t in (appended or {}).items()}
    if rows_old is None:
        rows_old = next(int(optimizer.bucket.params[i].shape[0]) for i in ext) if ext else next(int(p.shape[0]) for p in optimizer.bucket.params if p.dim() >= 1)
    with torch.no_grad():
        return optimizer._relayout_rows_torch(row_map.to(dev), ext, optimizer._row_params(int(rows_old)))


def _concat_appends(appends):
    """Several ``densification_postfix`` dicts as one (applied in order, the rows end up in the same places)."""
    keys = ("new_xyz", "new_features_dc", "new_features_rest", "new_opacities", "new_scaling", "new_rotation")
    if len(appends) == 1:
        return {k: appends[0][k] for k in keys}
    return {k: torch.cat([a[k] for a in appends], dim=0) for k in keys}


def densification_event(pc, optimizer, *, append=None, prune=None, reset_opacity=False, stats=None, context=None, graphed=None,
                        probe=None, per_gaussian=None, after_surgery=None, rows_changed=False, one_pass=False, keep_spatial_order=False):
    """Carry out one event.  ``append``: dict with the six tensors of ``densification_postfix`` (``new_xyz, new_features_dc,
    new_features_rest, new_opacities, new_scaling, new_rotation``) or a list of such dicts (MOSS appends twice per event: clones, then
    splits) -- applied first, in order; ``prune``: bool mask over the Gaussians AFTER the appends, True = remove (``prune_points``);
    ``reset_opacity``: last.  ``per_gaussian``: optional dict name -> (P, ...) tensor the CALLER keeps per Gaussian (an LBS transform
    table, cached neighbours): appended rows are taken from ``append[i]["source"]`` (index of the Gaussian each new row derives from)
    and pruned with the mask; the re-indexed dict is returned in the report and -- BEFORE the probe and the re-capture, whose step
    function reads those tables -- handed to ``after_surgery(per_gaussian)``.  ``rows_changed=True``: the rows of ``pc`` were appended and
    pruned BEFORE this call (``densify.densify_and_prune_fused``): the tail of an event -- capacity re-learning, probe, re-capture --
    runs although this call itself changes no row.  ``one_pass=True``: all appends, in order, and the prune are folded into ONE
    re-layout (``GaussianSet.relayout_points``: one gather kernel over the flat buffers instead of a torch pass per tensor and step)
    -- same bits; ``keep_spatial_order=True`` (needs ``one_pass``; used only when ``pc.spatially_ordered`` is set): the rows come out
    along the Morton curve of the NEW positions (``densify.spatial_order``), as if ``pc.reorder_spatially(optimizer)`` had followed,
    ``pc.spatially_ordered`` stays set, and statistics and ``per_gaussian`` tables follow the same order.

    Returns a report: rows before / after, what was re-captured, and the host-side cost of the event in milliseconds (it
    synchronises the device: the event is outside the step's asynchronous flow by nature).

    ``optimizer``: a ``FlatAdamW``, or an ``optim.FlatAdamWRows`` over several (``MossStep.rows``).  A shape change with ``context`` and
    ``graphed`` but no ``probe`` raises ``ValueError`` before anything is touched."""
    dev = pc._xyz.device
    if context is not None and graphed is not None and probe is None:
        # re-learning the capacity makes the next forward of the context the synchronous one, and without a probe that forward would
        # be the one inside the re-capture: refused before anything is touched
        will_move = bool(rows_changed) or (prune is not None and bool(prune.any())) or any(
            int(a["new_xyz"].shape[0]) > 0 for a in ([] if append is None else [append] if isinstance(append, dict) else append))
        if will_move:
            raise ValueError("densification_event: a shape change with `context` and `graphed` needs `probe` (a forward-only render of the "
                             "new set under torch.no_grad()): the binning capacity is re-learned by the next forward, which must not be "
                             "the one the re-capture records")
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    t0 = time.perf_counter()

    def counters():
        # the usual suspects when ONE event costs ten times the others: segments allocated from / returned to the driver (hipMalloc /
        # hipFree by torch's caching allocator), a full pass of Python's cyclic collector (45-55 ms in a process that has torch loaded).
        # (Zero in every event since round 6 -- the 40-95 ms outliers were the container's CPU quota: profiles/r06_notes.md section 10)
        st = torch.cuda.memory_stats(dev) if dev.type == "cuda" else {}
        return (int(st.get("segment.all.allocated", 0)), int(st.get("segment.all.freed", 0)), int(gc.get_stats()[2]["collections"]))
    c0 = counters()
    rows_before = int(pc._xyz.shape[0])
    per_gaussian = dict(per_gaussian or {})
    appends = [] if append is None else ([append] if isinstance(append, dict) else list(append))
    shape_changed = bool(rows_changed)
    if keep_spatial_order and not one_pass:
        raise ValueError("keep_spatial_order needs one_pass=True: the order is composed into the one-pass row map")
    kept_order = False
    if one_pass:
        appends = [a for a in appends if int(a["new_xyz"].shape[0]) > 0]
        rows_app = sum(int(a["new_xyz"].shape[0]) for a in appends)
        if prune is not None and int(prune.numel()) != rows_before + rows_app:
            raise ValueError(f"prune mask of {int(prune.numel())} entries for {rows_before + rows_app} Gaussians (it indexes the set AFTER the appends)")
        if per_gaussian and any("source" not in a for a in appends):
            raise ValueError("per_gaussian tensors need append['source']: the Gaussian each new row derives from")
        if rows_app or prune is not None:
            order = None
            if keep_spatial_order and getattr(pc, "spatially_ordered", False):
                from .densify import spatial_order
                order = spatial_order
            # (one host read inside, when there is a mask: the number of rows that stay; no row removed and none new: nothing is done)
            row_map = pc.relayout_points(optimizer, remove_mask=prune, new_rows=_concat_appends(appends) if appends else None, stats=stats,
                                         order=order)
            if rows_app or int(row_map.numel()) != rows_before:
                for k, t in list(per_gaussian.items()):
                    for a in appends:
                        t = torch.cat((t, t[a["source"].to(t.device)]), dim=0)
                    per_gaussian[k] = t[row_map.to(t.device).long()].contiguous()
                shape_changed, kept_order = True, order is not None
        appends, prune = [], None
    for a in appends:
        n_new = int(a["new_xyz"].shape[0])
        if n_new == 0:
            continue
        pc.densification_postfix(a["new_xyz"], a["new_features_dc"], a["new_features_rest"], a["new_opacities"], a["new_scaling"],
                                 a["new_rotation"], optimizer, stats=stats)
        for k, t in list(per_gaussian.items()):
            if "source" not in a:
                raise ValueError("per_gaussian tensors need append['source']: the Gaussian each new row derives from")
            per_gaussian[k] = torch.cat((t, t[a["source"].to(t.device)]), dim=0).contiguous()
        shape_changed = True
    if prune is not None and bool(prune.any()):
        if int(prune.numel()) != int(pc._xyz.shape[0]):
            raise ValueError(f"prune mask of {int(prune.numel())} entries for {int(pc._xyz.shape[0])} Gaussians (it indexes the set AFTER the appends)")
        pc.prune_points(prune, optimizer, stats=stats)
        keep = ~prune.bool()
        for k, t in list(per_gaussian.items()):
            per_gaussian[k] = t[keep.to(t.device)].contiguous()
        shape_changed = True
    if reset_opacity:
        pc.reset_opacity(optimizer)
    recaptured = False
    if after_surgery is not None:
        after_surgery(per_gaussian)

    def lap():
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        return time.perf_counter()
    t1 = t2 = t3 = lap()
    m1 = m2 = counters()[0]
    if shape_changed:
        if getattr(pc, "spatially_ordered", False) and not kept_order:
            pc.spatially_ordered = False                     # (appended rows sit at the end: index neighbours are no longer spatial neighbours)
        if context is not None:
            context.relearn_capacity()
        if probe is not None:
            probe()
        t2 = t3 = lap()
        m2 = counters()[0]
        if graphed is not None:
            graphed.recapture()
            recaptured = True
            t3 = lap()
    c1 = counters()
    return {"rows_before": rows_before, "rows_after": int(pc._xyz.shape[0]), "recaptured": recaptured,
            "event_ms": round(1e3 * (t3 - t0), 3), "surgery_ms": round(1e3 * (t1 - t0), 3), "probe_ms": round(1e3 * (t2 - t1), 3),
            "capture_ms": round(1e3 * (t3 - t2), 3), "device_mallocs": c1[0] - c0[0], "device_mallocs_by_phase": [m1 - c0[0], m2 - m1, c1[0] - m2], "device_frees": c1[1] - c0[1],
            "gc_full_collections": c1[2] - c0[2], "per_gaussian": per_gaussian}
