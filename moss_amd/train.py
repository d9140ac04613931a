"""MOSS's whole training iteration (``train_ZJU.py:100-131,171-174,189``) as ONE step of this repository's ops, capturable in a hipGraph.

:class:`MossStep` is a composition and a capture; it has no kernel and no mathematics of its own:

    render()            pose head + matrix-Fisher NLL, LBS-weight network, SMPL frame, LBS deformation, rasterizer with the raw
                        parameters and the pose inside the op (moss_amd/pose.py, lbs_weights.py, lbs.py, gaussian_renderer.py)
    loss                ``train_ZJU.py:131``: ROI photometric loss, LPIPS, NLL, S3IM (moss_amd/loss.py, lpips.py)
    three optimizers    (A) features / opacity / scaling / rotation inside the rasterizer's backward kernel, (B) the position,
                        (C) MOSS's two networks -- 52 + 16 tensors, two learning-rate segments, one launch (moss_amd/optim.py)
    statistics          what ``densify_and_prune_fused`` reads (moss_amd/densify.py)
    events              between steps: ``densify_and_prune`` / ``densification_event`` / ``oneup_sh_degree`` carry MOSS's densification
                        (``train_ZJU.py:176-186``) and its SH-degree raise (``:85-86``) out on both Gaussian optimizers at once
                        (``optim.FlatAdamWRows``, moss_amd/surgery.py) and capture the step again
    run_schedule        MOSS's loop order around the step (``train_ZJU.py:82-95,171-186``)

Nothing in the step reads the host (the events do: they sit between steps).  Everything here imports without a GPU.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

__all__ = ["MossStep", "run_schedule", "frame_order", "TERM_NAMES", "LOSS_WEIGHTS", "RENDER_FLAGS"]

# ``terms``, in this order.  ``ssim`` is the SSIM value itself (the loss takes 1 - ssim); ``total`` is train_ZJU.py:131
TERM_NAMES = ("l1", "ssim", "mask_l2", "lpips", "nll", "s3im", "total")
# train_ZJU.py:131: Ll1 + 0.5 * mask_loss + 0.2 * (1 - ssim_loss) + 0.5 * lpips_loss + 0.06 * nll_loss + 0.3 * s3im_loss
LOSS_WEIGHTS = {"mask_l2": 0.5, "ssim": 0.2, "lpips": 0.5, "nll": 0.06, "s3im": 0.3}
RENDER_FLAGS = ("lbs_in_op", "pose_head_in_op", "lbs_weights_in_op", "smpl_frame_in_op", "transforms_in_op", "pose_in_op",
                "raw_parameters_in_op")


def network_parameters(pc):
    """(the 52 tensors of ``pc.auto_regression``, the 16 of ``pc.cross_attention_lbs`` that its forward reads), in the order they
    cross the C ABI.  ``out_layer`` / ``gate_proj`` are not among them: their ``.grad`` is None in MOSS and ``torch.optim.AdamW`` never
    touches such a tensor, not even with its weight decay."""
    from .lbs_weights import net_parameters
    from .pose import head_parameters
    return list(head_parameters(pc.auto_regression)), list(net_parameters(pc.cross_attention_lbs))


class MossStep:
    """``step = MossStep(pc, view, gt_image, bkgd_mask, region, bg, lpips_net, lrs)``; ``step.compute()`` is one eager iteration,
    ``step.capture()`` captures it and ``step()`` replays it.

    ``pc``: a ``GaussianSet(unified_features=True)`` that carries what MOSS's ``GaussianModel`` gives the pose branch:
    ``auto_regression``, ``cross_attention_lbs``, ``SMPL_NEUTRAL``, ``knn``, ``coarse_deform_c2source`` and
    ``motion_offset_flag=True``.  ``view``: a camera with ``smpl_param`` (``pose_rotmats`` included), ``big_pose_smpl_param`` and
    ``big_pose_world_vertex``.  ``gt_image`` (3,H,W), ``bkgd_mask`` (1,H,W), ``region`` (a ``loss.ViewRegion``), ``bg`` (3,);
    ``lpips_net``: an ``lpips.LpipsVGG``; the net carries the precision of the term -- ``LpipsVGG(..., precision="bf16")`` runs the
    twelve wide convolutions with bf16 operands and float32 sums (the step at P = 45 695: 3.55 against 4.68 ms; the term moves by about
    1 % and its gradient by about 0.2 relative L2 on a person-like crop with synthetic weights, three times what float32 itself is from
    float64 there -- a training term, never the reported metric: ``lpips.py``, profiles/lpips_notes.md; ``precision="bf16x3"``, the
    split-bf16 form, sits between the two: 3.73 ms, the term within 1e-5 of float64's).  ALL of them are static inputs: the caller changes frame between steps by ``copy_`` into
    these tensors and ``region.copy_``.

    ``lpips_capacity``: ``(cap_h, cap_w)`` -- ``lpips.crop_capacity`` of the dataset's regions -- or ``"frame"``; it goes to
    ``lpips_vgg_roi_fused(capacity=)``, which then reads the crop's size from the device like the other loss terms, so the frames a
    capture is replayed on may have crops of any size up to the capacity (MOSS's do: the rectangle follows the pose).  Without it
    LPIPS has the size of the region at capture in its launches and every replayed frame must have exactly that crop size.  Under
    replay nothing on the host sees the region; :meth:`check` does, and raises on a region the capture cannot serve.

    ``lpips_reference``: a static ``lpips.LpipsReference`` -- ``LpipsReference.empty(lpips_net, lpips_capacity)``, or one of the crop's
    size without a capacity -- that ``compute()`` hands to ``lpips_vgg_roi_fused`` in ``gt_image``'s place: LPIPS then runs VGG16 on
    the render alone.  Build the per-camera references once (``refs, nbytes = lpips.reference_cache(lpips_net, gt_images, regions,
    lpips_capacity)``, 122 floats per pixel of the capacity each) and change frame by ``step.lpips_reference.copy_(refs[k])`` beside
    the input copies and ``region.copy_``.  The step's result is the same (bit for bit where the kernel shapes agree:
    ``lpips.LpipsReference``); :meth:`check` raises when the loaded reference's crop is not the region's.  None (the default): the
    step is what it was.

    ``template_index=True``: the nearest-vertex query of the LBS deformation (``knn(t_vertices, xyz)``: a cell grid built and walked on
    every step) goes through a ``knn_cuda.TemplateIndex`` built HERE, once, from ``view.big_pose_world_vertex`` -- one launch per step,
    the same ids bit for bit; it is set as ``pc.template_index`` and also serves :meth:`densify_and_prune`'s vertex distance.  The
    vertices are snapshotted: a step whose template changes needs a new step.  False (the default): the step is what it was.

    ``lbs_weights_precision``: ``"f32"`` (the default: the step is what it was) or ``"bf16x3"`` -- the LBS-weight network's five wide
    products, forward and in both gradients, on the bf16-input matrix cores with both operands split in two
    (``lbs_weights.cross_attention_lbs_fused(precision=)``, handed on as ``pipe.lbs_weights_precision``).  The gradient sinks, the
    capture and the events are the same.

    ``lrs``: ``{"auto_regression": lr, "cross_attention_lbs": lr}`` (MOSS: 2.5e-4 and 1e-4), optionally with rates for the Gaussian
    groups by their ``param_groups()`` names (``xyz``, ``features`` -- a number or ``(lr_dc, lr_rest)`` --, ``opacity``, ``scaling``,
    ``rotation``; default: the reference's).

    Three ``FlatAdamW(capturable=True, eps=1e-15, weight_decay=0.01)``:

    * ``opt_gaussians`` (A): ``_features``, ``_opacity``, ``_scaling``, ``_rotation``, taken inside the rasterizer's backward kernel
      (``fuse_into_backward``) -- the rasterizer is the only producer of their gradients;
    * ``opt_xyz`` (B): ``_xyz`` alone.  The rasterizer, the LBS deformation and the LBS-weight network all add to its gradient, so it
      is summed by autograd and ``collect()``-ed into the bucket;
    * ``opt_networks`` (C): the 52 + 16 network tensors, one learning-rate segment per network.  Both networks' backward kernels
      write their weight gradients straight into its bucket (``pipe.net_grad_sink``).

    (B) and (C) step with the frame's status word as ``skip_word`` and (A)'s kernel reads it itself: a frame that overflowed the
    binning capacity (it rendered nothing) is a no-op for all three -- parameters, moments and step counters stay bit for bit.

    ``stats`` (a ``densify.DensifyStats``): the step also keeps what ``densify_and_prune_fused`` reads -- ``stats.add(radii,
    viewspace.grad)``, ``joint_F_sum += Rs`` and ``lbs_weights_sum += lbs_weights`` (``train_ZJU.py:102-105,127,171-174``; a dropped
    frame adds to none of them).

    Between steps -- ``rows`` is ``optim.FlatAdamWRows([opt_gaussians, opt_xyz])``, the two Gaussian optimizers as one for row surgery:

    * :meth:`densify_and_prune`: ``train_ZJU.py:176-183`` in one call -- MOSS's decision on the step's own statistics, the rows moved
      in both optimizers by one gather launch per phase, the sums reset, the binning capacity re-learned, the step captured again;
    * :meth:`densification_event`: the same tail for a decision the caller made; ``reset_opacity`` alone is applied in place and the
      captured graph stays;
    * :meth:`oneup_sh_degree`: ``oneupSHdegree`` -- the model, optimizer (A) and the capture learn the new degree together, so the
      new coefficients cannot stay frozen behind a stale degree.

    A re-capture runs no training step; ``check()`` and ``dropped_frames`` carry on across events.  ORDER: MOSS densifies between
    ``backward()`` and ``optimizer.step()`` (``train_ZJU.py:176-189``), and the tensors it rebuilds there have lost their ``.grad``,
    so that iteration's update skips the Gaussians.  Here an event runs between two steps: the iteration's update HAS been taken
    when the decision reads the parameters (as INTEGRATION states for the step fused into the backward).

    ``terms`` (7 floats on the device, :data:`TERM_NAMES`): the six loss terms and the total of the last step."""

    def __init__(self, pc, view, gt_image, bkgd_mask, region, bg, lpips_net, lrs, context=None, stats=None, lpips_capacity=None,
                 lpips_reference=None, template_index=False, lbs_weights_precision="f32"):
        from .diff_gaussian_rasterization import RasterContext
        from .lbs_weights import PRECISIONS
        from .dist import GradBucket
        from .optim import FlatAdamW
        if not getattr(pc, "unified_features", False):
            raise ValueError("MossStep needs GaussianSet(unified_features=True): the update inside the backward kernel takes the SH "
                             "coefficients as one tensor")
        missing = [a for a in ("auto_regression", "cross_attention_lbs", "SMPL_NEUTRAL", "knn", "coarse_deform_c2source") if not hasattr(pc, a)]
        if missing or not getattr(pc, "motion_offset_flag", False):
            raise ValueError(f"MossStep: the model lacks {missing or 'motion_offset_flag=True'} (MOSS trains with --motion_offset_flag)")
        if "pose_rotmats" not in view.smpl_param:
            raise ValueError("MossStep: view.smpl_param has no 'pose_rotmats' (the target rotations of the matrix-Fisher term)")
        for k in ("auto_regression", "cross_attention_lbs"):
            if k not in lrs:
                raise ValueError(f"MossStep: lrs has no rate for '{k}'")
        if lbs_weights_precision not in PRECISIONS:
            raise ValueError(f"MossStep: lbs_weights_precision must be one of {PRECISIONS}, got {lbs_weights_precision!r}")
        self.pc, self.view, self.gt_image, self.bkgd_mask, self.region, self.bg, self.lpips_net = pc, view, gt_image, bkgd_mask, region, bg, lpips_net
        self.stats = stats
        if lpips_capacity is not None:
            from .lpips import resolve_capacity
            lpips_capacity = resolve_capacity("MossStep", lpips_capacity, *region.bound.shape)
        self.lpips_capacity = lpips_capacity
        if lpips_reference is not None:
            from .lpips import LpipsReference
            if not isinstance(lpips_reference, LpipsReference):
                raise TypeError(f"MossStep: lpips_reference must be an lpips.LpipsReference, got {type(lpips_reference).__name__}")
            if lpips_reference.capacity != lpips_capacity:
                raise ValueError(f"MossStep: lpips_reference is laid out for capacity {lpips_reference.capacity} and lpips_capacity is "
                                 f"{lpips_capacity} (LpipsReference.empty(lpips_net, lpips_capacity))")
        self.lpips_reference = lpips_reference
        self.template_index = None
        if template_index:
            from .knn_cuda import TemplateIndex
            # (does not depend on P: densification events and re-captures keep it)
            self.template_index = pc.template_index = TemplateIndex(view.big_pose_world_vertex)
        self._captured_crop = None                           # (h, w) of the region at capture: what LPIPS launched for without a capacity
        dev = pc._xyz.device
        self.context = cx = context if context is not None else RasterContext()
        if not cx.enabled:
            cx.set_async(True)                               # (the first forward is synchronous and sizes the binning capacity)
        kw = dict(capturable=True, eps=1e-15, weight_decay=0.01)
        groups = {}
        for g in pc.param_groups():
            g = dict(g)
            rate = lrs.get(g["name"])
            if isinstance(rate, (tuple, list)):
                g["lr"], g["lr_pattern"] = float(rate[0]), tuple(g["lr_pattern"][:2]) + (float(rate[1]),)
            elif rate is not None:
                g["lr"] = float(rate)
            groups[g["name"]] = g
        # (A) inside the rasterizer's backward
        names_a = ("features", "opacity", "scaling", "rotation")
        self.bucket_gaussians = GradBucket([p for n in names_a for p in groups[n]["params"]])
        self.opt_gaussians = FlatAdamW([groups[n] for n in names_a], self.bucket_gaussians, **kw)
        self.opt_gaussians.set_active_sh_degree(pc.active_sh_degree)
        self.opt_gaussians.fuse_into_backward(cx, sh=pc._features, opacity=pc._opacity, scales=pc._scaling, rotations=pc._rotation)
        # (B) the position
        self.bucket_xyz = GradBucket([pc._xyz])
        self.opt_xyz = FlatAdamW([groups["xyz"]], self.bucket_xyz, **kw)
        # (C) both networks: two groups, two segments, one launch
        head, net = network_parameters(pc)
        self.network_params = {"auto_regression": head, "cross_attention_lbs": net}
        self.bucket_networks = GradBucket(head + net)
        self.opt_networks = FlatAdamW([{"params": head, "lr": float(lrs["auto_regression"]), "name": "auto_regression"},
                                       {"params": net, "lr": float(lrs["cross_attention_lbs"]), "name": "cross_attention_lbs"}],
                                      self.bucket_networks, **kw)
        self.optimizers = (self.opt_gaussians, self.opt_xyz, self.opt_networks)
        from .optim import FlatAdamWRows
        self.rows = FlatAdamWRows([self.opt_gaussians, self.opt_xyz])     # (A) and (B) as one optimizer for row surgery
        self.pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raster_context=cx,
                                    net_grad_sink=self.bucket_networks.sink_for, lbs_weights_precision=lbs_weights_precision,
                                    **dict.fromkeys(RENDER_FLAGS, True))
        # [photometric loss | l1, ssim, mask_l2 | lpips, nll, s3im, total]: the photometric kernels write the first four themselves
        self._terms = torch.zeros(8, dtype=torch.float32, device=dev)
        self.terms = self._terms[1:]
        self.joint_F_sum = torch.zeros(23, 3, 3, dtype=torch.float32, device=dev)
        self.lbs_weights_sum = None                          # (made by the first step: the deformation says its shape)
        self.graphed = None
        self._dropped_carried = 0

    # ---- the step ------------------------------------------------------------------------------------------------------------------
    def compute(self):
        """One iteration, eagerly: render, the loss of ``train_ZJU.py:131``, backward, the three updates, the statistics.  Returns
        ``{"render", "terms"}`` (detached; under replay the static outputs of the capture)."""
        from .diff_gaussian_rasterization._C import frame_status_word
        from .gaussian_renderer import render
        from .loss import backward_from_loss, s3im_loss_roi_fused, training_loss_moss_fused
        from .lpips import lpips_vgg_roi_fused
        w = LOSS_WEIGHTS
        for b in (self.bucket_gaussians, self.bucket_xyz, self.bucket_networks):
            b.detach_grads()
        out = render(self.view, self.pc, self.pipe, self.bg)
        image, gt = out["render"], self.gt_image
        photometric = training_loss_moss_fused(image, out["render_alpha"], gt, self.bkgd_mask, self.region, w["ssim"], w["mask_l2"],
                                               terms_out=self._terms[:4])
        truth = gt if self.lpips_reference is None else self.lpips_reference         # (the ground truth's half, computed once)
        lpips = lpips_vgg_roi_fused(self.lpips_net, image, truth, self.region, capacity=self.lpips_capacity).reshape(())
        nll = out["pose_out"]["nll"].mean()
        s3im = s3im_loss_roi_fused(image, gt, self.region)
        loss = photometric + w["lpips"] * lpips + w["nll"] * nll + w["s3im"] * s3im
        backward_from_loss(loss)                             # (A) steps in here
        self.bucket_xyz.collect()
        self.bucket_networks.collect()                       # (costs nothing: every network gradient was written through its sink)
        img_buffer = self.context.last_img_buffer            # (None after the synchronous first forward of a context: it cannot overflow)
        word = None if img_buffer is None else frame_status_word(img_buffer)
        self.opt_xyz.step(skip_word=word)
        self.opt_networks.step(skip_word=word)
        with torch.no_grad():
            torch.stack((lpips.detach(), nll.detach(), s3im.detach(), loss.detach()), out=self._terms[4:])
            if self.stats is not None:
                radii, Rs, lbs_w = out["radii"], out["pose_out"]["Rs"].detach(), out["lbs_weights"].detach()
                if self.lbs_weights_sum is None:
                    self.lbs_weights_sum = torch.zeros_like(lbs_w)
                if word is None:
                    self.joint_F_sum.add_(Rs)
                    self.lbs_weights_sum.add_(lbs_w)
                else:
                    # a dropped frame contributes to no statistic either: its radii are set to zero (the preprocess computed them before
                    # the frame overflowed, so ``add`` would count the frame in ``denom``) and the two sums add zero times the frame
                    kept = 1 - ((word >> 1) & 1)                                 # int32 (1,): 0 for a dropped frame
                    radii = radii * kept
                    self.joint_F_sum.addcmul_(Rs, kept.to(torch.float32))
                    self.lbs_weights_sum.addcmul_(lbs_w, kept.to(torch.float32))
                self.stats.add(radii, out["viewspace_points"].grad)
        return {"render": image.detach(), "terms": self.terms}

    # ---- capture and replay -------------------------------------------------------------------------------------------------------
    def _state(self):
        s = [o.snapshot() for o in self.optimizers] + [self._terms.clone(), self.joint_F_sum.clone(),
                                                       None if self.lbs_weights_sum is None else self.lbs_weights_sum.clone()]
        if self.stats is not None:
            s += [self.stats.xyz_gradient_accum.clone(), self.stats.denom.clone(), self.stats.max_radii2D.clone()]
        return s

    def _restore(self, s):
        for o, snap in zip(self.optimizers, s[:3]):
            o.restore(snap)
        self._terms.copy_(s[3]); self.joint_F_sum.copy_(s[4])
        if self.lbs_weights_sum is not None:
            self.lbs_weights_sum.zero_() if s[5] is None else self.lbs_weights_sum.copy_(s[5])
        if self.stats is not None:
            self.stats.xyz_gradient_accum.copy_(s[6]); self.stats.denom.copy_(s[7]); self.stats.max_radii2D.copy_(s[8])

    def _crop_of_region(self):
        from .loss import region_xywh
        _, _, w, h = region_xywh(self.region, "MossStep")
        return int(h), int(w)

    def capture(self, warmup=3):
        """Capture ``compute`` in a hipGraph (``GraphedStep(self.compute, context=...)``).  The ``warmup`` eager runs a capture needs --
        the first of a fresh context is synchronous and sizes the binning capacity for the frame loaded NOW -- are training steps;
        they are undone here (parameters, moments, step counters, statistics: snapshot before, restore after), so a capture leaves the
        model where it found it.  Returns ``self``."""
        from .graphs import GraphedStep
        state = self._state()
        self._captured_crop = self._crop_of_region()
        self.graphed = GraphedStep(self.compute, warmup=warmup, device=self.pc._xyz.device, context=self.context)
        self._restore(state)
        return self

    # ---- between steps: densification and the SH degree -----------------------------------------------------------------------------
    def _probe(self):
        """Forward only, no side effect: the loaded frame rendered with the step's flags; after ``relearn_capacity()`` it is the
        synchronous forward that sizes the binning capacity for the new set."""
        from .gaussian_renderer import render
        with torch.no_grad():
            render(self.view, self.pc, self.pipe, self.bg)

    def _recapture(self):
        self._captured_crop = self._crop_of_region()
        self.graphed.recapture()                             # (no warm-up run: no training step is taken, the model stays where it is)

    def _reset_sums(self):
        """``joint_F = zeros``, ``lbs_weights = None`` (``train_ZJU.py:180-181``) -- the second as zeros at the CURRENT number of
        Gaussians: its address is baked into the capture, so it has to exist before the capture."""
        self.joint_F_sum.zero_()
        w, P = self.lbs_weights_sum, int(self.pc._xyz.shape[0])
        if w is not None:
            if int(w.shape[-2]) == P:
                w.zero_()
            else:
                self.lbs_weights_sum = torch.zeros(tuple(w.shape[:-2]) + (P, int(w.shape[-1])), dtype=w.dtype, device=w.device)

    def _event(self, t0, reads0, relayouts0, decision=None, **event):
        """The tail every event shares (``surgery.densification_event`` on ``rows``: capacity, probe, re-capture) and the report."""
        import time
        from . import densify
        from .surgery import densification_event
        moves = decision is not None or event.get("append") is not None or event.get("prune") is not None
        tail = densification_event(self.pc, self.rows, stats=self.stats, context=self.context, graphed=self.graphed, probe=self._probe,
                                   after_surgery=(lambda _: self._reset_sums()) if moves else None, **event)
        tail.pop("per_gaussian", None)
        if tail["recaptured"]:
            self._captured_crop = self._crop_of_region()
        report = dict(tail, **(decision or {}))
        report["relayouts"] = self.rows.relayouts - relayouts0
        report["host_reads"] = densify.host_reads() - reads0
        # (the decision and the row moves it made are the event's surgery; the clock started before them)
        report["event_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        report["surgery_ms"] = round(report["event_ms"] - tail["probe_ms"] - tail["capture_ms"], 3)
        return report

    def _begin_event(self):
        import time
        from . import densify
        if self.graphed is not None:
            self.check()                                     # (the frames dropped since the last check are counted before the capture goes)
        elif self.pc._xyz.is_cuda:
            torch.cuda.synchronize(self.pc._xyz.device)
        return time.perf_counter(), densify.host_reads(), self.rows.relayouts

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, kl_threshold=0.4, surface_mask=None, generator=None,
                          one_pass=True):
        """``gaussians.densify_and_prune(...)`` and the two resets behind it (``train_ZJU.py:176-183``).  The decision is
        ``densify.densify_and_prune_fused`` on ``rows`` with the step's own ``stats``, ``joint_F_sum``, ``lbs_weights_sum`` and
        ``view.big_pose_world_vertex`` (``surface_mask``, ``generator``, ``one_pass``: as there).  Then ``joint_F_sum`` is zeroed,
        ``lbs_weights_sum`` becomes zeros at the new size, the binning capacity is re-learned on the loaded frame and a captured step
        is captured again (``warmup=0``: no training step).  Returns the merged reports: ``cloned / split / merged / pruned``,
        ``rows_before / rows_after``, ``relayouts``, ``host_reads``, ``event_ms`` = ``surgery_ms`` (decision and row moves) +
        ``probe_ms`` + ``capture_ms``, ``recaptured``."""
        from .densify import densify_and_prune_fused
        if self.stats is None:
            raise RuntimeError("MossStep.densify_and_prune: the step was built without stats= (a densify.DensifyStats): there is nothing "
                               "to decide on")
        if self.lbs_weights_sum is None:
            raise RuntimeError("MossStep.densify_and_prune: no step has been taken yet (the statistics are empty)")
        t0, reads0, relayouts0 = self._begin_event()
        decision = densify_and_prune_fused(self.pc, self.rows, self.stats, self.joint_F_sum, self.lbs_weights_sum, max_grad, min_opacity,
                                           extent, max_screen_size, self.view.big_pose_world_vertex, kl_threshold=kl_threshold,
                                           surface_mask=surface_mask, generator=generator, one_pass=one_pass,
                                           template_index=self.template_index)
        moved = any(decision[k] for k in ("cloned", "split", "merged", "pruned"))
        return self._event(t0, reads0, relayouts0, decision=decision, rows_changed=moved)

    def densification_event(self, append=None, prune=None, reset_opacity=False, one_pass=True, keep_spatial_order=False):
        """The tail of :meth:`densify_and_prune` for a decision the caller made (``surgery.densification_event``: ``append``, a dict of
        the six ``densification_postfix`` tensors or a list of such; ``prune``, a mask over the set AFTER the appends, True = remove;
        ``reset_opacity`` last).  ``one_pass=True``: all of it is one gather launch over both optimizers.  With ``append`` or ``prune``
        the two sums are reset as after MOSS's own event.  ``reset_opacity`` alone changes no address: it is applied in place and a
        captured graph stays valid -- no re-capture.  Returns the report (``relayouts``, ``host_reads``, ``event_ms`` and its parts,
        ``recaptured``)."""
        t0, reads0, relayouts0 = self._begin_event()
        return self._event(t0, reads0, relayouts0, append=append, prune=prune, reset_opacity=reset_opacity, one_pass=one_pass,
                           keep_spatial_order=keep_spatial_order)

    def oneup_sh_degree(self) -> int:
        """``gaussians.oneupSHdegree()`` (``train_ZJU.py:85-86``): ``pc.active_sh_degree`` goes up by one (at most 3), optimizer (A)
        is told (``set_active_sh_degree``: the degree-aware update would otherwise never read the new coefficients' gradients), and a
        captured step is captured again -- the degree is a launch argument of the rasterizer and of the update.  Returns the degree."""
        pc = self.pc
        if pc.active_sh_degree >= pc.max_sh_degree:
            return int(pc.active_sh_degree)
        if self.graphed is not None:
            self.check()
        pc.active_sh_degree += 1
        self.rows.set_active_sh_degree(pc.active_sh_degree)
        if self.graphed is not None:
            self._recapture()
        return int(pc.active_sh_degree)

    def __call__(self):
        if self.graphed is None:
            raise RuntimeError("MossStep: capture() first (or call compute() for the eager step)")
        return self.graphed()

    def check(self) -> bool:
        """``GraphedStep.check()``: verifies the last replayed frame, counts the dropped ones (``dropped_frames``) and re-captures
        when the binning capacity has grown.  Synchronises; call it every few hundred steps.  True if it re-captured.  Raises if the
        region loaded now is one the captured LPIPS does not serve: a crop beyond ``lpips_capacity``, or, without a capacity, a crop
        of another size than the one captured (its LPIPS term was taken on a crop of the captured size); or, with
        ``lpips_reference``, a reference loaded now whose crop is not the region's (its rows were read at the region's size)."""
        if self.graphed is None:
            raise RuntimeError("MossStep.check(): nothing is captured")
        h, w = self._crop_of_region()
        if self.lpips_reference is not None and self.lpips_reference.crop != (h, w):
            raise RuntimeError(f"MossStep.check(): lpips_reference holds a crop of {self.lpips_reference.crop} and the region's is "
                               f"{h}x{w}: the LPIPS term of the last replay compared the render with another view's ground truth "
                               "(step.lpips_reference.copy_(refs[k]) goes with region.copy_)")
        if self.lpips_capacity is not None:
            if h > self.lpips_capacity[0] or w > self.lpips_capacity[1]:
                raise RuntimeError(f"MossStep.check(): the region's crop {h}x{w} exceeds lpips_capacity {self.lpips_capacity[0]}x"
                                   f"{self.lpips_capacity[1]}: the LPIPS term of the last replay was taken on a clamped crop")
        elif (h, w) != self._captured_crop:
            raise RuntimeError(f"MossStep.check(): the region's crop is {h}x{w} but LPIPS was captured at {self._captured_crop[0]}x"
                               f"{self._captured_crop[1]}, so the LPIPS term of the last replay was taken on the wrong crop; build the "
                               "step with lpips_capacity= (lpips.crop_capacity of the dataset's regions) to replay frames whose crops differ")
        return self.graphed.check()

    @property
    def dropped_frames(self) -> int:
        # (``_dropped_carried``: what a loaded state had counted before this process, ``load_state_dict``)
        return self._dropped_carried + (0 if self.graphed is None else self.graphed.dropped_frames)

    @property
    def recaptures(self) -> int:
        return 0 if self.graphed is None else self.graphed.recaptures

    def step_counts(self):
        """The three device-side step counters (A, B, C); synchronises."""
        return tuple(o.step_count() for o in self.optimizers)

    def set_learning_rates(self, rates):
        """A schedule, between replays, no re-capture (``FlatAdamW.set_learning_rates``).  ``rates``: ``{key: lr}`` with ``key`` a
        parameter, or ``"auto_regression"`` / ``"cross_attention_lbs"`` / a Gaussian group's name (``xyz``, ``features``: ``(lr_dc,
        lr_rest)``, ``opacity``, ``scaling``, ``rotation``).  Each entry goes to the optimizer that holds the parameter."""
        pc = self.pc
        named = {"xyz": pc._xyz, "features": pc._features, "opacity": pc._opacity, "scaling": pc._scaling, "rotation": pc._rotation,
                 "auto_regression": self.network_params["auto_regression"][0], "cross_attention_lbs": self.network_params["cross_attention_lbs"][0]}
        per = [{} for _ in self.optimizers]
        for key, val in rates.items():
            if isinstance(key, str) and key not in named:
                raise KeyError(f"MossStep.set_learning_rates: no parameter group '{key}'")
            p = named[key] if isinstance(key, str) else key
            for o, d in zip(self.optimizers, per):
                if id(p) in o.bucket._offset:
                    d[p] = val
                    break
            else:
                raise KeyError("MossStep.set_learning_rates: a parameter that none of the three optimizers holds")
        for o, d in zip(self.optimizers, per):
            if d:
                o.set_learning_rates(d)

    # ---- the training state: stop and continue (moss_amd/checkpoint.py) --------------------------------------------------------------
    STATE_VERSION = 1
    _OPTIMIZER_KEYS = ("gaussians", "xyz", "networks")

    def _layout(self):
        """What a state must agree on with the step that takes it: per optimizer (A), (B) the Gaussian groups' names and per-row
        shapes, per network the names and shapes of the tensors optimizer (C) holds."""
        pc = self.pc
        names = {id(pc._xyz): "xyz", id(pc._features): "features", id(pc._opacity): "opacity", id(pc._scaling): "scaling",
                 id(pc._rotation): "rotation"}
        gaussians = [[names[id(p)], [int(d) for d in p.shape[1:]]] for o in (self.opt_gaussians, self.opt_xyz) for p in o.bucket.params]
        networks = {}
        for key, held in self.network_params.items():
            named = {id(p): n for n, p in getattr(pc, key).named_parameters()}
            networks[key] = [[named[id(p)], [int(d) for d in p.shape]] for p in held]
        return gaussians, networks

    def state_dict(self):
        """All it takes to continue THIS run bit for bit in another process, as CPU tensors and plain Python values
        (``torch.load(weights_only=True)`` reads it; ``checkpoint.save_checkpoint`` writes it): a format ``version``; ``rows`` (P),
        ``max_sh_degree``, ``active_sh_degree`` and ``spatially_ordered`` (the hint changes the float32 summation order inside the
        op); the Gaussian groups' names and per-row shapes and the network tensors' names and shapes; ``FlatAdamW.state_dict()`` of
        the three optimizers (parameters, both moments, the step-state block with the counter and the rates, ``t``, the segments'
        rates, the SH degree in force); the three ``DensifyStats`` accumulators (None without ``stats``); ``joint_F_sum``;
        ``lbs_weights_sum`` (None before the first step); all of ``_terms``; ``dropped_frames``.  A captured step is ``check()``-ed
        first, so that the frames dropped since the last check are counted.  Synchronises.

        NOT kept: the binning capacity (re-learned by a probe on load); the captured graph (captured again on load); the caller's
        frame inputs -- ``view.smpl_param``, ``gt_image``, ``bkgd_mask``, ``region`` -- and ``lpips_reference`` (loaded per frame by
        the caller anyway); the densification noise generator, which the caller owns (``save_checkpoint(extra=)`` is the place for
        ``generator.get_state()``); the four ``out_layer`` / ``gate_proj`` tensors that no step changes (``save_scene`` writes them)."""
        if self.graphed is not None:
            self.check()
        pc = self.pc

        def host(t):
            return None if t is None else t.detach().to("cpu", copy=True)
        gaussians, networks = self._layout()
        st = self.stats
        return {"version": self.STATE_VERSION, "unified_features": True, "rows": int(pc._xyz.shape[0]),
                "max_sh_degree": int(pc.max_sh_degree), "active_sh_degree": int(pc.active_sh_degree),
                "spatially_ordered": bool(pc.spatially_ordered), "gaussians": gaussians, "networks": networks,
                "optimizers": {k: o.state_dict() for k, o in zip(self._OPTIMIZER_KEYS, self.optimizers)},
                "stats": None if st is None else {"xyz_gradient_accum": host(st.xyz_gradient_accum), "denom": host(st.denom),
                                                  "max_radii2D": host(st.max_radii2D)},
                "joint_F_sum": host(self.joint_F_sum), "lbs_weights_sum": host(self.lbs_weights_sum), "terms": host(self._terms),
                "dropped_frames": int(self.dropped_frames)}

    def _check_state(self, sd):
        who = "MossStep.load_state_dict"
        pc = self.pc
        if sd.get("version") != self.STATE_VERSION:
            raise ValueError(f"{who}: version: the state is of format version {sd.get('version')!r}, this code reads {self.STATE_VERSION}")
        if not sd.get("unified_features", False) or not getattr(pc, "unified_features", False):
            raise ValueError(f"{who}: unified_features: the state and the step's model must both keep the SH coefficients as one tensor")
        if int(sd["max_sh_degree"]) != int(pc.max_sh_degree):
            raise ValueError(f"{who}: max_sh_degree: the state has {sd['max_sh_degree']}, the step's model {pc.max_sh_degree}")
        gaussians, networks = self._layout()
        if [[n, list(s)] for n, s in sd["gaussians"]] != gaussians:
            raise ValueError(f"{who}: gaussians: the state's groups and per-row shapes are {sd['gaussians']}, the step's {gaussians}")
        for key, mine in networks.items():
            theirs = [[n, list(s)] for n, s in sd["networks"].get(key, [])]
            if theirs != mine:
                bad = next((a for a, b in zip(theirs, mine) if a != b), None) or f"{len(theirs)} tensors for {len(mine)}"
                raise ValueError(f"{who}: networks: {key}: tensor names or shapes differ ({bad})")
        if (sd["stats"] is None) != (self.stats is None):
            raise ValueError(f"{who}: stats: the state " + ("has no" if sd["stats"] is None else "has") + " densification statistics and "
                             "the step was built " + ("without" if self.stats is None else "with") + " stats=")
        P = int(sd["rows"])
        if P < 1:
            raise ValueError(f"{who}: rows: {P}")
        # (the Gaussian optimizers are checked at THEIR new layout by their own load, after the rows are re-laid: the groups and
        # per-row shapes agree, so it is the one a step of P rows has; the networks' layout does not depend on P)
        self.opt_networks.check_state_dict(sd["optimizers"]["networks"], who=f"{who}: optimizers: networks")
        for key in ("gaussians", "xyz"):
            shapes = sd["optimizers"][key]["shapes"]
            if any(int(s[0]) != P for s in shapes):
                raise ValueError(f"{who}: optimizers: {key}: shapes {shapes} in a state of {P} rows")
        if sd["stats"] is not None and [tuple(sd["stats"][k].shape) for k in ("xyz_gradient_accum", "denom", "max_radii2D")] != [(P, 1), (P, 1), (P,)]:
            raise ValueError(f"{who}: stats: the accumulators are not those of {P} rows")
        if tuple(sd["joint_F_sum"].shape) != tuple(self.joint_F_sum.shape) or tuple(sd["terms"].shape) != tuple(self._terms.shape):
            raise ValueError(f"{who}: joint_F_sum / terms: shapes {tuple(sd['joint_F_sum'].shape)}, {tuple(sd['terms'].shape)}")
        w = sd["lbs_weights_sum"]
        if w is not None and int(w.shape[-2]) != P:
            raise ValueError(f"{who}: lbs_weights_sum: shape {tuple(w.shape)} in a state of {P} rows")

    def load_state_dict(self, sd):
        """Take a :meth:`state_dict` -- of this run or of one with ANOTHER number of Gaussians (a run saved at 45 695 rows, loaded into
        a step built from the 6 890-vertex initialisation).  Refused with a ``ValueError`` that names the field, before anything is
        modified: another format version, another ``max_sh_degree``, other Gaussian group names or per-row shapes, network tensor
        names or shapes that differ, statistics on one side only, a non-unified model.

        The rows are re-laid ONCE through ``rows`` (``FlatAdamWRows.relayout_rows``: the Parameter objects stay, the bucket and the
        update inside the backward follow), then every buffer is overwritten.  The tail is a densification event's: statistics at the
        new size, ``lbs_weights_sum`` re-created there, the binning capacity re-learned by the forward-only probe on the frame loaded
        NOW, and a captured step captured again (always: the SH degree and the rates are launch arguments).  No training step is
        taken: the three step counters afterwards are the saved ones.  What a state does not keep: :meth:`state_dict`."""
        self._check_state(sd)
        self._overwrite(sd)
        dev = self.pc._xyz.device
        self.context.relearn_capacity()
        self._probe()
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        if self.graphed is not None:
            self._recapture()                                # (outside no_grad: the capture records a backward)
        # the count goes on from the saved one: frames the step dropped BEFORE the load belong to the state that was overwritten (the
        # re-capture has reset the context's sticky counter, so the next check() cannot count them either)
        self._dropped_carried = int(sd["dropped_frames"]) - (0 if self.graphed is None else self.graphed.dropped_frames)

    @torch.no_grad()
    def _overwrite(self, sd):
        """``load_state_dict``'s middle: the rows re-laid once, then every buffer and host-side value taken from the (checked) state."""
        from .checkpoint import resize_rows
        pc, dev = self.pc, self.pc._xyz.device
        P = int(sd["rows"])
        resize_rows(self.rows, int(pc._xyz.shape[0]), P)
        for key, o in zip(self._OPTIMIZER_KEYS, self.optimizers):
            o.load_state_dict(sd["optimizers"][key])
        pc.active_sh_degree, pc.spatially_ordered = int(sd["active_sh_degree"]), bool(sd["spatially_ordered"])
        if self.stats is not None:
            self.stats.reset(P)
            for k, v in sd["stats"].items():
                getattr(self.stats, k).copy_(v)
        self.joint_F_sum.copy_(sd["joint_F_sum"])
        self._terms.copy_(sd["terms"])
        w = sd["lbs_weights_sum"]
        if w is None:
            self._reset_sums()                               # (zeros at the new size if the step has taken one; else still None)
            self.joint_F_sum.copy_(sd["joint_F_sum"])
        elif self.lbs_weights_sum is not None and tuple(self.lbs_weights_sum.shape) == tuple(w.shape):
            self.lbs_weights_sum.copy_(w)
        else:
            self.lbs_weights_sum = w.to(dev)


# ---- MOSS's loop around the step ----------------------------------------------------------------------------------------------------
def frame_order(frames: int, iterations: int, seed: int = 0):
    """The frame of every iteration, drawn as ``train_ZJU.py:91-93`` draws its camera: without replacement from a stack that is
    refilled when it is empty.  ``frames``: how many there are; returns ``iterations`` indices."""
    import random
    rng, stack, order = random.Random(seed), [], []
    for _ in range(int(iterations)):
        if not stack:
            stack = list(range(int(frames)))
        order.append(stack.pop(rng.randint(0, len(stack) - 1)))
    return order


def run_schedule(step, frames, iterations, densify_from=400, densify_until=2000, interval=100, sh_every=1000, opacity_reset_interval=4000,
                 check_every=100, lr_schedule=None, on_event=None, load_frame=None, densify=None, seed=0, start_iteration=1,
                 saving_iterations=(), save=None):
    """MOSS's training loop (``train_ZJU.py:82-95,171-186``) around a :class:`MossStep`; no mathematics of its own.  Per iteration
    ``i = 1 .. iterations``, in MOSS's order:

    1. ``step.set_learning_rates(lr_schedule(i))`` if there is a schedule (``update_learning_rate``, ``:82``);
    2. ``step.oneup_sh_degree()`` when ``i % sh_every == 0`` (``:85-86``);
    3. ``load_frame(k)``: the caller's ``copy_`` of frame ``k`` into the step's static inputs and ``region.copy_``; ``k`` follows
       :func:`frame_order` over ``frames`` (a count, or a sequence whose elements are handed to ``load_frame``);
    4. the step: a replay if ``step`` is captured, else ``step.compute()`` -- the same schedule run eagerly;
    5. while ``i < densify_until``: the densification event when ``i > densify_from and i % interval == 0`` (``:176-183``) --
       ``on_event(step, i)``, which carries the event out and returns its report, or by default ``step.densify_and_prune(**densify,
       max_screen_size=20 if i > opacity_reset_interval else None)`` (``densify``: ``max_grad``, ``min_opacity``, ``extent`` and
       whatever else that call takes) -- and ``step.densification_event(reset_opacity=True)`` when ``i % opacity_reset_interval == 0``
       (``:184-185``).

    6. ``save(step, i)`` when ``i`` is one of ``saving_iterations`` -- after everything iteration ``i`` does, its event included
       (``save``: e.g. ``lambda step, i: (checkpoint.save_scene(model_path, i, step.pc), checkpoint.save_checkpoint(step, path, i))``).
       ORDER: MOSS calls ``scene.save`` between ``backward()`` and ``optimizer.step()`` (``train_ZJU.py:164-166,189``), so its file holds
       the parameters BEFORE that iteration's update; here the update has been taken (and the event carried out).

    ``start_iteration=k`` continues a run: iterations ``k .. iterations`` are run.  The frame order is still
    ``frame_order(len(frames), iterations, seed)`` over the WHOLE run, entered at ``k``; degree raises, events and saves happen only at
    iterations >= ``k``, and the phase bookkeeping starts in the phase ``k`` lies in (``load_checkpoint`` returns the iteration it was
    saved after: continue at that plus one).  With the defaults -- 1, no saving iterations -- the loop is what it was.

    A captured step is ``check()``-ed every ``check_every`` iterations.  The device is synchronised where a phase ends (and by every
    event), nowhere else.  Returns ``seconds``; ``phases`` (``before`` / ``during`` / ``after`` densification: ``iterations``,
    ``seconds``, ``it_per_s``; the events' time is in ``during``); ``events`` (each report with its ``iteration``); ``sh_raises``;
    ``opacity_resets``; ``dropped_frames``; ``recaptures``; ``rows``, the final number of Gaussians."""
    import time
    ids = list(range(frames)) if isinstance(frames, int) else list(frames)
    if load_frame is None and len(ids) > 1:
        raise ValueError("run_schedule: several frames need load_frame (the copies into the step's static inputs)")
    first = int(start_iteration)
    if first < 1:
        raise ValueError(f"run_schedule: start_iteration = {start_iteration} (iterations count from 1)")
    saving = {int(i) for i in saving_iterations}
    if saving and save is None:
        raise ValueError("run_schedule: saving_iterations without save= (a callable (step, iteration))")
    due = [i for i in range(first, int(iterations) + 1) if densify_from < i < densify_until and i % interval == 0]
    if due and on_event is None and densify is None:
        raise ValueError("run_schedule: densification events are due; give densify= (the arguments of step.densify_and_prune: max_grad, "
                         "min_opacity, extent) or on_event=")
    order = frame_order(len(ids), iterations, seed)
    captured = step.graphed is not None
    dev = step.pc._xyz.device
    phases = {name: {"iterations": 0, "seconds": 0.0} for name in ("before", "during", "after")}
    events, sh_raises, resets = [], 0, 0

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        return time.perf_counter()
    start = mark = sync()
    phase = "before" if first <= densify_from else "during" if first < densify_until else "after"
    for i in range(first, int(iterations) + 1):
        now = "before" if i <= densify_from else "during" if i < densify_until else "after"
        if now != phase:
            t = sync()
            phases[phase]["seconds"] += t - mark
            phase, mark = now, t
        if lr_schedule is not None:
            step.set_learning_rates(lr_schedule(i))
        if i % sh_every == 0:
            before = int(step.pc.active_sh_degree)
            sh_raises += int(step.oneup_sh_degree() != before)
        if load_frame is not None:
            load_frame(ids[order[i - 1]])
        step() if captured else step.compute()
        phases[phase]["iterations"] += 1
        if i < densify_until:
            if i > densify_from and i % interval == 0:
                if on_event is not None:
                    report = on_event(step, i)
                else:
                    report = step.densify_and_prune(**dict(densify, max_screen_size=20 if i > opacity_reset_interval else None))
                events.append(dict(report or {}, iteration=i))
            if i % opacity_reset_interval == 0:
                step.densification_event(reset_opacity=True)
                resets += 1
        if i in saving:
            save(step, i)
        if captured and i % check_every == 0:
            step.check()
    end = sync()
    phases[phase]["seconds"] += end - mark
    if captured:
        step.check()
    for p in phases.values():
        p["it_per_s"] = round(p["iterations"] / p["seconds"], 2) if p["iterations"] and p["seconds"] > 0 else None
        p["seconds"] = round(p["seconds"], 4)
    return {"seconds": round(end - start, 4), "iterations": int(iterations), "phases": phases, "events": events, "sh_raises": sh_raises,
            "opacity_resets": resets, "dropped_frames": step.dropped_frames, "recaptures": step.recaptures, "rows": int(step.pc._xyz.shape[0])}
