"""Flat fused AdamW over the gradient bucket (C ABI ``moss_adamw_flat_ex``, csrc/optim.hip) -- SURVEY.md section 8(f) n4.

Same update rule as ``torch.optim.AdamW`` (which MOSS uses per parameter group, scene/gaussian_model.py:215-226), applied by
ONE streaming kernel to all parameters: they are re-homed as views of one flat buffer, next to their flat gradients
(``moss_amd.dist.GradBucket``) and flat first/second moments."""
from __future__ import annotations

import ctypes as C

import torch

from ._lib import call, check, lib, ptr, stream


class _FusedAdamW:
    """What ``FlatAdamW.fuse_into_backward`` leaves on a RasterContext: the host struct of the C ABI (kept alive here), the data
    pointers of the parameters it describes (the backward refuses other inputs: the update is applied IN PLACE to what the op is given)."""

    def __init__(self, struct, param_ptrs, owner):
        self.struct, self.param_ptrs, self.owner = struct, dict(param_ptrs), owner
        self.address = C.addressof(struct)

    def check_inputs(self, **tensors):
        for name, ptr in self.param_ptrs.items():
            t = tensors.get(name)
            if t is None or t.data_ptr() != ptr or not t.is_contiguous() or t.dtype != torch.float32:
                raise RuntimeError(f"fused AdamW update: the rasterizer's `{name}` input is not the parameter tensor the optimizer was "
                                   f"given (a copy, a cast or an activated value?) -- use pipe.raw_parameters_in_op, or take the step "
                                   f"out of the backward again with optimizer.unfuse() (clears the context AND re-arms optimizer.step())")


class FlatAdamW:
    def __init__(self, param_groups, bucket, betas=(0.9, 0.999), eps=1e-15, weight_decay=0.01, capturable=False, shard=None):
        """capturable=True keeps the step counter on the device (``moss_adamw_flat_ex`` with a ``step_state``) so that a hipGraph capture of
        the training step replays with the right bias correction (the analogue of torch.optim.AdamW(capturable=True)).

        The kernel reads one learning rate per SEGMENT of the flat buffer, at most 8.  A segment is a run of consecutive bucket
        tensors of one entry of ``param_groups`` (a tensor with an ``lr_pattern`` is a segment of its own), so the number of TENSORS
        is not limited: MOSS's ``auto_regression`` (52 tensors) and ``cross_attention_lbs`` (16 that receive gradients) are two
        groups, two segments and one launch.  ``seg_of[i]`` is the segment of bucket parameter i.

        ``shard=(rank, world)``: this rank updates only its 1/world of the flat parameter buffer (the bucket's ``shard_layout``: the
        bucket must have been made with the same ``world``) and keeps moments for that shard alone (moments memory and update time
        / world); the caller reduce-scatters the gradient bucket into ``grad_shard`` before ``step()`` and all-gathers ``flat_params``
        after it -- ``moss_amd.dist.ShardedStep`` does both."""
        self.bucket = bucket
        self._lr_of, self._pat_of, self._group_of = {}, {}, {}
        for gidx, grp in enumerate(param_groups):
            for p in grp["params"]:
                self._lr_of[id(p)] = float(grp["lr"])
                # optional periodic pattern (period, split, lr_rest): first `split` of every `period` elements use lr, the rest lr_rest
                self._pat_of[id(p)] = grp.get("lr_pattern")
                self._group_of[id(p)] = gidx
        # ONE segment per run of consecutive bucket tensors of one parameter group (they share the group's rate; a tensor with an
        # lr_pattern is a segment of its own): MOSS's two network groups are 52 and 16 tensors and two segments
        if len(self._segment_runs(bucket.params)) > 8:
            raise ValueError("FlatAdamW supports at most 8 learning-rate segments (one per run of consecutive bucket tensors of one "
                             "parameter group; a tensor with an lr_pattern is a segment of its own)")
        self.shard = None if shard is None else (int(shard[0]), int(shard[1]))
        if self.shard is not None and self.shard[1] != bucket.world:
            raise ValueError(f"shard=(rank, {self.shard[1]}) but the bucket was laid out for {bucket.world} shards")
        self._adopt_layout([p.data for p in bucket.params], None, None)
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        self.t = 0
        self.fused = None                                    # set by fuse_into_backward
        # DEGREE-AWARE SH update (set_active_sh_degree): the SH tensor is the one whose learning rates follow MOSS's (48, 3) pattern --
        # features_dc / features_rest in one (P,16,3) parameter; 3 = every coefficient is active (nothing is skipped)
        self.sh_index = next((i for i, p in enumerate(bucket.params) if self._pat_of[id(p)] and tuple(self._pat_of[id(p)][:2]) == (48, 3)
                              and p.dim() == 3 and tuple(p.shape[1:]) == (16, 3)), None)
        self.sh_active_degree, self.sh_inactive_zero = 3, False
        # device-side step counter + completion counters, each on a cache line of its own: the LIBRARY says how large (csrc/optim.hip)
        dev = bucket.params[0].device
        self.step_state = torch.zeros(int(lib().moss_adamw_state_bytes()) // 4, dtype=torch.int32, device=dev) if capturable else None

    def _adopt_layout(self, values, exp_avg, exp_avg_sq):
        """(Re)build the flat buffers for the bucket's CURRENT layout: ``values[i]`` becomes parameter i (re-homed as a view of
        ``flat_params``), ``exp_avg[i]`` / ``exp_avg_sq[i]`` its moments (None: zeros -- a fresh optimizer).  The constructor and the
        row surgery (``prune_rows`` / ``append_rows``) end here; learning rates that ``set_learning_rates`` changed are kept.
        Allocate + copy; the bookkeeping is ``_adopt_segments`` (shared with ``relayout_rows``, whose kernel has filled the buffers)."""
        bucket = self.bucket
        params = bucket.params
        total = bucket.n_params                              # (every tensor starts 16-byte aligned: GradBucket.offsets)
        dev = params[0].device
        # (sharded: the parameter buffer mirrors the bucket's padded layout -- parameters, loss block, padding -- so that the
        # all-gather of the updated shards is in place)
        self.flat_params = torch.zeros(bucket.flat.numel() if self.shard is not None else total, dtype=torch.float32, device=dev)
        for i, (p, n, off) in enumerate(zip(params, bucket.sizes, bucket.offsets)):
            self.flat_params[off:off + n].copy_(values[i].reshape(-1))
            p.data = self.flat_params[off:off + n].view(values[i].shape)      # the parameter now lives in the flat buffer
        self._adopt_segments()
        self.exp_avg = torch.zeros(max(self.count, 1), dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(max(self.count, 1), dtype=torch.float32, device=dev)
        if exp_avg is not None:                              # (row surgery: unsharded by construction)
            for m, v, n, off in zip(exp_avg, exp_avg_sq, bucket.sizes, bucket.offsets):
                self.exp_avg[off:off + n].copy_(m.reshape(-1)); self.exp_avg_sq[off:off + n].copy_(v.reshape(-1))

    def _segment_runs(self, params):
        """Index of the first tensor of every learning-rate segment: consecutive bucket tensors form one segment when they belong to
        the same entry of ``param_groups`` and carry no ``lr_pattern`` (the pattern's period counts from the segment's start)."""
        firsts = []
        for i, p in enumerate(params):
            prev = params[i - 1] if i else None
            if (prev is None or self._group_of[id(p)] != self._group_of[id(prev)] or self._pat_of[id(p)] or self._pat_of[id(prev)]):
                firsts.append(i)
        return firsts

    def _adopt_segments(self):
        """The bookkeeping of a (re-)layout, from the bucket's CURRENT offsets: the learning-rate segments (rates a schedule changed
        survive), the parameter -> segment map ``seg_of`` (by index in the bucket), the element count, the shard range and its
        gradient buffer.  No parameter or moment is touched."""
        bucket = self.bucket
        params = bucket.params
        total = bucket.n_params
        dev = params[0].device
        old_lr = {i: (float(self.seg_lr[i]), float(self.seg_lr2[i])) for i in range(getattr(self, "nseg", 0))}
        ends, lrs, periods, splits, lr2s = [], [], [], [], []
        firsts = self._segment_runs(params)
        self.seg_of = [0] * len(params)
        for s, i in enumerate(firsts):
            p = params[i]
            nxt = firsts[s + 1] if s + 1 < len(firsts) else len(params)
            for k in range(i, nxt):
                self.seg_of[k] = s
            # a segment runs to the (aligned) start of the first tensor behind its run: the <= 3 floats of padding behind a tensor --
            # between the tensors of a run too -- are zeros with zero gradients, which the update leaves zero
            ends.append(bucket.offsets[nxt] if nxt < len(params) else total); lrs.append(self._lr_of[id(p)])
            pat = self._pat_of[id(p)]
            periods.append(int(pat[0]) if pat else 0); splits.append(int(pat[1]) if pat else 0); lr2s.append(float(pat[2]) if pat else 0.0)
        for i, (lr, lr2) in old_lr.items():                  # (a schedule's current rates survive a re-layout)
            lrs[i] = lr
            if periods[i]:
                lr2s[i] = lr2
        self.n = total
        self.seg_end = (C.c_longlong * len(ends))(*ends)
        self.seg_lr = (C.c_float * len(lrs))(*lrs)
        self.seg_period = (C.c_int * len(ends))(*periods)
        self.seg_split = (C.c_int * len(ends))(*splits)
        self.seg_lr2 = (C.c_float * len(ends))(*lr2s)
        self.nseg = len(ends)
        if self.shard is None:
            self.first, self.count = 0, total
        else:
            per = bucket.shard_len
            first = min(self.shard[0] * per, total)
            self.first, self.count = first, min(first + per, total) - first          # (the loss block and the padding are no parameters)
            # the reduce-scattered gradients of this rank's shard land here (equal-sized on every rank: the collective needs that)
            self.grad_shard = torch.zeros(per, dtype=torch.float32, device=dev)

    # ---- the update applied by the rasterizer's backward kernel itself -----------------------------------------------------------
    def fuse_into_backward(self, context, means3D=None, sh=None, opacity=None, scales=None, rotations=None, local_only=False):
        """Hand the update of the named parameters to the per-Gaussian backward kernel of the rasterizer (C ABI
        ``moss_raster_backward_ex`` with ``opt``): the kernel that produces a Gaussian's gradients applies its AdamW step on the spot --
        parameters in place, moments in this optimizer's buffers, same bits as ``step()`` would give -- and the gradients of those
        tensors never leave it (autograd sees ``None`` for them).  Valid when the rasterizer is the ONLY source of their gradients
        (MOSS: features, opacity, scaling, rotation -- every loss term of train_ZJU.py:111-131 goes through the image; the position only
        where it does not also feed the LBS network) and the op takes the RAW parameters (``pipe.raw_parameters_in_op``).

        ONE backward per forward: the parameters are updated IN PLACE by that backward (a second ``backward()`` over a retained
        graph would differentiate at the old parameters and step again), and nothing else may add to these tensors' gradients.

        Every parameter of the bucket must be named (give the rest to a second optimizer over its own bucket); needs
        ``capturable=True`` and no shard.  Afterwards ``step()`` is a no-op: the step is taken inside ``loss.backward()``, and a frame
        that overflowed its binning capacity takes none (the kernel reads the frame's status word itself).
        ``context``: the :class:`RasterContext` of the rasterizer whose backward does it (None: the default one).

        In a process group of more than one rank the fused step is LOCAL: the gradients never reach the bucket, so no exchange can
        average them and data-parallel replicas would drift apart without a word.  It is therefore refused there unless the caller
        says ``local_only=True`` -- every rank trains a model of its own (the loss-only exchange of BASELINE configs[3]).
        ``unfuse()`` takes the step out of the backward again."""
        import torch.distributed as tdist
        from ._lib import FusedAdamWStruct, OPT_BITS
        from .diff_gaussian_rasterization import _C
        if self.shard is not None or self.step_state is None:
            raise RuntimeError("fuse_into_backward needs capturable=True and an unsharded optimizer")
        if not local_only and tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
            raise RuntimeError("fuse_into_backward in a process group of %d ranks: the step inside the backward kernel is local to the rank "
                               "(its gradients never reach the bucket, so nothing averages them and replicas diverge).  Pass "
                               "local_only=True if every rank trains its OWN model (loss-only exchange); otherwise keep the flat "
                               "step() behind the gradient exchange" % tdist.get_world_size())
        named = {"means3D": means3D, "sh": sh, "opacity": opacity, "scales": scales, "rotations": rotations}
        given = {k: v for k, v in named.items() if v is not None}
        if {id(v) for v in given.values()} != {id(p) for p in self.bucket.params} or len(given) != len(self.bucket.params):
            raise ValueError("fuse_into_backward: name every parameter of the bucket exactly once (other parameters belong to a "
                             "second optimizer over their own bucket)")
        st = FusedAdamWStruct()
        for i in range(5):
            st.lr_segment[i] = -1
        offs = {id(p): (off, self.seg_of[i]) for i, (p, off) in enumerate(zip(self.bucket.params, self.bucket.offsets))}
        ptrs = {}
        for name, p in given.items():
            slot = OPT_BITS[name].bit_length() - 1
            off, seg = offs[id(p)]
            st.tensors |= OPT_BITS[name]
            st.exp_avg[slot] = self.exp_avg.data_ptr() + 4 * off
            st.exp_avg_sq[slot] = self.exp_avg_sq.data_ptr() + 4 * off
            st.lr[slot] = self.seg_lr[seg]
            st.lr_segment[slot] = seg
            if name == "sh":
                period, split = int(self.seg_period[seg]), int(self.seg_split[seg])
                if period == 0:
                    st.lr_sh_rest = self.seg_lr[seg]
                elif (period, split) == (48, 3):
                    st.lr_sh_rest = self.seg_lr2[seg]
                else:
                    raise ValueError("fuse_into_backward: the SH learning-rate pattern must be (48, 3, lr_rest) -- features_dc / features_rest")
            elif int(self.seg_period[seg]) != 0:
                raise ValueError(f"fuse_into_backward: a learning-rate pattern on {name} is not supported")
            ptrs[name] = p.data_ptr()
        st.beta1, st.beta2, st.eps, st.weight_decay = float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.weight_decay)
        st.step_state = self.step_state.data_ptr()
        st.sh_active_degree, st.sh_inactive_zero = int(self.sh_active_degree), int(self.sh_inactive_zero)
        self.fused = _FusedAdamW(st, ptrs, self)
        self._fused_context = context or _C.DEFAULT
        self._fused_context.fused_adamw = self.fused
        self._fused_args = (dict(given), bool(local_only))   # (row surgery re-fuses with the same names: the moments move)
        return self.fused

    def unfuse(self, context=None):
        """Take the step out of the backward kernel again: clears the context's ``fused_adamw`` AND this optimizer's own flag, so that
        the backward writes gradients to the bucket as before and ``step()`` applies them.  (Clearing only the context -- what round 4's
        error message suggested -- left ``step()`` a no-op: parameters silently stopped updating.)  ``context``: the one given to
        ``fuse_into_backward`` (default: that one).  A step captured in a hipGraph must be re-captured afterwards."""
        cx = context or getattr(self, "_fused_context", None)
        if cx is not None and cx.fused_adamw is self.fused:
            cx.fused_adamw = None
        self.fused = None
        self._fused_context = None
        self._fused_args = None

    # ---- degree-aware SH update --------------------------------------------------------------------------------------------------
    def set_active_sh_degree(self, degree: int):
        """Tell the optimizer the ACTIVE SH degree of its (P,16,3) SH parameter (MOSS: ``active_sh_degree`` starts at 0 and goes up every
        1000 iterations, train_ZJU.py:85-86, scene/gaussian_model.py:171-173 -- 2999 of 3000 iterations run below degree 3).  The
        optimizer keeps the HIGHEST degree it has been told since the coefficients above it were last seen to have zero moments: those
        coefficients have never received a gradient, so their AdamW step is the weight decay alone and their moments stay exactly zero --
        the update kernels (the flat one and the rasterizer backward that takes the step itself) then neither read nor write those
        moments, and when the parameters there are exactly zero as well (MOSS initialises ``features_rest`` with zeros,
        scene/gaussian_model.py:179-181: checked HERE, one device reduction and a host read per call) they are not touched at all.
        Results are bit-identical to the full update.  The degree is a launch argument: a captured step must be captured again
        (the rasterizer's own ``sh_degree`` is one too).  Returns the degree in force."""
        if self.sh_index is None:
            return 3
        degree = max(0, min(3, int(degree)))
        k_prev = (self.sh_active_degree + 1) ** 2
        m, v = self._moments_of(self.sh_index) if self.shard is None else (None, None)
        if self.shard is not None:
            degree = 3                                       # (a shard sees a slice of the tensor: everything stays active)
        elif degree < self.sh_active_degree:
            # lower than what is in force: only if the moments above it are (still) exactly zero -- a fresh optimizer, or one that
            # never trained above that degree
            k = (degree + 1) ** 2
            if bool(m[:, k:k_prev, :].any().item()) or bool(v[:, k:k_prev, :].any().item()):
                degree = self.sh_active_degree
        self.sh_active_degree = degree
        self._verify_sh_inactive()
        return self.sh_active_degree

    def _verify_sh_inactive(self):
        """Re-establish ``sh_inactive_zero`` (and that the moments above the active degree are zero: otherwise everything is active)."""
        if self.sh_index is None or self.sh_active_degree >= 3 or self.shard is not None:
            self.sh_active_degree = 3 if self.sh_index is None or self.shard is not None else self.sh_active_degree
            self.sh_inactive_zero = False
        else:
            k = (self.sh_active_degree + 1) ** 2
            p = self.bucket.params[self.sh_index]
            m, v = self._moments_of(self.sh_index)
            if bool(m[:, k:, :].any().item()) or bool(v[:, k:, :].any().item()):
                self.sh_active_degree, self.sh_inactive_zero = 3, False
            else:
                self.sh_inactive_zero = not bool(p.data[:, k:, :].any().item())
        if self.fused is not None:
            self.fused.struct.sh_active_degree = int(self.sh_active_degree)
            self.fused.struct.sh_inactive_zero = int(self.sh_inactive_zero)

    def _floor_sh_degree(self):
        """Raise the active SH degree to the highest one a rasterizer backward has run with on the SH parameter
        (``_C.sh_degree_run``): MOSS calls ``gaussians.oneupSHdegree()`` without the optimizer (train_ZJU.py:85-86), and a degree-aware
        step below the rasterizer's degree would never read the gradients of the newly active coefficients.  (The update inside the
        backward floors its degree with the call's own.)  Under graph capture the degree is a launch argument: a stale one is an error
        -- call ``set_active_sh_degree`` and capture again."""
        if self.sh_index is None or self.sh_active_degree >= 3:
            return
        from .diff_gaussian_rasterization._C import sh_degree_run
        ran = sh_degree_run(self.bucket.params[self.sh_index])
        if ran <= self.sh_active_degree:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"FlatAdamW.step() under graph capture: the rasterizer's backward ran at SH degree {ran}, but this optimizer "
                               f"was told degree {self.sh_active_degree} -- call set_active_sh_degree({ran}) (or oneupSHdegree(optimizer)) "
                               f"before capturing; the degree is a launch argument of the captured step")
        self.set_active_sh_degree(ran)

    def _seg_active(self):
        act = (C.c_int * self.nseg)(*([0] * self.nseg))
        if self.sh_index is not None and self.sh_active_degree < 3:
            act[self.seg_of[self.sh_index]] = 3 * (self.sh_active_degree + 1) ** 2     # (its lr_pattern makes the SH tensor a segment of its own)
        return act

    def set_learning_rates(self, rates):
        """A learning-rate schedule.  ``rates``: {parameter (or its index in the bucket): lr, or (lr, lr_rest) for a tensor with a
        periodic pattern}.  MOSS decays the position rate every iteration (``GaussianModel.update_learning_rate``,
        scene/gaussian_model.py:263-268, train_ZJU.py:82).

        With ``capturable=True`` the rates also go into the optimizer's device-side state block (one small asynchronous copy on the
        current stream) and every update kernel -- the flat ones and the rasterizer backward that takes the step itself -- reads them
        from there: call this BETWEEN replays of a captured step; no re-capture (the launch arguments baked into the graph are then
        ignored).

        The tensors of one parameter group that lie side by side in the bucket share ONE segment and one rate: naming any of them sets
        the rate of the whole run; two of them given different rates raise ``ValueError`` (nothing is changed then)."""
        index = {id(p): i for i, p in enumerate(self.bucket.params)}
        new = {}
        for key, val in rates.items():
            seg = self.seg_of[key if isinstance(key, int) else index[id(key)]]
            lr, lr2 = (val if isinstance(val, (tuple, list)) else (val, None))
            want = (float(lr), None if lr2 is None else float(lr2))
            if new.setdefault(seg, want) != want:
                raise ValueError(f"set_learning_rates: two parameters of one learning-rate segment (one parameter group) were given "
                                 f"different rates, {new[seg]} and {want}")
        for seg, (lr, lr2) in new.items():
            self.seg_lr[seg] = lr
            if lr2 is not None:
                self.seg_lr2[seg] = lr2
        self._fused_rates()
        if self.step_state is not None:
            # a small ring of pinned staging buffers: the copy is asynchronous and the device may be several steps behind the host, so a
            # buffer is rewritten only after the copy that last read it has completed (its event)
            if getattr(self, "_lr_ring", None) is None:
                self._lr_ring = [[torch.zeros(20, dtype=torch.float32).pin_memory(), None] for _ in range(8)]
                self._lr_next = 0
            slot = self._lr_ring[self._lr_next]
            self._lr_next = (self._lr_next + 1) % len(self._lr_ring)
            if slot[1] is not None:
                slot[1].synchronize()
            h = slot[0]
            hi = h.view(torch.int32)
            hi[0] = 1                                        # word 12: the table is valid; words 13-15 unused
            for s_ in range(8):
                h[4 + s_] = self.seg_lr[s_] if s_ < self.nseg else 0.0
                h[12 + s_] = (self.seg_lr2[s_] if int(self.seg_period[s_]) else self.seg_lr[s_]) if s_ < self.nseg else 0.0
            self.step_state.view(torch.float32)[12:32].copy_(h, non_blocking=True)
            slot[1] = torch.cuda.Event()
            slot[1].record(torch.cuda.current_stream(self.step_state.device))

    def _fused_rates(self):
        """The segments' rates in force, into the host struct of a step fused into the rasterizer's backward."""
        if self.fused is None:
            return
        st = self.fused.struct
        for slot in range(5):
            seg = st.lr_segment[slot]
            if seg >= 0:
                st.lr[slot] = self.seg_lr[seg]
                if slot == 1:
                    st.lr_sh_rest = self.seg_lr2[seg] if int(self.seg_period[seg]) else self.seg_lr[seg]

    def step_count(self) -> int:
        """Steps taken so far (reads the device-side counter when there is one: it synchronises)."""
        return int(self.step_state[0].item()) if self.step_state is not None else self.t

    def snapshot(self):
        """Copies of everything a step changes (parameters, both moments, step counters)."""
        return (self.flat_params.clone(), self.exp_avg.clone(), self.exp_avg_sq.clone(), self.t,
                None if self.step_state is None else self.step_state.clone())

    def restore(self, snap):
        self.flat_params.copy_(snap[0]); self.exp_avg.copy_(snap[1]); self.exp_avg_sq.copy_(snap[2]); self.t = snap[3]
        if self.step_state is not None:
            self.step_state.copy_(snap[4])

    # ---- the state as CPU tensors and plain values (moss_amd/checkpoint.py) ---------------------------------------------------------
    def state_dict(self):
        """Everything a later ``load_state_dict`` needs to go on bit for bit, as CPU tensors and plain Python values
        (``torch.load(weights_only=True)`` reads it): ``flat_params``, ``exp_avg``, ``exp_avg_sq``; the whole ``step_state`` block (the
        device-side step counter and the ``MOSS_ADAMW_LR_*`` words; None without ``capturable``); ``t``; ``seg_lr`` / ``seg_lr2``,
        the rates in force (a schedule's included); ``sh_active_degree`` / ``sh_inactive_zero``; and ``shapes``, the bucket's
        parameter shapes, which the load checks.  A sharded optimizer holds a part of the moments only: ``NotImplementedError``."""
        if self.shard is not None:
            raise NotImplementedError("FlatAdamW.state_dict on a sharded optimizer: every rank holds the moments of its shard alone")

        def host(t):
            return t.detach().to("cpu", copy=True)
        return {"flat_params": host(self.flat_params), "exp_avg": host(self.exp_avg), "exp_avg_sq": host(self.exp_avg_sq),
                "step_state": None if self.step_state is None else host(self.step_state), "t": int(self.t),
                "seg_lr": [float(x) for x in self.seg_lr], "seg_lr2": [float(x) for x in self.seg_lr2],
                "sh_active_degree": int(self.sh_active_degree), "sh_inactive_zero": bool(self.sh_inactive_zero),
                "shapes": [[int(d) for d in p.shape] for p in self.bucket.params]}

    def check_state_dict(self, sd, who="FlatAdamW.load_state_dict"):
        """Raise ``ValueError`` naming the field of ``sd`` that does not fit this optimizer's CURRENT layout; changes nothing."""
        if self.shard is not None:
            raise NotImplementedError(f"{who} on a sharded optimizer")
        shapes = [[int(d) for d in p.shape] for p in self.bucket.params]
        if [list(s) for s in sd["shapes"]] != shapes:
            diff = next((i for i, (a, b) in enumerate(zip(sd["shapes"], shapes)) if list(a) != b), min(len(shapes), len(sd["shapes"])))
            raise ValueError(f"{who}: shapes: the state holds {len(sd['shapes'])} tensors and the bucket {len(shapes)}; the first that "
                             f"differs is number {diff}")
        for k, mine in (("flat_params", self.flat_params), ("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
            if tuple(sd[k].shape) != tuple(mine.shape) or sd[k].dtype != torch.float32:
                raise ValueError(f"{who}: {k}: {tuple(sd[k].shape)} {sd[k].dtype} for a buffer of {tuple(mine.shape)} float32")
        if len(sd["seg_lr"]) != self.nseg or len(sd["seg_lr2"]) != self.nseg:
            raise ValueError(f"{who}: seg_lr: {len(sd['seg_lr'])} learning-rate segments for an optimizer of {self.nseg}")
        if (sd["step_state"] is None) != (self.step_state is None):
            raise ValueError(f"{who}: step_state: one of the two optimizers is capturable and the other is not")
        if self.step_state is not None and tuple(sd["step_state"].shape) != tuple(self.step_state.shape):
            raise ValueError(f"{who}: step_state: a block of {tuple(sd['step_state'].shape)} words for one of {tuple(self.step_state.shape)}")

    @torch.no_grad()
    def load_state_dict(self, sd):
        """Take a :meth:`state_dict` of an optimizer with the same layout (checked first: ``ValueError``, nothing changed): buffers and
        the state block by ``copy_`` -- no address changes, so a fused step stays armed; it is told the rates and the SH degree --, the
        host-side counter, rates and degree by value.  A step captured in a hipGraph bakes the rates and the degree into its launches:
        capture it again."""
        self.check_state_dict(sd)
        self.flat_params.copy_(sd["flat_params"]); self.exp_avg.copy_(sd["exp_avg"]); self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        if self.step_state is not None:
            self.step_state.copy_(sd["step_state"])
        self.t = int(sd["t"])
        for s in range(self.nseg):
            self.seg_lr[s], self.seg_lr2[s] = float(sd["seg_lr"][s]), float(sd["seg_lr2"][s])
        self._fused_rates()
        self.sh_active_degree, self.sh_inactive_zero = int(sd["sh_active_degree"]), bool(sd["sh_inactive_zero"])
        if self.fused is not None:
            self.fused.struct.sh_active_degree = int(self.sh_active_degree)
            self.fused.struct.sh_inactive_zero = int(self.sh_inactive_zero)

    def permute_rows(self, perm: torch.Tensor):
        """Re-index the Gaussians: row i of every parameter whose leading dimension is len(perm) -- and of its two moments -- becomes
        the old row perm[i] (e.g. ``moss_amd.densify.spatial_order(xyz)``).  The step count is shared and stays.  Not capturable:
        call it between graph captures, where MOSS rebuilds its tensors anyway (densify / prune)."""
        if self.shard is not None:
            raise RuntimeError("permute_rows on a sharded FlatAdamW: the moments of a parameter row live on several ranks; gather, "
                               "permute and rebuild the optimizer instead")
        n_rows = int(perm.numel())
        perm = perm.to(self.flat_params.device)
        with torch.no_grad():
            for p, n, off in zip(self.bucket.params, self.bucket.sizes, self.bucket.offsets):
                if p.dim() >= 1 and p.shape[0] == n_rows:
                    for flat in (self.flat_params, self.exp_avg, self.exp_avg_sq):
                        v = flat[off:off + n].view_as(p)
                        v.copy_(v[perm].clone())

    # ---- row surgery: MOSS's densification rebuilds its tensors AND its optimizer state (scene/gaussian_model.py:362-454) ----------
    def _row_params(self, n_rows):
        return [p.dim() >= 1 and p.shape[0] == n_rows for p in self.bucket.params]

    def _relayout(self, values, exp_avg, exp_avg_sq):
        """New parameter values / moments (one tensor per bucket parameter, the Parameter OBJECTS stay) -> new bucket layout, new flat
        buffers, the fused step re-armed on the new moment addresses.  Everything that holds device addresses of the old buffers -- a
        captured hipGraph above all -- is stale afterwards: ``GraphedStep.recapture()``."""
        if self.shard is not None:
            raise RuntimeError(_SHARDED_ROWS)
        fused = getattr(self, "_fused_args", None) if self.fused is not None else None
        cx = getattr(self, "_fused_context", None)
        for p, v in zip(self.bucket.params, values):
            p.data = v                                       # (the new shapes: what the bucket lays itself out from)
        self.bucket.relayout()
        self._adopt_layout(values, exp_avg, exp_avg_sq)
        if self.sh_active_degree < 3:
            self._verify_sh_inactive()                       # (appended rows may carry non-zero coefficients above the active degree)
        if fused is not None:
            self.fuse_into_backward(cx, local_only=fused[1], **fused[0])

    def _moments_of(self, i):
        off, n = self.bucket.offsets[i], self.bucket.sizes[i]
        shape = self.bucket.params[i].shape
        return self.exp_avg[off:off + n].view(shape), self.exp_avg_sq[off:off + n].view(shape)

    @torch.no_grad()
    def prune_rows(self, keep_mask: torch.Tensor):
        """``_prune_optimizer(mask)`` (scene/gaussian_model.py:377-394): every parameter whose leading dimension is len(keep_mask)
        keeps the rows where the mask is True, and so do its two moments; the shared step count stays (torch keeps ``state['step']``
        too).  The Parameter objects are the same afterwards (``.data`` re-homed in the new flat buffer, ``.grad`` dropped)."""
        keep = keep_mask.to(self.flat_params.device).bool()
        rows = self._row_params(int(keep.numel()))
        vals, ms, vs = [], [], []
        for i, (p, is_row) in enumerate(zip(self.bucket.params, rows)):
            m, v = self._moments_of(i)
            vals.append((p.data[keep] if is_row else p.data).clone()); ms.append((m[keep] if is_row else m).clone()); vs.append((v[keep] if is_row else v).clone())
        self._relayout(vals, ms, vs)

    @torch.no_grad()
    def append_rows(self, new_rows):
        """``cat_tensors_to_optimizer(tensors_dict)`` (scene/gaussian_model.py:413-434): ``new_rows`` maps a parameter (the object, or
        its index in the bucket) to the rows appended to it; their moments start at ZERO (``torch.zeros_like(extension_tensor)``,
        :422-423), the existing rows keep theirs, the shared step count stays.  Parameters not named keep their shape."""
        index = {id(p): i for i, p in enumerate(self.bucket.params)}
        ext = {}
        for key, t in new_rows.items():
            ext[key if isinstance(key, int) else index[id(key)]] = t
        vals, ms, vs = [], [], []
        for i, p in enumerate(self.bucket.params):
            m, v = self._moments_of(i)
            if i in ext:
                e = ext[i].detach().to(device=p.device, dtype=torch.float32)
                if tuple(e.shape[1:]) != tuple(p.shape[1:]):
                    raise ValueError(f"append_rows: rows of shape {tuple(e.shape)} do not extend a parameter of shape {tuple(p.shape)}")
                vals.append(torch.cat((p.data, e), dim=0)); ms.append(torch.cat((m, torch.zeros_like(e)), dim=0)); vs.append(torch.cat((v, torch.zeros_like(e)), dim=0))
            else:
                vals.append(p.data.clone()); ms.append(m.clone()); vs.append(v.clone())
        self._relayout(vals, ms, vs)

    @torch.no_grad()
    def relayout_rows(self, row_map: torch.Tensor, appended=None, check=True, rows_old=None, extra=None):
        """``append_rows(appended)`` followed by a gather of the rows ``row_map`` on every row-parameter and both its moments
        (``_prune_optimizer`` :377-394 after ``cat_tensors_to_optimizer`` :413-434) -- in ONE pass over memory: the new offsets are
        computed from the new shapes first, the three new flat buffers are allocated once (uninitialised), and one launch (C ABI
        ``moss_rows_relayout``) gathers from the old flat buffers straight into them, zero moments for appended rows and zeros in the
        alignment gaps included.  Same bits as the two calls; parameters that are not per-row keep values and moments, the shared
        step count stays, the Parameter objects stay, the fused step is re-armed.

        ``row_map``: integer tensor, one entry per row of the result: ``s < rows_old`` takes old row ``s``, ``s >= rows_old`` takes row
        ``s - rows_old`` of ``appended`` (``surgery.rows_map`` builds the map of a prune mask).  ``appended``: as ``append_rows``; every
        row-parameter must be named, with the same number of rows.  ``rows_old``: the row count that marks a row-parameter (default:
        that of the parameters named in ``appended``, else of the bucket's first parameter).  ``check=True`` validates the map's range
        with one host read (an entry out of range would otherwise give a row of zeros).  ``extra``: float32 tensors of ``rows_old``
        rows WITHOUT optimizer state (the densification statistics) gathered by the same launch -- only when nothing is appended;
        their gathered copies are returned as a list (else None).  CPU tensors take the torch restatement."""
        index = {id(p): i for i, p in enumerate(self.bucket.params)}
        ext = {(key if isinstance(key, int) else index[id(key)]): t for key, t in (appended or {}).items()}
        return _relayout_rows_of([self], row_map, [ext], check, rows_old, extra)

    def _rows_describe(self, args, k, is_row, ext, rows_new):
        """The first third of a GPU re-layout: the new layout from the new shapes (before anything is written), the three new flat
        buffers (uninitialised), and this optimizer's descriptors -- absolute addresses -- in ``args.tensors[k:]``.  Returns (the next
        free descriptor, the plan ``_rows_adopt`` takes).  Nothing of the optimizer has changed yet."""
        from .dist import flat_offsets
        bucket = self.bucket
        params = bucket.params
        dev = self.flat_params.device
        shapes = [((rows_new,) + tuple(p.shape[1:])) if r else tuple(p.shape) for p, r in zip(params, is_row)]
        sizes = [int(torch.Size(s).numel()) for s in shapes]
        offsets, total = flat_offsets(sizes)
        old = (self.flat_params, self.exp_avg, self.exp_avg_sq)
        new = tuple(torch.empty(max(total, 1), dtype=torch.float32, device=dev) for _ in range(3))
        if total == 0:
            for t in new:
                t.zero_()
        for i, (p, r, n, off) in enumerate(zip(params, is_row, sizes, offsets)):
            pad = (offsets[i + 1] if i + 1 < len(params) else total) - (off + n)
            if n + pad == 0:
                continue                                     # (no row left and no gap behind: nothing to write)
            d = args.tensors[k]
            k += 1
            off_old = bucket.offsets[i]
            d.src, d.src_m, d.src_v = (t.data_ptr() + 4 * off_old for t in old)
            d.dst, d.dst_m, d.dst_v = (t.data_ptr() + 4 * off for t in new)
            d.app = ext[i].data_ptr() if i in ext else None
            d.use_map, d.pad_after = int(r), pad
            d.width = max(int(torch.Size(p.shape[1:]).numel()), 1) if r else n
        return k, (new, shapes, sizes, offsets, total)

    def _rows_adopt(self, plan):
        """The last third: adopt the buffers the kernel has filled (no second copy) -- parameters re-homed, the bucket re-laid out,
        the segments re-adopted, the fused step re-armed on the new moment addresses."""
        new, shapes, sizes, offsets, total = plan
        bucket = self.bucket
        fused = getattr(self, "_fused_args", None) if self.fused is not None else None
        cx = getattr(self, "_fused_context", None)
        self.flat_params, self.exp_avg, self.exp_avg_sq = new
        for p, n, off, shape in zip(bucket.params, sizes, offsets, shapes):
            p.data = self.flat_params[off:off + n].view(shape)
        bucket.relayout()
        if list(bucket.offsets) != list(offsets) or bucket.n_params != total:
            raise RuntimeError("relayout_rows: the bucket laid itself out differently from the offsets the rows were written at")
        self._adopt_segments()
        if self.sh_active_degree < 3:
            self._verify_sh_inactive()                       # (appended rows may carry non-zero coefficients above the active degree)
        if fused is not None:
            self.fuse_into_backward(cx, local_only=fused[1], **fused[0])

    def _relayout_rows_torch(self, row_map, ext, is_row, extra=()):
        """``relayout_rows`` restated with torch indexing (what it does on CPU tensors, and what the tests compare the kernel with):
        ``cat`` the appended rows with zero moments, index with the map, then the two-copy ``_relayout``."""
        idx = row_map.long()
        vals, ms, vs = [], [], []
        for i, (p, r) in enumerate(zip(self.bucket.params, is_row)):
            m, v = self._moments_of(i)
            if r:
                e = ext.get(i)
                x = p.data if e is None else torch.cat((p.data, e), dim=0)
                if e is not None:
                    m, v = torch.cat((m, torch.zeros_like(e)), dim=0), torch.cat((v, torch.zeros_like(e)), dim=0)
                vals.append(x[idx].clone()); ms.append(m[idx].clone()); vs.append(v[idx].clone())
            else:
                vals.append(p.data.clone()); ms.append(m.clone()); vs.append(v.clone())
        gathered = [t[idx.to(t.device)].contiguous() for t in extra]
        self._relayout(vals, ms, vs)
        return gathered if extra else None

    @torch.no_grad()
    def reset_rows(self, param, values: torch.Tensor):
        """``replace_tensor_to_optimizer(tensor, name)`` (scene/gaussian_model.py:362-375; ``reset_opacity`` :314-317): the parameter
        takes ``values`` and BOTH its moments are zeroed.  Same shape, same addresses: in place, nothing is re-laid-out and a captured
        hipGraph stays valid (the copies run on the current stream, in order with the replays)."""
        i = param if isinstance(param, int) else {id(p): k for k, p in enumerate(self.bucket.params)}[id(param)]
        p = self.bucket.params[i]
        if tuple(values.shape) != tuple(p.shape):
            raise ValueError(f"reset_rows: values of shape {tuple(values.shape)} for a parameter of shape {tuple(p.shape)}")
        if self.shard is not None:
            raise RuntimeError("reset_rows on a sharded FlatAdamW: the parameter's moments live on several ranks")
        p.data.copy_(values.detach())
        m, v = self._moments_of(i)
        m.zero_(); v.zero_()

    def step(self, skip_word=None, skip_mask=2, extra_grads=None, grad_scale=1.0):
        """One update.  ``skip_word`` (capturable optimizers only): a one-element int32 / float32 DEVICE tensor; if
        ``skip_word & skip_mask`` is non-zero when the kernel runs, the step is a no-op on the device -- parameters, moments and the
        step counter stay bit for bit (C ABI ``moss_adamw_flat_ex`` with a ``skip_word``).  Not with ``shard``: the skip is a per-rank decision.  ``frame_status_word(img_buffer)`` of a rasterizer forward
        with the default mask 2 skips the step of a frame that overflowed its capacity and rendered nothing (inside a captured
        hipGraph nobody else can).  ``extra_grads`` (up to three flat tensors laid out like the bucket) + ``grad_scale``: the step's
        gradient is ((bucket + extra[0]) + extra[1] ...) x grad_scale, formed inside the update kernel in that order -- B views per
        optimizer step on one device (``moss_amd.multiview``)."""
        dev = self.flat_params.device
        if getattr(self, "fused", None) is not None:
            cx = getattr(self, "_fused_context", None)
            if cx is not None and cx.fused_adamw is self.fused:
                return                                       # the rasterizer's backward kernel took the step (fuse_into_backward)
            # somebody cleared the context by hand: the backward wrote gradients to the bucket again, and a silent no-op here would
            # freeze the parameters
            raise RuntimeError("FlatAdamW.step(): this optimizer was fused into a rasterizer backward, but that context no longer "
                               "carries it (context.fused_adamw was cleared by hand?) -- call optimizer.unfuse() to go back to step()")
        from ._lib import AdamWFlatArgs
        if skip_word is not None:
            if self.step_state is None:
                raise RuntimeError("a guarded step needs capturable=True: a host-side step count cannot know about the skipped step")
            if self.shard is not None:
                # one rank's frame overflowed, its peers' did not: this rank would skip ITS shard's update while the others step theirs,
                # and the all-gather would then spread a half-stepped parameter vector
                raise RuntimeError("a guarded step (skip_word) on a SHARDED optimizer: the skip is a per-rank decision and would leave the "
                                   "shards at different steps; guard the frame before the gradient exchange instead")
        else:
            self.t += 1
        first, count = (0, self.n) if self.shard is None else (self.first, self.count)
        if count == 0:
            return
        grads = self.bucket.flat if self.shard is None else self.grad_shard
        self._floor_sh_degree()
        # ONE entry point for every form (C ABI moss_adamw_flat_ex: host / device step count, shard range, frame guard) -- and the
        # degree-aware SH update (set_active_sh_degree)
        a = AdamWFlatArgs()
        a.first, a.count = first, count
        a.params, a.grads = self.flat_params[first:].data_ptr(), grads.data_ptr()
        a.exp_avg, a.exp_avg_sq = self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()
        a.num_segments = self.nseg
        a.segment_end, a.segment_lr = C.addressof(self.seg_end), C.addressof(self.seg_lr)
        a.segment_period, a.segment_split, a.segment_lr2 = C.addressof(self.seg_period), C.addressof(self.seg_split), C.addressof(self.seg_lr2)
        act = self._seg_active()
        a.segment_active, a.inactive_zero = C.addressof(act), int(self.sh_inactive_zero)
        a.beta1, a.beta2, a.eps, a.weight_decay = float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.weight_decay)
        a.step = max(self.t, 1)
        a.step_state, a.skip_word = ptr(self.step_state), ptr(skip_word)
        a.skip_mask = int(skip_mask) & 0xffffffff
        extra = list(extra_grads or [])
        if len(extra) > 3:
            raise ValueError("at most three extra gradient buffers (four views per step)")
        a.num_grads_extra, a.grad_scale = len(extra), float(grad_scale)
        for i, e in enumerate(extra):
            if e.numel() < grads.numel() or e.dtype != torch.float32 or e.device != grads.device or not e.is_contiguous():
                raise ValueError("an extra gradient buffer must be a contiguous float32 tensor laid out like the bucket")
            a.grads_extra[i] = e[first:].data_ptr() if self.shard is None else e.data_ptr()
        call("moss_adamw_flat_ex", dev, C.addressof(a))


_SHARDED_ROWS = ("row surgery on a SHARDED FlatAdamW: a parameter row's moments live on several ranks; use the all-reduce "
                 "exchange while the set densifies (or gather, rebuild and re-shard)")


def _relayout_rows_of(members, row_map, exts, check, rows_old, extra):
    """``FlatAdamW.relayout_rows`` for one optimizer or several (``FlatAdamWRows``): ``exts[k]`` maps an index in member k's bucket to
    the rows appended to that parameter.  Validate everything first, then describe (every member: new layout, new buffers,
    descriptors), launch ONCE, adopt (every member)."""
    from ._lib import ROWS_MAX_TENSORS, RowsRelayoutArgs
    if any(o.shard is not None for o in members):
        raise RuntimeError(_SHARDED_ROWS)
    dev = members[0].flat_params.device
    norm = []
    for o, ext in zip(members, exts):
        params, d = o.bucket.params, {}
        for i, t in ext.items():
            e = t.detach().to(device=dev, dtype=torch.float32).contiguous()
            if tuple(e.shape[1:]) != tuple(params[i].shape[1:]):
                raise ValueError(f"relayout_rows: rows of shape {tuple(e.shape)} do not extend a parameter of shape {tuple(params[i].shape)}")
            d[i] = e
        norm.append(d)
    rows_app = {int(e.shape[0]) for d in norm for e in d.values()}
    olds = {int(o.bucket.params[i].shape[0]) for o, d in zip(members, norm) for i in d}
    if len(rows_app) > 1 or len(olds) > 1:
        raise ValueError("relayout_rows: the appended tensors must extend parameters of ONE row count by ONE number of rows")
    rows_app = rows_app.pop() if rows_app else 0
    if rows_old is None:
        rows_old = olds.pop() if olds else next(int(p.shape[0]) for o in members for p in o.bucket.params if p.dim() >= 1)
    rows_old = int(rows_old)
    if rows_app == 0:
        norm = [{} for _ in members]
    is_rows = [o._row_params(rows_old) for o in members]
    if len(members) > 1:
        _same_row_count(members, rows_old)
    if rows_app and any([i for i, r in enumerate(is_row) if r] != sorted(d) for is_row, d in zip(is_rows, norm)):
        raise ValueError("relayout_rows: `appended` must name every parameter of rows_old rows (and no other)"
                         + (" of every member" if len(members) > 1 else ""))
    extra = list(extra or [])
    if extra and rows_app:
        raise ValueError("relayout_rows: `extra` tensors ride along only when nothing is appended")
    for t in extra:
        if t.dtype != torch.float32 or t.device != dev or t.dim() < 1 or int(t.shape[0]) != rows_old:
            raise ValueError("relayout_rows: an `extra` tensor must be float32, on the optimizer's device, with rows_old rows")
    row_map = row_map.to(dev)
    if row_map.dim() != 1 or row_map.dtype not in (torch.int32, torch.int64):
        raise ValueError("relayout_rows: row_map must be a 1-D int32 / int64 tensor")
    rows_new = int(row_map.numel())
    if check and rows_new and (int(row_map.min()) < 0 or int(row_map.max()) >= rows_old + rows_app):
        raise ValueError(f"relayout_rows: row_map has entries outside [0, {rows_old + rows_app})")
    # (the limit of one launch; a group holds to it on CPU tensors too, so that what passes there passes on the GPU)
    if (dev.type == "cuda" or len(members) > 1) and sum(len(o.bucket.params) for o in members) + len(extra) > ROWS_MAX_TENSORS:
        raise ValueError(f"relayout_rows: more than {ROWS_MAX_TENSORS} tensors in one launch")
    if dev.type != "cuda":
        gathered = [o._relayout_rows_torch(row_map, d, is_row, extra if k == 0 else ())
                    for k, (o, d, is_row) in enumerate(zip(members, norm, is_rows))]
        return gathered[0]
    row_map = row_map.to(torch.int32).contiguous()
    a = RowsRelayoutArgs()
    a.rows_old, a.rows_app, a.rows_new, a.map = rows_old, rows_app, rows_new, row_map.data_ptr()
    k, plans = 0, []
    for o, d, is_row in zip(members, norm, is_rows):
        k, plan = o._rows_describe(a, k, is_row, d, rows_new)
        plans.append(plan)
    gathered = []
    for t in extra:
        t = t.contiguous()
        g = torch.empty((rows_new,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev)
        gathered.append((t, g))
        if g.numel() == 0:
            continue
        d = a.tensors[k]
        k += 1
        d.src, d.dst, d.use_map, d.pad_after = t.data_ptr(), g.data_ptr(), 1, 0
        d.width = int(torch.Size(t.shape[1:]).numel())
    a.num_tensors = k
    call("moss_rows_relayout", dev, C.addressof(a))
    for o, plan in zip(members, plans):
        o._rows_adopt(plan)
    return [g for _, g in gathered] if extra else None


def _same_row_count(members, rows):
    for k, o in enumerate(members):
        if not any(o._row_params(rows)):
            lead = sorted({int(p.shape[0]) for p in o.bucket.params if p.dim() >= 1})
            raise ValueError(f"FlatAdamWRows: member {k} holds no parameter of {rows} rows (leading dimensions of its parameters: {lead}): "
                             "the members' row-parameters have different row counts")


class FlatAdamWRows:
    """Several ``FlatAdamW`` whose row-parameters have ONE row count, presented as one optimizer for row surgery:
    ``rows = FlatAdamWRows([opt_a, opt_b])``.  ``GaussianSet.densification_postfix / prune_points / relayout_points / reset_opacity /
    reorder_spatially``, ``densify.densify_and_prune_fused`` and ``surgery.densification_event`` take it where they take a
    ``FlatAdamW`` (``MossStep`` keeps the Gaussians in two: features / opacity / scaling / rotation, updated inside the rasterizer's
    backward kernel, and the position).  It steps nothing and owns nothing: every member keeps its step counter, its learning-rate
    state block and its parameters that are not per-row, bit for bit.

    ``bucket.params`` lists all members' parameters in member order; a parameter is named by the object or by its index in that list.
    ``relayout_rows`` on GPU tensors is ONE ``moss_rows_relayout`` launch for all members (absolute addresses in the descriptors, at
    most ``MOSS_ROWS_MAX_TENSORS`` of them, the ``extra`` tensors included); the other calls go to each member in turn.

    Refused: a sharded member, a parameter that two members hold, members whose row-parameters differ in row count (the row count is
    that of the first member's first parameter)."""

    def __init__(self, members):
        from types import SimpleNamespace
        self.members = list(members)
        if not self.members:
            raise ValueError("FlatAdamWRows: no member")
        if any(o.shard is not None for o in self.members):
            raise RuntimeError(_SHARDED_ROWS)
        params, self._where = [], {}
        for k, o in enumerate(self.members):
            for i, p in enumerate(o.bucket.params):
                if id(p) in self._where:
                    raise ValueError(f"FlatAdamWRows: members {self._where[id(p)][0]} and {k} both hold one parameter (of shape "
                                     f"{tuple(p.shape)}): its moments would be moved twice")
                self._where[id(p)] = (k, i)
                params.append(p)
        self.bucket = SimpleNamespace(params=params)         # (the Parameter objects survive every surgery: the list stays true)
        self.relayouts = 0                                   # relayout_rows calls carried out so far (on GPU tensors: launches)
        _same_row_count(self.members, self.rows)

    @property
    def rows(self) -> int:
        """The row count that marks a row-parameter now."""
        return next(int(p.shape[0]) for p in self.bucket.params if p.dim() >= 1)

    def _split(self, named):
        """``{parameter or index in bucket.params: value}`` -> one ``{index in the member's bucket: value}`` per member."""
        per = [{} for _ in self.members]
        for key, val in (named or {}).items():
            k, i = self._where[id(self.bucket.params[key] if isinstance(key, int) else key)]
            per[k][i] = val
        return per

    def append_rows(self, new_rows):
        per = self._split(new_rows)
        named = {int(o.bucket.params[i].shape[0]) for o, d in zip(self.members, per) for i in d}
        for k, (o, d) in enumerate(zip(self.members, per)):
            if any(r and i not in d for n in named for i, r in enumerate(o._row_params(n))):
                raise ValueError(f"FlatAdamWRows.append_rows: `new_rows` must name every row-parameter of every member (member {k} has "
                                 "one that is not named): the members would end with different row counts")
        for o, d in zip(self.members, per):
            if d:
                o.append_rows(d)

    def prune_rows(self, keep_mask):
        _same_row_count(self.members, int(keep_mask.numel()))
        for o in self.members:
            o.prune_rows(keep_mask)

    def permute_rows(self, perm):
        _same_row_count(self.members, int(perm.numel()))
        for o in self.members:
            o.permute_rows(perm)

    def reset_rows(self, param, values):
        k, i = self._where[id(self.bucket.params[param] if isinstance(param, int) else param)]
        self.members[k].reset_rows(i, values)

    def set_active_sh_degree(self, degree: int):
        """To every member (one without an SH parameter answers 3); returns the lowest degree in force."""
        return min(o.set_active_sh_degree(degree) for o in self.members)

    @torch.no_grad()
    def relayout_rows(self, row_map, appended=None, check=True, rows_old=None, extra=None):
        """``FlatAdamW.relayout_rows`` over all members: one launch on GPU tensors, the members' torch restatement on CPU tensors.
        ``appended`` must name every row-parameter of every member."""
        out = _relayout_rows_of(self.members, row_map, self._split(appended), check, rows_old, extra)
        self.relayouts += 1
        return out


class AdamW(torch.optim.Optimizer):
    """Drop-in for ``torch.optim.AdamW(params, lr, betas, eps, weight_decay)`` as MOSS builds it (scene/gaussian_model.py:226:
    eight parameter groups, ``lr=0.0, eps=1e-15``): the same update rule, ONE kernel for all the single-tensor groups (C ABI
    ``moss_adamw_multi``: up to eight tensors with their own state tensors and step counts per launch; rounds 4-5: one launch per tensor of
    the flat update, bit-identical) instead of torch's nine ``multi_tensor_apply`` launches per group -- with MOSS's six single-tensor
    Gaussian groups that is 54 launches of ~13 us per step, more than half of the patched call pattern's step (rocprofv3,
    ``profiles/r04_notes.md``).

    Everything MOSS does to its optimizer keeps working: ``param_groups`` with per-group ``lr`` rewritten every iteration
    (``update_learning_rate``), and the densification surgery on ``state[p]["exp_avg"] / ["exp_avg_sq"]`` (``cat_tensors_to_optimizer``,
    ``_prune_optimizer``, ``replace_tensor_to_optimizer``, scene/gaussian_model.py:362-430) -- the state keys and meanings are torch's
    (``step`` is kept as a Python int).  Parameters that are not contiguous float32 GPU tensors (or have no 16-byte aligned storage)
    take torch's own functional AdamW.  Not capturable in a hipGraph (the step count is a launch argument): the graph path uses
    :class:`FlatAdamW`."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        from ._lib import AdamWMultiArgs
        self._multi = AdamWMultiArgs()

    # A group of MANY tensors (MOSS's two network groups, scene/gaussian_model.py:222-223: the parameters of `auto_regression` and
    # `cross_attention_lbs`) is stepped with torch's multi-tensor primitives -- nine launches for the whole group, where one kernel per
    # tensor would be dozens; the single-tensor Gaussian groups are where one kernel replaces nine.  (THIS class keeps torch's
    # per-tensor state.  `FlatAdamW` takes such groups too -- one learning-rate segment per group, however many tensors, one launch for
    # both networks, capturable: `moss_amd.train.MossStep`.)
    FOREACH_ABOVE = 4

    def _foreach_group(self, group) -> bool:
        ps = [p for p in group["params"] if p.grad is not None]
        if not ps:
            return True
        for p in ps:
            st = self.state[p]
            if len(st) == 0:
                st["step"] = 0
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        steps = {int(self.state[p]["step"]) for p in ps}
        if len(steps) != 1 or len({(p.device, p.dtype) for p in ps}) != 1:
            return False                                     # (tensors that joined later, mixed devices: one by one below)
        t = steps.pop() + 1
        beta1, beta2 = group["betas"]
        lr, wd, eps = group["lr"], group["weight_decay"], group["eps"]
        gs = [p.grad for p in ps]
        ms = [self.state[p]["exp_avg"] for p in ps]
        vs = [self.state[p]["exp_avg_sq"] for p in ps]
        torch._foreach_mul_(ps, 1 - lr * wd)
        torch._foreach_lerp_(ms, gs, 1 - beta1)
        torch._foreach_mul_(vs, beta2)
        torch._foreach_addcmul_(vs, gs, gs, 1 - beta2)
        denom = torch._foreach_sqrt(vs)
        torch._foreach_div_(denom, (1 - beta2 ** t) ** 0.5)
        torch._foreach_add_(denom, eps)
        torch._foreach_addcdiv_(ps, ms, denom, -lr / (1 - beta1 ** t))
        for p in ps:
            self.state[p]["step"] = t
        return True

    @staticmethod
    def _native_ok(*tensors):
        return all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0 for t in tensors)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # the single tensors of ALL groups that the kernel can take, batched by what a launch holds as scalars (device, betas, eps, weight
        # decay): MOSS's six Gaussian groups share them, so its step is ONE launch (C ABI moss_adamw_multi; up to eight tensors each)
        batches = {}
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            if len(group["params"]) > self.FOREACH_ABOVE and self._foreach_group(group):
                continue
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] = int(st["step"]) + 1
                g, m, v = p.grad, st["exp_avg"], st["exp_avg_sq"]
                n = p.numel()
                if n == 0:
                    continue
                if self._native_ok(p, g, m, v):
                    key = (p.device, float(beta1), float(beta2), float(group["eps"]), float(group["weight_decay"]))
                    batches.setdefault(key, []).append((p, g, m, v, float(group["lr"]), int(st["step"])))
                else:                                        # torch's expressions (CPU tensors, other dtypes, views with odd alignment)
                    p.mul_(1 - group["lr"] * group["weight_decay"])
                    m.lerp_(g, 1 - beta1)
                    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
                    bc1, bc2 = 1 - beta1 ** st["step"], 1 - beta2 ** st["step"]
                    p.addcdiv_(m, (v.sqrt() / (bc2 ** 0.5)).add_(group["eps"]), value=-group["lr"] / bc1)
        if batches:
            L = lib()
            a = self._multi
            for (dev, beta1, beta2, eps, wd), items in batches.items():
                a.beta1, a.beta2, a.eps, a.weight_decay = beta1, beta2, eps, wd
                with torch.cuda.device(dev):
                    s = stream(dev)
                    for i0 in range(0, len(items), 8):
                        part = items[i0:i0 + 8]
                        a.num_tensors = len(part)
                        for k, (p, g, m, v, lr, t) in enumerate(part):
                            a.numel[k], a.params[k], a.grads[k], a.exp_avg[k], a.exp_avg_sq[k] = p.numel(), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
                            a.lr[k], a.step[k] = lr, t
                        check(L.moss_adamw_multi(C.addressof(a), s), "adamw_multi")
        return loss
