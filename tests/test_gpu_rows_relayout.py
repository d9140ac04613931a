"""The one-pass row re-layout on the GPU (csrc/rows.hip; include/moss_raster.h: moss_rows_keep_map, moss_rows_relayout).

  1  the row map against ``torch.nonzero``;  2  the gather through the C ABI against ``index_select``, compared as int32 (NaN payloads
  and -0.0 count), with zeroed gaps, zero moments for appended rows and untouched guard bands;  3  the refusals;  4
  ``FlatAdamW.relayout_rows`` on twin optimizers after real steps against the two-call path, and that the step is re-armed;  5
  ``densification_event(one_pass=True)`` on the scripted schedule of tests/test_gpu_surgery.py;  6  ``densify_and_prune_fused(one_pass=
  True)`` on the reference's own run (tests/golden/densify_decision.npz);  7  ``keep_spatial_order``.

Everything the one-pass path produces must be BIT-IDENTICAL to what the default path (torch indexing, two copies) produces."""
import ctypes as C

import numpy as np
import pytest
import torch

from moss_amd import densify as D
from moss_amd import scenes
from tests import test_densify_decision_cpu as cpu
from tests import test_gpu_densify_decision as dd
from tests import test_gpu_headline as thl
from tests import test_gpu_surgery as sg
from tests.golden import make_golden_densify as gold

pytestmark = pytest.mark.gpu

GUARD = 64                                   # floats of guard band on each side of a destination
NAN_BITS = 0x7FC12345


def _bits(shape, gen, gpu):
    """float32 tensors of RANDOM BIT PATTERNS (NaNs with payloads, infinities, denormals, -0.0 among them)."""
    t = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=gen, dtype=torch.int64).to(torch.int32)
    t.view(-1)[::17] = -2 ** 31                                              # -0.0
    return t.view(torch.float32).to(gpu)


def _i32(t):
    return t.contiguous().view(torch.int32)


# ---- 1: the row map ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_old", [1, 63, 64, 65, 255, 256, 257, 65537])
def test_keep_map_against_nonzero(gpu, hip_lib, rows_old):
    from moss_amd import _lib
    g = torch.Generator().manual_seed(rows_old)
    last = torch.ones(rows_old, dtype=torch.bool); last[-1] = False
    masks = {"none": torch.zeros(rows_old, dtype=torch.bool), "all": torch.ones(rows_old, dtype=torch.bool), "all_but_last": last,
             "random": torch.rand(rows_old, generator=g) < 0.3, "null": None}
    nbytes = int(hip_lib.moss_rows_map_workspace_bytes(rows_old))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    for name, mask in masks.items():
        for rows_app in (0, 1, 130):
            out = torch.full((rows_old + rows_app + 8,), -7, dtype=torch.int32, device=gpu)
            count = torch.full((1,), -7, dtype=torch.int32, device=gpu)
            m = None if mask is None else mask.to(gpu).to(torch.uint8)
            _lib.call("moss_rows_keep_map", gpu, rows_old, _lib.ptr(m), rows_app, out.data_ptr(), count.data_ptr(), ws.data_ptr(), C.c_size_t(nbytes))
            kept = torch.arange(rows_old) if mask is None else torch.nonzero(~mask).reshape(-1)
            want = torch.cat((kept, torch.arange(rows_old, rows_old + rows_app))).to(torch.int32)
            n = int(count.item())
            assert n == want.numel(), (name, rows_app)
            assert torch.equal(out[:n].cpu(), want), (name, rows_app)
            assert bool((out[n:] == -7).all()), (name, rows_app, "entries beyond the count were written")
    # the Python surface: same map, the count read once
    from moss_amd.surgery import rows_map
    reads = D.host_reads()
    m, n = rows_map(masks["random"].to(gpu), 130)
    assert D.host_reads() == reads + 1 and n == m.numel()
    assert torch.equal(m.cpu(), torch.cat((torch.nonzero(~masks["random"]).reshape(-1), torch.arange(rows_old, rows_old + 130))).to(torch.int32))
    m2, n2 = rows_map(masks["random"].to(gpu), 130, count=n)
    assert D.host_reads() == reads + 1 and torch.equal(m2, m)


# ---- 2: the gather through the C ABI ------------------------------------------------------------------------------------------------
WIDTHS = [1, 3, 4, 45, 48]
ROWS_APP = 5


def _guarded(total, gpu):
    t = torch.full((total + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=gpu)
    return t.view(torch.float32)


def _maps(rows_old, gpu):
    g = torch.Generator().manual_seed(100 + rows_old)
    total = rows_old + ROWS_APP
    remove = torch.rand(total, generator=g) < 0.3
    return {"identity": torch.arange(total), "keep_map": torch.nonzero(~remove).reshape(-1), "reversed": torch.arange(total - 1, -1, -1),
            "appended_only": torch.arange(rows_old, total), "empty": torch.zeros(0, dtype=torch.int64)}


@pytest.mark.parametrize("rows_old", [1, 64, 65, 1000])
def test_relayout_through_the_c_abi_against_index_select(gpu, hip_lib, rows_old):
    from moss_amd import _lib
    from moss_amd.dist import flat_offsets
    g = torch.Generator().manual_seed(rows_old)
    FIXED = 7                                                                # one tensor that is not per-row (use_map = 0)
    sizes_old = [rows_old * w for w in WIDTHS] + [FIXED]
    off_old, total_old = flat_offsets(sizes_old)
    src = [_bits((total_old,), g, gpu) for _ in range(3)]                    # values, exp_avg, exp_avg_sq
    app = [_bits((ROWS_APP, w), g, gpu) for w in WIDTHS]
    stat_old, stat_app = _bits((rows_old, 2), g, gpu), _bits((ROWS_APP, 2), g, gpu)      # one tensor WITHOUT moments
    for name, row_map in _maps(rows_old, gpu).items():
        rows_new = int(row_map.numel())
        sizes = [rows_new * w for w in WIDTHS] + [FIXED]
        off, total = flat_offsets(sizes)
        dst = [_guarded(total, gpu) for _ in range(3)]
        stat_dst = _guarded(rows_new * 2, gpu)
        m32 = row_map.to(torch.int32).to(gpu)
        a = _lib.RowsRelayoutArgs()
        a.rows_old, a.rows_app, a.rows_new, a.map, a.num_tensors = rows_old, ROWS_APP, rows_new, m32.data_ptr(), len(sizes) + 1
        ends = off[1:] + [total]
        for i, w in enumerate(WIDTHS + [FIXED]):
            d = a.tensors[i]
            d.src, d.src_m, d.src_v = (t.data_ptr() + 4 * off_old[i] for t in src)
            d.dst, d.dst_m, d.dst_v = (t.data_ptr() + 4 * (GUARD + off[i]) for t in dst)
            d.width, d.pad_after, d.use_map = w, ends[i] - (off[i] + sizes[i]), int(i < len(WIDTHS))
            d.app = app[i].data_ptr() if i < len(WIDTHS) else None
        d = a.tensors[len(sizes)]
        d.src, d.app, d.dst, d.width, d.pad_after, d.use_map = stat_old.data_ptr(), stat_app.data_ptr(), stat_dst.data_ptr() + 4 * GUARD, 2, 0, 1
        assert sum(a.tensors[i].pad_after for i in range(len(sizes))) > 0 or rows_new % 4 == 0
        _lib.call("moss_rows_relayout", gpu, C.addressof(a))
        idx = row_map.to(gpu)
        for k, (s, dt) in enumerate(zip(src, dst)):
            body = _i32(dt)[GUARD:GUARD + total]
            want = torch.zeros(total, dtype=torch.int32, device=gpu)         # (gaps read zero)
            for i, w in enumerate(WIDTHS):
                rows = _i32(s)[off_old[i]:off_old[i] + rows_old * w].view(rows_old, w)
                new = _i32(app[i]) if k == 0 else torch.zeros((ROWS_APP, w), dtype=torch.int32, device=gpu)   # appended rows: ZERO moments
                want[off[i]:off[i] + rows_new * w] = torch.cat((rows, new)).index_select(0, idx).reshape(-1)
            want[off[-1]:off[-1] + FIXED] = _i32(s)[off_old[-1]:off_old[-1] + FIXED]
            assert torch.equal(body, want), (name, ("values", "exp_avg", "exp_avg_sq")[k])
            assert bool((_i32(dt)[:GUARD] == NAN_BITS).all()) and bool((_i32(dt)[GUARD + total:] == NAN_BITS).all()), (name, "guard band")
        got = _i32(stat_dst)
        assert torch.equal(got[GUARD:GUARD + rows_new * 2], torch.cat((_i32(stat_old), _i32(stat_app))).index_select(0, idx).reshape(-1)), name
        assert bool((got[:GUARD] == NAN_BITS).all()) and bool((got[GUARD + rows_new * 2:] == NAN_BITS).all()), (name, "guard band")


# ---- 3: refusals ---------------------------------------------------------------------------------------------------------------------
def test_relayout_refusals_name_the_field_and_launch_nothing(gpu, hip_lib):
    from moss_amd import _lib
    st = _lib.stream(torch.device(gpu))
    src, dst = torch.ones(64, device=gpu), torch.full((64,), 5.0, device=gpu)
    row_map = torch.arange(8, dtype=torch.int32, device=gpu)

    def block():
        a = _lib.RowsRelayoutArgs()
        a.rows_old, a.rows_app, a.rows_new, a.map, a.num_tensors = 8, 0, 8, row_map.data_ptr(), 1
        d = a.tensors[0]
        d.src, d.dst, d.width, d.pad_after, d.use_map = src.data_ptr(), dst.data_ptr(), 4, 0, 1
        return a

    def refused(a, code, *words):
        rc = hip_lib.moss_rows_relayout(None if a is None else C.addressof(a), st)
        msg = hip_lib.moss_last_error().decode()
        assert rc == code and msg.startswith("moss_rows_relayout:") and all(w in msg for w in words), (rc, msg)
    with torch.cuda.device(gpu):
        refused(None, -1, "null argument block")
        a = block(); a.tensors[0].dst = None
        refused(a, -1, "tensors[0].dst")
        a = block(); a.map = None
        refused(a, -1, "map")
        a = block(); a.tensors[0].dst_m = dst.data_ptr() + 128                   # one moment pointer without the others
        refused(a, -1, "tensors[0].dst_v")
        a = block(); a.tensors[0].dst = src.data_ptr() + 16 * 4                  # destination inside the source range
        refused(a, -1, "tensors[0].dst", "overlaps", "tensors[0].src")
        a = block(); a.tensors[0].dst = row_map.data_ptr()
        refused(a, -1, "tensors[0].dst", "overlaps", "map")
        a = block(); a.rows_new = 2 ** 26; a.tensors[0].width = 48               # 2^26 * 48 >= 2^31
        refused(a, -5, "tensors[0].width", "2^31")
        a = block(); a.num_tensors = _lib.ROWS_MAX_TENSORS + 1
        refused(a, -5, "num_tensors")
        a = block(); a.tensors[0].pad_after = 4
        refused(a, -1, "tensors[0].pad_after")
        a = block(); a.tensors[0].width = 0
        refused(a, -1, "tensors[0].width")
        torch.cuda.synchronize(gpu)
        assert bool((dst == 5.0).all()) and bool((src == 1.0).all())             # nothing was launched
        a = block()
        assert hip_lib.moss_rows_relayout(C.addressof(a), st) == 0                 # (the block itself is fine)
        torch.cuda.synchronize(gpu)
        assert bool((dst[:32] == 1.0).all()) and bool((dst[32:] == 5.0).all())
        ws = torch.empty(4, dtype=torch.uint8, device=gpu)
        assert hip_lib.moss_rows_keep_map(8, None, 0, row_map.data_ptr(), None, ws.data_ptr(), C.c_size_t(4), st) == -1
        assert b"count_out" in hip_lib.moss_last_error()
        assert hip_lib.moss_rows_keep_map(300, None, 0, row_map.data_ptr(), row_map.data_ptr(), ws.data_ptr(), C.c_size_t(4), st) == -1
        assert b"workspace" in hip_lib.moss_last_error()


# ---- 4: FlatAdamW.relayout_rows on twin optimizers after real steps -------------------------------------------------------------------
class _Twin(sg.FormA):
    """tests/test_gpu_surgery.py's form A without the graph; ``fused=False`` takes the step out of the backward again (``step()`` applies
    the bucket's gradients with the flat kernel)."""

    def __init__(self, scene, gpu, gt, mask, T, fused):
        super().__init__(scene, gpu, gt, mask, T, degree=3, graph=False)
        if not fused:
            self.opt.unfuse()
        self.fused = fused

    def step(self):
        self.compute()
        if not self.fused:
            self.opt.step()
        self.steps += 1

    def state(self):
        o = self.opt
        return [o.flat_params, o.exp_avg, o.exp_avg_sq]


def _same_state(A, B, objs, relaid_out=False):
    for a, b, what in zip(A.state(), B.state(), ("parameters", "exp_avg", "exp_avg_sq")):
        assert a.shape == b.shape and torch.equal(_i32(a), _i32(b)), what
    assert list(A.bucket.offsets) == list(B.bucket.offsets) and A.bucket.n_params == B.bucket.n_params
    assert A.opt.step_count() == B.opt.step_count()
    assert [id(p) for p in A.bucket.params] == objs
    for p, off in zip(A.bucket.params, A.bucket.offsets):
        assert p.data_ptr() == A.opt.flat_params[off:off + 1].data_ptr()
        assert not relaid_out or p.grad is None                              # (a re-layout drops the gradients: they were views of the old bucket)


def _new_rows_like(pc, n, seed, gpu):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, pc._xyz.shape[0], (n,), generator=g).to(gpu)
    jitter = (0.01 * torch.randn(n, 3, generator=g)).to(gpu)
    return {pc._xyz: pc._xyz.data[src] + jitter, pc._features: pc._features.data[src].clone(), pc._opacity: pc._opacity.data[src].clone(),
            pc._scaling: pc._scaling.data[src] - 0.4, pc._rotation: pc._rotation.data[src].clone()}, src


@pytest.fixture(scope="module")
def cfg1_target(gpu):
    return sg._target(scenes.config1, gpu)


@pytest.mark.parametrize("case,fused", [("prune", True), ("append", False), ("append_prune", True), ("append_prune", False)])
def test_relayout_rows_equals_the_two_call_path_and_rearms_the_step(gpu, hip_lib, cfg1_target, case, fused):
    from moss_amd.surgery import rows_map
    scene = scenes.config1()
    gt, mask = cfg1_target
    T = thl.bench_transforms(scene.P)
    A, B = _Twin(scene, gpu, gt, mask, T, fused), _Twin(scene, gpu, gt, mask, T, fused)
    objs = [id(p) for p in A.bucket.params]
    for _ in range(3):
        A.step(); B.step()
    _same_state(A, B, objs)
    assert A.opt.step_count() == 3 and float(A.opt.exp_avg.abs().max()) > 0
    P = scene.P
    n_app = 37 if case != "prune" else 0
    g = torch.Generator().manual_seed(5)
    remove = torch.zeros(P + n_app, dtype=torch.bool)
    if case != "append":
        remove[torch.randperm(P + n_app, generator=g)[:41]] = True            # (old rows and, with an append, some of the new ones)
    remove = remove.to(gpu)
    rows_a, src = _new_rows_like(A.pc, n_app, 6, gpu) if n_app else (None, None)
    rows_b = _new_rows_like(B.pc, n_app, 6, gpu)[0] if n_app else None
    # one call ...
    row_map, n = rows_map(remove) if case != "append" else (torch.arange(P + n_app, dtype=torch.int32, device=gpu), P + n_app)
    A.opt.relayout_rows(row_map, rows_a)
    # ... against the existing two
    if n_app:
        B.opt.append_rows(rows_b)
    if case != "append":
        B.opt.prune_rows(~remove)
    assert A.pc._xyz.shape[0] == n == P + n_app - int(remove.sum())
    _same_state(A, B, objs, relaid_out=True)
    # the run goes on: the step (inside the backward, or the flat kernel) works on the NEW addresses
    Tn = T.to(gpu) if not n_app else torch.cat((T.to(gpu), T.to(gpu)[src]))
    for X in (A, B):
        X.T = Tn[row_map.long()].contiguous()
        X.ctx.relearn_capacity()
    before = A.opt.flat_params.clone()
    for _ in range(2):
        A.step(); B.step()
    _same_state(A, B, objs)
    assert A.opt.step_count() == 5 and not torch.equal(before, A.opt.flat_params)


# ---- 5: the event on the scripted schedule ------------------------------------------------------------------------------------------
class _FormAOnePass(sg.FormA):
    def __init__(self, *a, one_pass=False, keep_spatial_order=False, **k):
        super().__init__(*a, **k)
        self.one_pass, self.keep_spatial_order = one_pass, keep_spatial_order

    def event(self, ev):
        from moss_amd.surgery import densification_event
        return densification_event(self.pc, self.opt, append=ev["append"], prune=ev["prune"], reset_opacity=ev["reset_opacity"], stats=self.stats,
                                   context=self.ctx, graphed=self.graphed, probe=self.probe, per_gaussian={"T": self.T},
                                   after_surgery=lambda pg: setattr(self, "T", pg["T"]), one_pass=self.one_pass,
                                   keep_spatial_order=self.keep_spatial_order)


def _prune_only(form, seed, gpu):
    g = torch.Generator().manual_seed(seed)
    return {"append": [], "prune": (torch.rand(form.pc._xyz.shape[0], generator=g) < 0.05).to(gpu), "reset_opacity": False}


def _same_forms(A, B):
    ta, tb, ma, mb = A.tensors(), B.tensors(), A.moments(), B.moments()
    for k in sg.GROUPS:
        assert ta[k].shape == tb[k].shape and torch.equal(_i32(ta[k]), _i32(tb[k])), f"{k}: parameters differ"
        assert torch.equal(_i32(ma[k][0]), _i32(mb[k][0])) and torch.equal(_i32(ma[k][1]), _i32(mb[k][1])), f"{k}: moments differ"
    assert torch.equal(A.T, B.T) and list(A.bucket.offsets) == list(B.bucket.offsets)
    for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert getattr(A.stats, k).shape == getattr(B.stats, k).shape and torch.equal(getattr(A.stats, k), getattr(B.stats, k)), k


def test_event_one_pass_equals_the_default_event_on_the_scripted_schedule(gpu, hip_lib):
    scene = scenes.config2()
    gt, mask = sg._target(scenes.config2, gpu)
    T = thl.bench_transforms(scene.P)
    A = _FormAOnePass(scene, gpu, gt, mask, T, one_pass=True)
    B = _FormAOnePass(scene, gpu, gt, mask, T, one_pass=False)
    done = A.steps
    assert B.steps == done
    for target in (10, 20, 30):
        while done < target:
            A.step(); B.step(); done += 1
        torch.cuda.synchronize(gpu)
        for X in (A, B):                                        # (the statistics of a run: a prune keeps the surviving rows)
            gs = torch.Generator(device=gpu); gs.manual_seed(target)
            X.stats.denom.copy_(torch.rand(X.stats.denom.shape, generator=gs, device=gpu))
            X.stats.max_radii2D.copy_(torch.rand(X.stats.max_radii2D.shape, generator=gs, device=gpu))
        ev = sg.scripted_event(A.tensors(), target, gpu, reset_opacity=(target == 20))
        if target == 30:                                        # a prune alone: the statistics are gathered by the same launch
            ev = _prune_only(A, target, gpu)
        ra, rb = A.event(ev), B.event(ev)
        assert ra["recaptured"] and rb["recaptured"] and ra["rows_after"] == rb["rows_after"] != ra["rows_before"]
        assert set(ra) == set(rb)                               # (the report keys are unchanged)
        _same_forms(A, B)
        if target == 30:
            assert bool(A.stats.denom.any())
    for _ in range(5):
        A.step(); B.step()
    torch.cuda.synchronize(gpu)
    A.graphed.check(); B.graphed.check()
    _same_forms(A, B)
    assert A.opt.step_count() == B.opt.step_count() == done + 5


# ---- 6: the fused decision with one-pass surgery, on the reference's own run ---------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(cpu.FIXTURE)


def _drive(case, gpu, one_pass):
    g = gold.golden_inputs(case)
    pc, bucket, opt = dd._driver_set(g, gpu)
    stats = D.DensifyStats(gold.P, device=gpu)
    stats.xyz_gradient_accum.copy_(g["accum"].to(gpu)); stats.denom.copy_(g["denom"].to(gpu)); stats.max_radii2D.copy_(g["max_radii2D"].to(gpu))
    m_before = dd._moments(pc, opt)
    noise = iter([g["noise_clone"], g["noise_split"]])
    kw = {"one_pass": True} if one_pass else {}
    rep = D.densify_and_prune_fused(pc, opt, stats, g["joint_F"].to(gpu), g["lbs_weights"].to(gpu), gold.MAX_GRAD, gold.MIN_OPACITY, gold.EXTENT,
                                    gold.SCREEN[case], g["t_vertices"].to(gpu), kl_threshold=gold.KL_THRESHOLD,
                                    surface_mask=g["surface_mask"].to(gpu), generator=lambda n: next(noise)[:n], percent_dense=gold.PERCENT_DENSE, **kw)
    return g, pc, opt, stats, m_before, rep


@pytest.mark.parametrize("case", list(gold.CASES))
def test_fused_decision_one_pass_reproduces_the_reference_and_the_default_path(gpu, hip_lib, golden, case):
    """The comparisons of test_driver_reproduces_the_reference_on_a_gaussian_set (tests/test_gpu_densify_decision.py) on the one-pass
    path, then bit-equality with the default path.  ``host_reads``: the four counts of the decision ops, plus the ONE map length the
    counts do not give (the merge's mask is extended on the device by ``merge_rows``) -- the default path reads the same number
    inside its boolean indexing, uncounted."""
    g, pc, opt, stats, m_before, rep = _drive(case, gpu, True)
    print("\n", case, rep)
    assert rep["relayouts"] <= 4 and rep["host_reads"] <= 4 + (1 if rep["merged"] else 0)
    for ph, key in (("clone", "cloned"), ("split", "split"), ("merge", "merged")):
        assert rep[key] == int(golden[f"{case}_{ph}_mask"].sum()), ph
    assert rep["pruned"] == int(golden[f"{case}_final_prune_filter"].sum())
    assert rep["rows_after"] == golden[f"{case}_final_xyz"].shape[0] == pc._xyz.shape[0] == stats.denom.shape[0]
    lin = cpu.replay(case, torch.float64)["final"]["lineage"]
    got = {"xyz": pc._xyz, "features_dc": pc._features_dc, "features_rest": pc._features_rest, "opacity": pc._opacity,
           "scaling": pc._scaling, "rotation": pc._rotation}
    for k, v in cpu.final_ratios(got, lin, golden, case, g).items():
        assert v < 1.0, (k, v)
    old, origin = (lin.origin >= 0).to(gpu), lin.origin.clamp_min(0).to(gpu)
    assert int(old.sum()) > 100 and int((~old).sum()) > 100
    for k, (m, v) in dd._moments(pc, opt).items():
        for name, after, before in (("exp_avg", m, m_before[k][0]), ("exp_avg_sq", v, m_before[k][1])):
            assert after.shape[0] == rep["rows_after"], (k, name)
            assert torch.equal(after[old], before[origin[old]]), f"{k}.{name}: a surviving row lost its moments"
            assert not bool(after[~old].any()), f"{k}.{name}: a new row has non-zero moments"
    assert bool((stats.xyz_gradient_accum == 0).all()) and bool((stats.max_radii2D == 0).all())
    # ---- the default path, same inputs: the same bits everywhere
    _, pc2, opt2, stats2, _, rep2 = _drive(case, gpu, False)
    assert "relayouts" not in rep2 and {k: v for k, v in rep.items() if k not in ("relayouts", "host_reads")} == {k: v for k, v in rep2.items() if k != "host_reads"}
    for a, b, what in zip((opt.flat_params, opt.exp_avg, opt.exp_avg_sq), (opt2.flat_params, opt2.exp_avg, opt2.exp_avg_sq), ("parameters", "exp_avg", "exp_avg_sq")):
        assert a.shape == b.shape and torch.equal(_i32(a), _i32(b)), what
    assert list(opt.bucket.offsets) == list(opt2.bucket.offsets)
    for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert torch.equal(getattr(stats, k), getattr(stats2, k)), k


# ---- 7: keep_spatial_order ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_append", [True, False])
def test_keep_spatial_order_equals_the_default_event_then_reorder(gpu, hip_lib, monkeypatch, with_append):
    from moss_amd.diff_gaussian_rasterization import _C
    scene = scenes.config2()
    gt, mask = sg._target(scenes.config2, gpu)
    T = thl.bench_transforms(scene.P)
    A = _FormAOnePass(scene, gpu, gt, mask, T, graph=False, one_pass=True, keep_spatial_order=True)
    B = _FormAOnePass(scene, gpu, gt, mask, T, graph=False)
    for X in (A, B):
        perm = X.pc.reorder_spatially(X.opt)
        X.T = X.T[perm].contiguous()
        X.ctx.relearn_capacity()
        for _ in range(3):
            X.step()
        X.stats.denom.copy_(torch.arange(X.stats.denom.numel(), device=gpu, dtype=torch.float32).view(-1, 1) + 1.0)
    _same_forms(A, B)
    ev = sg.scripted_event(A.tensors(), 7, gpu, reset_opacity=False)
    if not with_append:
        ev = _prune_only(A, 7, gpu)
    ra, rb = A.event(ev), B.event(ev)
    assert A.pc.spatially_ordered and not B.pc.spatially_ordered
    perm = B.pc.reorder_spatially(B.opt)                       # the default event, THEN the re-ordering: statistics and tables by hand
    B.T = B.T[perm].contiguous()
    B.stats.xyz_gradient_accum, B.stats.denom, B.stats.max_radii2D = (t[perm].contiguous() for t in (B.stats.xyz_gradient_accum, B.stats.denom, B.stats.max_radii2D))
    assert ra["rows_after"] == rb["rows_after"] != ra["rows_before"]
    assert torch.equal(ra["per_gaussian"]["T"], B.T)
    _same_forms(A, B)
    assert with_append or bool(A.stats.denom.any())
    # the order is the Morton order of the new positions, and the hint bit reaches the op
    assert torch.equal(D.spatial_order(A.pc._xyz.detach()), torch.arange(A.pc._xyz.shape[0], device=gpu))
    import moss_amd.diff_gaussian_rasterization as dgr
    seen = []
    real = dgr.GaussianRasterizer.forward

    def spy(self, *a, **k):
        seen.append(int(k.get("raw_flags", 0)))
        return real(self, *a, **k)
    monkeypatch.setattr(dgr.GaussianRasterizer, "forward", spy)
    A.ctx.relearn_capacity(); A.step()
    assert seen and all(f & _C.HINT_SPATIAL_ORDER for f in seen)
    seen.clear()
    B.ctx.relearn_capacity(); B.step()
    assert seen and all(f & _C.HINT_SPATIAL_ORDER for f in seen)   # (B was re-ordered by hand: the same hint, the same step)
    _same_forms(A, B)
