"""CPU tests of the one-pass row re-layout (``moss_rows_relayout`` / ``moss_rows_keep_map``, csrc/rows.hip): the library exports the
entry points the header declares, the ctypes structs have the header's sizes, and -- on CPU tensors, where ``FlatAdamW.relayout_rows``
runs its torch restatement -- one call ends bit-identical to ``append_rows`` followed by ``prune_rows``: parameters, both moments,
offsets, and the Parameter objects.  The kernels themselves: tests/test_gpu_rows_relayout.py."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_surgery_cpu import _fill_moments, _model, _new_rows, _scripted_event
from tests.helpers import c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "moss_raster.h")
ENTRY_POINTS = ("moss_rows_relayout", "moss_rows_keep_map", "moss_rows_map_workspace_bytes")


def test_library_exports_the_row_entry_points_and_the_header_declares_them(hip_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/moss_raster.h"
        assert hasattr(hip_lib, name), f"{name} is not exported"
    assert re.search(r"#define\s+MOSS_ABI_VERSION\s+7\b", text) and hip_lib.moss_abi_version() == 7
    # one total per workgroup of 256 rows, at least one
    assert hip_lib.moss_rows_map_workspace_bytes(0) == 4 and hip_lib.moss_rows_map_workspace_bytes(256) == 4
    assert hip_lib.moss_rows_map_workspace_bytes(257) == 8 and hip_lib.moss_rows_map_workspace_bytes(65537) == 4 * 257


def test_ctypes_structs_have_the_headers_sizes(tmp_path):
    """A C program that includes the header prints sizeof / offsetof; the ctypes mirrors must agree."""
    from moss_amd import _lib
    cc = os.environ.get("CXX", "g++") + " -x c++"            # (the compiler the build uses for the torch extension)
    got = c_layout(tmp_path, "moss_rows_relayout_args", ["tensors", "map"], cc=cc,
                   extra=["sizeof(moss_rows_tensor)", "offsetof(moss_rows_tensor, width)", "MOSS_ROWS_MAX_TENSORS"])
    assert got == [ctypes.sizeof(_lib.RowsRelayoutArgs), _lib.RowsRelayoutArgs.tensors.offset, _lib.RowsRelayoutArgs.map.offset,
                   ctypes.sizeof(_lib.RowsTensor), _lib.RowsTensor.width.offset, _lib.ROWS_MAX_TENSORS]


def _appended(pc, d):
    return {pc._xyz: d["xyz"], pc._features: torch.cat((d["f_dc"], d["f_rest"]), dim=1), pc._opacity: d["opacity"],
            pc._scaling: d["scaling"], pc._rotation: d["rotation"]}


def _twins(seed=1):
    out = []
    for _ in range(2):
        pc, bucket, opt = _model(P=53)
        _fill_moments(opt, seed)
        opt.t = 17
        out.append((pc, bucket, opt))
    return out


def _assert_twins(a, b, objs):
    (pa, ba, oa), (pb, bb, ob) = a, b
    assert list(ba.offsets) == list(bb.offsets) and ba.sizes == bb.sizes and ba.n_params == bb.n_params
    assert torch.equal(oa.flat_params.view(torch.int32), ob.flat_params.view(torch.int32))
    assert torch.equal(oa.exp_avg.view(torch.int32), ob.exp_avg.view(torch.int32))
    assert torch.equal(oa.exp_avg_sq.view(torch.int32), ob.exp_avg_sq.view(torch.int32))
    for p, q in zip(ba.params, bb.params):
        assert p.shape == q.shape and torch.equal(p.data, q.data)
    assert [id(p) for p in ba.params] == objs and oa.t == ob.t == 17
    assert [int(e) for e in oa.seg_end] == [int(e) for e in ob.seg_end] and oa.n == ob.n
    for p, off in zip(ba.params, ba.offsets):
        assert p.grad is None and p.data_ptr() == oa.flat_params[off:off + 1].data_ptr()


def test_relayout_rows_on_cpu_equals_append_rows_then_prune_rows():
    from moss_amd.surgery import rows_map
    A, B = _twins()
    objs = [id(p) for p in A[1].params]
    P = 53
    # ---- an append alone (identity map over old + new rows)
    d = _new_rows(7, 10)
    A[2].relayout_rows(torch.arange(P + 7, dtype=torch.int32), _appended(A[0], d))
    B[2].append_rows(_appended(B[0], d))
    _assert_twins(A, B, objs)
    # ---- a prune alone
    g = torch.Generator().manual_seed(4)
    mask = torch.zeros(P + 7, dtype=torch.bool)
    mask[torch.randperm(P + 7, generator=g)[:9]] = True
    m, n = rows_map(mask)
    assert n == P + 7 - 9
    A[2].relayout_rows(m)
    B[2].prune_rows(~mask)
    _assert_twins(A, B, objs)
    # ---- append, then prune, in one call (the mask spans old + new rows and takes one of the new rows too)
    P1 = P - 2
    d2 = _new_rows(10, 11)
    mask = torch.zeros(P1 + 10, dtype=torch.bool)
    mask[torch.randperm(P1, generator=g)[:5]] = True
    mask[P1 + 3] = True
    m, n = rows_map(mask)
    A[2].relayout_rows(m, _appended(A[0], d2))
    B[2].append_rows(_appended(B[0], d2)); B[2].prune_rows(~mask)
    _assert_twins(A, B, objs)
    assert A[0]._xyz.shape[0] == P1 + 10 - 6
    # ---- refusals
    with pytest.raises(ValueError):
        A[2].relayout_rows(torch.tensor([0, 1, 10 ** 6], dtype=torch.int32))
    with pytest.raises(ValueError):
        A[2].relayout_rows(torch.arange(3, dtype=torch.int32), {A[0]._xyz: torch.zeros(2, 3)})      # (not every row-parameter named)


def test_event_one_pass_on_cpu_equals_the_default_event():
    """``densification_event(one_pass=True)`` on CPU objects (torch restatement of the gather) against the default path: two appends
    and a prune folded into one re-layout; statistics and a per-Gaussian table follow."""
    from moss_amd import surgery
    from moss_amd.densify import DensifyStats
    A, B = _twins(seed=2)
    objs = [id(p) for p in A[1].params]
    reports = []
    for (pc, bucket, opt), one_pass in ((A, True), (B, False)):
        stats = DensifyStats.__new__(DensifyStats)
        stats.xyz_gradient_accum, stats.denom, stats.max_radii2D = torch.rand(53, 1), torch.rand(53, 1), torch.rand(53)
        table = torch.arange(53 * 2, dtype=torch.float32).view(53, 2)
        real = surgery.densification_event
        try:
            surgery.densification_event = lambda *a, **k: real(*a, one_pass=one_pass, per_gaussian={"T": table}, **k)
            reports.append((_scripted_event(pc, opt, stats, step=3), stats))
        finally:
            surgery.densification_event = real
    _assert_twins(A, B, objs)
    (ra, sa), (rb, sb) = reports
    assert ra["rows_after"] == rb["rows_after"] != ra["rows_before"]
    assert torch.equal(ra["per_gaussian"]["T"], rb["per_gaussian"]["T"])
    for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert getattr(sa, k).shape == getattr(sb, k).shape and torch.equal(getattr(sa, k), getattr(sb, k))
    # a prune alone keeps the surviving rows of the statistics
    for (pc, bucket, opt), one_pass, stats in ((A, True, sa), (B, False, sb)):
        P = pc._xyz.shape[0]
        g = torch.Generator().manual_seed(9)
        stats.denom = torch.rand(P, 1, generator=g); stats.xyz_gradient_accum = torch.rand(P, 1, generator=g); stats.max_radii2D = torch.rand(P, generator=g)
        prune = torch.zeros(P, dtype=torch.bool)
        prune[::7] = True
        surgery.densification_event(pc, opt, prune=prune, stats=stats, one_pass=one_pass)
    _assert_twins(A, B, objs)
    for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert torch.equal(getattr(sa, k), getattr(sb, k)) and bool(getattr(sa, k).any())
    with pytest.raises(ValueError):
        surgery.densification_event(A[0], A[2], keep_spatial_order=True)


def test_rows_map_restated_in_torch_against_nonzero():
    from moss_amd.surgery import rows_map, rows_map_torch
    g = torch.Generator().manual_seed(0)
    for rows_old in (1, 63, 64, 65, 257):
        for mask in (torch.zeros(rows_old, dtype=torch.bool), torch.ones(rows_old, dtype=torch.bool), torch.rand(rows_old, generator=g) < 0.3):
            for rows_app in (0, 1, 130):
                m, n = rows_map(mask, rows_app)                # (CPU tensors: the torch form)
                want = torch.cat((torch.nonzero(~mask).reshape(-1), torch.arange(rows_old, rows_old + rows_app))).to(torch.int32)
                assert n == want.numel() and m.dtype == torch.int32 and torch.equal(m, want)
                assert torch.equal(rows_map_torch(mask.to(torch.uint8), rows_app)[0], want)
    m, n = rows_map(None, 3, rows_old=5)
    assert n == 8 and torch.equal(m, torch.arange(8, dtype=torch.int32))


@pytest.mark.parametrize("rows", [0, 1, 53, 1000])
def test_offsets_computed_ahead_equal_the_buckets(rows):
    """``dist.flat_offsets`` -- what ``relayout_rows`` places the rows with BEFORE any buffer exists -- against ``GradBucket._layout`` on
    parameters of widths 1, 3, 4, 45 and 48 (and one that is not per-row)."""
    from moss_amd import dist as mdist
    shapes = [(rows, 1), (rows, 3), (rows, 4), (rows, 15, 3), (rows, 16, 3), (7,), (rows,)]
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    b = mdist.GradBucket(params)
    offsets, total = mdist.flat_offsets([int(torch.Size(s).numel()) for s in shapes])
    assert offsets == list(b.offsets) and total == b.n_params and all(o % 4 == 0 for o in offsets)
    assert b.tail == (total + 3) // 4 * 4


def test_relayout_refusals_need_no_device(hip_lib):
    """The argument checks of ``moss_rows_relayout`` run on the host before anything is launched: made-up addresses are enough."""
    from moss_amd import _lib

    def block():
        a = _lib.RowsRelayoutArgs()
        a.rows_old, a.rows_app, a.rows_new, a.map, a.num_tensors = 8, 0, 8, 0x30000, 1
        d = a.tensors[0]
        d.src, d.dst, d.width, d.pad_after, d.use_map = 0x10000, 0x20000, 4, 0, 1
        return a

    def refused(a, code, *words):
        rc = hip_lib.moss_rows_relayout(None if a is None else ctypes.addressof(a), None)
        msg = hip_lib.moss_last_error().decode()
        assert rc == code and msg.startswith("moss_rows_relayout:") and all(w in msg for w in words), (rc, msg)
    refused(None, -1, "null argument block")
    a = block(); a.tensors[0].src = None
    refused(a, -1, "tensors[0].src")
    a = block(); a.tensors[0].dst = 0x10000 + 64
    refused(a, -1, "tensors[0].dst", "overlaps", "tensors[0].src")
    a = block(); a.tensors[0].dst = 0x30000 - 64                             # the last 16 floats of dst lie over the map
    refused(a, -1, "tensors[0].dst", "overlaps", "map")
    a = block(); a.rows_new = 2 ** 26; a.tensors[0].width = 48
    refused(a, -5, "tensors[0].width", "2^31")
    a = block(); a.num_tensors = _lib.ROWS_MAX_TENSORS + 1
    refused(a, -5, "num_tensors")
    a = block(); a.rows_app = 2; a.rows_new = 10
    refused(a, -1, "tensors[0].app")
