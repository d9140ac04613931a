"""The forward preprocess kernel after its reordering (one load round trip; part A = geometry, histogram, bucket reservations;
part B = colour behind them; SH staged per wave): every output is still the parent's, bit for bit.

Bars, as in tests/test_gpu_parity.py: radii, tiles_touched, depth bits, means2D, conic_opacity, rgb, clamped, cov3D of the visible
Gaussians, the SORTED keys, ids and per-tile ranges are BIT-EXACT -- the synchronous forward against the CPU oracle, and the
asynchronous (capacity-bounded, scatter-mode) forward against the synchronous one.  Slot order inside a key bucket is arbitrary, so
keys are compared after the sort.  Shapes are the smallest at which the reordering can go wrong (partial waves and blocks, more than
one reservation batch, no LDS histogram, a wave-walked rectangle, nothing to render, the unstaged SH paths, an outgrown bucket).

Raw parameters: the oracle has no raw mode, and a host-side exp / sigmoid is not the device's expf bit for bit.  The headline's form
(lbs transforms, raw flags 7, RAW_POSE with a translation) is therefore checked in two steps: with activated parameters, lbs
transforms and RAW_POSE + translation against the oracle, bit-exact (posing is plain float32 multiply-add, reproduced in numpy with
one rounding per operation); then with the raw flags added, asynchronous == synchronous bit for bit on every field above."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from moss_amd import scenes
from tests import helpers as hp
from tests import test_gpu_parity as tp

pytestmark = pytest.mark.gpu

GEOM_FIELDS = ("radii", "tiles_touched", "depths", "means2D", "conic_opacity", "rgb", "clamped")
BIN_FIELDS = ("point_list_keys", "point_list", "ranges")


@pytest.fixture
def async_mode():
    import moss_amd.diff_gaussian_rasterization as dgr
    yield dgr
    dgr.set_async(False)


def _scene(P, W, H, seed=7, spread=False, scale=1.0):
    """config1's Gaussians; spread=True: a camera whose focal length lays them over the whole image (config1's own covers ~60 px)."""
    s = scenes.config1(P=P, W=W, H=H, seed=seed)
    if spread:
        f = 2.4 * max(W, H)
        s.camera = scenes.make_camera(W, H, f, f, W / 2, H / 2, np.eye(3), np.array([0.0, 0.0, 3.0]))
    if scale != 1.0:
        s.scales = s.scales * scale
        s.cov3D_precomp = scenes.covariance_precomp(s.scales, s.rotations, 1.0, s.transforms)
    return s


def _forward(d, gpu, raw_flags=0, translation=None):
    """hp.hip_forward with the raw flags and the translation it has no argument for; the same namespace, so hp.hip_export takes it."""
    from moss_amd.diff_gaussian_rasterization import _C
    t = SimpleNamespace()
    c = d.cam
    dev = lambda x: torch.Tensor([]) if x is None else x.to(gpu)
    t.args = dict(bg=d.bg.to(gpu), means3D=d.means3D.to(gpu), colors=dev(d.colors_precomp), opacity=d.opacities.to(gpu),
                  scales=dev(d.scales), rotations=dev(d.rotations), cov3D=dev(d.cov3D_precomp), view=c.viewmatrix.to(gpu),
                  proj=c.projmatrix.to(gpu), sh=dev(d.shs), campos=c.campos.to(gpu),
                  transforms=None if getattr(d, "transforms", None) is None else d.transforms.to(gpu))
    a = t.args
    (t.R, t.color, t.depth, t.alpha, t.radii, t.geom, t.binning, t.img) = _C.rasterize_gaussians(
        a["bg"], a["means3D"], a["colors"], a["opacity"], a["scales"], a["rotations"], d.scale_modifier, a["cov3D"], a["view"], a["proj"],
        c.tanfovx, c.tanfovy, c.H, c.W, a["sh"], d.degree, a["campos"], False, False, transforms=a["transforms"], raw_flags=raw_flags,
        translation=None if translation is None else translation.to(gpu))
    return t


def _assert_same_export(a, b, d, what):
    for n in GEOM_FIELDS + BIN_FIELDS + ("n_contrib", "final_T", "color", "depth", "alpha"):
        x, y = getattr(a, n), getattr(b, n)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, n)
    if d.cov3D_precomp is None:
        vis = a.radii > 0
        assert a.cov3D[vis].tobytes() == b.cov3D[vis].tobytes(), (what, "cov3D")


def _sync_and_async(d, gpu, dgr, raw_flags=0, translation=None):
    """The synchronous forward, then the asynchronous one (scatter mode where the tile histogram fits the LDS) on a context that learned
    its capacity from a synchronous call: both exported; the asynchronous frame's instance count is the synchronous one's."""
    ts = _forward(d, gpu, raw_flags, translation)
    es = hp.hip_export(d, ts, gpu)
    dgr.set_async(True)
    _forward(d, gpu, raw_flags, translation)                   # synchronous: learns the capacity
    ta = _forward(d, gpu, raw_flags, translation)              # asynchronous
    ta2 = _forward(d, gpu, raw_flags, translation)             # ... and again on the re-zeroed frame state
    dgr.check_async_status()
    fs = dgr._C.ASYNC.frame_state
    assert fs is not None and int(fs.count_nonzero()) == 0
    for t in (ta, ta2):
        t.R = ts.R
    ea, ea2 = hp.hip_export(d, ta, gpu), hp.hip_export(d, ta2, gpu)
    dgr.set_async(False)
    _assert_same_export(es, ea, d, "async vs sync")
    _assert_same_export(es, ea2, d, "second async vs sync")
    return ts, es, ta, ea


def _against_oracle(d, es, fw):
    assert np.array_equal(es.radii, fw.radii) and np.array_equal(es.tiles_touched, fw.tiles_touched)
    np.testing.assert_array_equal(es.depths.view(np.uint32), fw.depths.view(np.uint32))
    np.testing.assert_array_equal(es.means2D, fw.means2D)
    np.testing.assert_array_equal(es.conic_opacity, fw.conic_opacity)
    if d.colors_precomp is None:
        np.testing.assert_array_equal(es.rgb, fw.rgb)
        np.testing.assert_array_equal(es.clamped, fw.clamped)
    if d.cov3D_precomp is None:
        vis = fw.radii > 0
        np.testing.assert_array_equal(es.cov3D[vis], fw.cov3D[vis])
    np.testing.assert_array_equal(es.point_list_keys, fw.point_list_keys)
    np.testing.assert_array_equal(es.point_list, fw.point_list)
    np.testing.assert_array_equal(es.ranges, fw.ranges)


def _three_way(d, gpu, dgr):
    fw = hp.oracle_forward(d)
    ts, es, ta, ea = _sync_and_async(d, gpu, dgr)
    assert ts.R == fw.num_rendered
    _against_oracle(d, es, fw)
    return fw, ts, es


def _posed(T, x, t):
    """p = T x + t as the kernel evaluates it: float32, one rounding per operation, left to right."""
    Tn, xn, tn = T.numpy(), x.numpy(), t.numpy()
    p = np.empty_like(xn)
    for r in range(3):
        p[:, r] = ((Tn[:, r, 0] * xn[:, 0] + Tn[:, r, 1] * xn[:, 1]) + Tn[:, r, 2] * xn[:, 2]) + tn[:, r]
    assert p.dtype == np.float32
    return torch.from_numpy(p)


# ---- partial waves and blocks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 257, 600])
def test_partial_waves_and_blocks_scale_rot(gpu, hip_lib, async_mode, P):
    _three_way(hp.inputs_of(_scene(P, 64, 64), "scale_rot"), gpu, async_mode)


@pytest.mark.parametrize("P", [1, 63, 257, 600])
def test_partial_waves_and_blocks_headline_form(gpu, hip_lib, async_mode, P):
    """lbs transforms, RAW_POSE with a translation: against the oracle on activated parameters; then with raw parameters (flags 7) as
    well, asynchronous == synchronous."""
    from moss_amd.diff_gaussian_rasterization import _C
    s = _scene(P, 64, 64)
    g = torch.Generator().manual_seed(31)
    tl = (0.05 * torch.randn(P, 3, generator=g)).float()
    d = hp.inputs_of(s, "lbs")
    d_or = hp.inputs_of(s, "lbs")
    d_or.means3D = _posed(d.transforms, d.means3D, tl)
    fw = hp.oracle_forward(d_or)
    ts, es, ta, ea = _sync_and_async(d, gpu, async_mode, raw_flags=_C.RAW_POSE, translation=tl)
    assert ts.R == fw.num_rendered
    _against_oracle(d, es, fw)
    # raw parameters: logits, log-scales, unnormalised quaternions
    d_raw = hp.inputs_of(s, "lbs")
    d_raw.opacities = torch.logit(d.opacities.clamp(1e-4, 1 - 1e-4)).float()
    d_raw.scales = torch.log(d.scales).float()
    d_raw.rotations = (d.rotations * (0.3 + 2.0 * torch.rand(P, 1, generator=g))).float()
    _sync_and_async(d_raw, gpu, async_mode, raw_flags=7 | _C.RAW_POSE, translation=tl)


# ---- more than 1 024 tiles, still an LDS histogram: one reservation batch consumed at once, the last one deferred ----------------------
def test_two_reservation_batches(gpu, hip_lib, async_mode):
    d = hp.inputs_of(_scene(2000, 528, 520, spread=True, scale=0.25), "scale_rot")
    fw, ts, es = _three_way(d, gpu, async_mode)
    gx = (d.W + 15) // 16
    n = (fw.ranges[:, 1] - fw.ranges[:, 0]).astype(np.int64)
    assert gx * ((d.H + 15) // 16) == 33 * 33 and n[:1024].sum() > 0 and n[1024:].sum() > 0   # both batches reserve something


# ---- more than MAX_LDS_TILES tiles: global histogram atomics, no scatter mode -------------------------------------------------------------
def test_beyond_the_lds_histogram(gpu, hip_lib, async_mode):
    d = hp.inputs_of(_scene(500, 1456, 1456, spread=True, scale=0.1), "scale_rot")
    assert ((d.W + 15) // 16) * ((d.H + 15) // 16) > 8192
    _three_way(d, gpu, async_mode)


# ---- a rectangle walked by the whole wave -------------------------------------------------------------------------------------------------
def test_wave_walked_rectangle(gpu, hip_lib, async_mode):
    s = _scene(300, 256, 256, spread=True, scale=0.2)
    s.means3D[5] = torch.tensor([0.0, 0.0, 0.0]); s.scales[5] = torch.tensor([4.0, 4.0, 4.0])
    d = hp.inputs_of(s, "scale_rot")
    fw, ts, es = _three_way(d, gpu, async_mode)
    assert int(fw.tiles_touched[5]) == 16 * 16


# ---- nothing to render ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["behind_near_plane", "empty_rectangles"])
def test_nothing_to_render(gpu, hip_lib, async_mode, case):
    s = _scene(300, 64, 64)
    if case == "behind_near_plane":
        s.means3D[:, 2] = -5.0 - s.means3D[:, 2].abs()       # camera at z = -3 looking down +z: view depth <= 0.2
    else:
        s.means3D[:, 0] = 40.0 + s.means3D[:, 0]             # far off to the side: rectangles clip to nothing
    d = hp.inputs_of(s, "scale_rot", bg=[0.1, 0.2, 0.3])
    fw = hp.oracle_forward(d)
    assert fw.num_rendered == 0
    ts, es, ta, ea = _sync_and_async(d, gpu, async_mode)
    assert ts.R == 0 and not es.radii.any() and not es.tiles_touched.any()
    for t in (ts, ta):
        assert torch.equal(t.color.cpu(), d.bg[:, None, None].expand(3, d.H, d.W)) and float(t.alpha.abs().max()) == 0.0


# ---- the unstaged paths ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,degree", [(4, 1), (9, 2)])
def test_unstaged_small_sh_arrays(gpu, hip_lib, async_mode, M, degree):
    d = hp.inputs_of(_scene(600, 64, 64), "scale_rot", degree=degree)
    d.shs = d.shs[:, :M].contiguous()
    _three_way(d, gpu, async_mode)


def test_unstaged_colors_precomp(gpu, hip_lib, async_mode):
    _three_way(hp.inputs_of(_scene(600, 64, 64), "scale_rot", colors=True), gpu, async_mode)


def test_cov3d_precomp(gpu, hip_lib, async_mode):
    _three_way(hp.inputs_of(_scene(600, 64, 64), "precomp"), gpu, async_mode)


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_staged_sh_degrees(gpu, hip_lib, async_mode, degree):
    _three_way(hp.inputs_of(_scene(600, 64, 64), "scale_rot", degree=degree), gpu, async_mode)


# ---- a tile that outgrows its bucket ----------------------------------------------------------------------------------------------------------
def test_outgrown_bucket_drops_the_frame_as_before(gpu, hip_lib, async_mode):
    """600 Gaussians clustered on four tiles of a 512 x 512 image (1 024 tiles): 2 540 instances, the fullest tile holds 600.  A
    capacity just above the frame's instance count holds the frame as a whole, but a tile's key bucket is 36 keys per instance of
    capacity / tiles (binning.hip, bucket_key_stride) -- some 90 slots: the tile outgrows it.  The frame is dropped and reported as
    tests/test_gpu_ops.py::test_async_overflow_renders_nothing_and_is_reported expects of an overflow: background, zero alpha, radii
    as ever, the overflow raised with the needed capacity, the sticky dropped-frame word, a clean frame state, and the grown capacity
    renders the synchronous frame."""
    s = _scene(600, 512, 512)
    s.means3D = s.means3D * 0.2
    d = hp.inputs_of(s, "scale_rot", bg=[0.1, 0.2, 0.3])
    ts = _forward(d, gpu)
    es = hp.hip_export(d, ts, gpu)
    n = (es.ranges[:, 1].astype(np.int64) - es.ranges[:, 0])
    cap = ts.R + 64
    assert n.max() > 4 * (36 * cap // 1024)                    # one tile's list is several buckets long; the frame itself fits
    async_mode.set_async(True, capacity=cap)
    ta = _forward(d, gpu)
    assert torch.equal(ta.color.cpu(), d.bg[:, None, None].expand(3, d.H, d.W)) and float(ta.alpha.abs().max()) == 0.0
    assert torch.equal(ta.radii.cpu(), ts.radii.cpu())         # preprocess still ran
    with pytest.raises(async_mode.CapacityOverflow, match="needed") as exc:
        async_mode.check_async_status()
    assert exc.value.needed > cap
    cx = async_mode._C.ASYNC
    assert int(cx.frame_state.view(torch.int32)[async_mode._C.FRAME_STATE_DROPPED_WORD]) == 1
    assert cx.read_dropped_frames(reset=False) == 0 and cx.read_dropped_frames() == 0
    assert int(cx.frame_state.count_nonzero()) == 0 and cx.capacity > cap
    tb = _forward(d, gpu)                                      # the grown capacity fits
    async_mode.check_async_status()
    tb.R = ts.R
    _assert_same_export(es, hp.hip_export(d, tb, gpu), d, "after growing")


# ---- one backward: rec_offsets, rec_count and the fourth geo word still address the record pool ------------------------------------------------
def test_backward_on_the_600_gaussian_case(gpu, hip_lib):
    d = hp.inputs_of(_scene(600, 64, 64), "lbs")
    fw, t, e = tp._check_forward(d, gpu)
    tp._check_backward(d, gpu, fw, t, e)
