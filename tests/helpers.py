"""Shared test plumbing: run the CPU oracle and the HIP library on the same inputs and expose both in the
reference's own terms (GeometryState / BinningState / ImageState fields), so every stage can be compared."""
from __future__ import annotations

import contextlib
from types import SimpleNamespace

import numpy as np
import torch

from oracle import oracle


def inputs_of(scene, mode="scale_rot", degree=None, colors=False, bg=None):
    """Select the op's input mode like gaussian_renderer/__init__.py:85-109 does.
    mode: 'scale_rot' (scales+rotations), 'precomp' (cov3D_precomp) or 'lbs' (scales+rotations+per-Gaussian 3x3 transforms applied
    inside the op: the n2 extension).  colors=True feeds colours instead of SHs."""
    d = SimpleNamespace()
    d.P = scene.means3D.shape[0]
    d.means3D = scene.means3D.float().contiguous()
    d.opacities = scene.opacities.float().contiguous()
    d.scale_modifier = 1.0
    d.transforms = None
    if mode == "lbs":
        d.scales, d.rotations, d.cov3D_precomp = scene.scales.float().contiguous(), scene.rotations.float().contiguous(), None
        d.transforms = scene.transforms.float().contiguous()
    elif mode == "scale_rot":
        d.scales, d.rotations, d.cov3D_precomp = scene.scales.float().contiguous(), scene.rotations.float().contiguous(), None
    else:
        d.scales, d.rotations, d.cov3D_precomp = None, None, scene.cov3D_precomp.float().contiguous()
    d.degree = scene.sh_degree if degree is None else degree
    if colors:
        g = torch.Generator().manual_seed(11)
        d.colors_precomp, d.shs = torch.rand(d.P, 3, generator=g), None
    else:
        d.colors_precomp, d.shs = None, scene.shs.float().contiguous()
    d.bg = scene.bg.float() if bg is None else torch.tensor(bg, dtype=torch.float32)
    c = scene.camera
    d.cam = c
    d.W, d.H = c.W, c.H
    return d


def oracle_forward(d, det_exp=False):
    """det_exp: the blend evaluates exp() with the deterministic expf the kernels' EXACT-MATH mode uses (oracle.det_exp)."""
    c = d.cam
    with oracle.det_exp(det_exp):
        return _oracle_forward(d, c)


def _oracle_forward(d, c):
    return oracle.forward(d.bg.numpy(), d.means3D.numpy(), _np(d.colors_precomp), d.opacities.numpy(), _np(d.scales),
                          _np(d.rotations), d.scale_modifier, _np(d.cov3D_precomp), c.viewmatrix.numpy(), c.projmatrix.numpy(),
                          c.tanfovx, c.tanfovy, c.H, c.W, _np(d.shs), d.degree, c.campos.numpy(), transforms=_np(d.transforms))


def oracle_backward(d, fw, dc, dd, da, f32_accumulators=False, sum_noise_ulps=0.0, noise_seed=0, det_exp=False):
    c = d.cam
    with oracle.det_exp(det_exp):
        return _oracle_backward(d, c, fw, dc, dd, da, f32_accumulators, sum_noise_ulps, noise_seed)


def _oracle_backward(d, c, fw, dc, dd, da, f32_accumulators, sum_noise_ulps, noise_seed):
    return oracle.backward(fw, d.bg.numpy(), d.means3D.numpy(), _np(d.colors_precomp), _np(d.scales), _np(d.rotations),
                           d.scale_modifier, _np(d.cov3D_precomp), c.viewmatrix.numpy(), c.projmatrix.numpy(), c.tanfovx,
                           c.tanfovy, _np(dc), _np(dd), _np(da), _np(d.shs), d.degree, c.campos.numpy(), transforms=_np(d.transforms),
                           f32_accumulators=f32_accumulators, sum_noise_ulps=sum_noise_ulps, noise_seed=noise_seed)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _dev(t, device):
    return torch.Tensor([]) if t is None else t.to(device)


def hip_forward(d, device, debug=False, prefiltered=False):
    """Call the drop-in `_C.rasterize_gaussians` and export its opaque buffers in reference terms."""
    from moss_amd.diff_gaussian_rasterization import _C
    c = d.cam
    t = SimpleNamespace()
    t.args = dict(bg=d.bg.to(device), means3D=d.means3D.to(device), colors=_dev(d.colors_precomp, device),
                  opacity=d.opacities.to(device), scales=_dev(d.scales, device), rotations=_dev(d.rotations, device),
                  cov3D=_dev(d.cov3D_precomp, device), view=c.viewmatrix.to(device), proj=c.projmatrix.to(device),
                  sh=_dev(d.shs, device), campos=c.campos.to(device),
                  transforms=None if getattr(d, "transforms", None) is None else d.transforms.to(device))
    a = t.args
    (t.R, t.color, t.depth, t.alpha, t.radii, t.geom, t.binning, t.img) = _C.rasterize_gaussians(
        a["bg"], a["means3D"], a["colors"], a["opacity"], a["scales"], a["rotations"], d.scale_modifier, a["cov3D"],
        a["view"], a["proj"], c.tanfovx, c.tanfovy, c.H, c.W, a["sh"], d.degree, a["campos"], prefiltered, debug,
        **({} if a["transforms"] is None else {"transforms": a["transforms"]}))
    return t


def hip_export(d, t, device):
    """GeometryState / BinningState / ImageState views of the HIP buffers (numpy)."""
    L = _lib()
    P, R, W, H = d.P, t.R, d.W, d.H
    e = SimpleNamespace()
    f32 = dict(dtype=torch.float32, device=device)
    depths = torch.zeros(P, **f32); means2D = torch.zeros(P, 2, **f32); conic = torch.zeros(P, 4, **f32)
    rgb = torch.zeros(P, 3, **f32); tiles = torch.zeros(P, dtype=torch.int32, device=device)
    clamped = torch.zeros(P, 3, dtype=torch.uint8, device=device); cov3D = torch.zeros(P, 6, **f32)
    stream = torch.cuda.current_stream(device).cuda_stream
    rc = L.moss_raster_export_geometry(t.geom.data_ptr(), P, depths.data_ptr(), means2D.data_ptr(), conic.data_ptr(),
                                       rgb.data_ptr(), tiles.data_ptr(), clamped.data_ptr(), cov3D.data_ptr(), stream)
    assert rc == 0
    gx, gy = oracle.tile_grid(W, H)
    keys = torch.zeros(max(R, 1), dtype=torch.int64, device=device)
    plist = torch.zeros(max(R, 1), dtype=torch.int32, device=device)
    ranges = torch.zeros(gx * gy, 2, dtype=torch.int32, device=device)
    final_T = torch.zeros(W * H, **f32); n_contrib = torch.zeros(W * H, dtype=torch.int32, device=device)
    rc = L.moss_raster_export_binning(t.geom.data_ptr(), t.binning.data_ptr(), t.img.data_ptr(), P, R, W, H,
                                      keys.data_ptr(), plist.data_ptr(), ranges.data_ptr(), final_T.data_ptr(),
                                      n_contrib.data_ptr(), stream)
    assert rc == 0
    torch.cuda.synchronize(device)
    e.depths = depths.cpu().numpy(); e.means2D = means2D.cpu().numpy(); e.conic_opacity = conic.cpu().numpy()
    e.rgb = rgb.cpu().numpy(); e.tiles_touched = tiles.cpu().numpy().view(np.uint32); e.clamped = clamped.cpu().numpy()
    e.cov3D = cov3D.cpu().numpy()
    e.point_list_keys = keys.cpu().numpy().view(np.uint64)[:R]; e.point_list = plist.cpu().numpy().view(np.uint32)[:R]
    e.ranges = ranges.cpu().numpy().view(np.uint32); e.final_T = final_T.cpu().numpy()
    e.n_contrib = n_contrib.cpu().numpy().view(np.uint32)
    e.radii = t.radii.cpu().numpy(); e.color = t.color.cpu().numpy(); e.depth = t.depth.cpu().numpy(); e.alpha = t.alpha.cpu().numpy()
    return e


def hip_backward(d, t, dc, dd, da, device, debug=False):
    from moss_amd.diff_gaussian_rasterization import _C
    c = d.cam
    a = t.args
    out = _C.rasterize_gaussians_backward(
        a["bg"], a["means3D"], t.radii, a["colors"], a["scales"], a["rotations"], d.scale_modifier, a["cov3D"], a["view"],
        a["proj"], c.tanfovx, c.tanfovy, dc.to(device), dd.to(device), da.to(device), a["sh"], d.degree, a["campos"],
        t.geom, t.R, t.binning, t.img, t.alpha, debug, **({} if a["transforms"] is None else {"transforms": a["transforms"]}))
    names = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations",
             "dL_dtransforms"]
    return SimpleNamespace(**{n: o for n, o in zip(names, out)})


def _lib():
    from moss_amd import _lib as m
    return m.lib()


def c_layout(tmp_path, cname, fields, cc="gcc", extra=()):
    """``[sizeof(cname), offsetof(cname, f) for f in fields] + extra`` as a host C compile of include/moss_raster.h sees them.  A field
    that ctypes spells with a trailing underscore because the name is a Python keyword (``in_``) is the C field without it; ``extra``:
    further integer expressions (``"MOSS_ROWS_MAX_TENSORS"``, ``"offsetof(moss_rows_tensor, width)"``); ``cc``: a compiler command."""
    import os
    import subprocess
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    exprs = ["sizeof(%s)" % cname] + ["offsetof(%s, %s)" % (cname, f.rstrip("_")) for f in fields] + list(extra)
    src = tmp_path / ("layout_%s.c" % cname)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "moss_raster.h"\nint main(void) {\n'
                   + "".join('    printf(" %%zu", (size_t)(%s));\n' % e for e in exprs) + "    return 0;\n}\n")
    exe = tmp_path / ("layout_%s" % cname)
    subprocess.run(cc.split() + ["-I", include, str(src), "-o", str(exe)], check=True)
    return [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]


def ctypes_layout(cls):
    """``[sizeof, every field's offset]`` of a ``ctypes.Structure``: what :func:`c_layout` of its C struct and fields must equal."""
    import ctypes
    return [ctypes.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_]


def image_grads(H, W, seed=5, zero_depth=False):
    g = torch.Generator().manual_seed(seed)
    dc = torch.randn(3, H, W, generator=g)
    dd = torch.zeros(1, H, W) if zero_depth else torch.randn(1, H, W, generator=g)
    da = torch.randn(1, H, W, generator=g)
    return dc, dd, da


def rel_err(a, b):
    """max |a-b| relative to the largest magnitude of the reference b (scale-aware infinity norm)."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30)) if a.size else 0.0


def replace_forward_state(fw, e):
    """Oracle forward namespace whose image state (final_T, n_contrib) is taken from the HIP forward, so that the
    backward arithmetic can be compared in isolation from forward threshold decisions."""
    import copy
    f2 = copy.copy(fw)
    f2.final_T = e.final_T.copy(); f2.n_contrib = e.n_contrib.copy()
    return f2


def oracle_forward64(d, fw32):
    """The float64 ADJUDICATOR over the float32 oracle's tile lists (oracle.forward(f64=True))."""
    c = d.cam
    return oracle.forward(d.bg.numpy(), d.means3D.numpy(), _np(d.colors_precomp), d.opacities.numpy(), _np(d.scales),
                          _np(d.rotations), d.scale_modifier, _np(d.cov3D_precomp), c.viewmatrix.numpy(), c.projmatrix.numpy(),
                          c.tanfovx, c.tanfovy, c.H, c.W, _np(d.shs), d.degree, c.campos.numpy(), transforms=_np(d.transforms),
                          f64=True, binning_from=fw32)


def oracle_gradient_scales(d, fw, dc, dd, da):
    """Per-element error scales (sum of absolute contributions) of every gradient, see oracle.gradient_scales."""
    c = d.cam
    return oracle.gradient_scales(fw, d.bg.numpy(), d.means3D.numpy(), _np(d.colors_precomp), _np(d.scales), _np(d.rotations),
                                  d.scale_modifier, _np(d.cov3D_precomp), c.viewmatrix.numpy(), c.projmatrix.numpy(), c.tanfovx,
                                  c.tanfovy, _np(dc), _np(dd), _np(da), _np(d.shs), d.degree, c.campos.numpy(), transforms=_np(d.transforms))


def stable_mask(d, *fws, thr=1e-4):
    """(H,W) float mask of the pixels whose every decision (power > 0, alpha < 1/255, T < 1e-4) is further than `thr` (relative)
    from its threshold in ALL the given oracle forwards: there every implementation takes the same branches, so differences are
    arithmetic only.  Multiply the incoming image gradients by it to compare backward passes end to end."""
    ok = np.ones(d.H * d.W, bool)
    for fw in fws:
        ok &= np.asarray(fw.margin) > thr
    return torch.from_numpy(ok.reshape(d.H, d.W).astype(np.float32))


def cosine_gap(a, b):
    """1 - cos(a, b) over the whole tensor (float64)."""
    a = np.asarray(a, dtype=np.float64).ravel(); b = np.asarray(b, dtype=np.float64).ravel()
    den = np.sqrt((a * a).sum() * (b * b).sum())
    return 0.0 if den == 0.0 else float(1.0 - (a * b).sum() / den)


def scaled_err(a, b, scale):
    """max over elements of |a - b| / scale, over the elements whose scale is positive; elements with a zero scale (no pixel
    contributes to them) must agree exactly."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64); s = np.asarray(scale, dtype=np.float64).reshape(a.shape)
    pos = s > 0
    dead = float(np.abs(a - b)[~pos].max()) if (~pos).any() else 0.0
    live = float((np.abs(a - b)[pos] / s[pos]).max()) if pos.any() else 0.0
    return live, dead


U32 = 2.0 ** -24      # unit roundoff of float32


def adjudication_excess(got, refs32, ref64, scale, factor=2.0):
    """The float64 adjudication of one gradient tensor, element by element, in units of the element's contribution mass:

        |got - f64|  <=  factor * E32 * mass  +  excess * mass

    E32 = the worst distance from float64, in mass units, of the float32 restatements in ``refs32`` on this tensor: the oracle with
    double accumulators (the centre of the reference's distribution) and the oracle with FLOAT32 accumulators added in loop order
    (``f32_accumulators=True``: one of the orders the reference's atomicAdd can take, i.e. the reference's arithmetic including the
    rounding of its atomics -- what an image-covering Gaussian with 10^4 contributing pixels actually gets).  Returns
    (largest excess, E32, largest |got - f64| / mass); elements without mass must agree exactly (asserted)."""
    a = np.asarray(got, dtype=np.float64); b64 = np.asarray(ref64, dtype=np.float64)
    s = np.asarray(scale, dtype=np.float64).reshape(a.shape)
    pos = s > 0
    assert not np.abs(a - b64)[~pos].any(), "an element that nothing contributes to is not exactly zero"
    if not pos.any():
        return 0.0, 0.0, 0.0
    e32 = max(float((np.abs(np.asarray(r, dtype=np.float64) - b64)[pos] / s[pos]).max()) for r in refs32)
    err = np.abs(a - b64)[pos] / s[pos]
    return float(err.max() - factor * e32), e32, float(err.max())


# ---- ONE parity rule for the gradients (round 4) -----------------------------------------------------------------------------------
# "Within a stated fp32 tolerance of the reference" needs a tolerance that follows from the INPUTS, per element, and holds for every
# scene -- the BASELINE configurations and the random ones alike, with no list of exceptions.  What a float32 implementation of the
# reference's algorithm is entitled to has two parts, and both are measured rather than estimated:
#   * SUMMATION: an element is a sum over pixels of terms that may cancel; any float32 order of that sum errs in proportion to the
#     sum of the ABSOLUTE terms, the element's contribution mass (oracle.gradient_scales);
#   * the NOISE FLOOR OF THE REFERENCE'S OWN ARITHMETIC at that element.  The per-Gaussian chain conic -> cov2D -> cov3D -> scale /
#     rotation / transform is riddled with cancellations (a 300:1 needle seen end-on: the scale gradient of its long axis is a
#     difference of terms 10^3 times its size, several times over).  How much float32 rounding moves the result there is measured by
#     stochastic arithmetic: the float32 restatement of the reference (oracle/moss_oracle.c: its statements, its operation order) is
#     run PROBES times on inputs moved by -1 / 0 / +1 float32 ulp at random -- every internal rounding then falls differently -- with
#     double and with float32 accumulators, over the same forward state; `spread` is the largest distance of those runs from the
#     float64 result, element by element.  (The float64 oracle's own response to the same one-ulp perturbations -- the conditioning
#     of the exact function -- is part of it by construction.)
# The rule, for EVERY element of every gradient tensor:      |hip - f64|  <=  RULE_K * (spread + RULE_EPS * mass)
# i.e. the kernels are never further from float64 than RULE_K times what the reference's arithmetic itself scatters by.
RULE_EPS = 16 * U32          # the summation share: sixteen unit roundoffs of the contribution mass (lists of 10^2-10^3 terms, summed in trees)
RULE_K = 8.0             # measured over 4 088 scenes (profiles/r04_fuzz_rule_*.log): median 0.5, 99th percentile 1.8, worst 6.1
RULE_K_BASELINE = 4.0    # the BASELINE configurations (cfg1-3, cfg5: well-conditioned Gaussians) are held to HALF of it: their measured worst
                         # is 1.01 (profiles/r04_parity_report.json); the 8 above is for random scenes with 50-600:1 needles
RULE_PROBES = 6


def _ulp_perturbed(a, rng):
    """float32 array -> every element moved by -1, 0 or +1 float32 ulp at random."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    step = rng.integers(-1, 2, size=a.shape)
    up = np.nextafter(a, np.float32(np.inf)); dn = np.nextafter(a, np.float32(-np.inf))
    return np.where(step > 0, up, np.where(step < 0, dn, a)).astype(np.float32)


RULE_NAMES = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations", "dL_dtransforms"]


def reference_noise_floor(d, fw, fw64, dc, dd, da, probes=RULE_PROBES, seed=0):
    """({name: spread}, float64 gradients): the float32 restatement run on one-ulp perturbed inputs `probes` times (alternating double /
    float32 accumulators; probe 0 is the unperturbed run), each compared with the float64 oracle on the UNPERTURBED inputs."""
    import copy
    c = d.cam
    ref64 = oracle_backward(d, fw64, dc, dd, da)
    spread = {n: np.zeros(np.asarray(getattr(ref64, n)).shape, np.float64) for n in RULE_NAMES}
    for s in range(probes):
        rng = np.random.default_rng(1000 * seed + s)
        P = (lambda a: None if a is None else np.ascontiguousarray(_np(a))) if s == 0 else (lambda a: None if a is None else _ulp_perturbed(_np(a), rng))
        fwp = copy.copy(fw)
        if s > 0:
            # the forward's per-Gaussian results the backward reads: rounded differently by every float32 implementation
            for name in ("cov3D", "means2D", "conic_opacity", "rgb", "depths"):
                v = getattr(fw, name, None)
                if v is not None and np.asarray(v).size:
                    setattr(fwp, name, _ulp_perturbed(v, rng))
        g = oracle.backward(fwp, d.bg.numpy(), P(d.means3D), _np(d.colors_precomp), P(d.scales), P(d.rotations), d.scale_modifier,
                            P(d.cov3D_precomp), P(c.viewmatrix), P(c.projmatrix), c.tanfovx, c.tanfovy, _np(dc), _np(dd), _np(da),
                            P(d.shs), d.degree, P(c.campos), transforms=P(d.transforms), f32_accumulators=bool(s & 1))
        for n in RULE_NAMES:
            spread[n] = np.maximum(spread[n], np.abs(np.asarray(getattr(g, n), np.float64) - np.asarray(getattr(ref64, n), np.float64)))
    return spread, ref64


def single_rule_ratio(got, ref64, mass, spread):
    """max over the elements of |got - ref64| / (spread + RULE_EPS * mass) -- the rule holds iff this is <= RULE_K -- plus the index of
    the worst element.  Elements with neither mass nor spread (nothing contributes to them) must agree exactly (asserted)."""
    a = np.asarray(got, np.float64); b = np.asarray(ref64, np.float64)
    den = np.asarray(spread, np.float64).reshape(a.shape) + RULE_EPS * np.asarray(mass, np.float64).reshape(a.shape)
    err = np.abs(a - b)
    pos = den > 0
    assert not err[~pos].any(), "an element that nothing contributes to is not exactly zero"
    if not pos.any():
        return 0.0, -1
    r = np.zeros_like(err); r[pos] = err[pos] / den[pos]
    k = int(np.argmax(r))
    return float(r.reshape(-1)[k]), k


# ---- poisoned allocator memory ---------------------------------------------------------------------------------------------------
# The ops take their outputs and scratch from torch.empty on the promise that the kernels write every element before anything reads
# it.  Early in a process the caching allocator hands out fresh pages from the driver -- zeros, the one content that hides a missing
# write.  `poisoned_allocator` makes every block the allocator can hand out hold a chosen byte instead.
POISON_FILLS = (0x00, 0xFF, 0x3C)      # benign | float NaN, int -1, bool true | float ~0.0115, a large positive int (passes x > 0 guards)
POISON_CANARIES = (512, 300 << 10, 3 << 20, 40 << 20)


class Poison:
    """What `poisoned_allocator` yields: the seeded address ranges and the allocator's segment count after seeding."""

    def __init__(self, device, byte, ranges, segments):
        self.device, self.byte, self.segments = device, byte, segments
        self.ranges = []                  # (neighbours merged: freed blocks coalesce, and a later allocation may straddle two of them)
        for lo, hi in sorted(ranges):
            if self.ranges and self.ranges[-1][1] == lo:
                self.ranges[-1] = (self.ranges[-1][0], hi)
            else:
                self.ranges.append((lo, hi))

    def owns(self, t):
        lo = t.data_ptr(); hi = lo + t.numel() * t.element_size()
        return any(a <= lo and hi <= b for a, b in self.ranges)

    def assert_owns(self, *tensors):
        """Every given tensor (None and empty ones excepted) was allocated out of the poisoned blocks."""
        for i, t in enumerate(tensors):
            if t is not None and t.numel():
                assert t.is_cuda and self.owns(t), f"tensor {i} ({tuple(t.shape)}, {t.dtype}) does not lie in poisoned memory"


def _free_blocks(device):
    """(size, is_small_pool) of every cached free block of the default pool on the default stream of `device`."""
    out = []
    for seg in torch.cuda.memory_snapshot():
        if seg["device"] != device.index or seg.get("stream", 0) != 0 or tuple(seg.get("segment_pool_id", (0, 0))) != (0, 0):
            continue
        for b in seg["blocks"]:
            if b["state"] == "inactive":
                out.append((int(b["size"]), seg["segment_type"] == "small"))
    return out


@contextlib.contextmanager
def poisoned_allocator(device, byte, large_bytes=256 << 20, small_segments=32):
    """Inside the block, torch's caching allocator hands out only memory filled with `byte` (on `device`, default stream, eager calls:
    captured graphs allocate from private pools and are out of scope).  Create the op's inputs BEFORE entering, so they lie outside
    the poison; move results to the CPU and drop the device tensors before the next use (the cache then holds the last run's data).

    Seeding: synchronise, empty_cache(); one uint8 block of `large_bytes`; 2 x `small_segments` tensors of 1 MiB (the small pool's
    limit; two fill one of its 2 MiB segments); then a sweep that claims every free block the cache still holds -- empty_cache()
    returns only wholly free segments to the driver, so the free remainders of the segments that hold live tensors (the op's inputs,
    other tests' module state) are still there, unpoisoned, and being the smallest blocks that fit they would be handed out FIRST.
    The sweep reads them from torch.cuda.memory_snapshot() and requests each one's exact size (a small-pool block larger than 1 MiB
    in pieces of 1 MiB, since a larger request would go to the large pool) until none is left.  Everything held is filled with
    `byte` and freed without emptying the cache.

    Found on ROCm torch 2.10 / MI355X: the allocator behaves as upstream's (small pool up to 1 MiB in 2 MiB segments, larger requests
    split off the one large block; no pool limit or split rule got in the way), and all four canaries, the segment count and the
    pointer check hold with this seeding -- also late in a suite run, when hundreds of earlier tests have left live tensors and
    fragmented segments behind.  The one surprise: freed neighbours coalesce, so an allocation may straddle two seeded tensors;
    `Poison` merges adjacent ranges.

    The helper shows that it worked, and fails otherwise:
      * canaries: torch.empty of 512 B, 300 KiB, 3 MiB and 40 MiB must come back all-`byte`; they are read through a device-to-host
        copy (a comparison on the device would allocate its result out of the poison and dirty it) and freed unwritten;
      * on exit memory_stats()["segment.all.allocated"] must equal its value after seeding: no fresh segment from the driver, so
        everything allocated inside came out of poisoned blocks;
      * `Poison.assert_owns(*tensors)`: the tensors an op returns lie inside the seeded ranges."""
    assert torch.cuda.current_stream(device).cuda_stream == 0, "poisoned_allocator seeds the default stream's blocks"
    torch.cuda.synchronize(device)
    torch.cuda.empty_cache()
    held = [torch.empty(large_bytes, dtype=torch.uint8, device=device)]
    held += [torch.empty(1 << 20, dtype=torch.uint8, device=device) for _ in range(2 * small_segments)]
    for _ in range(16):
        free = sorted(_free_blocks(device), reverse=True)
        if not free:
            break
        held += [torch.empty(min(size, 1 << 20) if small else size, dtype=torch.uint8, device=device) for size, small in free]
    assert not _free_blocks(device), "poisoned_allocator: free blocks are left that the sweep could not claim"
    for t in held:
        t.fill_(byte)
    ranges = [(t.data_ptr(), t.data_ptr() + t.numel()) for t in held]
    torch.cuda.synchronize(device)
    del held, t
    segments = torch.cuda.memory_stats(device)["segment.all.allocated"]
    poison = Poison(device, byte, ranges, segments)
    for n in POISON_CANARIES:
        c = torch.empty(n, dtype=torch.uint8, device=device)
        assert poison.owns(c), f"poison did not take: a {n}-byte request came from outside the seeded ranges"
        host = c.cpu().numpy()
        del c
        assert host.min() == byte == host.max(), f"poison did not take: a {n}-byte request is not all 0x{byte:02X}"
    assert torch.cuda.memory_stats(device)["segment.all.allocated"] == segments, "poison did not take: a canary needed a fresh segment"
    yield poison
    torch.cuda.synchronize(device)
    got = torch.cuda.memory_stats(device)["segment.all.allocated"]
    assert got == segments, f"{got - segments} fresh segment(s) came from the driver inside the poisoned block: not all memory was poisoned"
