"""The asynchronous forward's tile sort (chunk_sort_kernel's self-scan path: chunks dealt to workgroups by size class, csrc/sort_deal.h;
step masks of the bitonic network as scalar literals) against the CPU oracle's sorted (key, id) lists and tile ranges, bit for bit, on
frames built so that the chunks are what the deal has to get right: only short chunks; tiles of two and three chunks beside empty and
one-entry tiles; many equal depths (ties go by id); a tile of exactly 1024 and one of exactly 1025 instances in a row of 65 tiles; and
frames of more than 1024 tiles, which run the kernel's other instantiation (up to 8 tiles per thread of the self-scan)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from moss_amd import scenes
from tests import helpers as hp

pytestmark = pytest.mark.gpu

TILE = 16


def _placed_scene(W, H, piles, seed, depths=None, spread=0):
    """Pin-point Gaussians (2-pixel radius: each touches exactly the tile it sits in) at chosen tiles: ``piles`` = {tile index: count};
    ``spread`` more at random pixels.  Camera at the origin looking down +z; depths in [2, 4], or drawn from ``depths``."""
    g = torch.Generator().manual_seed(seed)
    gx = (W + TILE - 1) // TILE
    fx = 140.0
    u, v = [], []
    for tile, n in piles.items():
        u.append((tile % gx) * TILE + 8.0 + (torch.rand(n, generator=g) * 6.0 - 3.0))
        v.append((tile // gx) * TILE + 8.0 + (torch.rand(n, generator=g) * 6.0 - 3.0))
    if spread:
        u.append(torch.rand(spread, generator=g) * W); v.append(torch.rand(spread, generator=g) * H)
    u, v = torch.cat(u), torch.cat(v)
    P = u.numel()
    perm = torch.randperm(P, generator=g)                     # (ids are not in tile order)
    u, v = u[perm], v[perm]
    if depths is None:
        z = 2.0 + 2.0 * torch.rand(P, generator=g)
    else:
        z = torch.tensor(depths, dtype=torch.float32)[torch.randint(len(depths), (P,), generator=g)]
    s = SimpleNamespace(name="placed", P=P, sh_degree=3)
    s.means3D = torch.stack([(u - W / 2) * z / fx, (v - H / 2) * z / fx, z], dim=1)
    s.scales = torch.full((P, 3), 1.0e-3)
    s.rotations = scenes._rand_quat(P, g)
    s.opacities = torch.sigmoid(torch.randn(P, 1, generator=g))
    s.shs = scenes._rand_sh(P, g)
    s.bg = torch.zeros(3)
    s.camera = scenes.make_camera(W, H, fx, fx, W / 2, H / 2)
    return s


def _shape(name):
    if name == "short_chunks":                               # 16 tiles, 300 Gaussians: every chunk is short
        return scenes.config1(P=300, W=64, H=64), None
    if name in ("piles", "piles_equal_depths"):              # 64 tiles: three-, two-chunk, one-chunk, one-entry and empty tiles
        piles = {9: 2500, 10: 2200, 27: 1300, 0: 1, 63: 1, 36: 70, 37: 200, 38: 600}
        depths = (2.0, 2.5, 3.0, 3.75) if name == "piles_equal_depths" else None
        return _placed_scene(128, 128, piles, 3, depths), piles
    if name == "row_of_65_tiles":                            # T = 65: tile 0 exactly 1024, tile 1 exactly 1025, a few on the last
        piles = {0: 1024, 1: 1025, 64: 5}
        return _placed_scene(1040, 16, piles, 4), piles
    if name == "2112_tiles":                                 # 33 x 64 tiles: the instantiation with up to 8 tiles per thread
        return _placed_scene(528, 1024, {}, 5, spread=400), None
    assert name == "2112_tiles_piles"                        # ... with multi-chunk tiles and every padded size among its chunks
    piles = {0: 1024, 7: 1025, 8: 3000, 1000: 100, 1001: 200, 1002: 400, 1003: 800, 2111: 2049}
    return _placed_scene(528, 1024, piles, 6, spread=400), piles


@pytest.mark.parametrize("name", ["short_chunks", "piles", "piles_equal_depths", "row_of_65_tiles", "2112_tiles", "2112_tiles_piles"])
def test_async_sort_equals_the_oracles_lists(gpu, hip_lib, name):
    from moss_amd.diff_gaussian_rasterization import _C
    scene, piles = _shape(name)
    d = hp.inputs_of(scene, "scale_rot")
    fw = hp.oracle_forward(d)
    R = int(fw.num_rendered)
    counts = (fw.ranges[:, 1].astype(np.int64) - fw.ranges[:, 0])
    T = len(counts)
    assert T == math.ceil(d.W / TILE) * math.ceil(d.H / TILE) and (T > 1024) == name.startswith("2112")
    if piles is not None:                                    # the frame is the one the case describes
        spread = 400 if name.startswith("2112") else 0
        assert R >= sum(piles.values()) and R <= sum(piles.values()) + 4 * spread
        if not spread:
            assert {t: int(counts[t]) for t in piles} == piles and int((counts > 0).sum()) == len(piles)
    if name == "short_chunks":
        assert 0 < counts.max() < 1024
    # the asynchronous forward: a capacity given up front, no host read-back; keys bucketed by the preprocess kernel, scan inside the sort
    cx = _C.RasterContext()
    # (the key buckets are 36 keys per instance of capacity over the tiles: the capacity must also hold the longest list's bucket)
    cx.set_async(True, capacity=max(4 * R + 4096, int(counts.max()) * T // 24))
    c, dev = d.cam, gpu
    a = dict(bg=d.bg.to(dev), means3D=d.means3D.to(dev), opacity=d.opacities.to(dev), scales=d.scales.to(dev),
             rotations=d.rotations.to(dev), view=c.viewmatrix.to(dev), proj=c.projmatrix.to(dev), sh=d.shs.to(dev), campos=c.campos.to(dev))
    E = torch.empty(0, device=dev)
    t = SimpleNamespace()
    for _ in range(2):                                       # (twice: the second frame runs on the state the first one left)
        (_, t.color, t.depth, t.alpha, t.radii, t.geom, t.binning, t.img) = _C.rasterize_gaussians(
            a["bg"], a["means3D"], E, a["opacity"], a["scales"], a["rotations"], 1.0, E, a["view"], a["proj"],
            c.tanfovx, c.tanfovy, c.H, c.W, a["sh"], d.degree, a["campos"], False, 0, None, 0, cx)
        cx.check_status()
        assert cx.last_needed == R
    t.R = R
    e = hp.hip_export(d, t, dev)
    np.testing.assert_array_equal(e.ranges, fw.ranges)
    np.testing.assert_array_equal(e.point_list_keys, fw.point_list_keys)
    np.testing.assert_array_equal(e.point_list, fw.point_list)
