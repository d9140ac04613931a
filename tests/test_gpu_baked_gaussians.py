"""``moss_amd.bake`` on the GPU: ``render_baked`` of a model's own Gaussians is ``render()``'s plain branch bit for bit, a
concatenation renders as its rows do, and the PLY of device tensors holds their bits.  The scene is ``scenes.config1`` (256 Gaussians,
128 x 128, SH degree 3) and a second, shifted copy of it.  Bit for bit: the holder adds no mathematics, and the forward is
bit-reproducible (tests/test_gpu_player.py rests on the same)."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("render", "render_depth", "render_alpha", "radii")


@pytest.fixture(scope="module")
def world(gpu, hip_lib):
    from moss_amd import scenes
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import camera_view
    s = scenes.config1()
    other = copy.copy(s)
    g = torch.Generator().manual_seed(5)
    other.means3D = s.means3D[torch.randperm(s.P, generator=g)[:131]] + torch.tensor([0.25, -0.1, 0.4])
    other.scales, other.rotations, other.opacities, other.shs = s.scales[:131] * 1.3, s.rotations[:131].flip(0), s.opacities[:131], s.shs[:131].flip(0)
    pcs = [GaussianSet(x, device=gpu, unified_features=True) for x in (s, other)]
    return SimpleNamespace(pcs=pcs, cam=camera_view(s.camera, gpu), bg=torch.tensor([0.1, 0.2, 0.3], device=gpu))


def _plain(cam, pc, bg):
    from moss_amd.diff_gaussian_rasterization import RasterContext
    from moss_amd.gaussian_renderer import render
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raw_parameters_in_op=True,
                           raster_context=RasterContext())
    with torch.no_grad():
        return render(cam, pc, pipe, bg)


def test_render_baked_is_the_plain_render_of_the_model(gpu, world):
    from moss_amd.bake import BakedGaussians, render_baked
    from moss_amd.diff_gaussian_rasterization import RasterContext
    for pc in world.pcs:
        want = _plain(world.cam, pc, world.bg)
        got = render_baked(world.cam, BakedGaussians.of(pc), world.bg, context=RasterContext())
        assert float(want["render"].max()) > 0.3 and int((want["radii"] > 0).sum()) > 100
        assert not got["render"].requires_grad
        for k in KEYS:
            assert torch.equal(got[k], want[k]), k
    big = render_baked(world.cam, BakedGaussians.of(world.pcs[0]), world.bg, context=RasterContext(), scaling_modifier=1.5)
    base = render_baked(world.cam, BakedGaussians.of(world.pcs[0]), world.bg, context=RasterContext())
    assert bool((big["radii"] >= base["radii"]).all()) and int(big["radii"].sum()) > int(base["radii"].sum())     # the modifier reaches the op


def test_concatenated_avatars_render_in_one_frame(gpu, world):
    from moss_amd.bake import BakedGaussians, render_baked
    from moss_amd.diff_gaussian_rasterization import RasterContext
    a, b = (BakedGaussians.of(pc) for pc in world.pcs)
    alone = [render_baked(world.cam, x, world.bg, context=RasterContext()) for x in (a, b)]
    both = render_baked(world.cam, BakedGaussians.cat([a, b]), world.bg, context=RasterContext())
    torch.cuda.synchronize(gpu)
    assert both["radii"].shape == (len(a) + len(b),)
    assert torch.equal(both["radii"], torch.cat([alone[0]["radii"], alone[1]["radii"]]))     # a Gaussian's radius is its own
    assert not torch.equal(both["render"], alone[0]["render"]) and not torch.equal(both["render"], alone[1]["render"])
    # the same rows split and joined again are the same inputs: the same bits
    halves = BakedGaussians.cat([BakedGaussians(a._xyz[:100], a._features[:100], a._opacity[:100], a._scaling[:100], a._rotation[:100], 3),
                                 BakedGaussians(a._xyz[100:], a._features[100:], a._opacity[100:], a._scaling[100:], a._rotation[100:], 3)])
    again = render_baked(world.cam, halves, world.bg, context=RasterContext())
    for k in KEYS:
        assert torch.equal(again[k], alone[0][k]), k


def test_ply_of_device_tensors_holds_their_bits(gpu, world, tmp_path):
    from moss_amd.bake import BakedGaussians
    from moss_amd.checkpoint import read_ply
    c = BakedGaussians.cat([BakedGaussians.of(pc) for pc in world.pcs])
    a = read_ply(c.write_ply(str(tmp_path / "both.ply")))
    for names, t in ((("x", "y", "z"), c._xyz), (("opacity",), c._opacity), (("scale_0", "scale_1", "scale_2"), c._scaling),
                     (("rot_0", "rot_1", "rot_2", "rot_3"), c._rotation)):
        assert np.array_equal(np.stack([a[n] for n in names], 1).view(np.uint32), t.cpu().numpy().view(np.uint32)), names
