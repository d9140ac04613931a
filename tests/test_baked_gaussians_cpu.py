"""CPU tests of ``moss_amd.bake``: ``BakedGaussians`` holds what ``gaussian_renderer.render`` and ``checkpoint.ply_rows`` read, copies
nothing, concatenates by rows and writes a standard 3DGS PLY bit for bit."""
import inspect
import re

import numpy as np
import pytest
import torch


def _baked(P, seed, degree=3):
    from moss_amd.bake import BakedGaussians
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g)
    return BakedGaussians(r(P, 3), r(P, 16, 3), r(P, 1), r(P, 3), r(P, 4), degree)


def test_ply_round_trip_is_bit_exact(tmp_path):
    from moss_amd.checkpoint import ply_attributes, read_ply
    b = _baked(37, 1)
    path = b.write_ply(str(tmp_path / "deep" / "point_cloud.ply"))
    a = read_ply(path)
    assert list(a) == ply_attributes(16) and b.max_sh_degree == 3 and len(b) == 37
    same = lambda names, t: np.array_equal(np.stack([a[n] for n in names], 1).view(np.uint32), t.numpy().reshape(37, -1).view(np.uint32))
    assert same(("x", "y", "z"), b._xyz) and same(("opacity",), b._opacity)
    assert same(("scale_0", "scale_1", "scale_2"), b._scaling) and same(("rot_0", "rot_1", "rot_2", "rot_3"), b._rotation)
    assert same(("f_dc_0", "f_dc_1", "f_dc_2"), b._features_dc.transpose(1, 2).contiguous())
    assert same([f"f_rest_{i}" for i in range(45)], b._features_rest.transpose(1, 2).contiguous())
    assert not np.any([a[n] for n in ("nx", "ny", "nz")])


def test_cat_is_row_concatenation_and_refuses_mixed_degrees():
    from moss_amd.bake import BakedGaussians
    a, b = _baked(5, 2), _baked(9, 3)
    c = BakedGaussians.cat([a, b])
    for name in ("_xyz", "_features", "_opacity", "_scaling", "_rotation"):
        assert torch.equal(getattr(c, name), torch.cat([getattr(a, name), getattr(b, name)])), name
        assert getattr(c, name).data_ptr() not in (getattr(a, name).data_ptr(), getattr(b, name).data_ptr())
    assert len(c) == 14 and c.active_sh_degree == 3 and c.max_sh_degree == 3
    one = BakedGaussians.cat([a])
    assert torch.equal(one._xyz, a._xyz) and one._xyz.data_ptr() != a._xyz.data_ptr()          # fresh tensors also for one part
    with pytest.raises(ValueError, match="SH degrees differ"):
        BakedGaussians.cat([a, _baked(4, 4, degree=2)])
    with pytest.raises(ValueError, match="nothing"):
        BakedGaussians.cat([])
    with pytest.raises(ValueError, match="rotation must be"):
        BakedGaussians(a._xyz, a._features, a._opacity, a._scaling, a._xyz, 3)
    with pytest.raises(ValueError, match="features must be"):
        BakedGaussians(a._xyz, a._features[:, :, :2], a._opacity, a._scaling, a._rotation, 3)


def test_getters_copy_nothing_and_activate_as_the_model_does():
    from moss_amd import scenes
    from moss_amd.bake import BakedGaussians
    from moss_amd.gaussian_model import GaussianSet
    a = _baked(5, 2)
    assert a.get_xyz is a._xyz and a.get_features is a._features
    assert a._features_dc.shape == (5, 1, 3) and a._features_rest.shape == (5, 15, 3)
    assert a._features_dc.data_ptr() == a._features.data_ptr()
    pc = GaussianSet(scenes.config1(), device="cpu", unified_features=True)
    b = BakedGaussians.of(pc)
    for name in ("_xyz", "_features", "_opacity", "_scaling", "_rotation"):
        assert getattr(b, name).data_ptr() == getattr(pc, name).data_ptr() and not getattr(b, name).requires_grad, name
    for name in ("get_xyz", "get_features", "get_opacity", "get_scaling", "get_rotation"):
        assert torch.equal(getattr(b, name), getattr(pc, name).detach()), name
    assert (b.active_sh_degree, b.max_sh_degree, len(b)) == (pc.active_sh_degree, pc.max_sh_degree, 256)


def test_holder_carries_what_render_reads():
    """Every attribute ``gaussian_renderer.render`` reads from its model on the plain branch with the raw parameters in the op; the
    pose branches are entered through ``coarse_deform_c2source``, which the holder must not have."""
    from moss_amd import gaussian_renderer
    read = set(re.findall(r"\bpc\.(\w+)", inspect.getsource(gaussian_renderer.render)))
    posed_only = {"coarse_deform_c2source", "cross_attention_lbs", "auto_regression", "activate", "get_covariance"}
    assert {"get_xyz", "_opacity", "_scaling", "_rotation", "get_features", "active_sh_degree"} <= read
    b = _baked(3, 5)
    for name in sorted(read - posed_only):
        assert hasattr(b, name), name
    assert not any(hasattr(b, name) for name in posed_only)
    import moss_amd
    import moss_amd.bake
    assert moss_amd.BakedGaussians is moss_amd.bake.BakedGaussians and moss_amd.render_baked is moss_amd.bake.render_baked
