"""Standard 3D Gaussians -- ``(xyz, scale, quaternion, opacity, SH)`` and nothing else -- as an object ``gaussian_renderer.render`` and
``checkpoint.write_ply`` take: what every 3DGS viewer and tool reads, and what this project's plain forward path (``scales`` /
``rotations``, no ``transforms``) renders.

:class:`BakedGaussians` holds such a set without copying it; :meth:`BakedGaussians.cat` puts several sets -- two avatars, an avatar
and a scene -- into one; :meth:`BakedGaussians.write_ply` writes a standard 3DGS PLY; :func:`render_baked` renders one under
``no_grad`` on the rasterizer's forward-only path.

NOT HERE: the op that makes such a set from a POSED avatar.  MOSS poses a frame by a per-Gaussian 3x3 LBS matrix ``T`` -- a blend of
joint rotations, not a rotation -- applied to the means (``gaussian_renderer/__init__.py:74-77``) and to the covariance (``:88-90``,
``scene/gaussian_model.py:37-52``), so ``T R S^2 R^T T^T`` has no ``(scale, quaternion)`` until it is decomposed (the SVD of
``T R S``).  Until that op exists a holder is filled from a canonical model, a PLY or a caller's own decomposition.

Everything here imports without a GPU.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

__all__ = ["BakedGaussians", "render_baked"]


class BakedGaussians:
    """Standard 3D Gaussians: ``_xyz`` (P,3), ``_features`` (P,K,3), ``_opacity`` (P,1) logits, ``_scaling`` (P,3) logarithms,
    ``_rotation`` (P,4) with the real part first, ``active_sh_degree`` / ``max_sh_degree`` -- exactly what
    ``gaussian_renderer.render`` and ``checkpoint.ply_rows`` read.  A plain holder: it copies nothing and has no
    ``coarse_deform_c2source``, so ``render()`` takes its plain branch."""
    unified_features = True

    def __init__(self, xyz, features, opacity, scaling, rotation, active_sh_degree, max_sh_degree=None):
        P = int(xyz.shape[0])
        for name, t, tail in (("xyz", xyz, (3,)), ("opacity", opacity, (1,)), ("scaling", scaling, (3,)), ("rotation", rotation, (4,))):
            if tuple(t.shape) != (P,) + tail:
                raise ValueError(f"BakedGaussians: {name} must be {(P,) + tail}, got {tuple(t.shape)}")
        if features.dim() != 3 or features.shape[0] != P or features.shape[2] != 3:
            raise ValueError(f"BakedGaussians: features must be ({P},K,3), got {tuple(features.shape)}")
        self._xyz, self._features, self._opacity, self._scaling, self._rotation = xyz, features, opacity, scaling, rotation
        self.active_sh_degree = int(active_sh_degree)
        self.max_sh_degree = int(round(features.shape[1] ** 0.5)) - 1 if max_sh_degree is None else int(max_sh_degree)

    @classmethod
    def of(cls, pc):
        """The canonical set of a model (``GaussianSet(unified_features=True)`` or anything with the same attributes): the model's
        own tensors, detached, not copies."""
        return cls(pc._xyz.detach(), pc._features.detach(), pc._opacity.detach(), pc._scaling.detach(), pc._rotation.detach(),
                   pc.active_sh_degree, pc.max_sh_degree)

    get_xyz = property(lambda self: self._xyz)
    get_features = property(lambda self: self._features)
    get_opacity = property(lambda self: torch.sigmoid(self._opacity))
    get_scaling = property(lambda self: torch.exp(self._scaling))
    get_rotation = property(lambda self: torch.nn.functional.normalize(self._rotation))
    _features_dc = property(lambda self: self._features[:, :1, :])
    _features_rest = property(lambda self: self._features[:, 1:, :])

    def __len__(self):
        return int(self._xyz.shape[0])

    @staticmethod
    def cat(parts):
        """The rows of ``parts`` one after the other, as fresh tensors.  All parts share the active SH degree, the coefficient
        count and the device."""
        parts = list(parts)
        if not parts:
            raise ValueError("BakedGaussians.cat: nothing to concatenate")
        first = parts[0]
        for p in parts[1:]:
            if p.active_sh_degree != first.active_sh_degree or p.max_sh_degree != first.max_sh_degree:
                raise ValueError(f"BakedGaussians.cat: SH degrees differ ({first.active_sh_degree}/{first.max_sh_degree} and "
                                 f"{p.active_sh_degree}/{p.max_sh_degree})")
            if p._xyz.device != first._xyz.device:
                raise ValueError(f"BakedGaussians.cat: devices differ ({first._xyz.device} and {p._xyz.device})")
        join = lambda name: torch.cat([getattr(p, name).detach() for p in parts], dim=0)
        return BakedGaussians(join("_xyz"), join("_features"), join("_opacity"), join("_scaling"), join("_rotation"),
                              first.active_sh_degree, first.max_sh_degree)

    def write_ply(self, path):
        """A standard 3DGS ``point_cloud.ply`` of these rows (``checkpoint.write_ply``: MOSS's ``save_ply`` layout)."""
        from .checkpoint import write_ply
        write_ply(path, self)
        return path


def render_baked(camera, baked, bg, context=None, scaling_modifier=1.0):
    """``gaussian_renderer.render`` of a :class:`BakedGaussians` under ``no_grad``: the plain branch (``scales`` / ``rotations``, no
    ``transforms``) with the raw parameters activated inside the op, on the rasterizer's forward-only path.  ``context``: a
    ``RasterContext`` to keep between calls (None: the module's default)."""
    from .gaussian_renderer import render
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raw_parameters_in_op=True,
                           **({} if context is None else {"raster_context": context}))
    with torch.no_grad():
        return render(camera, baked, pipe, bg, scaling_modifier=scaling_modifier)
