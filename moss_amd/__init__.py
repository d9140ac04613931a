"""moss_amd: MOSS's hot paths as HIP kernels for the MI355X (gfx950).  The ops live in the submodules (``moss_amd.bounds``,
``moss_amd.play``, ...); importing the package loads none of them.  The names below resolve on first use."""

_LAZY = {"prepare_views": "images", "prepare_views_torch": "images",
         "BakedGaussians": "bake", "render_baked": "bake",
         "PoseFitter": "posefit", "posed_frame": "posefit",
         "keypoint_loss": "keypoints", "posed_vertices_fn": "keypoints", "KeypointTargets": "keypoints"}

__all__ = sorted(_LAZY)


def __getattr__(name):
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module("." + _LAZY[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
