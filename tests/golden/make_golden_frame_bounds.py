#!/usr/bin/env python3
"""Generates tests/golden/frame_bounds.npz by CALLING the reference's own numpy ``SMPL.__call__`` (smpl/smpl_numpy.py:46-98),
``get_bound_corners`` and ``project`` (scene/dataset_readers.py:1008-1032) from a MOSS checkout, on the CPU.

    python tests/golden/make_golden_frame_bounds.py <path of a MOSS checkout>

Both files are loaded on their own (importlib) with the third-party and sibling modules they import but these functions do not use
stubbed in ``sys.modules``.  The ONE stub that is used is ``cv2.Rodrigues``: ``SMPL.__call__`` turns the pose into rotations with
it, cv2 is not available here, and so it is a float64 numpy Rodrigues (R = I + sin K + (1 - cos) K K with K of the unit axis; the
identity below 1e-12 rad), returning ``(R, None)`` as cv2 does.  It differs from the project's float32 form (angle = |r + 1e-8|) by
about 1e-8 relative, far inside the vertex bar of the tests.

The reference hard-codes V = 6890, J = 24 and 207 pose features, so the body is ``moss_amd.lbs.synthetic_body_model(6890, 24,
BODY_SEED)``, its float32 values as float64 arrays (the pickled model's dtype), set onto an instance made with ``SMPL.__new__``.

Frames: two ``synthetic_frame``s (R far from the identity, pad 0.1) and MOSS's big pose (R = I, Th = 0, pad 0.05:
dataset_readers.py:331-339).  Per frame three cameras that look at the box's centre: ``near`` (3 m), ``far`` (12 m) and ``offside``
(2.5 m, the principal point moved so that the box leaves the frame on two sides).  What the reader does between the calls (:429-436,
:1037: to the world, float32, the padded min / max, np.round) is a few numpy operations, written here in this file's own words.
Every camera is drawn from a seed of its own, and seeds are tried until EVERY unrounded corner coordinate is at least 0.05 px from
a half-integer (asserted): the comparison of rounded corners leaves out no coordinate.  The reference cannot fill a polygon here (no
cv2), so no mask is stored.

Stored: the seeds, a SHA-256 of the body arrays (not the arrays), ``poses``, ``shapes``, ``R``, ``Th``, ``pad`` per frame, ``K`` /
``RT`` (float32-representable) per frame and camera, ``H``, ``W``, and the reference's float32 world vertices, float64 joints,
float32 ``world_bound``, float64 unrounded and int64 rounded corners.
"""
import hashlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from moss_amd import lbs as mlbs  # noqa: E402

V, J = 6890, 24
BODY_SEED = 2000
FRAME_SEEDS = (21, 22, 0)                    # (the last: the big pose)
PADS = (0.1, 0.1, 0.05)
H = W = 512
CAMERAS = ("near", "far", "offside")
MARGIN = 0.05
BODY_KEYS = ("J_regressor", "kintree_table", "posedirs", "shapedirs", "v_template", "weights")


def golden_body(dtype=torch.float32, device="cpu"):
    body = mlbs.synthetic_body_model(V, J, seed=BODY_SEED)
    return {k: (v.to(device) if k == "kintree_table" else v.to(dtype=dtype, device=device)) for k, v in body.items()}


def golden_frame(f):
    """The ``smpl_param`` of frame ``f`` (float32 CPU tensors) and its pad."""
    return mlbs.synthetic_frame(FRAME_SEEDS[f], J, big_pose=f == len(FRAME_SEEDS) - 1), PADS[f]


def body_sha256():
    body = golden_body()
    h = hashlib.sha256()
    for k in BODY_KEYS:
        h.update(np.ascontiguousarray(body[k].numpy()).tobytes())
    return h.hexdigest()


def numpy_rodrigues(r):
    """cv2.Rodrigues for a rotation vector, in float64 numpy: (R (3,3), None)."""
    r = np.asarray(r, dtype=np.float64).reshape(3)
    angle = np.linalg.norm(r)
    if angle < 1e-12:
        return np.eye(3), None
    n = r / angle
    K = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K), None


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


def _load(root, name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference(root):
    cv2 = _Stub("cv2")
    cv2.Rodrigues = numpy_rodrigues
    sys.modules["cv2"] = cv2
    smpl_numpy = _load(root, "moss_reference_smpl_numpy", os.path.join("smpl", "smpl_numpy.py"))
    for name in ("PIL", "scene", "scene.colmap_loader", "scene.gaussian_model", "utils", "utils.graphics_utils", "utils.sh_utils",
                 "imageio", "plyfile", "smpl", "smpl.smpl_numpy", "smplx", "smplx.body_models", "smplx.lbs", "data", "data.dna_rendering",
                 "data.dna_rendering.dna_rendering_sample_code", "data.dna_rendering.dna_rendering_sample_code.SMCReader"):
        sys.modules[name] = _Stub(name)
    readers = _load(root, "moss_reference_dataset_readers", os.path.join("scene", "dataset_readers.py"))
    return smpl_numpy.SMPL, readers


def reference_smpl(SMPL):
    body = golden_body()
    m = SMPL.__new__(SMPL)
    for k in ("J_regressor", "weights", "posedirs", "v_template", "shapedirs"):
        setattr(m, k, body[k].numpy().astype(np.float64))
    m.kintree_table = body["kintree_table"].numpy()
    m.parent = m.kintree_table[0, 1:].copy()
    return m


def look_at(kind, centre, seed):
    """(K (3,3), RT (3,4)) float32 of a camera of ``kind`` looking at ``centre``, drawn from ``seed``."""
    rng = np.random.Generator(np.random.PCG64(seed))
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    dist = {"near": 3.0, "far": 12.0, "offside": 2.5}[kind] * rng.uniform(0.95, 1.05)
    pos = centre + dist * d
    z = (centre - pos) / np.linalg.norm(centre - pos)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], 0)
    f = 500.0 * rng.uniform(0.9, 1.1)
    cx, cy = (W / 2 + 200.0, H / 2 + 180.0) if kind == "offside" else (W / 2 + rng.uniform(-5, 5), H / 2 + rng.uniform(-5, 5))
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]])
    return K.astype(np.float32), np.concatenate([R, (-R @ pos)[:, None]], 1).astype(np.float32)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    SMPL, readers = load_reference(os.path.abspath(sys.argv[1]))
    smpl = reference_smpl(SMPL)
    F, C = len(FRAME_SEEDS), len(CAMERAS)
    res = {"body_seed": np.int64(BODY_SEED), "body_sha256": np.array(body_sha256()), "frame_seeds": np.array(FRAME_SEEDS, dtype=np.int64),
           "pad": np.array(PADS, dtype=np.float32), "H": np.int64(H), "W": np.int64(W), "cameras": np.array(CAMERAS)}
    keys = ("poses", "shapes", "R", "Th", "vertices", "joints", "world_bound")
    per = {k: [] for k in keys}
    Ks, RTs, unrounded, rounded = np.zeros((F, C, 3, 3), np.float32), np.zeros((F, C, 3, 4), np.float32), np.zeros((F, C, 8, 2)), \
        np.zeros((F, C, 8, 2), np.int64)
    camera_seeds = np.zeros((F, C), dtype=np.int64)
    for f in range(F):
        frame, pad = golden_frame(f)
        p = {k: v.numpy().astype(np.float32) for k, v in frame.items()}
        xyz, joints = smpl(p["poses"], p["shapes"].reshape(-1))
        # what the reader does with them (dataset_readers.py:429-436), in this file's words: to the world in float64, rounded to
        # float32 once, then the box of the float32 vertices padded in float32
        xyz = (xyz @ p["R"].T + p["Th"]).astype(np.float32)
        world_bound = np.stack([xyz.min(0) - np.float32(pad), xyz.max(0) + np.float32(pad)])
        assert world_bound.dtype == np.float32
        for k, v in zip(keys, (p["poses"], p["shapes"], p["R"], p["Th"], xyz, joints, world_bound)):
            per[k].append(v)
        centre = world_bound.astype(np.float64).mean(0)
        corners_3d = readers.get_bound_corners(world_bound)
        for c, kind in enumerate(CAMERAS):
            seed = 1000 * (f + 1) + 100 * c
            while True:
                K, RT = look_at(kind, centre, seed)
                xy = readers.project(corners_3d, K.astype(np.float64), RT.astype(np.float64))
                if np.abs(xy - np.floor(xy) - 0.5).min() >= MARGIN:
                    break
                seed += 1
            assert np.abs(xy - np.floor(xy) - 0.5).min() >= MARGIN
            Ks[f, c], RTs[f, c], unrounded[f, c], camera_seeds[f, c] = K, RT, xy, seed
            rounded[f, c] = np.rint(xy).astype(np.int64)                                     # (half to even, as :1037's np.round)
        off = rounded[f, CAMERAS.index("offside")]
        assert (off[:, 0] >= W).any() and (off[:, 1] >= H).any(), "the offside camera must lose the box on two sides"
    res.update({k: np.stack(v, 0) for k, v in per.items()})
    res.update(K=Ks, RT=RTs, corners_unrounded=unrounded, corners=rounded, camera_seeds=camera_seeds)
    path = os.path.join(OUT, "frame_bounds.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
