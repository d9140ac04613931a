#!/usr/bin/env python3
"""Generates tests/golden/lbs_deform.npz by CALLING the reference's own ``GaussianModel.coarse_deform_c2source``
(scene/gaussian_model.py:820-923) from a MOSS checkout, on the CPU, in float32.

    python tests/golden/make_golden_lbs.py <path of a MOSS checkout>

scene/gaussian_model.py is loaded on its own (importlib, not through scene/__init__, which pulls in the data readers) with the
third-party modules it imports but this function does not use stubbed in ``sys.modules`` (open3d, plyfile, pytorch3d.transforms,
knn_cuda, simple_knn._C, cv2, sklearn.neighbors).  The function is called unbound on a bare object that carries ``SMPL_NEUTRAL`` =
``moss_amd.lbs.synthetic_body_model(V=256)`` and ``knn`` = an exhaustive nearest-vertex search; ``Tensor.cuda`` is the identity
while it runs.

Cases (P = 512, inputs from :func:`golden_inputs`, numpy PCG64 seeds):
  plain: no lbs_weights, no correct_Rs
  refined: lbs_weights (1,P,24) and correct_Rs (1,23,3,3), as MOSS's pose-refinement branch calls it
both with return_transl=True and a frame rotation R far from the identity.  Stored per case: the reference's float32 smpl_src_pts,
world_src_pts, bweights, transforms, translation; the gradients of <cotangents, (smpl_src_pts, world_src_pts, transforms,
translation)> with respect to query_pts, lbs_weights and correct_Rs; the seeds; and a SHA-256 of every input, so that a change of
the input generator is caught.  The fixture holds no inputs.
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

V, P, J = 256, 512, 24
CASES = {"plain": 11, "refined": 12}
OUTPUTS = ("smpl_src_pts", "world_src_pts", "bweights", "transforms", "translation")
COTANGENT_OF = ("smpl_src_pts", "world_src_pts", "transforms", "translation")


def golden_inputs(case, dtype=torch.float32, device="cpu"):
    """The inputs of one case, regenerated from its seed: a dict with ``body``, ``params``, ``t_params``, ``t_vertices`` (1,V,3),
    ``query_pts`` (1,P,3), ``lbs_weights`` / ``correct_Rs`` (None in the plain case) and ``cotangents`` {output name: tensor}."""
    seed = CASES[case]
    body = mlbs.synthetic_body_model(V, J, seed=1000)
    rng = np.random.Generator(np.random.PCG64(seed))
    params = mlbs.synthetic_frame(seed, J)
    t_params = mlbs.synthetic_frame(0, J, big_pose=True)
    t_vertices = body["v_template"] + torch.tensor(0.01 * rng.normal(size=(V, 3)), dtype=torch.float32)
    home = rng.integers(0, V, size=P)
    query = t_vertices[torch.tensor(home)] + torch.tensor(0.03 * rng.normal(size=(P, 3)), dtype=torch.float32)
    L = cR = None
    if case == "refined":
        L = torch.tensor(0.7 * rng.normal(size=(1, P, J)), dtype=torch.float32)
        cR = mlbs.batch_rodrigues(torch.tensor(0.15 * rng.normal(size=(J - 1, 3)), dtype=torch.float32)).reshape(1, J - 1, 3, 3)
    cot = {"smpl_src_pts": rng.normal(size=(1, P, 3)), "world_src_pts": rng.normal(size=(1, P, 3)),
           "transforms": rng.normal(size=(1, P, 3, 3)), "translation": rng.normal(size=(1, P, 3))}
    d = dict(dtype=dtype, device=device)
    conv = lambda t: None if t is None else t.to(**d)                      # noqa: E731
    return {"body": {k: (v.to(device) if k == "kintree_table" else v.to(**d)) for k, v in body.items()},
            "params": {k: v.to(**d) for k, v in params.items()}, "t_params": {k: v.to(**d) for k, v in t_params.items()},
            "t_vertices": t_vertices[None].to(**d), "query_pts": query[None].to(**d), "lbs_weights": conv(L), "correct_Rs": conv(cR),
            "cotangents": {k: torch.tensor(v, **d) for k, v in cot.items()}}


def inputs_checksum(case):
    """SHA-256 over the float32 bytes of every input of ``case`` in a fixed order."""
    g = golden_inputs(case)
    h = hashlib.sha256()
    parts = [g["body"][k] for k in sorted(g["body"])] + [g["params"][k] for k in sorted(g["params"])]
    parts += [g["t_params"][k] for k in sorted(g["t_params"])] + [g["t_vertices"], g["query_pts"]]
    parts += [t for t in (g["lbs_weights"], g["correct_Rs"]) if t is not None] + [g["cotangents"][k] for k in COTANGENT_OF]
    for t in parts:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def _load_reference(root):
    for name in ("open3d", "plyfile", "pytorch3d", "pytorch3d.transforms", "knn_cuda", "simple_knn", "simple_knn._C", "cv2",
                 "sklearn", "sklearn.neighbors"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = object
    sys.modules["pytorch3d.transforms"].matrix_to_quaternion = None
    sys.modules["knn_cuda"].KNN = object
    sys.modules["simple_knn._C"].distCUDA2 = None
    sys.modules["sklearn.neighbors"].KDTree = object
    sys.path.insert(0, root)
    spec = importlib.util.spec_from_file_location("moss_reference_gaussian_model", os.path.join(root, "scene", "gaussian_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cpu_knn(ref, query):
    """(dist, idx) of the nearest reference point, exhaustively: ref (1,Nr,3), query (1,Nq,3) -> (1,Nq,1) each."""
    d2 = ((query[0][:, None, :] - ref[0][None, :, :]) ** 2).sum(-1)
    dist, idx = d2.min(1)
    return dist[None, :, None], idx[None, :, None]


def run_reference(mod, case):
    g = golden_inputs(case)
    holder = types.SimpleNamespace(SMPL_NEUTRAL=g["body"], knn=cpu_knn)
    q = g["query_pts"].clone().requires_grad_(True)
    L = None if g["lbs_weights"] is None else g["lbs_weights"].clone().requires_grad_(True)
    cR = None if g["correct_Rs"] is None else g["correct_Rs"].clone().requires_grad_(True)
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        out = mod.GaussianModel.coarse_deform_c2source(holder, q, g["params"], g["t_params"], g["t_vertices"], lbs_weights=L,
                                                       correct_Rs=cR, return_transl=True)
    finally:
        torch.Tensor.cuda = cuda
    out = dict(zip(OUTPUTS, out))
    loss = sum((out[k] * g["cotangents"][k]).sum() for k in COTANGENT_OF)
    leaves = [t for t in (q, L, cR) if t is not None]
    grads = torch.autograd.grad(loss, leaves)
    res = {f"{case}_{k}": out[k].detach().numpy().astype(np.float32) for k in OUTPUTS}
    res[f"{case}_grad_query_pts"] = grads[0].numpy()
    if L is not None:
        res[f"{case}_grad_lbs_weights"] = grads[1].numpy()
        res[f"{case}_grad_correct_Rs"] = grads[2].numpy()
    res[f"{case}_seed"] = np.int64(CASES[case])
    res[f"{case}_inputs_sha256"] = np.array(inputs_checksum(case))
    return res


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    mod = _load_reference(os.path.abspath(sys.argv[1]))
    res = {}
    for case in CASES:
        res.update(run_reference(mod, case))
    path = os.path.join(OUT, "lbs_deform.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
