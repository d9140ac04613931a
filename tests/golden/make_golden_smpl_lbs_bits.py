#!/usr/bin/env python3
"""Generates tests/golden/smpl_lbs_bits.json: one SHA-256 per output tensor of the eight C entry points of the SMPL / LBS family
(moss_lbs_deform_forward / _backward / _backward_frame, moss_smpl_frame_forward / _backward / _backward_pose, moss_smpl_vertices,
moss_bound_mask), called through ctypes on an MI355X on inputs drawn on the CPU from fixed seeds.

    python tests/golden/make_golden_smpl_lbs_bits.py

These kernels form every sum in float64 in a fixed order, so their outputs are a function of the inputs and of the compiler alone:
the file also records ``torch.version.hip`` and the ``hipcc --version`` lines the library was built with, and
tests/test_gpu_smpl_lbs_bits.py compares bits only under the same toolchain.  The file is a record of ONE commit's kernels; a change
that is meant to keep the bits must pass against it, not regenerate it.

Cases (the smallest shapes at which the kernels take another path): V in {1, 17, 257} (one vertex; one past the 16-vertex workgroup
of the offsets and posed kernels; one past the 256-vertex skin workgroup), J in {1, 2, 24, 55, 64} (no pose blend shapes; one joint
with them; SMPL; a 6 J that does not divide the fold block; the limit), P in {0, 1, 129, 1025} (empty; one; one past the
128-Gaussian backward workgroup; one past the 1024-Gaussian gather workgroup): V = 257 with every J at P = 129, J = 24 with every V
and P.  Per case a chain -- the SMPL-frame forward with and without correct_Rs / saved, the LBS forward with and without
lbs_offsets / x / p / w, both LBS backwards and both SMPL-frame backwards with every output on and each optional output off in turn,
the vertex call with and without joints / shapes -- and at V = 257, J = 24, P = 129 the LBS calls once more with ``weights`` moved
by 4 bytes (the J = 24 instantiation without 16-byte row accesses).  At P = 1025 two ids lie outside [0, V).  moss_bound_mask at
(C, H, W) = (1, 1, 1), (3, 17, 23), (3, 130, 70); the last camera of three sits inside the box (flagged).

Every output buffer is filled with 123 (integers: 77) before the call and hashed whole, so an element that a call leaves unwritten
(P = 0, J = 1) is part of the record; workspaces are filled with 0xFF bytes.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from moss_amd import _lib  # noqa: E402
from moss_amd import build as hip_build  # noqa: E402
from moss_amd import lbs as mlbs  # noqa: E402

PATH = os.path.join(OUT, "smpl_lbs_bits.json")
SIZES = [(257, J, 129) for J in (1, 2, 55, 64)] + [(V, 24, P) for V in (1, 17, 257) for P in (0, 1, 129, 1025)]   # (V, J, P)
MASKS = [(1, 1, 1), (3, 17, 23), (3, 130, 70)]                                                                     # (C, H, W)
MISALIGNED = (257, 24, 129)
SAVED = _lib.SMPL_FRAME_SAVED_FLOATS_PER_JOINT


def case_names():
    return ["V%d_J%d_P%d" % s for s in SIZES] + ["mask_C%d_H%d_W%d" % m for m in MASKS]


def toolchain():
    """What the bits depend on besides the sources: torch's HIP version and hipcc's own version lines."""
    out = subprocess.run([hip_build.HIPCC, "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    lines = [ln.strip() for ln in out.splitlines() if ln.startswith("HIP version") or "clang version" in ln]
    return {"torch_hip": str(torch.version.hip), "hipcc": "; ".join(lines)}


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def run(name, cls, dev, **fields):
    """One call of entry point ``name`` on the current stream: tensors pass their address, ``parents`` its list, the rest as given."""
    a = cls()
    for k, v in fields.items():
        if k == "parents":
            a.parents[:len(v)] = v
        else:
            setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
    _lib.call(name, dev, ctypes.byref(a))


class Draw:
    """Seeded CPU draws (numpy PCG64), moved to the device as float32."""

    def __init__(self, seed, dev):
        self.rng, self.dev = np.random.Generator(np.random.PCG64(seed)), dev

    def normal(self, *shape, scale=1.0):
        return torch.tensor(scale * self.rng.normal(size=shape), dtype=torch.float32).to(self.dev)

    def rotations(self, n):
        """(n,3,3): the float32 Rodrigues of small random axis-angles (correct_Rs are rotations near the identity)."""
        return mlbs.batch_rodrigues(torch.tensor(0.2 * self.rng.normal(size=(n, 3)), dtype=torch.float32)).contiguous().to(self.dev)


def out(dev, *shape, dtype=torch.float32):
    return torch.full(shape, 77 if dtype != torch.float32 else 123.0, dtype=dtype, device=dev)


def workspace(dev, nbytes):
    return torch.full((max(int(nbytes), 1),), 255, dtype=torch.uint8, device=dev)


def leave_one_out(names):
    """Every output on, then each one off in turn: ('all', names), ('no_<k>', names without k)."""
    return [("all", tuple(names))] + [("no_" + k, tuple(n for n in names if n != k)) for k in names]


def size_case(V, J, P, dev):
    """name -> SHA-256 of every output of the chain at (V, J, P)."""
    lib = _lib.lib()
    res = {}
    seed = 1000003 * V + 1009 * J + P
    dr = Draw(seed, dev)
    body = mlbs.synthetic_body_model(V, J, seed=seed % 9973)
    par = [int(v) for v in body["kintree_table"][0].tolist()]
    par[0] = 0
    vt, sd, pd, jr, W = (body[k].to(dev) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights"))
    if J == 1:
        pd = torch.zeros(1, device=dev)                                 # (never read: 9 (J - 1) = 0 features)
    rows = max(P, 1)                                                    # (P = 0: valid addresses nevertheless)
    ids = torch.tensor(dr.rng.integers(0, V, size=rows), dtype=torch.int64)
    if P == 1025:
        ids[5], ids[700] = -1, V
    ids = ids.to(dev)
    poses_big, poses = dr.normal(3 * J, scale=0.3), dr.normal(3 * J, scale=0.3)
    shapes_big, shapes = dr.normal(10, scale=0.5), dr.normal(10, scale=0.5)
    cR = dr.rotations(max(J - 1, 1))
    R, Th, pad = dr.rotations(1)[0].contiguous(), dr.normal(3), torch.tensor([0.1], dtype=torch.float32).to(dev)
    L, x = dr.normal(rows, J, scale=0.5), dr.normal(rows, 3)
    gT, gt, gp = dr.normal(rows, 9), dr.normal(rows, 3), dr.normal(rows, 3)
    gA_in, gd_in = dr.normal(J, 16), dr.normal(rows, 3)

    # ---- moss_smpl_frame_forward: with correct_Rs and saved (what the backwards read), then without either and fewer betas
    ws_sf = lib.moss_smpl_frame_workspace_bytes(rows, V, J)
    fwd = {}
    for tag, with_cr, nb in (("cR", True, 10), ("plain", False, 7)):
        o = {"A_big": out(dev, J, 16), "A_obs": out(dev, J, 16), "d": out(dev, rows, 3), "rot_mats": out(dev, J, 9)}
        if with_cr:
            o["saved"] = out(dev, SAVED * J)
        ws = workspace(dev, ws_sf)
        run("moss_smpl_frame_forward", _lib.SmplFrameArgs, dev, P=P, V=V, J=J, num_betas_big=10, num_betas=nb, shapedirs_stride=10,
            parents=par, v_template=vt, shapedirs=sd, posedirs=pd, J_regressor=jr, poses_big=poses_big, shapes_big=shapes_big,
            poses=poses, shapes=shapes, correct_Rs=cR if with_cr and J > 1 else None, vert_ids=ids, workspace=ws, workspace_bytes=ws_sf, **o)
        res.update({f"smpl_frame_forward/{tag}/{k}": sha(v) for k, v in o.items()})
        fwd[tag] = o
    A_big, A_obs, d, saved = (fwd["cR"][k] for k in ("A_big", "A_obs", "d", "saved"))

    # ---- the LBS calls, on the forward's A_big, A_obs, d; ``weights`` 16-byte aligned, and once moved by 4 bytes
    layouts = [("", W)]
    if (V, J, P) == MISALIGNED:
        buf = torch.zeros(V * J + 1, device=dev)
        buf[1:] = W.reshape(-1)
        layouts.append(("misaligned/", buf[1:].view(V, J)))
        assert layouts[1][1].data_ptr() % 16 == 4
    for pre, Wl in layouts:
        common = dict(P=P, J=J, V=V, vert_ids=ids, weights=Wl, A_big=A_big, A_obs=A_obs, d=d, R=R, Th=Th)
        for tag, full in (("full", True), ("bare", False)):
            o = {"T": out(dev, rows, 9), "t": out(dev, rows, 3)}
            if full:
                o.update(p=out(dev, rows, 3), w=out(dev, rows, J))
            run("moss_lbs_deform_forward", _lib.LbsForwardArgs, dev, lbs_offsets=L if full else None, x=x if full else None, **common, **o)
            res.update({f"{pre}lbs_forward/{tag}/{k}": sha(v) for k, v in o.items()})
        for entry, cls, extra, ws_fn in (("moss_lbs_deform_backward", _lib.LbsBackwardArgs, (), lib.moss_lbs_workspace_bytes),
                                         ("moss_lbs_deform_backward_frame", _lib.LbsBackwardFrameArgs, ("g_R", "g_Th"),
                                          lib.moss_lbs_frame_workspace_bytes)):
            shapes_of = {"g_L": (rows, J), "g_A_obs": (J, 16), "g_d": (rows, 3), "g_x": (rows, 3), "g_R": (9,), "g_Th": (3,)}
            variants = leave_one_out(("g_L", "g_A_obs", "g_d", "g_x") + extra)
            variants.append(("bare", ("g_A_obs", "g_d") + extra))       # without lbs_offsets and x (so without g_L, g_p, g_x), g_t alone
            for tag, names in variants:
                bare = tag == "bare"
                o = {k: out(dev, *shapes_of[k]) for k in names}
                nbytes = ws_fn(rows, J)
                ws = workspace(dev, nbytes)
                run(entry, cls, dev, lbs_offsets=None if bare else L, x=None if bare else x, g_T=None if bare else gT, g_t=gt,
                    g_p=None if bare else gp, workspace=ws, workspace_bytes=nbytes, **common, **o)
                res.update({f"{pre}{entry[5:]}/{tag}/{k}": sha(v) for k, v in o.items()})

    # ---- the SMPL-frame backwards: cotangents of A_obs and d on and off; the pose form with g_correct_Rs and correct_Rs on and off
    back = dict(P=P, V=V, J=J, parents=par, posedirs=pd, vert_ids=ids, saved=saved)
    cots = (("gA_gd", gA_in, gd_in), ("gA", gA_in, None), ("gd", None, gd_in))
    for tag, gA, gd in cots:
        o = out(dev, max(J - 1, 1), 9)
        ws = workspace(dev, ws_sf)
        run("moss_smpl_frame_backward", _lib.SmplFrameBackwardArgs, dev, g_A_obs=gA, g_d=gd, g_correct_Rs=o, workspace=ws,
            workspace_bytes=ws_sf, **back)
        res[f"smpl_frame_backward/{tag}/g_correct_Rs"] = sha(o)
    for tag, gA, gd in cots:
        for sub, want_gcr, with_cr in (("gcR_cR", True, True), ("cR", False, True), ("gcR", True, False)):
            o = {"g_poses": out(dev, 3 * J)}
            if want_gcr:
                o["g_correct_Rs"] = out(dev, max(J - 1, 1), 9)
            ws = workspace(dev, ws_sf)
            run("moss_smpl_frame_backward_pose", _lib.SmplFrameBackwardPoseArgs, dev, g_A_obs=gA, g_d=gd, poses=poses,
                correct_Rs=cR if with_cr and J > 1 else None, workspace=ws, workspace_bytes=ws_sf, **back, **o)
            res.update({f"smpl_frame_backward_pose/{tag}/{sub}/{k}": sha(v) for k, v in o.items()})

    # ---- moss_smpl_vertices: with joints and shapes, then without either
    nbytes = lib.moss_smpl_vertices_workspace_bytes(V, J)
    for tag, full in (("full", True), ("bare", False)):
        o = {"world_vertex": out(dev, V, 3), "world_bound": out(dev, 6)}
        if full:
            o["joints"] = out(dev, J, 3)
        ws = workspace(dev, nbytes)
        run("moss_smpl_vertices", _lib.SmplVerticesArgs, dev, V=V, J=J, num_betas=10 if full else 0, shapedirs_stride=10, parents=par,
            v_template=vt, shapedirs=sd, posedirs=pd, J_regressor=jr, weights=W, poses=poses, shapes=shapes if full else None, R=R, Th=Th,
            pad=pad, workspace=ws, workspace_bytes=nbytes, **o)
        res.update({f"smpl_vertices/{tag}/{k}": sha(v) for k, v in o.items()})
    return res


def mask_case(C, H, W, dev):
    lib = _lib.lib()
    dr = Draw(7000 + 100 * C + H + W, dev)
    wb = torch.tensor([[-0.4, -0.5, -0.6], [0.5, 0.4, 0.7]], dtype=torch.float32).to(dev)
    f = 0.8 * max(H, W)
    K = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], dtype=torch.float32).repeat(C, 1, 1).to(dev)
    rot = mlbs.batch_rodrigues(torch.tensor(dr.rng.normal(size=(C, 3)), dtype=torch.float32))
    trans = torch.tensor([[0.1, -0.1, 0.3 if c == 2 else 3.0] for c in range(C)], dtype=torch.float32)      # (0.3: inside the box)
    RT = torch.cat([rot, trans[..., None]], -1).contiguous().to(dev)
    o = {"bound": out(dev, C, H, W, dtype=torch.uint8), "rect": out(dev, C, 5, dtype=torch.int32),
         "corners": out(dev, C, 16, dtype=torch.int32), "flags": out(dev, C, dtype=torch.int32)}
    nbytes = lib.moss_bound_mask_workspace_bytes(C, H, W)
    ws = workspace(dev, nbytes)
    run("moss_bound_mask", _lib.BoundMaskArgs, dev, C=C, H=H, W=W, world_bound=wb, K=K, RT=RT, workspace=ws, workspace_bytes=nbytes, **o)
    return {f"bound_mask/{k}": sha(v) for k, v in o.items()}


def run_case(name, dev):
    """name (one of :func:`case_names`) -> {output: SHA-256}."""
    parts = name.split("_")
    if parts[0] == "mask":
        res = mask_case(*(int(p[1:]) for p in parts[1:]), dev)
    else:
        res = size_case(*(int(p[1:]) for p in parts), dev)
    torch.cuda.synchronize(dev)
    return res


def main():
    assert torch.cuda.is_available(), "the bits are an MI355X's: this generator needs the GPU"
    dev = torch.device("cuda:0")
    doc = dict(toolchain(), cases={name: run_case(name, dev) for name in case_names()})
    with open(PATH, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(PATH, os.path.getsize(PATH), "bytes,", sum(len(c) for c in doc["cases"].values()), "hashes")


if __name__ == "__main__":
    main()
