"""CPU side of the fused densify-and-prune decision (moss_amd.densify): the ``*_torch`` restatements against the reference's own
float32 run of ``densify_and_prune`` (tests/golden/densify_decision.npz, made by tests/golden/make_golden_densify.py), and the ABI.

Masks and index lists are exact expectations: the fixture's generator asserted, in float64, that no decision quantity lies within a
relative 1e-3 of its threshold and that no neighbour pair ties.  Float rows: an element may differ from the reference's float32 by
``64 eps32 S_e``, S_e = the sum of the absolute values of the products that form the element, in float64 (64: the constant
tests/test_lbs_cpu.py uses for such chains).  For an element that is a logarithm, log(e^s b) = s + log b, the terms are |s|, the
relative weight of b's own sum (sum |w_j S_j| / |b|, 1 for a constant divisor) and the result; for a quaternion component, the sums
inside the chosen candidate and inside the square root it is divided by.  ``row_bars`` builds S_e; tests/test_gpu_densify_decision.py
uses the same function.
"""
import os
import re

import numpy as np
import pytest
import torch

from moss_amd import densify as D
from tests.golden import make_golden_densify as gold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "densify_decision.npz")
EPS32 = float(np.finfo(np.float32).eps)
K = 64.0


def _rot_abs(q):
    """build_rotation with every product taken in absolute value: the S of each entry of R(q)."""
    n = q / torch.sqrt((q * q).sum(1))[:, None]
    a, x, y, z = n.abs().unbind(1)
    return torch.stack([1 + 2 * (y * y + z * z), 2 * (x * y + a * z), 2 * (x * z + a * y),
                        2 * (x * y + a * z), 1 + 2 * (x * x + z * z), 2 * (y * z + a * x),
                        2 * (x * z + a * y), 2 * (y * z + a * x), 1 + 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def row_bars(mode, index, noise, xyz, features_dc, features_rest, opacity, scaling, rotation, ids=None, lbs_weights=None, denom=None,
             table=None):
    """{row name: K eps32 S_e} for the rows ``mode`` emits; all inputs float64."""
    i = index.long()
    if mode == "merge":
        pair = ids[i]
        S = {"new_xyz": xyz[pair].abs().mean(1), "new_features_dc": features_dc[pair].abs().mean(1),
             "new_features_rest": features_rest[pair].abs().mean(1), "new_opacities": opacity[pair].abs().mean(1),
             "new_scaling": scaling[pair][:, 0].abs() + 1 + torch.log(torch.exp(scaling[pair][:, 0]) / 0.8).abs(),
             "new_rotation": rotation[pair][:, 0].abs()}
        return {k: K * EPS32 * v for k, v in S.items()}
    if mode == "split":
        i = i.repeat(2)
    act, Rabs = torch.exp(scaling[i]), _rot_abs(rotation[i])
    S = {"new_features_dc": features_dc[i].abs(), "new_features_rest": features_rest[i].abs(), "new_opacities": opacity[i].abs()}
    if mode == "split":
        S["new_xyz"] = (Rabs @ (act * noise.abs())[..., None]).squeeze(-1) + xyz[i].abs()
        S["new_scaling"] = scaling[i].abs() + 1 + torch.log(act / 1.6).abs()
        S["new_rotation"] = rotation[i].abs()
    else:
        w = (lbs_weights.reshape(-1, D.JOINTS)[i] / denom.reshape(-1)[0])
        A, B = (w.abs() @ table[:, :9].abs()).reshape(-1, 3, 3), w.abs() @ table[:, 9:].abs()
        rot_joint, scl = (w @ table[:, :9]), w @ table[:, 9:]
        S["new_xyz"] = ((A @ Rabs) @ (B * act * noise.abs())[..., None]).squeeze(-1) + xyz[i].abs()
        S["new_scaling"] = scaling[i].abs() + B / scl.abs() + torch.log(act * scl).abs()
        # the quaternion of rot_joint: the candidate's entries with every sign +, and the sum under the square root
        m = rot_joint
        t = torch.stack([1 + m[:, 0] + m[:, 4] + m[:, 8], 1 + m[:, 0] - m[:, 4] - m[:, 8], 1 - m[:, 0] + m[:, 4] - m[:, 8],
                         1 - m[:, 0] - m[:, 4] + m[:, 8]], dim=1)
        q_abs = torch.sqrt(t.clamp_min(0))
        best = q_abs.argmax(1)
        rows = torch.arange(m.shape[0])
        a = A.reshape(-1, 9)
        t_abs = 1 + a[:, 0] + a[:, 4] + a[:, 8]
        off = [a[:, 7] + a[:, 5], a[:, 2] + a[:, 6], a[:, 3] + a[:, 1]]                 # |m21|+|m12|, |m02|+|m20|, |m10|+|m01|
        cand_abs = torch.stack([torch.stack([t_abs, off[0], off[1], off[2]], 1), torch.stack([off[0], t_abs, off[2], off[1]], 1),
                                torch.stack([off[1], off[2], t_abs, off[0]], 1), torch.stack([off[2], off[1], off[0], t_abs], 1)], 1)[rows, best]
        div = 2 * q_abs[rows, best].clamp_min(0.1)
        q = D.matrix_to_quaternion_torch(m)
        S["new_rotation"] = (cand_abs / div[:, None] + q.abs() * (t_abs / t[rows, best])[:, None]) * rotation[i].abs()
    return {k: K * EPS32 * v for k, v in S.items()}


def worst_ratio(got, ref, bar):
    """max |got - ref| / bar over the elements (0 / 0 counts as 0)."""
    err = (torch.as_tensor(got).double().reshape(-1) - torch.as_tensor(ref).double().reshape(-1)).abs()
    b = torch.as_tensor(bar).double().reshape(-1)
    return float(torch.where(err > 0, err / b.clamp_min(1e-300), torch.zeros_like(err)).max()) if err.numel() else 0.0


class Lineage:
    """Where every row of the set comes from, through the appends and prunes of the sequence: ``origin`` (the input row, or -1 for a
    row a phase made) and, per parameter, the bar the row is held to -- ZERO for a row that descends unchanged from the inputs (it must
    be bit-equal), the row's ``row_bars`` for an appended one.  Clone and split only ever select input rows (a made row has no
    gradient there: its index is beyond n_grads; asserted).  The merge can pair rows made before: its rows inherit their sources'
    bars the way they combine the sources -- the pair's mean for xyz, features and opacity, the first member's for scaling and
    rotation."""

    def __init__(self, n):
        shapes = {"xyz": (3,), "features_dc": (1, 3), "features_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
        self.origin = torch.arange(n)
        self.bar = {k: torch.zeros((n,) + shapes[k], dtype=torch.float64) for k in gold.PARAMS}

    def append(self, phase, index, ids, bars):
        """Adds the rows of ``phase``; returns ``bars`` with what the rows inherit from their sources added."""
        i = index.long()
        out = {}
        for k, r in zip(gold.PARAMS, gold.ROW_NAMES):
            b = bars[r].reshape((-1,) + tuple(self.bar[k].shape[1:]))
            if phase == "merge":
                pair = ids[i]
                b = b + (self.bar[k][pair[:, 0]] if k in ("scaling", "rotation") else self.bar[k][pair].mean(1))
            else:
                assert bool((self.origin[i] >= 0).all()), f"{phase}: a row made by an earlier phase was selected"
            out[r] = b
            self.bar[k] = torch.cat((self.bar[k], b), 0)
        self.origin = torch.cat((self.origin, torch.full((out[gold.ROW_NAMES[0]].shape[0],), -1, dtype=torch.int64)))
        return out

    def prune(self, filt):
        keep = ~torch.as_tensor(filt).cpu().bool()
        self.origin = self.origin[keep]
        self.bar = {k: v[keep] for k, v in self.bar.items()}


def final_ratios(params, lineage, golden, case, inputs):
    """{parameter: worst |final - fixture| / bar}: rows that descend from the inputs must EQUAL the fixture's (and the inputs'), made rows
    lie within their bars.  inf where an unchanged row differs at all."""
    out = {}
    for k in gold.PARAMS:
        ref = torch.as_tensor(golden[f"{case}_final_{k}"]).double()
        got = torch.as_tensor(params[k]).detach().cpu().double().reshape(ref.shape)
        old = lineage.origin >= 0
        assert torch.equal(ref[old], inputs[k].double()[lineage.origin[old]]), f"{k}: the fixture's surviving rows are not the input rows"
        err, bar = (got - ref).abs(), lineage.bar[k].reshape(ref.shape)
        out[k] = float(torch.where(err > 0, err / bar, torch.zeros_like(err)).max()) if err.numel() else 0.0
    return out


def replay(case, dtype, golden=None):
    """MOSS's sequence with the ``*_torch`` functions on the inputs of ``case`` in ``dtype``: yields per phase (name, mask, index, rows,
    prune filter or None, bars) and finally ("final", prune mask, ..., the parameters).  Neighbours from the float32 positions."""
    g = gold.golden_inputs(case, dtype)
    cur = {k: g[k].clone() for k in gold.PARAMS}
    accum, denom = g["accum"].reshape(-1), g["denom"].reshape(-1)
    table = D.joint_tables_torch(g["joint_F"], denom)
    sel_args = (accum, denom, gold.MAX_GRAD, gold.EXTENT, gold.PERCENT_DENSE)
    out, lin = {}, Lineage(gold.P)
    for ph in gold.PHASES:
        p = [cur[k] for k in gold.PARAMS]
        ids = gold.cpu_knn(cur["xyz"][None].float(), cur["xyz"][None].float(), 2)[1][0]
        p64 = [t.double() for t in p]
        if ph == "clone":
            mask, idx, n = D.select_clone_torch(cur["xyz"], cur["rotation"], cur["scaling"], ids, *sel_args, gold.KL_THRESHOLD, g["surface_mask"])
            noise = g["noise_clone"][:n]
            rows = D.clone_rows_torch(idx, noise, *p, g["lbs_weights"], denom, table)
            bars = row_bars(ph, idx, noise.double(), *p64, lbs_weights=g["lbs_weights"].double(), denom=denom.double(), table=table.double())
            filt = None
        elif ph == "split":
            mask, idx, n = D.select_split_torch(cur["xyz"], cur["rotation"], cur["scaling"], ids, *sel_args, gold.KL_THRESHOLD)
            noise = g["noise_split"][:2 * n]
            rows = D.split_rows_torch(idx, noise, *p)
            bars = row_bars(ph, idx, noise.double(), *p64)
            filt = torch.cat((mask, torch.zeros(2 * n, dtype=torch.bool)))
        else:
            mask, idx, n = D.select_merge_torch(cur["xyz"], cur["rotation"], cur["scaling"], ids, *sel_args, 0.1)
            filt = mask.clone()
            rows = D.merge_rows_torch(idx, ids, filt, *p)
            bars = row_bars(ph, idx, None, *p64, ids=ids)
            filt = torch.cat((filt, torch.zeros(n, dtype=torch.bool)))
        bars = lin.append(ph, idx, ids, bars)
        out[ph] = {"mask": mask, "index": idx, "rows": rows, "prune_filter": filt, "bars": bars}
        for k, r in zip(gold.PARAMS, gold.ROW_NAMES):
            cur[k] = torch.cat((cur[k], rows[r]), 0)
        if filt is not None:
            lin.prune(filt)
            for k in gold.PARAMS:
                cur[k] = cur[k][~filt]
    dist = gold.cpu_knn(g["t_vertices"][None].float(), cur["xyz"][None].float(), 1)[0].reshape(-1)
    radii = torch.zeros(cur["xyz"].shape[0], dtype=dtype)                 # (re-zeroed by the appends, scene/gaussian_model.py:452-454)
    final = D.prune_mask_torch(cur["opacity"], cur["scaling"], radii, dist.to(dtype), gold.MIN_OPACITY, gold.EXTENT, gold.SCREEN[case])
    lin.prune(final)
    out["final"] = {"prune_filter": final, "params": {k: cur[k][~final] for k in gold.PARAMS}, "lineage": lin}
    return out


@pytest.fixture(scope="module")
def golden():
    return np.load(FIXTURE)


@pytest.mark.parametrize("case", list(gold.CASES) + ["guard"])
def test_golden_inputs_checksum(golden, case):
    """The inputs regenerated from the seeds are the ones the fixture was made from."""
    n = gold.GUARD_P if case == "guard" else gold.P
    assert int(golden[f"{case}_seed"]) == gold.CASES.get(case, gold.GUARD_SEED)
    assert str(golden[f"{case}_inputs_sha256"]) == gold.inputs_checksum(case, n=n)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("case", list(gold.CASES))
def test_torch_restatements_reproduce_the_reference(golden, case, dtype):
    """select_*_torch / *_rows_torch / prune_mask_torch in MOSS's order reproduce the reference's run: masks, index lists and prune
    filters exactly, every new row and the final parameters within 64 eps32 S_e."""
    out = replay(case, dtype)
    worst = {}
    for ph in gold.PHASES:
        o = out[ph]
        assert np.array_equal(o["mask"].numpy(), golden[f"{case}_{ph}_mask"]), f"{ph}: mask"
        assert np.array_equal(o["index"].numpy(), golden[f"{case}_{ph}_index"]), f"{ph}: index list"
        assert 16 <= int(o["mask"].sum()) <= o["mask"].numel() // 2, ph
        if o["prune_filter"] is not None:
            assert np.array_equal(o["prune_filter"].numpy(), golden[f"{case}_{ph}_prune_filter"]), f"{ph}: prune filter"
        for name in gold.ROW_NAMES:
            ref = golden[f"{case}_{ph}_{name}"]
            assert tuple(o["rows"][name].shape) == ref.shape, (ph, name)
            worst[f"{ph}.{name}"] = worst_ratio(o["rows"][name], ref, o["bars"][name])
    assert np.array_equal(out["final"]["prune_filter"].numpy(), golden[f"{case}_final_prune_filter"])
    for k in gold.PARAMS:
        assert tuple(out["final"]["params"][k].shape) == golden[f"{case}_final_{k}"].shape, k
    lin = out["final"]["lineage"]
    assert int((lin.origin >= 0).sum()) > 100 and int((lin.origin < 0).sum()) > 100       # (both kinds of rows are there to compare)
    for k, v in final_ratios(out["final"]["params"], lin, golden, case, gold.golden_inputs(case)).items():
        worst[f"final.{k}"] = v
    print(f"\n{case} {dtype}: worst error / bar per row tensor: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items() if v > 0))
    for k, v in worst.items():
        assert v < 1.0, (k, v)


def test_guard_case_only_prunes(golden):
    """45 696 rows: every phase returns early (scene/gaussian_model.py:496,530,574); the final prune sees the statistics' max_radii2D."""
    g = gold.golden_inputs("guard", torch.float64, n=gold.GUARD_P)
    assert g["xyz"].shape[0] > D.MAX_POINTS
    dist = gold.cpu_knn(g["t_vertices"][None].float(), g["xyz"][None].float(), 1)[0].reshape(-1).double()
    m = D.prune_mask_torch(g["opacity"], g["scaling"], g["max_radii2D"], dist, gold.MIN_OPACITY, gold.EXTENT, 20)
    ref = np.unpackbits(golden["guard_final_prune_filter"])[:gold.GUARD_P].astype(bool)
    assert np.array_equal(m.numpy(), ref) and int(golden["guard_final_rows"]) == gold.GUARD_P - int(ref.sum())


def test_matrix_to_quaternion_convention():
    """Real part first; the candidate of the largest component: rotations about x, y, z by 0.3 and by 3.0 rad."""
    for axis in range(3):
        for angle in (0.3, 3.0):
            v = torch.zeros(3, dtype=torch.float64)
            v[axis] = 1.0
            Kx = torch.tensor([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=torch.float64)
            R = torch.eye(3, dtype=torch.float64) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)
            q = D.matrix_to_quaternion_torch(R[None])[0]
            want = torch.cat((torch.tensor([np.cos(angle / 2)]), np.sin(angle / 2) * v))
            assert torch.allclose(q, want, atol=1e-12), (axis, angle, q)
            assert torch.allclose(D.build_rotation_torch(q[None])[0], R, atol=1e-12)


def test_joint_tables_torch_row0_is_ones_and_rotations_are_proper():
    g = gold.golden_inputs("screen_none", torch.float64)
    t = D.joint_tables_torch(g["joint_F"], g["denom"])
    assert t.shape == (24, 12) and bool((t[0] == 1).all())
    rot = t[1:, :9].reshape(23, 3, 3)
    assert torch.allclose(rot @ rot.transpose(1, 2), torch.eye(3, dtype=torch.float64).expand(23, 3, 3), atol=1e-12)
    assert torch.allclose(torch.linalg.det(rot), torch.ones(23, dtype=torch.float64)) and bool((t[1:, 9:].diff(dim=1) <= 0).all())
    bad = D.joint_tables_torch(g["joint_F"], torch.zeros(4, dtype=torch.float64))
    assert bool((bad[0] == 1).all()) and bool(bad[1:].isnan().all())


def test_abi_declares_and_exports_the_decision_entry_points(hip_lib):
    """The header declares the three entry points and the workspace query in ABI 7 and the library exports them; the ctypes structs
    have the header's fields in the header's order."""
    from moss_amd import _lib
    text = open(os.path.join(ROOT, "include", "moss_raster.h")).read()
    assert re.search(r"#define\s+MOSS_ABI_VERSION\s+7\b", text) and hip_lib.moss_abi_version() == 7
    for n in ("moss_densify_joint_table", "moss_densify_select", "moss_densify_select_workspace_bytes", "moss_densify_emit"):
        assert re.search(rf"\b{n}\s*\(", text) and hasattr(hip_lib, n), n
    for cls, name in ((_lib.DensifySelectArgs, "moss_densify_select_args"), (_lib.DensifyEmitArgs, "moss_densify_emit_args")):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [f.strip().lstrip("*").strip() for f in re.sub(r"^(const\s+)?[A-Za-z0-9_ ]+?[\s\*]+(?=[a-z_A-Z0-9]+\s*(,|$))", "", decl).split(",")]
        assert fields == [f[0] for f in cls._fields_], (name, fields)
    for mode, value in _lib.DENSIFY_MODES.items():
        assert re.search(rf"#define\s+MOSS_DENSIFY_{mode.upper()}\s+{value}\b", text)
    assert hip_lib.moss_densify_select_workspace_bytes(1) >= 4 and hip_lib.moss_densify_select_workspace_bytes(45696) >= 4 * 179


def test_fused_ops_refuse_cpu_tensors():
    """No CPU path: the fused functions raise on CPU tensors like their neighbours (the ``*_torch`` forms are the torch path)."""
    g = gold.golden_inputs("screen_none")
    ids = torch.zeros((gold.P, 2), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU"):
        D.joint_tables(g["joint_F"], g["denom"])
    with pytest.raises(RuntimeError, match="GPU"):
        D.select_clone(g["xyz"], g["rotation"], g["scaling"], ids, g["accum"], g["denom"], gold.MAX_GRAD, gold.EXTENT)
    with pytest.raises(RuntimeError, match="GPU"):
        D.prune_mask(g["opacity"], g["scaling"], g["max_radii2D"], g["max_radii2D"], 0.1, 1.0)
    with pytest.raises(RuntimeError, match="GPU"):
        D.split_rows(torch.zeros(2, dtype=torch.int32), torch.zeros(4, 3), *[g[k] for k in gold.PARAMS])
    assert set(D.__all__) >= {"joint_tables", "select_clone", "select_split", "select_merge", "prune_mask", "clone_rows", "split_rows",
                              "merge_rows", "densify_and_prune_fused"}
