"""``moss_amd.checkpoint`` without a GPU: MOSS's PLY byte for byte, the reader's leniency and refusals, the model directory, the
optimizer state as plain values, and ``run_schedule(start_iteration=, saving_iterations=, save=)`` driven by a recording stub.  Every
comparison is equality of bytes or bits."""
import os
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HEAD = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n"


def _model(P, degree=3, unified=True, seed=0):
    """A GaussianSet of random parameters, every element distinct (a swapped index cannot pass)."""
    from moss_amd.gaussian_model import GaussianSet
    g = torch.Generator().manual_seed(1000 * seed + 17 * P + degree)
    k = (degree + 1) ** 2
    scene = SimpleNamespace(means3D=torch.randn(P, 3, generator=g), shs=torch.randn(P, k, 3, generator=g),
                            scales=0.01 + torch.rand(P, 3, generator=g), rotations=torch.randn(P, 4, generator=g),
                            opacities=0.05 + 0.9 * torch.rand(P, 1, generator=g))
    pc = GaussianSet(scene, sh_degree=degree, unified_features=unified)
    pc.max_sh_degree = degree
    every = torch.cat([p.detach().reshape(-1) for p in pc.parameters()])
    assert every.unique().numel() == every.numel()
    return pc


def _names(degree):
    """The attribute order, spelled out: scene/gaussian_model.py:271-283."""
    rest = 3 * ((degree + 1) ** 2 - 1)
    return (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + ["f_rest_%d" % i for i in range(rest)] + ["opacity"]
            + ["scale_0", "scale_1", "scale_2"] + ["rot_0", "rot_1", "rot_2", "rot_3"])


def _rows(pc):
    """The reference's own expression (scene/gaussian_model.py:289-300) on the model's tensors."""
    xyz = pc._xyz.detach().cpu().numpy()
    f_dc = pc._features_dc.detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
    f_rest = pc._features_rest.detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
    return np.concatenate((xyz, np.zeros_like(xyz), f_dc, f_rest, pc._opacity.detach().cpu().numpy(), pc._scaling.detach().cpu().numpy(),
                           pc._rotation.detach().cpu().numpy()), axis=1)


def _expected_bytes(pc, degree):
    header = HEAD % pc._xyz.shape[0] + "".join("property float %s\n" % n for n in _names(degree)) + "end_header\n"
    return header.encode("ascii") + _rows(pc).astype("<f4").tobytes()


@pytest.mark.parametrize("P,degree,unified", [(5, 3, True), (5, 1, True), (1, 3, True), (5, 3, False)])
def test_the_writer_is_byte_exact(tmp_path, P, degree, unified):
    from moss_amd.checkpoint import write_ply
    pc = _model(P, degree, unified)
    assert len(_names(3)) == 62 and _rows(pc).shape == (P, len(_names(degree)))
    path = tmp_path / "sub" / "point_cloud.ply"
    write_ply(str(path), pc)
    assert path.read_bytes() == _expected_bytes(pc, degree)
    pc.save_ply(str(tmp_path / "again.ply"))
    assert (tmp_path / "again.ply").read_bytes() == _expected_bytes(pc, degree)
    # f_rest_{c ((D+1)^2 - 1) + (j - 1)} = features[:, j, c], one element named by hand
    k1 = (degree + 1) ** 2 - 1
    assert _rows(pc)[0, 9 + 2 * k1 + (k1 - 1)] == float(pc.get_features.detach()[0, k1, 2])


@pytest.mark.parametrize("unified", [True, False])
def test_round_trip_gives_every_parameter_back(tmp_path, unified):
    src, dst = _model(7, 3, unified, seed=1), _model(4, 3, unified, seed=2)
    dst.active_sh_degree, dst.spatially_ordered = 1, True
    objects = [id(p) for p in dst.parameters()]
    src.save_ply(str(tmp_path / "a.ply"))
    dst.load_ply(str(tmp_path / "a.ply"))
    assert [id(p) for p in dst.parameters()] == objects
    for (n, a), (_, b) in zip(src.named_parameters(), dst.named_parameters()):
        assert a.shape == b.shape and torch.equal(a, b) and b.requires_grad, n
    assert dst.active_sh_degree == dst.max_sh_degree == 3 and dst.spatially_ordered is False
    dst.save_ply(str(tmp_path / "b.ply"))
    assert (tmp_path / "a.ply").read_bytes() == (tmp_path / "b.ply").read_bytes()


def test_load_ply_through_the_optimizers_row_surgery(tmp_path):
    """Into a model whose parameters live in two FlatAdamW (the layout of MossStep) at another row count: the Parameter objects
    survive, the values are the file's, the moments of the loaded rows are zero, the other optimizer state is untouched."""
    from moss_amd import dist as mdist
    from moss_amd.optim import FlatAdamW, FlatAdamWRows
    src, dst = _model(9, 3, seed=3), _model(4, 3, seed=4)
    groups = {g["name"]: g for g in dst.param_groups()}
    four = ("features", "opacity", "scaling", "rotation")
    other = torch.nn.Parameter(torch.arange(5.0))
    a = FlatAdamW([groups[n] for n in four], mdist.GradBucket([groups[n]["params"][0] for n in four]), capturable=True)
    b = FlatAdamW([groups["xyz"], {"params": [other], "lr": 1e-3, "name": "other"}], mdist.GradBucket([dst._xyz, other]), capturable=True)
    for o in (a, b):
        o.exp_avg.fill_(0.5); o.exp_avg_sq.fill_(0.25)
    a.set_active_sh_degree(1)
    rows = FlatAdamWRows([a, b])
    objects = [id(p) for p in dst.parameters()]
    src.save_ply(str(tmp_path / "a.ply"))
    dst.load_ply(str(tmp_path / "a.ply"), optimizer=rows)
    assert [id(p) for p in dst.parameters()] == objects and rows.rows == 9 and a.sh_active_degree == 3
    for (n, p), (_, q) in zip(src.named_parameters(), dst.named_parameters()):
        assert torch.equal(p, q), n
        assert q.data_ptr() >= (a if n != "_xyz" else b).flat_params.data_ptr()
    assert not bool(a.exp_avg.any()) and not bool(a.exp_avg_sq.any())
    m, v = b._moments_of(0)
    assert m.shape == (9, 3) and not bool(m.any()) and not bool(v.any())
    m, v = b._moments_of(1)
    assert torch.equal(other.detach(), torch.arange(5.0)) and bool((m == 0.5).all()) and bool((v == 0.25).all())


# ---- the reader -----------------------------------------------------------------------------------------------------------------------
def _ascii(names, types, rows, comments=()):
    lines = ["ply", "format ascii 1.0"] + ["comment %s" % c for c in comments] + ["element vertex %d" % len(rows)]
    lines += ["property %s %s" % (t, n) for n, t in zip(names, types)] + ["end_header"]
    lines += [" ".join(("%d" % v) if t == "uchar" else repr(float(v)) for v, t in zip(r, types)) for r in rows]
    return ("\n".join(lines) + "\n").encode("ascii")


def _binary(names, types, columns, fmt="binary_little_endian", extra_header=()):
    code = {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8", "uchar": "u1"}
    table = np.empty(len(columns[0]), dtype=[(n, code[t]) for n, t in zip(names, types)])
    for n, c in zip(names, columns):
        table[n] = c
    lines = ["ply", "format %s 1.0" % fmt] + list(extra_header) + ["element vertex %d" % len(table)]
    lines += ["property %s %s" % (t, n) for n, t in zip(names, types)] + ["end_header"]
    return ("\n".join(lines) + "\n").encode("ascii") + table.tobytes()


def test_the_reader_is_lenient_where_the_issue_says(tmp_path):
    from moss_amd.checkpoint import read_ply
    pc = _model(6, 3, seed=5)
    names, rows = _names(3), _rows(pc).astype(np.float32)
    base = tmp_path / "base.ply"
    pc.save_ply(str(base))
    want = read_ply(str(base))
    assert list(want) == names and all(v.dtype == np.float32 and v.shape == (6,) for v in want.values())
    for i, n in enumerate(names):
        assert np.array_equal(want[n], rows[:, i]), n
    perm = list(np.random.default_rng(0).permutation(len(names)))
    cols = [rows[:, i] for i in range(len(names))]
    variants = {
        "ascii": _ascii(names, ["float"] * 62, rows),
        "permuted": _binary([names[i] for i in perm], ["float"] * 62, [cols[i] for i in perm]),
        "extra_uchar": _binary(names[:3] + ["red"] + names[3:], ["float"] * 3 + ["uchar"] + ["float"] * 59,
                               cols[:3] + [np.arange(6, dtype=np.uint8)] + cols[3:]),
        "float32_spelled": _binary(names, ["float32"] * 62, cols),
        "comments": _binary(names, ["float"] * 62, cols, extra_header=["comment made by hand", "obj_info nothing", "comment two"]),
        "ascii_comments_uchar": _ascii(names + ["red"], ["float"] * 62 + ["uchar"], np.concatenate((rows, np.full((6, 1), 7.0)), axis=1),
                                       comments=["one"]),
        "double": _binary(names, ["double"] * 62, [c.astype(np.float64) for c in cols]),
        "float64_spelled": _binary(names, ["float64"] * 62, [c.astype(np.float64) for c in cols]),
    }
    for what, blob in variants.items():
        path = tmp_path / (what + ".ply")
        path.write_bytes(blob)
        got = read_ply(str(path))
        assert set(got) == set(names), what
        for n in names:
            assert got[n].dtype == np.float32 and np.array_equal(got[n], want[n]), (what, n)
        dst = _model(2, 3, seed=6)
        dst.load_ply(str(path))
        for (n, a), (_, b) in zip(pc.named_parameters(), dst.named_parameters()):
            assert torch.equal(a, b), (what, n)
    # a double that float32 cannot hold is read to the float32 of its value
    third = np.array([1.0 / 3.0, 1e-50, 2.0 ** 40 + 1.0])
    (tmp_path / "d.ply").write_bytes(_binary(["x"], ["double"], [third]))
    assert np.array_equal(read_ply(str(tmp_path / "d.ply"))["x"], third.astype(np.float32))


def test_the_reader_refuses_and_names_what_it_found(tmp_path):
    from moss_amd.checkpoint import read_ply
    pc = _model(3, 3, seed=7)
    names, rows = _names(3), _rows(pc).astype(np.float32)
    cols = [rows[:, i] for i in range(62)]
    path = tmp_path / "bad.ply"
    # big-endian
    path.write_bytes(_binary(names, ["float"] * 62, cols, fmt="binary_big_endian"))
    with pytest.raises(ValueError, match="binary_big_endian"):
        read_ply(str(path))
    # a list property
    blob = _binary(names, ["float"] * 62, cols).replace(b"property float nx\n", b"property list uchar int vertex_indices\n")
    path.write_bytes(blob)
    with pytest.raises(ValueError, match="list uchar int vertex_indices"):
        read_ply(str(path))
    # an unknown type, no PLY at all, a truncated body, another first element
    path.write_bytes(_binary(names, ["float"] * 62, cols).replace(b"property float nx\n", b"property half nx\n"))
    with pytest.raises(ValueError, match="half"):
        read_ply(str(path))
    path.write_bytes(b"solid not a ply\n")
    with pytest.raises(ValueError, match="solid"):
        read_ply(str(path))
    path.write_bytes(_binary(names, ["float"] * 62, cols)[:-5])
    with pytest.raises(ValueError, match="truncated"):
        read_ply(str(path))
    path.write_bytes(_binary(names, ["float"] * 62, cols).replace(b"element vertex 3\n", b"element face 3\n"))
    with pytest.raises(ValueError, match="face 3"):
        read_ply(str(path))
    # a missing attribute; an attribute that is there but not as a float; the model stays as it was
    for gone, types in (("opacity", None), ("rot_2", None), ("y", "uchar")):
        keep = [i for i, n in enumerate(names) if n != gone or types]
        kinds = [types if (types and names[i] == gone) else "float" for i in keep]
        target = _model(2, 3, seed=8)
        before = [p.detach().clone() for p in target.parameters()]
        path.write_bytes(_binary([names[i] for i in keep], kinds, [cols[i].astype(np.uint8) if k == "uchar" else cols[i] for i, k in zip(keep, kinds)]))
        with pytest.raises(ValueError, match=("rot_" if gone == "rot_2" else "'%s'" % gone)):
            target.load_ply(str(path))
        assert all(torch.equal(a, b) for a, b in zip(before, target.parameters())) and target._xyz.shape[0] == 2
    # an f_rest count that is not 3 ((D+1)^2 - 1) for the model's max_sh_degree: a degree-1 file into a degree-3 model and back
    low = _model(3, 1, seed=9)
    low.save_ply(str(path))
    with pytest.raises(ValueError, match=r"9 properties f_rest_\*.*f_rest_0\.\.44.*max_sh_degree = 3"):
        _model(2, 3, seed=8).load_ply(str(path))
    pc.save_ply(str(path))
    with pytest.raises(ValueError, match=r"45 properties f_rest_\*.*f_rest_0\.\.8.*max_sh_degree = 1"):
        low.load_ply(str(path))
    # ... and a gap in the numbering
    path.write_bytes(_binary(names, ["float"] * 62, cols).replace(b"property float f_rest_7\n", b"property float f_rest_77\n"))
    with pytest.raises(ValueError, match="f_rest_"):
        _model(2, 3, seed=8).load_ply(str(path))


# ---- the model directory --------------------------------------------------------------------------------------------------------------
def _with_networks(pc, seed):
    from moss_amd import lbs_weights as mlw
    from moss_amd import pose as mpose
    torch.manual_seed(seed)
    pc.auto_regression, pc.cross_attention_lbs, pc.motion_offset_flag = mpose.head_module(init_val=0.1), mlw.lbs_weight_module(), True
    return pc


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_save_scene_and_load_scene_keep_to_MOSS_layout(tmp_path):
    from moss_amd import lbs_weights as mlw
    from moss_amd import pose as mpose
    from moss_amd.checkpoint import load_scene, save_scene
    root = str(tmp_path / "model")
    a7, a30 = _with_networks(_model(5, 3, seed=10), 1), _with_networks(_model(8, 3, seed=11), 2)
    save_scene(root, 7, a7)
    assert _files(root) == ["mlp_ckpt/iteration_7/ckpt.pth", "point_cloud/iteration_7/point_cloud.ply"]       # exactly the two paths
    save_scene(root, 30, a30)
    ckpt = torch.load(os.path.join(root, "mlp_ckpt/iteration_30/ckpt.pth"), weights_only=True)
    assert sorted(ckpt) == ["Autoregression", "CrossAttention_lbs", "iter"] and ckpt["iter"] == 30 and type(ckpt["iter"]) is int
    assert tuple(ckpt["Autoregression"]) == mpose.PARAM_NAMES == tuple(a30.auto_regression.state_dict())
    assert set(ckpt["CrossAttention_lbs"]) == set(a30.cross_attention_lbs.state_dict()) and len(ckpt["CrossAttention_lbs"]) == 20
    assert all(n in ckpt["CrossAttention_lbs"] for n in mlw.UNUSED_NAMES)
    for key, module in (("Autoregression", a30.auto_regression), ("CrossAttention_lbs", a30.cross_attention_lbs)):
        for n, v in module.state_dict().items():
            assert ckpt[key][n].device.type == "cpu" and torch.equal(ckpt[key][n], v), (key, n)
    # -1 is the largest iteration
    b = _with_networks(_model(2, 3, seed=12), 3)
    tensors = [id(p) for p in b.auto_regression.parameters()]
    assert load_scene(root, b) == 30 and b._xyz.shape[0] == 8
    assert [id(p) for p in b.auto_regression.parameters()] == tensors                    # copied into the module's own tensors
    for x, y in zip(list(a30.parameters()), list(b.parameters())):
        assert torch.equal(x, y)
    assert load_scene(root, b, iteration=7) == 7 and b._xyz.shape[0] == 5
    for x, y in zip(list(a7.parameters()), list(b.parameters())):
        assert torch.equal(x, y)
    # without the flag only the PLY is written and read
    plain = _model(3, 3, seed=13)
    plain.motion_offset_flag = False
    save_scene(str(tmp_path / "plain"), 1, plain)
    assert _files(str(tmp_path / "plain")) == ["point_cloud/iteration_1/point_cloud.ply"]
    # strict
    path = os.path.join(root, "mlp_ckpt/iteration_30/ckpt.pth")
    torch.save({"iter": 30, "Autoregression": ckpt["Autoregression"]}, path)
    c = _with_networks(_model(2, 3, seed=14), 4)
    mine = [p.detach().clone() for p in c.cross_attention_lbs.parameters()]
    with pytest.raises(KeyError, match="CrossAttention_lbs"):
        load_scene(root, c, 30)
    with pytest.warns(UserWarning, match="CrossAttention_lbs"):
        assert load_scene(root, c, 30, strict=False) == 30
    assert all(torch.equal(x, y) for x, y in zip(mine, c.cross_attention_lbs.parameters()))
    assert all(torch.equal(x, y) for x, y in zip(a30.auto_regression.parameters(), c.auto_regression.parameters()))
    short = dict(ckpt["CrossAttention_lbs"])
    del short["gate_proj.bias"]
    torch.save({"iter": 30, "Autoregression": ckpt["Autoregression"], "CrossAttention_lbs": short}, path)
    with pytest.raises(RuntimeError, match="gate_proj.bias"):
        load_scene(root, c, 30)
    os.remove(path)
    with pytest.raises(FileNotFoundError, match="ckpt.pth"):
        load_scene(root, c, 30)
    with pytest.warns(UserWarning, match="ckpt.pth"):
        load_scene(root, c, 30, strict=False)
    with pytest.raises(FileNotFoundError):
        load_scene(root, c, 31)
    with pytest.raises(FileNotFoundError):
        load_scene(str(tmp_path / "nowhere"), c)


# ---- the optimizer's state ------------------------------------------------------------------------------------------------------------
def test_flat_adamw_state_dict_is_plain_and_loads_bit_for_bit(tmp_path):
    from moss_amd import dist as mdist
    from moss_amd.optim import FlatAdamW

    def build(seed, rows=5):
        pc = _model(rows, 3, seed=seed)
        groups = {g["name"]: g for g in pc.param_groups()}
        four = ("features", "opacity", "scaling", "rotation")
        return pc, FlatAdamW([groups[n] for n in four], mdist.GradBucket([groups[n]["params"][0] for n in four]), capturable=True)
    pa, a = build(20)
    g = torch.Generator().manual_seed(3)
    a.exp_avg.copy_(torch.randn(a.exp_avg.shape, generator=g)); a.exp_avg_sq.copy_(torch.rand(a.exp_avg_sq.shape, generator=g))
    a.step_state.copy_(torch.arange(a.step_state.numel(), dtype=torch.int32) + 5)
    a.t = 9
    a.seg_lr[0], a.seg_lr2[0], a.seg_lr[2] = 1.25e-3, 7e-5, 0.3
    a.sh_active_degree, a.sh_inactive_zero = 2, False
    torch.save(a.state_dict(), str(tmp_path / "o.pth"))
    sd = torch.load(str(tmp_path / "o.pth"), weights_only=True)
    assert all(v.device.type == "cpu" for v in sd.values() if torch.is_tensor(v))
    pb, b = build(21)
    objects = [id(p) for p in pb.parameters()]
    at = b.flat_params.data_ptr()
    b.load_state_dict(sd)
    assert b.flat_params.data_ptr() == at and [id(p) for p in pb.parameters()] == objects
    for k in ("flat_params", "exp_avg", "exp_avg_sq", "step_state"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert b.t == 9 and list(b.seg_lr) == list(a.seg_lr) and list(b.seg_lr2) == list(a.seg_lr2)
    assert (b.sh_active_degree, b.sh_inactive_zero) == (2, False) and b.step_count() == 5
    for x, y in zip(a.bucket.params, b.bucket.params):
        assert torch.equal(x, y)                                                     # (through the Parameter objects)
    # another layout is refused by name and nothing changes
    pc_, c = build(22, rows=6)
    before = (c.flat_params.clone(), c.exp_avg.clone(), c.step_state.clone())
    with pytest.raises(ValueError, match="shapes"):
        c.load_state_dict(sd)
    assert torch.equal(before[0], c.flat_params) and torch.equal(before[1], c.exp_avg) and torch.equal(before[2], c.step_state) and c.t == 0
    # a sharded optimizer has no whole state
    ps = [torch.nn.Parameter(torch.randn(40))]
    sharded = FlatAdamW([{"params": ps, "lr": 1e-3}], mdist.GradBucket(ps, world=2), capturable=True, shard=(0, 2))
    with pytest.raises(NotImplementedError):
        sharded.state_dict()


# ---- the loop -------------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """What ``run_schedule`` touches of a MossStep, recording every call in order."""

    def __init__(self, captured):
        self.calls = []
        self.pc = SimpleNamespace(active_sh_degree=0, max_sh_degree=3, _xyz=torch.zeros(4, 3))
        self.graphed = object() if captured else None
        self.dropped_frames = self.recaptures = 0

    def __call__(self):
        self.calls.append(("replay",))

    def compute(self):
        self.calls.append(("compute",))

    def set_learning_rates(self, rates):
        self.calls.append(("lr", rates["xyz"]))

    def oneup_sh_degree(self):
        self.pc.active_sh_degree = min(self.pc.active_sh_degree + 1, 3)
        self.calls.append(("sh",))
        return self.pc.active_sh_degree

    def densification_event(self, reset_opacity=False):
        self.calls.append(("reset_opacity",))

    def check(self):
        self.calls.append(("check",))


def _run(captured, **kw):
    from moss_amd.train import run_schedule
    step = _Recorder(captured)

    def on_event(s, i):
        s.calls.append(("event", i))
        return {"rows_after": 4}
    args = dict(densify_from=4, densify_until=17, interval=3, sh_every=5, opacity_reset_interval=12, check_every=4,
                lr_schedule=lambda i: {"xyz": float(i)}, on_event=on_event, load_frame=lambda k: step.calls.append(("frame", k)), seed=3)
    args.update(kw)
    report = run_schedule(step, [10, 11, 12], 20, **args)
    return step.calls, report


def _written_out(captured, first, saving=()):
    """The loop of ``run_schedule``'s docstring, written out for iterations first..20 of the miniature schedule."""
    from moss_amd.train import frame_order
    order, calls = frame_order(3, 20, 3), []
    for i in range(first, 21):
        calls.append(("lr", float(i)))
        if i % 5 == 0:
            calls.append(("sh",))
        calls.append(("frame", [10, 11, 12][order[i - 1]]))
        calls.append(("replay",) if captured else ("compute",))
        if i < 17:
            if i > 4 and i % 3 == 0:
                calls.append(("event", i))
            if i % 12 == 0:
                calls.append(("reset_opacity",))
        if i in saving:
            calls.append(("save", i))
        if captured and i % 4 == 0:
            calls.append(("check",))
    return calls + ([("check",)] if captured else [])


@pytest.mark.parametrize("captured", [False, True])
def test_run_schedule_entered_at_k_and_saving(captured):
    from moss_amd.train import frame_order
    # the defaults make the calls the loop always made
    calls, report = _run(captured)
    assert calls == _written_out(captured, 1)
    assert [c[1] for c in calls if c[0] == "frame"] == [[10, 11, 12][k] for k in frame_order(3, 20, 3)]
    assert [e["iteration"] for e in report["events"]] == [6, 9, 12, 15] and report["sh_raises"] == 3 and report["opacity_resets"] == 1
    assert [report["phases"][k]["iterations"] for k in ("before", "during", "after")] == [4, 12, 4]
    # entered at k = 8
    saved = []
    save = lambda s, i: (saved.append(i), s.calls.append(("save", i)))
    calls8, report8 = _run(captured, start_iteration=8, saving_iterations=(9, 12, 20, 3), save=save)
    assert calls8 == _written_out(captured, 8, saving=(9, 12, 20))
    assert [c[1] for c in calls8 if c[0] == "frame"] == [[10, 11, 12][k] for k in frame_order(3, 20, 3)[7:]]
    assert saved == [9, 12, 20] and calls8[calls8.index(("save", 9)) - 1] == ("event", 9)
    assert calls8[calls8.index(("save", 12)) - 2:calls8.index(("save", 12))] == [("event", 12), ("reset_opacity",)]
    assert [e["iteration"] for e in report8["events"]] == [9, 12, 15] and report8["sh_raises"] == 3 and report8["opacity_resets"] == 1
    assert calls8.count(("sh",)) == 3 and calls.count(("sh",)) == 4               # at 10, 15, 20 only
    assert [report8["phases"][k]["iterations"] for k in ("before", "during", "after")] == [0, 9, 4] and report8["iterations"] == 20
    # iterations 1..7 and then 8..20 make the calls of the whole run (the end-of-run check aside)
    whole, _ = _run(captured, check_every=100)
    tail, _ = _run(captured, check_every=100, start_iteration=8)
    cut = whole.index(("lr", 8.0))
    assert whole[cut:] == tail and cut > 0
    # entered in the last phase; entered behind the end; refusals
    _, r18 = _run(captured, start_iteration=18)
    assert [r18["phases"][k]["iterations"] for k in ("before", "during", "after")] == [0, 0, 3] and r18["events"] == []
    calls21, r21 = _run(captured, start_iteration=21)
    assert [c for c in calls21 if c[0] != "check"] == [] and sum(p["iterations"] for p in r21["phases"].values()) == 0
    with pytest.raises(ValueError, match="start_iteration"):
        _run(captured, start_iteration=0)
    with pytest.raises(ValueError, match="save="):
        _run(captured, saving_iterations=(5,))
