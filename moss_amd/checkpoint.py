"""Keeping what ``moss_amd.train.MossStep`` trained: MOSS's PLY and model directory, and the step's training state.  No kernel: the flat
buffers are contiguous and each crosses to the host whole, once per hundreds of steps.

    write_ply / read_ply            MOSS's ``point_cloud.ply`` (``GaussianModel.save_ply / load_ply``, scene/gaussian_model.py:271-360) without
                                    ``plyfile``; ``GaussianSet.save_ply / load_ply`` are these on a model
    save_scene / load_scene         MOSS's model directory (``Scene.save``, scene/__init__.py:86-123): what ``render_ZJU.py`` reads
    save_checkpoint / load_checkpoint   ``MossStep.state_dict()`` in a file: stop a run and continue it, bit for bit
    save_pose_tables / load_pose_tables The per-pose LBS tables of an evaluation (``play.evaluate_split``): MOSS's ``smpl_rot`` folder

Every file that holds tensors is written by ``torch.save`` with tensors on the CPU and plain containers only, so
``torch.load(..., weights_only=True)`` reads it.  Everything here imports and runs without a GPU.
"""
from __future__ import annotations

import os
import re
import warnings

import numpy as np
import torch

__all__ = ["write_ply", "read_ply", "ply_attributes", "ply_rows", "gaussians_from_ply", "resize_rows", "assign_rows", "save_scene",
           "load_scene", "latest_iteration", "save_checkpoint", "load_checkpoint", "CHECKPOINT_FORMAT", "save_pose_tables", "load_pose_tables",
           "POSE_TABLES_FORMAT"]

CHECKPOINT_FORMAT = "moss_amd.checkpoint"

# PLY scalar type names (both spellings) -> numpy codes without byte order
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


# ---- MOSS's PLY ----------------------------------------------------------------------------------------------------------------------
def ply_attributes(coefficients: int):
    """``construct_list_of_attributes`` (scene/gaussian_model.py:271-283) for ``coefficients`` = (D + 1)^2 SH coefficients per colour:
    ``x y z nx ny nz f_dc_0..2 f_rest_0..(3 (coefficients - 1) - 1) opacity scale_0..2 rot_0..3`` -- 62 names at degree 3."""
    k = int(coefficients)
    return (["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)] + [f"f_rest_{i}" for i in range(3 * (k - 1))]
            + ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)])


def _host(t):
    return t.detach().to("cpu", torch.float32).numpy()


def ply_rows(pc):
    """The (P, 17 + 3 (D + 1)^2 - 3) float32 table of ``save_ply`` (:289-300), columns in :func:`ply_attributes` order: the raw parameters
    (logit opacity, log scale, unnormalised rotation), zero normals, ``f_rest_{c ((D+1)^2 - 1) + (j - 1)} = features[:, j, c]`` -- the
    reference's ``transpose(1, 2).flatten(start_dim=1)``.  One device-to-host copy per parameter tensor; the columns are placed on the
    host, as whole slices."""
    if getattr(pc, "unified_features", False):
        feats = _host(pc._features)                          # (P, K, 3), one copy
        dc, rest = feats[:, :1, :], feats[:, 1:, :]
    else:
        dc, rest = _host(pc._features_dc), _host(pc._features_rest)
    xyz, opacity, scale, rot = _host(pc._xyz), _host(pc._opacity), _host(pc._scaling), _host(pc._rotation)
    P, k = int(xyz.shape[0]), int(dc.shape[1] + rest.shape[1])
    if k != (int(pc.max_sh_degree) + 1) ** 2:
        raise ValueError(f"write_ply: the model holds {k} SH coefficients per colour and max_sh_degree = {pc.max_sh_degree} asks for "
                         f"{(int(pc.max_sh_degree) + 1) ** 2}")
    rows = np.zeros((P, 17 + 3 * (k - 1)), dtype="<f4")
    rows[:, 0:3] = xyz                                       # (3:6, the normals, stay zero)
    rows[:, 6:9] = dc.transpose(0, 2, 1).reshape(P, -1)
    rows[:, 9:9 + 3 * (k - 1)] = rest.transpose(0, 2, 1).reshape(P, -1)
    at = 9 + 3 * (k - 1)
    rows[:, at:at + 1] = opacity.reshape(P, 1)
    rows[:, at + 1:at + 4] = scale
    rows[:, at + 4:at + 8] = rot
    return rows


def _replace(path, write):
    """``write(file)`` into a sibling of ``path`` that then takes its place: a reader never finds half a file."""
    folder = os.path.dirname(os.path.abspath(path))
    os.makedirs(folder, exist_ok=True)
    tmp = f"{path}.part"
    with open(tmp, "wb") as f:
        write(f)
    os.replace(tmp, path)


def write_ply(path, pc):
    """``pc.save_ply(path)`` of MOSS's ``GaussianModel``: binary little-endian, byte for byte what ``plyfile`` writes there -- the header
    ``ply / format binary_little_endian 1.0 / element vertex P / property float NAME ... / end_header`` and P rows of float32
    (:func:`ply_rows`).  The folder is created."""
    rows = ply_rows(pc)
    names = ply_attributes((int(pc.max_sh_degree) + 1) ** 2)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % rows.shape[0]
    header += "".join(f"property float {n}\n" for n in names) + "end_header\n"
    _replace(path, lambda f: (f.write(header.encode("ascii")), f.write(rows.tobytes())))


def read_ply(path):
    """The float properties of a PLY file's ``vertex`` element as ``{name: float32 array (P,)}``, in the file's order.

    Read: ``format ascii`` and ``binary_little_endian``; ``float`` / ``float32`` and ``double`` / ``float64`` properties (doubles are
    converted); ``comment`` and ``obj_info`` lines; properties in any order; properties of the other scalar types are stepped over
    and not returned; elements behind ``vertex`` are ignored.  Anything else raises ``ValueError`` that names what was found: another
    format (``binary_big_endian``), a ``list`` property, an unknown type name, a first element that is not ``vertex``, a file shorter
    than its header promises.  There is no second reader to fall back on."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    stop = data.find(b"\n", end) if end >= 0 else -1
    if not data.startswith(b"ply") or stop < 0:
        raise ValueError(f"read_ply: {path} is no PLY file (it starts with {data[:16]!r})")
    fmt, count, props, element = None, None, [], None
    for line in data[:stop].decode("ascii", "replace").splitlines()[1:]:
        words = line.split()
        if not words or words[0] in ("comment", "obj_info", "end_header"):
            continue
        if words[0] == "format":
            fmt = words[1] if len(words) > 1 else ""
            if fmt not in ("ascii", "binary_little_endian"):
                raise ValueError(f"read_ply: format '{fmt}' is not read (ascii and binary_little_endian are)")
        elif words[0] == "element":
            if element is None and (len(words) != 3 or words[1] != "vertex"):
                raise ValueError(f"read_ply: the first element is '{' '.join(words[1:])}', not 'vertex P'")
            if element is None:
                count = int(words[2])
            element = words[1] if element is None else "behind"
        elif words[0] == "property":
            if element is None:
                raise ValueError(f"read_ply: '{line}' stands before any element")
            if element != "vertex":
                continue
            if len(words) > 1 and words[1] == "list":
                raise ValueError(f"read_ply: '{line}': a list property in the vertex element is not read")
            if len(words) != 3 or words[1] not in _PLY_TYPES:
                raise ValueError(f"read_ply: '{line}': unknown property type '{words[1] if len(words) > 1 else ''}'")
            props.append((words[2], _PLY_TYPES[words[1]]))
        else:
            raise ValueError(f"read_ply: header line '{line}' is not understood")
    if fmt is None or count is None:
        raise ValueError(f"read_ply: the header has no {'format' if fmt is None else 'element vertex'} line")
    if len({n for n, _ in props}) != len(props):
        raise ValueError("read_ply: a property name appears twice in the vertex element")
    body = stop + 1
    if fmt == "ascii":
        tokens = data[body:].split()
        if len(tokens) < count * len(props):
            raise ValueError(f"read_ply: {len(tokens)} values for {count} vertices of {len(props)} properties: the file is truncated")
        table = np.array(tokens[:count * len(props)], dtype=np.float64).reshape(count, len(props))
        columns = {n: table[:, i] for i, (n, _) in enumerate(props)}
    else:
        dtype = np.dtype([(n, "<" + t) for n, t in props])
        if len(data) - body < count * dtype.itemsize:
            raise ValueError(f"read_ply: {len(data) - body} bytes for {count} vertices of {dtype.itemsize} bytes: the file is truncated")
        table = np.frombuffer(data, dtype=dtype, count=count, offset=body)
        columns = {n: table[n] for n, _ in props}
    return {n: np.ascontiguousarray(columns[n], dtype=np.float32) for n, t in props if t in ("f4", "f8")}


def gaussians_from_ply(arrays, max_sh_degree):
    """``load_ply`` (scene/gaussian_model.py:319-360) on what :func:`read_ply` returned: properties looked up by name, ``f_rest_*`` /
    ``scale_*`` / ``rot_*`` sorted by their numeric suffix.  Returns float32 CPU tensors ``xyz (P,3)``, ``features (P,(D+1)^2,3)``,
    ``opacity (P,1)``, ``scaling (P,3)``, ``rotation (P,4)``.  A missing attribute, or an ``f_rest`` count that is not
    ``3 ((D+1)^2 - 1)`` for ``max_sh_degree`` (the reference asserts it, :334), raises ``ValueError`` naming it."""
    def column(name):
        if name not in arrays:
            raise ValueError(f"load_ply: the file has no float property '{name}' (it has: {' '.join(arrays) or 'none'})")
        return arrays[name]

    def numbered(prefix, want):
        names = sorted((n for n in arrays if re.fullmatch(re.escape(prefix) + r"\d+", n)), key=lambda n: int(n.rsplit("_", 1)[1]))
        if names != [f"{prefix}{i}" for i in range(want)]:
            raise ValueError(f"load_ply: {len(names)} properties {prefix}* ({' '.join(names[:4])}{' ...' if len(names) > 4 else ''}) where "
                             f"{prefix}0..{want - 1} are expected" + (f" for max_sh_degree = {max_sh_degree}" if prefix == "f_rest_" else ""))
        return np.stack([arrays[n] for n in names], axis=1) if names else np.zeros((len(column("x")), 0), np.float32)
    k = (int(max_sh_degree) + 1) ** 2
    xyz = np.stack([column(n) for n in "xyz"], axis=1)
    P = xyz.shape[0]
    dc = np.stack([column(f"f_dc_{c}") for c in range(3)], axis=1)                 # (P, 3): colour c of coefficient 0
    rest = numbered("f_rest_", 3 * (k - 1)).reshape(P, 3, k - 1)                   # (P, colour, coefficient - 1)
    features = np.concatenate((dc[:, None, :], rest.transpose(0, 2, 1)), axis=1)   # (P, k, 3)
    out = {"xyz": xyz, "features": features, "opacity": column("opacity")[:, None], "scaling": numbered("scale_", 3),
           "rotation": numbered("rot_", 4)}
    return {n: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for n, v in out.items()}


def resize_rows(optimizer, rows_old, rows_new):
    """Give every row-parameter of a ``FlatAdamW`` / ``FlatAdamWRows`` (and both its moments) ``rows_new`` rows through the existing row
    surgery (``relayout_rows``: one gather launch on GPU tensors): the Parameter objects stay, the bucket and the fused step follow.
    The rows' CONTENT is the caller's to overwrite (row r holds old row ``r mod rows_old``)."""
    rows_old, rows_new = int(rows_old), int(rows_new)
    if rows_new == rows_old:
        return
    if rows_old < 1 or rows_new < 1:
        raise ValueError(f"resize_rows: {rows_old} -> {rows_new} rows (both must be positive)")
    dev = optimizer.bucket.params[0].device
    row_map = (torch.arange(rows_new, dtype=torch.int64, device=dev) % rows_old).to(torch.int32)
    optimizer.relayout_rows(row_map, check=False, rows_old=rows_old)


def assign_rows(pc, values, optimizer=None):
    """The model takes ``values`` (``xyz``, ``features``, ``opacity``, ``scaling``, ``rotation``: :func:`gaussians_from_ply`) as its
    parameters.  Without an optimizer each Parameter's ``.data`` becomes the new tensor, at the new row count.  With a ``FlatAdamW`` /
    ``FlatAdamWRows`` the rows are re-laid by :func:`resize_rows`, then overwritten in the flat buffers, and both moments of these
    parameters are zeroed: they are new Gaussians to the optimizer, as after MOSS's ``load_ply`` + ``training_setup``."""
    dev = pc._xyz.device
    feats = values["features"]
    if getattr(pc, "unified_features", False):
        targets = [(pc._features, feats)]
    else:
        targets = [(pc._parameters["_features_dc"], feats[:, :1, :]), (pc._parameters["_features_rest"], feats[:, 1:, :])]
    targets += [(pc._xyz, values["xyz"]), (pc._opacity, values["opacity"]), (pc._scaling, values["scaling"]), (pc._rotation, values["rotation"])]
    for p, v in targets:
        if tuple(p.shape[1:]) != tuple(v.shape[1:]):
            raise ValueError(f"load_ply: rows of shape {tuple(v.shape[1:])} for a parameter of rows {tuple(p.shape[1:])}")
    with torch.no_grad():
        if optimizer is None:
            for p, v in targets:
                p.data = v.to(dev).contiguous().clone()
                p.grad = None
            return
        members = getattr(optimizer, "members", [optimizer])
        held = {id(q): (o, i) for o in members for i, q in enumerate(o.bucket.params)}
        missing = [tuple(p.shape) for p, _ in targets if id(p) not in held]
        if missing:
            raise ValueError(f"load_ply: the optimizer does not hold the model's parameter of shape {missing[0]}")
        resize_rows(optimizer, int(pc._xyz.shape[0]), int(values["xyz"].shape[0]))
        for p, v in targets:
            o, i = held[id(p)]
            p.data.copy_(v.to(dev))
            for m in o._moments_of(i):
                m.zero_()
            p.grad = None


# ---- MOSS's model directory -----------------------------------------------------------------------------------------------------------
def _ply_path(model_path, iteration):
    return os.path.join(model_path, "point_cloud", f"iteration_{int(iteration)}", "point_cloud.ply")


def _mlp_path(model_path, iteration):
    return os.path.join(model_path, "mlp_ckpt", f"iteration_{int(iteration)}", "ckpt.pth")


def _cpu_state(module):
    return {k: v.detach().to("cpu", copy=True) for k, v in module.state_dict().items()}


def save_scene(model_path, iteration, pc):
    """``Scene.save(iteration)`` (scene/__init__.py:109-123): ``point_cloud/iteration_N/point_cloud.ply`` (:func:`write_ply`) and, when
    ``pc.motion_offset_flag`` is set, ``mlp_ckpt/iteration_N/ckpt.pth`` = ``{'iter': N, 'Autoregression': ..., 'CrossAttention_lbs':
    ...}`` with the modules' FULL state_dicts (``out_layer`` / ``gate_proj`` included: MOSS's ``load_state_dict`` is strict) as plain
    dicts of CPU tensors.  ``render_ZJU.py --iteration N`` on ``model_path`` reads exactly these two files.  Returns the two paths
    (the second None without the flag)."""
    ply = _ply_path(model_path, iteration)
    write_ply(ply, pc)
    if not getattr(pc, "motion_offset_flag", False):
        return ply, None
    ckpt = _mlp_path(model_path, iteration)
    payload = {"iter": int(iteration), "Autoregression": _cpu_state(pc.auto_regression),
               "CrossAttention_lbs": _cpu_state(pc.cross_attention_lbs)}
    _replace(ckpt, lambda f: torch.save(payload, f))
    return ply, ckpt


def latest_iteration(folder):
    """``searchForMaxIteration`` (utils/system_utils.py): the largest N among the ``iteration_N`` entries of ``folder``."""
    found = [int(m.group(1)) for m in (re.fullmatch(r"iteration_(\d+)", n) for n in os.listdir(folder)) if m]
    if not found:
        raise FileNotFoundError(f"load_scene: no iteration_N under {folder}")
    return max(found)


def load_scene(model_path, pc, iteration=-1, strict=True, optimizer=None):
    """What MOSS's ``Scene`` does with ``load_iteration`` (scene/__init__.py:86-107): ``pc.load_ply`` of
    ``point_cloud/iteration_N/point_cloud.ply`` (``optimizer``: as there), then -- when ``pc.motion_offset_flag`` is set --
    ``load_state_dict`` of both networks from ``mlp_ckpt/iteration_N/ckpt.pth``.  ``iteration=-1``: the largest ``iteration_*`` under
    ``point_cloud/``.  A missing file or key raises; with ``strict=False`` a network file or entry that is missing or does not fit is
    skipped with a warning (the reference's ``try / except: print``).  Returns N.

    Nothing needs refreshing afterwards: ``load_state_dict`` copies into the modules' existing tensors (also where a ``FlatAdamW`` has
    re-homed them in its flat buffer), and the fused network ops (``lbs_weights.cross_attention_lbs_fused``, ``pose.pose_head_fused``)
    take the modules' tensors by address on every call -- neither keeps a packed or cached copy of the weights."""
    if int(iteration) == -1:
        iteration = latest_iteration(os.path.join(model_path, "point_cloud"))
    iteration = int(iteration)
    pc.load_ply(_ply_path(model_path, iteration), optimizer=optimizer)
    if not getattr(pc, "motion_offset_flag", False):
        return iteration
    path = _mlp_path(model_path, iteration)
    if not os.path.exists(path):
        if strict:
            raise FileNotFoundError(f"load_scene: {path} is missing (the model has motion_offset_flag set)")
        warnings.warn(f"load_scene: {path} is missing; both networks keep their weights")
        return iteration
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    for key, module in (("Autoregression", pc.auto_regression), ("CrossAttention_lbs", pc.cross_attention_lbs)):
        try:
            if key not in ckpt:
                raise KeyError(f"load_scene: {path} has no entry '{key}'")
            module.load_state_dict(ckpt[key])
        except (KeyError, RuntimeError) as err:
            if strict:
                raise
            warnings.warn(f"load_scene: missing {key} ({err}); the network keeps its weights")
    return iteration


# ---- the training state ---------------------------------------------------------------------------------------------------------------
def save_checkpoint(step, path, iteration, extra=None):
    """``step.state_dict()`` (a ``train.MossStep``: all it takes to continue the run bit for bit) with the iteration it was taken
    after, as one file that ``torch.load(path, weights_only=True)`` reads.  ``extra``: the caller's own state, tensors and plain
    containers only -- the place for the densification noise generator (``generator.get_state()``), which the step does not own.
    Not kept (``MossStep.state_dict``): the binning capacity, the captured graph, the frame inputs and ``lpips_reference``."""
    payload = {"format": CHECKPOINT_FORMAT, "iteration": int(iteration), "step": step.state_dict(), "extra": extra}
    _replace(path, lambda f: torch.save(payload, f))
    return path


def load_checkpoint(step, path):
    """``step.load_state_dict`` of a :func:`save_checkpoint` file; the step may have another number of Gaussians than the file and may
    be captured (it is captured again).  Returns ``(iteration, extra)``; continue with
    ``run_schedule(..., start_iteration=iteration + 1)``."""
    payload = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(payload, dict) or payload.get("format") != CHECKPOINT_FORMAT:
        raise ValueError(f"load_checkpoint: {path} is no {CHECKPOINT_FORMAT} file (format: "
                         f"{payload.get('format') if isinstance(payload, dict) else type(payload).__name__!r})")
    step.load_state_dict(payload["step"])
    return int(payload["iteration"]), payload["extra"]


# ---- the pose tables of an evaluation -------------------------------------------------------------------------------------------------
POSE_TABLES_FORMAT = "moss_amd.pose_tables"


def _pose_tables_dir(model_path, iteration):
    return os.path.join(model_path, "smpl_rot", f"iteration_{int(iteration)}")


def _checked_tables(tables_by_split):
    """``{split: {pose_id: {"transforms" (1,P,3,3), "translation" (1,P,3)}}}`` with exactly these two tensors per pose (MOSS's layout,
    ``train_ZJU.py:255-259``); raises ``ValueError`` naming the entry otherwise."""
    out = {}
    for split, poses in tables_by_split.items():
        out[split] = {}
        for pose_id, entry in poses.items():
            T, t = entry["transforms"], entry["translation"]
            if T.dim() != 4 or tuple(T.shape[::3]) != (1, 3) or T.shape[2] != 3 or tuple(t.shape) != (1, T.shape[1], 3):
                raise ValueError(f"save_pose_tables: {split}[{pose_id!r}]: transforms {tuple(T.shape)} / translation {tuple(t.shape)} are "
                                 "not (1,P,3,3) / (1,P,3)")
            out[split][pose_id] = {"transforms": T.detach(), "translation": t.detach()}
    return out


def save_pose_tables(model_path, iteration, tables_by_split, moss_pickle=False):
    """The per-pose LBS tables MOSS's ``training_report`` collects through ``render(..., return_smpl_rot=True)`` and ``render_ZJU.py``
    renders from (``train_ZJU.py:242-259,283-286``, ``render_ZJU.py:42-58``).  ``tables_by_split``: ``{"train": {pose_id:
    {"transforms" (1,P,3,3), "translation" (1,P,3)}}, "test": {...}}`` -- ``play.evaluate_split(...)["tables"]`` per split.

    Writes ``smpl_rot/iteration_N/pose_tables.pth``: the same nesting with CPU tensors and plain containers, read by
    ``torch.load(weights_only=True)`` (:func:`load_pose_tables`).  ``moss_pickle=True`` ALSO writes MOSS's own
    ``smpl_rot/iteration_N/smpl_rot.pickle`` -- ``pickle.dump(tables, f, protocol=pickle.HIGHEST_PROTOCOL)`` with the tensors on the
    device they are on: ``render_ZJU.py:77`` multiplies them with CUDA positions, so the file unpickles to what MOSS itself would have
    written.  Returns the path(s) written, as a tuple ``(pth, pickle or None)``."""
    tables = _checked_tables(tables_by_split)
    folder = _pose_tables_dir(model_path, iteration)
    pth = os.path.join(folder, "pose_tables.pth")
    payload = {"format": POSE_TABLES_FORMAT, "iteration": int(iteration),
               "tables": {split: {pid: {k: v.to("cpu", copy=True) for k, v in e.items()} for pid, e in poses.items()}
                          for split, poses in tables.items()}}
    _replace(pth, lambda f: torch.save(payload, f))
    pkl = None
    if moss_pickle:
        import pickle
        pkl = os.path.join(folder, "smpl_rot.pickle")
        _replace(pkl, lambda f: pickle.dump(tables, f, protocol=pickle.HIGHEST_PROTOCOL))
    return pth, pkl


def load_pose_tables(model_path, iteration=-1, device=None, trust_pickle=False):
    """Read what :func:`save_pose_tables` wrote: ``{split: {pose_id: {"transforms", "translation"}}}`` with the tensors on ``device``
    (None: the CPU).  ``model_path``: the model directory (``iteration=-1``: the largest ``iteration_*`` under ``smpl_rot/``) or the
    path of one file.  A ``.pickle`` -- MOSS's own file -- is refused unless ``trust_pickle=True``: unpickling runs whatever code the
    file names, so it is only for files you wrote yourself; ``pose_tables.pth`` beside it holds the same tables and is read with
    ``weights_only=True``."""
    path = model_path
    if os.path.isdir(model_path):
        if int(iteration) == -1:
            iteration = latest_iteration(os.path.join(model_path, "smpl_rot"))
        folder = _pose_tables_dir(model_path, iteration)
        path = os.path.join(folder, "pose_tables.pth")
        if not os.path.exists(path) and os.path.exists(os.path.join(folder, "smpl_rot.pickle")):
            path = os.path.join(folder, "smpl_rot.pickle")
    if str(path).endswith((".pickle", ".pkl")):
        if not trust_pickle:
            raise ValueError(f"load_pose_tables: {path} is a pickle, and unpickling executes code the file chooses: it is not read unless "
                             "trust_pickle=True says the file is your own (pose_tables.pth holds the same tables and is read safely)")
        import pickle
        with open(path, "rb") as f:
            tables = pickle.load(f)
    else:
        payload = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(payload, dict) or payload.get("format") != POSE_TABLES_FORMAT:
            raise ValueError(f"load_pose_tables: {path} is no {POSE_TABLES_FORMAT} file")
        tables = payload["tables"]
    dev = torch.device("cpu" if device is None else device)
    return {split: {pid: {k: v.to(dev) for k, v in e.items()} for pid, e in poses.items()} for split, poses in tables.items()}
