"""The refusals of the SMPL / LBS ops' Python surface, word for word: ``lbs_deform``, ``smpl_frame_fused``, ``posed_frame``,
``posed_vertices`` and ``bound_masks`` share one tensor checker, one body-model check and one frame-parameter check
(moss_amd/_checks.py), and a caller that matches on a message must not notice.  One table of inputs with ONE fault each (so the order
of the checks inside the shared helpers is free); every expected message is the whole sentence, recorded from the ops as they were
when each carried its own copy of the checks.  The CPU rows are the faults an op reports before it asks for a GPU; the ``gpu`` twin
runs every row on the device."""
from types import SimpleNamespace

import pytest
import torch

from moss_amd import bounds as mb
from moss_amd import lbs as mlbs
from moss_amd import posefit


def case(dev, J=24, V=40, P=5):
    """Valid inputs of the five ops on ``dev``."""
    dev = torch.device(dev)
    body = {k: v.to(dev) for k, v in mlbs.synthetic_body_model(V, J, seed=1).items()}
    body["kintree_table"] = body["kintree_table"].cpu().clone()
    params = {k: v.to(dev) for k, v in mlbs.synthetic_frame(3, J).items()}
    t_params = {k: v.to(dev) for k, v in mlbs.synthetic_frame(0, J, big_pose=True).items()}
    g = torch.Generator().manual_seed(7)
    f = lambda *s: torch.randn(*s, generator=g).to(dev)                                  # noqa: E731
    eye4 = torch.eye(4).repeat(J, 1, 1).to(dev)
    return SimpleNamespace(
        body=body, W=body["weights"], params=params, t_params=t_params, ids=torch.randint(0, V, (P,), generator=g).to(dev),
        x=f(P, 3), L=f(P, J), cR=torch.eye(3).repeat(J - 1, 1, 1).to(dev), A_big=eye4, A_obs=eye4.clone(), d=f(P, 3),
        R=torch.eye(3).to(dev), Th=f(3), wb=torch.tensor([[-1.0, -1.0, 2.0], [1.0, 1.0, 4.0]]).to(dev),
        K=torch.tensor([[[8.0, 0.0, 4.0], [0.0, 8.0, 4.0], [0.0, 0.0, 1.0]]]).to(dev),
        RT=torch.eye(4)[None, :3].contiguous().to(dev))


CALLS = {
    "lbs_deform": lambda c: mlbs.lbs_deform(c.ids, c.W, c.L, c.A_big, c.A_obs, c.d, c.R, c.Th, x=c.x),
    "smpl_frame_fused": lambda c: mlbs.smpl_frame_fused(c.body, c.params, c.t_params, c.ids, correct_Rs=c.cR),
    "posed_frame": lambda c: posefit.posed_frame(c.body, c.W, c.params, c.t_params, c.ids, c.x, lbs_offsets=c.L, correct_Rs=c.cR),
    "posed_vertices": lambda c: mb.posed_vertices(c.body, c.params),
    "bound_masks": lambda c: mb.bound_masks(c.wb, c.K, c.RT, 8, 8),
}
BODY_OPS = ("smpl_frame_fused", "posed_frame", "posed_vertices")


def _body(c, key, value):
    c.body = {**c.body, key: value}
    if key == "weights":
        c.W = value


def _drop(c, key):
    c.body = {k: v for k, v in c.body.items() if k != key}


def _param(c, key, value, which="params"):
    setattr(c, which, {**getattr(c, which), key: value})


def _kintree(c):
    kt = c.body["kintree_table"].clone()
    kt[0, 5] = 7
    _body(c, "kintree_table", kt)


def _grad(t):
    return t.clone().requires_grad_(True)


# (fault, the ops it is put to, what it does to a valid case)
FAULTS = [
    ("cpu tensors", tuple(CALLS), lambda c: vars(c).update(vars(case("cpu")))),
    ("missing body key", BODY_OPS, lambda c: _drop(c, "posedirs")),
    ("65 joints", ("lbs_deform",) + BODY_OPS, None),                                      # (a whole case of J = 65: see run())
    ("dtype posedirs", BODY_OPS, lambda c: _body(c, "posedirs", c.body["posedirs"].double())),
    ("dtype d", ("lbs_deform",), lambda c: setattr(c, "d", c.d.double())),
    ("dtype vert_ids", ("lbs_deform", "smpl_frame_fused", "posed_frame"), lambda c: setattr(c, "ids", c.ids.int())),
    ("dtype K", ("bound_masks",), lambda c: setattr(c, "K", c.K.double())),
    ("shape posedirs", BODY_OPS, lambda c: _body(c, "posedirs", c.body["posedirs"][..., :-1].contiguous())),
    ("shape d", ("lbs_deform",), lambda c: setattr(c, "d", torch.cat([c.d, c.d[:, :1]], 1).contiguous())),
    ("shape correct_Rs", ("smpl_frame_fused", "posed_frame"), lambda c: setattr(c, "cR", torch.cat([c.cR, c.cR[:1]], 0).contiguous())),
    ("shape RT", ("bound_masks",), lambda c: setattr(c, "RT", c.RT[:, :, :3].contiguous())),
    ("strides J_regressor", BODY_OPS, lambda c: _body(c, "J_regressor", c.body["J_regressor"].t().contiguous().t())),
    ("strides d", ("lbs_deform",), lambda c: setattr(c, "d", c.d.t().contiguous().t())),
    ("strides world_bound", ("bound_masks",), lambda c: setattr(c, "wb", c.wb.t().contiguous().t())),
    ("69 pose elements", BODY_OPS, lambda c: _param(c, "poses", c.params["poses"][:, :69].contiguous())),
    ("11 shape coefficients", BODY_OPS, lambda c: _param(c, "shapes", torch.zeros(1, 11, device=c.W.device))),
    ("kintree_table", BODY_OPS, _kintree),
    ("device d", ("lbs_deform",), lambda c: setattr(c, "d", c.d.cpu())),
    ("device vert_ids", ("smpl_frame_fused", "posed_frame"), lambda c: setattr(c, "ids", c.ids.cpu())),
    ("device params poses", BODY_OPS, lambda c: _param(c, "poses", c.params["poses"].cpu())),
    ("device J_regressor", BODY_OPS, lambda c: _body(c, "J_regressor", c.body["J_regressor"].cpu())),
    ("device RT", ("bound_masks",), lambda c: setattr(c, "RT", c.RT.cpu())),
    ("grad W", ("lbs_deform", "posed_frame"), lambda c: setattr(c, "W", _grad(c.W))),
    ("grad A_big", ("lbs_deform",), lambda c: setattr(c, "A_big", _grad(c.A_big))),
    ("grad R", ("lbs_deform",), lambda c: setattr(c, "R", _grad(c.R))),
    ("grad Th", ("lbs_deform",), lambda c: setattr(c, "Th", _grad(c.Th))),
    ("grad posedirs", BODY_OPS, lambda c: _body(c, "posedirs", _grad(c.body["posedirs"]))),
    ("grad weights", ("posed_vertices",), lambda c: _body(c, "weights", _grad(c.body["weights"]))),
    ("grad params poses", ("smpl_frame_fused", "posed_vertices"), lambda c: _param(c, "poses", _grad(c.params["poses"]))),
    ("grad params shapes", BODY_OPS, lambda c: _param(c, "shapes", _grad(c.params["shapes"]))),
    ("grad t_params poses", ("smpl_frame_fused", "posed_frame"), lambda c: _param(c, "poses", _grad(c.t_params["poses"]), "t_params")),
    ("grad x", ("posed_frame",), lambda c: setattr(c, "x", _grad(c.x))),
    ("grad lbs_offsets", ("posed_frame",), lambda c: setattr(c, "L", _grad(c.L))),
    ("grad correct_Rs", ("posed_frame",), lambda c: setattr(c, "cR", _grad(c.cR))),
    ("grad K", ("bound_masks",), lambda c: setattr(c, "K", _grad(c.K))),
]
ROWS = [(op, fault, mutate) for fault, ops, mutate in FAULTS for op in ops]


def run(op, fault, mutate, dev):
    """The message ``op`` refuses the faulty case with."""
    if mutate is None:
        c = case(dev, J=65, V=70)
    else:
        c = case(dev)
        mutate(c)
    with pytest.raises(ValueError) as e:
        CALLS[op](c)
    return str(e.value)


EXPECTED = {
    ('lbs_deform', 'cpu tensors'):
        'lbs_deform runs the HIP LBS kernels: its tensors must be on a GPU (deform_torch is the torch form)',
    ('smpl_frame_fused', 'cpu tensors'):
        'smpl_frame_fused runs the HIP per-frame kernels: its tensors must be on a GPU (smpl_joint_transforms and vertex_offsets are the torch form)',
    ('posed_frame', 'cpu tensors'):
        'posed_frame runs the HIP deformation kernels: its tensors must be on a GPU (posed_frame_torch is the torch form)',
    ('posed_vertices', 'cpu tensors'):
        'posed_vertices runs the HIP kernels of csrc/frame_bounds.hip: its tensors must be on a GPU (posed_vertices_torch is the torch form)',
    ('bound_masks', 'cpu tensors'):
        'bound_masks runs the HIP kernels of csrc/frame_bounds.hip: its tensors must be on a GPU (project_corners_numpy and bound_mask_numpy are the CPU form)',
    ('smpl_frame_fused', 'missing body key'):
        "smpl_frame_fused: body['posedirs'] must be a tensor",
    ('posed_frame', 'missing body key'):
        "posed_frame: body['posedirs'] must be a tensor",
    ('posed_vertices', 'missing body key'):
        "posed_vertices: body['posedirs'] must be a tensor",
    ('lbs_deform', '65 joints'):
        'lbs_deform: J = 65 joints; the kernels take 1..64',
    ('smpl_frame_fused', '65 joints'):
        'smpl_frame_fused: J = 65 joints; the kernels take 1..64',
    ('posed_frame', '65 joints'):
        'posed_frame: J = 65 joints; the kernels take 1..64',
    ('posed_vertices', '65 joints'):
        'posed_vertices: J = 65 joints; the kernels take 1..64',
    ('smpl_frame_fused', 'dtype posedirs'):
        'smpl_frame_fused: posedirs must be torch.float32, got torch.float64',
    ('posed_frame', 'dtype posedirs'):
        'posed_frame: posedirs must be torch.float32, got torch.float64',
    ('posed_vertices', 'dtype posedirs'):
        'posed_vertices: posedirs must be torch.float32, got torch.float64',
    ('lbs_deform', 'dtype d'):
        'lbs_deform: d must be torch.float32, got torch.float64',
    ('lbs_deform', 'dtype vert_ids'):
        'lbs_deform: vert_ids must be torch.int64, got torch.int32',
    ('smpl_frame_fused', 'dtype vert_ids'):
        'smpl_frame_fused: vert_ids must be torch.int64, got torch.int32',
    ('posed_frame', 'dtype vert_ids'):
        'posed_frame: vert_ids must be torch.int64, got torch.int32',
    ('bound_masks', 'dtype K'):
        'bound_masks: K must be torch.float32, got torch.float64',
    ('smpl_frame_fused', 'shape posedirs'):
        'smpl_frame_fused: posedirs must have shape (40, 3, 207), got (40, 3, 206)',
    ('posed_frame', 'shape posedirs'):
        'posed_frame: posedirs must have shape (40, 3, 207), got (40, 3, 206)',
    ('posed_vertices', 'shape posedirs'):
        'posed_vertices: posedirs must have shape (40, 3, 207), got (40, 3, 206)',
    ('lbs_deform', 'shape d'):
        'lbs_deform: d must have shape (5, 3), got (5, 4)',
    ('smpl_frame_fused', 'shape correct_Rs'):
        'smpl_frame_fused: correct_Rs must have shape (23, 3, 3), got (24, 3, 3)',
    ('posed_frame', 'shape correct_Rs'):
        'posed_frame: correct_Rs must have shape (23, 3, 3), got (24, 3, 3)',
    ('bound_masks', 'shape RT'):
        'bound_masks: RT must have shape (1, 3, 4), got (1, 3, 3)',
    ('smpl_frame_fused', 'strides J_regressor'):
        'smpl_frame_fused: J_regressor must be contiguous',
    ('posed_frame', 'strides J_regressor'):
        'posed_frame: J_regressor must be contiguous',
    ('posed_vertices', 'strides J_regressor'):
        'posed_vertices: J_regressor must be contiguous',
    ('lbs_deform', 'strides d'):
        'lbs_deform: d must be contiguous',
    ('bound_masks', 'strides world_bound'):
        'bound_masks: world_bound must be contiguous',
    ('smpl_frame_fused', '69 pose elements'):
        "smpl_frame_fused: params['poses'] must have 72 elements, got 69",
    ('posed_frame', '69 pose elements'):
        "posed_frame: params['poses'] must have 72 elements, got 69",
    ('posed_vertices', '69 pose elements'):
        "posed_vertices: params['poses'] must have 72 elements, got 69",
    ('smpl_frame_fused', '11 shape coefficients'):
        'smpl_frame_fused: 11 shape coefficients, but shapedirs stores 10',
    ('posed_frame', '11 shape coefficients'):
        'posed_frame: 11 shape coefficients, but shapedirs stores 10',
    ('posed_vertices', '11 shape coefficients'):
        'posed_vertices: 11 shape coefficients, but shapedirs stores 10',
    ('smpl_frame_fused', 'kintree_table'):
        'smpl_frame_fused: kintree_table[0] must list J parents with 0 <= parent[j] < j for j >= 1',
    ('posed_frame', 'kintree_table'):
        'posed_frame: kintree_table[0] must list J parents with 0 <= parent[j] < j for j >= 1',
    ('posed_vertices', 'kintree_table'):
        'posed_vertices: kintree_table[0] must list J parents with 0 <= parent[j] < j for j >= 1',
    ('lbs_deform', 'device d'):
        'lbs_deform: d must be on cuda:0, got cpu',
    ('smpl_frame_fused', 'device vert_ids'):
        'smpl_frame_fused: vert_ids must be on cuda:0, got cpu',
    ('posed_frame', 'device vert_ids'):
        'posed_frame: vert_ids must be on cuda:0, got cpu',
    ('smpl_frame_fused', 'device params poses'):
        "smpl_frame_fused: params['poses'] must be on cuda:0, got cpu",
    ('posed_frame', 'device params poses'):
        "posed_frame: params['poses'] must be on cuda:0, got cpu",
    ('posed_vertices', 'device params poses'):
        "posed_vertices: params['poses'] must be on cuda:0, got cpu",
    ('smpl_frame_fused', 'device J_regressor'):
        'smpl_frame_fused: J_regressor must be on cuda:0, got cpu',
    ('posed_frame', 'device J_regressor'):
        'posed_frame: J_regressor must be on cuda:0, got cpu',
    ('posed_vertices', 'device J_regressor'):
        'posed_vertices: J_regressor must be on cuda:0, got cpu',
    ('bound_masks', 'device RT'):
        'bound_masks: RT must be on cuda:0, got cpu',
    ('lbs_deform', 'grad W'):
        'lbs_deform: W requires grad, but it is a constant of the deformation (no gradient is formed for it); detach it',
    ('posed_frame', 'grad W'):
        "posed_frame: W requires grad, but it is data of the fit (the avatar is frozen: gradients go to params['poses'], params['R'] and params['Th'] only); detach it",
    ('lbs_deform', 'grad A_big'):
        'lbs_deform: A_big requires grad, but it is a constant of the deformation (no gradient is formed for it); detach it',
    ('lbs_deform', 'grad R'):
        'lbs_deform: R requires grad, but it is a constant of the deformation (no gradient is formed for it); detach it',
    ('lbs_deform', 'grad Th'):
        'lbs_deform: Th requires grad, but it is a constant of the deformation (no gradient is formed for it); detach it',
    ('smpl_frame_fused', 'grad posedirs'):
        'smpl_frame_fused: posedirs requires grad, but it is data of the deformation (no gradient is formed for it); detach it',
    ('posed_frame', 'grad posedirs'):
        "posed_frame: posedirs requires grad, but it is data of the fit (the avatar is frozen: gradients go to params['poses'], params['R'] and params['Th'] only); detach it",
    ('posed_vertices', 'grad posedirs'):
        'posed_vertices: posedirs requires grad, but no gradient is formed for it; detach it',
    ('posed_vertices', 'grad weights'):
        'posed_vertices: weights requires grad, but no gradient is formed for it; detach it',
    ('smpl_frame_fused', 'grad params poses'):
        "smpl_frame_fused: params['poses'] requires grad, but it is data of the deformation (no gradient is formed for it); detach it",
    ('posed_vertices', 'grad params poses'):
        "posed_vertices: params['poses'] requires grad, but no gradient is formed for it; detach it",
    ('smpl_frame_fused', 'grad params shapes'):
        "smpl_frame_fused: params['shapes'] requires grad, but it is data of the deformation (no gradient is formed for it); detach it",
    ('posed_frame', 'grad params shapes'):
        "posed_frame: params['shapes'] requires grad, but it is data of the fit (the avatar is frozen: gradients go to params['poses'], params['R'] and params['Th'] only); detach it",
    ('posed_vertices', 'grad params shapes'):
        "posed_vertices: params['shapes'] requires grad, but no gradient is formed for it; detach it",
    ('smpl_frame_fused', 'grad t_params poses'):
        "smpl_frame_fused: t_params['poses'] requires grad, but it is data of the deformation (no gradient is formed for it); detach it",
    ('posed_frame', 'grad t_params poses'):
        "posed_frame: t_params['poses'] requires grad, but it is data of the fit (the avatar is frozen: gradients go to params['poses'], params['R'] and params['Th'] only); detach it",
    ('posed_frame', 'grad x'):
        "posed_frame: x requires grad, but it is data of the fit (the avatar is frozen: gradients go to params['poses'], params['R'] and params['Th'] only); detach it",
    ('posed_frame', 'grad lbs_offsets'):
        "posed_frame: lbs_offsets requires grad, but it is data of the fit (the avatar is frozen: gradients go to params['poses'], params['R'] and params['Th'] only); detach it",
    ('posed_frame', 'grad correct_Rs'):
        "posed_frame: correct_Rs requires grad, but it is data of the fit (the avatar is frozen: gradients go to params['poses'], params['R'] and params['Th'] only); detach it",
    ('bound_masks', 'grad K'):
        'bound_masks: K requires grad, but no gradient is formed for it; detach it',
}

# the rows an op refuses before it asks for a GPU: the CPU test runs these, with the same words
ON_CPU = [
    ('lbs_deform', 'cpu tensors'), ('smpl_frame_fused', 'cpu tensors'), ('posed_frame', 'cpu tensors'),
    ('posed_vertices', 'cpu tensors'), ('bound_masks', 'cpu tensors'), ('smpl_frame_fused', 'missing body key'),
    ('posed_frame', 'missing body key'), ('posed_vertices', 'missing body key'), ('smpl_frame_fused', '65 joints'),
    ('posed_frame', '65 joints'), ('posed_vertices', '65 joints'), ('smpl_frame_fused', 'dtype posedirs'),
    ('posed_vertices', 'dtype posedirs'), ('smpl_frame_fused', 'dtype vert_ids'), ('smpl_frame_fused', 'shape posedirs'),
    ('posed_vertices', 'shape posedirs'), ('smpl_frame_fused', 'shape correct_Rs'), ('smpl_frame_fused', 'strides J_regressor'),
    ('posed_vertices', 'strides J_regressor'), ('smpl_frame_fused', '69 pose elements'),
    ('smpl_frame_fused', '11 shape coefficients'), ('posed_frame', 'grad W'), ('smpl_frame_fused', 'grad posedirs'),
    ('posed_frame', 'grad posedirs'), ('posed_vertices', 'grad posedirs'), ('posed_vertices', 'grad weights'),
    ('smpl_frame_fused', 'grad params poses'), ('smpl_frame_fused', 'grad params shapes'), ('posed_frame', 'grad params shapes'),
    ('smpl_frame_fused', 'grad t_params poses'), ('posed_frame', 'grad t_params poses'), ('posed_frame', 'grad x'),
    ('posed_frame', 'grad lbs_offsets'), ('posed_frame', 'grad correct_Rs'),
]


MUTATE = {(op, fault): mutate for op, fault, mutate in ROWS}


@pytest.mark.parametrize("op,fault", ON_CPU)
def test_refusal_before_the_gpu_check_is_worded_as_before(op, fault):
    assert run(op, fault, MUTATE[op, fault], "cpu") == EXPECTED[op, fault]


@pytest.mark.gpu
@pytest.mark.parametrize("op,fault", list(EXPECTED))
def test_refusal_on_the_gpu_is_worded_as_before(gpu, op, fault):
    assert run(op, fault, MUTATE[op, fault], gpu) == EXPECTED[op, fault]


def test_every_row_is_pinned():
    assert set(EXPECTED) == set(MUTATE) and set(ON_CPU) <= set(EXPECTED)
