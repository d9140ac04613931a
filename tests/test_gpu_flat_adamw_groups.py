"""FlatAdamW with one learning-rate segment per parameter GROUP, on the tensors of MOSS's two networks: the 52 of the pose head
(``pose._param_shapes``) and the 16 of the LBS-weight network (``lbs_weights.PARAM_SHAPES``; numel 3, 9, 69 and 24 among them, so most
tensors are followed by padding).  One optimizer over both groups -- two segments, one launch per step -- against the same tensors
split over several optimizers of at most eight tensors, a segment each (the only form that existed before): bit-identical parameters
and moments after every step, exact zeros in the padding, and one step against float64 under the bars of tests/test_gpu_adamw.py."""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests.test_gpu_adamw import _bars, _check

pytestmark = pytest.mark.gpu

LR_HEAD, LR_NET = 2.5e-4, 1e-4
KW = dict(betas=(0.9, 0.999), eps=1e-15, weight_decay=0.01, capturable=True)
STEPS = 5


def _shapes():
    from moss_amd import lbs_weights, pose
    head = [tuple(s) for s in pose._param_shapes(pose.ancestor_lists())]
    net = [tuple(s) for s in lbs_weights.PARAM_SHAPES]
    assert len(head) == 52 and len(net) == 16
    return head, net


def _tensors(shapes, seed, gpu):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((0.2 * torch.randn(*s, generator=g)).to(gpu)) for s in shapes]


def _gradients(shapes, step, gpu):
    """Gradients of mixed magnitude, one tensor per parameter (a few exact zeros: what a ReLU leaves)."""
    g = torch.Generator().manual_seed(9000 + step)
    out = []
    for i, s in enumerate(shapes):
        t = torch.randn(*s, generator=g) * float(10.0 ** ((i % 7) - 4))
        t[torch.rand(*s, generator=g) < 0.05] = 0.0
        out.append(t.to(gpu))
    return out


def _moments(opt, i):
    off, n = opt.bucket.offsets[i], opt.bucket.sizes[i]
    return opt.exp_avg[off:off + n], opt.exp_avg_sq[off:off + n]


def _gaps(bucket):
    return [(off + n, nxt) for n, off, nxt in zip(bucket.sizes, bucket.offsets, list(bucket.offsets[1:]) + [bucket.n_params]) if nxt > off + n]


def test_two_network_groups_in_one_launch_equal_a_segment_per_tensor(gpu, hip_lib):
    from moss_amd.dist import GradBucket
    from moss_amd.optim import FlatAdamW
    head, net = _shapes()
    shapes = head + net
    rates = [LR_HEAD] * len(head) + [LR_NET] * len(net)
    # the grouped optimizer: 68 tensors, two groups, two segments
    pa = _tensors(shapes, 1, gpu)
    ba = GradBucket(pa)
    oa = FlatAdamW([{"params": pa[:52], "lr": LR_HEAD}, {"params": pa[52:], "lr": LR_NET}], ba, **KW)
    assert oa.nseg == 2 and [int(e) for e in oa.seg_end] == [ba.offsets[52], ba.n_params] and oa.seg_of == [0] * 52 + [1] * 16
    gaps = _gaps(ba)
    assert len(gaps) > 40 and any(b - a == 3 for a, b in gaps) and any(b - a == 1 for a, b in gaps)
    # the same tensors over optimizers of <= 8 tensors each, one group (= one segment) per tensor
    pb = _tensors(shapes, 1, gpu)
    parts = []
    for i0 in range(0, len(pb), 8):
        ps = pb[i0:i0 + 8]
        b = GradBucket(ps)
        parts.append((i0, b, FlatAdamW([{"params": [p], "lr": lr} for p, lr in zip(ps, rates[i0:i0 + 8])], b, **KW)))
        assert parts[-1][2].nseg == len(ps)
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
    checked64 = False
    for step in range(1, STEPS + 1):
        grads = _gradients(shapes, step, gpu)
        for v, g in zip(ba.views, grads):
            v.copy_(g)
        for i0, b, _ in parts:
            for v, g in zip(b.views, grads[i0:i0 + 8]):
                v.copy_(g)
        before = [t.cpu().numpy().copy() for t in (oa.flat_params, ba.flat[:ba.n_params], oa.exp_avg, oa.exp_avg_sq)]
        oa.step()
        for _, _, o in parts:
            o.step()
        torch.cuda.synchronize(gpu)
        for i0, b, o in parts:
            for k, p_ref in enumerate(b.params):
                i = i0 + k
                m, v = _moments(oa, i)
                m_ref, v_ref = _moments(o, k)
                assert torch.equal(pa[i], p_ref), (step, i, "parameter")
                assert torch.equal(m, m_ref) and torch.equal(v, v_ref), (step, i, "moments")
        for flat in (oa.flat_params, oa.exp_avg, oa.exp_avg_sq):
            for a, b in gaps:
                assert not bool(flat[a:b].any()), (step, a)            # exactly 0.0 (a -0.0 would compare equal: look at the bits too)
                assert not bool(flat[a:b].view(torch.int32).any()), (step, a)
        if step == 3:
            # this step against float64, from the kernel's own float32 state before it
            n = oa.n
            lr = oracle.adamw_lr_per_element(0, n, [int(e) for e in oa.seg_end], [oa.seg_lr[i] for i in range(oa.nseg)])
            p0, g0, m0, v0 = (a[:n] for a in before)
            ref = oracle.adamw_step_f64(p0, g0, m0, v0, lr, 0.9, 0.999, 1e-15, 0.01, step)
            bars = _bars(p0, g0, m0, v0, lr, 0.9, 0.999, 1e-15, 0.01, step, ref)
            got = tuple(t[:n].cpu().numpy() for t in (oa.flat_params, oa.exp_avg, oa.exp_avg_sq))
            _check(got, ref, bars, f"grouped step {step}")
            assert float(np.abs(got[0] - p0).max()) > 0
            checked64 = True
    assert checked64 and oa.step_count() == STEPS and all(o.step_count() == STEPS for _, _, o in parts)


def test_a_rate_set_on_one_network_tensor_reaches_the_whole_group_on_the_device(gpu, hip_lib):
    """set_learning_rates on ONE member of a run: the device-side rate table (what a captured step reads) carries the new rate for the
    whole segment -- the step equals, bit for bit, that of an optimizer built with that rate."""
    from moss_amd.dist import GradBucket
    from moss_amd.optim import FlatAdamW
    head, net = _shapes()
    shapes = head + net
    res = []
    for scheduled in (True, False):
        ps = _tensors(shapes, 2, gpu)
        b = GradBucket(ps)
        o = FlatAdamW([{"params": ps[:52], "lr": LR_HEAD if scheduled else 7e-4}, {"params": ps[52:], "lr": LR_NET}], b, **KW)
        if scheduled:
            o.set_learning_rates({ps[17]: 7e-4})
        for v, g in zip(b.views, _gradients(shapes, 1, gpu)):
            v.copy_(g)
        o.step()
        torch.cuda.synchronize(gpu)
        res.append((o.flat_params.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
