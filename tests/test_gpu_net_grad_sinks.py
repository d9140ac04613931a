"""``grad_sink`` of the two network ops (``pose_head_fused``, ``cross_attention_lbs_fused``): a parameter whose sink returns a tensor
gets its gradient written THERE (overwritten, not accumulated) and autograd receives that tensor; one whose sink returns None keeps its
slice of the op's scratch tensor; without the argument nothing changes.  Gradients are compared bit for bit with the sink-less call."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _nets(gpu):
    from moss_amd import lbs_weights as mlw
    from moss_amd import pose as mpose
    torch.manual_seed(11)
    head = mpose.head_module(init_val=0.05).to(gpu)
    net = mlw.lbs_weight_module().to(gpu)
    return head, net


def _run(gpu, head, net, P, sink):
    """One forward + backward of both ops chained as render() chains them; returns the gradients of x and of the 52 + 16 tensors."""
    from moss_amd import lbs as mlbs
    from moss_amd import lbs_weights as mlw
    from moss_amd import pose as mpose
    g = torch.Generator().manual_seed(5)
    poses = (0.2 * torch.randn(72, generator=g)).to(gpu)
    target = mlbs.batch_rodrigues(0.2 * torch.randn(23, 3, generator=g)).to(gpu)
    x = (0.5 * torch.randn(P, 3, generator=g)).to(gpu).requires_grad_(True)
    w = torch.randn(1, P, 24, generator=g).to(gpu)
    params = mpose.head_parameters(head) + mlw.net_parameters(net)
    for p in net.parameters():
        p.grad = None
    for p in head.parameters():
        p.grad = None
    kw = {} if sink is None else {"grad_sink": sink}
    out = mpose.pose_head_fused(head, poses, target, **kw)
    lw = mlw.cross_attention_lbs_fused(net, x, out["Rs"], **kw)
    ((lw * w).sum() + 0.06 * out["nll"].mean()).backward()
    torch.cuda.synchronize(gpu)
    return x.grad, params


@pytest.mark.parametrize("P", [1, 777])
def test_sinks_receive_the_same_bits_and_are_overwritten(gpu, hip_lib, P):
    from moss_amd.dist import GradBucket
    head, net = _nets(gpu)
    gx0, params = _run(gpu, head, net, P, None)
    ref = [p.grad.clone() for p in params]
    assert all(bool(torch.isfinite(r).all()) for r in ref) and sum(float(r.abs().sum()) for r in ref[:52]) > 0
    if P > 1:
        assert sum(float(r.abs().sum()) for r in ref[52:]) > 0
    # every second tensor through a bucket's sink (unaligned sizes among them: 3, 9, 69), the others stay scratch slices
    chosen = params[::2]
    bucket = GradBucket(chosen)
    bucket.detach_grads()
    bucket.flat.fill_(float("nan"))                                      # overwritten, not accumulated: NaN would survive an add
    asked = []

    def sink(p):
        asked.append(id(p))
        return bucket.sink_for(p)

    gx1, _ = _run(gpu, head, net, P, sink)
    assert sorted(asked) == sorted(id(p) for p in params)                # asked once per parameter
    assert torch.equal(gx1, gx0)
    for i, (p, r) in enumerate(zip(params, ref)):
        assert torch.equal(p.grad, r), i
        in_bucket = id(p) in bucket._offset
        assert in_bucket == (i % 2 == 0)
        if in_bucket:
            off = bucket._offset[id(p)]
            assert p.grad.data_ptr() == bucket.flat[off:off + 1].data_ptr(), i          # autograd adopted the sink itself
    for n, off, nxt in zip(bucket.sizes, bucket.offsets, list(bucket.offsets[1:]) + [bucket.n_params]):
        assert bool(torch.isnan(bucket.flat[off + n:nxt]).all())         # nothing was written outside a tensor's slice
    # the four tensors the forward never reads are never asked for and get no gradient
    assert all(p.grad is None for n_, p in net.named_parameters() if n_.startswith(("out_layer", "gate_proj")))
    # a sink of the wrong shape is refused
    with pytest.raises(ValueError):
        _run(gpu, head, net, P, lambda p: torch.zeros(p.numel() + 1, device=gpu))


def test_no_gaussian_at_all_zeroes_the_sinks(gpu, hip_lib):
    """P = 0: the LBS-weight network launches nothing backward, so it must zero its sinks itself."""
    from moss_amd import lbs_weights as mlw
    from moss_amd.dist import GradBucket
    head, net = _nets(gpu)
    params = mlw.net_parameters(net)
    bucket = GradBucket(params)
    bucket.detach_grads()
    bucket.flat.fill_(float("nan"))
    Rs = torch.eye(3, device=gpu).repeat(23, 1, 1).requires_grad_(True)
    x = torch.zeros(0, 3, device=gpu, requires_grad=True)
    out = mlw.cross_attention_lbs_fused(net, x, Rs, grad_sink=bucket.sink_for)
    assert tuple(out.shape) == (1, 0, 24)
    out.sum().backward()
    torch.cuda.synchronize(gpu)
    for p in params:
        off = bucket._offset[id(p)]
        assert p.grad.data_ptr() == bucket.flat[off:off + 1].data_ptr() and not bool(p.grad.any())
    assert not bool(Rs.grad.any()) and tuple(x.grad.shape) == (0, 3)
