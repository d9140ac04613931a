"""FlatAdamW's learning-rate segments follow PARAMETER GROUPS, not tensors (no GPU: the bookkeeping alone).

A segment is a run of consecutive bucket tensors of one entry of ``param_groups`` (a tensor with an ``lr_pattern`` is a segment of its
own).  MOSS's two network groups are 52 and 16 tensors: with a segment per tensor the constructor refused them (at most 8)."""
import pytest
import torch

from moss_amd.dist import GradBucket
from moss_amd.optim import FlatAdamW

SIZES_A, SIZES_B = [1, 3, 5, 69, 1023, 1025], [4, 7, 128]


def _two_groups(lr_a=2.5e-4, lr_b=1e-4):
    ga = [torch.nn.Parameter(torch.randn(n)) for n in SIZES_A]
    gb = [torch.nn.Parameter(torch.randn(n)) for n in SIZES_B]
    bucket = GradBucket(ga + gb)
    opt = FlatAdamW([{"params": ga, "lr": lr_a}, {"params": gb, "lr": lr_b}], bucket, capturable=False)
    return ga, gb, bucket, opt


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def test_two_groups_of_many_tensors_are_two_segments():
    torch.manual_seed(0)
    ga, gb, bucket, opt = _two_groups()
    # every tensor starts at a multiple of 4 floats: written out
    assert list(bucket.offsets) == [0, 4, 8, 16, 88, 1112, 2140, 2144, 2152] and bucket.n_params == 2280
    assert opt.nseg == 2 and len(opt.seg_end) == len(opt.seg_lr) == 2
    # a segment ends at the aligned start of the next group's first tensor; the last at n
    assert [int(e) for e in opt.seg_end] == [bucket.offsets[len(SIZES_A)], opt.n] == [2140, 2280]
    assert [opt.seg_lr[0], opt.seg_lr[1]] == [_f32(2.5e-4), _f32(1e-4)]
    assert [int(v) for v in opt.seg_period] == [0, 0] and [int(v) for v in opt.seg_split] == [0, 0]
    assert opt.seg_of == [0] * 6 + [1] * 3
    # the <= 3 floats between the tensors of a run are zeros (and have zero gradients and zero moments: they stay zero)
    for n, off, nxt in zip(bucket.sizes, bucket.offsets, list(bucket.offsets[1:]) + [bucket.n_params]):
        assert not bool(opt.flat_params[off + n:nxt].any()) and not bool(bucket.flat[off + n:nxt].any())
        assert not bool(opt.exp_avg[off + n:nxt].any()) and not bool(opt.exp_avg_sq[off + n:nxt].any())
    # the parameters were re-homed in the flat buffer, values kept
    for p, n, off in zip(bucket.params, bucket.sizes, bucket.offsets):
        assert p.data_ptr() == opt.flat_params[off:off + 1].data_ptr()


def test_a_rate_set_on_one_member_is_the_runs_rate():
    torch.manual_seed(1)
    ga, gb, bucket, opt = _two_groups()
    opt.set_learning_rates({ga[3]: 5e-4})                              # any member, by object ...
    assert opt.seg_lr[0] == _f32(5e-4) and opt.seg_lr[1] == _f32(1e-4)
    opt.set_learning_rates({7: 3e-5})                                  # ... or by its index in the bucket (gb[1])
    assert opt.seg_lr[0] == _f32(5e-4) and opt.seg_lr[1] == _f32(3e-5)
    opt.set_learning_rates({ga[0]: 1e-3, ga[5]: 1e-3, gb[2]: 2e-3})    # the same rate twice is no conflict
    assert opt.seg_lr[0] == _f32(1e-3) and opt.seg_lr[1] == _f32(2e-3)
    with pytest.raises(ValueError):
        opt.set_learning_rates({ga[0]: 1e-3, ga[1]: 2e-3})
    with pytest.raises(ValueError):
        opt.set_learning_rates({gb[0]: 7e-3, ga[2]: 1e-4, 8: 8e-3})    # (gb[0] and index 8 = gb[2])
    assert opt.seg_lr[0] == _f32(1e-3) and opt.seg_lr[1] == _f32(2e-3)  # a refused call changes nothing


def test_runs_are_cut_by_group_by_pattern_and_by_position():
    torch.manual_seed(2)
    a, b, c, d = (torch.nn.Parameter(torch.randn(n)) for n in (5, 96, 6, 7))
    # a | b (pattern) | c, d of the group of a: the run of that group is cut by the tensor between them -> three segments
    bucket = GradBucket([a, b, c, d])
    opt = FlatAdamW([{"params": [a, c, d], "lr": 1e-3}, {"params": [b], "lr": 2e-3, "lr_pattern": (48, 3, 1e-4)}], bucket)
    assert opt.nseg == 3 and opt.seg_of == [0, 1, 2, 2]
    assert [int(e) for e in opt.seg_end] == [8, 104, 119] and opt.n == 119
    assert [int(v) for v in opt.seg_period] == [0, 48, 0] and [int(v) for v in opt.seg_split] == [0, 3, 0]
    opt.set_learning_rates({d: 5e-3})
    assert [opt.seg_lr[i] for i in range(3)] == [_f32(1e-3), _f32(2e-3), _f32(5e-3)]      # (the run of c and d only)
    # two tensors with a pattern in ONE group stay two segments: the pattern's period counts from the segment's start
    e, f = (torch.nn.Parameter(torch.randn(n)) for n in (96, 48))
    o2 = FlatAdamW([{"params": [e, f], "lr": 2e-3, "lr_pattern": (48, 3, 1e-4)}], GradBucket([e, f]))
    assert o2.nseg == 2 and [int(v) for v in o2.seg_end] == [96, 144]
    # nine groups are nine segments: refused; nine TENSORS of two groups are not
    ps = [torch.nn.Parameter(torch.randn(3)) for _ in range(9)]
    with pytest.raises(ValueError, match="segments"):
        FlatAdamW([{"params": [p], "lr": 1e-3} for p in ps], GradBucket(ps))
    assert FlatAdamW([{"params": ps[:4], "lr": 1e-3}, {"params": ps[4:], "lr": 2e-3}], GradBucket(ps)).nseg == 2


def test_one_tensor_per_group_gives_the_segments_it_always_gave():
    """The five Gaussian tensors, a group each, SH with MOSS's (48, 3, lr / 20): the numbers are written out."""
    torch.manual_seed(3)
    P = 5
    shapes = {"xyz": (P, 3), "features": (P, 16, 3), "opacity": (P, 1), "scaling": (P, 3), "rotation": (P, 4)}
    rates = {"xyz": 0.00016, "features": 0.0025, "opacity": 0.05, "scaling": 0.005, "rotation": 0.001}
    ps = {k: torch.nn.Parameter(torch.randn(*s)) for k, s in shapes.items()}
    groups = [{"params": [ps[k]], "lr": rates[k], "name": k, **({"lr_pattern": (48, 3, 0.0025 / 20.0)} if k == "features" else {})}
              for k in shapes]
    bucket = GradBucket(list(ps.values()))
    opt = FlatAdamW(groups, bucket, capturable=False)
    assert list(bucket.offsets) == [0, 16, 256, 264, 280]
    assert opt.nseg == 5 and opt.n == 300 and opt.seg_of == [0, 1, 2, 3, 4] and opt.sh_index == 1
    assert [int(e) for e in opt.seg_end] == [16, 256, 264, 280, 300]
    assert [opt.seg_lr[i] for i in range(5)] == [_f32(0.00016), _f32(0.0025), _f32(0.05), _f32(0.005), _f32(0.001)]
    assert [int(v) for v in opt.seg_period] == [0, 48, 0, 0, 0] and [int(v) for v in opt.seg_split] == [0, 3, 0, 0, 0]
    assert [opt.seg_lr2[i] for i in range(5)] == [0.0, _f32(0.000125), 0.0, 0.0, 0.0]
    act = opt._seg_active()
    assert [int(v) for v in act] == [0] * 5
    opt.sh_active_degree = 1                                           # (the degree-aware update names the SH tensor's SEGMENT)
    assert [int(v) for v in opt._seg_active()] == [0, 12, 0, 0, 0]
    # a schedule on one tensor touches that tensor's segment alone, and survives a re-layout
    opt.set_learning_rates({ps["xyz"]: 3e-5, ps["features"]: (1e-3, 2e-4)})
    opt.sh_active_degree = 3
    opt.append_rows({ps[k]: torch.zeros((2,) + shapes[k][1:]) for k in shapes})
    assert [int(e) for e in opt.seg_end] == [24, 360, 368, 392, 420] and opt.seg_of == [0, 1, 2, 3, 4]
    assert [opt.seg_lr[i] for i in range(5)] == [_f32(3e-5), _f32(1e-3), _f32(0.05), _f32(0.005), _f32(0.001)]
    assert opt.seg_lr2[1] == _f32(2e-4)


def test_fused_step_names_the_segment_not_the_tensor(hip_lib):
    """fuse_into_backward's lr_segment is the SEGMENT of each named tensor: with opacity, scaling and rotation in one group that is
    one segment for the three (it was the tensor's index in the bucket)."""
    from moss_amd._lib import OPT_BITS
    from moss_amd.diff_gaussian_rasterization import RasterContext
    P = 4
    sh, opa, scl, rot = (torch.nn.Parameter(torch.zeros(*s)) for s in ((P, 16, 3), (P, 1), (P, 3), (P, 4)))
    bucket = GradBucket([sh, opa, scl, rot])
    opt = FlatAdamW([{"params": [sh], "lr": 2.5e-3, "lr_pattern": (48, 3, 1.25e-4)}, {"params": [opa, scl, rot], "lr": 1e-3}], bucket,
                    capturable=True)
    assert opt.nseg == 2 and opt.seg_of == [0, 1, 1, 1]
    cx = RasterContext()
    st = opt.fuse_into_backward(cx, sh=sh, opacity=opa, scales=scl, rotations=rot).struct
    slot = {n: OPT_BITS[n].bit_length() - 1 for n in ("means3D", "sh", "opacity", "scales", "rotations")}
    assert st.lr_segment[slot["means3D"]] == -1 and st.lr_segment[slot["sh"]] == 0
    assert [st.lr_segment[slot[n]] for n in ("opacity", "scales", "rotations")] == [1, 1, 1]
    assert st.lr[slot["scales"]] == _f32(1e-3) and st.lr_sh_rest == _f32(1.25e-4)
    for n, p in (("opacity", opa), ("scales", scl), ("rotations", rot)):       # the moments are still the tensor's own
        assert st.exp_avg[slot[n]] == opt.exp_avg.data_ptr() + 4 * bucket._offset[id(p)]
