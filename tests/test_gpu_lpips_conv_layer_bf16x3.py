"""The split-bf16 wide convolution kernel of the LPIPS term (moss_amd/csrc/lpips.hip: conv3x3_bf16x3_kernel), ONE LAYER PER CALL through
moss_lpips_vgg_conv3x3_bf16x3 with the kernel shape forced: every one of its 18 instantiations -- the 128-row shape with its 64-channel
slice and the 32-row shape with slices of 128 and of 64 channels, three modes, static and DYN -- at sizes of a few rows, per element
against float64.  The cases, the launch block, the guards and the structure checks are tests/test_gpu_lpips_conv_layer.py's.

Reference and bar: tests/test_lpips_bf16x3_cpu.py's ``split_layer_reference`` -- the split form as one float64 convolution over 3 Cin
channels (inputs [lo, hi, hi], weights [hi, lo, hi]), the error per element in units of that convolution's mass, within K = 8 times
E32, the float32 error of the same reference measured at test time (torch's float32 convolution of the concatenated operands,
contiguous and channels-last, and a sequential float32 sum in the kernel's k-interleaved order at 5 x 7).  No element excluded.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_gpu_lpips_conv_layer import (CAP, CASES, DYN_CASES, DYN_SIZE, LEVEL, MASK_SENTINEL, RECT, SHAPES, SPARE, _id, check, mask_words,
                                             rows_of)
from tests.test_lpips_bf16x3_cpu import split_layer_reference
from tests.test_lpips_conv_layer_cpu import MODES, forward_layer, layer_weights

pytestmark = pytest.mark.gpu


def instantiation(shape, cin, mode, dyn):
    """(shape, slice channels, mode, dyn): the instantiation launch_conv takes for a split call (the bf16 kernel's choice of slice)."""
    return (shape, 64 if shape == "rows128" or cin % 128 else 128, mode, dyn)


def test_every_instantiation_is_launched():
    """The parametrisations below cover all 18: conv3x3_bf16x3_kernel<WM,WK,KCB,MODE,DYN>, 3 shape and slice variants x 3 x 2."""
    want = {(s, k, m, d) for s, k in (("rows128", 64), ("rows32", 128), ("rows32", 64)) for m in MODES for d in (False, True)}
    assert len(want) == 18
    got = {instantiation(s, c[1], c[0], False) for c in CASES for s in SHAPES}
    got |= {instantiation(s, c[1], c[0], True) for c in DYN_CASES for s in SHAPES}
    assert got == want, sorted(map(str, want - got))


_packed = {}
_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report(gpu, hip_lib):
    yield
    _packed.clear()
    for key in sorted(_worst):
        print(f"lpips conv layer bf16x3, worst error / E32: {' '.join(key)}: {_worst[key]:.3f}")


def _note(shape, mode, ratio):
    _worst[(shape, mode)] = max(_worst.get((shape, mode), 0.0), ratio)


def packed(gpu, cin_f, cout_f):
    """(fwd, bwd, bias) of the forward layer cin_f -> cout_f on the device in the split packing, packed by the library, once."""
    from moss_amd._lib import call
    key = (cin_f, cout_f)
    if key not in _packed:
        w, bias = layer_weights(cin_f, cout_f)
        wd = w.to(gpu).contiguous()
        fwd = torch.empty(2 * w.numel(), dtype=torch.bfloat16, device=gpu)
        bwd = torch.empty_like(fwd)
        call("moss_lpips_vgg_pack_weights_bf16x3", gpu, cin_f, cout_f, wd.data_ptr(), fwd.data_ptr(), bwd.data_ptr())
        _packed[key] = (fwd, bwd, bias.to(gpu))
    return _packed[key]


class Launch:
    """tests/test_gpu_lpips_conv_layer.py's Launch for the split entry point: `out` NaN-filled and `mask_out` sentinel-filled, SPARE
    rows behind the grid's."""

    def __init__(self, gpu, mode, cin, cout, nimg, H, W, shape, x_rows, words=None, cap=None, rect=None, level=0):
        from moss_amd._lib import LpipsConv3x3Args
        self.gpu = gpu
        fwd, bwd, bias = packed(gpu, *forward_layer(mode, cin, cout))
        grid_rows = nimg * (cap[0] >> level) * (cap[1] >> level) if cap else nimg * H * W
        self.x = x_rows.to(gpu).contiguous()
        self.out = torch.empty(grid_rows + SPARE, cout, device=gpu)
        self.mask = torch.empty(grid_rows + SPARE, cout // 32, dtype=torch.int32, device=gpu) if mode == "fwd" else None
        self.words = torch.from_numpy(words.view(np.int32)).to(gpu) if mode == "bwd_mask" else None
        self.keep = (fwd, bwd, bias)
        a = LpipsConv3x3Args()
        a.in_, a.weights, a.out = self.x.data_ptr(), (fwd if mode == "fwd" else bwd).data_ptr(), self.out.data_ptr()
        if mode == "fwd":
            a.bias, a.mask_out = bias.data_ptr(), self.mask.data_ptr()
        if mode == "bwd_mask":
            a.mask_in = self.words.data_ptr()
        a.nimg, a.H, a.W, a.cin, a.cout = nimg, H, W, cin, cout
        a.mode, a.shape, a.bf16 = MODES.index(mode), shape, 0
        if cap:
            a.rect, a.cap_H, a.cap_W, a.level = rect.data_ptr(), cap[0], cap[1], level
            a.H = a.W = 0                                                 # (ignored with a capacity)
        self.args = a

    def run(self):
        """(out, mask) of one launch on freshly pre-filled buffers, on the CPU (all rows, the spare ones too)."""
        from moss_amd._lib import call
        self.out.fill_(float("nan"))
        if self.mask is not None:
            self.mask.fill_(MASK_SENTINEL)
        call("moss_lpips_vgg_conv3x3_bf16x3", self.gpu, ctypes.byref(self.args))
        torch.cuda.synchronize(self.gpu)
        return self.out.cpu(), None if self.mask is None else self.mask.cpu().numpy().view(np.uint32)


def _launch_case(gpu, case, shape):
    mode, cin, cout, nimg, H, W = case
    ref = split_layer_reference(mode, cin, cout, nimg, H, W)
    words = mask_words(mode, cin, cout, nimg * H * W) if mode == "bwd_mask" else None
    return ref, words, Launch(gpu, mode, cin, cout, nimg, H, W, shape, rows_of(ref["x"]), words)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_layer_matches_the_split_form_in_float64(gpu, hip_lib, case, shape):
    """The output under the bar; the forward's sign words equal to `out > 0` exactly and to `z64 > 0` away from zero; the masked gradient
    exactly +0 where its bit is clear; every row < M written and every row >= M untouched (``check`` of the float32 file)."""
    mode, cin, cout, nimg, H, W = case
    ref, words, launch = _launch_case(gpu, case, SHAPES[shape])
    out, mask = launch.run()
    _note(shape, mode, check(ref, mode, nimg, H, W, out, mask, words, f"bf16x3 {shape} {_id(case)}"))


def test_the_launchers_own_choice(gpu, hip_lib):
    """shape = 0 is bit for bit the shape the unchanged rows128() rule resolves to, and not the other shape's bits."""
    case = ("fwd", 512, 512, 2, 9, 17)
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    resolved = "rows128" if (306 + 127) // 128 * (512 // 64) >= cus else "rows32"
    got = _launch_case(gpu, case, 0)[2].run()
    same = _launch_case(gpu, case, SHAPES[resolved])[2].run()
    assert torch.equal(got[0][:306], same[0][:306]) and (got[1] == same[1]).all()
    other = _launch_case(gpu, case, 3 - SHAPES[resolved])[2].run()
    assert not torch.equal(got[0][:306], other[0][:306])                  # (the two shapes sum K in different orders)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_two_launches_are_bit_identical(gpu, hip_lib, shape):
    launch = _launch_case(gpu, ("fwd", 512, 512, 2, 9, 17), SHAPES[shape])[2]
    a, b = launch.run(), launch.run()
    assert torch.equal(a[0][:306], b[0][:306]) and (a[1] == b[1]).all()
    launch = _launch_case(gpu, ("bwd_mask", 512, 512, 1, 9, 17), SHAPES[shape])[2]
    assert torch.equal(launch.run()[0][:153], launch.run()[0][:153])


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("dcase", DYN_CASES, ids=lambda c: f"{c[0]}-{c[1]}to{c[2]}")
def test_dynamic_equals_the_static_call(gpu, hip_lib, dcase, shape):
    """The size read from the device (9 x 13 in a grid made for 12 x 16, level 2 of a (48,64) capacity): bit-identical to the static
    call at 9 x 13 in the same shape, under the bar, and the guards hold at the ACTUAL M."""
    mode, cin, cout, nimg = dcase
    H, W = DYN_SIZE
    case = (mode, cin, cout, nimg, H, W)
    ref, words, static = _launch_case(gpu, case, SHAPES[shape])
    rect = torch.tensor(RECT, dtype=torch.int32, device=gpu)
    dyn = Launch(gpu, mode, cin, cout, nimg, 0, 0, SHAPES[shape], rows_of(ref["x"]), words, cap=CAP, rect=rect, level=LEVEL)
    (so, sm), (do, dm) = static.run(), dyn.run()
    M = nimg * H * W
    assert do.shape[0] == nimg * 12 * 16 + SPARE and torch.equal(do[:M], so[:M])
    _note(shape, mode, check(ref, mode, nimg, H, W, do, dm, words, f"bf16x3 {shape} dyn {_id(case)}"))
    if mode == "fwd":
        assert (dm[:H * W] == sm[:H * W]).all()


def test_rect_rewritten_between_launches(gpu, hip_lib):
    """One argument block, launched at rect 37 x 53 and, rewritten on the device, at 20 x 33 (level 2: 9 x 13, then 5 x 8): each launch
    equals its static twin bit for bit and writes no row beyond its own M."""
    mode, cin, cout, nimg = "fwd", 128, 256, 2
    x_rows = rows_of(split_layer_reference(mode, cin, cout, nimg, DYN_SIZE[0], DYN_SIZE[1])["x"])
    for shape in SHAPES.values():
        rect = torch.tensor(RECT, dtype=torch.int32, device=gpu)
        dyn = Launch(gpu, mode, cin, cout, nimg, 0, 0, shape, x_rows, cap=CAP, rect=rect, level=LEVEL)
        for (w, h), (H, W) in (((53, 37), (9, 13)), ((33, 20), (5, 8))):
            rect.copy_(torch.tensor((1, 2, w, h), dtype=torch.int32))
            M = nimg * H * W
            do, dm = dyn.run()
            so, sm = Launch(gpu, mode, cin, cout, nimg, H, W, shape, x_rows[:M]).run()
            assert torch.equal(do[:M], so[:M]) and not bool(torch.isnan(do[:M]).any()) and bool(torch.isnan(do[M:]).all())
            assert (dm[:H * W] == sm[:H * W]).all() and (dm[H * W:] == MASK_SENTINEL).all()
