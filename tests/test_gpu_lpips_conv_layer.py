"""The wide convolution kernels of the LPIPS term (moss_amd/csrc/lpips.hip: conv3x3_mfma_kernel, conv3x3_bf16_kernel), ONE LAYER PER CALL
through moss_lpips_vgg_conv3x3 with the kernel shape forced: every one of the 30 instantiations -- two row shapes, three bf16 slice
variants, three modes, static and DYN -- at sizes of a few rows, per element against float64.

The full calls pick the shape from the row count and the device's compute units, so at test sizes they never run the 128-row shape
with Cin = 256 or 512, in MODE_BWD_PLAIN, or (DYN) for anything but conv 1_2 -- which is what production sizes launch.

Reference, bar and inputs: tests/test_lpips_conv_layer_cpu.py (float64 conv2d / conv_transpose2d on the CPU, the error per element in
units of the element's mass, within K = 8 times the reference's own float32 error E32 measured at test time; no element excluded).
Each test prints the worst error / E32 it met; the module prints the worst per precision, shape and mode when it is done.

Per case: the output under the bar (the forward as relu(z64): ReLU is 1-Lipschitz); the forward's sign words equal to `out > 0`
exactly and to `z64 > 0` wherever |z64| > K E32 mass (what is left out of that is at most 0.1 % of the case); the masked gradient
exactly +0 where its bit is clear; every row < M written and every row >= M, 128 spare rows included, untouched.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_lpips_conv_layer_cpu import K, MODES, forward_layer, layer_weights, reference, worst_ratio

pytestmark = pytest.mark.gpu

SHAPES = {"rows128": 1, "rows32": 2}                      # moss_lpips_conv3x3_args.shape
SPARE = 128                                               # rows behind every output: a 128-row workgroup's whole overhang
MASK_SENTINEL = 0x5A5A5A5A
LEFT_OUT = 1e-3

# the network's own channel pairs, as the CALL sees them (a data gradient runs from a layer's outputs to its inputs)
FWD = [(64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512)]
BWD_MASK = [(64, 64), (128, 128), (256, 256), (512, 512)]
BWD_PLAIN = [(128, 64), (256, 128), (512, 256), (512, 512)]                 # a pool below
# NOT a layer of the network: every plain gradient of VGG16 has Cin >= 128, so the bf16 launcher's 64-channel-slice branch is never
# taken in MODE_BWD_PLAIN -- but it is instantiated, static and DYN, and this is the only way to launch it
EXTRA_PLAIN = [(64, 64)]


def _cases():
    """(mode, cin, cout, nimg, H, W): the full channel list at 5 x 7 (two images: M = 70, one ragged 128-row block, the image boundary
    at row 35 inside a 32-row block); subsets that keep 512 -> 512 at 9 x 17 (M = 306: three 128-row blocks, the boundary inside the
    second, a 50-row tail) and at the degenerate levels a 16-pixel crop reaches.  The data gradient runs on one image."""
    out = []
    for mode, pairs in (("fwd", FWD), ("bwd_mask", BWD_MASK), ("bwd_plain", BWD_PLAIN + EXTRA_PLAIN)):
        out += [(mode, ci, co, 2 if mode == "fwd" else 1, 5, 7) for ci, co in pairs]
    for mode, pairs in (("fwd", [(64, 64), (256, 512), (512, 512)]), ("bwd_mask", [(128, 128), (512, 512)]),
                        ("bwd_plain", [(256, 128), (512, 512)])):
        out += [(mode, ci, co, 2 if mode == "fwd" else 1, 9, 17) for ci, co in pairs]
    for H, W in ((1, 1), (1, 3), (3, 1)):
        out += [("fwd", 64, 64, 2, H, W), ("fwd", 512, 512, 2, H, W), ("bwd_mask", 512, 512, 1, H, W), ("bwd_plain", 512, 512, 1, H, W)]
    return out


CASES = _cases()
# the dynamic form: capacity (48, 64), rect {., ., w 53, h 37}, level 2 -> the size is 9 x 13 in a grid made for 12 x 16
CAP, RECT, LEVEL, DYN_SIZE = (48, 64), (3, 5, 53, 37), 2, (9, 13)
DYN_CASES = [("fwd", 64, 128, 2), ("fwd", 512, 512, 2), ("bwd_mask", 64, 64, 1), ("bwd_mask", 512, 512, 1),
             ("bwd_plain", 64, 64, 1), ("bwd_plain", 512, 256, 1)]


def _id(case):
    mode, ci, co, nimg, H, W = case
    return f"{mode}-{ci}to{co}-{nimg}x{H}x{W}"


def instantiation(bf16, shape, cin, mode, dyn):
    """(precision, shape, slice, mode, dyn): the kernel instantiation launch_conv takes for a call."""
    if not bf16:
        return ("f32", shape, None, mode, dyn)
    return ("bf16", shape, 64 if shape == "rows128" or cin % 128 else 128, mode, dyn)


def test_every_instantiation_is_launched():
    """The parametrisations below cover all 30: conv3x3_mfma_kernel<WM,WK,MODE,DYN> 2 x 3 x 2, conv3x3_bf16_kernel<WM,WK,KCB,MODE,DYN>
    3 x 3 x 2."""
    want = {("f32", s, None, m, d) for s in SHAPES for m in MODES for d in (False, True)}
    want |= {("bf16", s, k, m, d) for s, k in (("rows128", 64), ("rows32", 128), ("rows32", 64)) for m in MODES for d in (False, True)}
    assert len(want) == 30
    got = {instantiation(b, s, c[1], c[0], False) for c in CASES for s in SHAPES for b in (False, True)}
    got |= {instantiation(b, s, c[1], c[0], True) for c in DYN_CASES for s in SHAPES for b in (False, True)}
    assert got == want, sorted(map(str, want - got))


# ---- the device side ---------------------------------------------------------------------------------------------------------------------

_packed = {}
_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report(gpu, hip_lib):
    yield
    _packed.clear()
    for key in sorted(_worst):
        print(f"lpips conv layer, worst error / E32: {' '.join(key)}: {_worst[key]:.3f}")


def _note(bf16, shape, mode, ratio):
    key = ("bf16" if bf16 else "f32", shape, mode)
    _worst[key] = max(_worst.get(key, 0.0), ratio)


def packed(gpu, cin_f, cout_f, bf16):
    """(fwd, bwd, bias) of the forward layer cin_f -> cout_f on the device, packed by the library, once."""
    from moss_amd._lib import call
    key = (cin_f, cout_f, bf16)
    if key not in _packed:
        w, bias = layer_weights(cin_f, cout_f)
        wd = w.to(gpu).contiguous()
        dt = torch.bfloat16 if bf16 else torch.float32
        fwd, bwd = torch.empty(w.numel(), dtype=dt, device=gpu), torch.empty(w.numel(), dtype=dt, device=gpu)
        call("moss_lpips_vgg_pack_weights_bf16" if bf16 else "moss_lpips_vgg_pack_weights", gpu, cin_f, cout_f, wd.data_ptr(),
             fwd.data_ptr(), bwd.data_ptr())
        _packed[key] = (fwd, bwd, bias.to(gpu))
    return _packed[key]


def rows_of(t):
    """(N,C,H,W) -> (N H W, C): the kernels' channels-last rows."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def mask_words(mode, cin, cout, rows):
    """Random ReLU words for a masked gradient, (rows, cout / 32) uint32, seeded."""
    rng = np.random.RandomState((MODES.index(mode) * 1000003 + cin * 1009 + cout * 31 + rows) % (2 ** 31))
    return rng.randint(0, 2 ** 32, size=(rows, cout // 32), dtype=np.uint64).astype(np.uint32)


def bits_of(words, cout):
    """(rows, cout / 32) uint32 -> (rows, cout) bool: bit j of word k is channel 32 k + j."""
    w = np.ascontiguousarray(words).view(np.uint32).reshape(words.shape[0], cout // 32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(w.shape[0], cout).astype(bool)


class Launch:
    """One argument block with its buffers: `out` NaN-filled and `mask_out` sentinel-filled, SPARE rows behind the grid's."""

    def __init__(self, gpu, mode, cin, cout, nimg, H, W, bf16, shape, x_rows, words=None, cap=None, rect=None, level=0):
        from moss_amd._lib import LpipsConv3x3Args
        self.gpu, self.mode, self.cout = gpu, mode, cout
        fwd, bwd, bias = packed(gpu, *forward_layer(mode, cin, cout), bf16)
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
        a.mode, a.shape, a.bf16 = MODES.index(mode), shape, int(bf16)
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
        call("moss_lpips_vgg_conv3x3", self.gpu, ctypes.byref(self.args))
        torch.cuda.synchronize(self.gpu)
        return self.out.cpu(), None if self.mask is None else self.mask.cpu().numpy().view(np.uint32)


def check(ref, mode, nimg, H, W, out, mask, words, tag):
    """Everything a case asserts of one launch's (out, mask); returns the worst error / E32."""
    M, HW, cout = nimg * H * W, H * W, out.shape[1]
    # guards: every row < M written, every row >= M (the grid's unused rows and the spare ones) untouched
    assert not bool(torch.isnan(out[:M]).any()), f"{tag}: a row < M was not written"
    assert bool(torch.isnan(out[M:]).all()), f"{tag}: a row >= M was written"
    z64, mass, e32 = rows_of(ref["z64"]), rows_of(ref["mass"]), ref["e32"]
    if mode == "fwd":
        want = z64.relu()
    elif mode == "bwd_mask":
        keep = torch.from_numpy(bits_of(words, cout))
        want = torch.where(keep, z64, torch.zeros_like(z64))
        off = out[:M][~keep]
        assert bool((off == 0).all()) and not bool(torch.signbit(off).any()), f"{tag}: not +0 where the ReLU bit is clear"
    else:
        want = z64
    ratio = worst_ratio(out[:M], want, mass, e32)
    print(f"{tag}: worst error / E32 = {ratio:.3f} (E32 = {e32 / 2.0 ** -24:.2f} roundoffs of the mass)")
    assert ratio <= K, (tag, ratio)
    if mode == "fwd":
        assert (mask[HW:] == MASK_SENTINEL).all(), f"{tag}: a mask row beyond the first image was written"
        bits = bits_of(mask[:HW], cout)
        assert (bits == (out[:HW] > 0).numpy()).all(), f"{tag}: a sign bit differs from out > 0"
        sure = (z64[:HW].abs() > K * e32 * mass[:HW]).numpy()
        assert (bits == (z64[:HW] > 0).numpy())[sure].all(), f"{tag}: a sign bit differs from z64 > 0 away from zero"
        left_out = 1.0 - sure.mean()
        assert left_out <= LEFT_OUT, (tag, left_out)
    return ratio


def _launch_case(gpu, case, bf16, shape):
    mode, cin, cout, nimg, H, W = case
    ref = reference(mode, cin, cout, nimg, H, W, bf16)
    words = mask_words(mode, cin, cout, nimg * H * W) if mode == "bwd_mask" else None
    return ref, words, Launch(gpu, mode, cin, cout, nimg, H, W, bf16, shape, rows_of(ref["x"]), words)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_layer_matches_float64(gpu, hip_lib, case, bf16, shape):
    mode, cin, cout, nimg, H, W = case
    ref, words, launch = _launch_case(gpu, case, bf16, SHAPES[shape])
    out, mask = launch.run()
    tag = f"{'bf16' if bf16 else 'f32'} {shape} {_id(case)}"
    _note(bf16, shape, mode, check(ref, mode, nimg, H, W, out, mask, words, tag))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_the_launchers_own_choice(gpu, hip_lib, bf16):
    """shape = 0 is bit for bit the shape launch_conv's rule resolves to: the 128-row one when its grid has a workgroup per compute
    unit, else the 32-row one -- and not the other shape's bits (one layer on 306 rows)."""
    case = ("fwd", 512, 512, 2, 9, 17)
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    resolved = "rows128" if (306 + 127) // 128 * (512 // 64) >= cus else "rows32"
    got = _launch_case(gpu, case, bf16, 0)[2].run()
    same = _launch_case(gpu, case, bf16, SHAPES[resolved])[2].run()
    assert torch.equal(got[0][:306], same[0][:306]) and (got[1] == same[1]).all()
    other = _launch_case(gpu, case, bf16, 3 - SHAPES[resolved])[2].run()
    assert not torch.equal(got[0][:306], other[0][:306])                  # (the two shapes sum K in different orders)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_two_launches_are_bit_identical(gpu, hip_lib, bf16, shape):
    launch = _launch_case(gpu, ("fwd", 512, 512, 2, 9, 17), bf16, SHAPES[shape])[2]
    a, b = launch.run(), launch.run()
    assert torch.equal(a[0][:306], b[0][:306]) and (a[1] == b[1]).all()
    launch = _launch_case(gpu, ("bwd_mask", 512, 512, 1, 9, 17), bf16, SHAPES[shape])[2]
    assert torch.equal(launch.run()[0][:153], launch.run()[0][:153])


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("dcase", DYN_CASES, ids=lambda c: f"{c[0]}-{c[1]}to{c[2]}")
def test_dynamic_equals_the_static_call(gpu, hip_lib, dcase, bf16, shape):
    """The size read from the device (9 x 13 in a grid made for 12 x 16): bit-identical to the static call at 9 x 13 in the same
    shape, under the bar, and the guards hold at the ACTUAL M."""
    mode, cin, cout, nimg = dcase
    H, W = DYN_SIZE
    case = (mode, cin, cout, nimg, H, W)
    ref, words, static = _launch_case(gpu, case, bf16, SHAPES[shape])
    rect = torch.tensor(RECT, dtype=torch.int32, device=gpu)
    dyn = Launch(gpu, mode, cin, cout, nimg, 0, 0, bf16, SHAPES[shape], rows_of(ref["x"]), words, cap=CAP, rect=rect, level=LEVEL)
    (so, sm), (do, dm) = static.run(), dyn.run()
    M = nimg * H * W
    assert do.shape[0] == nimg * 12 * 16 + SPARE and torch.equal(do[:M], so[:M])
    tag = f"{'bf16' if bf16 else 'f32'} {shape} dyn {_id(case)}"
    _note(bf16, shape, mode, check(ref, mode, nimg, H, W, do, dm, words, tag))
    if mode == "fwd":
        assert (dm[:H * W] == sm[:H * W]).all()


def test_rect_rewritten_between_launches(gpu, hip_lib):
    """One argument block, launched at rect 37 x 53 and, rewritten on the device, at 20 x 33 (level 2: 9 x 13, then 5 x 8, the same
    input buffer read compactly at each size): each launch equals its static twin bit for bit and writes no row beyond its own M."""
    mode, cin, cout, nimg = "fwd", 128, 256, 2
    ref = reference(mode, cin, cout, nimg, DYN_SIZE[0], DYN_SIZE[1], False)
    x_rows = rows_of(ref["x"])
    for shape in SHAPES.values():
        rect = torch.tensor(RECT, dtype=torch.int32, device=gpu)
        dyn = Launch(gpu, mode, cin, cout, nimg, 0, 0, False, shape, x_rows, cap=CAP, rect=rect, level=LEVEL)
        for (w, h), (H, W) in (((53, 37), (9, 13)), ((33, 20), (5, 8))):
            rect.copy_(torch.tensor((1, 2, w, h), dtype=torch.int32))
            M = nimg * H * W
            do, dm = dyn.run()
            so, sm = Launch(gpu, mode, cin, cout, nimg, H, W, False, shape, x_rows[:M]).run()
            assert torch.equal(do[:M], so[:M]) and not bool(torch.isnan(do[:M]).any()) and bool(torch.isnan(do[M:]).all())
            assert (dm[:H * W] == sm[:H * W]).all() and (dm[H * W:] == MASK_SENTINEL).all()
