"""One wide convolution of the LPIPS term (C ABI moss_lpips_vgg_conv3x3), without a GPU: the float64 references and the per-element bar the
GPU file (tests/test_gpu_lpips_conv_layer.py) judges the kernels by, that bar applied to references that were broken on purpose, the
ctypes mirror of the argument block against the header, the refusals of the entry point, and the largest H and W the convolution
kernels' packing of a pixel can hold.

The bar.  An element's error is measured in units of its MASS, conv(|in|, |w|) + |bias| in float64 (from the rounded operands for
bf16): the sum of the magnitudes a float32 sum of it rounds.  The yardstick E32 is the reference's own float32 error in those
units, measured when the test runs: the larger of the worst |z32 - z64| / mass of torch's float32 convolution (contiguous and
channels-last) on the case's inputs, and the same for a plain sequential float32 accumulation in tap-major order -- the order class
of the kernels' fmaf chain -- on the 5 x 7 inputs of the same layer.  A result passes when max |result - z64| / mass <= K E32,
K = 8 (the project's parity factor: tests/test_gpu_pose.py, tests/test_gpu_lpips.py).  No element is excluded.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from tests.helpers import c_layout, ctypes_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 8.0
MODES = ("fwd", "bwd_mask", "bwd_plain")                  # moss_lpips_conv3x3_args.mode 0, 1, 2
SMALL = (5, 7)                                            # the size the sequential float32 sum is taken at


# ---- inputs and references, shared with the GPU file ---------------------------------------------------------------------------------

def _seed(*key):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31 - 1)


@functools.lru_cache(maxsize=None)
def layer_weights(cin_f, cout_f):
    """(w (cout_f,cin_f,3,3), bias (cout_f,)) float32 of a FORWARD layer cin_f -> cout_f: w = randn / sqrt(9 cin), bias = 0.1 randn."""
    gen = torch.Generator().manual_seed(_seed(1, cin_f, cout_f))
    w = torch.randn(cout_f, cin_f, 3, 3, generator=gen) / (9.0 * cin_f) ** 0.5
    return w, 0.1 * torch.randn(cout_f, generator=gen)


def forward_layer(mode, cin, cout):
    """The (cin_f, cout_f) of the forward layer a CALL with cin -> cout belongs to: a data gradient runs from its outputs to its inputs."""
    return (cin, cout) if mode == "fwd" else (cout, cin)


def rounded(t, bf16):
    """The operand as the kernel multiplies it, in float64."""
    return (t.bfloat16() if bf16 else t).double()


def correlate(x, w, bias=None):
    return F.conv2d(x, w, bias, padding=1)


def sequential_float32(x, w_corr, bias=None):
    """conv2d(x, w_corr, bias, padding=1) as ONE float32 sum per element in tap-major order, k = tap * C + c ascending, the bias added
    last: a numpy im2col loop.  x (N,C,H,W), w_corr (Cout,C,3,3) float32 -> (N,Cout,H,W) float32."""
    N, C, H, W = x.shape
    xp = np.pad(x.numpy().astype(np.float32), ((0, 0), (0, 0), (1, 1), (1, 1)))
    cols = np.stack([xp[:, :, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], axis=1)         # (N, 9, C, H, W)
    a = np.ascontiguousarray(cols.reshape(N, 9 * C, H * W).transpose(1, 0, 2).reshape(9 * C, N * H * W, 1))
    b = np.ascontiguousarray(w_corr.numpy().astype(np.float32).transpose(2, 3, 1, 0).reshape(9 * C, 1, -1))
    acc = np.zeros((N * H * W, b.shape[2]), dtype=np.float32)
    tmp = np.empty_like(acc)
    for k in range(9 * C):
        np.multiply(a[k], b[k], out=tmp)
        acc += tmp
    if bias is not None:
        acc += bias.numpy().astype(np.float32)[None]
    return torch.from_numpy(acc.reshape(N, H, W, -1)).permute(0, 3, 1, 2).contiguous()


def _operands(mode, cin, cout, nimg, H, W, bf16):
    """(x float32 as the device gets it, xr / wr the rounded operands in float64, w, bias) of a case; x is relu(randn) for the forward
    (half the values zero, like activations) and randn for a gradient."""
    w, bias = layer_weights(*forward_layer(mode, cin, cout))
    gen = torch.Generator().manual_seed(_seed(2, MODES.index(mode), cin, cout, nimg, H, W))
    x = torch.randn(nimg, cin, H, W, generator=gen)
    if mode == "fwd":
        x = x.relu()
    return x, rounded(x, bf16), rounded(w, bf16), w, bias


def _float32_errors(mode, xr, wr, bias, z64, mass, sequential):
    """The worst |z32 - z64| / mass of the float32 forms of the reference on the (rounded) operands."""
    x32, w32 = xr.float(), wr.float()                                    # (exact: the operands are float32 or bf16 values)
    worst = 0.0
    for cl in (False, True):
        xi = x32.contiguous(memory_format=torch.channels_last) if cl else x32
        wi = w32.contiguous(memory_format=torch.channels_last) if cl else w32
        z32 = F.conv2d(xi, wi, bias, padding=1) if mode == "fwd" else F.conv_transpose2d(xi, wi, padding=1)
        worst = max(worst, float(((z32.double() - z64).abs() / mass).max()))
    if sequential:
        w_corr = w32 if mode == "fwd" else w32.flip(2, 3).transpose(0, 1).contiguous()
        z32 = sequential_float32(x32, w_corr, bias if mode == "fwd" else None)
        worst = max(worst, float(((z32.double() - z64).abs() / mass).max()))
    return worst


@functools.lru_cache(maxsize=None)
def reference(mode, cin, cout, nimg, H, W, bf16):
    """The case, computed once and shared: {x (nimg,cin,H,W) float32 the device's input, w, bias float32, z64 the float64 result BEFORE
    any ReLU or mask (nimg,cout,H,W), mass, e32}.  Forward: conv2d; data gradient: conv_transpose2d(dz, w, padding=1) on the UNPACKED
    weights, so the `bwd` packing is checked along the way."""
    x, xr, wr, w, bias = _operands(mode, cin, cout, nimg, H, W, bf16)
    if mode == "fwd":
        z64 = F.conv2d(xr, wr, bias.double(), padding=1)
        mass = F.conv2d(xr.abs(), wr.abs(), bias.double().abs(), padding=1)
    else:
        z64 = F.conv_transpose2d(xr, wr, padding=1)
        mass = F.conv_transpose2d(xr.abs(), wr.abs(), padding=1)
    assert float(mass.min()) > 0.0
    e32 = _float32_errors(mode, xr, wr, bias if mode == "fwd" else None, z64, mass, sequential=(H, W) == SMALL)
    if (H, W) != SMALL:
        e32 = max(e32, reference(mode, cin, cout, 2 if mode == "fwd" else 1, SMALL[0], SMALL[1], bf16)["e32"])
    assert e32 > 0.0
    return {"x": x, "w": w, "bias": bias, "z64": z64, "mass": mass, "e32": e32}


def worst_ratio(got, want64, mass, e32):
    """max over EVERY element of |got - want64| / mass, in units of e32.  A NaN anywhere is infinitely wrong."""
    r = (got.double() - want64).abs() / mass
    return float("inf") if bool(torch.isnan(r).any()) else float(r.max()) / e32


def within_bar(got, want64, mass, e32):
    return worst_ratio(got, want64, mass, e32) <= K


# ---- the checker bites -----------------------------------------------------------------------------------------------------------------

def _mutations(xr, wr, b64):
    """name -> a float64 forward result that is wrong the way a kernel could be."""
    N, C, H, W = xr.shape
    out = {}
    w = wr.clone()
    w[:, 64 * (C // 64 - 1):, 1, 2] = 0                                   # one (tap, 64-channel slice) dropped
    out["slice dropped"] = F.conv2d(xr, w, b64, padding=1)
    w = wr.clone()
    ci = int((xr[:, :, 1:-1, 1:-1].abs().sum((0, 2, 3)) > 0).nonzero()[0])          # (a channel that is not all zero)
    w[3, ci, 1, 1] = 0                                                    # one product term
    out["one weight dropped"] = F.conv2d(xr, w, b64, padding=1)
    xp = F.pad(xr, (1, 1, 1, 1))
    xp[:, :, 1:-1, 0] = xr[:, :, :, 0]                                    # the left border replicated where it is zero padding
    out["edge replicated"] = F.conv2d(xp, wr, b64)
    xp = F.pad(xr, (1, 1, 1, 1))
    xp[0, :, H + 1, 1:-1] = xr[1, :, 0, :]                                # image 0's last row sees image 1's first row below it
    out["images joined"] = F.conv2d(xp, wr, b64)
    return out


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("cin, cout", [(64, 64), (128, 256), (512, 512)])
def test_the_bar_fails_broken_references(cin, cout, bf16):
    """Four ways a layer could be slightly wrong, applied to the float64 reference: each fails K E32, on the forward and under the
    ReLU; torch's own float32 result passes."""
    ref = reference("fwd", cin, cout, 2, SMALL[0], SMALL[1], bf16)
    _, xr, wr, _, bias = _operands("fwd", cin, cout, 2, SMALL[0], SMALL[1], bf16)
    z64, mass, e32 = ref["z64"], ref["mass"], ref["e32"]
    eps = 2.0 ** -24
    print(f"conv {cin}->{cout} {'bf16' if bf16 else 'f32'}: E32 = {e32 / eps:.2f} unit roundoffs of the mass")
    # a float32 sum's error and not a loose number: above half a roundoff (the last rounding alone), below the sqrt(n) roundoffs a
    # random walk of the n = 9 cin roundings of a sequential sum reaches
    assert eps / 2 < e32 < (9.0 * cin) ** 0.5 * eps
    z32 = F.conv2d(xr.float(), wr.float(), bias, padding=1)
    assert within_bar(z32, z64, mass, e32) and within_bar(z32.relu(), z64.relu(), mass, e32)
    assert within_bar(z64, z64, mass, e32)
    for name, bad in _mutations(xr, wr, bias.double()).items():
        r, rr = worst_ratio(bad, z64, mass, e32), worst_ratio(bad.relu(), z64.relu(), mass, e32)
        print(f"    {name}: worst error {r:.0f} E32 ({rr:.0f} under the ReLU)")
        assert not within_bar(bad, z64, mass, e32), name
        assert not within_bar(bad.relu(), z64.relu(), mass, e32), name
    nan = z32.clone()
    nan[0, 0, 0, 0] = float("nan")
    assert not within_bar(nan, z64, mass, e32)


def test_sequential_sum_is_the_convolution():
    """The numpy loop computes the same convolution (to float32), forward and, on flipped and transposed weights, data gradient."""
    for mode, cin, cout in (("fwd", 64, 128), ("bwd_plain", 128, 64)):
        x, xr, wr, w, bias = _operands(mode, cin, cout, 2, 3, 4, False)
        if mode == "fwd":
            want, got = F.conv2d(xr, wr, bias.double(), padding=1), sequential_float32(x, w, bias)
        else:
            want, got = F.conv_transpose2d(xr, wr, padding=1), sequential_float32(x, w.flip(2, 3).transpose(0, 1).contiguous())
        assert got.shape == want.shape and float((got.double() - want).abs().max()) < 1e-5 * float(want.abs().max())


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------

def test_argument_block_mirrors_the_header(tmp_path):
    """sizeof and every offsetof as gcc sees the header (``in`` is ``in_`` in Python); the entry point is declared outside the
    diagnostic block and the version did not move."""
    from moss_amd._lib import LpipsConv3x3Args as cls
    fields = [f[0] for f in cls._fields_]
    assert fields == ["in_", "weights", "bias", "out", "mask_in", "mask_out", "nimg", "H", "W", "cin", "cout", "mode", "shape", "bf16",
                      "rect", "cap_H", "cap_W", "level"]
    assert c_layout(tmp_path, "moss_lpips_conv3x3_args", fields) == ctypes_layout(cls)
    z = cls()
    assert z.shape == 0 and z.cap_H == 0 and z.cap_W == 0                 # zero-initialised: the launcher's choice, the static call


def test_c_abi_is_declared():
    text = open(os.path.join(ROOT, "include", "moss_raster.h")).read()
    assert "int moss_lpips_vgg_conv3x3(const moss_lpips_conv3x3_args* args, void* stream);" in text
    assert text.index("moss_lpips_vgg_conv3x3(") < text.index("#ifdef MOSS_DIAG")
    assert "#define MOSS_ABI_VERSION 7" in text
    assert "bit j of word k of row m is channel 32 k + j" in text        # the mask word layout is documented


FAKE = 0x1000                                             # a non-NULL address nothing reads: every call below returns before a launch


def _block(**kw):
    from moss_amd._lib import LpipsConv3x3Args
    a = LpipsConv3x3Args()
    a.in_, a.weights, a.bias, a.out, a.mask_in = FAKE, FAKE, FAKE, FAKE, FAKE
    a.nimg, a.H, a.W, a.cin, a.cout = 2, 5, 7, 64, 64
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _refused(hip_lib, block, text):
    rc = hip_lib.moss_lpips_vgg_conv3x3(ctypes.byref(block) if block is not None else None, None)
    msg = hip_lib.moss_last_error().decode()
    assert rc == -1, (rc, msg, text)                                      # MOSS_ERR_INVALID_ARG
    assert msg.startswith("moss_lpips_vgg_conv3x3") and text in msg, (msg, text)


def test_refusals(hip_lib):
    """Through the library, before any launch (there is no device here)."""
    _refused(hip_lib, None, "null argument block")
    for field in ("in_", "weights", "out"):
        _refused(hip_lib, _block(**{field: None}), "null in, weights or out")
    _refused(hip_lib, _block(bias=None), "needs bias")
    _refused(hip_lib, _block(mode=1, mask_in=None), "needs mask_in")
    for field in ("cin", "cout"):
        for v in (0, -64, 32, 96, 65):
            _refused(hip_lib, _block(**{field: v}), "multiples of 64")
    for v in (-1, 3):
        _refused(hip_lib, _block(mode=v), "mode must be")
        _refused(hip_lib, _block(shape=v), "shape must be")
    for v in (-1, 2):
        _refused(hip_lib, _block(bf16=v), "bf16 must be")
    for v in (0, 3, -1):
        _refused(hip_lib, _block(nimg=v), "nimg must be")
    for field in ("H", "W"):
        for v in (0, -5):
            _refused(hip_lib, _block(**{field: v}), ">= 1")
    _refused(hip_lib, _block(cap_H=48, cap_W=64), "needs rect")
    _refused(hip_lib, _block(cap_H=48, rect=FAKE), "both be set")
    _refused(hip_lib, _block(cap_W=64, rect=FAKE), "both be set")
    _refused(hip_lib, _block(cap_H=15, cap_W=64, rect=FAKE), "capacity must be >= 16")
    _refused(hip_lib, _block(cap_H=48, cap_W=64, rect=FAKE, level=5), "level must be")
    _refused(hip_lib, _block(cap_H=48, cap_W=64, rect=FAKE, level=-1), "level must be")


# ---- the sizes the kernels' packing holds ------------------------------------------------------------------------------------------------

MAX_H, MAX_W = 1 << 15, 1 << 16


def test_packing_limit_derivation():
    """Both kernels keep a row's pixel as (y << 16) | x in a signed 32-bit int and read x = v & 0xffff, y = v >> 16 (arithmetic).  The
    round trip holds exactly for x <= 65535 and y <= 32767, that is W <= 65536 and H <= 32768, and fails one past either."""
    def roundtrip(y, x):
        v = np.array([(y << 16) | x], dtype=np.uint64).astype(np.uint32).view(np.int32)[0]       # what the int holds
        return int(v >> 16), int(v & 0xffff)
    for y, x in ((0, 0), (MAX_H - 1, MAX_W - 1), (MAX_H - 1, 0), (0, MAX_W - 1), (12345, 54321)):
        assert roundtrip(y, x) == (y, x)
    assert roundtrip(0, MAX_W) != (0, MAX_W)                              # x spills into y
    assert roundtrip(MAX_H, 0) != (MAX_H, 0)                              # y reaches the sign bit


def test_sizes_beyond_the_packing_are_refused(hip_lib):
    """H * W <= 2^22 admits 16 x 262144: the byte-size queries return 0 beyond H = 32768 or W = 65536, the full calls and the one-layer
    call refuse with a text -- and the largest sizes the packing does hold are still accepted."""
    from moss_amd._lib import LpipsVggArgs, LpipsVggBackwardArgs
    for q in (hip_lib.moss_lpips_vgg_workspace_bytes, hip_lib.moss_lpips_vgg_saved_bytes):
        for H, W in ((16, 70000), (40000, 16), (16, MAX_W + 1), (MAX_H + 1, 16), (16, 1 << 18), (1 << 18, 16)):
            assert q(H, W) == 0, (H, W)
        for H, W in ((16, MAX_W), (MAX_H, 16), (64, MAX_W), (MAX_H, 128), (2048, 2048), (16, 16)):
            assert q(H, W) > 0, (H, W)
        assert q(15, 16) == 0 and q(2048, 2049) == 0                      # (the limits there were)
    for name, cls in (("moss_lpips_vgg_forward", LpipsVggArgs), ("moss_lpips_vgg_backward", LpipsVggBackwardArgs),
                      ("moss_lpips_vgg_forward_bf16", LpipsVggArgs), ("moss_lpips_vgg_backward_bf16", LpipsVggBackwardArgs)):
        for H, W in ((16, 70000), (40000, 16)):
            a = cls()
            a.H, a.W = H, W
            assert getattr(hip_lib, name)(ctypes.byref(a), None) == -1
            msg = hip_lib.moss_last_error().decode()
            assert msg.startswith(name + ":") and "H <= 32768, W <= 65536" in msg, msg
            a = cls()
            a.cap_H, a.cap_W, a.rect = H, W, FAKE
            assert getattr(hip_lib, name)(ctypes.byref(a), None) == -1
            msg = hip_lib.moss_last_error().decode()
            assert "capacity must be >= 16" in msg and "cap_H <= 32768, cap_W <= 65536" in msg, msg
    for H, W in ((16, 70000), (40000, 16), (1, MAX_W + 1), (MAX_H + 1, 1), (2048, 2049)):
        _refused(hip_lib, _block(H=H, W=W), "H <= 32768, W <= 65536 and H * W <= 2^22")
        _refused(hip_lib, _block(cap_H=max(H, 16), cap_W=max(W, 16), rect=FAKE), "capacity must be >= 16")
    text = open(os.path.join(ROOT, "include", "moss_raster.h")).read()
    assert "H <= 32768, W <= 65536" in text
