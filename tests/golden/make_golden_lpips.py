"""Regenerates tests/golden/lpips_vgg.npz from the reference's own modules:

    python tests/golden/make_golden_lpips.py <MOSS checkout>

``VGG16``, ``BaseNet.forward``, ``LinLayers`` and ``LPIPS.forward`` (lpipsPyTorch/modules) are imported from the checkout and run on the
CPU.  Nothing is downloaded: a stub ``torchvision.models`` sits in ``sys.modules`` for the duration (its ``vgg16(...)`` returns an
unpretrained ``features`` Sequential of the standard layout), and ``LPIPS`` is built via ``__new__`` so that ``get_state_dict`` is
never reached.  The weights are ``moss_amd.lpips.synthetic_weights(SEED)`` -- 14.7 M values from a frozen ``numpy.random.RandomState``
stream, rebuilt by the tests at run time; the fixture stores their SHA-256.

Cases (images in [0,1]; y = clip(x + 0.15 normal)):

* ``min``   16x16 -- conv5 runs on 1x1;
* ``odd``   37x53 -- every pool floors, nothing divides a tile;
* ``strip`` 16x40 -- the deep layers are one row high;
* ``same``  20x28, y = x -- value and gradient are exactly 0.

Stored per case: ``x``, ``y``, the five per-tap terms and the total in float64, dL/dx of the total in float64 rounded once to float32,
and the reference's own float32 errors over TWO float32 runs (contiguous and channels-last; a single scalar's float32 error can be
accidentally tiny): ``value_err32`` = the largest |float32 - float64| over the five terms and their sum over both runs,
``grad_err32_max`` / ``grad_err32_l2`` = the larger of the two runs' max-norm / L2 gradient errors.  The float32 runs are made on
ONE CPU thread: the CPU convolutions split their sums by the size of the thread team, so a float32 result is only repeatable (and the
test that the torch form stays within these numbers only meaningful) at a fixed team size.
"""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
SEED = 20240917
CASES = {"min": (16, 16, 1), "odd": (37, 53, 2), "strip": (16, 40, 3), "same": (20, 28, 4)}


def stub_torchvision():
    def vgg16(weights=None, **_):
        cfg = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]
        layers, cin = [], 3
        for v in cfg:
            if v == "M":
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        return types.SimpleNamespace(features=nn.Sequential(*layers))

    tv = types.ModuleType("torchvision")
    models = types.ModuleType("torchvision.models")
    models.vgg16 = vgg16
    models.VGG16_Weights = types.SimpleNamespace(IMAGENET1K_V1=None)
    tv.models = models
    return {"torchvision": tv, "torchvision.models": models}


def main(checkout):
    from moss_amd.lpips import synthetic_weights, weights_sha256
    stubs = stub_torchvision()
    before = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    sys.path.insert(0, checkout)
    try:
        from lpipsPyTorch.modules.lpips import LPIPS
        from lpipsPyTorch.modules.networks import VGG16, LinLayers
        params = synthetic_weights(SEED)

        def module(dtype):
            lp = LPIPS.__new__(LPIPS)
            nn.Module.__init__(lp)
            lp.net = VGG16()
            lp.lin = LinLayers(lp.net.n_channels_list)
            convs = [m for m in lp.net.layers if isinstance(m, nn.Conv2d)]
            assert len(convs) == 13
            with torch.no_grad():
                for m, w, b in zip(convs, params["conv_weights"], params["conv_biases"]):
                    m.weight.copy_(w)
                    m.bias.copy_(b)
                for seq, w in zip(lp.lin, params["lin_weights"]):
                    seq[1].weight.copy_(w.reshape(1, -1, 1, 1))
            return lp.to(dtype)

        def run(lp, x, y, channels_last=False):
            x = x.clone()[None]
            y = y.clone()[None]
            if channels_last:
                x, y = x.contiguous(memory_format=torch.channels_last), y.contiguous(memory_format=torch.channels_last)
            x.requires_grad_(True)
            fx, fy = lp.net(x), lp.net(y)                                          # LPIPS.forward, with the per-tap terms kept
            res = [l((a - b) ** 2).mean((2, 3), True) for a, b, l in zip(fx, fy, lp.lin)]
            total = lp(x, y)
            assert total.shape == (1, 1, 1, 1)
            assert torch.equal(total, torch.sum(torch.cat(res, 0), 0, True))
            (g,) = torch.autograd.grad(total.sum(), x)
            return torch.cat(res, 0).reshape(5).detach(), total.detach().reshape(()), g[0].contiguous()

        lp64, lp32 = module(torch.float64), module(torch.float32)
        lp32cl = module(torch.float32).to(memory_format=torch.channels_last)
        rec = {"weights_sha256": weights_sha256(params), "seed": np.int64(SEED)}
        for case, (H, W, seed) in CASES.items():
            rng = np.random.RandomState(seed)
            x = rng.uniform(0, 1, size=(3, H, W)).astype(np.float32)
            y = x.copy() if case == "same" else np.clip(x + 0.15 * rng.standard_normal((3, H, W)), 0, 1).astype(np.float32)
            x, y = torch.from_numpy(x), torch.from_numpy(y)
            t64, v64, g64 = run(lp64, x.double(), y.double())
            threads = torch.get_num_threads()
            torch.set_num_threads(1)
            try:
                runs = [run(lp32, x, y), run(lp32cl, x, y, channels_last=True)]
            finally:
                torch.set_num_threads(threads)
            verr = max(max(float((t.double() - t64).abs().max()), float((v.double() - v64).abs())) for t, v, _ in runs)
            gmax = max(float((g.double() - g64).abs().max()) for _, _, g in runs)
            gl2 = max(float((g.double() - g64).norm()) for _, _, g in runs)
            rec.update({f"{case}_x": x.numpy(), f"{case}_y": y.numpy(), f"{case}_terms": t64.numpy(), f"{case}_total": np.float64(v64),
                        f"{case}_grad": g64.numpy().astype(np.float32), f"{case}_value_err32": np.float64(verr),
                        f"{case}_grad_err32_max": np.float64(gmax), f"{case}_grad_err32_l2": np.float64(gl2)})
            print(case, (H, W), "total %.6g" % float(v64), "value_err32 %.3g" % verr, "grad max %.3g" % float(g64.abs().max()),
                  "grad_err32 max %.3g l2 %.3g" % (gmax, gl2), "runs differ: value x%.1f" % (
                      max(float((t.double() - t64).abs().max()) for t, _, _ in runs)
                      / max(min(float((t.double() - t64).abs().max()) for t, _, _ in runs), 1e-300)))
        np.savez(os.path.join(HERE, "lpips_vgg.npz"), **rec)
    finally:
        for k, v in before.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


if __name__ == "__main__":
    main(sys.argv[1])
