#!/usr/bin/env python3
"""Generates tests/golden/s3im.npz by IMPORTING the reference's own ``s3im_fun`` from a MOSS checkout (the other fixtures' generators
are separate and unchanged).

    python tests/golden/make_golden_s3im.py <path of a MOSS checkout>

Reference function exercised, on the CPU in float64, called as train_ZJU.py:123 calls it -- two (1,3,h,w) crops:
  utils/loss_utils.py   s3im_fun (:17-38), and through it ssim (:57-87)

Cases keyed <name>, each a (3,h,w) crop pair: ``a`` 97 x 131, ``b`` 64 x 48, ``c`` 1 x 1, ``d`` 3 x 2 (narrower than the window),
``e`` 424 x 172 (the person's rectangle of a 512 x 512 frame).  Per case: src_q, tar_q (3,h,w) uint8 -- the images are EXACTLY q / 128
(a textured blob on black, as MOSS's crops are; every value exact in float32); for R in (10, 3): value_r<R> float64 = the reference's
s3im_fun(src, tar, R), grad_r<R> float32 = its gradient w.r.t. src (float64 autograd, rounded once).  For ``e`` the gradient keeps the
rows listed in grad_rows only (top, middle and bottom bands: the whole of it would not fit the size limit of a committed file).
The CPU RNG state is checked to be unchanged by every call (batch 1: randperm(1) draws nothing).
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
CASES = {"a": (97, 131), "b": (64, 48), "c": (1, 1), "d": (3, 2), "e": (424, 172)}
REPEATS = (10, 3)
E_ROWS = np.r_[0:8, 208:216, 416:424]


def _pair(g, h, w):
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    blob = (((yy - 0.5 * h) / (0.4 * h + 0.5)) ** 2 + ((xx - 0.5 * w) / (0.35 * w + 0.5)) ** 2 < 1.0).double()
    tar = torch.round(torch.rand(3, h, w, generator=g, dtype=torch.float64) * 32) * 4 * blob      # (multiples of 4 / 128)
    src = torch.clamp(tar + torch.round(torch.randn(3, h, w, generator=g, dtype=torch.float64) * 16), 0, 128) * blob
    return src.to(torch.uint8), tar.to(torch.uint8)


def main(moss_root):
    sys.path.insert(0, moss_root)
    from utils.loss_utils import s3im_fun
    g = torch.Generator().manual_seed(20261016)
    out = {"e_grad_rows": E_ROWS.astype(np.int32)}
    for name, (h, w) in CASES.items():
        src_q, tar_q = _pair(g, h, w)
        out[f"{name}_src_q"], out[f"{name}_tar_q"] = src_q.numpy(), tar_q.numpy()
        for R in REPEATS:
            src = (src_q.double() / 128.0).unsqueeze(0).requires_grad_(True)
            tar = (tar_q.double() / 128.0).unsqueeze(0)
            state = torch.random.get_rng_state()
            v = s3im_fun(src, tar, repeat_time=R)
            assert torch.equal(state, torch.random.get_rng_state())
            v.backward()
            grad = src.grad[0].to(torch.float32).numpy()
            out[f"{name}_value_r{R}"] = np.float64(v.item())
            out[f"{name}_grad_r{R}"] = grad[:, E_ROWS] if name == "e" else grad
            print(f"{name} {h}x{w} R={R}: {v.item():.9f}")
    path = os.path.join(OUT, "s3im.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
