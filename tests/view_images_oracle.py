"""The yardstick of the view-image tests: the contract of ``moss_view_images_prepare`` (include/moss_raster.h) restated in numpy,
and the inputs both test files share.  It does not import ``moss_amd.images``.

Arithmetic: the map in float64 arrays, the colour path in ``np.float32`` arrays (numpy rounds every array operation on its own and
never fuses two), the rounding mask rule in integers.  The tests compare bytes for equality: no tolerance, no excluded pixel."""
import functools

import numpy as np

F32 = np.float32
SIZES = ((8, 12), (36, 52), (64, 48))                      # (H0, W0); the factor 4 runs on (36, 52): 13 output columns, 117 output pixels
LENSES = ("zero", "mild", "strong")
MILD = (-0.2, 0.1, 1e-3, -2e-3, 0.01)
STRONG = (1.5, 0.0, 0.0, 0.0, 0.0)                          # border samples leave the image on every side


def scales_of(size):
    return (1, 2, 4) if size == (36, 52) else (1, 2)


def lens(name, H0, W0, B, half_pixel_centre=False):
    """K (B,3,3) and D (B,5) float64: every view its own principal point and focal lengths."""
    K = np.zeros((B, 3, 3))
    for b in range(B):
        fx, fy = 0.9 * W0 + 1.7 * b, 0.95 * W0 - 0.6 * b
        cx, cy = W0 / 2 - 0.37 + 0.13 * b, H0 / 2 + 0.21 - 0.09 * b
        if half_pixel_centre:
            cx, cy = W0 // 2 + 0.5, H0 // 2 - 0.5
        K[b] = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]
    D = np.zeros((B, 5))
    if name == "mild":
        D[:] = MILD
    elif name == "strong":
        D[:] = STRONG
    else:
        assert name == "zero"
    return K, D


def raw_views(B, H0, W0, mode, seed=0, checkerboard=False):
    """rgb (B,H0,W0,3) random bytes; mask (B,H0,W0): a blob, lines and gaps one pixel wide, foreground bytes 1 and 255 mixed; with
    mode "any" some values in between.  ``checkerboard``: the mask alternates pixel by pixel."""
    rng = np.random.Generator(np.random.PCG64(1000 * H0 + W0 + 7 * seed))
    rgb = rng.integers(0, 256, size=(B, H0, W0, 3), dtype=np.uint8)
    rgb[:, :2, :3] = 255                                     # (both ends of the byte range are there)
    rgb[:, -2:, -3:] = 0
    yy, xx = np.meshgrid(np.arange(H0), np.arange(W0), indexing="ij")
    mask = np.zeros((B, H0, W0), dtype=np.uint8)
    for b in range(B):
        if checkerboard:
            mask[b] = (((yy + xx + b) & 1) * 255).astype(np.uint8)
            continue
        cy, cx = H0 * (0.45 + 0.03 * b), W0 * (0.5 - 0.02 * b)
        blob = ((yy - cy) / (0.33 * H0)) ** 2 + ((xx - cx) / (0.3 * W0)) ** 2 <= 1.0
        blob[H0 // 3, :] = True                              # a row, a column and a diagonal one pixel wide, reaching the borders
        blob[:, (W0 // 4 + b) % W0] = True
        blob[yy == (xx * H0) // W0] = True
        blob[(H0 // 2 + b) % H0, :] = False                  # gaps one pixel wide through the blob
        blob[:, W0 // 2] = False
        value = np.where(rng.random((H0, W0)) < 0.5, 255, 1)
        if mode == "any":
            value = np.where(rng.random((H0, W0)) < 0.3, rng.integers(1, 255, size=(H0, W0)), value)
        mask[b] = np.where(blob, value, 0).astype(np.uint8)
    return rgb, mask


def _pairwise(values):
    """The balanced tree over a list: neighbours first."""
    values = list(values)
    while len(values) > 1:
        values = [values[k] + values[k + 1] for k in range(0, len(values), 2)]
    return values[0]


def prepare_oracle(rgb, mask, K, D, scale, white_background, mode):
    """gt_u8 (B,3,H,W), bkgd_u8 (B,H,W) and a dict of counts: samples whose four taps all lie beyond the left / right / top / bottom
    border, non-finite samples, and exact-half ties of the rounding rule."""
    B, H0, W0, _ = rgb.shape
    assert H0 % scale == 0 and W0 % scale == 0
    H, W = H0 // scale, W0 // scale
    gt = np.zeros((B, 3, H, W), dtype=np.uint8)
    bkgd = np.zeros((B, H, W), dtype=np.uint8)
    counts = dict(left=0, right=0, top=0, bottom=0, nonfinite=0, ties=0)
    unit = np.arange(256, dtype=F32) / F32(255)
    for b in range(B):
        fx, fy, cx, cy = (np.float64(K[b][0][0]), np.float64(K[b][1][1]), np.float64(K[b][0][2]), np.float64(K[b][1][2]))
        k1, k2, p1, p2, k3 = (np.float64(v) for v in D[b])
        with np.errstate(all="ignore"):
            u = np.arange(W0, dtype=np.float64)[None, :]
            v = np.arange(H0, dtype=np.float64)[:, None]
            x = np.broadcast_to((u - cx) / fx, (H0, W0))
            y = np.broadcast_to((v - cy) / fy, (H0, W0))
            x2 = x * x
            y2 = y * y
            r2 = x2 + y2
            xy2 = (2.0 * x) * y
            kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
            xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2)
            yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2
            su = fx * xd + cx
            sv = fy * yd + cy
            iu = np.rint(su * 32.0)
            iv = np.rint(sv * 32.0)
            usable = np.isfinite(iu) & np.isfinite(iv) & (np.abs(iu) < 2.0 ** 30) & (np.abs(iv) < 2.0 ** 30)
        counts["nonfinite"] += int((~usable).sum())
        qu = np.where(usable, iu, 0.0).astype(np.int64)
        qv = np.where(usable, iv, 0.0).astype(np.int64)
        ix, ax = qu >> 5, qu & 31
        iy, ay = qv >> 5, qv & 31
        counts["left"] += int((usable & (ix + 1 < 0)).sum())
        counts["right"] += int((usable & (ix >= W0)).sum())
        counts["top"] += int((usable & (iy + 1 < 0)).sum())
        counts["bottom"] += int((usable & (iy >= H0)).sum())

        def tap(image, tx, ty):
            inside = usable & (tx >= 0) & (tx < W0) & (ty >= 0) & (ty < H0)
            got = image[np.clip(ty, 0, H0 - 1), np.clip(tx, 0, W0 - 1)]
            return np.where(inside if got.ndim == 2 else inside[..., None], got, 0)
        c = [tap(rgb[b], ix + dx, iy + dy) for dy in (0, 1) for dx in (0, 1)]              # 00, 01, 10, 11
        t = [tap(mask[b], ix + dx, iy + dy) for dy in (0, 1) for dx in (0, 1)]
        bx, by = ax.astype(F32) / F32(32), ay.astype(F32) / F32(32)
        weights = [(F32(1) - by) * (F32(1) - bx), (F32(1) - by) * bx, by * (F32(1) - bx), by * bx]

        def bilinear(taps):
            p = [unit[q] for q in taps]
            w = weights if p[0].ndim == 2 else [k[..., None] for k in weights]
            return ((p[0] * w[0] + p[1] * w[1]) + p[2] * w[2]) + p[3] * w[3]
        colour = bilinear(c)
        assert colour.dtype == F32
        if mode == "round":
            parts = [(32 - ax) * (32 - ay), ax * (32 - ay), (32 - ax) * ay, ax * ay]
            total = sum(np.where(q != 0, w, 0) for q, w in zip(t, parts))
            counts["ties"] += int((total == 512).sum())
            foreground = total >= 512
            m = foreground.astype(F32)
        else:
            m = bilinear(t)
            foreground = m != 0
        colour = np.where(foreground[..., None], colour, F32(1 if white_background else 0)).astype(F32)
        samples = [colour[dy::scale, dx::scale] for dy in range(scale) for dx in range(scale)]        # row-major
        mean = _pairwise(samples)
        if scale > 1:
            mean = mean * F32(1.0 / (scale * scale))
        assert mean.dtype == F32
        gt[b] = np.trunc(mean * F32(255)).astype(np.uint8).transpose(2, 0, 1)
        bkgd[b] = np.trunc(m[::scale, ::scale] * F32(255)).astype(np.uint8)
    return gt, bkgd, counts


@functools.lru_cache(maxsize=None)
def case(size, scale, lens_name, mode, white_background, B=9, half_pixel_centre=False, checkerboard=False):
    """One shared case, computed once: (rgb, mask, K, D, gt_u8, bkgd_u8, counts), all numpy and not to be written to.  The first views
    of a case of 9 are the cases of 1 and 3: every view is computed on its own."""
    H0, W0 = size
    rgb, mask = raw_views(B, H0, W0, mode, checkerboard=checkerboard)
    K, D = lens(lens_name, H0, W0, B, half_pixel_centre)
    gt, bkgd, counts = prepare_oracle(rgb, mask, K, D, scale, white_background, mode)
    for a in (rgb, mask, K, D, gt, bkgd):
        a.setflags(write=False)
    return rgb, mask, K, D, gt, bkgd, counts
