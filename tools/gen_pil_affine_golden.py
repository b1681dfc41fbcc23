#!/usr/bin/env python3
"""Writes tests/golden/pil_affine.npz: the bytes of Pillow's Image.transform((ow, oh), Image.AFFINE, m, resample=BILINEAR) on small
uint8 images, RGB and L, the yardstick of tf2_amd.align.warp_pil (and through it of tf2_roi_warp) where Pillow is not installed.
Run it where Pillow is; no test imports Pillow through this file.
  cases     int32 [n, 6]: channels (3: RGB, 1: L), h, w, oh, ow, family
  mats      float64 [n, 6]: the matrix as Pillow received it
  src       uint8, the source images [h, w, channels] of the cases back to back
  out       uint8, Pillow's results [oh, ow, channels] back to back
  pillow    the version that made them
Families: 0 a rotation by exactly 90 degrees, 1 by exactly 180, 2 by any angle (with a scale), 3 magnification 16x, 4 minification 8x,
5 sample coordinates exactly on 0, 0.5, w and h, 6 1 x N and N x 1 sources, 7 a matrix entirely outside the image, 8 a matrix rounded
to float32, 9 integer shifts of the identity."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "pil_affine.npz")

ROT90, ROT180, ROTATION, MAGNIFY, MINIFY, BOUNDARY, THIN, OUTSIDE, FLOAT32, SHIFT = range(10)


def rotation(deg: float, scale: float, h: int, w: int, oh: int, ow: int, shift=(0.0, 0.0)):
    """output -> source: rotate by deg and scale by `scale` about the centres of the two images, then shift in the source"""
    c, s = scale * math.cos(math.radians(deg)), scale * math.sin(math.radians(deg))
    ox, oy, cx, cy = ow / 2.0, oh / 2.0, w / 2.0 + shift[0], h / 2.0 + shift[1]
    return (c, -s, cx - c * ox + s * oy, s, c, cy - s * ox - c * oy)


def geometries():
    """[(channels, h, w, oh, ow, family, matrix)]"""
    f32 = lambda m: tuple(float(np.float32(v)) for v in m)
    g = [
        # exact quarter and half turns: the bytes themselves, turned
        (3, 5, 7, 7, 5, ROT90, (0.0, 1.0, 0.0, -1.0, 0.0, 5.0)), (1, 6, 4, 4, 6, ROT90, (0.0, -1.0, 4.0, 1.0, 0.0, 0.0)),
        (3, 5, 7, 9, 8, ROT90, (0.0, 1.0, -1.0, -1.0, 0.0, 6.0)),              # ... with a border outside the image
        (3, 5, 7, 5, 7, ROT180, (-1.0, 0.0, 7.0, 0.0, -1.0, 5.0)), (1, 8, 3, 9, 5, ROT180, (-1.0, 0.0, 4.0, 0.0, -1.0, 8.5)),
        # any angle, over the full circle, with scales on both sides of 1
        (3, 16, 20, 12, 14, ROTATION, rotation(17.0, 1.0, 16, 20, 12, 14)), (1, 16, 20, 12, 14, ROTATION, rotation(-63.5, 1.3, 16, 20, 12, 14)),
        (3, 11, 9, 15, 13, ROTATION, rotation(135.0, 0.6, 11, 9, 15, 13)), (1, 25, 31, 10, 9, ROTATION, rotation(201.25, 2.7, 25, 31, 10, 9)),
        (3, 13, 13, 16, 16, ROTATION, rotation(45.0, 1.0, 13, 13, 16, 16, (2.5, -3.25))),
        (3, 19, 23, 8, 21, ROTATION, rotation(-8.0, 0.9, 19, 23, 8, 21)), (1, 39, 37, 7, 6, ROTATION, rotation(300.0, 4.4, 39, 37, 7, 6)),
        (3, 10, 12, 11, 11, ROTATION, rotation(90.5, 1.0, 10, 12, 11, 11)), (1, 7, 8, 20, 24, ROTATION, rotation(33.0, 0.22, 7, 8, 20, 24)),
        # magnification 16x (upright, turned) and minification 8x
        (3, 2, 3, 32, 48, MAGNIFY, (0.0625, 0.0, 0.0, 0.0, 0.0625, 0.0)), (1, 3, 3, 32, 32, MAGNIFY, rotation(30.0, 0.0625, 3, 3, 32, 32)),
        (1, 2, 2, 30, 30, MAGNIFY, (0.0625, 0.0, 0.0625, 0.0, 0.0625, -0.03125)),
        (3, 40, 64, 5, 8, MINIFY, (8.0, 0.0, 0.0, 0.0, 8.0, 0.0)), (1, 39, 39, 6, 6, MINIFY, rotation(-40.0, 8.0, 39, 39, 6, 6)),
        (1, 33, 35, 4, 4, MINIFY, (8.0, 0.0, 0.5, 0.0, 8.0, 1.0)),
        # sample coordinates exactly on 0 and w (shift -0.5: fx = x), on 0.5 (the identity), on h, and on all of them at half scale
        (3, 4, 5, 6, 7, BOUNDARY, (1.0, 0.0, -0.5, 0.0, 1.0, -0.5)), (1, 4, 5, 6, 7, BOUNDARY, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)),
        (3, 3, 4, 9, 11, BOUNDARY, (0.5, 0.0, -0.25, 0.0, 0.5, -0.25)), (1, 5, 3, 12, 8, BOUNDARY, (0.5, 0.0, 0.0, 0.0, 0.5, 0.0)),
        (1, 4, 4, 6, 6, BOUNDARY, (-1.0, 0.0, 4.5, 0.0, -1.0, 4.5)),           # fx = 4 - x: w first, then w - 1 .. 0, then below 0
        (3, 6, 5, 7, 7, BOUNDARY, (0.0, 1.0, -0.5, 1.0, 0.0, -0.5)),           # the same on a transposition
        (1, 3, 3, 5, 5, BOUNDARY, (1.0, 0.0, -1.0, 0.0, 1.0, -1.0)),           # fx = x - 0.5: -0.5 outside, 2.5 the last half pixel
        # one row, one column, one pixel
        (3, 1, 9, 5, 9, THIN, (1.0, 0.0, 0.0, 0.0, 0.25, -0.125)), (1, 9, 1, 9, 4, THIN, (0.3, 0.0, -0.1, 0.0, 1.0, 0.0)),
        (3, 1, 12, 8, 8, THIN, rotation(20.0, 1.0, 1, 12, 8, 8)), (1, 14, 1, 8, 8, THIN, rotation(-70.0, 1.5, 14, 1, 8, 8)),
        (3, 1, 1, 3, 3, THIN, (0.5, 0.0, -0.25, 0.0, 0.5, -0.25)),
        # nothing of the image is reached
        (3, 4, 4, 3, 5, OUTSIDE, (1.0, 0.0, 1000.0, 0.0, 1.0, 1000.0)), (1, 4, 4, 3, 5, OUTSIDE, (1.0, 0.0, -1e30, 0.0, 1.0, 0.0)),
        (1, 4, 4, 2, 2, OUTSIDE, (1e300, 1e300, 1.0, -1e300, 1e300, 1.0)),     # products that overflow to infinities and their sum to NaN
        # matrices rounded to float32
        (3, 14, 17, 10, 12, FLOAT32, f32(rotation(27.0, 1.1, 14, 17, 10, 12))), (1, 21, 18, 9, 9, FLOAT32, f32(rotation(-115.0, 1.9, 21, 18, 9, 9))),
        (3, 8, 8, 12, 12, FLOAT32, f32(rotation(61.0, 0.37, 8, 8, 12, 12))),
        # integer shifts of the identity: the bytes themselves, 0 outside
        (3, 6, 7, 6, 7, SHIFT, (1.0, 0.0, 2.0, 0.0, 1.0, -1.0)), (1, 5, 5, 8, 9, SHIFT, (1.0, 0.0, -3.0, 0.0, 1.0, -2.0)),
    ]
    return g


def load(path: str = PATH):
    """[(family, source [h, w, c], matrix float64 [6], oh, ow, Pillow's bytes [oh, ow, c])] and the Pillow version"""
    z = np.load(path)
    out, s_at, o_at = [], 0, 0
    for (c, h, w, oh, ow, family), m in zip(z["cases"].tolist(), z["mats"]):
        src = z["src"][s_at:s_at + h * w * c].reshape(h, w, c)
        res = z["out"][o_at:o_at + oh * ow * c].reshape(oh, ow, c)
        s_at, o_at = s_at + h * w * c, o_at + oh * ow * c
        out.append((family, src, m.astype(np.float64), oh, ow, res))
    assert s_at == z["src"].size and o_at == z["out"].size
    return out, str(z["pillow"])


def pillow_affine(img, m, oh: int, ow: int) -> np.ndarray:
    """Pillow's own result for an [h, w, c] uint8 image (c 1: mode L, 3: RGB): uint8 [oh, ow, c]"""
    from PIL import Image
    c = img.shape[2]
    im = Image.fromarray(np.ascontiguousarray(img[:, :, 0])) if c == 1 else Image.fromarray(np.ascontiguousarray(img))
    assert im.mode == ("L" if c == 1 else "RGB")
    res = np.asarray(im.transform((ow, oh), Image.AFFINE, tuple(float(v) for v in m), resample=Image.BILINEAR))
    return res.reshape(oh, ow, c)


def main():
    import PIL
    cases, mats, srcs, outs = [], [], [], []
    for seed, (c, h, w, oh, ow, family, m) in enumerate(geometries()):
        rng = np.random.default_rng(2000 + seed)
        img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        if seed % 5 == 4:
            img = (rng.integers(0, 2, (h, w, c), dtype=np.uint8) * 255).astype(np.uint8)      # 0 / 255 bytes: the largest differences
        res = pillow_affine(img, m, oh, ow)
        assert res.dtype == np.uint8
        cases.append((c, h, w, oh, ow, family))
        mats.append(m)
        srcs.append(img.reshape(-1))
        outs.append(res.reshape(-1))
    np.savez_compressed(PATH, cases=np.asarray(cases, np.int32), mats=np.asarray(mats, np.float64), src=np.concatenate(srcs),
                        out=np.concatenate(outs), pillow=np.asarray(PIL.__version__))
    print(f"{PATH}: {len(cases)} cases, {os.path.getsize(PATH)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    sys.exit(main())
