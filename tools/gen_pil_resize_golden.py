#!/usr/bin/env python3
"""Writes tests/golden/pil_resize.npz: the bytes of Pillow's Image.resize((rw, rh), BILINEAR) on small RGB uint8 images, the yardstick
of tf2_amd.preprocess.resize_pil (and through it of tf2_preprocess_aa) where Pillow is not installed.  Run it where Pillow is; no
test imports Pillow through this file.  The inputs are not stored: each case is (seed, kind, h, w, rh, rw) and `case_image` makes its
image again from a seeded numpy generator.
  cases     int32 [n, 6]
  out       uint8, the resized images [rh, rw, 3] of the cases back to back
  pillow    the version that made them
Kinds: 0 uniform random bytes, 1 every byte 255, 2 a checkerboard of 0 and 255 pixels, 3 random 0 / 255 bytes."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "pil_resize.npz")

RANDOM, ALL_255, CHECKER, BINARY = 0, 1, 2, 3

# (kind, h, w, rh, rw); the seed is the case's index
GEOMETRIES = [
    (RANDOM, 47, 61, 31, 40), (RANDOM, 90, 70, 37, 41), (RANDOM, 50, 75, 34, 51), (RANDOM, 33, 29, 32, 17),   # 1x .. 3x, non-integer
    (RANDOM, 40, 40, 20, 20),                                                                                   # 2x
    (RANDOM, 64, 5, 2, 5), (RANDOM, 7, 96, 7, 3), (RANDOM, 64, 64, 2, 2),                                     # exactly 32x
    (RANDOM, 1, 1, 5, 7), (RANDOM, 1, 9, 4, 30), (RANDOM, 9, 1, 30, 4), (RANDOM, 6, 5, 29, 31),               # upscales
    (RANDOM, 20, 50, 45, 21), (RANDOM, 50, 20, 21, 45),                                                       # one axis up, the other down
    (RANDOM, 17, 23, 17, 23),                                                                                   # identity
    (ALL_255, 40, 52, 19, 23), (ALL_255, 5, 5, 13, 11), (ALL_255, 64, 3, 2, 3),
    (CHECKER, 48, 48, 20, 31), (CHECKER, 31, 64, 30, 2), (BINARY, 37, 45, 16, 29), (BINARY, 12, 10, 25, 33),
]


def case_image(seed: int, kind: int, h: int, w: int) -> np.ndarray:
    """the RGB uint8 image [h, w, 3] of a case"""
    rng = np.random.default_rng(int(seed))
    if kind == RANDOM:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == ALL_255:
        return np.full((h, w, 3), 255, np.uint8)
    if kind == CHECKER:
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    if kind == BINARY:
        return (rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    raise ValueError(kind)


def load(path: str = PATH):
    """[(seed, kind, h, w, rh, rw, Pillow's bytes [rh, rw, 3])] and the Pillow version"""
    z = np.load(path)
    out, at = [], 0
    for seed, kind, h, w, rh, rw in z["cases"].tolist():
        out.append((seed, kind, h, w, rh, rw, z["out"][at:at + rh * rw * 3].reshape(rh, rw, 3)))
        at += rh * rw * 3
    assert at == z["out"].size
    return out, str(z["pillow"])


def main():
    import PIL
    from PIL import Image
    cases, outs = [], []
    for seed, (kind, h, w, rh, rw) in enumerate(GEOMETRIES):
        img = case_image(seed, kind, h, w)
        res = np.asarray(Image.fromarray(img, "RGB").resize((rw, rh), Image.BILINEAR))
        assert res.shape == (rh, rw, 3) and res.dtype == np.uint8
        cases.append((seed, kind, h, w, rh, rw))
        outs.append(res.reshape(-1))
    np.savez_compressed(PATH, cases=np.asarray(cases, np.int32), out=np.concatenate(outs), pillow=np.asarray(PIL.__version__))
    print(f"{PATH}: {len(cases)} cases, {os.path.getsize(PATH)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    sys.exit(main())
