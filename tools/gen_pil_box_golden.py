#!/usr/bin/env python3
"""Writes tests/golden/pil_resize_box.npz: the bytes of Pillow's Image.resize((ow, oh), BILINEAR, box=(x0, y0, x1, y1)) on small
uint8 images, RGB and L, the yardstick of tf2_amd.roi.crop_pil (and through it of tf2_roi_crop_aa) where Pillow is not installed.
Run it where Pillow is; no test imports Pillow through this file.
  cases     int32 [n, 6]: channels (3: RGB, 1: L), h, w, oh, ow, family
  boxes     float32 [n, 4]: x0, y0, x1, y1 as Pillow received them
  src       uint8, the source images [h, w, channels] of the cases back to back
  out       uint8, Pillow's results [oh, ow, channels] back to back
  pillow    the version that made them
Families: 0 the whole image, 1 integer corners, 2 a box touching image edges, 3 fractional float32 corners, 4 a side below one pixel.
The sources are thin where they are long, so that a few hundred taps fit a small file."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "pil_resize_box.npz")

WHOLE, INTEGER, EDGE, FRACTIONAL, THIN = 0, 1, 2, 3, 4

# (channels, h, w, oh, ow, family, box or None: drawn from the case's seeded generator)
GEOMETRIES = [
    (3, 1, 1, 1, 1, WHOLE, None), (3, 1, 1, 5, 7, WHOLE, None), (1, 9, 7, 4, 3, WHOLE, None), (3, 12, 10, 12, 10, WHOLE, None),
    (3, 2, 386, 2, 1, WHOLE, None),                                          # scale 386 along x: 386 taps
    (1, 300, 2, 1, 2, WHOLE, None),                                          # 300 taps along y
    (3, 20, 30, 7, 9, INTEGER, (4, 3, 25, 17)), (1, 20, 30, 14, 21, INTEGER, (4, 3, 25, 17)),      # downscale; scale exactly 1
    (1, 16, 16, 33, 40, INTEGER, (5, 6, 9, 10)),                             # upscale to the largest output
    (3, 20, 20, 3, 3, INTEGER, (4, 4, 16, 16)), (1, 2, 200, 1, 3, INTEGER, (10, 0, 190, 2)),
    (3, 21, 13, 6, 5, INTEGER, None), (1, 25, 40, 9, 13, INTEGER, None),
    (3, 18, 22, 6, 8, EDGE, (0.0, 2.5, 10.25, 18.0)), (1, 18, 22, 6, 8, EDGE, (7.75, 0.0, 22.0, 9.5)),
    (1, 30, 9, 11, 4, EDGE, (0.0, 0.0, 4.5, 30.0)), (3, 9, 30, 4, 11, EDGE, (12.125, 1.5, 30.0, 9.0)),
    (3, 1, 50, 3, 6, EDGE, (3.3, 0.0, 50.0, 1.0)), (1, 50, 1, 6, 3, EDGE, (0.0, 7.7, 1.0, 44.1)),
    (1, 2, 150, 2, 2, EDGE, (0.0, 0.0, 140.6, 2.0)),
    (3, 22, 22, 8, 8, FRACTIONAL, (3.3, 4.7, 20.1, 19.9)), (3, 16, 16, 20, 17, FRACTIONAL, (10.01, 9.99, 14.5, 13.25)),
    (1, 23, 37, 10, 12, FRACTIONAL, None), (1, 37, 23, 3, 5, FRACTIONAL, None), (3, 15, 15, 15, 15, FRACTIONAL, (0.5, 0.5, 14.5, 14.5)),
    (1, 3, 320, 2, 3, FRACTIONAL, (0.1, 0.3, 300.7, 2.9)), (1, 260, 3, 2, 2, FRACTIONAL, (0.2, 1.1, 2.8, 255.3)),
    (3, 19, 19, 9, 31, FRACTIONAL, None), (3, 64, 5, 2, 5, FRACTIONAL, (0.25, 0.0, 4.75, 64.0)),
    (3, 10, 10, 3, 4, THIN, (4.2, 2.0, 4.57, 8.0)), (3, 10, 10, 4, 3, THIN, (1.0, 6.1, 9.0, 6.35)),
    (1, 12, 9, 5, 5, THIN, (3.4, 3.4, 3.9, 3.9)), (3, 1, 1, 2, 3, THIN, (0.25, 0.25, 0.75, 0.5)),
    (3, 8, 40, 1, 6, THIN, (0.0, 7.5, 40.0, 8.0)), (1, 6, 6, 7, 1, THIN, (5.99, 0.0, 6.0, 6.0)),
]


def draw_box(rng, family: int, h: int, w: int):
    """a box of the family inside a w x h image, as float32 (x0, y0, x1, y1)"""
    if family == WHOLE:
        return 0.0, 0.0, float(w), float(h)
    if family == INTEGER:
        x0, y0 = int(rng.integers(0, w - 1)), int(rng.integers(0, h - 1))
        return float(x0), float(y0), float(rng.integers(x0 + 1, w + 1)), float(rng.integers(y0 + 1, h + 1))
    x0, y0 = rng.uniform(0, w - 1.5), rng.uniform(0, h - 1.5)
    x1, y1 = rng.uniform(x0 + 1, w), rng.uniform(y0 + 1, h)
    return tuple(float(np.float32(v)) for v in (x0, y0, x1, y1))


def load(path: str = PATH):
    """[(family, source [h, w, c], box float32 [4], oh, ow, Pillow's bytes [oh, ow, c])] and the Pillow version"""
    z = np.load(path)
    out, s_at, o_at = [], 0, 0
    for (c, h, w, oh, ow, family), box in zip(z["cases"].tolist(), z["boxes"]):
        src = z["src"][s_at:s_at + h * w * c].reshape(h, w, c)
        res = z["out"][o_at:o_at + oh * ow * c].reshape(oh, ow, c)
        s_at, o_at = s_at + h * w * c, o_at + oh * ow * c
        out.append((family, src, box.astype(np.float32), oh, ow, res))
    assert s_at == z["src"].size and o_at == z["out"].size
    return out, str(z["pillow"])


def pillow_resize_box(img, box, oh: int, ow: int) -> np.ndarray:
    """Pillow's own result for an [h, w, c] uint8 image (c 1: mode L, 3: RGB): uint8 [oh, ow, c]"""
    from PIL import Image
    c = img.shape[2]
    im = Image.fromarray(img[:, :, 0], "L") if c == 1 else Image.fromarray(img, "RGB")
    res = np.asarray(im.resize((ow, oh), Image.BILINEAR, box=tuple(float(v) for v in box)))
    return res.reshape(oh, ow, c)


def main():
    import PIL
    cases, boxes, srcs, outs = [], [], [], []
    for seed, (c, h, w, oh, ow, family, box) in enumerate(GEOMETRIES):
        rng = np.random.default_rng(1000 + seed)
        img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        if seed % 5 == 4:
            img = (rng.integers(0, 2, (h, w, c), dtype=np.uint8) * 255).astype(np.uint8)      # 0 / 255 bytes: the clip is reached
        box = np.asarray(box if box is not None else draw_box(rng, family, h, w), np.float32)
        res = pillow_resize_box(img, box, oh, ow)
        assert res.dtype == np.uint8
        cases.append((c, h, w, oh, ow, family))
        boxes.append(box)
        srcs.append(img.reshape(-1))
        outs.append(res.reshape(-1))
    np.savez_compressed(PATH, cases=np.asarray(cases, np.int32), boxes=np.asarray(boxes, np.float32), src=np.concatenate(srcs),
                        out=np.concatenate(outs), pillow=np.asarray(PIL.__version__))
    print(f"{PATH}: {len(cases)} cases, {os.path.getsize(PATH)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    sys.exit(main())
