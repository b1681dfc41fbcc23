#!/usr/bin/env python3
"""Writes tests/golden/pil_ycc.npz: what Pillow's JPEG decoder (libjpeg-turbo: "fancy" upsampling, the jdcolor tables) makes of
planes that are known exactly, the yardstick of tf2_amd.ycc.upsample_fancy / to_rgb (and through them of tf2_ycc_to_rgb) where Pillow
is not installed.  Run it where Pillow is; no test imports Pillow through this file.

How the decoder's subsampled planes come to be known: a mode-YCbCr image is built with Y constant per 8 x 8 block and Cb, Cr constant
per (8 * sub_y) x (8 * sub_x) block, and saved with quality=100 (every quantiser 1) and the subsampling.  The encoder's box filter
leaves the chroma constants as they are, every block is DC-only, and a DC-only block survives the integer IDCT exactly: the decoded
planes are the block constants.  The tool asserts that for Y (and, for 4:4:4, for the chroma) while it records.
  cases     int32 [n, 5]: seed, kind, sub index (0: 4:4:4, 1: 4:2:2, 2: 4:2:0 -- Pillow's `subsampling`), h, w
  rgb       uint8, Pillow's RGB images [h, w, 3] of the cases back to back
  ycc       uint8, Pillow's upsampled YCbCr (draft('YCbCr', size)) [h, w, 3], back to back
  pillow    the version that made them
The planes are not stored: `case_planes` makes them again from the seed.  Kinds: 0 block values uniform in 0..255, 1 only 0 or 255."""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "pil_ycc.npz")

RANDOM, BINARY = 0, 1
SUBS = ((1, 1), (2, 1), (2, 2))                     # (sub_x, sub_y) of Pillow's subsampling 0, 1, 2
SIZES = [(48, 64), (37, 53), (16, 16), (17, 33), (8, 8), (1, 1), (9, 2), (2, 9), (33, 17), (50, 75)]     # (h, w)


def geometries():
    return [(kind, si, h, w) for kind in (RANDOM, BINARY) for si in range(3) for h, w in SIZES]


def _blocks(rng, kind: int, rows: int, cols: int) -> np.ndarray:
    v = rng.integers(0, 256, (rows, cols)) if kind == RANDOM else rng.integers(0, 2, (rows, cols)) * 255
    return v.astype(np.uint8)


def case_planes(seed: int, kind: int, si: int, h: int, w: int):
    """(Y [h, w], Cb [ch, cw], Cr [ch, cw]) of a case: the planes the decoder reconstructs"""
    rng = np.random.default_rng(int(seed))
    sx, sy = SUBS[si]
    ch, cw = -(-h // sy), -(-w // sx)
    y = np.kron(_blocks(rng, kind, -(-h // 8), -(-w // 8)), np.ones((8, 8), np.uint8))[:h, :w]
    cb = np.kron(_blocks(rng, kind, -(-ch // 8), -(-cw // 8)), np.ones((8, 8), np.uint8))[:ch, :cw]
    cr = np.kron(_blocks(rng, kind, -(-ch // 8), -(-cw // 8)), np.ones((8, 8), np.uint8))[:ch, :cw]
    return np.ascontiguousarray(y), np.ascontiguousarray(cb), np.ascontiguousarray(cr)


def load(path: str = PATH):
    """[(seed, kind, sub, h, w, Pillow's RGB [h, w, 3], Pillow's YCbCr [h, w, 3])] and the Pillow version"""
    z = np.load(path)
    out, at = [], 0
    for seed, kind, si, h, w in z["cases"].tolist():
        n = h * w * 3
        out.append((seed, kind, SUBS[si], h, w, z["rgb"][at:at + n].reshape(h, w, 3), z["ycc"][at:at + n].reshape(h, w, 3)))
        at += n
    assert at == z["rgb"].size == z["ycc"].size
    return out, str(z["pillow"])


def main():
    import PIL
    from PIL import Image
    cases, rgbs, yccs = [], [], []
    for seed, (kind, si, h, w) in enumerate(geometries()):
        y, cb, cr = case_planes(seed, kind, si, h, w)
        sx, sy = SUBS[si]
        full = np.stack([y, np.repeat(np.repeat(cb, sy, 0), sx, 1)[:h, :w], np.repeat(np.repeat(cr, sy, 0), sx, 1)[:h, :w]], axis=-1)
        f = io.BytesIO()
        Image.fromarray(full, "YCbCr").save(f, "JPEG", quality=100, subsampling=si)
        im = Image.open(io.BytesIO(f.getvalue()))
        rgb = np.asarray(im.convert("RGB"))
        im = Image.open(io.BytesIO(f.getvalue()))
        im.draft("YCbCr", im.size)
        assert im.mode == "YCbCr", im.mode
        ycc = np.asarray(im)
        assert rgb.shape == ycc.shape == (h, w, 3) and rgb.dtype == ycc.dtype == np.uint8
        assert np.array_equal(ycc[:, :, 0], y), f"case {seed}: the decoded Y is not the constructed Y"
        if si == 0:
            assert np.array_equal(ycc[:, :, 1], cb) and np.array_equal(ycc[:, :, 2], cr), f"case {seed}: decoded chroma"
        cases.append((seed, kind, si, h, w))
        rgbs.append(rgb.reshape(-1))
        yccs.append(ycc.reshape(-1))
    np.savez_compressed(PATH, cases=np.asarray(cases, np.int32), rgb=np.concatenate(rgbs), ycc=np.concatenate(yccs),
                        pillow=np.asarray(PIL.__version__))
    print(f"{PATH}: {len(cases)} cases, {os.path.getsize(PATH)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    sys.exit(main())
