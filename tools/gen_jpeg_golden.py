#!/usr/bin/env python3
"""Writes tests/golden/pil_jpeg.npz: JPEG files and what Pillow's decoder (libjpeg-turbo) makes of them, the yardstick of
tf2_amd.jpeg (tf2_jpeg_parse / tf2_jpeg_entropy / tf2_jpeg_idct and the statements beside them) where Pillow is not installed.  Run it
where Pillow is and the library is built; no test imports Pillow through this file.

The files are Pillow's own encodings of seeded synthetic images -- noise, smooth gradients with noise, 0 / 255 checkers and sharp
edges, so that high AC terms and both clamps of the inverse DCT occur -- as mode L and as colour with subsampling 0, 1, 2 (4:4:4,
4:2:2, 4:2:0), at every size of SIZES, with quality 30 / 75 / 95 / 100, optimize (the file's own Huffman tables) and restart markers
every 1 or 3 MCUs spread over them; plus one progressive and one CMYK file, which the parser refuses.
  cases     int32 [n, 8]: seed, kind, mode (-1: L, 0..2: Pillow's subsampling, 3: progressive 4:2:0, 4: CMYK), h, w, quality,
            optimize, restart_marker_blocks
  files     uint8, the files back to back;  offsets int64 [n + 1]
  rgb       uint8, Pillow's convert('RGB') images [h, w, 3] back to back
  ycc       uint8, Pillow's draft('YCbCr', size) images [h, w, 3] back to back: the decoder's Y, and its upsampled Cb, Cr (mode L
            files stay mode L under draft: Y in channel 0, 128 in the others; CMYK: zeros)
  pillow    the version that made them
While it records, the tool asserts that the parser accepts every case it is specified to accept and refuses the two others with
their bit, and that the whole host statement (entropy, reference_idct, the file's upsampling rule, JFIF) gives Pillow's RGB."""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "pil_jpeg.npz")

NOISE, GRADIENT, CHECKER, EDGES = 0, 1, 2, 3
MODE_L, MODE_PROGRESSIVE, MODE_CMYK = -1, 3, 4
SUBS = ((1, 1), (2, 1), (2, 2))                     # (sub_x, sub_y) of Pillow's subsampling 0, 1, 2
SIZES = [(1, 1), (8, 8), (2, 9), (9, 2), (9, 3), (9, 4), (9, 5), (15, 15), (16, 16), (17, 17), (17, 33), (37, 53), (48, 64), (50, 75)]
QUALITIES = (30, 75, 95, 100)
RESTARTS = (0, 0, 1, 0, 3)


def geometries():
    """(kind, mode, h, w, quality, optimize, restart) of every case; the seed is the index"""
    out = []
    for mi, mode in enumerate((MODE_L, 0, 1, 2)):
        for si, (h, w) in enumerate(SIZES):
            i = mi * len(SIZES) + si
            out.append(((i + mi) % 4, mode, h, w, QUALITIES[(si + mi) % 4], int(i % 3 == 0), RESTARTS[(si + 2 * mi) % 5]))
    out.append((GRADIENT, MODE_PROGRESSIVE, 37, 53, 75, 0, 0))
    out.append((NOISE, MODE_CMYK, 17, 17, 75, 0, 0))
    return out


def case_image(seed: int, kind: int, mode: int, h: int, w: int) -> np.ndarray:
    """the image a case encodes: uint8 [h, w] (L), [h, w, 4] (CMYK) or [h, w, 3] (RGB)"""
    rng = np.random.default_rng(1000 + int(seed))
    ch = 1 if mode == MODE_L else (4 if mode == MODE_CMYK else 3)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == NOISE:
        img = rng.integers(0, 256, (h, w, ch))
    elif kind == GRADIENT:
        slope = rng.uniform(-4, 4, (2, ch))
        img = 128 + yy[:, :, None] * slope[0] + xx[:, :, None] * slope[1] + rng.normal(0, 6, (h, w, ch))
    elif kind == CHECKER:
        step = rng.integers(1, 4, ch)
        img = np.stack([((yy // step[c] + xx // step[c]) & 1) * 255 for c in range(ch)], axis=-1)
    else:
        img = np.zeros((h, w, ch))
        for c in range(ch):
            cut = rng.integers(0, max(h, w), 3)
            img[:, :, c] = np.where(xx > cut[0], 255, 0) ^ np.where(yy > cut[1], 255, 0) ^ np.where(xx + yy > cut[2], 255, 0)
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return img[:, :, 0] if ch == 1 else img


def load(path: str = PATH):
    """[dict(seed, kind, mode, sub, h, w, quality, optimize, restart, file (bytes), rgb [h, w, 3], ycc [h, w, 3])] and the Pillow
    version; sub is None for mode L and CMYK"""
    z = np.load(path)
    out, at = [], 0
    for i, (seed, kind, mode, h, w, quality, optimize, restart) in enumerate(z["cases"].tolist()):
        n = h * w * 3
        sub = SUBS[2] if mode == MODE_PROGRESSIVE else (SUBS[mode] if 0 <= mode <= 2 else None)
        out.append(dict(seed=seed, kind=kind, mode=mode, sub=sub, h=h, w=w, quality=quality, optimize=optimize, restart=restart,
                        file=z["files"][z["offsets"][i]:z["offsets"][i + 1]].tobytes(),
                        rgb=z["rgb"][at:at + n].reshape(h, w, 3), ycc=z["ycc"][at:at + n].reshape(h, w, 3)))
        at += n
    assert at == z["rgb"].size == z["ycc"].size and z["offsets"][-1] == z["files"].size
    return out, str(z["pillow"])


def supported(case) -> bool:
    return case["mode"] in (MODE_L, 0, 1, 2)


def main():
    import PIL
    from PIL import Image
    sys.path.insert(0, ROOT)
    from tf2_amd import jpeg as J
    cases, files, rgbs, yccs = [], [], [], []
    for seed, (kind, mode, h, w, quality, optimize, restart) in enumerate(geometries()):
        img = case_image(seed, kind, mode, h, w)
        f = io.BytesIO()
        kw = dict(quality=quality, optimize=bool(optimize))
        if restart:
            kw["restart_marker_blocks"] = restart
        if mode == MODE_L:
            Image.fromarray(img, "L").save(f, "JPEG", **kw)
        elif mode == MODE_CMYK:
            Image.fromarray(img, "CMYK").save(f, "JPEG", **kw)
        elif mode == MODE_PROGRESSIVE:
            Image.fromarray(img, "RGB").save(f, "JPEG", subsampling=2, progressive=True, **kw)
        else:
            Image.fromarray(img, "RGB").save(f, "JPEG", subsampling=mode, **kw)
        data = f.getvalue()
        rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        im = Image.open(io.BytesIO(data))
        im.draft("YCbCr", im.size)
        if mode == MODE_L:
            assert im.mode == "L", im.mode
            ycc = np.stack([np.asarray(im), np.full((h, w), 128, np.uint8), np.full((h, w), 128, np.uint8)], axis=-1)
        elif mode == MODE_CMYK:
            ycc = np.zeros((h, w, 3), np.uint8)
        else:
            assert im.mode == "YCbCr", im.mode
            ycc = np.asarray(im)
        assert rgb.shape == ycc.shape == (h, w, 3) and rgb.dtype == ycc.dtype == np.uint8
        info = J.parse(data)
        if mode == MODE_PROGRESSIVE:
            assert info.status & J.UNSUPPORTED_PROGRESSIVE and not info.status & ~J.UNSUPPORTED, info.status
        elif mode == MODE_CMYK:
            assert info.status & J.UNSUPPORTED_COMPONENTS and not info.status & ~J.UNSUPPORTED, info.status
        else:
            assert info.status == 0 and (info.h, info.w) == (h, w), (seed, info.status)
            assert info.components == (1 if mode == MODE_L else 3) and (mode == MODE_L or info.sub == SUBS[mode])
            assert info.restart_interval == restart, (seed, info.restart_interval, restart)
            coef, st = J.entropy(data, info)
            assert st == 0, (seed, st)
            assert np.array_equal(J.rgb_of_file(info, coef), rgb), f"case {seed}: the host statement is not Pillow's RGB"
        cases.append((seed, kind, mode, h, w, quality, optimize, restart))
        files.append(np.frombuffer(data, np.uint8))
        rgbs.append(rgb.reshape(-1))
        yccs.append(ycc.reshape(-1))
    offsets = np.concatenate([[0], np.cumsum([f.size for f in files])]).astype(np.int64)
    np.savez_compressed(PATH, cases=np.asarray(cases, np.int32), files=np.concatenate(files), offsets=offsets, rgb=np.concatenate(rgbs),
                        ycc=np.concatenate(yccs), pillow=np.asarray(PIL.__version__))
    print(f"{PATH}: {len(cases)} cases, {os.path.getsize(PATH)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    sys.exit(main())
