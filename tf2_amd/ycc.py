"""YCbCr frames on the device (tf2_ycc_to_rgb, include/tf2_amd.h; csrc/ycc_convert.hip): the planes a JPEG or a video decoder
leaves -- planar, NV12 / NV21 or grey, 4:4:4, 4:2:2 or 4:2:0 -- in, the interleaved uint8 pixels out that tf2_preprocess,
tf2_preprocess_aa and tf2_roi_crop read, written where their tf2_image_src records point.

`reference` is the one exact statement of the call, statuses included, and the yardstick of the device, which is bit-identical to
it.  All of it is integer arithmetic and >> is arithmetic.  Image b is h x w (srcs[b]); chroma planes are ch = ceil(h / sub_y) by
cw = ceil(w / sub_x).
  upsampled chroma at (y, x) of a plane P (`upsample`, `upsample_fancy`)
    REPLICATE      P[y // sub_y][x // sub_x]
    FANCY (1,1)    P[y][x]
    FANCY (2,1)    p = P[y], k = x >> 1;  x even: k == 0 ? p[0] : (3*p[k] + p[k-1] + 1) >> 2
                                          x odd:  k == cw-1 ? p[k] : (3*p[k] + p[k+1] + 2) >> 2
    FANCY (2,2)    r = y >> 1, k = x >> 1, o = max(r-1, 0) for even y, min(r+1, ch-1) for odd y, s[j] = 3*P[r][j] + P[o][j]
                   x even: k == 0 ? (4*s[0] + 8) >> 4 : (3*s[k] + s[k-1] + 8) >> 4
                   x odd:  k == cw-1 ? (4*s[k] + 7) >> 4 : (3*s[k] + s[k+1] + 7) >> 4
  colour (`to_rgb`), FIX(v) = int(v * 65536 + 0.5), cb = Cb - 128, cr = Cr - 128, every result clamped to 0..255
    JFIF           R = Y + ((FIX(1.40200)*cr + 32768) >> 16);  G = Y + ((-FIX(0.34414)*cb + 32768 - FIX(0.71414)*cr) >> 16)
                   B = Y + ((FIX(1.77200)*cb + 32768) >> 16)
    BT601 / BT709  yy = Y - 16; channel = (FIX(ky)*yy + FIX(a)*cb + FIX(b)*cr + 32768) >> 16 with the constants of MATRIX
FANCY + JFIF is libjpeg-turbo's decoder ("fancy" upsampling, the jdcolor tables), and with it Pillow's, byte for byte:
tests/golden/pil_ycc.npz holds Pillow's own bytes of JPEGs whose decoded planes are known exactly (tools/gen_ycc_golden.py).  What
is not claimed: that a hardware JPEG decoder's planes equal libjpeg's -- that is a question of its IDCT, upstream of this call.

`pack_ycc` builds the source buffer and both record tables from a list of frames (or refills buffers a captured graph reads);
`DeviceConverter(desc).run(...)` is the device call; `subsample_box` makes planes from an image for tests and tools."""
import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import preprocess as P

# tf2_ycc_src, byte for byte (32 bytes)
YCC_DTYPE = np.dtype([("off_y", "<i8"), ("off_cb", "<i8"), ("off_cr", "<i8"), ("pitch_y", "<i4"), ("pitch_c", "<i4")])
YCC_WORDS = YCC_DTYPE.itemsize // 4

PLANAR, SEMI_CBCR, SEMI_CRCB, GRAY = 0, 1, 2, 3                 # TF2_YCC_* layout
FANCY, REPLICATE = 0, 1                                          # upsample
JFIF, BT601, BT709 = 0, 1, 2                                     # matrix
BAD_SIZE, BAD_PITCH, BAD_OFFSET, OUT_OF_SRC, OUT_OF_DST = 1, 2, 4, 8, 16
SUBSAMPLINGS = ((1, 1), (2, 1), (2, 2))
TILE_W, TILE_H = 128, 16                                         # TF2_YCC_TILE_W / _H: the kernel's tile, in output pixels
MAX_BLOCKS_PER_IMAGE = 64
MAX_SIDE = P.MAX_SIDE


def fix(v: float) -> int:
    return int(v * 65536 + 0.5)


# matrix -> (ky, y offset, R: cr, G: cb, G: cr, B: cb) as the real numbers the fixed point is made of
MATRIX = {
    JFIF: (1.0, 0, 1.40200, -0.34414, -0.71414, 1.77200),
    BT601: (1.164383, 16, 1.596027, -0.391762, -0.812968, 2.017232),
    BT709: (1.164384, 16, 1.792741, -0.213249, -0.532909, 2.112402),
}


def default_blocks_per_image(batch: int) -> int:
    """what blocks_per_image = 0 stands for (csrc/ycc_convert.h): about 2048 blocks a launch, 1..64 an image"""
    return max(1, min(MAX_BLOCKS_PER_IMAGE, 2048 // max(int(batch), 1)))


@dataclass(frozen=True)
class Desc:
    """tf2_ycc_desc: layout, (sub_x, sub_y), upsample, matrix, the output pixel (bytes, where R, G, B go, alpha) and the grid"""
    layout: int = PLANAR
    sub: Tuple[int, int] = (2, 2)
    upsample: int = FANCY
    matrix: int = JFIF
    pixel_bytes: int = 3
    dst_channel: Tuple[int, int, int] = (0, 1, 2)
    alpha: int = 255
    blocks_per_image: int = 0

    def c(self):
        from . import _lib
        d = _lib.YccDesc()
        d.size = C.sizeof(_lib.YccDesc)
        d.layout, d.sub_x, d.sub_y, d.upsample, d.matrix = self.layout, self.sub[0], self.sub[1], self.upsample, self.matrix
        d.pixel_bytes, d.alpha, d.blocks_per_image = self.pixel_bytes, self.alpha, self.blocks_per_image
        for k in range(3):
            d.dst_channel[k] = self.dst_channel[k]
        return d

    @property
    def eff_sub(self) -> Tuple[int, int]:
        return (1, 1) if self.layout == GRAY else tuple(self.sub)


def chroma_size(h: int, w: int, sub) -> Tuple[int, int]:
    """(ch, cw) of an h x w image"""
    return -(-h // sub[1]), -(-w // sub[0])


def upsample_fancy(plane, sub, h: int, w: int) -> np.ndarray:
    """libjpeg's "fancy" upsampling of one chroma plane [ch, cw] to [h, w] (the module docstring), uint8"""
    p = np.asarray(plane).astype(np.int32)
    ch, cw = chroma_size(h, w, sub)
    assert p.shape == (ch, cw), (p.shape, (ch, cw))
    if tuple(sub) == (1, 1):
        return p.astype(np.uint8)
    xs = np.arange(w)
    k, even = xs >> 1, (xs & 1) == 0
    km, kp = np.maximum(k - 1, 0), np.minimum(k + 1, cw - 1)
    if tuple(sub) == (2, 1):
        ev = np.where(k == 0, p[:, np.zeros_like(k)], (3 * p[:, k] + p[:, km] + 1) >> 2)
        od = np.where(k == cw - 1, p[:, k], (3 * p[:, k] + p[:, kp] + 2) >> 2)
        return np.where(even, ev, od).astype(np.uint8)
    assert tuple(sub) == (2, 2), sub
    ys = np.arange(h)
    r = ys >> 1
    o = np.where((ys & 1) == 0, np.maximum(r - 1, 0), np.minimum(r + 1, ch - 1))
    s = 3 * p[r] + p[o]                                           # [h, cw]
    ev = np.where(k == 0, (4 * s[:, np.zeros_like(k)] + 8) >> 4, (3 * s[:, k] + s[:, km] + 8) >> 4)
    od = np.where(k == cw - 1, (4 * s[:, k] + 7) >> 4, (3 * s[:, k] + s[:, kp] + 7) >> 4)
    return np.where(even, ev, od).astype(np.uint8)


def upsample(plane, sub, h: int, w: int, rule: int = FANCY) -> np.ndarray:
    """one chroma plane [ch, cw] at every pixel of the h x w image, by either rule"""
    if rule == FANCY:
        return upsample_fancy(plane, sub, h, w)
    p = np.asarray(plane, np.uint8)
    assert p.shape == chroma_size(h, w, sub)
    return p[np.arange(h) // sub[1]][:, np.arange(w) // sub[0]]


def to_rgb(y, cb, cr, matrix: int = JFIF) -> np.ndarray:
    """uint8 [..., 3] (R, G, B) of Y, Cb, Cr arrays of one shape, in the fixed point of the module docstring"""
    y, cb, cr = (np.asarray(v).astype(np.int64) for v in (y, cb, cr))
    cb, cr = cb - 128, cr - 128
    ky, yoff, r_cr, g_cb, g_cr, b_cb = MATRIX[matrix]
    if matrix == JFIF:
        r = y + ((fix(r_cr) * cr + 32768) >> 16)
        g = y + ((-fix(-g_cb) * cb + 32768 - fix(-g_cr) * cr) >> 16)
        b = y + ((fix(b_cb) * cb + 32768) >> 16)
    else:
        yy = fix(ky) * (y - yoff)
        r = (yy + fix(r_cr) * cr + 32768) >> 16
        g = (yy - fix(-g_cb) * cb - fix(-g_cr) * cr + 32768) >> 16
        b = (yy + fix(b_cb) * cb + 32768) >> 16
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def record_status(ycc, srcs, desc: Desc, src_bytes: int, pixels_bytes: int) -> np.ndarray:
    """The device's validity rule per image (TF2_YCC_* bits; 0: converted) -- a statement in Python integers, no overflow"""
    ycc = np.asarray(ycc, YCC_DTYPE).reshape(-1)
    srcs = np.asarray(srcs, P.SRC_DTYPE).reshape(-1)
    assert len(ycc) == len(srcs)
    chroma, planar = desc.layout != GRAY, desc.layout == PLANAR
    sx, sy = desc.eff_sub
    pb = desc.pixel_bytes
    out = np.zeros(len(srcs), np.int32)
    for i, (r, p) in enumerate(zip(srcs, ycc)):
        h, w, pitch, off = int(r["h"]), int(r["w"]), int(r["row_pitch"]), int(r["offset"])
        oy, ocb, ocr, py, pc = int(p["off_y"]), int(p["off_cb"]), int(p["off_cr"]), int(p["pitch_y"]), int(p["pitch_c"])
        cw, ch = (w + sx - 1) >> (sx - 1), (h + sy - 1) >> (sy - 1)
        crow = cw if planar else 2 * cw
        st = 0
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            st |= BAD_SIZE
        if pitch < w * pb or py < w or (chroma and pc < crow):
            st |= BAD_PITCH
        if off < 0 or oy < 0 or (chroma and ocb < 0) or (planar and ocr < 0):
            st |= BAD_OFFSET
        if st == 0:
            if (oy + (h - 1) * py + w > src_bytes or (chroma and ocb + (ch - 1) * pc + crow > src_bytes) or
                    (planar and ocr + (ch - 1) * pc + crow > src_bytes)):
                st |= OUT_OF_SRC
            if off + (h - 1) * pitch + w * pb > pixels_bytes:
                st |= OUT_OF_DST
        out[i] = st
    return out


def _plane(src, off: int, pitch: int, rows: int, cols: int, step: int = 1, first: int = 0) -> np.ndarray:
    return np.stack([src[off + y * pitch + first: off + y * pitch + first + cols * step: step] for y in range(rows)])


def planes_of(src, p, h: int, w: int, desc: Desc):
    """(Y [h, w], Cb, Cr [ch, cw]) of a valid record; GRAY: planes of 128"""
    src = np.asarray(src, np.uint8).reshape(-1)
    y = _plane(src, int(p["off_y"]), int(p["pitch_y"]), h, w)
    ch, cw = chroma_size(h, w, desc.eff_sub)
    if desc.layout == GRAY:
        return y, np.full((ch, cw), 128, np.uint8), np.full((ch, cw), 128, np.uint8)
    if desc.layout == PLANAR:
        return y, _plane(src, int(p["off_cb"]), int(p["pitch_c"]), ch, cw), _plane(src, int(p["off_cr"]), int(p["pitch_c"]), ch, cw)
    a = _plane(src, int(p["off_cb"]), int(p["pitch_c"]), ch, cw, 2, 0)
    b = _plane(src, int(p["off_cb"]), int(p["pitch_c"]), ch, cw, 2, 1)
    return (y, a, b) if desc.layout == SEMI_CBCR else (y, b, a)


def convert_image(y, cb, cr, desc: Desc) -> np.ndarray:
    """uint8 [h, w, pixel_bytes]: the output pixels of one image's planes"""
    h, w = y.shape
    sub = desc.eff_sub
    rgb = to_rgb(y, upsample(cb, sub, h, w, desc.upsample), upsample(cr, sub, h, w, desc.upsample), desc.matrix)
    px = np.full((h, w, desc.pixel_bytes), desc.alpha, np.uint8)
    for k in range(3):
        px[:, :, desc.dst_channel[k]] = rgb[:, :, k]
    return px


def reference(src, ycc, srcs, desc: Desc, pixels):
    """The statement of the whole call on the device's own inputs: src (uint8, 1-D), ycc (YCC_DTYPE records), srcs (SRC_DTYPE
    records), and the pixel buffer as it is before the call (uint8 1-D, or its size for a buffer of zeros) -> (pixels after the
    call, status int32 [B]).  Only the first w * pixel_bytes bytes of the rows of images with status 0 change."""
    src = np.asarray(src, np.uint8).reshape(-1)
    ycc = np.asarray(ycc, YCC_DTYPE).reshape(-1)
    srcs = np.asarray(srcs, P.SRC_DTYPE).reshape(-1)
    out = np.zeros(int(pixels), np.uint8) if np.isscalar(pixels) else np.array(pixels, np.uint8).reshape(-1)
    status = record_status(ycc, srcs, desc, src.size, out.size)
    pb = desc.pixel_bytes
    for b, (r, p) in enumerate(zip(srcs, ycc)):
        if status[b]:
            continue
        h, w, pitch, off = int(r["h"]), int(r["w"]), int(r["row_pitch"]), int(r["offset"])
        px = convert_image(*planes_of(src, p, h, w, desc), desc).reshape(h, w * pb)
        for y in range(h):
            out[off + y * pitch: off + y * pitch + w * pb] = px[y]
    return out, status


def subsample_box(img, sub):
    """Planes of an [h, w, 3] uint8 image whose channels are taken as Y, Cb, Cr (or anything): channel 0 whole, channels 1 and 2
    averaged over sub_x x sub_y boxes (the edge repeated, rounded half up).  For tests and tools; a decoder has its own planes."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    sx, sy = sub
    ch, cw = chroma_size(h, w, sub)
    pad = np.pad(img[:, :, 1:].astype(np.int32), ((0, ch * sy - h), (0, cw * sx - w), (0, 0)), mode="edge")
    box = pad.reshape(ch, sy, cw, sx, 2).sum(axis=(1, 3))
    c = ((box + (sx * sy) // 2) // (sx * sy)).astype(np.uint8)
    return np.ascontiguousarray(img[:, :, 0]), np.ascontiguousarray(c[:, :, 0]), np.ascontiguousarray(c[:, :, 1])


def _up(n: int, align: int) -> int:
    return -(-n // align) * align


def pack_ycc_host(frames, layout: int, sub, pixel_bytes: int = 3, preset: Optional[P.Preset] = None, align: int = 4):
    """(src uint8 [n], ycc YCC_DTYPE [B], srcs SRC_DTYPE [B], pixels_bytes) of a list of frames: (Y, Cb, Cr) arrays -- for the
    semi-planar layouts also (Y, CbCr) with CbCr [ch, cw, 2] in the layout's byte order, for GRAY (Y,) or Y alone.  Planes lie back
    to back, every plane and every row starting at a multiple of `align` bytes; the destination images likewise.  The srcs records
    carry preset.geometry (none: no resize, no crop), ready for tf2_preprocess / tf2_preprocess_aa."""
    sub = (1, 1) if layout == GRAY else tuple(sub)
    B = len(frames)
    assert B, "no frames"
    ycc, srcs = np.zeros(B, YCC_DTYPE), np.zeros(B, P.SRC_DTYPE)
    chunks, at, dat = [], 0, 0

    def put(plane):
        nonlocal at
        rows, cols = plane.shape
        pitch = _up(cols, align)
        buf = np.zeros((rows, pitch), np.uint8)
        buf[:, :cols] = plane
        off = at
        chunks.append(buf.reshape(-1))
        at += buf.size
        return off, pitch

    for i, f in enumerate(frames):
        f = (f,) if isinstance(f, np.ndarray) else tuple(f)
        y = np.asarray(f[0], np.uint8)
        h, w = y.shape
        ch, cw = chroma_size(h, w, sub)
        oy, py = put(y)
        ocb = ocr = pc = 0
        if layout == PLANAR:
            assert len(f) == 3 and f[1].shape == (ch, cw) and f[2].shape == (ch, cw), f"frame {i}: chroma planes must be {(ch, cw)}"
            ocb, pc = put(np.asarray(f[1], np.uint8))
            ocr, _ = put(np.asarray(f[2], np.uint8))
        elif layout in (SEMI_CBCR, SEMI_CRCB):
            if len(f) == 3:
                pair = (f[1], f[2]) if layout == SEMI_CBCR else (f[2], f[1])
                inter = np.stack([np.asarray(v, np.uint8) for v in pair], axis=-1)
            else:
                inter = np.asarray(f[1], np.uint8)
            assert inter.shape == (ch, cw, 2), f"frame {i}: interleaved chroma must be {(ch, cw, 2)}"
            ocb, pc = put(inter.reshape(ch, 2 * cw))
        pitch = _up(w * pixel_bytes, align)
        rh, rw, cy, cx = preset.geometry(h, w) if preset is not None else (h, w, 0, 0)
        ycc[i] = (oy, ocb, ocr, py, pc)
        srcs[i] = (dat, h, w, pitch, rh, rw, cy, cx, 0)
        dat += h * pitch
    return np.concatenate(chunks), ycc, srcs, dat


def records_to_words(recs, words: int):
    recs = np.ascontiguousarray(recs)
    return recs.view(np.int32).reshape(len(recs), words).copy()


def pack_ycc(frames, layout: int, sub, device, pixel_bytes: int = 3, preset: Optional[P.Preset] = None, align: int = 4,
             src=None, ycc=None, srcs=None, pixels=None):
    """The device inputs of tf2_ycc_to_rgb from a list of frames (`pack_ycc_host`): (src uint8 tensor, ycc int32 [B, 8], srcs int32
    [B, 10], pixels uint8 tensor) -- srcs and pixels are what Preprocessor / DeviceCropper read once the conversion has run.  With
    src= / ycc= / srcs= / pixels= the caller's tensors are filled instead (a captured graph reads the same buffers at every replay):
    the planes go to the front of `src`, the records fill `ycc` and `srcs`, and `pixels` only has to be large enough."""
    import torch
    host, yrec, srec, need = pack_ycc_host(frames, layout, sub, pixel_bytes, preset, align)
    yw, sw = torch.from_numpy(records_to_words(yrec, YCC_WORDS)), torch.from_numpy(records_to_words(srec, P.SRC_WORDS))
    if src is None:
        src = torch.from_numpy(host).to(device)
    else:
        assert src.dtype == torch.uint8 and src.numel() >= host.size, "source buffer too small"
        src.view(-1)[:host.size].copy_(torch.from_numpy(host))
    if ycc is None:
        ycc = yw.to(device)
    else:
        assert ycc.dtype == torch.int32 and tuple(ycc.shape) == tuple(yw.shape), "ycc must be int32 [B, 8] of this batch"
        ycc.copy_(yw)
    if srcs is None:
        srcs = sw.to(device)
    else:
        assert srcs.dtype == torch.int32 and tuple(srcs.shape) == tuple(sw.shape), "srcs must be int32 [B, 10] of this batch"
        srcs.copy_(sw)
    if pixels is None:
        pixels = torch.zeros(need, dtype=torch.uint8, device=device)
    else:
        assert pixels.dtype == torch.uint8 and pixels.numel() >= need, "pixel buffer too small"
    return src, ycc, srcs, pixels


class DeviceConverter:
    """tf2_ycc_to_rgb with `desc` (a Desc).
      run(src, ycc, pixels, srcs, stream=None, status=None) -> status
    src: uint8 device tensor holding the planes, ycc: int32 [B, 8] (tf2_ycc_src records), pixels: the uint8 device tensor the pixels
    are written into, srcs: int32 [B, 10] (tf2_image_src records) -- `pack_ycc` makes all four.  status: int32 [B], 0 or the
    TF2_YCC_* bits of an image that was left alone.  Enqueued on `stream` (default: the current one); nothing synchronises or
    allocates beyond the status, which may be passed in."""

    def __init__(self, desc: Desc = Desc()):
        self.desc = desc
        self._c = desc.c()

    def run(self, src, ycc, pixels, srcs, stream=None, status=None):
        import torch
        from . import _lib
        dev = _lib.expect(src, torch.uint8)
        _lib.expect(pixels, torch.uint8, device=dev)
        _lib.expect(srcs, torch.int32, device=dev, cols=P.SRC_WORDS)
        B = srcs.shape[0]
        _lib.expect(ycc, torch.int32, (B, YCC_WORDS), dev)
        stream = stream or torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            if status is None:
                status = torch.empty(B, dtype=torch.int32, device=dev)
            _lib.expect(status, torch.int32, (B,), dev)
            _lib.check(_lib.lib().tf2_ycc_to_rgb(C.byref(self._c), src.data_ptr(), src.numel(), ycc.data_ptr(), pixels.data_ptr(),
                                                 pixels.numel(), srcs.data_ptr(), B, status.data_ptr(), stream.cuda_stream))
        return status

    def reference(self, src, ycc, srcs, pixels):
        """`reference` on host copies of the tensors (pixels: the buffer as it is before the call)"""
        host = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
        yr = np.ascontiguousarray(host(ycc), np.int32).view(YCC_DTYPE).reshape(-1)
        sr = np.ascontiguousarray(host(srcs), np.int32).view(P.SRC_DTYPE).reshape(-1)
        return reference(host(src), yr, sr, self.desc, host(pixels))
