"""Image preprocessing on the device (tf2_preprocess, include/tf2_amd.h; csrc/preprocess.hip): raw uint8 HWC pixels in, the
net's input out -- float32 [B, 3, image_h, image_w] as tf2_net_run reads it, or int8 quantised with 2^-Q0 as tf2_net_run_q /
images_are_q = 1 reads it.

`reference` is the one exact statement of the arithmetic and the yardstick of the device, which is bit-identical to it.  For
net channel c, output row y and column x of image b with source size (H, W), resized size (RH, RW) and crop (cy, cx):
  coordinates (float64)   fy = (y + cy + 0.5) * (H / RH) - 0.5; y0 = floor(fy), wy = float32(fy - y0); y0 < 0: y0 = 0, wy = 0;
                          y0 >= H - 1: y0 = H - 1, wy = 0; y1 = min(y0 + 1, H - 1); the same for columns.  The geometry of cv2
                          INTER_LINEAR and torch interpolate(bilinear, align_corners=False): half-pixel centres, edge clamp, no
                          antialiasing.
  interpolation (float32, in this order, no contraction)
                          top = p00*(1-wx) + p01*wx, bot = p10*(1-wx) + p11*wx, r = top*(1-wy) + bot*wy, p the uint8 samples of
                          source byte src_channel[c]; (RH, RW) == (H, W) makes every weight 0 and r == p exactly.
  optional rounding       r = clamp(rint(r), 0, 255) (half to even)
  mean and scale          v = (r - mean[c]) * scale[c]
  output                  v as float32, or int8 quant_input(v, 2^-Q0) (runner.cpp:158-164, csrc/input_quant.h).

Presets restate the per-network preprocessing of TransForm_Kit/Quantization/data_loader.py (see each one).  What they cannot
match: cv2.resize on uint8 images (GOOGLENET's reference) is a fixed-point resize (11-bit weights) whose bytes may differ from
this float resize + rint by one in places -- nobody has compared them; torchvision's Resize on PIL
images (TORCHVISION) antialiases when it downscales, which this resize does not -- TORCHVISION_PIL below does, bit for bit.
cv2.resize on float images (RESNET50, SSD300) has the same geometry, but its float32 rounding has not been compared either.

Antialiased resize (tf2_preprocess_aa; csrc/preprocess_aa.hip, csrc/resample_aa.h): presets with antialias=True resize as Pillow's
Image.resize(size, BILINEAR) does on an RGB uint8 image (ImagingResample's 8-bit path, default box, reducing_gap None), which is
integer arithmetic and is restated exactly: `resize_pil` / `reference_aa` are the statement (tests/golden/pil_resize.npz holds
Pillow's own bytes) and the device is bit-identical to it.  For one axis with n_in source and n_out resized samples, in IEEE double:
  scale = n_in / n_out; fs = max(scale, 1.0); support = fs; ss = 1.0 / fs
  resized index X (crop offset added): center = (X + 0.5) * scale
    lo = max((int)(center - support + 0.5), 0); hi = min((int)(center + support + 0.5), n_in); n = hi - lo
    w[k] = tri((((k + lo) - center) + 0.5) * ss), tri(a) = 1 - |a| if |a| < 1 else 0;  ww = w[0] + w[1] + ... in that order
    if ww != 0: w[k] = w[k] / ww;  coef[k] = (int)(w[k] * 4194304.0 + 0.5)
  horizontal pass first   t[y][X][c] = clip((2097152 + sum_k src[y][lo+k][c] * coef[k]) >> 22, 0, 255) in int32, a byte
  vertical pass           the same rule on the bytes t with the row coefficients
  output                  v = (r - mean[c]) * scale[c] in float32 on the final byte r, as float32 or quant_input(v, 2^-Q0).

`Preprocessor(net, preset)` runs the device path; `pack(images, preset, device)` builds the pixel buffer and the per-image
records (tf2_image_src) from a list of HWC arrays, or refills buffers a captured graph reads."""
import contextlib
import ctypes as C
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np

# tf2_image_src, byte for byte (40 bytes)
SRC_DTYPE = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4"), ("row_pitch", "<i4"), ("resize_h", "<i4"), ("resize_w", "<i4"),
                      ("crop_y", "<i4"), ("crop_x", "<i4"), ("reserved", "<i4")])
SRC_WORDS = SRC_DTYPE.itemsize // 4

# status bits of a malformed record (TF2_PREP_*, include/tf2_amd.h)
BAD_SIZE, BAD_PITCH, BAD_OFFSET, OUT_OF_BUFFER, BAD_RESIZE, BAD_CROP = 1, 2, 4, 8, 16, 32
BAD_SCALE = 64                  # tf2_preprocess_aa only: h > AA_MAX_SCALE * resize_h or w > AA_MAX_SCALE * resize_w
MAX_SIDE = 32767
AA_MAX_SCALE = 32               # TF2_PREP_AA_MAX_SCALE: a filter of at most 2 * 32 + 1 taps an axis
AA_BITS = 22                    # fractional bits of a coefficient


@dataclass(frozen=True)
class Preset:
    """Resize, crop, channel order and per-channel mean / scale of one network's input.
      out_hw        the net's input size (image_h, image_w)
      resize        fixed (RH, RW); None: out_hw (no resize for a source of that size: SqueezeNet's 227 x 227 images)
      short_side    > 0: resize the shorter side to this and the longer one to int(short_side * long / short) (torchvision Resize(int))
      center_crop   crop the out_hw window from the middle, (RH - h) / 2 rounded as torchvision's center_crop does; else `crop`
      channels      the net's channel order over the letters of the source order ("BGR": net channel 0 is blue)
      antialias     resize as Pillow's Image.resize(size, BILINEAR) does (tf2_preprocess_aa) instead of the two-tap gather"""
    name: str
    out_hw: Tuple[int, int]
    mean: Tuple[float, float, float]
    scale: Tuple[float, float, float] = (1.0, 1.0, 1.0)
    channels: str = "BGR"
    resize: Optional[Tuple[int, int]] = None
    short_side: int = 0
    crop: Tuple[int, int] = (0, 0)
    center_crop: bool = False
    round_resized: bool = False
    antialias: bool = False

    def geometry(self, h: int, w: int) -> Tuple[int, int, int, int]:
        """(resize_h, resize_w, crop_y, crop_x) of an h x w source"""
        if self.short_side:
            s = self.short_side
            if w <= h:
                rw, rh = s, int(s * h / w)
            else:
                rh, rw = s, int(s * w / h)
        elif self.resize is not None:
            rh, rw = self.resize
        else:
            rh, rw = self.out_hw                # a source of another size is resized to the net's input
        if self.center_crop:
            cy, cx = int(round((rh - self.out_hw[0]) / 2.0)), int(round((rw - self.out_hw[1]) / 2.0))
        else:
            cy, cx = self.crop
        return rh, rw, cy, cx


# data_loader.py:26-44 ResNet50PreProcess: BGR swap, cv2.resize of the float image to 224 x 224, means 110.177 / 117.644 / 117.378
RESNET50 = Preset("resnet50", (224, 224), (110.177, 117.644, 117.378), resize=(224, 224))
# data_loader.py:46-68 GoogLeNetPreProcess: BGR swap, cv2.resize of the uint8 image to 256 x 256 (rounded to bytes: round_resized),
# means 104 / 117 / 123, crop int((256 - 224) / 2) = 16 from the top and the left
GOOGLENET = Preset("googlenet", (224, 224), (104.0, 117.0, 123.0), resize=(256, 256), crop=(16, 16), round_resized=True)
# data_loader.py:70-81 SqueezeNetPreProcess: BGR swap, (x - 127.5) / 128 on the image as it is (the reference feeds 227 x 227
# images: no resize); 1/128 is a power of two, so the scale is exact.  Sources of another size are resized to 227 x 227.
SQUEEZENET = Preset("squeezenet", (227, 227), (127.5, 127.5, 127.5), scale=(1 / 128,) * 3)
# data/SSD/__init__.py:30-38 base_transform (MEANS, data/SSD/config.py:12): cv2.resize to 300 x 300, means 104 / 117 / 123, BGR
SSD300 = Preset("ssd300", (300, 300), (104.0, 117.0, 123.0), resize=(300, 300))
# data_loader.py:83-90 load_data('resnet50'): Resize(256) (shorter side), CenterCrop(224), ToTensor (/255), Normalize(mean, std)
# in RGB; restated on 0..255 values as mean 255 * m and scale 1 / (255 * s).  PIL's resize antialiases when it shrinks; this does not.
_TV_MEAN, _TV_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TORCHVISION = Preset("torchvision", (224, 224), tuple(255.0 * m for m in _TV_MEAN), scale=tuple(1.0 / (255.0 * s) for s in _TV_STD),
                     channels="RGB", short_side=256, center_crop=True)
PRESETS = {p.name: p for p in (RESNET50, GOOGLENET, SQUEEZENET, SSD300, TORCHVISION)}
# load_data('resnet50') as torchvision runs it on PIL images: the same geometry and constants with Pillow's antialiased resize
TORCHVISION_PIL = replace(TORCHVISION, name="torchvision_pil", antialias=True)
AA_PRESETS = {p.name: p for p in (TORCHVISION_PIL,)}


def src_channels(preset: Preset, src_order: str = "RGB"):
    """src_channel[c] of the desc: the byte of a source pixel (letters of src_order, e.g. "RGB", "BGR", "RGBA") net channel c reads"""
    return [src_order.index(ch) for ch in preset.channels]


def quant_input(v, trans):
    """runner.cpp:158-164 as csrc/input_quant.h states it: int8 of v * trans rounded half away from zero, clamped; |v * trans| >= 2^31
    (or NaN) gives -128"""
    tmp = (np.asarray(v, np.float32) * np.float32(trans)).astype(np.float32)
    m = np.abs(tmp)
    with np.errstate(invalid="ignore"):
        ok = m < np.float32(2147483648.0)
        f = np.floor(np.where(ok, m, 0)).astype(np.float32)
        r = f + ((np.where(ok, m, 0) - f) >= np.float32(0.5)).astype(np.float32)
    r = np.where(tmp > 0, r, -r)
    r = np.clip(r, -128, 127)
    return np.where(ok, r, -128).astype(np.int8)


def trans_of(q0: int) -> float:
    """2^-Q0 (q0: the runtime value, net.q[0, 0])"""
    return float(np.float32(2.0 ** -int(q0)))


def record_status(srcs, pixel_bytes: int, pixels_bytes: int, out_hw) -> np.ndarray:
    """The device's validity rule per record (TF2_PREP_* bits; 0: valid) -- a statement in Python integers, no overflow"""
    srcs = np.asarray(srcs, SRC_DTYPE).reshape(-1)
    oh, ow = out_hw
    out = np.zeros(len(srcs), np.int32)
    for i, r in enumerate(srcs):
        h, w, pitch, off = int(r["h"]), int(r["w"]), int(r["row_pitch"]), int(r["offset"])
        rh, rw, cy, cx = int(r["resize_h"]), int(r["resize_w"]), int(r["crop_y"]), int(r["crop_x"])
        st = 0
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            st |= BAD_SIZE
        if pitch < w * pixel_bytes:
            st |= BAD_PITCH
        if off < 0:
            st |= BAD_OFFSET
        if st == 0 and off + (h - 1) * pitch + w * pixel_bytes > pixels_bytes:
            st |= OUT_OF_BUFFER
        if not (1 <= rh <= MAX_SIDE and 1 <= rw <= MAX_SIDE):
            st |= BAD_RESIZE
        if cy < 0 or cx < 0 or cy + oh > rh or cx + ow > rw:
            st |= BAD_CROP
        out[i] = st
    return out


def taps_of(f, n_src: int):
    """(i0, i1, w) of float64 source coordinates f on an axis of n_src samples: i0 = floor(f), float32 weight, both edge clamps with
    weight 0 (decided on the float64 value: a coordinate far outside the image is as good as any)"""
    f = np.asarray(f, np.float64)
    fl = np.floor(f)
    w = (f - fl).astype(np.float32)
    lo, hi = fl < 0, fl >= n_src - 1
    i0 = np.clip(fl, 0, n_src - 1).astype(np.int64)
    w[lo | hi] = 0
    return i0, np.minimum(i0 + 1, n_src - 1), w


def _taps(n_out: int, start: int, n_src: int, n_resized: int):
    return taps_of((np.arange(n_out, dtype=np.int64) + start + 0.5) * (n_src / n_resized) - 0.5, n_src)


def lerp_taps(img, ytaps, xtaps, round_resized: bool = False) -> np.ndarray:
    """The statement's interpolation of one HWC uint8 image (all its channels) at row taps (y0, y1, wy) and column taps (x0, x1, wx):
    float32 [C, len(y0), len(x0)] (0..255 units), optionally rounded to bytes"""
    img = np.asarray(img)
    h, w = img.shape[:2]
    (y0, y1, wy), (x0, x1, wx) = ytaps, xtaps
    p = np.moveaxis(img.reshape(h, w, -1), 2, 0).astype(np.float32)
    one = np.float32(1)
    wx, wy = wx[None, None, :], wy[None, :, None]
    top = p[:, y0][:, :, x0] * (one - wx) + p[:, y0][:, :, x1] * wx
    bot = p[:, y1][:, :, x0] * (one - wx) + p[:, y1][:, :, x1] * wx
    r = top * (one - wy) + bot * wy
    if round_resized:
        r = np.clip(np.rint(r), 0, 255).astype(np.float32)
    return r


def resize_one(img, rh: int, rw: int, cy: int, cx: int, oh: int, ow: int, round_resized: bool = False) -> np.ndarray:
    """The statement's resize + crop of one HWC uint8 image (all its channels): float32 [C, oh, ow] (0..255 units)"""
    h, w = np.asarray(img).shape[:2]
    return lerp_taps(img, _taps(oh, cy, h, rh), _taps(ow, cx, w, rw), round_resized)


def source_image(pixels, r, pixel_bytes: int, src_channel) -> np.ndarray:
    """the net's channels of the image a (valid) record describes: uint8 [h, w, 3]"""
    h, w, pitch, off = int(r["h"]), int(r["w"]), int(r["row_pitch"]), int(r["offset"])
    rows = np.stack([pixels[off + y * pitch: off + y * pitch + w * pixel_bytes] for y in range(h)]).reshape(h, w, pixel_bytes)
    return rows[:, :, list(src_channel)]


def reference(pixels, srcs, out_hw, pixel_bytes: int, src_channel, mean, scale, round_resized: bool = False, q0: Optional[int] = None):
    """The statement on the device's own inputs: pixels (uint8, 1-D), srcs (SRC_DTYPE records) -> (out, status).  out is float32
    [B, 3, oh, ow], or int8 quantised with 2^-q0 when q0 is given; a malformed record (status != 0) gives zeros."""
    pixels = np.asarray(pixels, np.uint8).reshape(-1)
    srcs = np.asarray(srcs, SRC_DTYPE).reshape(-1)
    oh, ow = out_hw
    status = record_status(srcs, pixel_bytes, pixels.size, out_hw)
    out = np.zeros((len(srcs), 3, oh, ow), np.float32)
    m32, s32 = np.asarray(mean, np.float32), np.asarray(scale, np.float32)
    for b, r in enumerate(srcs):
        if status[b]:
            continue
        res = resize_one(source_image(pixels, r, pixel_bytes, src_channel), int(r["resize_h"]), int(r["resize_w"]), int(r["crop_y"]),
                         int(r["crop_x"]), oh, ow, round_resized)
        out[b] = (res - m32[:, None, None]) * s32[:, None, None]
    if q0 is not None:
        q = quant_input(out, trans_of(q0))
        q[status != 0] = 0
        return q, status
    return out, status


def record_status_aa(srcs, pixel_bytes: int, pixels_bytes: int, out_hw) -> np.ndarray:
    """tf2_preprocess_aa's validity rule per record: record_status, and BAD_SCALE when the source is more than AA_MAX_SCALE times
    the resized image on an axis (an integer compare, evaluated when BAD_SIZE and BAD_RESIZE are clear)"""
    srcs = np.asarray(srcs, SRC_DTYPE).reshape(-1)
    out = record_status(srcs, pixel_bytes, pixels_bytes, out_hw)
    for i, r in enumerate(srcs):
        if not out[i] & (BAD_SIZE | BAD_RESIZE) and (int(r["h"]) > AA_MAX_SCALE * int(r["resize_h"]) or
                                                     int(r["w"]) > AA_MAX_SCALE * int(r["resize_w"])):
            out[i] |= BAD_SCALE
    return out


def aa_coefs(n_in: int, n_out: int, start: int = 0, count: Optional[int] = None):
    """The coefficient rule of one axis (csrc/resample_aa.h: aa_axis, aa_bounds, aa_weight, aa_coef) for the resized indices
    start .. start + count - 1: (lo int64 [count], n int64 [count], coef int32 [count, max n], zero beyond n)"""
    count = n_out - start if count is None else count
    scale = np.float64(n_in) / np.float64(n_out)
    fs = max(scale, np.float64(1.0))
    support, ss = fs, np.float64(1.0) / fs
    center = (np.arange(start, start + count, dtype=np.float64) + 0.5) * scale
    lo = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    hi = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in)
    n = hi - lo
    kmax = int(n.max()) if count else 0
    k = np.arange(kmax, dtype=np.int64)[None, :]
    a = np.abs((((k + lo[:, None]).astype(np.float64) - center[:, None]) + 0.5) * ss)
    w = np.where((a < 1.0) & (k < n[:, None]), 1.0 - a, 0.0)
    ww = np.zeros(count, np.float64)
    for j in range(kmax):                                  # in that order: not numpy's pairwise sum (the zeros beyond n add nothing)
        ww = ww + w[:, j]
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(ww[:, None] != 0, w / ww[:, None], w)
    coef = np.trunc(w * 4194304.0 + 0.5).astype(np.int32)
    coef[k >= n[:, None]] = 0
    return lo, n, coef


def aa_coefs_box(n_in: int, a0, a1, n_out: int):
    """The coefficient rule of one axis in its box form (csrc/resample_aa.h: aa_axis_box, aa_bounds_box, aa_weight, aa_coef; Pillow's
    Image.resize(size, BILINEAR, box=...)): n_out samples over the source interval [a0, a1) of an axis of n_in samples, a0 and a1
    float32.  d = float64(a1 - a0) with the subtraction in float32, scale = d / n_out, center = float64(a0) + (X + 0.5) * scale;
    support, the clamps at 0 and n_in, weights and coefficients as aa_coefs has them: (lo int64 [n_out], n int64 [n_out],
    coef int32 [n_out, max n], zero beyond n).  a0 = 0, a1 = n_in is aa_coefs(n_in, n_out)."""
    a0, a1 = np.float32(a0), np.float32(a1)
    scale = np.float64(a1 - a0) / np.float64(n_out)
    fs = max(scale, np.float64(1.0))
    support, ss = fs, np.float64(1.0) / fs
    center = np.float64(a0) + (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    lo = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    hi = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in)
    n = np.maximum(hi - lo, 0)
    kmax = int(n.max()) if n_out else 0
    k = np.arange(kmax, dtype=np.int64)[None, :]
    a = np.abs((((k + lo[:, None]).astype(np.float64) - center[:, None]) + 0.5) * ss)
    w = np.where((a < 1.0) & (k < n[:, None]), 1.0 - a, 0.0)
    ww = np.zeros(n_out, np.float64)
    for j in range(kmax):                                  # in that order, as in aa_coefs
        ww = ww + w[:, j]
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(ww[:, None] != 0, w / ww[:, None], w)
    coef = np.trunc(w * 4194304.0 + 0.5).astype(np.int32)
    coef[k >= n[:, None]] = 0
    return lo, n, coef


def resample_pass(src, lo, n, coef) -> np.ndarray:
    """One pass along axis 1 of uint8 [rows, n_in, C]: out[y, X, c] = clip((2^21 + sum_k src[y, lo[X] + k, c] * coef[X, k]) >> 22, 0, 255)
    in int32, as bytes [rows, len(lo), C]"""
    src = np.asarray(src, np.uint8)
    acc = np.full((src.shape[0], len(lo), src.shape[2]), 1 << (AA_BITS - 1), np.int32)
    for j in range(coef.shape[1]):
        idx = np.minimum(lo + j, src.shape[1] - 1)        # (beyond n the coefficient is 0)
        acc += src[:, idx, :].astype(np.int32) * coef[:, j][None, :, None]
    return np.clip(acc >> AA_BITS, 0, 255).astype(np.uint8)


def resize_pil(img, rh: int, rw: int, window=None) -> np.ndarray:
    """Pillow's Image.resize((rw, rh), BILINEAR) of an HWC uint8 image, restated (the module docstring): uint8 [rh, rw, C], or with
    window = (y0, x0, h_out, w_out) that window of it, uint8 [h_out, w_out, C] -- the crop of the whole resize, since every output
    byte depends on its own row and column coefficients alone.  The horizontal pass runs first and only on the source rows the
    vertical pass reads."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    img = img.reshape(h, w, -1)
    y0, x0, ho, wo = window if window is not None else (0, 0, rh, rw)
    assert 0 <= y0 and 0 <= x0 and y0 + ho <= rh and x0 + wo <= rw, "window outside the resized image"
    xlo, xn, xcoef = aa_coefs(w, rw, x0, wo)
    ylo, yn, ycoef = aa_coefs(h, rh, y0, ho)
    r0, r1 = int(ylo.min()), int((ylo + yn).max())
    t = resample_pass(img[r0:r1], xlo, xn, xcoef)                                        # [rows, wo, C]
    return np.swapaxes(resample_pass(np.swapaxes(t, 0, 1), ylo - r0, yn, ycoef), 0, 1)   # [ho, wo, C]


def reference_aa(pixels, srcs, out_hw, pixel_bytes: int, src_channel, mean, scale, q0: Optional[int] = None):
    """tf2_preprocess_aa's statement on the device's own inputs, in the form of `reference`: (out, status)"""
    pixels = np.asarray(pixels, np.uint8).reshape(-1)
    srcs = np.asarray(srcs, SRC_DTYPE).reshape(-1)
    oh, ow = out_hw
    status = record_status_aa(srcs, pixel_bytes, pixels.size, out_hw)
    out = np.zeros((len(srcs), 3, oh, ow), np.float32)
    m32, s32 = np.asarray(mean, np.float32), np.asarray(scale, np.float32)
    for b, r in enumerate(srcs):
        if status[b]:
            continue
        res = resize_pil(source_image(pixels, r, pixel_bytes, src_channel), int(r["resize_h"]), int(r["resize_w"]),
                         (int(r["crop_y"]), int(r["crop_x"]), oh, ow))
        out[b] = (np.moveaxis(res, 2, 0).astype(np.float32) - m32[:, None, None]) * s32[:, None, None]
    if q0 is not None:
        q = quant_input(out, trans_of(q0))
        q[status != 0] = 0
        return q, status
    return out, status


def pack_host(images, preset: Preset, align: int = 1):
    """(pixels uint8 [n], srcs SRC_DTYPE [B], pixel_bytes): the images (HWC uint8, 3 or 4 bytes a pixel) back to back, each row
    starting at a multiple of `align` bytes, with resize and crop from preset.geometry"""
    imgs = [np.ascontiguousarray(np.asarray(im.cpu() if hasattr(im, "cpu") else im, np.uint8)) for im in images]
    assert imgs, "no images"
    pb = imgs[0].shape[2] if imgs[0].ndim == 3 else 1
    srcs = np.zeros(len(imgs), SRC_DTYPE)
    chunks, at = [], 0
    for i, im in enumerate(imgs):
        assert im.ndim == 3 and im.shape[2] == pb and pb in (3, 4), f"image {i}: expected HWC uint8 with {pb} bytes a pixel, got {im.shape}"
        h, w = im.shape[:2]
        pitch = -(-w * pb // align) * align
        buf = np.zeros((h, pitch), np.uint8)
        buf[:, :w * pb] = im.reshape(h, w * pb)
        rh, rw, cy, cx = preset.geometry(h, w)
        srcs[i] = (at, h, w, pitch, rh, rw, cy, cx, 0)
        chunks.append(buf.reshape(-1))
        at += buf.size
    return np.concatenate(chunks), srcs, pb


def pack(images, preset: Preset, device, pixels=None, srcs=None, align: int = 1):
    """The device inputs of tf2_preprocess from a list of HWC uint8 arrays or tensors: (pixels uint8 tensor, srcs int32 tensor [B, 10]
    holding the tf2_image_src records).  With pixels= / srcs= the caller's tensors are filled instead (a captured graph reads the
    same buffers every replay): the pixels go to the front of `pixels`, the records fill `srcs`, whose row count is the batch."""
    import torch
    host, recs, _pb = pack_host(images, preset, align)
    rec_words = torch.from_numpy(recs.view(np.int32).reshape(len(recs), SRC_WORDS).copy())
    if pixels is None:
        pixels = torch.from_numpy(host).to(device)
    else:
        assert pixels.dtype == torch.uint8 and pixels.numel() >= host.size, "pixel buffer too small"
        pixels.view(-1)[:host.size].copy_(torch.from_numpy(host), non_blocking=False)
    if srcs is None:
        srcs = rec_words.to(device)
    else:
        assert srcs.dtype == torch.int32 and tuple(srcs.shape) == tuple(rec_words.shape), "srcs must be int32 [B, 10] of this batch"
        srcs.copy_(rec_words)
    return pixels, srcs


def desc_of(preset: Preset, src_order: str = "RGB"):
    from . import _lib
    d = _lib.PreprocessDesc()
    d.size = C.sizeof(_lib.PreprocessDesc)
    d.pixel_bytes = len(src_order)
    for c, s in enumerate(src_channels(preset, src_order)):
        d.src_channel[c] = s
    d.round_resized = int(preset.round_resized)
    for c in range(3):
        d.mean[c], d.scale[c] = preset.mean[c], preset.scale[c]
    return d


def reference_images(images, preset: Preset, src_order: str = "RGB", q0: Optional[int] = None, out_hw=None):
    """`reference` on a list of HWC images, laid out as `pack` lays them out"""
    pixels, srcs, pb = pack_host(images, preset)
    assert pb == len(src_order)
    return reference(pixels, srcs, out_hw or preset.out_hw, pb, src_channels(preset, src_order),
                     np.float32(preset.mean), np.float32(preset.scale), preset.round_resized, q0)[0]


@contextlib.contextmanager
def image_outputs(out: str, n: int, out_hw, dev, stream=None, images=None, status=None):
    """The outputs of an image entry point (tf2_preprocess*, tf2_roi_crop*, tf2_roi_warp), as a context that makes `stream` (default:
    the current one of `dev`) current: images int8 (out="q") or float32 [n, 3, h, w] and status int32 [n], allocated on the stream or
    -- passed in -- checked and left alone.  Yields (images, status, stream)."""
    import torch
    from . import _lib
    dtype = torch.int8 if out == "q" else torch.float32
    stream = stream or torch.cuda.current_stream(dev)
    with torch.cuda.stream(stream):
        if images is None:
            images = torch.empty(n, 3, *out_hw, dtype=dtype, device=dev)
        if status is None:
            status = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.expect(images, dtype, (n, 3) + tuple(out_hw), dev)
        _lib.expect(status, torch.int32, (n,), dev)
        yield images, status, stream


class Preprocessor:
    """tf2_preprocess -- tf2_preprocess_aa when preset.antialias -- for `net` (a tf2_amd.network.NetWork) with `preset`, on
    sources whose pixel bytes are the letters of src_order ("RGB", "BGR", "RGBA", "BGRA"...).
      pp(pixels, srcs, out="q" | "f32", stream=None) -> (images, status)
    pixels: uint8 device tensor, srcs: int32 [B, 10] device tensor of tf2_image_src records (`pack`).  images: int8 (out="q",
    quantised with the net's 2^-Q0 as tf2_net_run_q reads them) or float32 [B, 3, image_h, image_w]; status: int32 [B], 0 or the
    TF2_PREP_* bits of a malformed record (its image is zeros).  Enqueued on `stream` (default: the current one)."""

    def __init__(self, net, preset: Preset, src_order: str = "RGB"):
        self.net, self.preset, self.src_order = net, preset, src_order
        self.desc = desc_of(preset, src_order)
        self.out_hw = (int(net._nd.image_h), int(net._nd.image_w))

    def __call__(self, pixels, srcs, out: str = "q", stream=None):
        import torch
        from . import _lib
        assert out in ("q", "f32"), out
        dev = _lib.expect(pixels, torch.uint8)
        _lib.expect(srcs, torch.int32, device=dev, cols=SRC_WORDS)
        B = srcs.shape[0]
        with image_outputs(out, B, self.out_hw, dev, stream) as (res, status, stream):
            fn = _lib.lib().tf2_preprocess_aa if self.preset.antialias else _lib.lib().tf2_preprocess
            _lib.check(fn(self.net._h, C.byref(self.desc), pixels.data_ptr(), pixels.numel(), srcs.data_ptr(), B, int(out == "q"), res.data_ptr(),
                          status.data_ptr(), stream.cuda_stream))
        return res, status

    def reference(self, pixels, srcs, out: str = "q"):
        """The statement on the same inputs (host copies of the tensors), with the net's Q0 for out="q" """
        p = pixels.cpu().numpy() if hasattr(pixels, "cpu") else np.asarray(pixels)
        s = srcs.cpu().numpy() if hasattr(srcs, "cpu") else np.asarray(srcs)
        s = np.ascontiguousarray(s, np.int32).view(SRC_DTYPE).reshape(-1)
        q0 = int(self.net.q[0, 0]) if out == "q" else None
        if self.preset.antialias:
            return reference_aa(p, s, self.out_hw, len(self.src_order), src_channels(self.preset, self.src_order),
                                np.float32(self.preset.mean), np.float32(self.preset.scale), q0)
        return reference(p, s, self.out_hw, len(self.src_order), src_channels(self.preset, self.src_order),
                         np.float32(self.preset.mean), np.float32(self.preset.scale), self.preset.round_resized, q0)
