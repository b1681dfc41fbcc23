"""Second-stage crops on the device (tf2_roi_select / tf2_roi_crop, include/tf2_amd.h; csrc/roi_crop.hip): the det / counts a
detector left in device memory (ssd.DeviceDetector) and the source pixels of its images (preprocess.pack) in, the input of a second
network out -- one image per chosen box, float32 or int8 quantised with that net's 2^-Q0 -- with no copy to the host in between: the
middle of the reference's detect -> crop -> embed -> match cascade (TransForm_Kit/Compression/faceverify/README.md).

The reference gives no program text for this step, so the two functions below ARE the statement and the yardstick of the device,
which is bit-identical to them.
  reference_select  per source image b the candidates are the rows (c, r) of det[b] with c among `classes`, r < min(counts[b, c],
                    top_k), score > min_score (strict, float32; a NaN never passes) and a valid transformed box; the best max_rois
                    by (score descending, class ascending, rank ascending) fill the image's slots b * max_rois + 0.., the rest get
                    the empty record (image -1, every other field 0).  The transform (float64 from the float32 det values, each
                    operation rounded separately; w, h the source's size):
                      X1 = x1 * w, X2 = x2 * w, Y1 = y1 * h, Y2 = y2 * h;  cx = (X1 + X2) / 2, cy = (Y1 + Y2) / 2
                      bw = (X2 - X1) * expand_w, bh = (Y2 - Y1) * expand_h;  square: bw = bh = (bh if bh > bw else bw)
                      x0 = cx - bw / 2, x1' = cx + bw / 2, y0 = cy - bh / 2, y1' = cy + bh / 2
                      clip: v = 0 if v < 0 else (limit if v > limit else v), limit w for x, h for y (a NaN stays a NaN)
                      one rounding to float32
                    valid iff the four float32 values are finite and x1' - x0 >= 1 and y1' - y0 >= 1 (float64 on the float32
                    values).  A source record whose h or w is outside 1..32767 gives its image no ROI.
  reference_crop    per slot with record R, source r = srcs[R.image] and output pixel (y, x) of the OH x OW output (float64):
                      sy = (R.y1 - R.y0) / OH;  t = (y + 0.5) * sy;  t = R.y0 + t;  fy = t - 0.5;  the same for columns
                    then preprocess's rule from fy on (preprocess.taps_of, lerp_taps, quant_input: the same code): taps, float32
                    weights, edge clamps with weight 0 (a box may leave the image), interpolation, optional rounding, mean, scale,
                    quantisation.  R = (0, 0, w, h) is preprocess.reference with resize = (OH, OW) and no crop, bit for bit.
                    status per slot: EMPTY alone for image == -1; else BAD_IMAGE (outside 0..B-1), BAD_BOX (the validity rule)
                    and, for an image inside the batch, BAD_SRC (the record fails preprocess's size / pitch / offset / extent
                    rule; its resize_* and crop_* fields are not read) in any combination; a slot with a status is zeros.

Antialiased crops (tf2_roi_crop_aa; csrc/roi_crop_aa.hip): the same table through Pillow's Image.resize((ow, oh), BILINEAR,
box=(x0, y0, x1, y1)) on the 8-bit source, restated exactly (preprocess.aa_coefs_box is the coefficient rule of a box; tests/golden/
pil_resize_box.npz holds Pillow's own bytes).
  crop_pil            Pillow's resize(box=) of one HWC uint8 image.  The filter is centred on the box and clamped at the IMAGE: it reads
                      pixels outside the box and inside the image, so this is not "crop, then resize".
  reference_crop_aa   per slot crop_pil of the source's net channels with the slot's float32 box, then (r - mean) * scale in float32 and
                      the quantisation, in the form of reference_crop.  R = (0, 0, w, h) is preprocess.reference_aa with
                      resize = (OH, OW) and crop (0, 0), bit for bit.
  roi_status_aa       roi_status's rule and, for a slot it passes (an image inside the batch, BAD_BOX and BAD_SRC clear), BOX_OUTSIDE
                      unless 0 <= x0, x1 <= w, 0 <= y0, y1 <= h (float64 on the float32 values) and BAD_SCALE when the float32 side
                      x1 - x0 > 32 * OW or y1 - y0 > 32 * OH; a slot with a status is zeros.

`DeviceCropper(net2, preset, ...)` runs the device path; antialias=True (or a preset with antialias) takes the antialiased one."""
import ctypes as C
from typing import Optional

import numpy as np

from . import preprocess as P

# tf2_roi, byte for byte (32 bytes)
ROI_DTYPE = np.dtype([("image", "<i4"), ("cls", "<i4"), ("rank", "<i4"), ("score", "<f4"), ("x0", "<f4"), ("y0", "<f4"), ("x1", "<f4"),
                      ("y1", "<f4")])
ROI_WORDS = ROI_DTYPE.itemsize // 4
# status bits of a slot that was not cropped (TF2_ROI_*, include/tf2_amd.h)
EMPTY, BAD_IMAGE, BAD_BOX, BAD_SRC = 1, 2, 4, 8
BOX_OUTSIDE, BAD_SCALE = 16, 32         # tf2_roi_crop_aa only
MAX_ROIS, MAX_CLASSES, MAX_TOP_K = 64, 256, 256
_SRC_BITS = P.BAD_SIZE | P.BAD_PITCH | P.BAD_OFFSET | P.OUT_OF_BUFFER


def box_ok(x0, y0, x1, y1):
    """the validity rule of a float32 box: finite, both sides at least one source pixel (float64 on the float32 values)"""
    b = [np.asarray(v, np.float32) for v in (x0, y0, x1, y1)]
    fin = np.isfinite(b[0]) & np.isfinite(b[1]) & np.isfinite(b[2]) & np.isfinite(b[3])
    with np.errstate(invalid="ignore"):
        return fin & (b[2].astype(np.float64) - b[0].astype(np.float64) >= 1.0) & (b[3].astype(np.float64) - b[1].astype(np.float64) >= 1.0)


def transform_boxes(rows, w: int, h: int, expand=(1.0, 1.0), square: bool = False, clip: bool = True) -> np.ndarray:
    """det rows [..., 5] (score, x1, y1, x2, y2; float32) -> float32 boxes [..., 4] (x0, y0, x1, y1) in pixels of a w x h source"""
    d = np.asarray(rows, np.float32).astype(np.float64)
    w, h = np.float64(w), np.float64(h)
    ew, eh = np.float64(np.float32(expand[0])), np.float64(np.float32(expand[1]))
    with np.errstate(all="ignore"):
        X1, X2, Y1, Y2 = d[..., 1] * w, d[..., 3] * w, d[..., 2] * h, d[..., 4] * h
        cx, cy = (X1 + X2) / 2.0, (Y1 + Y2) / 2.0
        bw, bh = (X2 - X1) * ew, (Y2 - Y1) * eh
        if square:
            bw = bh = np.where(bh > bw, bh, bw)
        box = [cx - bw / 2.0, cy - bh / 2.0, cx + bw / 2.0, cy + bh / 2.0]
        if clip:
            box = [np.where(v < 0.0, 0.0, np.where(v > lim, lim, v)) for v, lim in zip(box, (w, h, w, h))]
        return np.stack(box, axis=-1).astype(np.float32)


def empty_rois(n: int) -> np.ndarray:
    r = np.zeros(n, ROI_DTYPE)
    r["image"] = -1
    return r


def reference_select(det, counts, srcs, classes=(15,), min_score: float = 0.5, max_rois: int = 4, expand=(1.0, 1.0),
                     square: bool = False, clip: bool = True):
    """The statement: det float32 [B, C, K, 5], counts int32 [B, C], srcs SRC_DTYPE [B] -> (rois ROI_DTYPE [B * max_rois],
    roi_counts int32 [B])"""
    det = np.asarray(det, np.float32)
    B, Cn, K = det.shape[:3]
    counts = np.asarray(counts).reshape(B, Cn).astype(np.int64)
    srcs = np.asarray(srcs, P.SRC_DTYPE).reshape(-1)
    taken = np.zeros(Cn, bool)
    taken[list(classes)] = True
    rois, n_out = empty_rois(B * max_rois), np.zeros(B, np.int32)
    cls, rank = np.meshgrid(np.arange(Cn), np.arange(K), indexing="ij")
    for b in range(B):
        h, w = int(srcs[b]["h"]), int(srcs[b]["w"])
        if not (1 <= h <= P.MAX_SIDE and 1 <= w <= P.MAX_SIDE):
            continue
        score = det[b, :, :, 0]
        box = transform_boxes(det[b], w, h, expand, square, clip)
        cand = taken[:, None] & (rank < np.minimum(counts[b], K)[:, None]) & (score > np.float32(min_score))
        cand &= box_ok(box[..., 0], box[..., 1], box[..., 2], box[..., 3])
        c, r = cls[cand], rank[cand]
        order = np.lexsort((r, c, -score[cand]))[:max_rois]          # score descending, class ascending, rank ascending
        n = len(order)
        out = rois[b * max_rois: b * max_rois + n]
        out["image"], out["cls"], out["rank"], out["score"] = b, c[order], r[order], score[cand][order]
        for k, name in enumerate(("x0", "y0", "x1", "y1")):
            out[name] = box[cand][order, k]
        n_out[b] = n
    return rois, n_out


def roi_status(rois, srcs, pixel_bytes: int, pixels_bytes: int) -> np.ndarray:
    """The device's validity rule per slot (TF2_ROI_* bits; 0: cropped)"""
    rois = np.asarray(rois, ROI_DTYPE).reshape(-1)
    srcs = np.asarray(srcs, P.SRC_DTYPE).reshape(-1)
    out = np.zeros(len(rois), np.int32)
    for s, R in enumerate(rois):
        i = int(R["image"])
        if i == -1:
            out[s] = EMPTY
            continue
        st = 0
        if not 0 <= i < len(srcs):
            st |= BAD_IMAGE
        elif P.record_status(srcs[i:i + 1], pixel_bytes, pixels_bytes, (1, 1))[0] & _SRC_BITS:
            st |= BAD_SRC
        if not box_ok(R["x0"], R["y0"], R["x1"], R["y1"]):
            st |= BAD_BOX
        out[s] = st
    return out


def _roi_taps(lo, hi, n_out: int, n_src: int):
    lo, hi = np.float64(np.float32(lo)), np.float64(np.float32(hi))
    step = (hi - lo) / np.float64(n_out)
    t = (np.arange(n_out, dtype=np.float64) + 0.5) * step
    t = lo + t
    return P.taps_of(t - 0.5, n_src)


def reference_crop(pixels, srcs, rois, out_hw, pixel_bytes: int, src_channel, mean, scale, round_resized: bool = False,
                   q0: Optional[int] = None):
    """The statement on the device's own inputs: pixels (uint8, 1-D), srcs (SRC_DTYPE [B]), rois (ROI_DTYPE [S]) -> (out, status).
    out is float32 [S, 3, oh, ow], or int8 quantised with 2^-q0 when q0 is given; a slot with a status gives zeros."""
    pixels = np.asarray(pixels, np.uint8).reshape(-1)
    srcs = np.asarray(srcs, P.SRC_DTYPE).reshape(-1)
    rois = np.asarray(rois, ROI_DTYPE).reshape(-1)
    oh, ow = out_hw
    status = roi_status(rois, srcs, pixel_bytes, pixels.size)
    out = np.zeros((len(rois), 3, oh, ow), np.float32)
    m32, s32 = np.asarray(mean, np.float32), np.asarray(scale, np.float32)
    images = {}
    for s, R in enumerate(rois):
        if status[s]:
            continue
        i = int(R["image"])
        if i not in images:
            images[i] = P.source_image(pixels, srcs[i], pixel_bytes, src_channel)
        r = srcs[i]
        res = P.lerp_taps(images[i], _roi_taps(R["y0"], R["y1"], oh, int(r["h"])), _roi_taps(R["x0"], R["x1"], ow, int(r["w"])),
                          round_resized)
        out[s] = (res - m32[:, None, None]) * s32[:, None, None]
    if q0 is not None:
        q = P.quant_input(out, P.trans_of(q0))
        q[status != 0] = 0
        return q, status
    return out, status


def crop_pil(img, box, oh: int, ow: int) -> np.ndarray:
    """Pillow's Image.resize((ow, oh), BILINEAR, box=box) of an HWC (or HW) uint8 image, restated: uint8 [oh, ow, C].  box =
    (x0, y0, x1, y1) in source pixels, taken as float32 (Pillow's box is float[4]) and inside the image (Pillow's precondition).  The
    horizontal pass runs first and only on the source rows the vertical pass reads."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    img = img.reshape(h, w, -1)
    x0, y0, x1, y1 = (np.float32(v) for v in box)
    xlo, xn, xcoef = P.aa_coefs_box(w, x0, x1, ow)
    ylo, yn, ycoef = P.aa_coefs_box(h, y0, y1, oh)
    r0, r1 = int(ylo.min()), int((ylo + yn).max())
    t = P.resample_pass(img[r0:r1], xlo, xn, xcoef)                                          # [rows, ow, C]
    return np.swapaxes(P.resample_pass(np.swapaxes(t, 0, 1), ylo - r0, yn, ycoef), 0, 1)     # [oh, ow, C]


def roi_status_aa(rois, srcs, pixel_bytes: int, pixels_bytes: int, out_hw) -> np.ndarray:
    """tf2_roi_crop_aa's validity rule per slot: roi_status, and for a slot it passes BOX_OUTSIDE / BAD_SCALE (the module docstring)"""
    rois = np.asarray(rois, ROI_DTYPE).reshape(-1)
    srcs = np.asarray(srcs, P.SRC_DTYPE).reshape(-1)
    out = roi_status(rois, srcs, pixel_bytes, pixels_bytes)
    oh, ow = out_hw
    for s, R in enumerate(rois):
        if out[s]:
            continue
        r = srcs[int(R["image"])]
        x0, y0, x1, y1 = (np.float32(R[k]) for k in ("x0", "y0", "x1", "y1"))
        if not (np.float64(x0) >= 0.0 and np.float64(x1) <= np.float64(r["w"]) and np.float64(y0) >= 0.0 and
                np.float64(y1) <= np.float64(r["h"])):
            out[s] |= BOX_OUTSIDE
        if np.float64(x1 - x0) > np.float64(P.AA_MAX_SCALE * ow) or np.float64(y1 - y0) > np.float64(P.AA_MAX_SCALE * oh):
            out[s] |= BAD_SCALE
    return out


def reference_crop_aa(pixels, srcs, rois, out_hw, pixel_bytes: int, src_channel, mean, scale, round_resized: bool = False,
                      q0: Optional[int] = None):
    """tf2_roi_crop_aa's statement on the device's own inputs, in the form of reference_crop: (out, status).  round_resized is not
    used (the resize result is bytes already)."""
    pixels = np.asarray(pixels, np.uint8).reshape(-1)
    srcs = np.asarray(srcs, P.SRC_DTYPE).reshape(-1)
    rois = np.asarray(rois, ROI_DTYPE).reshape(-1)
    oh, ow = out_hw
    status = roi_status_aa(rois, srcs, pixel_bytes, pixels.size, out_hw)
    out = np.zeros((len(rois), 3, oh, ow), np.float32)
    m32, s32 = np.asarray(mean, np.float32), np.asarray(scale, np.float32)
    images = {}
    for s, R in enumerate(rois):
        if status[s]:
            continue
        i = int(R["image"])
        if i not in images:
            images[i] = P.source_image(pixels, srcs[i], pixel_bytes, src_channel)
        res = crop_pil(images[i], (R["x0"], R["y0"], R["x1"], R["y1"]), oh, ow)
        out[s] = (np.moveaxis(res, 2, 0).astype(np.float32) - m32[:, None, None]) * s32[:, None, None]
    if q0 is not None:
        q = P.quant_input(out, P.trans_of(q0))
        q[status != 0] = 0
        return q, status
    return out, status


def whole_image_rois(srcs) -> np.ndarray:
    """one ROI per source record covering the whole image, (0, 0, w, h): reference_crop of it is preprocess.reference with
    resize = out_hw and no crop, reference_crop_aa of it preprocess.reference_aa with the same"""
    srcs = np.asarray(srcs, P.SRC_DTYPE).reshape(-1)
    rois = np.zeros(len(srcs), ROI_DTYPE)
    rois["image"] = np.arange(len(srcs))
    rois["x1"], rois["y1"] = srcs["w"], srcs["h"]
    return rois


def class_mask(classes, num_classes: int):
    """class_mask[8] of the desc; refuses what the library refuses"""
    words = [0] * 8
    for c in classes:
        c = int(c)
        if not 1 <= c < num_classes:
            raise ValueError(f"class {c} outside 1..{num_classes - 1}")
        words[c >> 5] |= 1 << (c & 31)
    if not any(words):
        raise ValueError("no class taken")
    return words


def rois_to_device(rois, device):
    """ROI_DTYPE records -> the int32 [S, 8] device tensor the cropper reads"""
    import torch
    rois = np.ascontiguousarray(np.asarray(rois, ROI_DTYPE).reshape(-1))
    return torch.from_numpy(rois.view(np.int32).reshape(len(rois), ROI_WORDS).copy()).to(device)


def rois_to_host(rois) -> np.ndarray:
    """the int32 [S, 8] tensor of a select -> ROI_DTYPE records [S]"""
    a = rois.cpu().numpy() if hasattr(rois, "cpu") else np.asarray(rois)
    return np.ascontiguousarray(a, np.int32).view(ROI_DTYPE).reshape(-1)


def _srcs_host(srcs) -> np.ndarray:
    a = srcs.cpu().numpy() if hasattr(srcs, "cpu") else np.asarray(srcs)
    return a.reshape(-1) if a.dtype == P.SRC_DTYPE else np.ascontiguousarray(a, np.int32).view(P.SRC_DTYPE).reshape(-1)


class DeviceCropper:
    """tf2_roi_select + tf2_roi_crop for the second network `net2` (a tf2_amd.network.NetWork) with `preset`'s means, scales,
    channel order and round_resized (its resize and crop are not used: the boxes say what is resampled), on sources whose pixel
    bytes are the letters of src_order.  num_classes / top_k: the layout of the detector's det [B, C, K, 5] / counts [B, C].
    antialias: crop with tf2_roi_crop_aa (Pillow's resize(box=); the boxes must lie inside their images, as clip=True makes them)
    instead of tf2_roi_crop; None: preset.antialias.  crop, __call__, reference_crop and reference follow the choice.
      select(det, counts, srcs, stream=None, rois=None, roi_counts=None) -> (rois int32 [B * max_rois, 8], roi_counts int32 [B])
      crop(pixels, srcs, rois, out="q" | "f32", stream=None, images=None, status=None) -> (images [S, 3, h, w], status int32 [S])
      __call__(det, counts, pixels, srcs, out="q", stream=None, ...) -> (images, status, rois, roi_counts)
    pixels / srcs: the uint8 buffer and int32 [B, 10] records of preprocess.pack (the detector's own sources); rois: the table as
    int32 words (rois_to_host / rois_to_device convert to and from ROI_DTYPE).  images: int8 (out="q", quantised with net2's 2^-Q0) or
    float32; a slot with a nonzero status (EMPTY, BAD_*) is zeros.  Everything is enqueued on `stream` (default: the current one),
    nothing synchronises or allocates beyond the outputs, which may be passed in (a captured graph then writes the same tensors at
    every replay)."""

    def __init__(self, net2, preset: P.Preset, src_order: str = "RGB", num_classes: int = 21, top_k: int = 200, classes=(15,),
                 min_score: float = 0.5, max_rois: int = 4, expand=(1.0, 1.0), square: bool = False, clip: bool = True,
                 antialias: Optional[bool] = None):
        from . import _lib
        self.net, self.preset, self.src_order = net2, preset, src_order
        self.antialias = bool(preset.antialias if antialias is None else antialias)
        self.num_classes, self.top_k, self.classes = int(num_classes), int(top_k), tuple(int(c) for c in classes)
        self.min_score, self.max_rois, self.expand = float(min_score), int(max_rois), (float(expand[0]), float(expand[1]))
        self.square, self.clip = bool(square), bool(clip)
        self.desc = P.desc_of(preset, src_order)
        self.out_hw = (int(net2._nd.image_h), int(net2._nd.image_w))
        d = _lib.RoiDesc()
        d.size = C.sizeof(_lib.RoiDesc)
        d.num_classes, d.top_k, d.min_score, d.max_rois = self.num_classes, self.top_k, self.min_score, self.max_rois
        for k, word in enumerate(class_mask(self.classes, self.num_classes)):
            d.class_mask[k] = word
        d.expand_w, d.expand_h = self.expand
        d.square, d.clip = int(self.square), int(self.clip)
        self.roi_desc = d

    def select(self, det, counts, srcs, stream=None, rois=None, roi_counts=None):
        import torch
        from . import _lib
        B = srcs.shape[0]
        dev = _lib.expect(det, torch.float32, (B, self.num_classes, self.top_k, 5))
        _lib.expect(counts, torch.int32, (B, self.num_classes), dev)
        _lib.expect(srcs, torch.int32, device=dev, cols=P.SRC_WORDS)
        stream = stream or torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            if rois is None:
                rois = torch.empty(B * self.max_rois, ROI_WORDS, dtype=torch.int32, device=dev)
            if roi_counts is None:
                roi_counts = torch.empty(B, dtype=torch.int32, device=dev)
            _lib.expect(rois, torch.int32, (B * self.max_rois, ROI_WORDS), dev)
            _lib.expect(roi_counts, torch.int32, (B,), dev)
            _lib.check(_lib.lib().tf2_roi_select(C.byref(self.roi_desc), det.data_ptr(), counts.data_ptr(), srcs.data_ptr(), B,
                                                 rois.data_ptr(), roi_counts.data_ptr(), stream.cuda_stream))
        return rois, roi_counts

    def crop(self, pixels, srcs, rois, out: str = "q", stream=None, images=None, status=None):
        import torch
        from . import _lib
        assert out in ("q", "f32"), out
        dev = _lib.expect(pixels, torch.uint8)
        _lib.expect(srcs, torch.int32, device=dev, cols=P.SRC_WORDS)
        _lib.expect(rois, torch.int32, device=dev, cols=ROI_WORDS)
        B, S = srcs.shape[0], rois.shape[0]
        with P.image_outputs(out, S, self.out_hw, dev, stream, images, status) as (images, status, stream):
            fn = _lib.lib().tf2_roi_crop_aa if self.antialias else _lib.lib().tf2_roi_crop
            _lib.check(fn(self.net._h, C.byref(self.desc), pixels.data_ptr(), pixels.numel(), srcs.data_ptr(), B, rois.data_ptr(), S,
                          int(out == "q"), images.data_ptr(), status.data_ptr(), stream.cuda_stream))
        return images, status

    def __call__(self, det, counts, pixels, srcs, out: str = "q", stream=None, rois=None, roi_counts=None, images=None, status=None):
        rois, roi_counts = self.select(det, counts, srcs, stream, rois, roi_counts)
        images, status = self.crop(pixels, srcs, rois, out, stream, images, status)
        return images, status, rois, roi_counts

    def reference_select(self, det, counts, srcs):
        """reference_select on host copies of the tensors, with this cropper's settings"""
        host = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
        return reference_select(host(det), host(counts), _srcs_host(srcs), self.classes, self.min_score, self.max_rois, self.expand,
                                self.square, self.clip)

    def reference_crop(self, pixels, srcs, rois, out: str = "q"):
        """reference_crop -- reference_crop_aa when antialias -- on host copies of the tensors, with net2's Q0 for out="q" """
        p = pixels.cpu().numpy() if hasattr(pixels, "cpu") else np.asarray(pixels)
        r = rois if isinstance(rois, np.ndarray) and rois.dtype == ROI_DTYPE else rois_to_host(rois)
        fn = reference_crop_aa if self.antialias else reference_crop
        return fn(p, _srcs_host(srcs), r, self.out_hw, len(self.src_order), P.src_channels(self.preset, self.src_order),
                  np.float32(self.preset.mean), np.float32(self.preset.scale), self.preset.round_resized,
                  int(self.net.q[0, 0]) if out == "q" else None)

    def reference(self, det, counts, pixels, srcs, out: str = "q"):
        """The statement of __call__ on host copies of the same inputs: (images, status, rois ROI_DTYPE, roi_counts)"""
        rois, n = self.reference_select(det, counts, srcs)
        images, status = self.reference_crop(pixels, srcs, rois, out)
        return images, status, rois, n
