"""Aligned crops on the device (tf2_roi_fit / tf2_roi_warp, include/tf2_amd.h; csrc/roi_warp.hip): the select / crop split of roi.py
for windows that are not upright.  The reference's face network is calibrated and evaluated on ALIGNED faces (TransForm_Kit/
Quantization/data_loader.py:103-107 loads test_images_aligned_test): a similarity warp that puts eyes, nose and mouth corners on a
fixed template.  tf2_roi_fit turns K landmarks a slot into a table of transforms in device memory, tf2_roi_warp resamples each
transform's window out of the source pixels into one image of the second net's input, with no copy to the host in between.

The functions below ARE the statement and the yardstick of the device, which is bit-identical to them.  Everything is IEEE float64
from the float32 inputs, every operation rounded separately, sums in index order from 0.0.
  reference_fit   per slot with record R (roi.ROI_DTYPE) and float32 landmarks (u_i, v_i), i < K: space 0 takes them as source pixels
                  (sx = u, sy = v), space 1 as relative to the slot's box (sx = x0 + u * (x1 - x0), sy = y0 + v * (y1 - y0)).  With the
                  template (tx_i, ty_i) in output pixels, the least-squares similarity without reflection landmarks -> template,
                  inverted into the output -> source map:
                    mx = (sum sx_i) / K, my, ux = (sum tx_i) / K, uy
                    px = sx_i - mx, py = sy_i - my, qx = tx_i - ux, qy = ty_i - uy
                    var += px*px + py*py;   c += px*qx + py*qy;   s += px*qy - py*qx        (i = 0 .. K-1)
                    A = c / var;  B = s / var;  n = A*A + B*B;  a = A / n;  b = -B / n
                    m = { a, -b, (mx - a*ux) + b*uy,   b, a, (my - b*ux) - a*uy }
                  status per slot: EMPTY alone for image == -1; else BAD_BOX (space 1 and the box fails roi.box_ok) and BAD_LANDMARKS
                  (a landmark coordinate not finite) in any combination; with both clear the fit runs and BAD_LANDMARKS is set unless
                  var > 0, n > 0 and the six results are finite.  A slot with a status gets the empty record (image -1, m all +0.0).
  warp_pil        Pillow's Image.transform((ow, oh), Image.AFFINE, m, resample=BILINEAR) of one HWC uint8 image, restated byte for
                  byte (ImagingGenericTransform with affine_transform and the 8-bit bilinear filter); tests/golden/pil_affine.npz holds
                  Pillow's own bytes.  For output pixel (y, x):
                    xin = x + 0.5; yin = y + 0.5;  fx = (m0*xin + m1*yin) + m2;  fy = (m3*xin + m4*yin) + m5
                    inside iff fx >= 0 and fx < w and fy >= 0 and fy < h (a NaN is outside); outside: byte 0 in every channel
                    inside: fx -= 0.5; fy -= 0.5; X = floor(fx); dx = fx - X; Y = floor(fy); dy = fy - Y
                            xa = clamp(X, 0, w-1); xb = clamp(X+1, 0, w-1); ya = clamp(Y, 0, h-1)
                            v1 = p[ya][xa] + (p[ya][xb] - p[ya][xa]) * dx
                            v2 = p[Y+1][xa] + (p[Y+1][xb] - p[Y+1][xa]) * dx if Y + 1 < h else v1
                            byte = trunc(v1 + (v2 - v1) * dy)
                  There is no antialiasing: Pillow's transform has none.
  reference_warp  per slot warp_pil of the source's net channels with the slot's matrix, then (byte - mean) * scale in float32 (a fill
                  byte 0 goes through the same line) and the quantisation, in the form of roi.reference_crop.  status per slot: EMPTY
                  alone for image == -1; else BAD_IMAGE, BAD_SRC (roi.roi_status's rules) and BAD_MATRIX (an entry of m not finite) in
                  any combination; a slot with a status is zeros.

`DeviceAligner(net2, preset, template, ...)` runs the device path."""
import ctypes as C
from typing import Optional

import numpy as np

from . import preprocess as P
from . import roi as R

# tf2_roi_xform, byte for byte (56 bytes)
XFORM_DTYPE = np.dtype([("image", "<i4"), ("reserved", "<i4"), ("m", "<f8", (6,))])
XFORM_WORDS = XFORM_DTYPE.itemsize // 4
EMPTY, BAD_IMAGE, BAD_BOX, BAD_SRC = R.EMPTY, R.BAD_IMAGE, R.BAD_BOX, R.BAD_SRC
BAD_LANDMARKS, BAD_MATRIX = 64, 128     # tf2_roi_fit only, tf2_roi_warp only
MIN_POINTS, MAX_POINTS = 2, 16


def empty_xforms(n: int) -> np.ndarray:
    x = np.zeros(n, XFORM_DTYPE)
    x["image"] = -1
    return x


def scaled_template(points, from_hw, to_hw) -> np.ndarray:
    """template points (x, y) given in pixels of a from_hw = (h, w) image -> float32 [K, 2] in pixels of a to_hw image (pixel i covers
    [i, i + 1), so the map is the plain scale)"""
    p = np.asarray(points, np.float64).reshape(-1, 2)
    return (p * np.array([to_hw[1] / from_hw[1], to_hw[0] / from_hw[0]], np.float64)).astype(np.float32)


def check_template(tpl) -> np.ndarray:
    """the template as float32 [K, 2]; refuses what the library refuses"""
    t = np.asarray(tpl, np.float32)
    if t.ndim != 2 or t.shape[1] != 2 or not MIN_POINTS <= t.shape[0] <= MAX_POINTS:
        raise ValueError(f"template must be [K, 2] with K in {MIN_POINTS}..{MAX_POINTS}, got {t.shape}")
    if not np.isfinite(t).all():
        raise ValueError("template value not finite")
    ux, uy, q = _template_terms(t)
    tvar = np.float64(0.0)
    for qx, qy in q:
        tvar = tvar + (qx * qx + qy * qy)
    if not tvar > 0.0:
        raise ValueError("the template has zero variance")
    return t


def _template_terms(t):
    K = len(t)
    sx = sy = np.float64(0.0)
    for i in range(K):
        sx, sy = sx + np.float64(t[i, 0]), sy + np.float64(t[i, 1])
    ux, uy = sx / np.float64(K), sy / np.float64(K)
    return ux, uy, [(np.float64(t[i, 0]) - ux, np.float64(t[i, 1]) - uy) for i in range(K)]


def reference_fit(rois, lmk, tpl, space: int = 0):
    """The statement: rois (roi.ROI_DTYPE [S]), lmk float32 [S, K, 2], tpl float32 [K, 2] -> (xforms XFORM_DTYPE [S], status int32 [S])"""
    rois = np.asarray(rois, R.ROI_DTYPE).reshape(-1)
    t = check_template(tpl)
    K = len(t)
    lmk = np.asarray(lmk, np.float32).reshape(len(rois), K, 2)
    assert space in (0, 1), space
    ux, uy, q = _template_terms(t)
    xf, status = empty_xforms(len(rois)), np.zeros(len(rois), np.int32)
    f64 = np.float64
    for s, rec in enumerate(rois):
        if int(rec["image"]) == -1:
            status[s] = EMPTY
            continue
        st = 0
        if space == 1 and not R.box_ok(rec["x0"], rec["y0"], rec["x1"], rec["y1"]):
            st |= BAD_BOX
        if not np.isfinite(lmk[s]).all():
            st |= BAD_LANDMARKS
        if st:
            status[s] = st
            continue
        with np.errstate(all="ignore"):
            if space == 1:
                x0, y0 = f64(rec["x0"]), f64(rec["y0"])
                bw, bh = f64(rec["x1"]) - x0, f64(rec["y1"]) - y0
                pts = [(x0 + f64(u) * bw, y0 + f64(v) * bh) for u, v in lmk[s]]
            else:
                pts = [(f64(u), f64(v)) for u, v in lmk[s]]
            sumx = sumy = f64(0.0)
            for sx, sy in pts:
                sumx, sumy = sumx + sx, sumy + sy
            mx, my = sumx / f64(K), sumy / f64(K)
            var = c = sn = f64(0.0)
            for (sx, sy), (qx, qy) in zip(pts, q):
                px, py = sx - mx, sy - my
                var = var + (px * px + py * py)
                c = c + (px * qx + py * qy)
                sn = sn + (px * qy - py * qx)
            ok = bool(var > 0.0)
            A, B = c / var, sn / var
            n = A * A + B * B
            ok = ok and bool(n > 0.0)
            a, b = A / n, -B / n
            m = np.array([a, -b, (mx - a * ux) + b * uy, b, a, (my - b * ux) - a * uy], f64)
        if not (ok and np.isfinite(m).all()):
            status[s] = BAD_LANDMARKS
            continue
        xf[s]["image"], xf[s]["m"] = rec["image"], m
    return xf, status


def warp_pil(img, m, oh: int, ow: int) -> np.ndarray:
    """Pillow's Image.transform((ow, oh), Image.AFFINE, m, resample=BILINEAR) of an HWC (or HW) uint8 image, restated: uint8
    [oh, ow, C] (the module docstring has the lines)"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    p = img.reshape(h, w, -1).astype(np.int64)
    m = np.asarray(m, np.float64).reshape(6)
    xin = np.arange(ow, dtype=np.float64)[None, :] + 0.5
    yin = np.arange(oh, dtype=np.float64)[:, None] + 0.5
    with np.errstate(all="ignore"):
        fx = (m[0] * xin + m[1] * yin) + m[2]
        fy = (m[3] * xin + m[4] * yin) + m[5]
        inside = (fx >= 0.0) & (fx < np.float64(w)) & (fy >= 0.0) & (fy < np.float64(h))
        fx, fy = np.where(inside, fx - 0.5, 0.0), np.where(inside, fy - 0.5, 0.0)
    X, Y = np.floor(fx), np.floor(fy)
    dx, dy = (fx - X)[..., None], (fy - Y)[..., None]
    X, Y = X.astype(np.int64), Y.astype(np.int64)
    xa, xb = np.clip(X, 0, w - 1), np.clip(X + 1, 0, w - 1)
    ya = np.clip(Y, 0, h - 1)
    below = Y + 1 < h
    yb = np.where(below, Y + 1, ya)
    a, b = p[ya, xa], p[ya, xb]
    v1 = a.astype(np.float64) + (b - a).astype(np.float64) * dx
    a, b = p[yb, xa], p[yb, xb]
    v2 = np.where(below[..., None], a.astype(np.float64) + (b - a).astype(np.float64) * dx, v1)
    res = v1 + (v2 - v1) * dy
    return np.where(inside[..., None], res.astype(np.int64), 0).astype(np.uint8)


def warp_status(xforms, srcs, pixel_bytes: int, pixels_bytes: int) -> np.ndarray:
    """tf2_roi_warp's validity rule per slot (TF2_ROI_* bits; 0: warped)"""
    xforms = np.asarray(xforms, XFORM_DTYPE).reshape(-1)
    srcs = np.asarray(srcs, P.SRC_DTYPE).reshape(-1)
    out = np.zeros(len(xforms), np.int32)
    for s, T in enumerate(xforms):
        i = int(T["image"])
        if i == -1:
            out[s] = EMPTY
            continue
        st = 0
        if not 0 <= i < len(srcs):
            st |= BAD_IMAGE
        elif P.record_status(srcs[i:i + 1], pixel_bytes, pixels_bytes, (1, 1))[0] & R._SRC_BITS:
            st |= BAD_SRC
        if not np.isfinite(T["m"]).all():
            st |= BAD_MATRIX
        out[s] = st
    return out


def reference_warp(pixels, srcs, xforms, out_hw, pixel_bytes: int, src_channel, mean, scale, out: str = "f32",
                   q0: Optional[int] = None):
    """The statement on the device's own inputs: pixels (uint8, 1-D), srcs (SRC_DTYPE [B]), xforms (XFORM_DTYPE [S]) -> (images,
    status).  images is float32 [S, 3, oh, ow] (out="f32"), or int8 quantised with 2^-q0 (out="q"); a slot with a status gives zeros."""
    assert out in ("q", "f32") and (out == "f32" or q0 is not None), (out, q0)
    pixels = np.asarray(pixels, np.uint8).reshape(-1)
    srcs = np.asarray(srcs, P.SRC_DTYPE).reshape(-1)
    xforms = np.asarray(xforms, XFORM_DTYPE).reshape(-1)
    oh, ow = out_hw
    status = warp_status(xforms, srcs, pixel_bytes, pixels.size)
    res = np.zeros((len(xforms), 3, oh, ow), np.float32)
    m32, s32 = np.asarray(mean, np.float32), np.asarray(scale, np.float32)
    images = {}
    for s, T in enumerate(xforms):
        if status[s]:
            continue
        i = int(T["image"])
        if i not in images:
            images[i] = P.source_image(pixels, srcs[i], pixel_bytes, src_channel)
        b = warp_pil(images[i], T["m"], oh, ow)
        res[s] = (np.moveaxis(b, 2, 0).astype(np.float32) - m32[:, None, None]) * s32[:, None, None]
    if out == "q":
        q = P.quant_input(res, P.trans_of(q0))
        q[status != 0] = 0
        return q, status
    return res, status


def xforms_to_device(xforms, device):
    """XFORM_DTYPE records -> the int32 [S, 14] device tensor the aligner reads"""
    import torch
    x = np.ascontiguousarray(np.asarray(xforms, XFORM_DTYPE).reshape(-1))
    return torch.from_numpy(x.view(np.int32).reshape(len(x), XFORM_WORDS).copy()).to(device)


def xforms_to_host(xforms) -> np.ndarray:
    """the int32 [S, 14] tensor of a fit -> XFORM_DTYPE records [S]"""
    a = xforms.cpu().numpy() if hasattr(xforms, "cpu") else np.asarray(xforms)
    return np.ascontiguousarray(a, np.int32).view(XFORM_DTYPE).reshape(-1)


class DeviceAligner:
    """tf2_roi_fit + tf2_roi_warp for the second network `net2` (a tf2_amd.network.NetWork) with `preset`'s means, scales and channel
    order (its resize and crop are not used: the transforms say what is resampled), on sources whose pixel bytes are the letters of
    src_order.  template: K points (x, y) in output pixels of net2's input (scaled_template rescales a published one); space: 0 for
    landmarks in source pixels, 1 for landmarks relative to the slot's box.
      fit(rois, lmk, stream=None, xforms=None, status=None) -> (xforms int32 [S, 14], status int32 [S])
      warp(pixels, srcs, xforms, out="q" | "f32", stream=None, images=None, status=None) -> (images [S, 3, h, w], status int32 [S])
      __call__(rois, lmk, pixels, srcs, out="q", stream=None, ...) -> (images, status, xforms, fit_status)
    rois: the int32 [S, 8] table of roi.DeviceCropper.select; lmk: float32 [S, K, 2]; pixels / srcs: the uint8 buffer and int32
    [B, 10] records of preprocess.pack; xforms: the table as int32 words (xforms_to_host / xforms_to_device convert to and from
    XFORM_DTYPE).  images: int8 (out="q", quantised with net2's 2^-Q0) or float32; a slot with a nonzero status is zeros.
    Everything is enqueued on `stream` (default: the current one), nothing synchronises or allocates beyond the outputs, which may
    be passed in (a captured graph then writes the same tensors at every replay)."""

    def __init__(self, net2, preset: P.Preset, template, src_order: str = "RGB", space: int = 0):
        from . import _lib
        if space not in (0, 1):
            raise ValueError(f"space must be 0 or 1, got {space}")
        self.net, self.preset, self.src_order, self.space = net2, preset, src_order, int(space)
        self.template = check_template(template)
        self.n_points = len(self.template)
        self.desc = P.desc_of(preset, src_order)
        self.out_hw = (int(net2._nd.image_h), int(net2._nd.image_w))
        d = _lib.RoiFitDesc()
        d.size = C.sizeof(_lib.RoiFitDesc)
        d.n_points, d.space = self.n_points, self.space
        for i, (x, y) in enumerate(self.template):
            d.tpl[i][0], d.tpl[i][1] = float(x), float(y)
        self.fit_desc = d

    def fit(self, rois, lmk, stream=None, xforms=None, status=None):
        import torch
        from . import _lib
        dev = _lib.expect(rois, torch.int32, cols=R.ROI_WORDS)
        S = rois.shape[0]
        _lib.expect(lmk, torch.float32, (S, self.n_points, 2), dev)
        stream = stream or torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            if xforms is None:
                xforms = torch.empty(S, XFORM_WORDS, dtype=torch.int32, device=dev)
            if status is None:
                status = torch.empty(S, dtype=torch.int32, device=dev)
            _lib.expect(xforms, torch.int32, (S, XFORM_WORDS), dev)
            _lib.expect(status, torch.int32, (S,), dev)
            _lib.check(_lib.lib().tf2_roi_fit(C.byref(self.fit_desc), rois.data_ptr(), lmk.data_ptr(), S, xforms.data_ptr(),
                                              status.data_ptr(), stream.cuda_stream))
        return xforms, status

    def warp(self, pixels, srcs, xforms, out: str = "q", stream=None, images=None, status=None):
        import torch
        from . import _lib
        assert out in ("q", "f32"), out
        dev = _lib.expect(pixels, torch.uint8)
        _lib.expect(srcs, torch.int32, device=dev, cols=P.SRC_WORDS)
        _lib.expect(xforms, torch.int32, device=dev, cols=XFORM_WORDS)
        B, S = srcs.shape[0], xforms.shape[0]
        with P.image_outputs(out, S, self.out_hw, dev, stream, images, status) as (images, status, stream):
            _lib.check(_lib.lib().tf2_roi_warp(self.net._h, C.byref(self.desc), pixels.data_ptr(), pixels.numel(), srcs.data_ptr(), B,
                                               xforms.data_ptr(), S, int(out == "q"), images.data_ptr(), status.data_ptr(),
                                               stream.cuda_stream))
        return images, status

    def __call__(self, rois, lmk, pixels, srcs, out: str = "q", stream=None, xforms=None, fit_status=None, images=None, status=None):
        xforms, fit_status = self.fit(rois, lmk, stream, xforms, fit_status)
        images, status = self.warp(pixels, srcs, xforms, out, stream, images, status)
        return images, status, xforms, fit_status

    def reference_fit(self, rois, lmk):
        """reference_fit on host copies of the tensors, with this aligner's template and space"""
        r = rois if isinstance(rois, np.ndarray) and rois.dtype == R.ROI_DTYPE else R.rois_to_host(rois)
        l = lmk.cpu().numpy() if hasattr(lmk, "cpu") else np.asarray(lmk)
        return reference_fit(r, l, self.template, self.space)

    def reference_warp(self, pixels, srcs, xforms, out: str = "q"):
        """reference_warp on host copies of the tensors, with net2's Q0 for out="q" """
        p = pixels.cpu().numpy() if hasattr(pixels, "cpu") else np.asarray(pixels)
        x = xforms if isinstance(xforms, np.ndarray) and xforms.dtype == XFORM_DTYPE else xforms_to_host(xforms)
        return reference_warp(p, R._srcs_host(srcs), x, self.out_hw, len(self.src_order), P.src_channels(self.preset, self.src_order),
                              np.float32(self.preset.mean), np.float32(self.preset.scale), out,
                              int(self.net.q[0, 0]) if out == "q" else None)

    def reference(self, rois, lmk, pixels, srcs, out: str = "q"):
        """The statement of __call__ on host copies of the same inputs: (images, status, xforms XFORM_DTYPE, fit_status)"""
        xforms, fit_status = self.reference_fit(rois, lmk)
        images, status = self.reference_warp(pixels, srcs, xforms, out)
        return images, status, xforms, fit_status
