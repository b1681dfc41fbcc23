"""JPEG files on the device (tf2_jpeg_parse, tf2_jpeg_entropy, tf2_jpeg_idct, include/tf2_amd.h; csrc/jpeg_entropy.cpp,
csrc/jpeg_idct.hip): a baseline JPEG file in, the planes libjpeg's decoder reconstructs out -- written where the tf2_ycc_src records
of tf2_ycc_to_rgb point, so that file -> coefficients -> planes -> RGB -> resize -> network -> labels is one chain on the device
behind a host step that only parses headers and decodes Huffman codes.

The arithmetic is stated whole in include/tf2_amd.h.  Here `reference_idct` is its numpy statement (uint32 arithmetic, so it wraps
as the header says), `reference_entropy` an independent pure-Python decoder of the scan (a bitwise walk of the canonical codes: for
small files only), `record_status` the device's validity rule and `reference` the whole device call on its own inputs, statuses
included; the device is bit-identical to it.  With the upsampling rule a file's Info names (`Info.upsample`: libjpeg replicates
chroma planes at most 2 samples wide and filters wider ones) and the JFIF matrix, `ycc.to_rgb` of the upsampled planes is
Pillow's `Image.open(file).convert("RGB")` byte for byte: tests/golden/pil_jpeg.npz holds Pillow's own bytes
(tools/gen_jpeg_golden.py).

`parse` / `entropy` / `decode_host` are the host step, `pack` builds the device inputs (or refills buffers a captured graph
reads), `DeviceDecoder(desc).run(...)` is the device call.  A batch shares one desc: group files by `group_key`."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import preprocess as P
from . import ycc as Y

# tf2_jpeg_src, byte for byte (48 bytes)
JPEG_DTYPE = np.dtype([("block_off", "<i8", (3,)), ("bw", "<i4", (3,)), ("bh", "<i4", (3,))])
JPEG_WORDS = JPEG_DTYPE.itemsize // 4

TILE_BW, TILE_BH = 8, 4                                          # TF2_JPEG_TILE_BW / _BH: the kernel's tile, in coefficient blocks
MAX_BLOCKS_PER_IMAGE = 64
MAX_SIDE = P.MAX_SIDE
# tf2_jpeg_info.status / tf2_jpeg_entropy's status
(UNSUPPORTED_PROGRESSIVE, UNSUPPORTED_ARITHMETIC, UNSUPPORTED_PRECISION, UNSUPPORTED_COMPONENTS, UNSUPPORTED_SAMPLING,
 UNSUPPORTED_SCANS, UNSUPPORTED_COLORSPACE, BAD_HEADER, TRUNCATED, BAD_CODE) = (1 << i for i in range(10))
UNSUPPORTED = 127
# TF2_JPEG_REC_*: status bits of an image the device left alone
REC_BAD_SIZE, REC_BAD_GRID, REC_BAD_PITCH, REC_BAD_OFFSET, REC_OUT_OF_COEF, REC_OUT_OF_PLANES = 1, 2, 4, 8, 16, 32

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])                         # natural index of the k-th coefficient of the zigzag sequence


def default_blocks_per_image(batch: int) -> int:
    """what blocks_per_image = 0 stands for (csrc/jpeg_idct.h): about 2048 blocks a launch, 1..64 an image"""
    return max(1, min(MAX_BLOCKS_PER_IMAGE, 2048 // max(int(batch), 1)))


@dataclass(frozen=True)
class Desc:
    """tf2_jpeg_desc: layout (ycc.PLANAR: three components, ycc.GRAY: one), (sub_x, sub_y) and the grid"""
    layout: int = Y.PLANAR
    sub: Tuple[int, int] = (2, 2)
    blocks_per_image: int = 0

    def c(self):
        from . import _lib
        d = _lib.JpegDesc()
        d.size = C.sizeof(_lib.JpegDesc)
        d.layout, d.sub_x, d.sub_y, d.blocks_per_image = self.layout, self.sub[0], self.sub[1], self.blocks_per_image
        return d

    @property
    def eff_sub(self) -> Tuple[int, int]:
        return (1, 1) if self.layout == Y.GRAY else tuple(self.sub)

    @property
    def components(self) -> int:
        return 1 if self.layout == Y.GRAY else 3


@dataclass(frozen=True, eq=False)
class Info:
    """tf2_jpeg_info as Python values; `key()` is everything a decoder depends on (not where in the file the scan starts)"""
    status: int
    h: int
    w: int
    components: int
    sub: Tuple[int, int]
    restart_interval: int
    upsample: int
    bw: Tuple[int, ...]
    bh: Tuple[int, ...]
    ph: Tuple[int, ...]
    pw: Tuple[int, ...]
    total_blocks: int
    scan_offset: int
    quant: np.ndarray                                            # uint16 [3, 64], natural order
    raw: object                                                  # the _lib.JpegInfo the library filled

    def key(self):
        return (self.status, self.h, self.w, self.components, self.sub, self.restart_interval, self.upsample, self.bw, self.bh,
                self.ph, self.pw, self.total_blocks, self.quant.tobytes())


def _bytes(data) -> np.ndarray:
    return np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8).reshape(-1)


def parse(data) -> Info:
    """tf2_jpeg_parse of a file's bytes.  info.status != 0: the file is not one this decoder takes (UNSUPPORTED_* / BAD_HEADER)."""
    from . import _lib
    buf = _bytes(data)
    raw = _lib.JpegInfo()
    rc = _lib.lib().tf2_jpeg_parse(buf.ctypes.data, buf.size, C.byref(raw))
    if rc != 0:                                                  # (the host calls set no tf2_last_error: the message is made here)
        raise _lib.Tf2Error(rc, "tf2_jpeg_parse: null argument")
    n = raw.components if raw.status == 0 else 0
    return Info(raw.status, raw.h, raw.w, raw.components, (raw.sub_x, raw.sub_y), raw.restart_interval, raw.upsample,
                tuple(raw.bw[:n]), tuple(raw.bh[:n]), tuple(raw.ph[:n]), tuple(raw.pw[:n]), raw.total_blocks, raw.scan_offset,
                np.ctypeslib.as_array(raw.quant).astype(np.uint16).reshape(3, 64), raw)


def make_info(h: int, w: int, layout: int, sub, quant) -> Info:
    """The Info of an h x w image that exists as coefficients only (tests and tools): the grids, the planes and the upsampling rule
    as tf2_jpeg_parse derives them; quant: uint16 [64] (every component's) or [>= components, 64]"""
    n = 1 if layout == Y.GRAY else 3
    sx, sy = (1, 1) if n == 1 else tuple(sub)
    mw, mh = -(-w // (8 * sx)), -(-h // (8 * sy))
    ch, cw = Y.chroma_size(h, w, (sx, sy))
    bw, bh = ((mw * sx, mw, mw), (mh * sy, mh, mh)) if n == 3 else ((mw,), (mh,))
    q = np.zeros((3, 64), np.uint16)
    quant = np.asarray(quant, np.uint16).reshape(-1, 64)
    q[:n] = quant[:n] if len(quant) > 1 else quant
    return Info(0, h, w, n, (sx, sy), 0, Y.REPLICATE if n == 3 and sx > 1 and cw <= 2 else Y.FANCY, bw, bh, (h, ch, ch)[:n],
                (w, cw, cw)[:n], sum(a * b for a, b in zip(bw, bh)), 0, q, None)


def entropy(data, info: Info, out: Optional[np.ndarray] = None):
    """tf2_jpeg_entropy: (coef int16 [info.total_blocks, 64] in natural order, status).  out: an int16 array of at least that many
    blocks to decode into (its first total_blocks blocks are returned as a view)."""
    from . import _lib
    assert info.status == 0, f"the file is not decodable (status {info.status})"
    assert info.raw is not None, "an Info of `parse` is needed (make_info describes coefficients that have no file)"
    buf = _bytes(data)
    if out is None:
        out = np.empty((info.total_blocks, 64), np.int16)
    assert out.dtype == np.int16 and out.flags.c_contiguous and out.size >= info.total_blocks * 64, "out: int16, contiguous, large enough"
    st = C.c_int32(0)
    rc = _lib.lib().tf2_jpeg_entropy(buf.ctypes.data, buf.size, C.byref(info.raw), out.ctypes.data, out.size // 64, C.byref(st))
    if rc != 0:
        raise _lib.Tf2Error(rc, "tf2_jpeg_entropy: " + ("fewer than info.total_blocks blocks of room" if rc == -3 else
                                                        "null argument, or an info whose status is not 0"))
    return out.reshape(-1)[:info.total_blocks * 64].reshape(info.total_blocks, 64), st.value


def group_key(info: Info):
    """(layout, sub, upsample): the files of one tf2_jpeg_idct / tf2_ycc_to_rgb batch share it"""
    return (Y.GRAY if info.components == 1 else Y.PLANAR, tuple(info.sub), info.upsample)


def decode_host(files, threads: int = 16):
    """[(info, coef or None, status)] of a list of files' bytes, parsed and entropy-decoded on `threads` threads (the library
    calls release the GIL).  A file the parser refuses has coef None and the parser's status."""
    def one(data):
        info = parse(data)
        if info.status:
            return info, None, info.status
        coef, st = entropy(data, info)
        return info, coef, st
    files = list(files)
    if threads <= 1 or len(files) <= 1:
        return [one(f) for f in files]
    with ThreadPoolExecutor(max_workers=int(threads)) as pool:
        return list(pool.map(one, files))


# ---------------------------------------------------------------- the statements

def reference_entropy(data):
    """An independent decoder of a baseline file, in Python integers: (dict of h, w, components, sub, restart_interval, bw, bh,
    quant uint16 [components, 64] natural order; coef int16 [total blocks, 64] natural order, component after component in raster
    order).  Codes are walked bit by bit through the canonical code list.  Raises ValueError on anything it does not take."""
    d = bytes(data)
    if d[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    pos, qt, huff, frame, dri = 2, {}, {}, None, 0
    while True:
        if d[pos] != 0xFF:
            raise ValueError("marker expected")
        while d[pos] == 0xFF:
            pos += 1
        m = d[pos]
        pos += 1
        ln = (d[pos] << 8) | d[pos + 1]
        seg = d[pos + 2:pos + ln]
        pos += ln
        if m == 0xDB:
            at = 0
            while at < len(seg):
                pq, tq = seg[at] >> 4, seg[at] & 15
                at += 1
                vals = [((seg[at + 2 * k] << 8) | seg[at + 2 * k + 1]) if pq else seg[at + k] for k in range(64)]
                at += 64 * (pq + 1)
                nat = [0] * 64
                for k in range(64):
                    nat[int(ZIGZAG[k])] = vals[k]
                qt[tq] = nat
        elif m == 0xC4:
            at = 0
            while at < len(seg):
                tc_th = seg[at]
                counts = list(seg[at + 1:at + 17])
                n = sum(counts)
                syms = list(seg[at + 17:at + 17 + n])
                at += 17 + n
                codes, code, k = {}, 0, 0
                for ln_ in range(1, 17):
                    for _ in range(counts[ln_ - 1]):
                        codes[(ln_, code)] = syms[k]
                        code, k = code + 1, k + 1
                    code <<= 1
                huff[tc_th] = codes
        elif m in (0xC0, 0xC1):
            if seg[0] != 8:
                raise ValueError("precision")
            h, w, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            frame = (h, w, [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nc)])
        elif 0xC2 <= m <= 0xCF and m not in (0xC8,):
            raise ValueError("not a baseline file")
        elif m == 0xDD:
            dri = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            if frame is None or seg[0] != len(frame[2]):
                raise ValueError("scan")
            tabs = [(seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(seg[0])]
            break
    h, w, comps = frame
    nc = len(comps)
    if nc == 1:
        hs = [1]
        vs = [1]
        mcus_x, mcus_y = -(-w // 8), -(-h // 8)
    else:
        hs, vs = [c[1] for c in comps], [c[2] for c in comps]
        mcus_x, mcus_y = -(-w // (8 * max(hs))), -(-h // (8 * max(vs)))
    bw, bh = [mcus_x * v for v in hs], [mcus_y * v for v in vs]
    base = [sum(bw[i] * bh[i] for i in range(c)) for c in range(nc)]
    coef = np.zeros((sum(a * b for a, b in zip(bw, bh)), 64), np.int64)

    # the scan's bits: bytes with stuffing removed, cut at markers
    state = {"pos": pos, "acc": 0, "n": 0}

    def bit():
        if state["n"] == 0:
            b = d[state["pos"]]
            if b == 0xFF:
                if d[state["pos"] + 1] != 0:
                    raise ValueError("marker inside the data")
                state["pos"] += 2
            else:
                state["pos"] += 1
            state["acc"], state["n"] = b, 8
        state["n"] -= 1
        return (state["acc"] >> state["n"]) & 1

    def sym(table):
        code = 0
        for ln_ in range(1, 17):
            code = (code << 1) | bit()
            if (ln_, code) in table:
                return table[(ln_, code)]
        raise ValueError("bad code")

    def value(s):
        v = 0
        for _ in range(s):
            v = (v << 1) | bit()
        return v if v >= (1 << (s - 1)) else v - (1 << s) + 1

    pred, left, rst = [0] * nc, dri, 0
    for r in range(mcus_y):
        for q in range(mcus_x):
            if dri and left == 0:
                state["n"] = 0
                while d[state["pos"]] == 0xFF and d[state["pos"] + 1] == 0xFF:
                    state["pos"] += 1
                if d[state["pos"]] != 0xFF or d[state["pos"] + 1] != 0xD0 + rst:
                    raise ValueError("restart marker")
                state["pos"] += 2
                rst, left, pred = (rst + 1) & 7, dri, [0] * nc
            for c in range(nc):
                dc, ac = huff[tabs[c][0]], huff[0x10 | tabs[c][1]]
                for y in range(vs[c]):
                    for x in range(hs[c]):
                        blk = coef[base[c] + (r * vs[c] + y) * bw[c] + q * hs[c] + x]
                        s = sym(dc)
                        if s:
                            pred[c] += value(s)
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = sym(ac)
                            run, s = rs >> 4, rs & 15
                            if s == 0:
                                if run != 15:
                                    break
                                k += 16
                                continue
                            k += run
                            blk[int(ZIGZAG[k])] = value(s)
                            k += 1
            left -= 1
    head = dict(h=h, w=w, components=nc, sub=(max(hs), max(vs)) if nc > 1 else (1, 1), restart_interval=dri, bw=tuple(bw), bh=tuple(bh),
                quant=np.array([qt[c[3]] for c in comps], np.uint16))
    return head, coef.astype(np.int16)


def _sar(v, s):
    return (v.view(np.int32) >> s).view(np.uint32)


def _idct8(x, s):
    """K(x0..x7; s) along the last axis of a uint32 array [..., 8]"""
    u = np.uint32
    x0, x1, x2, x3, x4, x5, x6, x7 = (x[..., i] for i in range(8))
    z1 = (x2 + x6) * u(4433)
    t2, t3 = z1 - x6 * u(15137), z1 + x2 * u(6270)
    t0, t1 = (x0 + x4) << u(13), (x0 - x4) << u(13)
    a0, a3, a1, a2 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    b0, b1, b2, b3 = x7, x5, x3, x1
    z1, z2, z3, z4 = b0 + b3, b1 + b2, b0 + b2, b1 + b3
    z5 = (z3 + z4) * u(9633)
    b0, b1, b2, b3 = b0 * u(2446), b1 * u(16819), b2 * u(25172), b3 * u(12299)
    neg = lambda v: u((1 << 32) - v)
    z1, z2 = z1 * neg(7373), z2 * neg(20995)
    z3, z4 = z3 * neg(16069) + z5, z4 * neg(3196) + z5
    b0, b1, b2, b3 = b0 + z1 + z3, b1 + z2 + z4, b2 + z2 + z3, b3 + z1 + z4
    half = u(1 << (s - 1))
    return np.stack([_sar(o + half, s) for o in (a0 + b3, a1 + b2, a2 + b1, a3 + b0, a3 - b0, a2 - b1, a1 - b2, a0 - b3)], axis=-1)


def reference_idct(coef, q) -> np.ndarray:
    """uint8 [n, 8, 8] samples of n blocks: coef int16 [n, 64] (natural order), q uint16 [64] or [n, 64].  32-bit arithmetic that
    wraps, as include/tf2_amd.h states it."""
    with np.errstate(over="ignore"):
        c = np.asarray(coef, np.int16).reshape(-1, 8, 8).astype(np.int32).view(np.uint32)
        qq = np.asarray(q, np.uint16).astype(np.uint32)
        d = c * (qq.reshape(8, 8) if qq.size == 64 else qq.reshape(-1, 8, 8))
        ws = _idct8(d.transpose(0, 2, 1), 11).transpose(0, 2, 1)  # pass 1: down each column
        out = _idct8(np.ascontiguousarray(ws), 18).view(np.int32)  # pass 2: along each row
        return np.clip(out.astype(np.int64) + 128, 0, 255).astype(np.uint8)


def plane_of(samples, bw: int, bh: int, ph: int, pw: int) -> np.ndarray:
    """the ph x pw plane of a component's bw * bh blocks of samples [bw * bh, 8, 8] in raster order"""
    s = np.asarray(samples).reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
    return np.ascontiguousarray(s[:ph, :pw])


def planes_of_file(info, coef):
    """[Y] or [Y, Cb, Cr]: the planes of a decoded file (Info or reference_entropy's dict, its coefficients)"""
    g = (lambda k: info[k]) if isinstance(info, dict) else (lambda k: getattr(info, k))
    n, (sx, sy), h, w = g("components"), g("sub"), g("h"), g("w")
    out, at = [], 0
    for c in range(n):
        bw, bh = g("bw")[c], g("bh")[c]
        ph, pw = (h, w) if c == 0 else Y.chroma_size(h, w, (sx, sy))
        out.append(plane_of(reference_idct(coef[at:at + bw * bh], g("quant")[c]), bw, bh, ph, pw))
        at += bw * bh
    return out


def rgb_of_file(info: Info, coef) -> np.ndarray:
    """uint8 [h, w, 3]: what Pillow's convert('RGB') makes of the file -- reference_idct, the file's own upsampling rule, JFIF"""
    pl = planes_of_file(info, coef)
    if len(pl) == 1:
        return np.repeat(pl[0][:, :, None], 3, axis=2)
    up = [Y.upsample(p, info.sub, info.h, info.w, info.upsample) for p in pl[1:]]
    return Y.to_rgb(pl[0], up[0], up[1], Y.JFIF)


def record_status(jrec, yrec, srec, desc: Desc, coef_blocks: int, planes_bytes: int) -> np.ndarray:
    """The device's validity rule per image (TF2_JPEG_REC_* bits; 0: reconstructed) -- a statement in Python integers"""
    jrec = np.asarray(jrec, JPEG_DTYPE).reshape(-1)
    yrec = np.asarray(yrec, Y.YCC_DTYPE).reshape(-1)
    srec = np.asarray(srec, P.SRC_DTYPE).reshape(-1)
    assert len(jrec) == len(yrec) == len(srec)
    nc = desc.components
    sx, sy = desc.eff_sub
    out = np.zeros(len(srec), np.int32)
    for i, (j, p, r) in enumerate(zip(jrec, yrec, srec)):
        h, w = int(r["h"]), int(r["w"])
        cw, ch = (w + sx - 1) >> (sx - 1), (h + sy - 1) >> (sy - 1)
        size = [(h, w), (ch, cw), (ch, cw)][:nc]
        offs = [int(p["off_y"]), int(p["off_cb"]), int(p["off_cr"])][:nc]
        pitch = [int(p["pitch_y"]), int(p["pitch_c"]), int(p["pitch_c"])][:nc]
        st = 0
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            st |= REC_BAD_SIZE
        for c in range(nc):
            bw, bh = int(j["bw"][c]), int(j["bh"][c])
            if bw < 1 or bh < 1 or 8 * bw < size[c][1] or 8 * bh < size[c][0]:
                st |= REC_BAD_GRID
            if int(j["block_off"][c]) < 0 or offs[c] < 0:
                st |= REC_BAD_OFFSET
            if pitch[c] < size[c][1]:
                st |= REC_BAD_PITCH
        if st == 0:
            for c in range(nc):
                if int(j["block_off"][c]) + int(j["bw"][c]) * int(j["bh"][c]) > coef_blocks:
                    st |= REC_OUT_OF_COEF
                if offs[c] + (size[c][0] - 1) * pitch[c] + size[c][1] > planes_bytes:
                    st |= REC_OUT_OF_PLANES
        out[i] = st
    return out


def reference(coef, jrec, quant, yrec, srec, desc: Desc, planes):
    """The statement of the whole call on the device's own inputs: coef (int16 [n, 64]), jrec (JPEG_DTYPE), quant (uint16 [B, 3, 64]),
    yrec (ycc.YCC_DTYPE), srec (preprocess.SRC_DTYPE) and the plane buffer as it is before the call (uint8 1-D, or its size for
    zeros) -> (planes after the call, status int32 [B]).  Only the ph x pw samples of the planes of images with status 0 change."""
    coef = np.asarray(coef, np.int16).reshape(-1, 64)
    jrec = np.asarray(jrec, JPEG_DTYPE).reshape(-1)
    yrec = np.asarray(yrec, Y.YCC_DTYPE).reshape(-1)
    srec = np.asarray(srec, P.SRC_DTYPE).reshape(-1)
    quant = np.asarray(quant, np.uint16).reshape(len(srec), 3, 64)
    out = np.zeros(int(planes), np.uint8) if np.isscalar(planes) else np.array(planes, np.uint8).reshape(-1)
    status = record_status(jrec, yrec, srec, desc, len(coef), out.size)
    for b, (j, p, r) in enumerate(zip(jrec, yrec, srec)):
        if status[b]:
            continue
        h, w = int(r["h"]), int(r["w"])
        ch, cw = Y.chroma_size(h, w, desc.eff_sub)
        for c in range(desc.components):
            ph, pw = (h, w) if c == 0 else (ch, cw)
            off = int(p[("off_y", "off_cb", "off_cr")[c]])
            pitch = int(p["pitch_c" if c else "pitch_y"])
            bw, nby, nbx = int(j["bw"][c]), -(-ph // 8), -(-pw // 8)
            first = int(j["block_off"][c])
            idx = (first + np.arange(nby)[:, None] * bw + np.arange(nbx)[None, :]).reshape(-1)
            plane = plane_of(reference_idct(coef[idx], quant[b, c]), nbx, nby, ph, pw)
            for y in range(ph):
                out[off + y * pitch: off + y * pitch + pw] = plane[y]
    return out, status


# ---------------------------------------------------------------- device inputs

def pack_host(items, layout: int, sub, pixel_bytes: int = 3, preset: Optional[P.Preset] = None, align: int = 4):
    """(coef int16 [n, 64], jrec JPEG_DTYPE [B], quant uint16 [B, 3, 64], yrec YCC_DTYPE [B], srec SRC_DTYPE [B], planes_bytes,
    pixels_bytes) of a list of (Info, coef) -- or of files' bytes, decoded here.  The coefficient blocks lie back to back, the
    planes and the destination images exactly as ycc.pack_ycc_host lays them out."""
    sub = (1, 1) if layout == Y.GRAY else tuple(sub)
    decoded = []
    for it in items:
        if isinstance(it, (bytes, bytearray, memoryview)):
            info = parse(it)
            assert info.status == 0, f"status {info.status}"
            it = (info, entropy(it, info)[0])
        decoded.append((it[0], it[1]))
    B = len(decoded)
    assert B, "no files"
    frames = []
    for info, _ in decoded:
        assert group_key(info)[:2] == (layout, sub), f"a file of group {group_key(info)} in a batch of {(layout, sub)}"
        frames.append(tuple(np.zeros((info.ph[c], info.pw[c]), np.uint8) for c in range(info.components)))
    src, yrec, srec, need = Y.pack_ycc_host(frames, layout, sub, pixel_bytes, preset, align)
    jrec, quant = np.zeros(B, JPEG_DTYPE), np.ones((B, 3, 64), np.uint16)
    at = 0
    for i, (info, coef) in enumerate(decoded):
        for c in range(info.components):
            jrec[i]["block_off"][c], jrec[i]["bw"][c], jrec[i]["bh"][c] = at, info.bw[c], info.bh[c]
            at += info.bw[c] * info.bh[c]
        quant[i] = info.quant
    coef = np.concatenate([np.asarray(c, np.int16).reshape(-1, 64) for _, c in decoded])
    assert len(coef) == at
    return coef, jrec, quant, yrec, srec, int(src.size), need


def pack(items, layout: int, sub, device, pixel_bytes: int = 3, preset: Optional[P.Preset] = None, align: int = 4,
         coef=None, jpeg=None, quant=None, planes=None, ycc=None, srcs=None, pixels=None):
    """The device inputs of tf2_jpeg_idct and of the tf2_ycc_to_rgb behind it, from `pack_host`: (coef int16 [n, 64], jpeg int32
    [B, 12], quant uint16 [B, 3, 64], planes uint8, ycc int32 [B, 8], srcs int32 [B, 10], pixels uint8) tensors.  With coef= .. pixels=
    the caller's tensors are filled instead (a captured graph reads the same buffers at every replay): the blocks go to the front of
    `coef`, the records fill the tables, `planes` and `pixels` only have to be large enough."""
    import torch
    hc, jrec, hq, yrec, srec, pbytes, need = pack_host(items, layout, sub, pixel_bytes, preset, align)

    def table(t, host, what):
        host = torch.from_numpy(np.ascontiguousarray(host))
        if t is None:
            return host.to(device)
        assert t.dtype == host.dtype and tuple(t.shape) == tuple(host.shape), f"{what} must be {host.dtype} {tuple(host.shape)}"
        t.copy_(host)
        return t

    def room(t, n, what):
        if t is None:
            return torch.zeros(n, dtype=torch.uint8, device=device)
        assert t.dtype == torch.uint8 and t.numel() >= n, f"{what} too small"
        return t
    if coef is None:
        coef = torch.from_numpy(hc).to(device)
    else:
        assert coef.dtype == torch.int16 and coef.dim() == 2 and coef.shape[1] == 64 and coef.shape[0] >= len(hc), "coefficient buffer too small"
        coef[:len(hc)].copy_(torch.from_numpy(hc))
    jpeg = table(jpeg, Y.records_to_words(jrec, JPEG_WORDS), "jpeg")
    quant = table(quant, hq.view(np.int16), "quant").view(torch.int16)
    ycc = table(ycc, Y.records_to_words(yrec, Y.YCC_WORDS), "ycc")
    srcs = table(srcs, Y.records_to_words(srec, P.SRC_WORDS), "srcs")
    return coef, jpeg, quant, room(planes, pbytes, "plane buffer"), ycc, srcs, room(pixels, need, "pixel buffer")


class DeviceDecoder:
    """tf2_jpeg_idct with `desc` (a Desc).
      run(coef, jpeg, quant, planes, ycc, srcs, stream=None, status=None) -> status
    coef: int16 [n, 64] device tensor of coefficient blocks, jpeg: int32 [B, 12] (tf2_jpeg_src records), quant: int16 [B, 3, 64] (the
    uint16 quantisers' bits), planes: the uint8 device tensor the planes are written into, ycc: int32 [B, 8] (tf2_ycc_src), srcs:
    int32 [B, 10] (tf2_image_src) -- `pack` makes all six, and ycc.DeviceConverter reads planes / ycc / srcs next.  status: int32 [B],
    0 or the TF2_JPEG_REC_* bits of an image that was left alone.  Enqueued on `stream` (default: the current one); nothing
    synchronises or allocates beyond the status, which may be passed in."""

    def __init__(self, desc: Desc = Desc()):
        self.desc = desc
        self._c = desc.c()

    def run(self, coef, jpeg, quant, planes, ycc, srcs, stream=None, status=None):
        import torch
        from . import _lib
        dev = coef.device
        assert coef.dtype == torch.int16 and coef.is_contiguous() and dev.type == "cuda" and coef.dim() == 2 and coef.shape[1] == 64
        assert planes.dtype == torch.uint8 and planes.is_contiguous() and planes.device == dev
        assert srcs.dtype == torch.int32 and srcs.is_contiguous() and srcs.device == dev and srcs.dim() == 2 and srcs.shape[1] == P.SRC_WORDS
        B = srcs.shape[0]
        assert ycc.dtype == torch.int32 and ycc.is_contiguous() and ycc.device == dev and tuple(ycc.shape) == (B, Y.YCC_WORDS)
        assert jpeg.dtype == torch.int32 and jpeg.is_contiguous() and jpeg.device == dev and tuple(jpeg.shape) == (B, JPEG_WORDS)
        assert quant.dtype == torch.int16 and quant.is_contiguous() and quant.device == dev and tuple(quant.shape) == (B, 3, 64)
        stream = stream or torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            if status is None:
                status = torch.empty(B, dtype=torch.int32, device=dev)
            assert status.dtype == torch.int32 and status.is_contiguous() and status.device == dev and tuple(status.shape) == (B,)
            _lib.check(_lib.lib().tf2_jpeg_idct(C.byref(self._c), coef.data_ptr(), coef.shape[0], jpeg.data_ptr(), quant.data_ptr(),
                                                planes.data_ptr(), planes.numel(), ycc.data_ptr(), srcs.data_ptr(), B,
                                                status.data_ptr(), stream.cuda_stream))
        return status

    def reference(self, coef, jpeg, quant, planes, ycc, srcs):
        """`reference` on host copies of the tensors (planes: the buffer as it is before the call)"""
        host = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
        jr = np.ascontiguousarray(host(jpeg), np.int32).view(JPEG_DTYPE).reshape(-1)
        yr = np.ascontiguousarray(host(ycc), np.int32).view(Y.YCC_DTYPE).reshape(-1)
        sr = np.ascontiguousarray(host(srcs), np.int32).view(P.SRC_DTYPE).reshape(-1)
        return reference(host(coef), jr, host(quant).view(np.uint16), yr, sr, self.desc, host(planes))
