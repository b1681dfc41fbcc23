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
reads), `DeviceDecoder(desc).run(...)` is the device call.  A batch shares one desc: group files by `group_key`.

The entropy decoding can run on the device as well (tf2_jpeg_huff, csrc/jpeg_huff.hip; the section at the end of this file):
`scan_record` is the host fill call, `pack_bytes` builds the device inputs from files' bytes, `DeviceEntropy(desc).run(...)` is the
device call and `reference_huff` the statement of its parallel algorithm -- subsequences, tolerant rounds, strict pass."""
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
        dev = _lib.expect(coef, torch.int16, cols=64)
        _lib.expect(planes, torch.uint8, device=dev)
        _lib.expect(srcs, torch.int32, device=dev, cols=P.SRC_WORDS)
        B = srcs.shape[0]
        _lib.expect(ycc, torch.int32, (B, Y.YCC_WORDS), dev)
        _lib.expect(jpeg, torch.int32, (B, JPEG_WORDS), dev)
        _lib.expect(quant, torch.int16, (B, 3, 64), dev)
        stream = stream or torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            if status is None:
                status = torch.empty(B, dtype=torch.int32, device=dev)
            _lib.expect(status, torch.int32, (B,), dev)
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


# ---------------------------------------------------------------- entropy decoding on the device (tf2_jpeg_huff, csrc/jpeg_huff.hip)

# tf2_jpeg_scan, byte for byte (1664 bytes)
SCAN_DTYPE = np.dtype([("byte_off", "<i8"), ("byte_len", "<i8"), ("components", "<i4"), ("sub_x", "<i4"), ("sub_y", "<i4"),
                       ("restart_interval", "<i4"),
                       ("tab", [("dc_counts", "u1", (16,)), ("dc_vals", "u1", (256,)), ("ac_counts", "u1", (16,)), ("ac_vals", "u1", (256,))], (3,))])
SCAN_WORDS = SCAN_DTYPE.itemsize // 4
HUFF_LANES = 1024                                                # TF2_JPEG_HUFF_LANES: threads of a workgroup
HUFF_DEFAULT_SUBSEQ = 64
HUFF_MAX_BYTES = 1 << 28
HUFF_WORK_HEADER = 16
REC_BAD_RANGE, REC_BAD_SCAN, REC_BAD_TABLE, REC_WORK_TOO_SMALL = 1024, 2048, 4096, 8192
_STOPPED = 1 << 16
_M64 = (1 << 64) - 1


@dataclass(frozen=True)
class HuffDesc:
    """tf2_jpeg_huff_desc: layout (ycc.PLANAR: three components, ycc.GRAY: one), (sub_x, sub_y), subseq_bytes (0: the default)"""
    layout: int = Y.PLANAR
    sub: Tuple[int, int] = (2, 2)
    subseq_bytes: int = 0

    def c(self):
        from . import _lib
        d = _lib.JpegHuffDesc()
        d.size = C.sizeof(_lib.JpegHuffDesc)
        d.layout, d.sub_x, d.sub_y, d.subseq_bytes = self.layout, self.sub[0], self.sub[1], self.subseq_bytes
        return d

    @property
    def eff_sub(self) -> Tuple[int, int]:
        return (1, 1) if self.layout == Y.GRAY else tuple(self.sub)

    @property
    def components(self) -> int:
        return 1 if self.layout == Y.GRAY else 3

    @property
    def subseq(self) -> int:
        return self.subseq_bytes or HUFF_DEFAULT_SUBSEQ


def huff_chunk_lanes(subseq_bytes: int) -> int:
    """subsequences of a chunk (csrc/jpeg_huff.h): 256, 512, 1024, 512, 256 for 16 .. 256 bytes a subsequence"""
    return min(HUFF_LANES, 65536 // subseq_bytes, 16 * subseq_bytes)


def huff_work_bytes(desc: HuffDesc, batch: int, max_scan_bytes: int) -> int:
    """tf2_jpeg_huff_work_bytes: 16 + 8 bytes a subsequence, per image"""
    return int(batch) * (HUFF_WORK_HEADER + 8 * max(1, -(-int(max_scan_bytes) // desc.subseq)))


def scan_record(data, info: Info, byte_off: int) -> np.ndarray:
    """tf2_jpeg_scan_fill: the SCAN_DTYPE record (shape ()) of a file whose entropy-coded bytes, data[info.scan_offset:], lie at
    byte_off of the batch's byte buffer"""
    from . import _lib
    assert info.raw is not None, "an Info of `parse` is needed"
    buf = _bytes(data)
    raw = _lib.JpegScan()
    rc = _lib.lib().tf2_jpeg_scan_fill(buf.ctypes.data, buf.size, C.byref(info.raw), int(byte_off), C.byref(raw))
    if rc != 0:
        raise _lib.Tf2Error(rc, "tf2_jpeg_scan_fill: null argument, an info whose status is not 0, or headers that do not parse to it")
    return np.frombuffer(bytes(raw), SCAN_DTYPE)[0].copy()


def _huff_table(counts, vals):
    """(look [512], maxcode [17], valoff [17], vals [256]) of a canonical code, or None: build_huff's test"""
    counts = [int(v) for v in counts]
    if sum(counts) > 256:
        return None
    vals = [int(v) for v in vals]
    look, maxcode, valoff, code, k = [0] * 512, [-1] * 17, [0] * 17, 0, 0
    for ln in range(1, 17):
        valoff[ln] = k - code
        for _ in range(counts[ln - 1]):
            if code >= (1 << ln):
                return None
            if ln <= 9:
                first = code << (9 - ln)
                look[first:first + (1 << (9 - ln))] = [(ln << 8) | vals[k]] * (1 << (9 - ln))
            k, code = k + 1, code + 1
        maxcode[ln] = code - 1 if counts[ln - 1] else -1
        code <<= 1
    return look, maxcode, valoff, vals


class _HuffImage:
    """what a lane needs of its image (csrc/jpeg_huff.hip's Ctx)"""


def _huff_lane(c, in0, in1, endkey, last, strict, s, tolerant=True):
    """csrc/jpeg_huff.hip's lane(), statement for statement: (out0, out1, (m, bs, a0 .. a5), err) -- a: the DC sums per block slot
    from the entry's first block on (rounds) or per component (strict pass).  tolerant False (rounds only): a lane stops at the
    first impossible event -- the rule that does not synchronise."""
    if not strict:
        s = (0, 0, 0, 0, 0, 0, 0, 0)
    if in1 & _STOPPED:
        return in0, in1, s, 0
    d, n = c.d, c.len
    track = c.ri != 0
    # -- the reader (p, acc, have, stop, ff) and its entry
    rem, lead = in1 & 7, (in1 >> 3) & 15
    p = in0
    if rem and p >= 1:
        p = p - 2 if (p >= 2 and d[p - 1] == 0 and d[p - 2] == 0xFF) else p - 1
    R = [p, 0, 0, False, 0]                                       # p, acc, have, stop, ff

    def load1():
        q = R[0]
        if q >= n:
            R[3] = True
            return
        v = d[q]
        if v == 0xFF:
            if n - q < 2 or d[q + 1] != 0:
                R[3] = True
                return
            R[0], R[4] = q + 2, ((R[4] << 1) | 1) & 0xFFFFFFFF
        else:
            R[0], R[4] = q + 1, (R[4] << 1) & 0xFFFFFFFF
        R[1] |= v << (56 - R[2])
        R[2] += 8

    def fill():
        while R[2] <= 56 and not R[3]:
            load1()

    def take(k):
        if k > R[2]:
            return False
        R[1] = (R[1] << k) & _M64
        R[2] -= k
        return True

    def reset():
        R[1], R[2], R[3], R[4] = 0, 0, False, 0

    def position():
        whole, rm = R[2] >> 3, R[2] & 7
        return R[0] - whole - bin(R[4] & ((1 << whole) - 1)).count("1"), rm, (whole if track else 0)

    def symbol(t):
        look, maxcode, valoff, vals = t
        if R[2] < 16:
            fill()
        e = look[R[1] >> 55]
        if e:
            return (e & 0xFF) if take(e >> 8) else -1
        for ln in range(10, 17):
            code = R[1] >> (64 - ln)
            if code <= maxcode[ln]:
                if not take(ln):
                    return -1
                return vals[(valoff[ln] + code) & 255]
        return -2

    def extend(sz):
        if R[2] < sz:
            fill()
        r = R[1] >> (64 - sz)
        if not take(sz):
            return None
        return r - (1 << sz) + 1 if r < (1 << (sz - 1)) else r

    for _ in range(lead + (1 if rem else 0)):
        if R[3]:
            break
        load1()
    if rem and R[2] >= 8:
        take(8 - rem)
    blk, k, slot = (in1 >> 7) & 7, (in1 >> 10) & 63, 0
    freeze = c.same and not strict
    m, bs = s[0], s[1]
    dd = list(s[2:])
    if strict:
        blk = bs % c.mcub
    tol, stopped, err, cur = not strict, False, 0, None
    if strict:
        g = m * c.rim + bs
        if g >= c.total:
            return in0, in1, s, 0
        if track and (bs > c.rim or (bs == c.rim and k != 0)):
            tol = True
        else:
            cur = c.coef[c.block_of(g)]
    it = 0
    while it < c.cap:
        it += 1
        pc, rm, ld = position()
        if not last and pc - (1 if rm else 0) >= endkey:
            break
        if not tol and k == 0:
            g = m * c.rim + bs
            if g >= c.total:
                break
            if track and bs == c.rim:
                q = R[0]
                if q >= n:
                    err = TRUNCATED
                    break
                if d[q] != 0xFF:
                    err = BAD_CODE
                    break
                while q < n and d[q] == 0xFF:
                    q += 1
                if q >= n:
                    err = TRUNCATED
                    break
                if d[q] != 0xD0 + (m & 7):
                    err = BAD_CODE
                    break
                R[0] = q + 1
                reset()
                m, bs, dd, blk = m + 1, 0, [0] * 6, 0
                continue
            cur = c.coef[c.block_of(g)]
        comp = 0 if blk < c.ylum else blk - c.ylum + 1
        nobits = endblock = False
        sym = symbol(c.tabs[2 * comp + (1 if k else 0)])
        if sym == -1:
            nobits = True
        elif sym == -2:
            if not tol:
                err = TRUNCATED if R[2] < 16 else BAD_CODE
                break
            if not tolerant:
                stopped = True
                break
            if not take(1):
                nobits = True
        elif k == 0:
            sz = sym
            if sz > 15:
                if not tol:
                    err = BAD_CODE
                    break
                if not tolerant:
                    stopped = True
                    break
                sz = 15
            v = extend(sz) if sz else 0
            if v is None:
                nobits = True
            else:
                dd[comp if strict else slot] = (dd[comp if strict else slot] + v) & 0xFFFFFFFF
                if not tol:
                    cur[0] = dd[comp] & 0xFFFF
                k = 1
        else:
            r, sz = sym >> 4, sym & 15
            if sz == 0:
                if r == 15:
                    k += 16
                    if k > 64 and not tol:
                        err = BAD_CODE
                        break
                    if k > 64 and not tolerant:
                        stopped = True
                        break
                    if k >= 64:
                        endblock = True
                else:
                    endblock = True
            else:
                k += r
                if k > 63:
                    if not tol:
                        err = BAD_CODE
                        break
                    if not tolerant:
                        stopped = True
                        break
                    endblock = True
                else:
                    v = extend(sz)
                    if v is None:
                        nobits = True
                    else:
                        if not tol:
                            cur[ZIGZAG[k]] = v & 0xFFFF
                        k += 1
                        if k >= 64:
                            endblock = True
        if nobits:
            if not tol:
                err = TRUNCATED
                break
            q = R[0]
            while q < n and d[q] == 0xFF:
                q += 1
            if q > R[0] and q < n and (d[q] & 0xF8) == 0xD0:
                R[0] = q + 1
                reset()
                m, bs, dd, blk, k, slot = m + 1, 0, [0] * 6, 0, 0, 0
                if strict:
                    tol = False
                continue
            stopped = True
            break
        if endblock:
            k, blk, bs = 0, (0 if freeze or blk + 1 == c.mcub else blk + 1), bs + 1
            slot = 0 if slot + 1 == c.mcub else slot + 1
    if strict:
        return in0, in1, s, err
    pc, rm, ld = position()
    return pc, rm | ld << 3 | blk << 7 | k << 10 | (_STOPPED if stopped else 0), (m, bs) + tuple(dd), 0


def huff_record_status(scan, jrec, desc: HuffDesc, bytes_len: int, coef_blocks: int, work_bytes: Optional[int] = None) -> np.ndarray:
    """The device's validity rule per image (TF2_JPEG_REC_* bits; 0: decoded) -- a statement in Python integers.  work_bytes None:
    a workspace that is large enough."""
    scan = np.asarray(scan, SCAN_DTYPE).reshape(-1)
    jrec = np.asarray(jrec, JPEG_DTYPE).reshape(-1)
    B, nc, (mx, my), S = len(scan), desc.components, desc.eff_sub, desc.subseq
    slice_ = None if work_bytes is None else (int(work_bytes) // B) & ~7
    out = np.zeros(B, np.int32)
    for i, (sc, j) in enumerate(zip(scan, jrec)):
        off, ln, ri, st = int(sc["byte_off"]), int(sc["byte_len"]), int(sc["restart_interval"]), 0
        if off < 0 or ln < 0 or ln > HUFF_MAX_BYTES or off > bytes_len or ln > bytes_len - off:
            st |= REC_BAD_RANGE
        if (int(sc["components"]), int(sc["sub_x"]), int(sc["sub_y"])) != (nc, mx, my) or not 0 <= ri <= 65535:
            st |= REC_BAD_SCAN
        for c in range(nc):
            if _huff_table(sc["tab"][c]["dc_counts"], sc["tab"][c]["dc_vals"]) is None or \
               _huff_table(sc["tab"][c]["ac_counts"], sc["tab"][c]["ac_vals"]) is None:
                st |= REC_BAD_TABLE
        if not st & REC_BAD_RANGE and slice_ is not None and HUFF_WORK_HEADER + 8 * max(1, -(-ln // S)) > slice_:
            st |= REC_WORK_TOO_SMALL
        bw, bh, bo = [int(v) for v in j["bw"]], [int(v) for v in j["bh"]], [int(v) for v in j["block_off"]]
        for c in range(nc):
            if not (1 <= bw[c] <= 8192 and 1 <= bh[c] <= 8192):
                st |= REC_BAD_GRID
            if bo[c] < 0:
                st |= REC_BAD_OFFSET
        if not st & REC_BAD_GRID:
            if bw[0] % mx or bh[0] % my:
                st |= REC_BAD_GRID
            elif nc == 3 and (bw[1] != bw[0] // mx or bw[2] != bw[1] or bh[1] != bh[0] // my or bh[2] != bh[1]):
                st |= REC_BAD_GRID
        if not st & (REC_BAD_GRID | REC_BAD_OFFSET):
            for c in range(nc):
                if bo[c] > coef_blocks or bw[c] * bh[c] > coef_blocks - bo[c]:
                    st |= REC_OUT_OF_COEF
        out[i] = st
    return out


def reference_huff(data, scan, jrec, desc: HuffDesc, coef_blocks: int, coef=None, work_bytes: Optional[int] = None,
                   tolerant: bool = True):
    """The statement of tf2_jpeg_huff on the device's own inputs: data (the byte buffer), scan (SCAN_DTYPE [B]), jrec (JPEG_DTYPE
    [B]) -> (coef int16 [coef_blocks, 64], status int32 [B], rounds int32 [B]).  It runs the parallel algorithm itself:
    subsequences of desc.subseq bytes in chunks of huff_chunk_lanes, tolerant rounds until no entry state changes, the prefix sums, the
    strict pass, the record statuses and the zeroing; `rounds` is the rounds used, summed over the chunks.  coef: the buffer as it is
    before the call (default zeros); only the extents of images without a record bit change.  tolerant False switches the tolerance
    of the rounds off (a lane stops at the first impossible event): what the rule is there for."""
    buf = _bytes(data)
    scan = np.asarray(scan, SCAN_DTYPE).reshape(-1)
    jrec = np.asarray(jrec, JPEG_DTYPE).reshape(-1)
    B, nc, (mx, my), S = len(scan), desc.components, desc.eff_sub, desc.subseq
    out = np.zeros((coef_blocks, 64), np.int16) if coef is None else np.array(coef, np.int16).reshape(coef_blocks, 64)
    u16 = out.view(np.uint16)
    status = huff_record_status(scan, jrec, desc, buf.size, coef_blocks, work_bytes)
    rounds = np.zeros(B, np.int32)
    for b in range(B):
        if status[b]:
            continue
        sc, j = scan[b], jrec[b]
        c = _HuffImage()
        off, c.len = int(sc["byte_off"]), int(sc["byte_len"])
        c.d = bytes(buf[off:off + c.len])
        c.tabs = [t for k in range(nc) for t in (_huff_table(sc["tab"][k]["dc_counts"], sc["tab"][k]["dc_vals"]),
                                                 _huff_table(sc["tab"][k]["ac_counts"], sc["tab"][k]["ac_vals"]))]
        c.mcub, c.ylum = (1, 1) if nc == 1 else (mx * my + 2, mx * my)
        c.same = nc == 3 and sc["tab"][0].tobytes() == sc["tab"][1].tobytes() == sc["tab"][2].tobytes()
        c.ri = int(sc["restart_interval"])
        c.rim = c.ri * c.mcub
        bw, bh, bo = [int(v) for v in j["bw"]], [int(v) for v in j["bh"]], [int(v) for v in j["block_off"]]
        c.mcus_x = bw[0] // mx
        c.total = c.mcus_x * (bh[0] // my) * c.mcub
        c.coef, c.cap = u16, 9 * c.len + 64

        def block_of(g, mcub=c.mcub, mcus_x=c.mcus_x, ylum=c.ylum, bw0=bw[0], bo=bo):
            mcu, bi = divmod(g, mcub)
            r, q = divmod(mcu, mcus_x)
            if bi < ylum:
                y, x = divmod(bi, mx)
                return bo[0] + (r * my + y) * bw0 + q * mx + x
            return bo[bi - ylum + 1] + r * mcus_x + q
        c.block_of = block_of
        for k in range(nc):
            out[bo[k]:bo[k] + bw[k] * bh[k]] = 0
        N = max(1, -(-c.len // S))
        carry, run, err = (0, 0), (0, 0, 0, 0, 0), 0
        L = huff_chunk_lanes(S)
        for first in range(0, N, L):
            nl = min(L, N - first)
            ends = [(first + t + 1) * S for t in range(nl)]
            lasts = [first + t == N - 1 for t in range(nl)]
            ins = [carry]
            for t in range(1, nl):
                at = (first + t) * S
                ins.append((at + 1 if c.d[at] == 0 and c.d[at - 1] == 0xFF else at, 0))
            res = [_huff_lane(c, ins[t][0], ins[t][1], ends[t], lasts[t], False, None, tolerant) for t in range(nl)]
            used = 1
            for _ in range(1, nl):
                new = [carry] + [(res[t - 1][0], res[t - 1][1]) for t in range(1, nl)]
                changed = [t for t in range(nl) if new[t] != ins[t]]
                if not changed:
                    break
                used += 1
                for t in changed:                                 # (all of them from the exits of the round before)
                    ins[t] = new[t]
                res_new = {t: _huff_lane(c, ins[t][0], ins[t][1], ends[t], lasts[t], False, None, tolerant) for t in changed}
                for t, v in res_new.items():
                    res[t] = v
            rounds[b] += used
            pre = []
            for t in range(nl):
                pre.append(run + (0, 0, 0))
                lm = res[t][2]
                phase, per = (0 if lm[0] else run[1] % c.mcub), [0, 0, 0]          # slot 0 is this block of the MCU
                for q in range(c.mcub):
                    comp = 0 if phase < c.ylum else phase - c.ylum + 1
                    per[comp] = (per[comp] + lm[2 + q]) & 0xFFFFFFFF
                    phase = 0 if phase + 1 == c.mcub else phase + 1
                run = (run[0] + lm[0], lm[1], per[0], per[1], per[2]) if lm[0] else \
                    (run[0], run[1] + lm[1], (run[2] + per[0]) & 0xFFFFFFFF, (run[3] + per[1]) & 0xFFFFFFFF, (run[4] + per[2]) & 0xFFFFFFFF)
            carry = (res[nl - 1][0], res[nl - 1][1])
            for t in range(nl):
                e = _huff_lane(c, ins[t][0], ins[t][1], ends[t], lasts[t], True, pre[t])[3]
                if e and not err:
                    err = e
            if err:
                break
        if err:
            for k in range(nc):
                out[bo[k]:bo[k] + bw[k] * bh[k]] = 0
        status[b] = err
    return out, status, rounds


def pack_bytes_host(files_and_infos, layout: int, sub, pixel_bytes: int = 3, preset: Optional[P.Preset] = None, align: int = 4,
                    gap: int = 0):
    """(bytes uint8 [n], scan SCAN_DTYPE [B], jrec, quant, yrec, srec, coef_blocks, planes_bytes, pixels_bytes) of a list of (file
    bytes, Info): the files' entropy-coded bytes back to back (`gap` bytes of 0xA5 between them) and everything behind the
    coefficients exactly as `pack_host` lays it out"""
    items = [(f, i if i is not None else parse(f)) for f, i in files_and_infos]
    for _, info in items:
        assert info.status == 0, f"status {info.status}"
    blank = [(info, np.zeros((info.total_blocks, 64), np.int16)) for _, info in items]
    hc, jrec, quant, yrec, srec, pbytes, need = pack_host(blank, layout, sub, pixel_bytes, preset, align)
    parts, scan, at = [], np.zeros(len(items), SCAN_DTYPE), 0
    for i, (f, info) in enumerate(items):
        data = _bytes(f)[info.scan_offset:]
        scan[i] = scan_record(f, info, at)
        parts += [data, np.full(gap, 0xA5, np.uint8)]
        at += data.size + gap
    return np.concatenate(parts), scan, jrec, quant, yrec, srec, len(hc), pbytes, need


def pack_bytes(files_and_infos, layout: int, sub, device, pixel_bytes: int = 3, preset: Optional[P.Preset] = None, align: int = 4,
               subseq_bytes: int = 0, data=None, scan=None, coef=None, jpeg=None, quant=None, planes=None, ycc=None, srcs=None,
               pixels=None, work=None):
    """The device inputs of tf2_jpeg_huff and of the tf2_jpeg_idct / tf2_ycc_to_rgb behind it, from `pack_bytes_host`: (data uint8,
    scan int32 [B, 416], coef int16 [n, 64], jpeg int32 [B, 12], quant int16 [B, 3, 64], planes uint8, ycc int32 [B, 8], srcs int32
    [B, 10], pixels uint8, work uint8) tensors.  With data= .. work= the caller's tensors are refilled instead (a captured graph reads
    the same buffers at every replay): the bytes go to the front of `data`, the records fill the tables, `coef`, `planes`, `pixels`
    and `work` only have to be large enough (`work`: huff_work_bytes of the longest scan)."""
    import torch
    hb, hscan, jrec, hq, yrec, srec, nblocks, pbytes, need = pack_bytes_host(files_and_infos, layout, sub, pixel_bytes, preset, align)
    B = len(hscan)

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
    if data is None:
        data = torch.from_numpy(hb).to(device)
    else:
        assert data.dtype == torch.uint8 and data.dim() == 1 and data.numel() >= hb.size, "byte buffer too small"
        data[:hb.size].copy_(torch.from_numpy(hb))
    if coef is None:
        coef = torch.zeros(nblocks, 64, dtype=torch.int16, device=device)
    else:
        assert coef.dtype == torch.int16 and coef.dim() == 2 and coef.shape[1] == 64 and coef.shape[0] >= nblocks, "coefficient buffer too small"
    wneed = huff_work_bytes(HuffDesc(layout, tuple(sub), subseq_bytes), B, int(hscan["byte_len"].max()))
    return (data, table(scan, Y.records_to_words(hscan, SCAN_WORDS), "scan"), coef, table(jpeg, Y.records_to_words(jrec, JPEG_WORDS), "jpeg"),
            table(quant, hq.view(np.int16), "quant").view(torch.int16), room(planes, pbytes, "plane buffer"),
            table(ycc, Y.records_to_words(yrec, Y.YCC_WORDS), "ycc"), table(srcs, Y.records_to_words(srec, P.SRC_WORDS), "srcs"),
            room(pixels, need, "pixel buffer"), room(work, wneed, "workspace"))


class DeviceEntropy:
    """tf2_jpeg_huff with `desc` (a HuffDesc).
      run(data, scan, jpeg, coef, work, stream=None, status=None) -> status
    data: the uint8 device tensor the scans' bytes lie in, scan: int32 [B, 416] (tf2_jpeg_scan records), jpeg: int32 [B, 12]
    (tf2_jpeg_src), coef: int16 [n, 64] device tensor the blocks are written into, work: uint8 workspace of at least
    huff_work_bytes(desc, B, longest scan) -- `pack_bytes` makes all five, and DeviceDecoder reads coef / jpeg next.  status: int32
    [B]: 0, TRUNCATED or BAD_CODE (the image's blocks are zero), or TF2_JPEG_REC_* bits of an image that was left alone.  Enqueued on
    `stream` (default: the current one); nothing synchronises or allocates beyond the status, which may be passed in."""

    def __init__(self, desc: HuffDesc = HuffDesc()):
        self.desc = desc
        self._c = desc.c()

    def run(self, data, scan, jpeg, coef, work, stream=None, status=None):
        import torch
        from . import _lib
        dev = _lib.expect(coef, torch.int16, cols=64)
        _lib.expect(data, torch.uint8, device=dev, ndim=1)
        _lib.expect(work, torch.uint8, device=dev)
        _lib.expect(scan, torch.int32, device=dev, cols=SCAN_WORDS)
        B = scan.shape[0]
        _lib.expect(jpeg, torch.int32, (B, JPEG_WORDS), dev)
        stream = stream or torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            if status is None:
                status = torch.empty(B, dtype=torch.int32, device=dev)
            _lib.expect(status, torch.int32, (B,), dev)
            _lib.check(_lib.lib().tf2_jpeg_huff(C.byref(self._c), data.data_ptr(), data.numel(), scan.data_ptr(), jpeg.data_ptr(),
                                                coef.data_ptr(), coef.shape[0], work.data_ptr(), work.numel(), B, status.data_ptr(),
                                                stream.cuda_stream))
        return status

    def reference(self, data, scan, jpeg, coef, work_bytes=None):
        """`reference_huff` on host copies of the tensors (coef: the buffer as it is before the call)"""
        host = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
        sr = np.ascontiguousarray(host(scan), np.int32).view(SCAN_DTYPE).reshape(-1)
        jr = np.ascontiguousarray(host(jpeg), np.int32).view(JPEG_DTYPE).reshape(-1)
        hc = host(coef)
        return reference_huff(host(data), sr, jr, self.desc, len(hc), hc, work_bytes)
