"""JPEG files, CPU side: the host library (tf2_jpeg_parse / tf2_jpeg_entropy) against an independent pure-Python decoder, the
statement reference_idct against Pillow's recorded planes and -- through ycc.upsample / ycc.to_rgb and the file's own upsampling
rule -- against Pillow's RGB of every fixture file (tests/golden/pil_jpeg.npz), the narrow-image rule, header rewrites that change
nothing, every status bit of the parser, of the entropy decoder (cuts at every byte of a scan, seeded bit flips, guard words) and of
record_status, the host refusals of tf2_jpeg_idct (fake device pointers: a refusal touches no device), the wrap regime against
Python integers, the binding's layouts and constants against the header, the scratch-free ISA of jpeg_idct.hip, and the host
decoder under the address and undefined-behaviour sanitizers as a stand-alone program.  The device is checked in
tests/test_gpu_jpeg.py."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from tf2_amd import _lib, jpeg as J, preprocess as P, ycc as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_jpeg_golden as G  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return G.load()[0]


@pytest.fixture(scope="module")
def decoded(golden):
    """[(case, Info, coef)] of the supported files, through the host library"""
    out = []
    for c in golden:
        if G.supported(c):
            info = J.parse(c["file"])
            assert info.status == 0, (c["seed"], info.status)
            coef, st = J.entropy(c["file"], info)
            assert st == 0, (c["seed"], st)
            out.append((c, info, coef))
    return out


def test_record_layouts_and_constants_match_the_header():
    assert J.JPEG_DTYPE.itemsize == C.sizeof(_lib.JpegSrc) == 48 and J.JPEG_WORDS == 12
    assert [J.JPEG_DTYPE.fields[n][1] for n in J.JPEG_DTYPE.names] == [getattr(_lib.JpegSrc, n).offset for n in J.JPEG_DTYPE.names]
    assert C.sizeof(_lib.JpegDesc) == 20 and C.sizeof(_lib.JpegInfo) == 480
    assert (_lib.JpegInfo.total_blocks.offset, _lib.JpegInfo.scan_offset.offset, _lib.JpegInfo.quant.offset) == (80, 88, 96)
    hdr = open(os.path.join(ROOT, "include", "tf2_amd.h")).read()
    val = lambda name: int(re.search(r"\b%s\s*=?\s*(\d+)" % name, hdr).group(1))
    assert (J.TILE_BW, J.TILE_BH) == (val("TF2_JPEG_TILE_BW"), val("TF2_JPEG_TILE_BH"))
    names = ("UNSUPPORTED_PROGRESSIVE", "UNSUPPORTED_ARITHMETIC", "UNSUPPORTED_PRECISION", "UNSUPPORTED_COMPONENTS", "UNSUPPORTED_SAMPLING",
             "UNSUPPORTED_SCANS", "UNSUPPORTED_COLORSPACE", "BAD_HEADER", "TRUNCATED", "BAD_CODE")
    assert [getattr(J, n) for n in names] == [val("TF2_JPEG_" + n) for n in names] == [1 << i for i in range(10)]
    assert J.UNSUPPORTED == sum(getattr(J, n) for n in names[:7])
    rec = ("BAD_SIZE", "BAD_GRID", "BAD_PITCH", "BAD_OFFSET", "OUT_OF_COEF", "OUT_OF_PLANES")
    assert [getattr(J, "REC_" + n) for n in rec] == [val("TF2_JPEG_REC_" + n) for n in rec]
    assert [J.default_blocks_per_image(b) for b in (1, 32, 33, 2048, 5000)] == [64, 64, 62, 1, 1]
    # the struct the header prints is the struct the binding declares, field for field
    body = re.search(r"typedef struct tf2_jpeg_src \{(.*?)\} tf2_jpeg_src;", hdr, re.S).group(1)
    assert re.findall(r"\b(block_off|bw|bh)\[3\]", body) == ["block_off", "bw", "bh"]
    body = re.search(r"typedef struct tf2_jpeg_info \{(.*?)\} tf2_jpeg_info;", hdr, re.S).group(1)
    fields = re.findall(r"\b([a-z_]+)(?:\[\d+\])*\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in _lib.JpegInfo._fields_]
    body = re.search(r"typedef struct tf2_jpeg_desc \{(.*?)\} tf2_jpeg_desc;", hdr, re.S).group(1)
    fields = re.findall(r"\b([a-z_]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in _lib.JpegDesc._fields_]


def test_the_fixture_is_complete(golden):
    """L and the three subsamplings at every size of the issue, the four qualities, optimize, restart markers every 1 and 3 blocks in
    every mode, the four kinds of content, and the two files the parser refuses"""
    sizes = [(1, 1), (8, 8), (2, 9), (9, 2), (9, 3), (9, 4), (9, 5), (15, 15), (16, 16), (17, 17), (17, 33), (37, 53), (48, 64), (50, 75)]
    ok = [c for c in golden if G.supported(c)]
    assert {(c["mode"], c["h"], c["w"]) for c in ok} == {(m, h, w) for m in (-1, 0, 1, 2) for h, w in sizes} and len(ok) == 56
    for mode in (-1, 0, 1, 2):
        mine = [c for c in ok if c["mode"] == mode]
        assert {c["quality"] for c in mine} == {30, 75, 95, 100} and {c["optimize"] for c in mine} == {0, 1}
        assert {c["restart"] for c in mine} == {0, 1, 3} and {c["kind"] for c in mine} == {0, 1, 2, 3}
    assert sorted(c["mode"] for c in golden if not G.supported(c)) == [G.MODE_PROGRESSIVE, G.MODE_CMYK] and len(golden) == 58
    assert os.path.getsize(G.PATH) < 400_000
    for c in golden:
        assert c["file"][:2] == b"\xff\xd8" and c["rgb"].shape == (c["h"], c["w"], 3)
    assert any((c["rgb"] == 0).any() and (c["rgb"] == 255).any() for c in ok)


def test_entropy_equals_the_independent_decoder(decoded):
    for c, info, coef in decoded:
        head, want = J.reference_entropy(c["file"])
        assert (head["h"], head["w"], head["components"], head["sub"]) == (info.h, info.w, info.components, info.sub), c["seed"]
        assert (head["bw"], head["bh"], head["restart_interval"]) == (info.bw, info.bh, info.restart_interval), c["seed"]
        assert np.array_equal(head["quant"], info.quant[:info.components]), c["seed"]
        assert coef.dtype == want.dtype == np.int16 and np.array_equal(coef, want), c["seed"]
    assert any(np.abs(coef[:, 32:]).max() > 50 for _, _, coef in decoded)          # high AC terms occur


def test_info_is_what_the_header_says(decoded):
    for c, info, coef in decoded:
        n = 1 if c["mode"] == G.MODE_L else 3
        sub = (1, 1) if n == 1 else G.SUBS[c["mode"]]
        mw, mh = -(-c["w"] // (8 * sub[0])), -(-c["h"] // (8 * sub[1]))
        assert info.bw == ((mw * sub[0], mw, mw) if n == 3 else (mw,)) and info.bh == ((mh * sub[1], mh, mh) if n == 3 else (mh,))
        ch, cw = Y.chroma_size(c["h"], c["w"], sub)
        assert info.ph == (c["h"], ch, ch)[:n] and info.pw == (c["w"], cw, cw)[:n]
        assert info.total_blocks == len(coef) == sum(a * b for a, b in zip(info.bw, info.bh))
        synth_info = J.make_info(c["h"], c["w"], J.group_key(info)[0], sub, info.quant)
        assert synth_info.key()[:5] + synth_info.key()[6:] == info.key()[:5] + info.key()[6:]      # all but the restart interval
        assert c["file"][info.scan_offset - 3:info.scan_offset] == b"\x00\x3f\x00"           # Ss, Se, Ah / Al: the scan follows


def test_the_narrow_rule(decoded):
    """libjpeg replicates chroma planes at most 2 samples wide: REPLICATE exactly for the subsampled cases with w <= 4"""
    narrow = set()
    for c, info, _ in decoded:
        want = c["mode"] in (1, 2) and c["w"] <= 4
        assert (info.upsample == Y.REPLICATE) == want and info.upsample in (Y.FANCY, Y.REPLICATE), (c["mode"], c["h"], c["w"])
        if want:
            narrow.add((c["mode"], c["h"], c["w"]))
    assert narrow == {(m, h, w) for m in (1, 2) for h, w in [(1, 1), (9, 2), (9, 3), (9, 4)]}


def test_reference_idct_gives_pillows_planes(decoded):
    for c, info, coef in decoded:
        planes = J.planes_of_file(info, coef)
        assert np.array_equal(planes[0], c["ycc"][:, :, 0]), c["seed"]
        if c["mode"] == 0:
            assert np.array_equal(planes[1], c["ycc"][:, :, 1]) and np.array_equal(planes[2], c["ycc"][:, :, 2]), c["seed"]
        elif c["mode"] in (1, 2):
            for k in (1, 2):
                assert np.array_equal(Y.upsample(planes[k], info.sub, info.h, info.w, info.upsample), c["ycc"][:, :, k]), (c["seed"], k)


def test_end_to_end_is_pillows_rgb(decoded):
    """file -> entropy -> reference_idct -> the file's upsampling rule -> ycc.to_rgb == Pillow's convert('RGB'), every supported
    case, the narrow ones included; and with the other rule the narrow ones differ (the rule matters)"""
    other = 0
    for c, info, coef in decoded:
        assert np.array_equal(J.rgb_of_file(info, coef), c["rgb"]), (c["seed"], c["mode"], c["h"], c["w"])
        if c["mode"] in (1, 2) and c["w"] in (2, 3, 4):
            pl = J.planes_of_file(info, coef)
            up = [Y.upsample(p, info.sub, info.h, info.w, Y.FANCY) for p in pl[1:]]
            other += not np.array_equal(Y.to_rgb(pl[0], up[0], up[1]), c["rgb"])
    assert other >= 1


def test_the_whole_device_statement_on_fixture_files(decoded):
    """pack_host + reference (the statement of tf2_jpeg_idct) + ycc.reference on one batch per group: Pillow's RGB in the pixel
    buffer"""
    groups = {}
    for c, info, coef in decoded:
        groups.setdefault(J.group_key(info), []).append((c, info, coef))
    assert len(groups) == 6
    for (layout, sub, upsample), members in groups.items():
        coef, jrec, quant, yrec, srec, pbytes, need = J.pack_host([(i, k) for _, i, k in members], layout, sub)
        planes, st = J.reference(coef, jrec, quant, yrec, srec, J.Desc(layout, sub), pbytes)
        px, st2 = Y.reference(planes, yrec, srec, Y.Desc(layout=layout, sub=sub, upsample=upsample), need)
        assert (st == 0).all() and (st2 == 0).all()
        for (c, _, _), r in zip(members, srec):
            got = np.stack([px[int(r["offset"]) + y * int(r["row_pitch"]):][:3 * c["w"]] for y in range(c["h"])])
            assert np.array_equal(got.reshape(c["h"], c["w"], 3), c["rgb"]), c["seed"]


# ---------------------------------------------------------------- header surgery

def segments(data):
    """[(marker, start of the FF, end)] of the segments up to and including SOS"""
    out, p = [], 2
    while True:
        assert data[p] == 0xFF
        m = data[p + 1]
        n = (data[p + 2] << 8) | data[p + 3]
        out.append((m, p, p + 2 + n))
        p += 2 + n
        if m == 0xDA:
            return out


def rebuild(data, edit):
    """the file with every header segment passed through edit(marker, segment bytes) -> bytes (or a list of segments)"""
    segs = segments(data)
    out = [data[:2]]
    for m, a, b in segs:
        out.append(edit(m, data[a:b]))
    return b"".join(out) + data[segs[-1][2]:]


def seg(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def test_header_rewrites_change_nothing(decoded):
    for c, info, coef in decoded[::3]:
        def wide(m, s):
            if m != 0xDB:
                return s
            at, out = 4, b""
            while at < len(s):
                assert s[at] >> 4 == 0
                out += bytes([0x10 | (s[at] & 15)]) + b"".join(struct.pack(">H", v) for v in s[at + 1:at + 65])
                at += 65
            return seg(0xDB, out)
        extra = lambda m, s: (seg(0xFE, b"a comment \xff\xd9 inside") + seg(0xE5, b"\x00" * 300) + s) if m in (0xDB, 0xDA) else s
        for data in (rebuild(c["file"], wide), rebuild(c["file"], extra), rebuild(rebuild(c["file"], extra), wide)):
            assert data != c["file"]
            info2 = J.parse(data)
            assert info2.key() == info.key() and info2.status == 0, c["seed"]
            coef2, st = J.entropy(data, info2)
            assert st == 0 and np.array_equal(coef2, coef), c["seed"]


def _case(golden, mode, h, w):
    return next(c for c in golden if (c["mode"], c["h"], c["w"]) == (mode, h, w))


def test_every_parser_status_bit(golden):
    prog = next(c for c in golden if c["mode"] == G.MODE_PROGRESSIVE)
    cmyk = next(c for c in golden if c["mode"] == G.MODE_CMYK)
    assert J.parse(prog["file"]).status == J.UNSUPPORTED_PROGRESSIVE
    assert J.parse(cmyk["file"]).status & J.UNSUPPORTED_COMPONENTS and not J.parse(cmyk["file"]).status & ~J.UNSUPPORTED
    base = _case(golden, 2, 17, 33)["file"]
    assert J.parse(base).status == 0

    def sof(fn):
        return rebuild(base, lambda m, s: fn(bytearray(s)) if m == 0xC0 else s)

    def patch(s, i, v):
        s = bytearray(s)
        s[i] = v
        return bytes(s)
    st = lambda data: J.parse(data).status
    assert st(sof(lambda s: patch(s, 1, 0xC9))) == J.UNSUPPORTED_ARITHMETIC
    assert st(sof(lambda s: patch(s, 1, 0xC3))) == J.UNSUPPORTED_PROGRESSIVE
    assert st(sof(lambda s: patch(s, 1, 0xC1))) == 0                                   # SOF1 with 8-bit samples is taken
    assert st(sof(lambda s: patch(s, 4, 12))) == J.UNSUPPORTED_PRECISION
    assert st(sof(lambda s: patch(s, 11, 0x12))) == J.UNSUPPORTED_SAMPLING             # luma 1 x 2
    assert st(sof(lambda s: patch(s, 14, 0x21))) == J.UNSUPPORTED_SAMPLING             # chroma 2 x 1
    assert st(sof(lambda s: patch(s, 11, 0x41))) == J.UNSUPPORTED_SAMPLING
    assert st(sof(lambda s: patch(patch(patch(s, 4, 12), 11, 0x12), 1, 0xC2))) == (
        J.UNSUPPORTED_PRECISION | J.UNSUPPORTED_SAMPLING | J.UNSUPPORTED_PROGRESSIVE)
    one_scan = rebuild(base, lambda m, s: seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) if m == 0xDA else s)
    assert st(one_scan) == J.UNSUPPORTED_SCANS
    # libjpeg's rule for RGB: no JFIF marker and an Adobe marker with transform 0, or neither marker and the ids R, G, B
    no_jfif = lambda m, s: b"" if m == 0xE0 else s
    adobe = lambda t: (lambda m, s: (seg(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([t])) + s) if m == 0xC0 else no_jfif(m, s))
    assert st(rebuild(base, adobe(0))) == J.UNSUPPORTED_COLORSPACE and st(rebuild(base, adobe(1))) == 0
    assert st(rebuild(base, lambda m, s: (seg(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x00") + s) if m == 0xC0 else s)) == 0     # JFIF wins

    def ids(m, s):
        s = bytearray(s)
        if m == 0xC0:
            s[10], s[13], s[16] = b"RGB"
        if m == 0xDA:
            s[5], s[7], s[9] = b"RGB"
        return no_jfif(m, bytes(s))
    assert st(rebuild(base, ids)) == J.UNSUPPORTED_COLORSPACE
    assert st(rebuild(base, lambda m, s: ids(m, s) if m != 0xE0 else s)) == 0          # with JFIF the ids mean nothing
    # malformed headers
    sos = segments(base)[-1]
    for data in (b"", b"\xff", base[:1], b"\x00" + base[1:], base[:sos[1]], base[:sos[2] - 1], base[:2] + base[4:],
                 rebuild(base, lambda m, s: b"" if m == 0xC4 else s), rebuild(base, lambda m, s: b"" if m == 0xDB else s),
                 rebuild(base, lambda m, s: b"" if m == 0xC0 else s), sof(lambda s: patch(s, 9, 0)), sof(lambda s: patch(patch(s, 5, 0), 6, 0)),
                 rebuild(base, lambda m, s: s[:4] + bytes([0x25]) + s[5:] if m == 0xDB else s)):
        assert st(data) == J.BAD_HEADER, data[:24]
    for cut in range(0, sos[2]):
        assert st(base[:cut]) == J.BAD_HEADER, cut
    assert st(base[:sos[2]]) == 0                                                      # the headers are whole: the scan is not the parser's


def _entropy_guarded(data, info, guard=3):
    """tf2_jpeg_entropy into a buffer with guard blocks behind capacity_blocks: (status, coef); asserts the guards"""
    buf = np.full((info.total_blocks + guard, 64), 0x7B7B, np.int16)
    raw = np.frombuffer(data, np.uint8)
    st = C.c_int32(-1)
    rc = _lib.lib().tf2_jpeg_entropy(raw.ctypes.data, raw.size, C.byref(info.raw), buf.ctypes.data, info.total_blocks, C.byref(st))
    assert rc == 0 and (buf[info.total_blocks:] == 0x7B7B).all()
    return st.value, buf[:info.total_blocks]


def test_every_entropy_status_bit(golden, decoded):
    """cuts at every byte of the scan of five files (with and without restart markers, with and without their own Huffman tables): TRUNCATED, the blocks
    decoded so far equal the whole file's, the rest zero; seeded bit flips: 0, TRUNCATED or BAD_CODE and no write behind the
    capacity; a wrong restart marker: BAD_CODE"""
    seen = set()
    picks = [(2, 17, 33), (0, 15, 15), (-1, 15, 15), (1, 16, 16), (2, 16, 16)]
    assert {_case(golden, *p)["restart"] for p in picks} == {0, 1, 3} and {_case(golden, *p)["optimize"] for p in picks} == {0, 1}
    rng = np.random.default_rng(5)
    for mode, h, w in picks:
        c, info, coef = next(d for d in decoded if (d[0]["mode"], d[0]["h"], d[0]["w"]) == (mode, h, w))
        data = c["file"]
        assert data[-2:] == b"\xff\xd9"
        for cut in range(info.scan_offset, len(data) - 2):
            st, got = _entropy_guarded(data[:cut], info)
            assert st == J.TRUNCATED, (cut, st)
            differ = (got != coef).any(axis=1)                  # blocks not reached are zero; one block may be partial
            assert (differ & got.any(axis=1)).sum() <= 1, cut
            seen.add(st)
        assert _entropy_guarded(data[:-2], info)[0] == 0                                   # EOI is not needed
        for _ in range(400):
            v = bytearray(data)
            for _ in range(int(rng.integers(1, 4))):
                v[int(rng.integers(info.scan_offset, len(v)))] ^= 1 << int(rng.integers(0, 8))
            st, got = _entropy_guarded(bytes(v), info)
            assert st in (0, J.TRUNCATED, J.BAD_CODE), st
            seen.add(st)
    assert seen == {0, J.TRUNCATED, J.BAD_CODE}
    c, info, coef = next(d for d in decoded if d[0]["restart"] == 1 and d[0]["mode"] == 2 and d[0]["h"] >= 16)
    at = c["file"].index(b"\xff\xd0", info.scan_offset)
    st, got = _entropy_guarded(c["file"][:at + 1] + b"\xd3" + c["file"][at + 2:], info)
    assert st == J.BAD_CODE and got[1:info.bw[0] * info.bh[0]].any() == (info.sub != (1, 1))  # only the first MCU was decoded
    # the refusals of the call itself
    raw = np.frombuffer(c["file"], np.uint8)
    out = np.zeros((info.total_blocks, 64), np.int16)
    stw = C.c_int32(0)
    L = _lib.lib()
    assert L.tf2_jpeg_entropy(raw.ctypes.data, raw.size, C.byref(info.raw), out.ctypes.data, info.total_blocks - 1, C.byref(stw)) == -3
    assert not out.any()
    assert L.tf2_jpeg_entropy(None, raw.size, C.byref(info.raw), out.ctypes.data, info.total_blocks, C.byref(stw)) == -1
    assert L.tf2_jpeg_parse(raw.ctypes.data, raw.size, None) == -1
    other = decoded[0][0]["file"]                                                          # a file that `info` does not describe
    raw2 = np.frombuffer(other, np.uint8)
    assert L.tf2_jpeg_entropy(raw2.ctypes.data, raw2.size, C.byref(info.raw), out.ctypes.data, info.total_blocks, C.byref(stw)) == 0
    assert stw.value == J.BAD_HEADER and not out.any()


def test_decode_host_threads(golden):
    files = [c["file"] for c in golden]
    one, many = J.decode_host(files, threads=1), J.decode_host(files)
    assert J.decode_host.__defaults__ == (16,)
    for c, (i1, c1, s1), (i2, c2, s2) in zip(golden, one, many):
        assert i1.key() == i2.key() and s1 == s2 and (s1 == 0) == G.supported(c)
        assert (c1 is None and c2 is None) or np.array_equal(c1, c2)


def _records(n=1, h=20, w=30, sub=(2, 2), gray=False):
    """n valid records of h x w images in a coefficient buffer of exactly the blocks they need and planes likewise"""
    info = J.make_info(h, w, Y.GRAY if gray else Y.PLANAR, sub, np.ones(64))
    jrec, yrec, srec = np.zeros(n, J.JPEG_DTYPE), np.zeros(n, Y.YCC_DTYPE), np.zeros(n, P.SRC_DTYPE)
    at = nb = 0
    for i in range(n):
        offs = []
        for c in range(info.components):
            jrec[i]["block_off"][c], jrec[i]["bw"][c], jrec[i]["bh"][c] = nb, info.bw[c], info.bh[c]
            nb += info.bw[c] * info.bh[c]
            offs.append(at)
            at += info.ph[c] * info.pw[c]
        offs += [0] * (3 - len(offs))
        yrec[i] = (offs[0], offs[1], offs[2], w, info.pw[-1] if not gray else 0)
        srec[i] = (0, h, w, 3 * w, h, w, 0, 0, 0)
    return jrec, yrec, srec, nb, at


def test_every_record_status_bit_alone_and_in_combination():
    d = J.Desc()
    jrec, yrec, srec, nb, ns = _records(16)
    assert (J.record_status(jrec, yrec, srec, d, nb, ns) == 0).all()
    assert J.record_status(jrec, yrec, srec, d, nb - 1, ns).tolist() == [0] * 15 + [J.REC_OUT_OF_COEF]
    assert J.record_status(jrec, yrec, srec, d, nb, ns - 1).tolist() == [0] * 15 + [J.REC_OUT_OF_PLANES]
    srec[1]["h"] = 0
    srec[2]["w"] = 32768
    yrec[2]["pitch_y"], yrec[2]["pitch_c"], jrec[2]["bw"] = 32768, 16384, 4096                   # BAD_SIZE alone
    jrec[3]["bw"][0] = 3                                                                          # 24 < 30
    jrec[4]["bh"][2] = 1                                                                          # 8 < 10
    jrec[5]["bh"][1] = 0
    yrec[6]["pitch_y"] = 29
    yrec[7]["pitch_c"] = 14
    jrec[8]["block_off"][1] = -1
    yrec[9]["off_cr"] = -1
    yrec[10]["off_y"] = -4
    jrec[11]["block_off"][2] = nb - 3                                                             # 2 x 2 blocks: one too late
    yrec[12]["off_cb"] = ns - 10 * 15 + 1
    srec[13]["h"], yrec[13]["pitch_y"], yrec[13]["off_cb"], jrec[13]["bw"][1] = -5, 3, -9, -1   # SIZE | GRID | PITCH | OFFSET
    jrec[14]["block_off"][0], yrec[14]["off_y"] = nb, ns                                          # both extents
    want = [0, J.REC_BAD_SIZE, J.REC_BAD_SIZE, J.REC_BAD_GRID, J.REC_BAD_GRID, J.REC_BAD_GRID, J.REC_BAD_PITCH, J.REC_BAD_PITCH,
            J.REC_BAD_OFFSET, J.REC_BAD_OFFSET, J.REC_BAD_OFFSET, J.REC_OUT_OF_COEF, J.REC_OUT_OF_PLANES,
            J.REC_BAD_SIZE | J.REC_BAD_GRID | J.REC_BAD_PITCH | J.REC_BAD_OFFSET, J.REC_OUT_OF_COEF | J.REC_OUT_OF_PLANES, 0]
    assert J.record_status(jrec, yrec, srec, d, nb, ns).tolist() == want
    # GRAY reads component 0, off_y and pitch_y alone
    jrec, yrec, srec, nb, ns = _records(3, gray=True)
    g = J.Desc(layout=Y.GRAY)
    jrec[0]["bw"][1], jrec[0]["block_off"][2], yrec[0]["off_cb"], yrec[0]["pitch_c"] = 0, -1, -1, -1
    yrec[1]["pitch_y"] = 29
    assert J.record_status(jrec, yrec, srec, g, nb, ns).tolist() == [0, J.REC_BAD_PITCH, 0]
    # an image with a status is neither read nor written; its neighbours are what they are alone
    rng = np.random.default_rng(3)
    jrec, yrec, srec, nb, ns = _records(3)
    coef = rng.integers(-300, 300, (nb, 64)).astype(np.int16)
    quant = rng.integers(1, 40, (3, 3, 64)).astype(np.uint16)
    alone, _ = J.reference(coef, jrec, quant, yrec, srec, d, ns)
    jrec[1]["bw"][0] = 2
    out, st = J.reference(coef, jrec, quant, yrec, srec, d, np.full(ns, 9, np.uint8))
    n1 = ns // 3
    assert st.tolist() == [0, J.REC_BAD_GRID, 0] and (out[n1:2 * n1] == 9).all()
    assert np.array_equal(out[:n1], alone[:n1]) and np.array_equal(out[2 * n1:], alone[2 * n1:])


FAKE = 0x7f0000001000      # never dereferenced: every case is refused before a device call
PTRS = tuple(FAKE + (i << 26) for i in range(7))     # coef, jpeg, quant, planes, ycc, srcs, status


def _call(desc=None, batch=2, ptrs=PTRS, coef_blocks=1 << 13, planes_bytes=1 << 20, **kw):
    d = (desc if desc is not None else J.Desc()).c() if desc is not False else None
    for k, v in kw.items():
        setattr(d, k, v)
    coef, jpeg, quant, planes, ycc, srcs, status = ptrs
    st = _lib.lib().tf2_jpeg_idct(C.byref(d) if d is not None else None, coef, coef_blocks, jpeg, quant, planes, planes_bytes, ycc, srcs,
                                  batch, status, None)
    return st, _lib.lib().tf2_last_error().decode()


def _with(i, v):
    return tuple(v if k == i else p for k, p in enumerate(PTRS))


@pytest.mark.parametrize("kw,message", [
    (dict(desc=False), "null desc"), (dict(size=24), "desc size"),
    (dict(layout=-1), "layout"), (dict(layout=Y.SEMI_CBCR), "layout"), (dict(layout=Y.SEMI_CRCB), "layout"), (dict(layout=4), "layout"),
    (dict(sub_x=1, sub_y=2), "sub_x"), (dict(sub_x=4, sub_y=1), "sub_x"), (dict(sub_x=0, sub_y=0), "sub_x"), (dict(sub_y=3), "sub_x"),
    (dict(blocks_per_image=-1), "blocks_per_image"), (dict(batch=0), "batch"), (dict(batch=-3), "batch"),
    (dict(coef_blocks=1 << 62), "wraps"),
    (dict(ptrs=_with(3, FAKE + (1 << 20) - 1)), "overlap"), (dict(ptrs=_with(0, PTRS[3] + 5)), "overlap"), (dict(ptrs=_with(3, FAKE)), "overlap"),
] + [(dict(ptrs=_with(k, None)), "null device pointer") for k in range(7)])
def test_host_refusals(kw, message):
    st, err = _call(**kw)
    assert st == -1 and err.startswith("tf2_jpeg_idct: ") and message in err, (st, err)


def test_the_limits_of_the_desc_pass_every_check():
    """the extremes pass every check on the desc and are refused for the batch only; GRAY does not look at sub_x / sub_y; buffers
    that touch are disjoint"""
    for d in (J.Desc(layout=Y.GRAY, sub=(7, 9), blocks_per_image=1 << 20), J.Desc(layout=Y.PLANAR, sub=(2, 1))):
        st, err = _call(desc=d, batch=0, ptrs=_with(3, FAKE + (1 << 20)), coef_blocks=1 << 13)
        assert st == -1 and "batch" in err, err


def _idct_python(c, q):
    """the header's arithmetic in Python integers reduced modulo 2^32 after every operation"""
    M = (1 << 32) - 1
    sgn = lambda v: v - (1 << 32) if v & (1 << 31) else v

    def K(x, s):
        x0, x1, x2, x3, x4, x5, x6, x7 = x
        z1 = ((x2 + x6) * 4433) & M
        t2, t3 = (z1 - x6 * 15137) & M, (z1 + x2 * 6270) & M
        t0, t1 = ((x0 + x4) << 13) & M, ((x0 - x4) << 13) & M
        a0, a3, a1, a2 = (t0 + t3) & M, (t0 - t3) & M, (t1 + t2) & M, (t1 - t2) & M
        b0, b1, b2, b3 = x7, x5, x3, x1
        z1, z2, z3, z4 = (b0 + b3) & M, (b1 + b2) & M, (b0 + b2) & M, (b1 + b3) & M
        z5 = ((z3 + z4) * 9633) & M
        b0, b1, b2, b3 = (b0 * 2446) & M, (b1 * 16819) & M, (b2 * 25172) & M, (b3 * 12299) & M
        z1, z2 = (z1 * -7373) & M, (z2 * -20995) & M
        z3, z4 = (z3 * -16069 + z5) & M, (z4 * -3196 + z5) & M
        b0, b1, b2, b3 = (b0 + z1 + z3) & M, (b1 + z2 + z4) & M, (b2 + z2 + z3) & M, (b3 + z1 + z4) & M
        outs = (a0 + b3, a1 + b2, a2 + b1, a3 + b0, a3 - b0, a2 - b1, a1 - b2, a0 - b3)
        return [(sgn((o + (1 << (s - 1))) & M) >> s) & M for o in outs]
    d = [[(int(c[v * 8 + u]) * int(q[v * 8 + u])) & M for u in range(8)] for v in range(8)]
    ws = [[0] * 8 for _ in range(8)]
    for u in range(8):
        col = K([d[k][u] for k in range(8)], 11)
        for k in range(8):
            ws[k][u] = col[k]
    return [[min(255, max(0, sgn(v) + 128)) for v in K(ws[k], 18)] for k in range(8)]


def test_reference_idct_wraps_like_python_integers():
    """full-range int16 coefficients with quantisers up to 65535: every intermediate wraps, and the numpy statement equals the
    arithmetic of the header in Python integers; the same on tame blocks, on extreme DC and on zero"""
    rng = np.random.default_rng(8)
    coef = rng.integers(-32768, 32768, (48, 64)).astype(np.int16)
    q = rng.integers(1, 65536, (48, 64)).astype(np.uint16)
    q[0], coef[1] = 65535, -32768
    coef[2], coef[3, 1:] = 0, 0
    coef[4:10] = rng.integers(-12, 13, (6, 64))
    q[4:10] = rng.integers(1, 6, (6, 64))
    got = J.reference_idct(coef, q)
    want = np.array([_idct_python(c, k) for c, k in zip(coef.tolist(), q.tolist())], np.uint8)
    assert np.array_equal(got, want)
    assert (got[2] == 128).all() and len(np.unique(got[3])) == 1 and len(np.unique(got[4:10])) > 50
    assert np.array_equal(J.reference_idct(coef[7], q[7]), got[7:8])                       # one table for all blocks


def test_jpeg_kernels_compile_without_scratch():
    import vmcnt_check
    seg_, lds, txt = vmcnt_check.kernel_segments("jpeg_idct")
    names = [k for k in seg_ if "jpeg_idct_kernel" in k]
    assert len(names) == 2, seg_                                   # one and three components
    assert all(seg_[k] == 0 for k in names), seg_
    assert "global_atomic" not in txt and "ds_add" not in txt


def test_host_decoder_under_the_sanitizers_stand_alone(golden, tmp_path):
    """jpeg_entropy.cpp + tests/native/jpeg_fuzz_main.cpp as one program under ASan and UBSan: every fixture file, then seeded
    truncations and bit flips of each, inputs and outputs in heap blocks of exactly their size.  Exit status 0."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "jpeg_fuzz")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tf2_amd", "csrc", "jpeg_entropy.cpp"), os.path.join(ROOT, "tests", "native", "jpeg_fuzz_main.cpp"), "-o", exe]
    # the runtimes inside the program where the compiler has them as archives (it then runs whatever else the loader brings along)
    built = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if built.returncode != 0:
        built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)\b|unrecognized[^\n]*-fsanitize", built.stderr):
        pytest.skip("this g++ has no sanitizer runtime: " + built.stderr.strip().splitlines()[-1])
    assert built.returncode == 0, built.stderr
    blob = tmp_path / "files.bin"
    with open(blob, "wb") as f:
        f.write(struct.pack("<I", len(golden)))
        for c in golden:
            f.write(struct.pack("<II", len(c["file"]), int(G.supported(c))) + c["file"])
    run = subprocess.run([exe, str(blob), "3000"], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    m = re.search(r"decoded (\d+), flagged (\d+), refused (\d+)", run.stdout)
    assert m and int(m.group(1)) >= 56 and int(m.group(2)) > 1000 and int(m.group(3)) > 1000, run.stdout
