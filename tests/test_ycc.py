"""YCbCr frames, CPU side: the statement ycc.reference / upsample_fancy against Pillow's recorded bytes (tests/golden/pil_ycc.npz:
every case, byte for byte), the JFIF terms against their formula, the two video matrices over all 2^24 triples, REPLICATE against
np.repeat, NV12 / NV21 / GRAY against planar, every status bit alone and in combination, the host refusals of tf2_ycc_to_rgb (fake
device pointers: a refusal touches no device), the binding's constants against the header, and the scratch-free ISA of
ycc_convert.hip.  The device itself is checked in tests/test_gpu_ycc.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from tf2_amd import _lib, preprocess as P, ycc as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_ycc_golden as G  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    cases, _ = G.load()
    return cases


def test_record_layout_and_constants_match_the_header():
    assert Y.YCC_DTYPE.itemsize == C.sizeof(_lib.YccSrc) == 32 and Y.YCC_WORDS == 8
    assert [Y.YCC_DTYPE.fields[n][1] for n in Y.YCC_DTYPE.names] == [getattr(_lib.YccSrc, n).offset for n in Y.YCC_DTYPE.names]
    assert C.sizeof(_lib.YccDesc) == 48
    hdr = open(os.path.join(ROOT, "include", "tf2_amd.h")).read()
    val = lambda name: int(re.search(r"\b%s\s*=?\s*(\d+)" % name, hdr).group(1))
    assert (Y.TILE_W, Y.TILE_H) == (val("TF2_YCC_TILE_W"), val("TF2_YCC_TILE_H"))
    assert (Y.PLANAR, Y.SEMI_CBCR, Y.SEMI_CRCB, Y.GRAY) == tuple(val("TF2_YCC_" + n) for n in ("PLANAR", "SEMI_CBCR", "SEMI_CRCB", "GRAY"))
    assert (Y.FANCY, Y.REPLICATE) == (val("TF2_YCC_FANCY"), val("TF2_YCC_REPLICATE"))
    assert (Y.JFIF, Y.BT601, Y.BT709) == (val("TF2_YCC_JFIF"), val("TF2_YCC_BT601"), val("TF2_YCC_BT709"))
    assert (Y.BAD_SIZE, Y.BAD_PITCH, Y.BAD_OFFSET, Y.OUT_OF_SRC, Y.OUT_OF_DST) == tuple(
        val("TF2_YCC_" + n) for n in ("BAD_SIZE", "BAD_PITCH", "BAD_OFFSET", "OUT_OF_SRC", "OUT_OF_DST"))
    assert [Y.default_blocks_per_image(b) for b in (1, 32, 33, 2048, 5000)] == [64, 64, 62, 1, 1]
    assert Y.TILE_W % 8 == 0 and Y.TILE_H % 2 == 0          # a tile starts at an even pixel and a whole chroma dword


def test_the_fixture_is_complete(golden):
    """every subsampling x every size of the issue x random and 0 / 255 values: 60 cases, none excluded below"""
    want = {(kind, sub, h, w) for kind in (0, 1) for sub in Y.SUBSAMPLINGS
            for h, w in [(48, 64), (37, 53), (16, 16), (17, 33), (8, 8), (1, 1), (9, 2), (2, 9), (33, 17), (50, 75)]}
    assert {(kind, sub, h, w) for _, kind, sub, h, w, _, _ in golden} == want and len(golden) == 60
    for seed, kind, sub, h, w, rgb, ycc in golden:
        y, cb, cr = G.case_planes(seed, kind, G.SUBS.index(sub), h, w)
        assert np.array_equal(ycc[:, :, 0], y)
        if kind == 1:
            assert set(np.unique(np.concatenate([y.ravel(), cb.ravel(), cr.ravel()]))) <= {0, 255}


def test_upsample_fancy_is_pillows_ycbcr(golden):
    for seed, kind, sub, h, w, _, ycc in golden:
        _, cb, cr = G.case_planes(seed, kind, G.SUBS.index(sub), h, w)
        assert np.array_equal(Y.upsample_fancy(cb, sub, h, w), ycc[:, :, 1]), (seed, sub, h, w)
        assert np.array_equal(Y.upsample_fancy(cr, sub, h, w), ycc[:, :, 2]), (seed, sub, h, w)
        assert np.array_equal(Y.upsample(cb, sub, h, w, Y.FANCY), ycc[:, :, 1])


@pytest.mark.parametrize("sub", Y.SUBSAMPLINGS)
def test_reference_is_pillows_rgb(golden, sub):
    """the whole call -- pack, records, upsampling, colour, the write into the pixel buffer -- on every case of one subsampling as one
    batch: Pillow's RGB bytes, and nothing else in the buffer changed"""
    cases = [c for c in golden if c[2] == sub]
    assert len(cases) == 20
    frames = [G.case_planes(seed, kind, G.SUBS.index(sub), h, w) for seed, kind, _, h, w, _, _ in cases]
    desc = Y.Desc(layout=Y.PLANAR, sub=sub)
    src, yrec, srec, need = Y.pack_ycc_host(frames, Y.PLANAR, sub, align=4)
    before = np.full(need + 5, 0xA5, np.uint8)
    out, st = Y.reference(src, yrec, srec, desc, before)
    assert (st == 0).all()
    touched = np.zeros(out.size, bool)
    for (seed, kind, _, h, w, rgb, _), r in zip(cases, srec):
        for y in range(h):
            a = int(r["offset"]) + y * int(r["row_pitch"])
            assert np.array_equal(out[a:a + 3 * w], rgb[y].reshape(-1)), (seed, h, w, y)
            touched[a:a + 3 * w] = True
    assert (out[~touched] == 0xA5).all()


def test_jfif_terms_against_their_formula():
    """the four terms of libjpeg's tables over all 256 values: each is the rounded product within the fixed point's error, and the
    whole conversion is Y + term, clamped, for every Y"""
    x = np.arange(256, dtype=np.int64) - 128
    terms = {"r_cr": (Y.fix(1.40200) * x + 32768) >> 16,
             "b_cb": (Y.fix(1.77200) * x + 32768) >> 16}
    assert (Y.fix(1.40200), Y.fix(0.34414), Y.fix(0.71414), Y.fix(1.77200)) == (91881, 22554, 46802, 116130)
    for name, k in (("r_cr", 1.40200), ("b_cb", 1.77200)):
        assert np.abs(terms[name] - k * x).max() <= 0.5 + 128 * 2.0 ** -17
    g = (-Y.fix(0.34414) * x[:, None] + 32768 - Y.fix(0.71414) * x[None, :]) >> 16               # [cb, cr]
    assert np.abs(g - (-0.34414 * x[:, None] - 0.71414 * x[None, :])).max() <= 0.5 + 2 * 128 * 2.0 ** -17
    cb, cr = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for yv in range(256):
        rgb = Y.to_rgb(np.full_like(cb, yv), cb, cr, Y.JFIF)
        assert np.array_equal(rgb[:, :, 0], np.clip(yv + terms["r_cr"][None, :], 0, 255).repeat(256, 0))
        assert np.array_equal(rgb[:, :, 1], np.clip(yv + g, 0, 255))
        assert np.array_equal(rgb[:, :, 2], np.clip(yv + terms["b_cb"][:, None], 0, 255).repeat(256, 1))


@pytest.mark.parametrize("matrix", [Y.BT601, Y.BT709])
def test_video_matrices_over_all_triples(matrix):
    """all 2^24 (Y, Cb, Cr): at most 1 from floor(the double formula + 0.5) clamped, and every sum inside 27 bits (so inside
    int32).  How often it differs is counted, not bounded: 9298 (BT601) and 10122 (BT709) triples, 0.055 % and 0.060 % of them --
    0.018 % and 0.020 % of the channel values."""
    ky, yoff, r_cr, g_cb, g_cr, b_cb = Y.MATRIX[matrix]
    cb, cr = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    cbd, crd = cb - 128.0, cr - 128.0
    worst, differ, top = 0, 0, 0
    for yv in range(256):
        got = Y.to_rgb(np.full_like(cb, yv), cb, cr, matrix).astype(np.int64)
        yy = ky * (yv - yoff)
        want = np.stack([yy + r_cr * crd, yy + g_cb * cbd + g_cr * crd, yy + b_cb * cbd], axis=-1)
        want = np.clip(np.floor(want + 0.5), 0, 255).astype(np.int64)
        d = np.abs(got - want)
        worst, differ = max(worst, int(d.max())), differ + int((d != 0).any(axis=-1).sum())
        yi = Y.fix(ky) * (yv - yoff) + 32768
        sums = [yi + Y.fix(r_cr) * (cr - 128), yi - Y.fix(-g_cb) * (cb - 128) - Y.fix(-g_cr) * (cr - 128), yi + Y.fix(b_cb) * (cb - 128)]
        top = max(top, max(int(np.abs(s).max()) for s in sums))
    print(f"matrix {matrix}: {differ} of 2^24 triples differ from the rounded double formula, largest |sum| {top}")
    assert worst <= 1, (worst, differ)
    assert top < 2 ** 26, top


def _planes(rng, h, w, sub, binary=False):
    ch, cw = Y.chroma_size(h, w, sub)
    mk = (lambda s: (rng.integers(0, 2, s) * 255).astype(np.uint8)) if binary else (lambda s: rng.integers(0, 256, s, dtype=np.uint8))
    return mk((h, w)), mk((ch, cw)), mk((ch, cw))


SIZES = [(1, 1), (2, 9), (9, 2), (17, 33), (5, 4), (16, 31)]


@pytest.mark.parametrize("sub", Y.SUBSAMPLINGS)
def test_replicate_is_np_repeat(sub):
    rng = np.random.default_rng(sub[0] * 3 + sub[1])
    for h, w in SIZES:
        _, cb, _ = _planes(rng, h, w, sub)
        want = np.repeat(np.repeat(cb, sub[1], axis=0), sub[0], axis=1)[:h, :w]
        assert np.array_equal(Y.upsample(cb, sub, h, w, Y.REPLICATE), want)


def _run(frames, desc, **kw):
    src, yrec, srec, need = Y.pack_ycc_host(frames, desc.layout, desc.sub, desc.pixel_bytes, **kw)
    out, st = Y.reference(src, yrec, srec, desc, need)
    assert (st == 0).all()
    return out


@pytest.mark.parametrize("sub", Y.SUBSAMPLINGS)
@pytest.mark.parametrize("upsample", [Y.FANCY, Y.REPLICATE])
def test_semi_planar_and_gray_equal_planar(sub, upsample):
    rng = np.random.default_rng(17 + sub[0] + sub[1] + upsample)
    frames = [_planes(rng, h, w, sub, binary=(i % 2 == 1)) for i, (h, w) in enumerate(SIZES)]
    for matrix in (Y.JFIF, Y.BT601, Y.BT709):
        kw = dict(sub=sub, upsample=upsample, matrix=matrix, pixel_bytes=4, dst_channel=(2, 0, 3), alpha=7)
        want = _run(frames, Y.Desc(layout=Y.PLANAR, **kw))
        assert np.array_equal(_run(frames, Y.Desc(layout=Y.SEMI_CBCR, **kw)), want)
        assert np.array_equal(_run(frames, Y.Desc(layout=Y.SEMI_CRCB, **kw)), want)
        pairs = [(y, np.stack([cr, cb], axis=-1)) for y, cb, cr in frames]             # NV21 given as interleaved pairs
        assert np.array_equal(_run(pairs, Y.Desc(layout=Y.SEMI_CRCB, **kw)), want)
        px = want.reshape(-1, 4)
        assert (px[:, 1] == 7).all()                                                     # alpha in the byte no channel took
        grey = [(y, np.full_like(cb, 128), np.full_like(cr, 128)) for y, cb, cr in frames]
        assert np.array_equal(_run([y for y, _, _ in frames], Y.Desc(layout=Y.GRAY, **kw)), _run(grey, Y.Desc(layout=Y.PLANAR, **kw)))


def test_subsample_box_and_pack():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    y, cb, cr = Y.subsample_box(img, (2, 2))
    assert y.shape == (5, 7) and cb.shape == cr.shape == (3, 4) and np.array_equal(y, img[:, :, 0])
    assert cb[0, 0] == (int(img[0, 0, 1]) + int(img[0, 1, 1]) + int(img[1, 0, 1]) + int(img[1, 1, 1]) + 2) // 4
    assert cr[2, 3] == img[4, 6, 2]                                                      # the corner box is one sample, repeated
    y1, cb1, cr1 = Y.subsample_box(img, (1, 1))
    assert np.array_equal(np.stack([y1, cb1, cr1], axis=-1), img)
    src, yrec, srec, need = Y.pack_ycc_host([(y, cb, cr)], Y.PLANAR, (2, 2), 3, preset=P.TORCHVISION_PIL, align=4)
    assert tuple(srec[0])[1:4] == (5, 7, 24) and tuple(srec[0])[4:8] == P.TORCHVISION_PIL.geometry(5, 7)
    assert (int(yrec[0]["pitch_y"]), int(yrec[0]["pitch_c"])) == (8, 4) and need == 5 * 24
    got = Y.planes_of(src, yrec[0], 5, 7, Y.Desc())
    assert all(np.array_equal(a, b) for a, b in zip(got, (y, cb, cr)))


def _records(n=1, h=6, w=10, sub=(2, 2), pb=3, semi=False):
    """n valid records of h x w images in a source of exactly the bytes they need and a destination likewise"""
    ch, cw = Y.chroma_size(h, w, sub)
    crow = 2 * cw if semi else cw
    yrec, srec = np.zeros(n, Y.YCC_DTYPE), np.zeros(n, P.SRC_DTYPE)
    at = 0
    for i in range(n):
        yrec[i] = (at, at + h * w, at + h * w + ch * crow, w, crow)
        at += h * w + (1 if semi else 2) * ch * crow
        srec[i] = (i * h * w * pb, h, w, w * pb, h, w, 0, 0, 0)
    return yrec, srec, at, n * h * w * pb


def test_every_status_bit_alone_and_in_combination():
    d = Y.Desc()
    yrec, srec, ns, nd = _records(14)
    assert (Y.record_status(yrec, srec, d, ns, nd) == 0).all()
    assert Y.record_status(yrec, srec, d, ns - 1, nd).tolist() == [0] * 13 + [Y.OUT_OF_SRC]        # the last Cr byte
    assert Y.record_status(yrec, srec, d, ns, nd - 1).tolist() == [0] * 13 + [Y.OUT_OF_DST]
    srec[1]["h"] = 0
    srec[2]["w"] = 32768
    yrec[2]["pitch_y"], yrec[2]["pitch_c"], srec[2]["row_pitch"] = 32768, 16384, 3 * 32768             # BAD_SIZE alone
    yrec[3]["pitch_y"] = 9
    yrec[4]["pitch_c"] = 4
    srec[5]["row_pitch"] = 29
    yrec[6]["off_y"] = -1
    yrec[7]["off_cb"] = -4
    yrec[8]["off_cr"] = -1
    srec[9]["offset"] = -1
    yrec[10]["off_cr"] = ns - 14                                                                   # one byte too late: 3 rows of 5
    srec[11]["offset"] = nd - 6 * 30 + 1
    srec[12]["h"], yrec[12]["pitch_y"], yrec[12]["off_cb"] = -5, 3, -9                             # SIZE | PITCH | OFFSET
    yrec[13]["off_y"], srec[13]["offset"] = ns, nd                                                 # both extents
    want = [0, Y.BAD_SIZE, Y.BAD_SIZE, Y.BAD_PITCH, Y.BAD_PITCH, Y.BAD_PITCH, Y.BAD_OFFSET, Y.BAD_OFFSET, Y.BAD_OFFSET, Y.BAD_OFFSET,
            Y.OUT_OF_SRC, Y.OUT_OF_DST, Y.BAD_SIZE | Y.BAD_PITCH | Y.BAD_OFFSET, Y.OUT_OF_SRC | Y.OUT_OF_DST]
    assert Y.record_status(yrec, srec, d, ns, nd).tolist() == want
    # what a layout does not read is not judged: NV12 ignores off_cr and wants 2 * cw bytes a chroma row, GRAY ignores all chroma
    yrec, srec, ns, nd = _records(3, semi=True)
    semi = Y.Desc(layout=Y.SEMI_CBCR)
    yrec[0]["off_cr"] = -7
    yrec[1]["pitch_c"] = 9
    assert Y.record_status(yrec, srec, semi, ns, nd).tolist() == [0, Y.BAD_PITCH, 0]
    yrec[2]["off_cb"], yrec[2]["pitch_c"] = -1, -1
    assert Y.record_status(yrec, srec, Y.Desc(layout=Y.GRAY), ns, nd).tolist() == [0, 0, 0]
    # an image with a status is neither read nor written; its neighbours are what they are alone
    rng = np.random.default_rng(3)
    yrec, srec, ns, nd = _records(3)
    src = rng.integers(0, 256, ns, dtype=np.uint8)
    alone, _ = Y.reference(src, yrec, srec, d, nd)
    yrec[1]["pitch_y"] = 2
    out, st = Y.reference(src, yrec, srec, d, np.full(nd, 9, np.uint8))
    n1 = nd // 3
    assert st.tolist() == [0, Y.BAD_PITCH, 0] and (out[n1:2 * n1] == 9).all()
    assert np.array_equal(out[:n1], alone[:n1]) and np.array_equal(out[2 * n1:], alone[2 * n1:])


FAKE = 0x7f0000001000      # never dereferenced: every case is refused before a device call


def _call(desc=None, batch=2, ptrs=(FAKE, FAKE + (1 << 24), FAKE + (2 << 24), FAKE + (3 << 24), FAKE + (4 << 24)), src_bytes=1 << 20,
          pixels_bytes=1 << 20, **kw):
    d = (desc if desc is not None else Y.Desc()).c() if desc is not False else None
    for k, v in kw.items():
        if k == "dst":
            d.dst_channel[v[0]] = v[1]
        else:
            setattr(d, k, v)
    src, ycc, pixels, srcs, status = ptrs
    st = _lib.lib().tf2_ycc_to_rgb(C.byref(d) if d is not None else None, src, src_bytes, ycc, pixels, pixels_bytes, srcs, batch, status, None)
    return st, _lib.lib().tf2_last_error().decode()


@pytest.mark.parametrize("kw,message", [
    (dict(desc=False), "null desc"), (dict(size=44), "desc size"),
    (dict(layout=-1), "layout"), (dict(layout=4), "layout"),
    (dict(sub_x=1, sub_y=2), "sub_x"), (dict(sub_x=4, sub_y=1), "sub_x"), (dict(sub_x=0, sub_y=0), "sub_x"), (dict(sub_y=3), "sub_x"),
    (dict(upsample=2), "upsample"), (dict(upsample=-1), "upsample"), (dict(matrix=3), "matrix"), (dict(matrix=-1), "matrix"),
    (dict(pixel_bytes=2), "pixel_bytes"), (dict(pixel_bytes=5), "pixel_bytes"),
    (dict(dst=(1, 3)), "dst_channel[1]"), (dict(dst=(0, -1)), "dst_channel[0]"), (dict(dst=(2, 0)), "distinct"), (dict(dst=(1, 2)), "distinct"),
    (dict(alpha=256), "alpha"), (dict(alpha=-1), "alpha"), (dict(blocks_per_image=-1), "blocks_per_image"),
    (dict(batch=0), "batch"), (dict(batch=-3), "batch"),
    (dict(ptrs=(FAKE, FAKE + (2 << 24), FAKE + (1 << 20) - 1, FAKE + (3 << 24), FAKE + (4 << 24))), "overlap"),
    (dict(ptrs=(FAKE + 5, FAKE + (2 << 24), FAKE, FAKE + (3 << 24), FAKE + (4 << 24))), "overlap"),
    (dict(ptrs=(FAKE, FAKE + (2 << 24), FAKE, FAKE + (3 << 24), FAKE + (4 << 24))), "overlap"),
] + [(dict(ptrs=tuple(None if i == k else FAKE + (i << 24) for i in range(5))), "null device pointer") for k in range(5)])
def test_host_refusals(kw, message):
    st, err = _call(**kw)
    assert st == -1 and err.startswith("tf2_ycc_to_rgb: ") and message in err, (st, err)


def test_the_limits_of_the_desc_pass_every_check():
    """the extremes pass every check on the desc and are refused for the batch only; GRAY does not look at sub_x / sub_y"""
    for d in (Y.Desc(layout=Y.GRAY, sub=(7, 9), upsample=Y.REPLICATE, matrix=Y.BT709, pixel_bytes=4, dst_channel=(3, 2, 1), alpha=0,
                     blocks_per_image=1 << 20),
              Y.Desc(layout=Y.SEMI_CRCB, sub=(2, 1), pixel_bytes=3, dst_channel=(2, 1, 0), alpha=255)):
        st, err = _call(desc=d, batch=0, ptrs=(FAKE, FAKE + (2 << 24), FAKE + (1 << 20), FAKE + (3 << 24), FAKE + (4 << 24)))
        assert st == -1 and "batch" in err, err


def test_ycc_kernels_compile_without_scratch():
    import vmcnt_check
    seg, lds, txt = vmcnt_check.kernel_segments("ycc_convert")
    names = [k for k in seg if "ycc_to_rgb_kernel" in k]
    assert len(names) == 8, seg                                    # 3- and 4-byte pixels x grey, point, h2v1, h2v2 chroma
    assert all(seg[k] == 0 for k in names), seg
    assert "global_atomic" not in txt and "ds_add" not in txt
