"""The statement of the antialiased crop (tf2_amd.roi: crop_pil, roi_status_aa, reference_crop_aa; tf2_roi_crop_aa on the device):
crop_pil byte-identical to Pillow's recorded resize(box=) output (tests/golden/pil_resize_box.npz, tools/gen_pil_box_golden.py) and to
a live Pillow where one is installed; the whole-image ROI against preprocess.reference_aa; a case where it is not "crop, then
resize"; the validity rule at its limits; the host refusals of tf2_roi_crop_aa (fake device pointers: a refusal touches no device);
the cropper's antialias switch; and roi_crop_aa.hip's private and group segment sizes.  The device itself is checked in
tests/test_gpu_roi_aa.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from tf2_amd import _lib, config as cfg, preprocess as P, roi as R, synth
from tf2_amd.network import NetWork

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_pil_box_golden as golden  # noqa: E402


def _taps(src, box, oh, ow):
    h, w = src.shape[:2]
    return max(int(P.aa_coefs_box(w, box[0], box[2], ow)[1].max()), int(P.aa_coefs_box(h, box[1], box[3], oh)[1].max()))


def test_crop_pil_is_pillows_recorded_bytes():
    cases, version = golden.load(os.path.join(ROOT, "tests", "golden", "pil_resize_box.npz"))
    assert len(cases) >= 30 and version
    families, channels, taps = set(), set(), 0
    for family, src, box, oh, ow, want in cases:
        got = R.crop_pil(src, box, oh, ow)
        assert got.dtype == np.uint8 and got.shape == want.shape == (oh, ow, src.shape[2])
        assert np.array_equal(got, want), (family, src.shape, box, oh, ow, np.argwhere(got != want)[:4])
        families.add(family)
        channels.add(src.shape[2])
        taps = max(taps, _taps(src, box, oh, ow))
    assert families == {golden.WHOLE, golden.INTEGER, golden.EDGE, golden.FRACTIONAL, golden.THIN} and channels == {1, 3}
    assert taps >= 300                                                           # a few hundred taps
    shapes = [(src.shape[0], src.shape[1], oh, ow) for _, src, _, oh, ow, _ in cases]
    assert any(s[:2] == (1, 1) for s in shapes) and any(s[2:] == (1, 1) for s in shapes) and any(s[2] >= 33 and s[3] >= 40 for s in shapes)
    sides = [(box[2] - box[0], box[3] - box[1], oh, ow) for _, _, box, oh, ow, _ in cases]
    assert any(dx < ow and dy < oh for dx, dy, oh, ow in sides) and any(dx > ow and dy > oh for dx, dy, oh, ow in sides)
    assert any(dx < 1 or dy < 1 for dx, dy, _, _ in sides)


def test_crop_pil_is_a_live_pillow_where_installed():
    """an extra check where PIL imports (the recorded bytes above are the one that never skips)"""
    pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(77)
    for i in range(60):
        c = (1, 3)[i & 1]
        h, w = (int(v) for v in rng.integers(3, 150, 2))
        oh, ow = (int(v) for v in rng.integers(1, 41, 2))
        family = i % 5
        if family == golden.THIN:
            x0, y0 = rng.uniform(0, w - 0.7), rng.uniform(0, h - 0.7)
            box = (x0, y0, x0 + rng.uniform(0.05, 0.7), rng.uniform(y0 + 0.05, h))
        elif family == golden.EDGE:
            box = (0.0, rng.uniform(0, h - 1.5), rng.uniform(1, w), float(h)) if i & 2 else (rng.uniform(0, w - 1.5), 0.0, float(w), rng.uniform(1, h))
        else:
            box = golden.draw_box(rng, family, h, w)
        box = np.asarray(box, np.float32)
        img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        want = golden.pillow_resize_box(img, box, oh, ow)
        assert np.array_equal(R.crop_pil(img, box, oh, ow), want), (h, w, c, box, oh, ow)


def test_box_coefficients_of_the_whole_axis_are_the_plain_rule():
    for n_in, n_out in ((500, 227), (7, 30), (64, 2), (227, 227), (1, 5)):
        a, b = P.aa_coefs(n_in, n_out), P.aa_coefs_box(n_in, 0.0, n_in, n_out)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    lo, n, coef = P.aa_coefs_box(10, 2.0, 6.0, 4)                # scale exactly 1 at an integer offset: the bytes themselves
    assert lo.tolist() == [2, 3, 4, 5] and (coef[:, 0] == 1 << 22).all() and (coef[:, 1:] == 0).all()
    lo, n, coef = P.aa_coefs_box(10, 2.0, 6.0, 2)                # 2x: the window reaches one pixel outside the box, inside the image
    assert lo.tolist() == [1, 3] and n.tolist() == [4, 4] and coef.sum(axis=1).tolist() == [1 << 22, 1 << 22]


@pytest.mark.parametrize("src_order,align", [("RGB", 1), ("BGRA", 16)])
def test_whole_image_roi_is_preprocess_aa(src_order, align):
    """reference_crop_aa on (0, 0, w, h) == preprocess.reference_aa with resize = out_hw and crop (0, 0), bit for bit, float32 and
    int8, on 3- and 4-byte pixels, nonzero offsets and padded rows"""
    rng = np.random.default_rng(len(src_order) + align)
    pb = len(src_order)
    imgs = [rng.integers(0, 256, s + (pb,), dtype=np.uint8) for s in ((75, 100), (40, 21), (1, 9), (33, 1), (17, 13))]
    pre = P.TORCHVISION_PIL
    pixels, srcs, got_pb = P.pack_host(imgs, pre, align=align)
    assert got_pb == pb and (align == 1 or (srcs["row_pitch"] > srcs["w"] * pb).any())
    pixels = np.concatenate([rng.integers(0, 256, 37, dtype=np.uint8), pixels])      # every offset nonzero
    srcs["offset"] += 37
    out_hw = (12, 17)
    srcs["resize_h"], srcs["resize_w"], srcs["crop_y"], srcs["crop_x"] = out_hw[0], out_hw[1], 0, 0
    args = (out_hw, pb, P.src_channels(pre, src_order), np.float32(pre.mean), np.float32(pre.scale))
    rois = R.whole_image_rois(srcs)
    for q0 in (None, -5):
        want, wst = P.reference_aa(pixels, srcs, *args, q0)
        got, st = R.reference_crop_aa(pixels, srcs, rois, *args, False, q0)
        assert (wst == 0).all() and (st == 0).all()
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))
        assert len(np.unique(got)) > 4
    assert got.dtype == np.int8


def test_it_is_not_crop_then_resize():
    """an integer box inside a random image, downscaled 4x: Pillow's resize(box=) lets the filter read the pixels around the box, the
    resize of the cropped array clamps it at the crop's edge -- the border pixels differ, the interior ones do not"""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (64, 80, 3), dtype=np.uint8)
    x0, y0, x1, y1 = 16, 12, 64, 52
    boxed = R.crop_pil(img, (x0, y0, x1, y1), 10, 12)
    cropped = P.resize_pil(img[y0:y1, x0:x1], 10, 12)
    assert boxed.shape == cropped.shape == (10, 12, 3)
    assert (boxed != cropped).any() and (boxed[0] != cropped[0]).any() and (boxed[:, -1] != cropped[:, -1]).any()
    assert np.array_equal(boxed[1:-1, 1:-1], cropped[1:-1, 1:-1])         # windows that stay inside the box see the same pixels
    # ... and the pixels outside the box matter: changing one next to it changes the boxed result only
    img2 = img.copy()
    img2[y0 - 1, x0:x1] ^= 255
    assert (R.crop_pil(img2, (x0, y0, x1, y1), 10, 12) != boxed).any()


def _srcs(*hw):
    recs, at = np.zeros(len(hw), P.SRC_DTYPE), 0
    for i, (h, w) in enumerate(hw):
        recs[i] = (at, h, w, 3 * w, 0, 0, 0, 0, 0)
        at += h * w * 3
    return recs, at


def _rois(rows):
    rois = np.zeros(len(rows), R.ROI_DTYPE)
    for k, (image, x0, y0, x1, y1) in enumerate(rows):
        rois[k] = (image, 1, k, 0.5, x0, y0, x1, y1)
    return rois


def test_slot_validity_rule_at_its_limits():
    OH, OW = 4, 5
    srcs, size = _srcs((10, 8), (10, 8), (3, 200), (200, 3))
    srcs[1]["row_pitch"] = 23                                            # BAD_PITCH: the slot is BAD_SRC
    up, f32 = (lambda v: np.nextafter(np.float32(v), np.float32(np.inf))), np.float32
    neg = -np.nextafter(f32(0), f32(1))                                  # the largest negative float32
    cases = [
        ((0, 0.0, 0.0, 8.0, 10.0), 0), ((-1, 0.0, 0.0, 8.0, 10.0), R.EMPTY), ((4, 0.0, 0.0, 8.0, 10.0), R.BAD_IMAGE),
        ((0, 0.0, 0.0, up(8), 10.0), R.BOX_OUTSIDE), ((0, 0.0, 0.0, 8.0, up(10)), R.BOX_OUTSIDE),                 # x1 == w passes
        ((0, -0.0, -0.0, 8.0, 10.0), 0), ((0, neg, 0.0, 8.0, 10.0), R.BOX_OUTSIDE), ((0, 0.0, neg, 8.0, 10.0), R.BOX_OUTSIDE),
        ((2, 20.0, 0.0, 20.0 + 32 * OW, 3.0), 0), ((2, 20.0, 0.0, up(20.0 + 32 * OW), 3.0), R.BAD_SCALE),        # a side of exactly 32 * OW
        ((3, 0.0, 50.0, 3.0, 50.0 + 32 * OH), 0), ((3, 0.0, 50.0, 3.0, up(50.0 + 32 * OH)), R.BAD_SCALE),
        ((2, 0.0, 0.0, 200.0, 3.0), R.BAD_SCALE), ((2, 50.0, 0.0, 250.0, 3.0), R.BOX_OUTSIDE | R.BAD_SCALE),
        # the new bits are absent when BAD_BOX or BAD_SRC is set (or there is no source at all)
        ((0, -5.0, 0.0, -4.5, 10.0), R.BAD_BOX), ((0, np.nan, 0.0, 8.0, 10.0), R.BAD_BOX), ((0, 0.0, 0.0, np.inf, 10.0), R.BAD_BOX),
        ((1, -3.0, 0.0, 1000.0, 10.0), R.BAD_SRC), ((1, 0.0, 0.0, 0.5, 1000.0), R.BAD_SRC | R.BAD_BOX),
        ((9, -3.0, 0.0, 1000.0, 10.0), R.BAD_IMAGE), ((-1, -3.0, 0.0, 1000.0, 10.0), R.EMPTY),
        ((0, 2.25, 3.5, 6.75, 9.0), 0),
    ]
    rois = _rois([c for c, _ in cases])
    want = [bits for _, bits in cases]
    assert R.roi_status_aa(rois, srcs, 3, size, (OH, OW)).tolist() == want
    # the plain rule on the same table has none of the new bits and passes what they refuse
    plain = R.roi_status(rois, srcs, 3, size).tolist()
    assert plain == [bits & ~(R.BOX_OUTSIDE | R.BAD_SCALE) for bits in want]
    # a slot with a status is zeros; its neighbours are what they are alone
    rng = np.random.default_rng(4)
    pixels = rng.integers(1, 256, size, dtype=np.uint8)
    args = ((OH, OW), 3, [2, 1, 0], [1, 2, 3], [1, 1, 1])
    out, st = R.reference_crop_aa(pixels, srcs, rois, *args)
    assert st.tolist() == want
    for k, bits in enumerate(want):
        assert (out[k] == 0).all() if bits else (out[k] != 0).any(), k
    alone = R.reference_crop_aa(pixels, srcs, rois[8:9], *args)[0]
    assert np.array_equal(out[8], alone[0])
    q, st = R.reference_crop_aa(pixels, srcs, rois, *args, q0=-2)
    assert q.dtype == np.int8 and all((q[k] == 0).all() for k, bits in enumerate(want) if bits) and (q != 0).any()
    # a side of exactly 32 * OW has the longest filter a valid slot can have: hi - lo = trunc(A + 2 * support) - trunc(A) with
    # 2 * support = 64 an integer is 64 taps at every alignment, one below the 2 * 32 + 1 the kernel's coefficient rows hold
    for a0 in (20.0, 20.25, 19.5, 0.0, 40.0):
        assert int(P.aa_coefs_box(200, a0, a0 + 32 * OW, OW)[1].max()) == 2 * P.AA_MAX_SCALE


def test_reference_crop_aa_is_crop_pil_then_mean_and_scale():
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (90, 120, 4), dtype=np.uint8)
    pre = P.SQUEEZENET
    pixels, srcs, pb = P.pack_host([img], pre)
    rois = _rois([(0, 10.5, 20.25, 100.0, 80.75)])
    ch = P.src_channels(pre, "RGBA")
    out, st = R.reference_crop_aa(pixels, srcs, rois, (9, 11), pb, ch, np.float32(pre.mean), np.float32(pre.scale))
    assert st.tolist() == [0]
    res = R.crop_pil(img[:, :, ch], (10.5, 20.25, 100.0, 80.75), 9, 11)
    want = (np.moveaxis(res, 2, 0).astype(np.float32) - np.float32(pre.mean)[:, None, None]) * np.float32(pre.scale)[:, None, None]
    assert np.array_equal(out[0].view(np.uint32), want.view(np.uint32))
    plain = R.reference_crop(pixels, srcs, rois, (9, 11), pb, ch, np.float32(pre.mean), np.float32(pre.scale))[0]
    assert (plain != out).mean() > 0.5                                    # the two-tap rule aliases at 8x


# ---- the library on the CPU: host refusals (fake device pointers, never dereferenced) --------------------------------------------------
@pytest.fixture(scope="module")
def host_net():
    t = cfg.tiny_tables()
    net = NetWork(t)
    net.Quantization(synth.q_text(synth.synth_q_values(t, 1)))
    return net


FAKE = 0x7f0000001000


def _crop(net, desc=None, batch=2, n_slots=3, out_q=1, ptrs=(FAKE,) * 5):
    d = desc if desc is not None else P.desc_of(P.SQUEEZENET, "RGB")
    px, srcs, rois, out, st = ptrs
    code = _lib.lib().tf2_roi_crop_aa(net._h if net is not None else None, C.byref(d) if d is not False else None, px, 1 << 20, srcs, batch,
                                      rois, n_slots, out_q, out, st, None)
    return code, _lib.lib().tf2_last_error().decode()


def _pdesc(**kw):
    d = P.desc_of(P.SQUEEZENET, "RGB")
    for k, v in kw.items():
        if k in ("src_channel", "mean", "scale"):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,message", [
    (dict(desc=_pdesc(size=8)), "desc size"), (dict(desc=False), "null desc"),
    (dict(desc=_pdesc(pixel_bytes=2)), "pixel_bytes"), (dict(desc=_pdesc(pixel_bytes=5)), "pixel_bytes"),
    (dict(desc=_pdesc(src_channel=(1, 3))), "src_channel[1]"), (dict(desc=_pdesc(src_channel=(0, -1))), "src_channel[0]"),
    (dict(desc=_pdesc(mean=(2, float("nan")))), "finite"), (dict(desc=_pdesc(scale=(0, float("inf")))), "finite"),
    (dict(desc=_pdesc(round_resized=2)), "round_resized"),               # still validated, otherwise ignored
    (dict(batch=0), "batch"), (dict(batch=-1), "batch"), (dict(out_q=2), "out_q"),
    (dict(n_slots=0), "n_slots"), (dict(n_slots=-4), "n_slots"),
] + [(dict(ptrs=tuple(None if i == k else FAKE for i in range(5))), "null device pointer") for k in range(5)])
def test_crop_aa_host_refusals(host_net, kw, message):
    st, err = _crop(host_net, **kw)
    assert st == -1 and err.startswith("tf2_roi_crop_aa: ") and message in err, (st, err)


def test_crop_aa_host_refusals_of_the_net():
    st, err = _crop(None)
    assert st == -1 and "null tf2_net" in err
    t4 = cfg.tiny_tables(c0=4)
    net4 = NetWork(t4)
    net4.Quantization(synth.q_text(synth.synth_q_values(t4, 1)))
    st, err = _crop(net4)
    assert st == -1 and "image_c" in err
    bare = NetWork(cfg.tiny_tables())                      # no q table: int8 output refused
    st, err = _crop(bare, out_q=1)
    assert st == -1 and "q table" in err


def test_cropper_antialias_switch(host_net):
    """None follows the preset; the statements follow the choice; antialias=False is the cropper as it was"""
    plain, aa = R.DeviceCropper(host_net, P.SQUEEZENET, "RGB"), R.DeviceCropper(host_net, P.SQUEEZENET, "RGB", antialias=True)
    assert plain.antialias is False and aa.antialias is True
    assert R.DeviceCropper(host_net, P.TORCHVISION_PIL, "RGB").antialias is True
    assert R.DeviceCropper(host_net, P.TORCHVISION_PIL, "RGB", antialias=False).antialias is False
    assert (R.BOX_OUTSIDE, R.BAD_SCALE) == (16, 32)
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (60, 50, 3), dtype=np.uint8)
    pixels, srcs, pb = P.pack_host([img], P.SQUEEZENET)
    rois = _rois([(0, 5.0, 6.0, 45.0, 56.0), (0, -5.0, 6.0, 45.0, 56.0)])
    words = np.ascontiguousarray(srcs).view(np.int32).reshape(1, P.SRC_WORDS)
    args = (plain.out_hw, pb, [2, 1, 0], np.float32(P.SQUEEZENET.mean), np.float32(P.SQUEEZENET.scale), False)
    for c, fn, want_st in ((plain, R.reference_crop, [0, 0]), (aa, R.reference_crop_aa, [0, R.BOX_OUTSIDE])):
        for out, q0 in (("f32", None), ("q", int(host_net.q[0, 0]))):
            got, st = c.reference_crop(pixels, words, rois, out=out)
            want, _ = fn(pixels, srcs, rois, *args, q0)
            assert st.tolist() == want_st and got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def test_roi_crop_aa_kernels_use_no_private_segment_and_bounded_lds():
    import vmcnt_check
    seg, lds, txt = vmcnt_check.kernel_segments("roi_crop_aa")
    names = [k for k in seg if "aa_tile_kernel" in k]
    assert len(names) == 2, seg                                    # int8 / float32 output
    assert all(seg[k] == 0 for k in names), seg
    assert lds and max(lds) <= 16384, lds                          # bounded whatever the scale: coefficients 40 x 65, two chunks
