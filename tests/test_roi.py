"""Second-stage crops, CPU side: the statement roi.reference_select on hand-worked cases (the order on tied scores, the strict
min_score, the class mask, counts above top_k, NaN / inf / clipped-away boxes, square, expand, empty images), reference_crop on
whole-image ROIs against preprocess.reference bit for bit, a hand-worked crop, the slot validity rule, the host refusals of
tf2_roi_select / tf2_roi_crop (fake device pointers: a refusal touches no device) and the scratch-free ISA of roi_crop.hip.  The
device itself is checked in tests/test_gpu_roi.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tf2_amd import _lib, config as cfg, preprocess as P, roi as R, synth
from tf2_amd.network import NetWork


def _srcs(*hw):
    s = np.zeros(len(hw), P.SRC_DTYPE)
    for i, (h, w) in enumerate(hw):
        s[i] = (0, h, w, 3 * w, h, w, 0, 0, 0)
    return s


def _det(B, Cn, K):
    return np.zeros((B, Cn, K, 5), np.float32), np.zeros((B, Cn), np.int32)


def _put(det, counts, b, c, rows):
    """rows of (score, x1, y1, x2, y2) into det[b, c], counts[b, c] = their number"""
    det[b, c, :len(rows)] = np.float32(rows)
    counts[b, c] = len(rows)


def _table(rois):
    return [(int(r["image"]), int(r["cls"]), int(r["rank"]), float(r["score"]), float(r["x0"]), float(r["y0"]), float(r["x1"]), float(r["y1"]))
            for r in rois]


EMPTY = (-1, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)


def test_record_layout():
    assert R.ROI_DTYPE.itemsize == C.sizeof(_lib.Roi) == 32 and R.ROI_WORDS == 8
    assert [R.ROI_DTYPE.fields[n][1] for n in R.ROI_DTYPE.names] == [getattr(_lib.Roi, n).offset for n in R.ROI_DTYPE.names]
    assert C.sizeof(_lib.RoiDesc) == 68
    assert (R.EMPTY, R.BAD_IMAGE, R.BAD_BOX, R.BAD_SRC) == (1, 2, 4, 8)


def test_select_order_on_tied_scores_and_the_strict_threshold():
    """a 100 x 200 source; exact binary fractions, so every product below is exact"""
    det, counts = _det(1, 4, 3)
    box = (0.25, 0.25, 0.75, 0.5)                              # -> (50, 25, 150, 50)
    _put(det, counts, 0, 1, [(0.75,) + box, (0.5,) + box, (0.5,) + box])
    _put(det, counts, 0, 2, [(0.875,) + box, (0.5,) + box])
    _put(det, counts, 0, 3, [(0.5,) + box, (0.25,) + box])    # 0.25 is not > 0.25
    rois, n = R.reference_select(det, counts, _srcs((100, 200)), classes=(1, 2, 3), min_score=0.25, max_rois=8)
    px = (50.0, 25.0, 150.0, 50.0)
    assert n.tolist() == [6]
    assert _table(rois) == [(0, 2, 0, 0.875) + px, (0, 1, 0, 0.75) + px, (0, 1, 1, 0.5) + px, (0, 1, 2, 0.5) + px, (0, 2, 1, 0.5) + px,
                            (0, 3, 0, 0.5) + px, EMPTY, EMPTY]
    # fewer slots than candidates: the best three, in the same order; the class mask takes class 2 out
    rois, n = R.reference_select(det, counts, _srcs((100, 200)), classes=(1, 3), min_score=0.25, max_rois=3)
    assert n.tolist() == [3] and [t[:3] for t in _table(rois)] == [(0, 1, 0), (0, 1, 1), (0, 1, 2)]
    # a NaN score never passes; +inf is the best score there is
    det[0, 1, 0, 0], det[0, 3, 1, 0] = np.nan, np.inf
    rois, n = R.reference_select(det, counts, _srcs((100, 200)), classes=(1, 2, 3), min_score=0.25, max_rois=2)
    assert [t[:3] for t in _table(rois)] == [(0, 3, 1), (0, 2, 0)] and np.isposinf(rois[0]["score"])


def test_select_counts_above_top_k_and_below_the_rows():
    det, counts = _det(2, 3, 2)
    box = (0.0, 0.0, 1.0, 1.0)
    det[:, 1:, :, 0] = 0.5
    det[:, 1:, :, 1:] = box
    counts[0] = (0, 7, 1)                                      # 7 > top_k = 2: both rows; 1: the first row only
    counts[1] = (0, -3, 0)                                     # nothing, whatever the rows hold
    rois, n = R.reference_select(det, counts, _srcs((10, 10), (10, 10)), classes=(1, 2), min_score=0.0, max_rois=4)
    assert n.tolist() == [3, 0]
    assert [t[:3] for t in _table(rois)] == [(0, 1, 0), (0, 1, 1), (0, 2, 0)] + [EMPTY[:3]] * 5


def test_select_skips_boxes_that_are_not_usable():
    det, counts = _det(1, 2, 8)
    _put(det, counts, 0, 1, [
        (0.9, np.nan, 0.0, 1.0, 1.0),                          # NaN coordinate
        (0.8, 0.0, 0.0, np.inf, 1.0),                          # inf coordinate
        (0.7, 1.5, 0.0, 2.5, 1.0),                             # wholly right of the image: clip leaves (w, w)
        (0.6, 0.0, 0.0, 0.015625, 1.0),                        # 64 * 1/64 = 1 px wide: kept
        (0.5, 0.0, 0.0, 0.0078125, 1.0),                       # half a pixel wide
        (0.4, 0.75, 0.5, 0.25, 1.0),                           # x2 < x1: negative width
        (0.3, -0.5, 0.0, 0.0078125, 1.0),                      # clip shrinks it from 32.5 px to half a pixel
        (0.2, -0.5, -0.5, 1.5, 1.5),                           # larger than the image: clipped to it
    ])
    rois, n = R.reference_select(det, counts, _srcs((32, 64)), classes=(1,), min_score=0.1, max_rois=8, clip=True)
    assert n.tolist() == [2]
    f32 = lambda v: float(np.float32(v))
    assert _table(rois)[:2] == [(0, 1, 3, f32(0.6), 0.0, 0.0, 1.0, 32.0), (0, 1, 7, f32(0.2), 0.0, 0.0, 64.0, 32.0)]
    rois, n = R.reference_select(det, counts, _srcs((32, 64)), classes=(1,), min_score=0.1, max_rois=8, clip=False)
    assert [t[2] for t in _table(rois)[:int(n[0])]] == [2, 3, 6, 7]
    assert _table(rois)[0][4:] == (96.0, 0.0, 160.0, 32.0) and _table(rois)[2][4:] == (-32.0, 0.0, 0.5, 32.0)
    assert _table(rois)[3][4:] == (-32.0, -16.0, 96.0, 48.0)


def test_select_square_and_expand():
    det, counts = _det(1, 2, 1)
    _put(det, counts, 0, 1, [(0.5, 0.25, 0.25, 0.75, 0.5)])   # (50, 25, 150, 50) of a 100 x 200 source: 100 x 25, centre (100, 37.5)
    src = _srcs((100, 200))
    one = lambda **kw: _table(R.reference_select(det, counts, src, classes=(1,), min_score=0.0, max_rois=1, **kw)[0])[0][4:]
    assert one(clip=False) == (50.0, 25.0, 150.0, 50.0)
    assert one(clip=False, square=True) == (50.0, -12.5, 150.0, 87.5)
    assert one(clip=True, square=True) == (50.0, 0.0, 150.0, 87.5)
    assert one(clip=False, expand=(1.5, 2.0)) == (25.0, 12.5, 175.0, 62.5)
    assert one(clip=False, expand=(0.5, 8.0), square=True) == (0.0, -62.5, 200.0, 137.5)      # 50 x 200 -> 200 x 200
    assert one(clip=True, expand=(4.0, 4.0)) == (0.0, 0.0, 200.0, 87.5)
    # the rounding to float32 is the only one: 1/3 of 200 in double, then float32
    _put(det, counts, 0, 1, [(0.5, np.float32(1 / 3), 0.0, 1.0, 1.0)])
    assert one()[0] == float(np.float32(np.float64(np.float32(1 / 3)) * 200.0))


def test_select_empty_images_and_malformed_sources():
    det, counts = _det(4, 2, 2)
    for b in range(4):
        _put(det, counts, b, 1, [(0.5, 0.0, 0.0, 1.0, 1.0)])
    counts[1] = 0                                              # image 1 has no detection
    srcs = _srcs((10, 20), (10, 20), (0, 20), (10, 32768))     # images 2 and 3: sizes outside 1..32767
    rois, n = R.reference_select(det, counts, srcs, classes=(1,), min_score=0.0, max_rois=2)
    assert n.tolist() == [1, 0, 0, 0]
    assert _table(rois) == [(0, 1, 0, 0.5, 0.0, 0.0, 20.0, 10.0)] + [EMPTY] * 7
    assert (R.roi_status(rois, srcs, 3, 10 * 60) == [0] + [R.EMPTY] * 7).all()


@pytest.mark.parametrize("name", sorted(P.PRESETS))
@pytest.mark.parametrize("hw", [(375, 500), (500, 333), (227, 227), (300, 300), (64, 48)])
def test_whole_image_roi_is_preprocess(name, hw):
    """reference_crop on (0, 0, w, h) == preprocess.reference with resize = out_hw and crop (0, 0), bit for bit, float32 and int8"""
    pre = P.PRESETS[name]
    rng = np.random.default_rng([ord(ch) for ch in name] + list(hw))
    img = rng.integers(0, 256, hw + (3,), dtype=np.uint8)
    pixels, srcs, pb = P.pack_host([img], pre, align=4)
    oh, ow = pre.out_hw
    srcs["resize_h"], srcs["resize_w"], srcs["crop_y"], srcs["crop_x"] = oh, ow, 0, 0
    args = (pre.out_hw, pb, P.src_channels(pre, "RGB"), np.float32(pre.mean), np.float32(pre.scale), pre.round_resized)
    rois = R.whole_image_rois(srcs)
    assert _table(rois) == [(0, 0, 0, 0.0, 0.0, 0.0, float(hw[1]), float(hw[0]))]
    for q0 in (None, -1):
        want, wst = P.reference(pixels, srcs, *args, q0)
        got, st = R.reference_crop(pixels, srcs, rois, *args, q0)
        assert wst.tolist() == [0] and st.tolist() == [0]
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert len(np.unique(got)) > 4


def test_crop_by_hand():
    """a 4 x 4 one-byte-a-channel ramp: the ROI (1, 1, 3, 3) at 2 x 2 samples the centres of pixels (1..2, 1..2) exactly; at 4 x 4 it
    interpolates between them; a ROI outside the image reads the edge"""
    img = (np.arange(16, dtype=np.uint8).reshape(4, 4, 1) * 4).repeat(3, axis=2)
    pixels, srcs, pb = P.pack_host([img], P.SQUEEZENET)
    rois = R.whole_image_rois(srcs).repeat(3)
    rois[0]["x0"], rois[0]["y0"], rois[0]["x1"], rois[0]["y1"] = 1, 1, 3, 3
    rois[1]["x0"], rois[1]["y0"], rois[1]["x1"], rois[1]["y1"] = -9, -9, -5, -5        # wholly outside: pixel (0, 0) everywhere
    rois[2]["x0"], rois[2]["y0"], rois[2]["x1"], rois[2]["y1"] = 3, 0, 7, 4             # the right half is outside: column 3 repeated
    kw = dict(pixel_bytes=pb, src_channel=[0, 1, 2], mean=[0, 0, 0], scale=[1, 1, 1])
    out, st = R.reference_crop(pixels, srcs, rois, (2, 2), **kw)
    assert st.tolist() == [0, 0, 0]
    assert out[0, 0].tolist() == [[20.0, 24.0], [36.0, 40.0]] and (out[1] == 0).all()
    assert out[2, 0].tolist() == [[20.0, 20.0], [52.0, 52.0]]                         # rows 0.5 and 2.5: halfway (12, 28) and (44, 60)
    out, st = R.reference_crop(pixels, srcs, rois[:1], (4, 4), **kw)
    assert out[0, 0, 0].tolist() == [15.0, 17.0, 19.0, 21.0]                          # centres 1.25, 1.75.. -> 0.75, 1.25.. of the ramp
    assert out[0, 0, :, 0].tolist() == [15.0, 23.0, 31.0, 39.0]


def test_slot_validity_rule():
    srcs = _srcs((10, 8), (10, 8), (10, 8))
    srcs[1]["row_pitch"] = 23                                  # BAD_PITCH
    srcs[2]["offset"] = 1                                      # one byte past the 240-byte buffer
    srcs[0]["resize_h"], srcs[0]["crop_x"] = 0, -5             # not read
    good = (0.0, 0.0, 8.0, 10.0)
    cases = [
        ((0,) + good, 0), ((-1,) + good, R.EMPTY), ((-1, np.nan, 0, 0, 0), R.EMPTY),
        ((3,) + good, R.BAD_IMAGE), ((-2,) + good, R.BAD_IMAGE), ((2 ** 31 - 1,) + good, R.BAD_IMAGE),
        ((0, 0.0, 0.0, 0.5, 10.0), R.BAD_BOX), ((0, 0.0, 0.0, 8.0, np.inf), R.BAD_BOX), ((0, np.nan, 0.0, 8.0, 10.0), R.BAD_BOX),
        ((0, 5.0, 0.0, 4.0, 10.0), R.BAD_BOX), ((0, 2.0, 3.0, 3.0, 4.0), 0),
        ((0, -3e38, 0.0, 3e38, 10.0), 0),                      # finite in float32, and the side is taken in double
        ((1,) + good, R.BAD_SRC), ((2,) + good, R.BAD_SRC), ((1, 0.0, 0.0, 0.0, 0.0), R.BAD_SRC | R.BAD_BOX),
        ((7, 0.0, 0.0, 0.0, 0.0), R.BAD_IMAGE | R.BAD_BOX),
    ]
    rois = np.zeros(len(cases), R.ROI_DTYPE)
    for k, ((image, x0, y0, x1, y1), _) in enumerate(cases):
        rois[k] = (image, 1, 0, 0.5, x0, y0, x1, y1)
    assert R.roi_status(rois, srcs, 3, 240).tolist() == [bits for _, bits in cases]
    # slots with a status are zeros and read nothing; their neighbours are what they are alone
    rng = np.random.default_rng(4)
    pixels = rng.integers(1, 256, 240, dtype=np.uint8)
    out, st = R.reference_crop(pixels, srcs, rois, (4, 4), 3, [2, 1, 0], [1, 2, 3], [1, 1, 1])
    for k, (_, bits) in enumerate(cases):
        assert st[k] == bits and ((out[k] == 0).all() if bits else (out[k] != 0).any())
    alone = R.reference_crop(pixels, srcs, rois[10:11], (4, 4), 3, [2, 1, 0], [1, 2, 3], [1, 1, 1])[0]
    assert np.array_equal(out[10], alone[0])
    q, st = R.reference_crop(pixels, srcs, rois, (4, 4), 3, [2, 1, 0], [1, 2, 3], [1, 1, 1], q0=-2)
    assert q.dtype == np.int8 and all((q[k] == 0).all() for k, (_, bits) in enumerate(cases) if bits)


@pytest.fixture(scope="module")
def host_net():
    t = cfg.tiny_tables()
    net = NetWork(t)
    net.Quantization(synth.q_text(synth.synth_q_values(t, 1)))
    return net


FAKE = 0x7f0000001000      # never dereferenced: every case is refused before a device call


def _roi_desc(**kw):
    d = _lib.RoiDesc()
    d.size = C.sizeof(_lib.RoiDesc)
    d.num_classes, d.top_k, d.min_score, d.max_rois, d.expand_w, d.expand_h, d.square, d.clip = 21, 200, 0.5, 4, 1.0, 1.0, 0, 1
    d.class_mask[0] = 1 << 15
    for k, v in kw.items():
        if k == "mask":
            for i in range(8):
                d.class_mask[i] = v[i] if i < len(v) else 0
        else:
            setattr(d, k, v)
    return d


def _select(desc=None, batch=2, ptrs=(FAKE,) * 5):
    d = desc if desc is not None else _roi_desc()
    st = _lib.lib().tf2_roi_select(C.byref(d) if d is not False else None, ptrs[0], ptrs[1], ptrs[2], batch, ptrs[3], ptrs[4], None)
    return st, _lib.lib().tf2_last_error().decode()


@pytest.mark.parametrize("kw,message", [
    (dict(desc=False), "null desc"), (dict(desc=_roi_desc(size=64)), "desc size"),
    (dict(desc=_roi_desc(num_classes=1)), "num_classes"), (dict(desc=_roi_desc(num_classes=257)), "num_classes"),
    (dict(desc=_roi_desc(top_k=0)), "top_k"), (dict(desc=_roi_desc(top_k=257)), "top_k"),
    (dict(desc=_roi_desc(max_rois=0)), "max_rois"), (dict(desc=_roi_desc(max_rois=65)), "max_rois"),
    (dict(desc=_roi_desc(mask=[0])), "class_mask is empty"), (dict(desc=_roi_desc(mask=[1 | 1 << 15])), "class 0"),
    (dict(desc=_roi_desc(mask=[1 << 21])), "class 21"), (dict(desc=_roi_desc(mask=[1 << 15, 0, 0, 0, 0, 0, 0, 1 << 31])), "class 255"),
    (dict(desc=_roi_desc(min_score=-0.5)), "min_score"), (dict(desc=_roi_desc(min_score=float("nan"))), "min_score"),
    (dict(desc=_roi_desc(min_score=float("inf"))), "min_score"),
    (dict(desc=_roi_desc(expand_w=0.0)), "expand"), (dict(desc=_roi_desc(expand_h=-1.0)), "expand"),
    (dict(desc=_roi_desc(expand_w=float("inf"))), "expand"), (dict(desc=_roi_desc(expand_h=float("nan"))), "expand"),
    (dict(desc=_roi_desc(square=2)), "square"), (dict(desc=_roi_desc(clip=-1)), "clip"),
    (dict(batch=0), "batch"),
] + [(dict(ptrs=tuple(None if i == k else FAKE for i in range(5))), "null device pointer") for k in range(5)])
def test_select_host_refusals(kw, message):
    st, err = _select(**kw)
    assert st == -1 and err.startswith("tf2_roi_select: ") and message in err, (st, err)


def test_select_accepts_the_limits_of_the_desc():
    """the largest desc passes every check and is refused for its batch only"""
    d = _roi_desc(num_classes=256, top_k=256, max_rois=64, min_score=0.0, mask=[0xfffffffe] + [0xffffffff] * 7, square=1, clip=0)
    st, err = _select(desc=d, batch=0)
    assert st == -1 and "batch" in err
    with pytest.raises(ValueError):
        R.class_mask((0,), 21)
    with pytest.raises(ValueError):
        R.class_mask((21,), 21)
    with pytest.raises(ValueError):
        R.class_mask((), 21)
    assert R.class_mask((15, 40), 41) == [1 << 15, 1 << 8, 0, 0, 0, 0, 0, 0]


def _crop(net, desc=None, batch=2, n_slots=3, out_q=1, ptrs=(FAKE,) * 5):
    d = desc if desc is not None else P.desc_of(P.SQUEEZENET, "RGB")
    px, srcs, rois, out, st = ptrs
    code = _lib.lib().tf2_roi_crop(net._h if net is not None else None, C.byref(d) if d is not False else None, px, 1 << 20, srcs, batch,
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
    (dict(desc=_pdesc(round_resized=2)), "round_resized"),
    (dict(batch=0), "batch"), (dict(batch=-1), "batch"), (dict(out_q=2), "out_q"),
    (dict(n_slots=0), "n_slots"), (dict(n_slots=-4), "n_slots"),
] + [(dict(ptrs=tuple(None if i == k else FAKE for i in range(5))), "null device pointer") for k in range(5)])
def test_crop_host_refusals(host_net, kw, message):
    st, err = _crop(host_net, **kw)
    assert st == -1 and err.startswith("tf2_roi_crop: ") and message in err, (st, err)


def test_crop_host_refusals_of_the_net():
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


def test_cropper_takes_the_presets_constants_not_its_geometry(host_net):
    c = R.DeviceCropper(host_net, P.GOOGLENET, "BGRA", classes=(3, 15), min_score=0.25, max_rois=7, expand=(1.5, 1.25), square=True,
                        clip=False)
    assert c.desc.pixel_bytes == 4 and c.desc.round_resized == 1 and list(c.desc.src_channel) == P.src_channels(P.GOOGLENET, "BGRA")
    assert c.out_hw == (int(host_net._nd.image_h), int(host_net._nd.image_w))     # the net's input, not the preset's 224
    d = c.roi_desc
    assert (d.size, d.num_classes, d.top_k, d.max_rois, d.square, d.clip) == (68, 21, 200, 7, 1, 0)
    assert list(d.class_mask) == [1 << 3 | 1 << 15] + [0] * 7 and (d.min_score, d.expand_w, d.expand_h) == (0.25, 1.5, 1.25)


def test_roi_kernels_compile_without_scratch():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import vmcnt_check
    seg, lds, txt = vmcnt_check.kernel_segments("roi_crop")
    names = [k for k in seg if "roi_" in k]
    assert len(names) == 5, seg                                    # select; crop: int8 / float32 output, vector / byte stores
    assert sum("roi_select_kernel" in k for k in names) == 1 and sum("roi_crop_kernel" in k for k in names) == 4
    assert all(seg[k] == 0 for k in names), seg
