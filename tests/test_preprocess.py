"""Image preprocessing, CPU side: the statement preprocess.reference against torch's bilinear interpolate (align_corners=False) for
every shape class and preset, the exact identity resize, GOOGLENET's rounding and crop window, TORCHVISION's per-image resize and
centre crop, the device's record validity rule restated in numpy, the host refusals of tf2_preprocess (fake device pointers: a
refusal touches no device) and the scratch-free ISA of preprocess.hip.  The device itself is checked in
tests/test_gpu_preprocess.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tf2_amd import _lib, config as cfg, preprocess as P, synth
from tf2_amd.network import NetWork


def _torch_resize(img, rh, rw):
    """torch's bilinear interpolate (half-pixel centres, edge clamp, no antialiasing) in float64: [C, rh, rw]"""
    x = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1)[None].double()
    return torch.nn.functional.interpolate(x, size=(rh, rw), mode="bilinear", align_corners=False)[0].numpy()


@pytest.mark.parametrize("h,w,rh,rw", [
    (375, 500, 224, 224),     # downscale, non-integer ratios
    (480, 640, 240, 320),     # downscale by exactly 2
    (7, 9, 30, 41),           # upscale, non-integer
    (50, 60, 150, 120),       # upscale by 3 and 2
    (1, 1, 5, 6),             # 1 x 1
    (1, 13, 4, 8),            # 1 x N
    (13, 1, 4, 4),            # N x 1
    (31, 17, 31, 17),         # identity
])
def test_statement_matches_torch_bilinear(h, w, rh, rw):
    rng = np.random.default_rng(h * 1000 + w)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = P.resize_one(img, rh, rw, 0, 0, rh, rw)
    np.testing.assert_allclose(got, _torch_resize(img, rh, rw), rtol=0, atol=1e-3)
    mean, scale = np.float32([104, 117, 123]), np.float32([0.5, 1.0, 1 / 58.0])
    v = (got - mean[:, None, None]) * scale[:, None, None]
    want = (_torch_resize(img, rh, rw) - mean[:, None, None].astype(np.float64)) * scale[:, None, None].astype(np.float64)
    np.testing.assert_allclose(v / scale[:, None, None], want / scale[:, None, None].astype(np.float64), rtol=0, atol=1e-3)


@pytest.mark.parametrize("name", sorted(P.PRESETS))
@pytest.mark.parametrize("hw", [(375, 500), (500, 333), (227, 227), (300, 300), (64, 48)])
def test_every_preset_against_torch(name, hw):
    """reference_images (RGB sources) == torch resize to preset.geometry, crop, channel swap, (rint), mean and scale, within 1e-3
    in 0..255 units"""
    pre = P.PRESETS[name]
    rng = np.random.default_rng([ord(ch) for ch in name] + list(hw))
    img = rng.integers(0, 256, hw + (3,), dtype=np.uint8)
    got = P.reference_images([img], pre, "RGB")[0]
    rh, rw, cy, cx = pre.geometry(*hw)
    oh, ow = pre.out_hw
    r = _torch_resize(img, rh, rw)[:, cy:cy + oh, cx:cx + ow]
    r = r[["RGB".index(c) for c in pre.channels]]
    if pre.round_resized:
        near_half = np.abs(r - np.floor(r) - 0.5) < 1e-3          # where float64 and float32 may round differently
        r = np.clip(np.rint(r), 0, 255)
    else:
        near_half = np.zeros(r.shape, bool)
    m, s = np.float32(pre.mean).astype(np.float64), np.float32(pre.scale).astype(np.float64)
    want = (r - m[:, None, None]) * s[:, None, None]
    err = np.abs(got - want) / s[:, None, None]
    assert err[~near_half].max() < 1e-3, err.max()
    assert near_half.mean() < 0.01


def test_identity_resize_is_exact():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (227, 227, 4), dtype=np.uint8)
    for pre, src in ((P.SQUEEZENET, img), (P.RESNET50, img[:224, :224])):      # 227 / 224 sources: no resize
        got = P.reference_images([src], pre, "RGBA")[0]
        p = np.moveaxis(src[:, :, ["RGBA".index(c) for c in pre.channels]], 2, 0).astype(np.float32)
        want = (p - np.float32(pre.mean)[:, None, None]) * np.float32(pre.scale)[:, None, None]
        assert np.array_equal(got, want)
    # the weights of an identity resize are exactly zero
    for n in (1, 2, 17, 227):
        i0, i1, w = P._taps(n, 0, n, n)
        assert (w == 0).all() and (i0 == np.arange(n)).all()


def test_googlenet_rounds_then_crops_the_centre():
    pre = P.GOOGLENET
    assert pre.geometry(375, 500) == (256, 256, 16, 16) and pre.geometry(256, 256) == (256, 256, 16, 16)
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)
    got = P.reference_images([img], pre, "BGR")[0]                    # BGR source, BGR net: no swap; identity resize
    want = img[16:240, 16:240].transpose(2, 0, 1).astype(np.float32) - np.float32([104, 117, 123])[:, None, None]
    assert np.array_equal(got, want)
    # upscaled sources: every resized value is an integer before the mean
    small = rng.integers(0, 256, (100, 90, 3), dtype=np.uint8)
    out = P.reference_images([small], pre, "BGR")[0] + np.float32([104, 117, 123])[:, None, None]
    assert np.array_equal(out, np.rint(out)) and out.min() >= 0 and out.max() <= 255
    full = P.resize_one(small, 256, 256, 0, 0, 256, 256, round_resized=True)
    assert np.array_equal(out, full[:, 16:240, 16:240])
    # rint is half to even: 0.5 -> 0, 1.5 -> 2 (a 1 x 2 row 0, 1 resized to 1 x 4 has weights 0.25 / 0.75 ...; 0 / 3 to 1 x 2 ...)
    two = np.array([[[0, 0, 0], [1, 1, 1]]], np.uint8)
    r = P.resize_one(two, 1, 4, 0, 0, 1, 4, round_resized=True)[0, 0]
    assert r.tolist() == [0.0, 0.0, 1.0, 1.0]                        # 0, 0.25, 0.75, 1 -> 0, 0, 1, 1
    mid = np.array([[[1, 1, 1], [2, 2, 2]], [[1, 1, 1], [2, 2, 2]]], np.uint8)
    assert P.resize_one(mid, 2, 1, 0, 0, 2, 1, round_resized=True)[0, :, 0].tolist() == [2.0, 2.0]   # 1.5 -> 2


@pytest.mark.parametrize("hw,want", [
    ((375, 500), (256, 341, 16, 58)),      # landscape: (341 - 224) / 2 = 58.5 rounds half to even
    ((500, 375), (341, 256, 58, 16)),
    ((256, 256), (256, 256, 16, 16)),
    ((224, 300), (256, 342, 16, 59)),      # upscale: int(256 * 300 / 224) = 342
    ((480, 640), (256, 341, 16, 58)),
    ((333, 500), (256, 384, 16, 80)),
])
def test_torchvision_geometry(hw, want):
    assert P.TORCHVISION.geometry(*hw) == want


def test_torchvision_per_image_records():
    rng = np.random.default_rng(2)
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((375, 500), (500, 333), (224, 224))]
    pixels, srcs, pb = P.pack_host(imgs, P.TORCHVISION, align=16)
    assert pb == 3 and pixels.size == sum(h * (-(-w * 3 // 16) * 16) for h, w in ((375, 500), (500, 333), (224, 224)))
    for im, r in zip(imgs, srcs):
        h, w = im.shape[:2]
        assert (r["h"], r["w"]) == (h, w) and r["row_pitch"] % 16 == 0 and r["row_pitch"] >= 3 * w
        assert tuple(int(r[k]) for k in ("resize_h", "resize_w", "crop_y", "crop_x")) == P.TORCHVISION.geometry(h, w)
    assert (P.record_status(srcs, 3, pixels.size, (224, 224)) == 0).all()
    # the packed buffer, read through the records, gives what each image alone gives
    out, st = P.reference(pixels, srcs, (224, 224), 3, [0, 1, 2], P.TORCHVISION.mean, P.TORCHVISION.scale)
    for b, im in enumerate(imgs):
        assert np.array_equal(out[b], P.reference_images([im], P.TORCHVISION, "RGB")[0])


def test_torchvision_constants():
    m, s = np.float32(P.TORCHVISION.mean), np.float32(P.TORCHVISION.scale)
    assert np.allclose(m, 255 * np.float64([0.485, 0.456, 0.406])) and np.allclose(s, 1 / (255 * np.float64([0.229, 0.224, 0.225])))
    assert np.float32(P.SQUEEZENET.scale[0]) == np.float32(2.0 ** -7)


def _rec(**kw):
    r = dict(offset=0, h=10, w=8, row_pitch=24, resize_h=4, resize_w=4, crop_y=0, crop_x=0, reserved=0)
    r.update(kw)
    return np.array([tuple(r[k] for k in P.SRC_DTYPE.names)], P.SRC_DTYPE)


@pytest.mark.parametrize("change,bits", [
    (dict(), 0),
    (dict(h=0), P.BAD_SIZE), (dict(w=0), P.BAD_SIZE | 0), (dict(h=32768), P.BAD_SIZE), (dict(w=-3), P.BAD_SIZE),
    (dict(row_pitch=23), P.BAD_PITCH),
    (dict(offset=-1), P.BAD_OFFSET),
    (dict(offset=1), P.OUT_OF_BUFFER),                               # last row ends one byte past pixels_bytes (240)
    (dict(h=11), P.OUT_OF_BUFFER),
    (dict(offset=2**62), P.OUT_OF_BUFFER),
    (dict(resize_h=0), P.BAD_RESIZE | P.BAD_CROP), (dict(resize_w=32768), P.BAD_RESIZE),
    (dict(crop_y=1), P.BAD_CROP), (dict(crop_x=-1), P.BAD_CROP), (dict(resize_w=3), P.BAD_CROP),
    (dict(h=0, row_pitch=2, offset=-5), P.BAD_SIZE | P.BAD_OFFSET),     # w = 8: pitch 2 < 24 too
    (dict(row_pitch=24, h=1, w=8, offset=216), 0),                   # the last 24 bytes exactly
])
def test_record_validity_rule(change, bits):
    pitch_bad = P.BAD_PITCH if change.get("row_pitch", 24) < change.get("w", 8) * 3 else 0
    want = bits | pitch_bad
    assert P.record_status(_rec(**change), 3, 240, (4, 4))[0] == want


def test_validity_rule_pixel_bytes_4():
    r = _rec(row_pitch=32, w=8, h=10)                                # 10 rows of 32 bytes: 9 * 32 + 32 = 320
    assert P.record_status(r, 4, 320, (4, 4))[0] == 0
    assert P.record_status(r, 4, 319, (4, 4))[0] == P.OUT_OF_BUFFER
    assert P.record_status(r, 3, 312, (4, 4))[0] == 0                 # 9 * 32 + 24
    assert P.record_status(r, 3, 311, (4, 4))[0] == P.OUT_OF_BUFFER


def test_malformed_records_give_zeros_and_read_nothing():
    """the statement reads no pixel of a malformed record: its output is zero even where valid neighbours are not"""
    rng = np.random.default_rng(4)
    pixels = rng.integers(0, 256, 240, dtype=np.uint8)
    recs = np.concatenate([_rec(), _rec(offset=1), _rec(crop_y=1)])
    out, st = P.reference(pixels, recs, (4, 4), 3, [2, 1, 0], [1, 2, 3], [1, 1, 1])
    assert st.tolist() == [0, P.OUT_OF_BUFFER, P.BAD_CROP]
    assert (out[1:] == 0).all() and (out[0] != 0).any()
    q, st = P.reference(pixels, recs, (4, 4), 3, [2, 1, 0], [1, 2, 3], [1, 1, 1], q0=-2)
    assert q.dtype == np.int8 and (q[1:] == 0).all()


def test_quant_input_rule():
    v = np.float32([0.0, 0.49, 0.5, -0.5, 1.5, -1.5, 2.5, 126.6, 127.5, 300.0, -128.4, -129, 3e9, -3e9])
    got = P.quant_input(v, 1.0).tolist()
    assert got == [0, 0, 1, -1, 2, -2, 3, 127, 127, 127, -128, -128, -128, -128]
    assert P.quant_input(np.float32([1.25]), 2.0 ** 1).tolist() == [3]          # 2.5 rounds away from zero
    assert P.trans_of(-2) == 4.0 and P.trans_of(3) == 0.125


@pytest.fixture(scope="module")
def host_net():
    t = cfg.tiny_tables()
    q = synth.synth_q_values(t, 1)
    net = NetWork(t)
    net.Quantization(synth.q_text(q))
    return net


FAKE = 0x7f0000001000      # never dereferenced: every case is refused before a device call


def _call(net, desc=None, batch=2, out_q=1, ptrs=(FAKE, FAKE, FAKE, FAKE)):
    d = desc if desc is not None else P.desc_of(P.RESNET50, "RGB")
    px, srcs, out, st = ptrs
    return _lib.lib().tf2_preprocess(net._h if net is not None else None, C.byref(d) if d is not False else None, px, 1 << 20, srcs,
                                     batch, out_q, out, st, None)


def _desc(**kw):
    d = P.desc_of(P.RESNET50, "RGB")
    for k, v in kw.items():
        if k in ("src_channel", "mean", "scale"):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,message", [
    (dict(desc=_desc(size=8)), "desc size"),
    (dict(desc=False), "null desc"),
    (dict(desc=_desc(pixel_bytes=2)), "pixel_bytes"), (dict(desc=_desc(pixel_bytes=5)), "pixel_bytes"),
    (dict(desc=_desc(src_channel=(1, 3))), "src_channel[1]"),
    (dict(desc=_desc(src_channel=(0, -1))), "src_channel[0]"),
    (dict(desc=_desc(mean=(2, float("nan")))), "finite"), (dict(desc=_desc(scale=(0, float("inf")))), "finite"),
    (dict(desc=_desc(round_resized=2)), "round_resized"),
    (dict(batch=0), "batch"), (dict(batch=-1), "batch"),
    (dict(out_q=2), "out_q"),
    (dict(ptrs=(None, FAKE, FAKE, FAKE)), "null device pointer"), (dict(ptrs=(FAKE, None, FAKE, FAKE)), "null device pointer"),
    (dict(ptrs=(FAKE, FAKE, None, FAKE)), "null device pointer"), (dict(ptrs=(FAKE, FAKE, FAKE, None)), "null device pointer"),
])
def test_host_refusals(host_net, kw, message):
    st = _call(host_net, **kw)
    err = _lib.lib().tf2_last_error().decode()
    assert st == -1 and message in err, (st, err)


def test_host_refusals_of_the_net():
    assert _call(None) == -1 and "null tf2_net" in _lib.lib().tf2_last_error().decode()
    t4 = cfg.tiny_tables(c0=4)
    net4 = NetWork(t4)
    net4.Quantization(synth.q_text(synth.synth_q_values(t4, 1)))
    assert _call(net4) == -1 and "image_c" in _lib.lib().tf2_last_error().decode()
    bare = NetWork(cfg.tiny_tables())                      # no q table: float output is fine to check, int8 output refused
    assert _call(bare, out_q=1) == -1 and "q table" in _lib.lib().tf2_last_error().decode()


def test_src_channels_and_desc():
    assert P.src_channels(P.RESNET50, "RGB") == [2, 1, 0] and P.src_channels(P.RESNET50, "BGR") == [0, 1, 2]
    assert P.src_channels(P.TORCHVISION, "BGRA") == [2, 1, 0] and P.src_channels(P.SSD300, "RGBA") == [2, 1, 0]
    d = P.desc_of(P.GOOGLENET, "BGRA")
    assert d.size == C.sizeof(_lib.PreprocessDesc) == 48 and d.pixel_bytes == 4 and d.round_resized == 1
    assert C.sizeof(_lib.ImageSrc) == P.SRC_DTYPE.itemsize == 40


def test_preprocess_kernels_compile_without_scratch():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import vmcnt_check
    seg, lds, txt = vmcnt_check.kernel_segments("preprocess")
    names = [k for k in seg if "preprocess_kernel" in k]
    assert len(names) == 4, seg                                    # int8 / float32 output, vector / byte stores
    assert all(seg[k] == 0 for k in names), seg
    assert "scratch_" not in txt.split("amdhsa.kernels")[0]
