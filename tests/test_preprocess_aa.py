"""The statement of the antialiased resize (tf2_amd.preprocess: resize_pil, reference_aa, record_status_aa; tf2_preprocess_aa on
the device): byte-identical to Pillow's recorded output (tests/golden/pil_resize.npz, tools/gen_pil_resize_golden.py) and to a live
Pillow where one is installed, within one grey level of torch's antialiased interpolate, the window form against the crop of the whole
resize, identity against the plain statement, the scale bit of the validity rule, the host refusals of tf2_preprocess_aa (fake device
pointers: a refusal touches no device), the presets, and the scratch-free ISA of preprocess_aa.hip.  The device itself is checked in
tests/test_gpu_preprocess_aa.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from tf2_amd import _lib, config as cfg, preprocess as P, synth
from tf2_amd.network import NetWork

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_pil_resize_golden as golden  # noqa: E402


@pytest.fixture(scope="module")
def golden_cases():
    return golden.load(os.path.join(ROOT, "tests", "golden", "pil_resize.npz"))


def test_resize_pil_is_pillows_recorded_bytes(golden_cases):
    cases, version = golden_cases
    assert len(cases) >= 20 and version
    kinds = set()
    for seed, kind, h, w, rh, rw, want in cases:
        got = P.resize_pil(golden.case_image(seed, kind, h, w), rh, rw)
        assert got.dtype == np.uint8 and got.shape == (rh, rw, 3)
        assert np.array_equal(got, want), (seed, kind, h, w, rh, rw, np.argwhere(got != want)[:4])   # (all-255: whatever Pillow recorded)
        kinds.add(kind)
    assert kinds == {golden.RANDOM, golden.ALL_255, golden.CHECKER, golden.BINARY}
    geo = [(h, w, rh, rw) for _, _, h, w, rh, rw, _ in cases]
    assert any(h == 32 * rh for h, w, rh, rw in geo) and any(w == 32 * rw for h, w, rh, rw in geo)      # exactly 32x
    assert any((h, w) == (1, 1) for h, w, rh, rw in geo) and any(h == 1 and w > 1 for h, w, rh, rw in geo)
    assert any(w == 1 and h > 1 for h, w, rh, rw in geo) and any((h, w) == (rh, rw) for h, w, rh, rw in geo)
    assert any(h < rh and w > rw for h, w, rh, rw in geo) and any(h > rh and w < rw for h, w, rh, rw in geo)


def test_resize_pil_is_a_live_pillow_where_installed():
    """an extra check where PIL imports (the recorded bytes above are the one that never skips)"""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(21)
    geo = [(375, 500, 256, 341), (1, 1, 9, 4), (1, 40, 7, 90), (40, 1, 90, 7), (96, 64, 3, 2), (64, 64, 64, 64)]
    while len(geo) < 30:
        h, w, rh, rw = (int(v) for v in rng.integers(1, 160, 4))
        if h <= 32 * rh and w <= 32 * rw:
            geo.append((h, w, rh, rw))
    for i, (h, w, rh, rw) in enumerate(geo):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if i % 4 else (rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255)
        want = np.asarray(Image.fromarray(img.astype(np.uint8), "RGB").resize((rw, rh), Image.BILINEAR))
        assert np.array_equal(P.resize_pil(img, rh, rw), want), (h, w, rh, rw)


TORCH_GEOMETRIES = [(480, 640, 300, 300), (375, 500, 256, 341), (500, 375, 341, 256), (97, 131, 64, 64), (131, 97, 50, 71), (64, 64, 64, 64),
                    (30, 40, 75, 111), (1, 1, 8, 8), (1, 50, 20, 33), (50, 1, 33, 20), (60, 200, 150, 90), (200, 60, 90, 150),
                    (320, 320, 10, 10), (100, 100, 99, 101), (256, 256, 128, 128), (33, 65, 17, 31), (199, 211, 97, 89)]


@pytest.mark.parametrize("h,w,rh,rw", TORCH_GEOMETRIES)
def test_statement_against_torch_antialiased_bilinear(h, w, rh, rw):
    """An independent implementation that needs no Pillow: torch's uint8 channels_last interpolate(bilinear, antialias=True) on the CPU.
    It keeps fewer coefficient bits, so single grey levels differ: at most 1 everywhere, and on at most 5 % of the bytes of a
    uniform-random image."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(h * 1000 + w + rh)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    x = torch.from_numpy(img).permute(2, 0, 1)[None].contiguous(memory_format=torch.channels_last)
    want = F.interpolate(x, size=(rh, rw), mode="bilinear", antialias=True)[0].permute(1, 2, 0).numpy()
    got = P.resize_pil(img, rh, rw)
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"{h}x{w} -> {rh}x{rw}: max diff {diff.max()}, differing {100.0 * (diff != 0).mean():.3f} %")
    assert diff.max() <= 1
    assert (diff != 0).mean() <= 0.05


def test_window_is_the_crop_of_the_whole_resize():
    rng = np.random.default_rng(2)
    for h, w, rh, rw in [(97, 131, 40, 57), (20, 31, 45, 64), (64, 30, 2, 45), (50, 50, 50, 50)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        whole = P.resize_pil(img, rh, rw)
        ho, wo = max(rh // 2, 1), max(rw // 3, 1)
        for y0, x0 in [(0, 0), (0, rw - wo), (rh - ho, 0), (rh - ho, rw - wo), ((rh - ho) // 2, (rw - wo) // 2)]:   # every edge, and none
            got = P.resize_pil(img, rh, rw, window=(y0, x0, ho, wo))
            assert np.array_equal(got, whole[y0:y0 + ho, x0:x0 + wo]), (h, w, rh, rw, y0, x0)
        assert np.array_equal(P.resize_pil(img, rh, rw, window=(rh - 1, rw - 1, 1, 1)), whole[-1:, -1:])
    with pytest.raises(AssertionError):
        P.resize_pil(img, rh, rw, window=(1, 0, rh, rw))


def test_equal_sizes_give_the_bytes_back():
    lo, n, coef = P.aa_coefs(9, 9)
    assert lo.tolist() == list(range(9)) and n.tolist() == [2] * 8 + [1]
    assert (coef[:, 0] == 1 << 22).all() and (coef[:, 1:] == 0).all()
    img = np.random.default_rng(3).integers(0, 256, (9, 13, 3), dtype=np.uint8)
    assert np.array_equal(P.resize_pil(img, 9, 13), img)
    assert np.array_equal(P.resize_pil(img, 9, 5)[:, :, 0], P.resize_pil(img[:, :, :1], 9, 5)[:, :, 0])     # channels are independent


def test_coefficient_rule_values():
    """2x: center X * 2 + 1, support 2, taps (1, 3, 3, 1) / 8 inside, and the clipped windows at both ends renormalised"""
    lo, n, coef = P.aa_coefs(8, 4)
    assert lo.tolist() == [0, 1, 3, 5] and n.tolist() == [3, 4, 4, 3]
    q = 1 << 22
    assert coef[1].tolist() == [q // 8, 3 * q // 8, 3 * q // 8, q // 8]
    assert coef[0, :3].tolist() == [int(3 / 7 * q + 0.5), int(3 / 7 * q + 0.5), int(1 / 7 * q + 0.5)] and coef[0, 3] == 0
    lo, n, coef = P.aa_coefs(64, 2)                                   # 32x: 64 taps of the 65 a window may hold, clipped at the edges
    assert n.max() == 48 and (lo + n <= 64).all()
    assert P.aa_coefs(3200, 100)[1].max() <= 2 * P.AA_MAX_SCALE + 1


def test_identity_geometry_equals_the_plain_statement():
    """(RH, RW) == (H, W): reference_aa == reference bit for bit, in float32 and int8, crops and channel orders included"""
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (24, 31, 4), dtype=np.uint8), rng.integers(0, 256, (16, 20, 4), dtype=np.uint8)]
    ident = P.Preset("ident", (16, 20), (104.0, 117.5, 123.25), scale=(0.5, 0.017, 1.0), channels="BGR")
    pixels, srcs, pb = P.pack_host(imgs, ident, align=8)
    for i, im in enumerate(imgs):                                     # no resize; the first image keeps a crop
        srcs[i]["resize_h"], srcs[i]["resize_w"] = im.shape[:2]
    srcs[0]["crop_y"], srcs[0]["crop_x"] = 8, 11
    ch = P.src_channels(ident, "RGBA")
    for q0 in (None, -1, 2):
        a, sa = P.reference_aa(pixels, srcs, (16, 20), pb, ch, np.float32(ident.mean), np.float32(ident.scale), q0=q0)
        b, sb = P.reference(pixels, srcs, (16, 20), pb, ch, np.float32(ident.mean), np.float32(ident.scale), q0=q0)
        assert a.dtype == b.dtype and (sa == 0).all() and (sb == 0).all()
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _rec(**kw):
    r = dict(offset=0, h=10, w=8, row_pitch=24, resize_h=4, resize_w=4, crop_y=0, crop_x=0, reserved=0)
    r.update(kw)
    return np.array([tuple(r[k] for k in P.SRC_DTYPE.names)], P.SRC_DTYPE)


@pytest.mark.parametrize("change,bits,buf", [
    (dict(), 0, 240),
    (dict(h=128, resize_h=4), 0, 128 * 24),                                        # h = 32 * rh
    (dict(h=129, resize_h=4), P.BAD_SCALE, 129 * 24),                              # h = 32 * rh + 1
    (dict(w=128, row_pitch=384), 0, 3840), (dict(w=129, row_pitch=387), P.BAD_SCALE, 3870),
    (dict(h=129, w=129, row_pitch=387), P.BAD_SCALE, 129 * 387),
    (dict(h=129), P.BAD_SCALE | P.OUT_OF_BUFFER, 240),                             # combined with the other bits
    (dict(h=129, crop_y=1), P.BAD_SCALE | P.BAD_CROP, 129 * 24),
    (dict(h=129, row_pitch=23, offset=-1), P.BAD_SCALE | P.BAD_PITCH | P.BAD_OFFSET, 129 * 24),
    (dict(h=40000), P.BAD_SIZE, 240),                                              # not evaluated when the sizes are bad
    (dict(w=-3), P.BAD_SIZE, 240),
    (dict(resize_h=0), P.BAD_RESIZE | P.BAD_CROP, 240),                            # (h > 32 * 0 would hold)
    (dict(h=32767, resize_w=32768), P.BAD_RESIZE | P.OUT_OF_BUFFER, 240),
])
def test_scale_bit_of_the_validity_rule(change, bits, buf):
    assert P.BAD_SCALE == 64 and P.AA_MAX_SCALE == 32
    rec = _rec(**change)
    assert P.record_status_aa(rec, 3, buf, (4, 4))[0] == bits
    assert P.record_status_aa(rec, 3, buf, (4, 4))[0] & ~P.BAD_SCALE == P.record_status(rec, 3, buf, (4, 4))[0]


def test_malformed_records_give_zeros_in_the_statement():
    rng = np.random.default_rng(4)
    pixels = rng.integers(0, 256, 129 * 24, dtype=np.uint8)
    recs = np.concatenate([_rec(), _rec(h=129), _rec(h=128)])
    out, st = P.reference_aa(pixels, recs, (4, 4), 3, [2, 1, 0], [1, 2, 3], [1, 1, 1])
    assert st.tolist() == [0, P.BAD_SCALE, 0] and (out[1] == 0).all() and (out[0] != 0).any() and (out[2] != 0).any()
    q, st = P.reference_aa(pixels, recs, (4, 4), 3, [2, 1, 0], [1, 2, 3], [1, 1, 1], q0=-2)
    assert q.dtype == np.int8 and (q[1] == 0).all()


@pytest.fixture(scope="module")
def host_net():
    t = cfg.tiny_tables()
    net = NetWork(t)
    net.Quantization(synth.q_text(synth.synth_q_values(t, 1)))
    return net


FAKE = 0x7f0000001000      # never dereferenced: every case is refused before a device call


def _call(net, desc=None, batch=2, out_q=1, ptrs=(FAKE, FAKE, FAKE, FAKE)):
    d = desc if desc is not None else P.desc_of(P.TORCHVISION_PIL, "RGB")
    px, srcs, out, st = ptrs
    return _lib.lib().tf2_preprocess_aa(net._h if net is not None else None, C.byref(d) if d is not False else None, px, 1 << 20, srcs,
                                        batch, out_q, out, st, None)


def _desc(**kw):
    d = P.desc_of(P.TORCHVISION_PIL, "RGB")
    for k, v in kw.items():
        if k in ("src_channel", "mean", "scale"):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,message", [
    (dict(desc=_desc(size=8)), "desc size"),
    (dict(desc=False), "null desc"),
    (dict(desc=_desc(pixel_bytes=5)), "pixel_bytes"), (dict(desc=_desc(pixel_bytes=2)), "pixel_bytes"),
    (dict(desc=_desc(src_channel=(1, 3))), "src_channel[1]"), (dict(desc=_desc(src_channel=(0, -1))), "src_channel[0]"),
    (dict(desc=_desc(mean=(2, float("nan")))), "finite"), (dict(desc=_desc(scale=(0, float("inf")))), "finite"),
    (dict(desc=_desc(round_resized=2)), "round_resized"),             # still validated, otherwise ignored
    (dict(batch=0), "batch"), (dict(batch=-1), "batch"),
    (dict(out_q=2), "out_q"),
    (dict(ptrs=(None, FAKE, FAKE, FAKE)), "null device pointer"), (dict(ptrs=(FAKE, None, FAKE, FAKE)), "null device pointer"),
    (dict(ptrs=(FAKE, FAKE, None, FAKE)), "null device pointer"), (dict(ptrs=(FAKE, FAKE, FAKE, None)), "null device pointer"),
])
def test_host_refusals(host_net, kw, message):
    st = _call(host_net, **kw)
    err = _lib.lib().tf2_last_error().decode()
    assert st == -1 and err.startswith("tf2_preprocess_aa: ") and message in err, (st, err)


def test_host_refusals_of_the_net():
    assert _call(None) == -1 and "null tf2_net" in _lib.lib().tf2_last_error().decode()
    t4 = cfg.tiny_tables(c0=4)
    net4 = NetWork(t4)
    net4.Quantization(synth.q_text(synth.synth_q_values(t4, 1)))
    assert _call(net4) == -1 and "image_c" in _lib.lib().tf2_last_error().decode()
    bare = NetWork(cfg.tiny_tables())                      # no q table: int8 output refused
    assert _call(bare, out_q=1) == -1 and "q table" in _lib.lib().tf2_last_error().decode()
    assert _lib.lib().tf2_abi_version() == 1


def test_presets():
    assert sorted(P.PRESETS) == ["googlenet", "resnet50", "squeezenet", "ssd300", "torchvision"]     # as before: no new key
    assert all(not p.antialias for p in P.PRESETS.values())
    assert sorted(P.AA_PRESETS) == ["torchvision_pil"] and P.AA_PRESETS["torchvision_pil"] is P.TORCHVISION_PIL
    a, b = P.TORCHVISION_PIL, P.TORCHVISION
    assert a.antialias and a.name == "torchvision_pil"
    from dataclasses import replace
    assert replace(a, name=b.name, antialias=False) == b
    assert a.geometry(375, 500) == (256, 341, 16, 58)
    assert P.desc_of(a, "RGB").round_resized == 0


def test_reference_aa_is_resize_pil_then_mean_and_scale():
    """the TORCHVISION_PIL pipeline on a 500 x 375 source: Resize(256) to 341 x 256, the centre 224 x 224, bytes through mean / scale"""
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (500, 375, 3), dtype=np.uint8)
    pre = P.TORCHVISION_PIL
    pixels, srcs, pb = P.pack_host([img], pre)
    out, st = P.reference_aa(pixels, srcs, pre.out_hw, pb, P.src_channels(pre, "RGB"), np.float32(pre.mean), np.float32(pre.scale))
    rh, rw, cy, cx = pre.geometry(500, 375)
    assert (rh, rw) == (341, 256) and st.tolist() == [0]
    crop = P.resize_pil(img, rh, rw)[cy:cy + 224, cx:cx + 224]
    want = (np.moveaxis(crop, 2, 0).astype(np.float32) - np.float32(pre.mean)[:, None, None]) * np.float32(pre.scale)[:, None, None]
    assert np.array_equal(out[0].view(np.uint32), want.view(np.uint32))
    # ... and it is not the plain statement's image: the antialiased bytes differ on a downscale
    plain = P.reference(pixels, srcs, pre.out_hw, pb, P.src_channels(pre, "RGB"), np.float32(pre.mean), np.float32(pre.scale))[0]
    assert (plain != out).mean() > 0.5


def test_preprocess_aa_kernels_compile_without_scratch():
    import vmcnt_check
    seg, lds, txt = vmcnt_check.kernel_segments("preprocess_aa")
    names = [k for k in seg if "aa_tile_kernel" in k]
    assert len(names) == 2, seg                                    # int8 / float32 output
    assert all(seg[k] == 0 for k in names), seg
    assert "scratch_" not in txt.split("amdhsa.kernels")[0]
    assert lds and max(lds) <= 16384, lds                          # bounded whatever the scale: coefficients 40 x 65, two chunks
