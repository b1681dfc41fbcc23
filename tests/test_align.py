"""The statement of aligned crops (tf2_amd.align: reference_fit, warp_pil, reference_warp; tf2_roi_fit / tf2_roi_warp on the device):
warp_pil byte-identical to Pillow's recorded Image.transform(AFFINE, BILINEAR) output (tests/golden/pil_affine.npz, tools/
gen_pil_affine_golden.py) and to a live Pillow where one is installed; reference_fit against an SVD Umeyama fit followed by a 3 x 3
inverse written here; two points, box-relative landmarks, every status bit of both calls; integer shifts and the fit to a shifted
template; the host refusals of both calls (fake device pointers: a refusal touches no device); the bindings.  The device itself is
checked in tests/test_gpu_align.py."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from tf2_amd import _lib, align as A, config as cfg, preprocess as P, roi as R, synth
from tf2_amd.network import NetWork

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_pil_affine_golden as golden  # noqa: E402

# the five-point face template published for 112 x 112 aligned faces (eyes, nose, mouth corners)
FACE_112 = [(38.2946, 51.6963), (73.5318, 51.5014), (56.0252, 71.7366), (41.5493, 92.3655), (70.7299, 92.2041)]


def test_bindings_and_record_layout():
    assert A.XFORM_DTYPE.itemsize == 56 == C.sizeof(_lib.RoiXform) and A.XFORM_WORDS == 14
    assert A.XFORM_DTYPE.fields["m"][1] == 8 == _lib.RoiXform.m.offset
    assert C.sizeof(_lib.RoiFitDesc) == 4 + 4 + 16 * 2 * 4 + 4 and _lib.RoiFitDesc.space.offset == 136
    assert {"tf2_roi_fit", "tf2_roi_warp"} <= set(_lib.EXPORTED)
    L = _lib.lib()
    assert L.tf2_roi_fit and L.tf2_roi_warp
    assert (A.BAD_LANDMARKS, A.BAD_MATRIX) == (64, 128)


def test_warp_pil_is_pillows_recorded_bytes():
    cases, version = golden.load(os.path.join(ROOT, "tests", "golden", "pil_affine.npz"))
    assert len(cases) >= 36 and version
    families, channels = set(), set()
    for family, src, m, oh, ow, want in cases:
        got = A.warp_pil(src, m, oh, ow)
        assert got.dtype == np.uint8 and got.shape == want.shape == (oh, ow, src.shape[2])
        assert np.array_equal(got, want), (family, src.shape, m, oh, ow, np.argwhere(got != want)[:4])
        families.add(family)
        channels.add(src.shape[2])
        if family == golden.OUTSIDE:
            assert (want == 0).all()
        if family == golden.FLOAT32:
            assert np.array_equal(m, m.astype(np.float32).astype(np.float64))
    assert families == set(range(10)) and channels == {1, 3}
    shapes = [src.shape[:2] for _, src, *_ in cases]
    assert any(h == 1 and w > 1 for h, w in shapes) and any(w == 1 and h > 1 for h, w in shapes) and (1, 1) in shapes
    # the exact turns are the bytes themselves
    family, src, m, oh, ow, want = cases[0]
    assert family == golden.ROT90 and np.array_equal(want, np.rot90(src, -1))
    family, src, m, oh, ow, want = cases[3]
    assert family == golden.ROT180 and np.array_equal(want, src[::-1, ::-1])


def test_warp_pil_is_a_live_pillow_where_installed():
    """an extra check where PIL imports (the recorded bytes above are the one that never skips)"""
    pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(78)
    for i in range(120):
        c = (1, 3)[i & 1]
        h, w = (int(v) for v in rng.integers(1, 40, 2))
        oh, ow = (int(v) for v in rng.integers(1, 33, 2))
        m = golden.rotation(rng.uniform(0, 360), math.exp(rng.uniform(-1.5, 1.5)), h, w, oh, ow, (rng.uniform(-3, 3), rng.uniform(-3, 3)))
        if i % 6 == 0:
            m = (1.0, 0.0, float(rng.integers(-3, 4)), 0.0, 1.0, float(rng.integers(-3, 4)))
        elif i % 6 == 1:
            m = (0.5, 0.0, -0.25, 0.0, 0.5, -0.25)
        elif i % 6 == 2:
            m = tuple(float(np.float32(v)) for v in m)
        img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        assert np.array_equal(A.warp_pil(img, m, oh, ow), golden.pillow_affine(img, m, oh, ow)), (h, w, c, m, oh, ow)


def test_integer_shifts_reproduce_the_bytes_and_fill_zero_outside():
    rng = np.random.default_rng(1)
    img = rng.integers(1, 256, (9, 11, 3), dtype=np.uint8)
    for tx, ty in ((0, 0), (2, -1), (-3, 4), (11, 0), (0, -9), (5, 5)):
        got = A.warp_pil(img, (1, 0, tx, 0, 1, ty), 9, 11)
        want = np.zeros_like(img)
        ys, xs = np.arange(9) + ty, np.arange(11) + tx
        oky, okx = (ys >= 0) & (ys < 9), (xs >= 0) & (xs < 11)
        want[np.ix_(oky, okx)] = img[np.ix_(ys[oky], xs[okx])]
        assert np.array_equal(got, want), (tx, ty)
    assert (A.warp_pil(img, (1, 0, 11, 0, 1, 0), 9, 11) == 0).all()


# ---- the fit ---------------------------------------------------------------------------------------------------------------------
def _umeyama_then_inverse(src, dst):
    """an independent statement: the SVD similarity src -> dst without reflection (Umeyama 1991), then the inverse of its 3 x 3 matrix"""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    ms, md = src.mean(0), dst.mean(0)
    xs, xd = src - ms, dst - md
    cov = xd.T @ xs / len(src)
    U, S, Vt = np.linalg.svd(cov)
    d = np.ones(2)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        d[-1] = -1
    rot = U @ np.diag(d) @ Vt
    scale = (S * d).sum() / xs.var(0).sum()
    T = np.eye(3)
    T[:2, :2] = scale * rot
    T[:2, 2] = md - scale * rot @ ms
    return np.linalg.inv(T)[:2].reshape(6)


def _rois(rows):
    rois = np.zeros(len(rows), R.ROI_DTYPE)
    for k, (image, x0, y0, x1, y1) in enumerate(rows):
        rois[k] = (image, 1, k, 0.5, x0, y0, x1, y1)
    return rois


def _poses(rng, tpl, n):
    """landmarks: the template turned, scaled, moved and jittered"""
    out = np.zeros((n, len(tpl), 2), np.float32)
    for s in range(n):
        th, sc = rng.uniform(0, 2 * np.pi), math.exp(rng.uniform(-1.5, 1.5))
        rot = sc * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
        out[s] = (np.asarray(tpl, np.float64) @ rot.T + rng.uniform(-300, 300, 2) + rng.normal(0, 0.03 * sc * 30, (len(tpl), 2))).astype(np.float32)
    return out


@pytest.mark.parametrize("K", [2, 3, 5, 16])
def test_reference_fit_agrees_with_svd_umeyama_then_inverse(K):
    rng = np.random.default_rng(K)
    tpl = A.scaled_template(FACE_112, (112, 112), (227, 227)) if K == 5 else rng.uniform(20, 200, (K, 2)).astype(np.float32)
    n = 200
    lmk = _poses(rng, tpl, n)
    rois = _rois([(s % 3, 0, 0, 0, 0) for s in range(n)])
    xf, st = A.reference_fit(rois, lmk, tpl, 0)
    assert (st == 0).all() and xf["image"].tolist() == rois["image"].tolist() and (xf["reserved"] == 0).all()
    worst = 0.0
    for s in range(n):
        want = _umeyama_then_inverse(lmk[s], tpl)
        rel = np.abs(xf[s]["m"] - want).max() / np.abs(want).max()
        worst = max(worst, rel)
    assert worst <= 1e-9, worst
    assert np.array_equal(xf["m"][:, 0], xf["m"][:, 4]) and np.array_equal(xf["m"][:, 1], -xf["m"][:, 3])    # a similarity


def test_a_fit_to_the_shifted_template_is_that_shift():
    assert np.allclose(A.scaled_template(FACE_112, (112, 112), (224, 224)), 2 * np.asarray(FACE_112))
    # the face template for 224 x 224 on quarter pixels, its sums multiples of five: every sum, mean and difference of the fit is exact
    tpl = np.float32([(76.5, 103.5), (147.0, 103.0), (112.0, 143.5), (83.0, 185.0), (141.5, 185.0)])
    for dx, dy in ((0.0, 0.0), (64.0, -32.0), (-7.0, 1001.0), (1024.25, 512.5)):
        lmk = (tpl + np.float32([dx, dy]))[None]
        assert np.array_equal(lmk[0].astype(np.float64), tpl.astype(np.float64) + [dx, dy])
        xf, st = A.reference_fit(_rois([(0, 0, 0, 0, 0)]), lmk, tpl, 0)
        assert st.tolist() == [0] and xf[0]["m"].tolist() == [1.0, 0.0, dx, 0.0, 1.0, dy], (dx, dy, xf[0]["m"])
    # and the warp with it reads the source at that shift
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    xf, _ = A.reference_fit(_rois([(0, 0, 0, 0, 0)]), (tpl + np.float32([16.0, 8.0]))[None], tpl, 0)
    assert np.array_equal(A.warp_pil(img, xf[0]["m"], 12, 14), img[8:20, 16:30])


def test_two_points_and_box_relative_landmarks():
    tpl = np.float32([[10.0, 20.0], [30.0, 20.0]])
    lmk = np.float32([[[100.0, 50.0], [100.0, 90.0]]])                   # the segment turned by a quarter and doubled
    xf, st = A.reference_fit(_rois([(0, 0, 0, 0, 0)]), lmk, tpl, 0)
    assert st.tolist() == [0]
    m = xf[0]["m"]
    for (tx, ty), (sx, sy) in zip(tpl, lmk[0]):
        assert abs(m[0] * tx + m[1] * ty + m[2] - sx) < 1e-9 and abs(m[3] * tx + m[4] * ty + m[5] - sy) < 1e-9
    # space 1 equals space 0 on the mapped points
    rng = np.random.default_rng(4)
    tpl5 = A.scaled_template(FACE_112, (112, 112), (227, 227))
    boxes = [(0, 10.5, 20.25, 110.75, 150.5), (1, 0.0, 0.0, 64.0, 48.0), (0, -30.0, 5.0, 200.0, 400.0)]
    rois = _rois(boxes)
    rel = rng.uniform(0.1, 0.9, (3, 5, 2)).astype(np.float32)
    mapped = np.zeros_like(rel, dtype=np.float64)
    for s, (_, x0, y0, x1, y1) in enumerate(boxes):
        x0, y0, x1, y1 = (np.float64(np.float32(v)) for v in (x0, y0, x1, y1))
        mapped[s, :, 0] = x0 + rel[s, :, 0].astype(np.float64) * (x1 - x0)
        mapped[s, :, 1] = y0 + rel[s, :, 1].astype(np.float64) * (y1 - y0)
    xf1, st1 = A.reference_fit(rois, rel, tpl5, 1)
    assert (st1 == 0).all()
    if np.array_equal(mapped, mapped.astype(np.float32).astype(np.float64)):      # (the mapped points need not be float32 values)
        xf0, _ = A.reference_fit(rois, mapped.astype(np.float32), tpl5, 0)
        assert xf0.tobytes() == xf1.tobytes()
    for s in range(3):
        want = _umeyama_then_inverse(mapped[s], tpl5)
        assert np.abs(xf1[s]["m"] - want).max() / np.abs(want).max() <= 1e-9
    # a box with exactly representable products: space 1 is space 0 bit for bit
    rel = np.float32([[[0.25, 0.5], [0.75, 0.5], [0.5, 0.625], [0.375, 0.75], [0.625, 0.75]]])
    roi = _rois([(2, 16.0, 32.0, 144.0, 160.0)])
    xf1, st1 = A.reference_fit(roi, rel, tpl5, 1)
    xf0, st0 = A.reference_fit(roi, np.float32([16.0, 32.0]) + rel * np.float32(128.0), tpl5, 0)
    assert st1.tolist() == st0.tolist() == [0] and xf1.tobytes() == xf0.tobytes() and xf1[0]["image"] == 2


def test_every_fit_status():
    tpl = A.scaled_template(FACE_112, (112, 112), (227, 227))
    good = (tpl + np.float32([40.0, 30.0]))
    nan_l, inf_l, same = good.copy(), good.copy(), np.repeat(good[:1], 5, 0)
    nan_l[3, 1], inf_l[0, 0] = np.nan, np.inf
    huge = np.float32([[3e38, 0], [-3e38, 0], [0, 3e38], [0, -3e38], [0, 0]])   # finite float32 landmarks: nothing overflows in double
    box, bad_box = (0.0, 0.0, 100.0, 100.0), (0.0, 0.0, 0.5, 100.0)
    rows = [
        ((0,) + box, good, 0), ((-1,) + box, good, A.EMPTY), ((-1,) + bad_box, nan_l, A.EMPTY), ((3,) + box, nan_l, A.BAD_LANDMARKS),
        ((1,) + box, inf_l, A.BAD_LANDMARKS), ((0,) + box, same, A.BAD_LANDMARKS), ((7,) + box, good, 0),
        ((0,) + box, huge, 0),
    ]
    rois, lmk, want = _rois([r for r, _, _ in rows]), np.stack([l for _, l, _ in rows]), [b for _, _, b in rows]
    xf, st = A.reference_fit(rois, lmk, tpl, 0)
    assert st.tolist() == want
    for s, bits in enumerate(want):
        if bits:
            assert xf[s].tobytes() == A.empty_xforms(1).tobytes(), s              # image -1, every m +0.0
        else:
            assert xf[s]["image"] == rois[s]["image"] and np.isfinite(xf[s]["m"]).all()
    assert np.array_equal(xf[0]["m"], xf[6]["m"])                                # (the image index is carried, not judged)
    # n > 0 fails where the landmarks have no correlation with the template: a square, mirrored
    square = np.float32([[-1, -1], [1, -1], [1, 1], [-1, 1]])
    xs, sst = A.reference_fit(_rois([(0,) + box] * 2), np.stack([square * np.float32([1, -1]), square]), square, 0)
    assert sst.tolist() == [A.BAD_LANDMARKS, 0] and xs[0].tobytes() == A.empty_xforms(1).tobytes()
    assert xs[1]["m"].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    # space 1: the box is judged too, and a space-0 fit does not read it
    rows1 = [((0,) + box, good / 100, 0), ((0,) + bad_box, good / 100, A.BAD_BOX), ((0, np.nan, 0, 1, 1), good / 100, A.BAD_BOX),
             ((0,) + bad_box, nan_l, A.BAD_BOX | A.BAD_LANDMARKS), ((-1,) + bad_box, good, A.EMPTY)]
    rois1, lmk1 = _rois([r for r, _, _ in rows1]), np.stack([l for _, l, _ in rows1]).astype(np.float32)
    assert A.reference_fit(rois1, lmk1, tpl, 1)[1].tolist() == [b for _, _, b in rows1]
    assert A.reference_fit(rois1, lmk1, tpl, 0)[1].tolist() == [0, 0, 0, A.BAD_LANDMARKS, A.EMPTY]
    for bad in (np.repeat(tpl[:1], 5, 0), np.float32([[1, 2]]), np.zeros((17, 2), np.float32), np.float32([[0, 0], [np.nan, 1]])):
        with pytest.raises(ValueError):
            A.reference_fit(rois[:1], lmk[:1, :len(bad)], bad, 0)


# ---- the warp's statuses -----------------------------------------------------------------------------------------------------------
def _xforms(rows):
    xf = A.empty_xforms(len(rows))
    for k, (image, m) in enumerate(rows):
        xf[k]["image"], xf[k]["m"] = image, m
    return xf


def test_every_warp_status():
    rng = np.random.default_rng(9)
    srcs = np.zeros(3, P.SRC_DTYPE)
    srcs[0] = (0, 10, 8, 24, 0, 0, 0, 0, 0)
    srcs[1] = (240, 10, 8, 23, 0, 0, 0, 0, 0)                             # BAD_PITCH: the slot is BAD_SRC
    srcs[2] = (240, 6, 7, 21, 0, 0, 0, 0, 0)
    size = 240 + 6 * 21
    pixels = rng.integers(1, 256, size, dtype=np.uint8)
    ident, nan_m, inf_m = (1.0, 0, 0, 0, 1.0, 0), (1.0, 0, np.nan, 0, 1.0, 0), (1.0, 0, 0, 0, -np.inf, 0)
    rows = [((0, ident), 0), ((-1, nan_m), A.EMPTY), ((3, ident), A.BAD_IMAGE), ((-2, ident), A.BAD_IMAGE), ((2, ident), 0),
            ((1, ident), A.BAD_SRC), ((0, nan_m), A.BAD_MATRIX), ((0, inf_m), A.BAD_MATRIX), ((1, nan_m), A.BAD_SRC | A.BAD_MATRIX),
            ((9, inf_m), A.BAD_IMAGE | A.BAD_MATRIX), ((0, ident), 0), ((0, (1.0, 0, 1e30, 0, 1.0, 0)), 0)]
    xf, want = _xforms([r for r, _ in rows]), [b for _, b in rows]
    assert A.warp_status(xf, srcs, 3, size).tolist() == want
    args = ((5, 6), 3, [2, 1, 0], [1, 2, 3], [1, 1, 1])
    out, st = A.reference_warp(pixels, srcs, xf, *args)
    assert st.tolist() == want and out.dtype == np.float32
    for k, bits in enumerate(want):
        assert (out[k] == 0).all() if bits else (out[k] != 0).any(), k
    assert np.array_equal(out[0], out[10])
    img = pixels[:240].reshape(10, 8, 3)
    assert np.array_equal(out[0], (img[:5, :6, ::-1].transpose(2, 0, 1).astype(np.float32) - np.float32([1, 2, 3])[:, None, None]))
    assert np.array_equal(out[11], np.broadcast_to(np.float32([-1, -2, -3])[:, None, None], (3, 5, 6)))   # all fill: (0 - mean) * scale
    q, st = A.reference_warp(pixels, srcs, xf, *args, out="q", q0=-1)
    assert q.dtype == np.int8 and all((q[k] == 0).all() for k, bits in enumerate(want) if bits) and (q[0] != 0).any()
    assert np.array_equal(q[11], np.broadcast_to(np.int8([-2, -4, -6])[:, None, None], (3, 5, 6)))


# ---- the library on the CPU: host refusals (fake device pointers, never dereferenced) --------------------------------------------------
@pytest.fixture(scope="module")
def host_net():
    t = cfg.tiny_tables()
    net = NetWork(t)
    net.Quantization(synth.q_text(synth.synth_q_values(t, 1)))
    return net


FAKE = 0x7f0000001000


def _fdesc(n_points=5, space=0, size=None, tpl=None):
    d = _lib.RoiFitDesc()
    d.size = C.sizeof(_lib.RoiFitDesc) if size is None else size
    d.n_points, d.space = n_points, space
    for i, (x, y) in enumerate(FACE_112 if tpl is None else tpl):
        d.tpl[i][0], d.tpl[i][1] = x, y
    return d


def _fit(desc=None, n_slots=3, ptrs=(FAKE,) * 4):
    d = desc if desc is not None else _fdesc()
    rois, lmk, xf, st = ptrs
    code = _lib.lib().tf2_roi_fit(C.byref(d) if d is not False else None, rois, lmk, n_slots, xf, st, None)
    return code, _lib.lib().tf2_last_error().decode()


@pytest.mark.parametrize("kw,message", [
    (dict(desc=False), "null desc"), (dict(desc=_fdesc(size=8)), "desc size"), (dict(desc=_fdesc(n_points=1)), "n_points"),
    (dict(desc=_fdesc(n_points=17)), "n_points"), (dict(desc=_fdesc(space=2)), "space"), (dict(desc=_fdesc(space=-1)), "space"),
    (dict(desc=_fdesc(tpl=[(1, 2), (float("nan"), 3), (4, 5), (6, 7), (8, 9)])), "not finite"),
    (dict(desc=_fdesc(tpl=[(1, 2), (3, 4), (4, 5), (6, float("inf")), (8, 9)])), "not finite"),
    (dict(desc=_fdesc(tpl=[(7, 7)] * 5)), "zero variance"), (dict(desc=_fdesc(n_points=2, tpl=[(3, 4), (3, 4), (9, 9)])), "zero variance"),
    (dict(n_slots=0), "n_slots"), (dict(n_slots=-2), "n_slots"),
    (dict(ptrs=(FAKE, FAKE, FAKE + 4, FAKE)), "8-byte aligned"),
] + [(dict(ptrs=tuple(None if i == k else FAKE for i in range(4))), "null device pointer") for k in range(4)])
def test_fit_host_refusals(kw, message):
    st, err = _fit(**kw)
    assert st == -1 and err.startswith("tf2_roi_fit: ") and message in err, (st, err)


def test_fit_reads_only_the_first_n_points_of_the_template():
    """values past n_points are not judged: the refusal that follows is the next one in line"""
    d = _fdesc(n_points=2, tpl=[(3, 4), (5, 6), (float("nan"), 0)])
    st, err = _fit(desc=d, n_slots=0)
    assert st == -1 and "n_slots" in err


def _warp(net, desc=None, batch=2, n_slots=3, out_q=1, ptrs=(FAKE,) * 5):
    d = desc if desc is not None else P.desc_of(P.SQUEEZENET, "RGB")
    px, srcs, xf, out, st = ptrs
    code = _lib.lib().tf2_roi_warp(net._h if net is not None else None, C.byref(d) if d is not False else None, px, 1 << 20, srcs, batch,
                                   xf, n_slots, out_q, out, st, None)
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
    (dict(ptrs=(FAKE, FAKE, FAKE + 4, FAKE, FAKE)), "8-byte aligned"),
] + [(dict(ptrs=tuple(None if i == k else FAKE for i in range(5))), "null device pointer") for k in range(5)])
def test_warp_host_refusals(host_net, kw, message):
    st, err = _warp(host_net, **kw)
    assert st == -1 and err.startswith("tf2_roi_warp: ") and message in err, (st, err)


def test_warp_host_refusals_of_the_net():
    st, err = _warp(None)
    assert st == -1 and "null tf2_net" in err
    t4 = cfg.tiny_tables(c0=4)
    net4 = NetWork(t4)
    net4.Quantization(synth.q_text(synth.synth_q_values(t4, 1)))
    st, err = _warp(net4)
    assert st == -1 and "image_c" in err
    bare = NetWork(cfg.tiny_tables())                      # no q table: int8 output refused
    st, err = _warp(bare, out_q=1)
    assert st == -1 and "q table" in err


def test_aligner_statements_follow_its_settings(host_net):
    tpl = A.scaled_template(FACE_112, (112, 112), (int(host_net._nd.image_h), int(host_net._nd.image_w)))
    al = A.DeviceAligner(host_net, P.SQUEEZENET, tpl, "BGR", space=1)
    assert al.n_points == 5 and al.fit_desc.space == 1 and al.fit_desc.size == C.sizeof(_lib.RoiFitDesc)
    assert [al.fit_desc.tpl[i][k] for i in range(5) for k in (0, 1)] == tpl.reshape(-1).tolist()
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (60, 50, 3), dtype=np.uint8)
    pixels, srcs, pb = P.pack_host([img], P.SQUEEZENET)
    rois = _rois([(0, 5.0, 6.0, 45.0, 56.0), (-1, 0, 0, 0, 0), (0, 0.0, 0.0, 50.0, 60.0)])
    lmk = rng.uniform(0.2, 0.8, (3, 5, 2)).astype(np.float32)
    words = np.ascontiguousarray(srcs).view(np.int32).reshape(1, P.SRC_WORDS)
    for out, q0 in (("f32", None), ("q", int(host_net.q[0, 0]))):
        got, st, xf, fst = al.reference(rois, lmk, pixels, words, out=out)
        wxf, wfst = A.reference_fit(rois, lmk, tpl, 1)
        want, wst = A.reference_warp(pixels, srcs, wxf, al.out_hw, pb, P.src_channels(P.SQUEEZENET, "BGR"), np.float32(P.SQUEEZENET.mean),
                                     np.float32(P.SQUEEZENET.scale), out, q0)
        assert fst.tolist() == wfst.tolist() == [0, A.EMPTY, 0] and st.tolist() == wst.tolist() == [0, A.EMPTY, 0]
        assert xf.tobytes() == wxf.tobytes() and got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    with pytest.raises(ValueError):
        A.DeviceAligner(host_net, P.SQUEEZENET, tpl, space=2)
    with pytest.raises(ValueError):
        A.DeviceAligner(host_net, P.SQUEEZENET, np.repeat(tpl[:1], 5, 0))
