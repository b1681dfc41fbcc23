"""Aligned crops on the MI355X (tf2_roi_fit / tf2_roi_warp, roi_warp.hip): both calls bit-identical to align.reference_fit /
reference_warp -- records as bytes, float32 as bits, int8 -- on a 227 x 227 and a 224 x 224 net, over sources with offsets, padded
rows, 3- and 4-byte pixels, a channel swap and 1 x N / N x 1 images, with matrices that turn by any angle and by exactly 90 and 180
degrees, magnify 16x, minify 8x, put sample coordinates exactly on the four boundaries of the inside test, lie entirely outside and
carry 1e30 translations; empty and malformed slots of every status between good ones; Pillow's recorded bytes (tests/golden/
pil_affine.npz) through the device; a misaligned output; fit + warp captured in one graph and replayed on refilled pixels, records,
landmarks and boxes, and two streams side by side; the detect -> select -> fit -> warp -> embed -> match cascade in one captured graph."""
import os
import sys
from dataclasses import replace

import numpy as np
import pytest

from tf2_amd import align as A, preprocess as P, roi as R

from tests.test_gpu_roi import CASCADE_MAX_ROIS, _Cascade, _image_sets, _same_table, cascade_nets  # noqa: F401  (cascade_nets: a fixture)
from tests.test_gpu_roi_aa import _dev, _pack, _same, _src_words, nets  # noqa: F401  (nets: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_pil_affine_golden as golden  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACE_112 = [(38.2946, 51.6963), (73.5318, 51.5014), (56.0252, 71.7366), (41.5493, 92.3655), (70.7299, 92.2041)]
IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _xforms(rows):
    xf = A.empty_xforms(len(rows))
    for k, (image, m) in enumerate(rows):
        xf[k]["image"], xf[k]["m"] = image, m
    return xf


def _rois(rows):
    rois = np.zeros(len(rows), R.ROI_DTYPE)
    for k, (image, x0, y0, x1, y1) in enumerate(rows):
        rois[k] = (image, 15, k, 0.5, x0, y0, x1, y1)
    return rois


def _aligner(net, preset, src_order="RGB", space=0, K=5):
    hw = (int(net._nd.image_h), int(net._nd.image_w))
    return A.DeviceAligner(net, preset, A.scaled_template(FACE_112, (112, 112), hw)[:K], src_order, space=space)


SIZES = [(1850, 1900), (40, 33), (1, 257), (300, 1), (300, 400)]


def _good_xforms(hw):
    """{family: rows} on the sources SIZES for a hw x hw output"""
    f32 = lambda m: tuple(float(np.float32(v)) for v in m)
    rot = lambda deg, scale, i, shift=(0.0, 0.0): golden.rotation(deg, scale, SIZES[i][0], SIZES[i][1], hw, hw, shift)
    return {
        "rotations": [(4, rot(17.0, 1.0, 4)), (0, rot(-63.5, 3.1, 0, (40.5, -7.25))), (4, rot(201.25, 0.8, 4)), (1, rot(135.0, 0.12, 1))],
        "90": [(4, (0.0, 1.0, 3.0, -1.0, 0.0, float(hw)))],               # fx = y + 3.5, fy = hw - x - 0.5: dx = dy = 0, the bytes, turned
        "180": [(4, (-1.0, 0.0, 300.0, 0.0, -1.0, 250.0))],
        "16x up": [(1, (0.0625, 0.0, 10.0, 0.0, 0.0625, 5.0)), (1, rot(30.0, 0.0625, 1))],
        "8x down": [(0, (8.0, 0.0, 20.0, 0.0, 8.0, 3.0)), (0, rot(-40.0, 8.0, 0))],
        "boundaries": [(1, (1.0, 0.0, -0.5, 0.0, 1.0, -0.5))],            # fx = x, fy = y: exactly 0, w = 33 and h = 40 are reached
        "outside": [(1, (1.0, 0.0, 5000.0, 0.0, 1.0, 5000.0))],
        "1e30": [(4, (1.0, 0.0, 1e30, 0.0, 1.0, 0.0)), (4, (1e300, 1e300, 1.0, -1e300, 1e300, -1e30))],   # ... and products that overflow
        "1 x N": [(2, rot(5.0, 1.0, 2)), (2, (1.0, 0.0, 10.0, 0.0, 0.004, 0.0))],
        "N x 1": [(3, rot(-80.0, 1.2, 3)), (3, (0.004, 0.0, 0.0, 0.0, 1.0, 20.25))],
        "float32": [(4, f32(rot(27.0, 1.1, 4)))],
        "mirror": [(4, (-1.0, 0.0, 390.25, 0.0, 1.0, 10.5))],
    }


@pytest.mark.parametrize("hw,preset,src_order", [(227, P.SQUEEZENET, "RGB"), (227, P.GOOGLENET, "BGRA"), (224, P.RESNET50, "RGBA"),
                                                 (224, P.TORCHVISION, "BGR")])
def test_warp_bit_identical(nets, hw, preset, src_order):
    import torch
    rng = np.random.default_rng(hw + len(src_order))
    pb = len(src_order)
    pixels, recs = _pack(rng, SIZES, pb)
    assert (recs["offset"] > 0).all() and (recs["row_pitch"] > recs["w"] * pb).any()
    families = _good_xforms(hw)
    xf = _xforms([row for rows in families.values() for row in rows])
    S = len(xf)
    assert S == 20
    first, at = {}, 0
    for name, rows in families.items():
        first[name], at = at, at + len(rows)
    al = _aligner(nets[hw], preset, src_order)
    assert al.out_hw == (hw, hw) and A.warp_status(xf, recs, pb, pixels.size).tolist() == [0] * S
    # the case list does what it says, by the statement
    xin = np.arange(hw) + 0.5
    m = xf[first["boundaries"]]["m"]
    fx = (m[0] * xin + m[1] * 0.5) + m[2]
    assert fx[0] == 0.0 and fx[33] == 33.0 and (m[4] * xin + m[5])[40] == 40.0
    ch = P.src_channels(preset, src_order)
    px, sr, xt = _dev(pixels), _src_words(recs), A.xforms_to_device(xf, DEV)
    for out in ("f32", "q"):
        got, st = al.warp(px, sr, xt, out=out)
        torch.cuda.synchronize()
        want, wst = al.reference_warp(pixels, recs, xf, out=out)
        assert wst.tolist() == [0] * S and st.cpu().numpy().tolist() == [0] * S
        g = _same(got, want, out)
        fills = [first["outside"], first["1e30"], first["1e30"] + 1]
        assert all(len(np.unique(g[s, c])) == 1 for s in fills for c in range(3))            # all fill: one value a channel
        assert all(len(np.unique(g[s])) > 4 for s in range(S) if s not in fills) or out == "q"
        b = g[first["boundaries"]]
        assert len(np.unique(b[:, :40, :33])) > 4 and all(len(np.unique(b[c, 40:])) == 1 and len(np.unique(b[c, :, 33:])) == 1 for c in range(3))
    # the quarter turn is the source's bytes, turned (float32, before mean and scale are undone: compare through the statement's line)
    img = P.source_image(pixels, recs[4], pb, ch)
    rows, cols = np.arange(hw), np.arange(hw)
    turned = img[(hw - 1 - cols)[None, :], (rows + 3)[:, None]]                                 # out[y][x] = src[hw - 1 - x][y + 3]
    m32, s32 = np.float32(preset.mean), np.float32(preset.scale)
    want90 = (np.moveaxis(turned, 2, 0).astype(np.float32) - m32[:, None, None]) * s32[:, None, None]
    got90 = al.warp(px, sr, xt, out="f32")[0][first["90"]].cpu().numpy()
    assert np.array_equal(got90.view(np.uint32), want90.view(np.uint32))


def test_bad_slots_between_good_ones(nets):
    import torch
    rng = np.random.default_rng(5)
    pixels, recs = _pack(rng, [(300, 400), (40, 33)], 3, past_the_buffer=True)
    good = (0, golden.rotation(25.0, 1.2, 300, 400, 227, 227))
    nan_m, inf_m = (1.0, 0.0, np.nan, 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, -np.inf, 1.0, 0.0)
    rows = [
        (good, 0), ((-1, IDENT), A.EMPTY), ((-1, nan_m), A.EMPTY), ((3, IDENT), A.BAD_IMAGE), ((1, IDENT), 0), ((-2, IDENT), A.BAD_IMAGE),
        ((0, nan_m), A.BAD_MATRIX), (good, 0), ((2, IDENT), A.BAD_SRC), ((0, inf_m), A.BAD_MATRIX), ((2, nan_m), A.BAD_SRC | A.BAD_MATRIX),
        ((1 << 30, inf_m), A.BAD_IMAGE | A.BAD_MATRIX), (good, 0), ((1, (0.1, 0.0, 0.0, 0.0, 0.1, 0.0)), 0),
    ]
    xf, want_status = _xforms([r for r, _ in rows]), [bits for _, bits in rows]
    al = _aligner(nets[227], P.SQUEEZENET)
    assert A.warp_status(xf, recs, 3, pixels.size).tolist() == want_status
    px, sr, xt = _dev(pixels), _src_words(recs), A.xforms_to_device(xf, DEV)
    for out in ("f32", "q"):
        got, st = al.warp(px, sr, xt, out=out)
        torch.cuda.synchronize()
        want, wst = al.reference_warp(pixels, recs, xf, out=out)
        assert wst.tolist() == want_status and st.cpu().numpy().tolist() == want_status
        g = _same(got, want, out)
        assert all((g[s] == 0).all() for s, bits in enumerate(want_status) if bits) and len(np.unique(g)) > 4
        assert out == "q" or all(len(np.unique(g[s])) > 2 for s, bits in enumerate(want_status) if not bits)
        assert np.array_equal(g[0], g[7]) and np.array_equal(g[0], g[12])      # the good slots between them are what they are alone


def _fit_case(rng, tpl, n, space):
    """n slots: boxes, and landmarks that are the template turned, scaled, moved and jittered (relative to the box for space 1)"""
    K = len(tpl)
    rows, lmk = [], np.zeros((n, K, 2), np.float32)
    for s in range(n):
        x0, y0 = rng.uniform(-50, 900, 2)
        bw, bh = rng.uniform(20, 600, 2)
        rows.append((s % 7, x0, y0, x0 + bw, y0 + bh))
        th, sc = rng.uniform(0, 2 * np.pi), np.exp(rng.uniform(-1.5, 1.5))
        rot = sc * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        pts = np.asarray(tpl, np.float64) @ rot.T + rng.uniform(0, 800, 2) + rng.normal(0, sc, (K, 2))
        lmk[s] = ((pts - [x0, y0]) / [bw, bh] if space else pts).astype(np.float32)
    return _rois(rows), lmk


@pytest.mark.parametrize("K,space", [(2, 0), (5, 0), (5, 1), (16, 1), (4, 0)])
def test_fit_bit_identical_with_every_status(nets, K, space):
    import torch
    rng = np.random.default_rng(10 * K + space)
    square = np.float32([[-1, -1], [1, -1], [1, 1], [-1, 1]]) * 50 + 100
    tpl = square if K == 4 else (A.scaled_template(FACE_112, (112, 112), (227, 227)) if K == 5 else rng.uniform(20, 200, (K, 2)).astype(np.float32))
    n = 150                                                               # three blocks, the last one partly filled
    rois, lmk = _fit_case(rng, tpl, n, space)
    want_bits = {}
    rois[3]["image"] = -1; want_bits[3] = A.EMPTY
    rois[64]["image"] = -1; lmk[64, 0, 0] = np.nan; rois[64]["x1"] = np.nan; want_bits[64] = A.EMPTY
    lmk[10, K - 1, 1] = np.nan; want_bits[10] = A.BAD_LANDMARKS
    lmk[65, 0, 0] = -np.inf; want_bits[65] = A.BAD_LANDMARKS
    lmk[149] = lmk[149, 0]                                                # all landmarks equal: var == 0 where the sums are exact,
    if space == 0:                                                        # as they are on float32 values (a mapped point has 53 bits)
        want_bits[149] = A.BAD_LANDMARKS
    rois[20]["x1"] = rois[20]["x0"] + np.float32(0.5); want_bits[20] = A.BAD_BOX if space else 0
    rois[130]["y0"] = np.inf; lmk[130, 1, 0] = np.nan; want_bits[130] = (A.BAD_BOX if space else 0) | A.BAD_LANDMARKS
    rois[77]["image"] = 1 << 20                                            # carried, not judged
    if K == 4:                                                            # the square, mirrored: no correlation, n == 0
        lmk[40] = (square - 100) * np.float32([1, -1]) + 300; want_bits[40] = A.BAD_LANDMARKS
        lmk[41] = square + np.float32([32, 64])
    al = A.DeviceAligner(nets[227], P.SQUEEZENET, tpl, space=space)
    want, wst = al.reference_fit(rois, lmk)
    judged = [s for s in range(n) if space == 0 or s != 149]
    assert all(wst[s] == want_bits.get(s, 0) for s in judged), [(s, wst[s]) for s in judged if wst[s] != want_bits.get(s, 0)]
    assert want[77]["image"] == 1 << 20 and (K != 4 or want[41]["m"].tolist() == [1.0, 0.0, 32.0, 0.0, 1.0, 64.0])
    xt, st = al.fit(R.rois_to_device(rois, DEV), _dev(lmk))
    torch.cuda.synchronize()
    got = A.xforms_to_host(xt)
    assert np.array_equal(st.cpu().numpy(), wst)
    bad = [s for s in range(n) if got[s].tobytes() != want[s].tobytes()]
    assert not bad, (len(bad), bad[:5], got[bad[0]], want[bad[0]])
    assert all(got[s].tobytes() == A.empty_xforms(1).tobytes() for s in want_bits if want_bits[s])


def test_recorded_pillow_cases_through_the_device(nets):
    """every case of pil_affine.npz as a slot of one call with mean 0 and scale 1: the top-left oh x ow of the 227 x 227 output is
    Pillow's bytes (an output pixel depends on its own coordinates alone), the rest is the statement's"""
    import torch
    cases, _ = golden.load(os.path.join(ROOT, "tests", "golden", "pil_affine.npz"))
    imgs = [np.ascontiguousarray(np.broadcast_to(src, src.shape[:2] + (3,))) for _, src, *_ in cases]       # L: the byte three times
    preset = replace(P.SQUEEZENET, mean=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0))
    order = preset.channels
    pixels, recs, pb = P.pack_host(imgs, preset, align=4)
    xf = _xforms([(i, m) for i, (_, _, m, *_) in enumerate(cases)])
    al = _aligner(nets[227], preset, order)
    assert P.src_channels(preset, order) == [0, 1, 2]
    got, st = al.warp(_dev(pixels), _src_words(recs), A.xforms_to_device(xf, DEV), out="f32")
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    g = got.cpu().numpy()
    for s, (family, src, m, oh, ow, want) in enumerate(cases):
        w3 = np.broadcast_to(want, (oh, ow, 3)).transpose(2, 0, 1).astype(np.float32)
        assert np.array_equal(g[s, :, :oh, :ow], w3), (s, family, np.argwhere(g[s, :, :oh, :ow] != w3)[:4])
    want_all, _ = al.reference_warp(pixels, recs, xf, out="f32")
    _same(got, want_all, "recorded cases")


def test_warp_into_a_misaligned_output(nets):
    import torch
    rng = np.random.default_rng(12)
    pixels, recs = _pack(rng, [(300, 400), (40, 33)], 3)
    xf = _xforms([(0, golden.rotation(33.0, 1.4, 300, 400, 224, 224)), (-1, IDENT), (1, golden.rotation(-20.0, 0.15, 40, 33, 224, 224)),
                  (0, (1.0, 0.0, 100.0, 0.0, 1.0, 150.0))])
    al = _aligner(nets[224], P.RESNET50)
    px, sr, xt = _dev(pixels), _src_words(recs), A.xforms_to_device(xf, DEV)
    S, (oh, ow) = len(xf), al.out_hw
    for out in ("f32", "q"):
        flat = torch.zeros(S * 3 * oh * ow + 1, dtype=torch.int8 if out == "q" else torch.float32, device=DEV)
        images = flat[1:].view(S, 3, oh, ow)                      # one element past the allocation's start
        assert images.data_ptr() % (4 if out == "q" else 16) != 0
        got, st = al.warp(px, sr, xt, out=out, images=images)
        torch.cuda.synchronize()
        want, wst = al.reference_warp(pixels, recs, xf, out=out)
        assert wst.tolist() == [0, A.EMPTY, 0, 0] and st.cpu().numpy().tolist() == wst.tolist()
        _same(got, want, out)
        assert flat[0].item() == 0


def _align_set(seed, sizes, n_slots, tpl):
    """images of `sizes`, a table of n_slots boxes over them (some empty) and box-relative landmarks of a turned face in each"""
    rng = np.random.default_rng(seed)
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
    rows, lmk = [], np.zeros((n_slots, len(tpl), 2), np.float32)
    for s in range(n_slots):
        b = int(rng.integers(0, len(sizes)))
        h, w = sizes[b]
        bw, bh = rng.uniform(0.2, 0.7) * w, rng.uniform(0.2, 0.7) * h
        x0, y0 = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
        rows.append((-1 if s % 5 == seed % 5 else b, x0, y0, x0 + bw, y0 + bh))
        th = rng.uniform(-0.6, 0.6)
        rot = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        lmk[s] = (((np.asarray(tpl, np.float64) / 227 - 0.5) * rng.uniform(0.5, 0.9)) @ rot.T + 0.5).astype(np.float32)
    if seed == 1:
        lmk[2, 3, 0] = np.nan
    return imgs, _rois(rows), lmk


def test_graph_replay_with_refilled_buffers_and_two_streams(nets):
    """fit + warp captured once; pixels, records, landmarks and boxes refilled with other sizes and poses; each replay against the
    statement.  Then two streams with their own inputs and outputs side by side."""
    import torch
    al = _aligner(nets[227], P.SQUEEZENET, space=1)
    S = 12
    sets = [_align_set(k, sizes, S, al.template) for k, sizes in enumerate((((375, 500), (300, 300)), ((120, 90), (640, 480)),
                                                                             ((333, 500), (227, 227))))]
    cap = max(P.pack_host(s[0], P.SQUEEZENET)[0].size for s in sets)
    pixels = torch.zeros(cap, dtype=torch.uint8, device=DEV)
    srcs = torch.zeros(2, P.SRC_WORDS, dtype=torch.int32, device=DEV)
    rois, lmk = R.rois_to_device(sets[0][1], DEV), _dev(sets[0][2])

    def refill(k):
        P.pack(sets[k][0], P.SQUEEZENET, DEV, pixels=pixels, srcs=srcs)
        rois.copy_(R.rois_to_device(sets[k][1], "cpu"))
        lmk.copy_(torch.from_numpy(sets[k][2]))

    def check(out, inputs, where):
        want_img, want_st, want_xf, want_fst = al.reference(*inputs, out="q")
        assert A.xforms_to_host(out[2]).tobytes() == want_xf.tobytes(), where
        assert np.array_equal(out[3].cpu().numpy(), want_fst) and np.array_equal(out[1].cpu().numpy(), want_st), where
        _same(out[0], want_img, where)
        return want_fst

    refill(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        al(rois, lmk, pixels, srcs)                                    # (allocates nothing the capture keeps)
        torch.cuda.current_stream().synchronize()
        with torch.cuda.graph(g, stream=side):
            out = al(rois, lmk, pixels, srcs)
    torch.cuda.current_stream().wait_stream(side)
    seen = set()
    for k in (1, 2, 0, 1):
        refill(k)
        g.replay()
        torch.cuda.synchronize()
        seen.update(check(out, (rois, lmk, pixels, srcs), f"replay of set {k}").tolist())
    assert seen == {0, A.EMPTY, A.BAD_LANDMARKS}
    # two streams, their own inputs and outputs, side by side
    ins = []
    for k in (0, 1):
        px, sr = P.pack(sets[k][0], P.SQUEEZENET, DEV)
        ins.append((R.rois_to_device(sets[k][1], DEV), _dev(sets[k][2]), px, sr))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    outs = []
    for _ in range(3):
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                outs.append((i, al(*ins[i], stream=streams[i])))
    torch.cuda.synchronize()
    for i, o in outs[:2]:
        check(o, ins[i], f"stream {i}")
    for i, o in outs[2:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[i][1])), f"stream {i}, a later round"


class _AlignedCascade(_Cascade):
    """test_gpu_roi's cascade with fit + warp in the place of the crop; the landmarks are a device tensor the test fills"""

    def __init__(self, ssd_net, face_net, gallery, lmk):
        super().__init__(ssd_net, face_net, gallery)
        self.align, self.lmk = _aligner(face_net, P.SQUEEZENET, space=1), lmk

    def __call__(self, pixels, srcs):
        x, _ = self.pp(pixels, srcs, out="q")
        det, counts = self.det.run(x)
        rois, n = self.crop.select(det, counts, srcs)
        crops, status, xf, fit_status = self.align(rois, self.lmk, pixels, srcs, out="q")
        outputs = self.runner.run_batch(crops)
        res = self.matcher.match(outputs, self.gallery)
        return dict(det=det, counts=counts, rois=rois, n=n, xf=xf, fit_status=fit_status, crops=crops, status=status, outputs=outputs,
                    idx=res.idx, dist=res.dist, ids=res.ids, emb=res.embeddings)


def test_cascade_with_aligned_crops_in_one_graph(cascade_nets):
    """detect -> select -> fit -> warp -> SqueezeNet -> match captured in one graph, replayed on refilled pixels, records and landmarks:
    every replay equal to the statements applied to the device's own det"""
    import torch
    ssd_net, face, gallery = cascade_nets
    sets = _image_sets()
    S = 2 * CASCADE_MAX_ROIS
    rng = np.random.default_rng(41)
    tpl = A.scaled_template(FACE_112, (112, 112), (227, 227)).astype(np.float64)
    poses = []
    for _ in sets:
        l = np.zeros((S, 5, 2), np.float32)
        for s in range(S):
            th = rng.uniform(-0.7, 0.7)
            rot = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
            l[s] = (((tpl / 227 - 0.5) * rng.uniform(0.5, 0.9)) @ rot.T + 0.5).astype(np.float32)
        poses.append(l)
    lmk = _dev(poses[0])
    cas = _AlignedCascade(ssd_net, face, gallery, lmk)
    cap = max(P.pack_host(s, P.SSD300)[0].size for s in sets)
    pixels = torch.zeros(cap, dtype=torch.uint8, device=DEV)
    srcs = torch.zeros(2, P.SRC_WORDS, dtype=torch.int32, device=DEV)
    P.pack(sets[0], P.SSD300, DEV, pixels=pixels, srcs=srcs)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cas(pixels, srcs)                                              # warm the launch plans of this stream's workspaces
        torch.cuda.current_stream().synchronize()
        with torch.cuda.graph(g, stream=side):
            out = cas(pixels, srcs)
    torch.cuda.current_stream().wait_stream(side)
    warped = 0
    for k in (1, 0):
        P.pack(sets[k], P.SSD300, DEV, pixels=pixels, srcs=srcs)
        lmk.copy_(torch.from_numpy(poses[k]))
        g.replay()
        torch.cuda.synchronize()
        want_rois, want_n = cas.crop.reference_select(out["det"], out["counts"], srcs)
        _same_table(out["rois"], out["n"], want_rois, want_n, f"set {k}")
        want_crops, want_status, want_xf, want_fst = cas.align.reference(want_rois, poses[k], pixels, srcs, out="q")
        assert A.xforms_to_host(out["xf"]).tobytes() == want_xf.tobytes()
        assert np.array_equal(out["fit_status"].cpu().numpy(), want_fst) and np.array_equal(out["status"].cpu().numpy(), want_status)
        assert (want_status == 0).sum() == want_n.sum() and (want_status[want_status != 0] == A.EMPTY).all()
        assert np.array_equal(out["crops"].cpu().numpy(), want_crops)
        assert len(np.unique(want_crops[want_status == 0])) > 4 and (want_crops[want_status != 0] == 0).all()
        upright = cas.crop.reference_crop(pixels, srcs, want_rois, out="q")[0]
        assert not np.array_equal(want_crops, upright)                  # not the upright boxes
        ref, _ = cas.matcher.reference(out["outputs"], gallery)
        assert np.array_equal(out["idx"].cpu().numpy(), ref.idx) and np.array_equal(out["ids"].cpu().numpy(), ref.ids)
        assert np.array_equal(out["dist"].cpu().numpy().view(np.uint32), ref.dist.view(np.uint32))
        assert np.array_equal(out["emb"].cpu().numpy().view(np.uint32), ref.embeddings.view(np.uint32))
        warped += int(want_n.sum())
    assert warped >= 2 and out["outputs"].shape == (S, 128)
