"""Antialiased second-stage crops on the MI355X (tf2_roi_crop_aa, roi_crop_aa.hip): bit-identical to roi.reference_crop_aa in float32
and int8 on a 227 x 227 net (edge tiles on both axes) and a 224 x 224 net, over sources with offsets, padded rows, 3- and 4-byte pixels
and 1 x N / N x 1 images, with boxes that upscale, sit at scale exactly 1, downscale 1.5x and about 7x from fractional corners, touch
each image edge, have a side of exactly 32 times the output (the longest filter a valid slot can have) and make a tile walk an odd
number of chunks; empty and malformed slots, BOX_OUTSIDE and BAD_SCALE among them, between good ones; the whole-image identity with
tf2_preprocess_aa on the device; a misaligned output; select + crop captured in one graph and replayed on refilled pixels, records and
det, and two streams side by side; the detect -> select -> crop -> embed -> match cascade with DeviceCropper(antialias=True)."""
from dataclasses import replace

import numpy as np
import pytest

from tf2_amd import config as cfg, preprocess as P, roi as R, synth
from tf2_amd.network import NetWork

from tests.test_gpu_roi import CASCADE_MAX_ROIS, _Cascade, _image_sets, _same_table, cascade_nets  # noqa: F401  (cascade_nets: a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK, TILE_H = 16, 8            # source rows of a chunk, output rows of a tile (roi_crop_aa.hip)


def _host_net(tables, seed=1):
    """a net handle with a q table (all tf2_roi_crop_aa reads of it: image size, Q0)"""
    net = NetWork(tables)
    net.Quantization(synth.q_text(synth.synth_q_values(tables, seed)))
    return net


@pytest.fixture(scope="module")
def nets():
    return {224: _host_net(cfg.resnet50_tables()), 227: _host_net(cfg.squeezenet11_tables())}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _src_words(recs):
    return _dev(np.ascontiguousarray(recs).view(np.int32).reshape(len(recs), P.SRC_WORDS).copy())


def _pack(rng, sizes, pb, past_the_buffer=False):
    """a pixel buffer and records: gaps before each image (nonzero offsets), rows padded past w * pb, and optionally a last record
    whose extent leaves the buffer"""
    recs = np.zeros(len(sizes) + int(past_the_buffer), P.SRC_DTYPE)
    at = int(rng.integers(1, 64))
    for i, (h, w) in enumerate(sizes):
        pitch = w * pb + (i % 3) * int(rng.integers(1, 33))
        recs[i] = (at, h, w, pitch, 0, 0, -7, 0, 0)               # resize_* / crop_* are not read
        at += (h - 1) * pitch + w * pb + int(rng.integers(0, 100))
    if past_the_buffer:
        recs[len(sizes)] = (at - 100, 50, 50, 50 * pb, 50, 50, 0, 0, 0)
    return rng.integers(0, 256, at, dtype=np.uint8), recs


def _table(rows):
    rois = np.zeros(len(rows), R.ROI_DTYPE)
    for k, (image, x0, y0, x1, y1) in enumerate(rows):
        rois[k] = (image, 15, k, 0.5, x0, y0, x1, y1)
    return rois


def _taps_and_chunks(roi, rec, oh, ow):
    """from the statement: the longest filter of the slot on either axis, and the chunk count of each of its tile rows"""
    xn = P.aa_coefs_box(int(rec["w"]), roi["x0"], roi["x1"], ow)[1]
    ylo, yn, _ = P.aa_coefs_box(int(rec["h"]), roi["y0"], roi["y1"], oh)
    chunks = []
    for y in range(0, oh, TILE_H):
        last = min(y + TILE_H, oh) - 1
        chunks.append(-(-int(ylo[last] + yn[last] - ylo[y]) // CHUNK))
    return max(int(xn.max()), int(yn.max())), chunks


def _same(got, want, where):
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape, where
    view = np.uint8 if g.dtype == np.int8 else np.uint32
    bad = np.argwhere(g.view(view) != want.view(view))
    assert bad.size == 0, (where, len(bad), bad[:5], g[tuple(bad[0])], want[tuple(bad[0])])
    return g


SIZES = [(1640, 1620), (40, 33), (1, 257), (300, 1), (8, 7264)]


def _good_rois(hw):
    """{family: rows} on the sources SIZES for a hw x hw output"""
    H, W = SIZES[0]
    f = np.float32
    return {
        "upscale": [(1, 10.3, 7.7, 17.3, 12.7)],
        "scale 1": [(0, 100.0, 50.0, 100.0 + hw, 50.0 + hw)],
        "1.5x": [(0, 20.25, 30.5, f(20.25) + f(1.5 * hw), f(30.5) + f(1.5 * hw))],
        "7x": [(0, 10.3, 7.7, f(10.3) + f(7.03 * hw), f(7.7) + f(6.97 * hw))],
        "edges": [(0, 0.0, 300.5, 400.25, 700.75), (0, 300.5, 0.0, 700.25, 410.5), (0, W - 350.5, 200.25, float(W), 640.75),
                  (0, 100.5, H - 500.25, 560.75, float(H))],
        "32x": [(4, 7264.0 - 32 * hw, 0.0, 7264.0, 8.0)],
        "1 x N": [(2, 0.0, 0.0, 257.0, 1.0)],
        "N x 1": [(3, 0.0, 10.5, 1.0, 290.25)],
        "odd chunks": [(0, 50.5, 100.25, 550.75, f(100.25) + f(4.1 * hw))],
    }


@pytest.mark.parametrize("hw,preset,src_order", [(227, P.SQUEEZENET, "RGB"), (227, P.GOOGLENET, "BGRA"), (224, P.RESNET50, "RGBA"),
                                                 (224, P.TORCHVISION, "BGR")])
def test_crop_aa_bit_identical(nets, hw, preset, src_order):
    import torch
    rng = np.random.default_rng(hw + len(src_order))
    pb = len(src_order)
    pixels, recs = _pack(rng, SIZES, pb)
    families = _good_rois(hw)
    rois = _table([row for rows in families.values() for row in rows])
    assert len(rois) == 12
    c = R.DeviceCropper(nets[hw], preset, src_order, antialias=True)
    assert c.out_hw == (hw, hw)
    # the case list does what it says, by the statement: every slot valid, the longest filter and an odd chunk count >= 3 reached
    status = R.roi_status_aa(rois, recs, pb, pixels.size, c.out_hw)
    assert status.tolist() == [0] * 12
    first, at = {}, 0
    for name, rows in families.items():
        first[name], at = at, at + len(rows)
    assert all(status[first[name]:first[name] + len(rows)].tolist() == [0] * len(rows) for name, rows in families.items())
    tc = [_taps_and_chunks(r, recs[int(r["image"])], hw, hw) for r in rois]
    # (2 * 32 + 1 = 65 is the bound of a coefficient row; with 2 * support <= 64 the rule's hi - lo is at most 64, which a side of
    # exactly 32 * hw gives at every alignment -- tests/test_roi_aa.py)
    assert max(t for t, _ in tc) == 2 * P.AA_MAX_SCALE and tc[first["32x"]][0] == 2 * P.AA_MAX_SCALE
    assert any(n >= 3 and n % 2 == 1 for n in tc[first["odd chunks"]][1]) and any(n >= 4 and n % 2 == 0 for n in tc[first["7x"]][1])
    assert tc[first["upscale"]][0] <= 3 and tc[first["scale 1"]][0] == 2 and all(n == 1 for k in (0, 1) for n in tc[k][1])
    px, sr, rt = _dev(pixels), _src_words(recs), R.rois_to_device(rois, DEV)
    for out in ("f32", "q"):
        got, st = c.crop(px, sr, rt, out=out)
        torch.cuda.synchronize()
        want, wst = c.reference_crop(pixels, recs, rois, out=out)
        assert wst.tolist() == [0] * 12 and st.cpu().numpy().tolist() == [0] * 12
        g = _same(got, want, out)
        assert len(np.unique(g)) > 4 and (out == "q" or all(len(np.unique(g[s])) > 4 for s in range(12)))


def test_bad_slots_between_good_ones(nets):
    import torch
    rng = np.random.default_rng(5)
    pixels, recs = _pack(rng, [(300, 400), (40, 33), (3, 7400)], 3, past_the_buffer=True)
    nan, good = np.nan, (0, 20.5, 30.25, 380.0, 290.75)
    rows = [
        (good, 0), ((-1, 0.0, 0.0, 0.0, 0.0), R.EMPTY), ((4, 0.0, 0.0, 10.0, 10.0), R.BAD_IMAGE), ((1, 3.3, 4.4, 30.3, 39.9), 0),
        ((1, nan, 0.0, 10.0, 10.0), R.BAD_BOX), ((1, 5.0, 5.0, 5.5, 30.0), R.BAD_BOX), (good, 0), ((3, 0.0, 0.0, 50.0, 50.0), R.BAD_SRC),
        ((0, -0.5, 0.0, 100.0, 100.0), R.BOX_OUTSIDE), ((0, 0.0, 0.0, 400.5, 300.0), R.BOX_OUTSIDE), (good, 0),
        ((2, 0.0, 0.0, 7300.0, 3.0), R.BAD_SCALE), ((2, 100.0, 0.0, 7400.5, 3.0), R.BOX_OUTSIDE | R.BAD_SCALE),
        ((2, 10.0, 0.0, 7000.0, 3.0), 0),
    ]
    rois, want_status = _table([r for r, _ in rows]), [bits for _, bits in rows]
    c = R.DeviceCropper(nets[227], P.SQUEEZENET, "RGB", antialias=True)
    assert R.roi_status_aa(rois, recs, 3, pixels.size, c.out_hw).tolist() == want_status
    px, sr, rt = _dev(pixels), _src_words(recs), R.rois_to_device(rois, DEV)
    for out in ("f32", "q"):
        got, st = c.crop(px, sr, rt, out=out)
        torch.cuda.synchronize()
        want, wst = c.reference_crop(pixels, recs, rois, out=out)
        assert wst.tolist() == want_status and st.cpu().numpy().tolist() == want_status
        g = _same(got, want, out)
        assert all((g[s] == 0).all() for s, bits in enumerate(want_status) if bits) and len(np.unique(g)) > 4
        assert out == "q" or all(len(np.unique(g[s])) > 2 for s, bits in enumerate(want_status) if not bits)
        assert np.array_equal(g[0], g[6]) and np.array_equal(g[0], g[10])      # the good slots between them are what they are alone


@pytest.mark.parametrize("hw,preset", [(227, replace(P.SQUEEZENET, antialias=True)), (224, P.TORCHVISION_PIL)])
def test_whole_image_rois_equal_tf2_preprocess_aa(nets, hw, preset):
    """roi_crop_aa on (0, 0, w, h) == tf2_preprocess_aa with resize = (hw, hw) and crop (0, 0), on the device, float32 and int8"""
    import torch
    rng = np.random.default_rng(hw)
    sizes = [(375, 500), (500, 333), (hw, hw), (97, 131), (1, 40), (33, 1), (640, 479)]
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
    pixels, recs, pb = P.pack_host(imgs, preset, align=16)
    recs["resize_h"], recs["resize_w"], recs["crop_y"], recs["crop_x"] = hw, hw, 0, 0
    px, sr = _dev(pixels), _src_words(recs)
    pp, c = P.Preprocessor(nets[hw], preset, "RGB"), R.DeviceCropper(nets[hw], preset, "RGB")
    assert c.antialias
    rois = R.rois_to_device(R.whole_image_rois(recs), DEV)
    for out in ("f32", "q"):
        want, wst = pp(px, sr, out=out)
        got, st = c.crop(px, sr, rois, out=out)
        torch.cuda.synchronize()
        assert (wst.cpu() == 0).all() and (st.cpu() == 0).all()
        assert torch.equal(got.cpu().view(torch.uint8), want.cpu().view(torch.uint8))
        assert len(torch.unique(got.cpu())) > 4


def test_crop_aa_into_a_misaligned_output(nets):
    import torch
    rng = np.random.default_rng(12)
    pixels, recs = _pack(rng, [(300, 400), (40, 33)], 3)
    rois = _table([(0, 20.5, 30.25, 380.0, 290.75), (-1, 0.0, 0.0, 0.0, 0.0), (1, 3.3, 4.4, 30.3, 39.9), (0, 0.0, 0.0, 400.0, 300.0)])
    c = R.DeviceCropper(nets[224], P.RESNET50, "RGB", antialias=True)
    px, sr, rt = _dev(pixels), _src_words(recs), R.rois_to_device(rois, DEV)
    S, (oh, ow) = len(rois), c.out_hw
    for out in ("f32", "q"):
        flat = torch.zeros(S * 3 * oh * ow + 1, dtype=torch.int8 if out == "q" else torch.float32, device=DEV)
        images = flat[1:].view(S, 3, oh, ow)                      # one element past the allocation's start
        assert images.data_ptr() % (4 if out == "q" else 16) != 0
        got, st = c.crop(px, sr, rt, out=out, images=images)
        torch.cuda.synchronize()
        want, wst = c.reference_crop(pixels, recs, rois, out=out)
        assert wst.tolist() == [0, R.EMPTY, 0, 0] and st.cpu().numpy().tolist() == wst.tolist()
        _same(got, want, out)
        assert flat[0].item() == 0


def _det_set(seed, sizes, boxes):
    """images of `sizes`, and det / counts (21 classes, top_k 200) holding boxes[b] = [(score, x1, y1, x2, y2)..] as class 15 of image b"""
    rng = np.random.default_rng(seed)
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
    det, counts = np.zeros((len(sizes), 21, 200, 5), np.float32), np.zeros((len(sizes), 21), np.int32)
    for b, rows in enumerate(boxes):
        if rows:
            det[b, 15, :len(rows)] = rows
            counts[b, 15] = len(rows)
    return imgs, det, counts


SETS = [
    ((375, 500), (300, 300), [[(0.9, 0.1, 0.1, 0.6, 0.7), (0.8, 0.3, 0.2, 0.95, 0.9), (0.3, 0.0, 0.0, 1.0, 1.0)],
                              [(0.7, -0.2, 0.25, 0.5, 1.3)]]),
    ((120, 90), (640, 480), [[(0.95, 0.4, 0.4, 0.6, 0.6)],
                             [(0.6 + 0.05 * k, 0.1 * k, 0.05 * k, 0.5 + 0.1 * k, 0.45 + 0.1 * k) for k in range(6)]]),
    ((333, 500), (227, 227), [[], [(0.99, 0.0, 0.0, 1.0, 1.0), (0.51, 0.2, 0.3, 0.21, 0.9)]]),
]


def test_graph_replay_with_refilled_buffers_and_two_streams(nets):
    """select + crop_aa captured once; pixels, records and det refilled with other sizes, boxes and scales; each replay against the
    statement.  Then two streams with their own inputs and outputs side by side."""
    import torch
    c = R.DeviceCropper(nets[227], P.SQUEEZENET, "RGB", max_rois=4, expand=(1.1, 1.2), antialias=True)
    sets = [_det_set(k, s[:2], s[2]) for k, s in enumerate(SETS)]
    cap = max(P.pack_host(s[0], P.SQUEEZENET)[0].size for s in sets)
    pixels = torch.zeros(cap, dtype=torch.uint8, device=DEV)
    srcs = torch.zeros(2, P.SRC_WORDS, dtype=torch.int32, device=DEV)
    det, counts = _dev(sets[0][1]), _dev(sets[0][2])

    def refill(k):
        P.pack(sets[k][0], P.SQUEEZENET, DEV, pixels=pixels, srcs=srcs)
        det.copy_(torch.from_numpy(sets[k][1]))
        counts.copy_(torch.from_numpy(sets[k][2]))

    def check(out, inputs, where):
        want_img, want_st, want_rois, want_n = c.reference(*inputs, out="q")
        _same_table(out[2], out[3], want_rois, want_n, where)
        assert np.array_equal(out[1].cpu().numpy(), want_st), where
        _same(out[0], want_img, where)
        return want_st

    refill(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c(det, counts, pixels, srcs)                                   # (allocates nothing the capture keeps)
        torch.cuda.current_stream().synchronize()
        with torch.cuda.graph(g, stream=side):
            out = c(det, counts, pixels, srcs)
    torch.cuda.current_stream().wait_stream(side)
    seen = set()
    for k in (1, 2, 0, 1):
        refill(k)
        g.replay()
        torch.cuda.synchronize()
        seen.update(check(out, (det, counts, pixels, srcs), f"replay of set {k}").tolist())
    assert seen == {0, R.EMPTY}                                        # ROIs to crop, and slots that stay empty
    # two streams, their own inputs and outputs, side by side
    ins = []
    for k in (0, 1):
        px, sr = P.pack(sets[k][0], P.SQUEEZENET, DEV)
        ins.append((_dev(sets[k][1]), _dev(sets[k][2]), px, sr))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    outs = []
    for _ in range(3):
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                outs.append((i, c(*ins[i], stream=streams[i])))
    torch.cuda.synchronize()
    for i, o in outs[:2]:
        check(o, ins[i], f"stream {i}")
    for i, o in outs[2:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[i][1])), f"stream {i}, a later round"


def test_cascade_with_antialiased_crops(cascade_nets):
    """detect -> select -> crop_aa -> SqueezeNet -> match against the statements applied to the device's own det"""
    import torch
    ssd_net, face, gallery = cascade_nets
    cas = _Cascade(ssd_net, face, gallery)
    plain = cas.crop
    cas.crop = R.DeviceCropper(face, P.SQUEEZENET, "RGB", classes=plain.classes, min_score=plain.min_score, max_rois=plain.max_rois,
                               expand=plain.expand, square=plain.square, antialias=True)
    pixels, srcs = P.pack(_image_sets()[0], P.SSD300, DEV)
    out = cas(pixels, srcs)
    torch.cuda.synchronize()
    want_rois, want_n = cas.crop.reference_select(out["det"], out["counts"], srcs)
    assert want_n.max() >= 1 and (want_n < CASCADE_MAX_ROIS).any()          # a ROI to crop, and a slot that stays empty
    _same_table(out["rois"], out["n"], want_rois, want_n, "cascade")
    want_crops, want_status = cas.crop.reference_crop(pixels, srcs, want_rois, out="q")
    assert np.array_equal(out["status"].cpu().numpy(), want_status)
    assert (want_status == 0).sum() == want_n.sum() and (want_status[want_status != 0] == R.EMPTY).all()
    assert np.array_equal(out["crops"].cpu().numpy(), want_crops)
    assert len(np.unique(want_crops[want_status == 0])) > 4 and (want_crops[want_status != 0] == 0).all()
    assert not np.array_equal(want_crops, plain.reference_crop(pixels, srcs, want_rois, out="q")[0])    # not the two-tap crops
    ref, _ = cas.matcher.reference(out["outputs"], gallery)
    assert np.array_equal(out["idx"].cpu().numpy(), ref.idx) and np.array_equal(out["ids"].cpu().numpy(), ref.ids)
    assert np.array_equal(out["dist"].cpu().numpy().view(np.uint32), ref.dist.view(np.uint32))
    assert np.array_equal(out["emb"].cpu().numpy().view(np.uint32), ref.embeddings.view(np.uint32))
    assert out["outputs"].shape == (2 * CASCADE_MAX_ROIS, 128)
