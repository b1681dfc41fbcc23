"""Antialiased preprocessing on the MI355X (tf2_preprocess_aa, preprocess_aa.hip): float32 and int8 outputs bit-identical to the
statement preprocess.reference_aa (Pillow's Image.resize(BILINEAR) restated) for mixed batches -- identity, non-integer downscales,
exactly 32x on one axis, upscales from 1 x 1 / 1 x N / N x 1, one axis up and the other down; crops at both corners, padded pitches,
offsets, 3- and 4-byte pixels, RGB and BGR sources, random and 0 / 255 pixels; an output width that is no multiple of the tile width
(227) -- malformed records (status codes, zeros, the rest exact), a captured graph replayed on refilled buffers, two streams side by
side, and ResNet-50 end to end on the int8 output."""
import os

import numpy as np
import pytest

from tf2_amd import config as cfg, preprocess as P, synth
from tf2_amd.network import NetWork, Runner

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIL = P.TORCHVISION_PIL


def _host_net(tables, seed=1):
    """a net handle with a q table (all tf2_preprocess_aa reads of it: image size, Q0)"""
    net = NetWork(tables)
    net.Quantization(synth.q_text(synth.synth_q_values(tables, seed)))
    return net


@pytest.fixture(scope="module")
def nets():
    return {224: _host_net(cfg.resnet50_tables()), 227: _host_net(cfg.squeezenet11_tables())}


def _dev(pixels, recs):
    import torch
    return (torch.from_numpy(pixels).to("cuda:0"),
            torch.from_numpy(np.ascontiguousarray(recs).view(np.int32).reshape(len(recs), P.SRC_WORDS).copy()).to("cuda:0"))


def _check(pp, pixels, srcs, want_status=None):
    import torch
    for out in ("f32", "q"):
        got, st = pp(pixels, srcs, out=out)
        torch.cuda.synchronize()
        want, wst = pp.reference(pixels, srcs, out=out)
        assert np.array_equal(st.cpu().numpy(), wst), (st.cpu().numpy(), wst)
        if want_status is not None:
            assert st.cpu().numpy().tolist() == want_status
        g = got.cpu().numpy()
        assert g.dtype == want.dtype and g.shape == want.shape
        bad = np.argwhere(g.view(np.uint8 if out == "q" else np.uint32) != want.view(np.uint8 if out == "q" else np.uint32))
        assert bad.size == 0, (out, len(bad), bad[:5], g[tuple(bad[0])], want[tuple(bad[0])])


def _mixed(rng, batch, pb, out_hw):
    """a pixel buffer and records of `batch` images, seven kinds of geometry in turn (a batch of 1 is a non-integer downscale): gaps
    before each image, rows padded past w * pb, the crop at (0, 0), at (rh - oh, rw - ow) or anywhere between; every third image
    holds only 0 and 255 bytes.  Sources stay small where the geometry allows (the numpy statement runs on them too)."""
    oh, ow = out_hw
    recs = np.zeros(batch, P.SRC_DTYPE)
    at = int(rng.integers(0, 64))
    n32 = 0
    for i in range(batch):
        kind = (i + 1) % 7
        if kind == 0:                                  # identity
            h, w, rh, rw = oh, ow, oh, ow
        elif kind == 1:                                # downscale between 1x and 3x, non-integer
            rh, rw = oh + int(rng.integers(0, 40)), ow + int(rng.integers(0, 40))
            h, w = int(rh * rng.uniform(1.05, 2.9)) + 1, int(rw * rng.uniform(1.05, 2.9)) + 1
        elif kind == 2 and n32 < 2:                    # exactly 32x on one axis, 1x on the other (7168 x 224 -> 224 x 224)
            rh, rw = oh, ow
            h, w = (32 * oh, ow) if n32 == 0 else (oh, 32 * ow)
            n32 += 1
        elif kind == 2:                                # (further ones: a larger non-integer downscale, 4x .. 6x on one axis)
            rh, rw = oh + int(rng.integers(0, 9)), ow + int(rng.integers(0, 9))
            h, w = int(rh * rng.uniform(4.0, 6.0)), rw + int(rng.integers(0, 30))
        elif kind == 3:                                # upscale from 1 x 1 and from small odd sources
            h, w = (1, 1) if i < 7 else (int(rng.integers(1, 40)), int(rng.integers(1, 40)))
            rh, rw = oh + int(rng.integers(0, 50)), ow + int(rng.integers(0, 50))
        elif kind == 4:                                # 1 x N
            h, w = 1, int(rng.integers(2, 200))
            rh, rw = oh + int(rng.integers(0, 9)), ow + int(rng.integers(0, 9))
        elif kind == 5:                                # N x 1
            h, w = int(rng.integers(2, 200)), 1
            rh, rw = oh + int(rng.integers(0, 9)), ow + int(rng.integers(0, 9))
        else:                                          # one axis up, the other down
            h, w = int(rng.integers(oh // 3, oh)), int(rng.integers(ow + 41, 3 * ow))
            rh, rw = oh + int(rng.integers(0, 40)), ow + int(rng.integers(0, 40))
            if i % 2:
                h, w, rh, rw = w, h, rw, rh
                rh, rw = max(rh, oh), max(rw, ow)
        pitch = w * pb + int(rng.integers(0, 3)) * int(rng.integers(1, 33))
        corner = i % 3
        cy, cx = ((0, 0), (rh - oh, rw - ow), (int(rng.integers(0, rh - oh + 1)), int(rng.integers(0, rw - ow + 1))))[corner]
        recs[i] = (at, h, w, pitch, rh, rw, cy, cx, 0)
        at += (h - 1) * pitch + w * pb + int(rng.integers(0, 100))
    pixels = rng.integers(0, 256, at, dtype=np.uint8)
    for i in range(0, batch, 3):                       # 0 / 255 images
        r = recs[i]
        a, b = int(r["offset"]), int(r["offset"]) + (int(r["h"]) - 1) * int(r["row_pitch"]) + int(r["w"]) * pb
        pixels[a:b] = (pixels[a:b] >> 7) * 255
    return pixels, recs


@pytest.mark.parametrize("batch", [1, 7, 33])
@pytest.mark.parametrize("hw", [224, 227])
@pytest.mark.parametrize("src_order", ["BGR", "RGBA"])
def test_mixed_batches_bit_identical(nets, batch, hw, src_order):
    rng = np.random.default_rng(batch * 11 + hw + len(src_order))
    pixels, recs = _mixed(rng, batch, len(src_order), (hw, hw))
    assert (P.record_status_aa(recs, len(src_order), pixels.size, (hw, hw)) == 0).all()
    if batch >= 7:
        assert any(int(r["h"]) == 32 * int(r["resize_h"]) and r["w"] == r["resize_w"] for r in recs)
        assert any(r["h"] == 1 and r["w"] == 1 for r in recs)
    _check(P.Preprocessor(nets[hw], PIL, src_order), *_dev(pixels, recs), [0] * batch)


def test_malformed_records(nets):
    """valid and malformed records in one batch: the codes of the statement, zeros for the bad images, the rest exact.  BAD_SCALE by
    one pixel (h = 32 * rh + 1, and 32 * rh beside it), alone and with other bits; an out-of-buffer record ending exactly one byte
    past the buffer."""
    rng = np.random.default_rng(12)
    oh = ow = 224
    pixels, recs = _mixed(rng, 14, 3, (oh, ow))
    n = pixels.size
    last = recs[13].copy()
    bad = recs.copy()
    tall = (0, 32 * oh + 1, 8, 24, oh, ow + 3, 0, 3, 0)                # 7169 x 8 -> 224 x 227: in the buffer, one row too many
    assert 7169 * 24 <= n
    bad[1] = tall
    bad[2] = tall
    bad[2]["h"] = 32 * oh                                              # the bound itself: valid
    bad[3] = tall
    bad[3]["crop_x"] = 4                                               # + BAD_CROP
    bad[4]["offset"] = n - ((last["h"] - 1) * last["row_pitch"] + last["w"] * 3) + 1
    for k in ("h", "w", "row_pitch"):
        bad[4][k] = last[k]
    bad[5] = tall
    bad[5]["offset"] = n - (7169 - 1) * 24 - 8 * 3 + 1                 # + OUT_OF_BUFFER by one byte
    bad[6] = (0, 4, 32 * ow + 1, (32 * ow + 1) * 3, oh, ow, 0, 0, 0)   # the same on the other axis
    bad[7]["h"] = 40000                                                # BAD_SIZE: the scale is not evaluated
    bad[8]["resize_w"] = 0                                             # BAD_RESIZE (+ BAD_CROP): not evaluated either (w > 32 * 0)
    bad[9]["row_pitch"] = bad[9]["w"] * 3 - 1
    bad[10]["offset"] = -1
    want = P.record_status_aa(bad, 3, n, (oh, ow))
    assert want.tolist()[:11] == [0, P.BAD_SCALE, 0, P.BAD_SCALE | P.BAD_CROP, P.OUT_OF_BUFFER, P.BAD_SCALE | P.OUT_OF_BUFFER, P.BAD_SCALE,
                                  P.BAD_SIZE, P.BAD_RESIZE | P.BAD_CROP, P.BAD_PITCH, P.BAD_OFFSET], want
    assert (want[11:] == 0).all()
    pp = P.Preprocessor(nets[224], PIL, "RGB")
    _check(pp, *_dev(pixels, bad), want.tolist())
    got, st = pp(*_dev(pixels, bad), out="f32")
    g = got.cpu().numpy()
    assert (g[want != 0] == 0).all() and all((g[i] != 0).any() for i in np.flatnonzero(want == 0))


def test_graph_replay_with_refilled_buffers_and_two_streams(nets):
    """capture tf2_preprocess_aa once, refill the pixel buffer and the records with images of other sizes and scales, replay: every
    replay is the statement.  Then two streams with their own batches side by side."""
    import torch
    pp = P.Preprocessor(nets[224], PIL, "RGB")
    rng = np.random.default_rng(6)
    sets = [[rng.integers(0, 256, (int(rng.integers(100, 600)), int(rng.integers(100, 600)), 3), dtype=np.uint8) for _ in range(4)]
            for _ in range(3)]
    packed = [P.pack_host(s, PIL) for s in sets]
    wants = {out: [pp.reference(px, sr.view(np.int32).reshape(4, P.SRC_WORDS), out=out) for px, sr, _ in packed] for out in ("q", "f32")}
    assert all((st == 0).all() for _, st in wants["q"])
    cap = max(px.size for px, _, _ in packed)
    pixels = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    srcs = torch.zeros(4, P.SRC_WORDS, dtype=torch.int32, device="cuda:0")
    P.pack(sets[0], PIL, "cuda:0", pixels=pixels, srcs=srcs)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pp(pixels, srcs, out="q")
        torch.cuda.current_stream().synchronize()
        with torch.cuda.graph(g, stream=side):
            x, st = pp(pixels, srcs, out="q")
            xf, stf = pp(pixels, srcs, out="f32")
    torch.cuda.current_stream().wait_stream(side)
    for k in (1, 2, 0, 1):
        P.pack(sets[k], PIL, "cuda:0", pixels=pixels, srcs=srcs)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(x.cpu().numpy(), wants["q"][k][0]) and (st.cpu() == 0).all()
        assert np.array_equal(xf.cpu().numpy().view(np.uint32), wants["f32"][k][0].view(np.uint32)) and (stf.cpu() == 0).all()
    # two streams, their own inputs, side by side
    ins = [P.pack(s, PIL, "cuda:0") for s in sets[:2]]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream()); s2.wait_stream(torch.cuda.current_stream())
    outs = []
    for _ in range(4):
        outs.append((pp(*ins[0], out="q", stream=s1), pp(*ins[1], out="f32", stream=s2)))
    torch.cuda.synchronize()
    for (a, sa), (b, sb) in outs:
        assert np.array_equal(a.cpu().numpy(), wants["q"][0][0]) and (sa.cpu() == 0).all()
        assert np.array_equal(b.cpu().numpy().view(np.uint32), wants["f32"][1][0].view(np.uint32)) and (sb.cpu() == 0).all()


def test_resnet50_end_to_end():
    """pack -> Preprocessor(TORCHVISION_PIL, out="q") -> Runner.run_batch == the same net on the statement's int8 output"""
    import torch
    t = cfg.resnet50_tables()
    qv = np.loadtxt(os.path.join(ROOT, "tests", "golden", "resnet50_Q"), dtype=np.int32)
    net = NetWork(t)
    net.Init(synth.synth_model(t, qv, 0), synth.q_text(qv), device="cuda:0")
    rng = np.random.default_rng(4)
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((375, 500), (480, 301))]
    pp = P.Preprocessor(net, PIL, "RGB")
    pixels, srcs = P.pack(imgs, PIL, "cuda:0")
    xq, st = pp(pixels, srcs, out="q")
    got = Runner(None, net).run_batch(xq).clone()
    wq, wst = pp.reference(pixels, srcs, out="q")
    want = Runner(None, net).run_batch(torch.from_numpy(wq).to("cuda:0")).clone()
    torch.cuda.synchronize()
    assert (st.cpu() == 0).all() and (wst == 0).all()
    assert np.array_equal(xq.cpu().numpy(), wq)
    assert torch.equal(got.cpu(), want.cpu()) and int(got.cpu().abs().sum()) > 0
