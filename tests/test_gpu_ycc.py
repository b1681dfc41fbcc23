"""YCbCr frames on the MI355X (tf2_ycc_to_rgb, ycc_convert.hip): the whole pixel buffer after the call, and the statuses, bit-identical
to the statement ycc.reference -- mixed batches of the smallest sizes that can go wrong (1 x 1, 2 x 9, 9 x 2, 17 x 33, one below, at
and one above the kernel's tile) across every layout, subsampling, upsampling rule and matrix, 3- and 4-byte pixels with permuted
channels, padded pitches, offsets of every residue mod 4 (the dword and the byte paths in one batch), guard bytes, 0 / 255 planes;
blocks_per_image 1, 3 and the default; malformed records; Pillow's own RGB of the fixture's planes; the chain into tf2_preprocess_aa,
tf2_preprocess and tf2_roi_crop; and convert + preprocess + network + classify in one captured graph replayed on refilled planes."""
import os
import sys
from dataclasses import replace

import numpy as np
import pytest

from tf2_amd import classify as K, config as cfg, preprocess as P, roi as R, synth, ycc as Y
from tf2_amd.network import NetWork, Runner

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_ycc_golden as G  # noqa: E402

# the smallest sizes at which the kernel takes another path: one pixel, one chroma column, one chroma row, odd sizes, and one below,
# at and one above its tile (the constants are the binding's, checked against the header in tests/test_ycc.py)
SIZES = [(1, 1), (2, 9), (9, 2), (17, 33), (Y.TILE_H - 1, Y.TILE_W - 1), (Y.TILE_H, Y.TILE_W), (Y.TILE_H + 1, Y.TILE_W + 1)]
LAYOUTS = [Y.PLANAR, Y.SEMI_CBCR, Y.SEMI_CRCB, Y.GRAY]
OUTS = [(3, (0, 1, 2)), (3, (2, 0, 1)), (4, (0, 1, 2)), (4, (3, 0, 2))]


def mixed(rng, sizes, layout, sub, pb):
    """A source buffer, both record tables and the size of a pixel buffer for images of `sizes`.  Image i's offsets (every plane's and
    the destination's) are i mod 4 modulo 4; images 0, 4, .. also have pitches that are multiples of 4 (the dword paths), the others
    any pitch from the row's bytes up.  Gaps of guard bytes lie before every plane and behind every row; odd images hold 0 / 255 only."""
    sub = (1, 1) if layout == Y.GRAY else sub
    n = len(sizes)
    yrec, srec = np.zeros(n, Y.YCC_DTYPE), np.zeros(n, P.SRC_DTYPE)
    planes, at, dat = [], 0, 0

    def place(rows, row_bytes, i, at):
        pitch = row_bytes + int(rng.integers(0, 9))
        if i % 4 == 0:
            pitch = -(-pitch // 4) * 4 + 4 * int(rng.integers(0, 2))
        off = -(-(at + int(rng.integers(1, 20))) // 4) * 4 + i % 4
        return off, pitch, off + (rows - 1) * pitch + row_bytes

    for i, (h, w) in enumerate(sizes):
        ch, cw = Y.chroma_size(h, w, sub)
        crow = cw if layout == Y.PLANAR else 2 * cw
        oy, py, at = place(h, w, i, at)
        ocb = ocr = pc = 0
        if layout != Y.GRAY:
            ocb, pc, at = place(ch, crow, i, at)
        if layout == Y.PLANAR:
            ocr, _, at = place(ch, crow, i, at)
            ocr, at = ocr, ocr + (ch - 1) * pc + crow
        yrec[i] = (oy, ocb, ocr, py, pc)
        off, pitch, dat = place(h, w * pb, i, dat)
        srec[i] = (off, h, w, pitch, h, w, 0, 0, 0)
        planes.append([(oy, py, h, w)] + ([(ocb, pc, ch, crow)] if layout != Y.GRAY else []) + ([(ocr, pc, ch, crow)] if layout == Y.PLANAR else []))
    src = rng.integers(0, 256, at + int(rng.integers(0, 9)), dtype=np.uint8)
    for i in range(1, n, 2):
        for off, pitch, rows, cols in planes[i]:
            for y in range(rows):
                a = off + y * pitch
                src[a:a + cols] = (src[a:a + cols] >> 7) * 255
    return src, yrec, srec, dat + int(rng.integers(0, 9))


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr)).to("cuda:0")


def _words(recs, words):
    return _dev(Y.records_to_words(recs, words))


def run_and_check(desc, src, yrec, srec, before, want_status=None):
    """the device on host inputs: the whole pixel buffer and the statuses equal the statement; returns (pixels, status)"""
    import torch
    pixels = _dev(before)
    st = Y.DeviceConverter(desc).run(_dev(src), _words(yrec, Y.YCC_WORDS), pixels, _words(srec, P.SRC_WORDS))
    torch.cuda.synchronize()
    want, wst = Y.reference(src, yrec, srec, desc, before)
    got, gst = pixels.cpu().numpy(), st.cpu().numpy()
    assert np.array_equal(gst, wst), (gst, wst)
    if want_status is not None:
        assert gst.tolist() == list(want_status), gst
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (desc, len(bad), bad[:8], got[bad[:8]], want[bad[:8]])
    return got, gst


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("sub", Y.SUBSAMPLINGS)
@pytest.mark.parametrize("upsample", [Y.FANCY, Y.REPLICATE])
def test_mixed_batches_bit_identical(layout, sub, upsample):
    """batches of 5 drawn from SIZES in turn, so the seven sizes meet every residue and every pitch rule; every matrix and every
    output pixel on each batch.  The reference leaves every byte outside the rows' w * pixel_bytes as it was, so equality of the
    whole buffer is also the guard-byte check."""
    case = (LAYOUTS.index(layout) * 3 + Y.SUBSAMPLINGS.index(sub)) * 2 + upsample
    rng = np.random.default_rng(100 + case)
    k = 0
    for matrix in (Y.JFIF, Y.BT601, Y.BT709):
        for pb, dst in OUTS:
            sizes = [SIZES[(case + k + i) % len(SIZES)] for i in range(5)]
            k += 3
            desc = Y.Desc(layout=layout, sub=sub, upsample=upsample, matrix=matrix, pixel_bytes=pb, dst_channel=dst, alpha=7)
            src, yrec, srec, nd = mixed(rng, sizes, layout, sub, pb)
            before = rng.integers(0, 256, nd, dtype=np.uint8)
            got, _ = run_and_check(desc, src, yrec, srec, before, [0] * 5)
            assert (got != before).any()


def test_every_size_meets_every_alignment():
    """(what the rotation above rests on) over the 12 batches of one case every size of SIZES lands on an aligned slot (0, 4) and
    on an unaligned one"""
    seen = {s: set() for s in SIZES}
    for k in range(0, 36, 3):
        for i in range(5):
            seen[SIZES[(k + i) % len(SIZES)]].add(i % 4 == 0)
    assert all(v == {True, False} for v in seen.values()), seen


@pytest.mark.parametrize("sub,layout", [((2, 2), Y.PLANAR), ((2, 1), Y.SEMI_CBCR), ((1, 1), Y.SEMI_CRCB), ((2, 2), Y.GRAY)])
def test_blocks_per_image_do_not_change_the_bytes(sub, layout):
    """1, 3 and the default: an image of several tiles in both directions, walked by one block, by three, and by more blocks than
    it has tiles"""
    rng = np.random.default_rng(7)
    sizes = [(3 * Y.TILE_H + 5, 2 * Y.TILE_W + 9), (1, 1), (Y.TILE_H + 1, 3 * Y.TILE_W - 2)]
    src, yrec, srec, nd = mixed(rng, sizes, layout, sub, 3)
    before = rng.integers(0, 256, nd, dtype=np.uint8)
    outs = [run_and_check(Y.Desc(layout=layout, sub=sub, blocks_per_image=n), src, yrec, srec, before, [0] * 3)[0] for n in (1, 3, 0)]
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


@pytest.mark.parametrize("layout,sub", [(Y.PLANAR, (2, 2)), (Y.SEMI_CBCR, (2, 1))])
def test_malformed_records(layout, sub):
    """one record per status bit and a combination, between valid ones: the statuses of the statement, the malformed images' bytes
    untouched, the valid neighbours exact.  The extent cases end exactly one byte past their buffer.  The source and the pixel
    buffer are the two halves of one allocation: buffers that touch are disjoint."""
    import torch
    rng = np.random.default_rng(21)
    sizes = [SIZES[i % len(SIZES)] for i in range(3, 11)]
    src, yrec, srec, nd = mixed(rng, sizes, layout, sub, 4)
    ns = src.size
    planar = layout == Y.PLANAR
    srec[1]["w"] = 0                                           # BAD_SIZE
    yrec[2]["pitch_c"] = (1 if planar else 2) * Y.chroma_size(*sizes[2], sub)[1] - 1     # BAD_PITCH by one byte
    yrec[3]["off_cr" if planar else "off_cb"] = -1             # BAD_OFFSET
    last = "off_cr" if planar else "off_cb"
    h4, w4 = sizes[4]
    ch4, cw4 = Y.chroma_size(h4, w4, sub)
    yrec[4][last] = ns - ((ch4 - 1) * int(yrec[4]["pitch_c"]) + (cw4 if planar else 2 * cw4)) + 1      # OUT_OF_SRC by one byte
    srec[5]["offset"] = nd - ((sizes[5][0] - 1) * int(srec[5]["row_pitch"]) + sizes[5][1] * 4) + 1     # OUT_OF_DST by one byte
    srec[6]["h"], yrec[6]["pitch_y"], srec[6]["offset"] = 40000, 0, -8                                  # SIZE | PITCH | OFFSET
    desc = Y.Desc(layout=layout, sub=sub, pixel_bytes=4, dst_channel=(2, 1, 0), alpha=7)
    want = [0, Y.BAD_SIZE, Y.BAD_PITCH, Y.BAD_OFFSET, Y.OUT_OF_SRC, Y.OUT_OF_DST, Y.BAD_SIZE | Y.BAD_PITCH | Y.BAD_OFFSET, 0]
    assert Y.record_status(yrec, srec, desc, ns, nd).tolist() == want
    before = rng.integers(0, 256, nd, dtype=np.uint8)
    both = torch.empty(ns + nd, dtype=torch.uint8, device="cuda:0")
    both[:ns].copy_(torch.from_numpy(src))
    both[ns:].copy_(torch.from_numpy(before))
    st = Y.DeviceConverter(desc).run(both[:ns], _words(yrec, Y.YCC_WORDS), both[ns:], _words(srec, P.SRC_WORDS))
    torch.cuda.synchronize()
    ref, _ = Y.reference(src, yrec, srec, desc, before)
    assert st.cpu().numpy().tolist() == want
    assert np.array_equal(both[ns:].cpu().numpy(), ref) and np.array_equal(both[:ns].cpu().numpy(), src)
    alone, _ = Y.reference(src, yrec[[0, 7]], srec[[0, 7]], desc, before)
    assert np.array_equal(ref, alone) and (ref != before).any()        # the malformed ones changed nothing


@pytest.fixture(scope="module")
def golden():
    return G.load()[0]


@pytest.mark.parametrize("sub", Y.SUBSAMPLINGS)
def test_fixture_planes_give_pillows_rgb(golden, sub):
    """the decoder's planes of every fixture JPEG of one subsampling, one batch: Pillow's own RGB bytes out of the device"""
    import torch
    cases = [c for c in golden if c[2] == sub]
    frames = [G.case_planes(seed, kind, G.SUBS.index(sub), h, w) for seed, kind, _, h, w, _, _ in cases]
    src, ycc, srcs, pixels = Y.pack_ycc(frames, Y.PLANAR, sub, "cuda:0")
    st = Y.DeviceConverter(Y.Desc(sub=sub)).run(src, ycc, pixels, srcs)
    torch.cuda.synchronize()
    assert (st.cpu() == 0).all()
    out = pixels.cpu().numpy()
    for (seed, _, _, h, w, rgb, _), r in zip(cases, Y.pack_ycc_host(frames, Y.PLANAR, sub)[2]):
        got = np.stack([out[int(r["offset"]) + y * int(r["row_pitch"]):][:3 * w] for y in range(h)]).reshape(h, w, 3)
        assert np.array_equal(got, rgb), (seed, h, w)


# TORCHVISION_PIL (Resize(256), CenterCrop(224)) scaled to the 24 x 24 test net: Resize(28), CenterCrop(24)
TINY_HW = 24
TINY_PIL = replace(P.TORCHVISION_PIL, name="torchvision_pil_tiny", out_hw=(TINY_HW, TINY_HW), short_side=28)
TINY_PLAIN = replace(TINY_PIL, name="torchvision_tiny", antialias=False)


@pytest.fixture(scope="module")
def tiny_net():
    t = cfg.tiny_tables(hw=TINY_HW)
    q = synth.synth_q_values(t, 2, spread=2)
    net = NetWork(t)
    net.Init(synth.synth_model(t, q, 2), synth.q_text(q), device="cuda:0")
    return net


def _rgb_records(cases, preset):
    """Pillow's RGB images of fixture cases as tf2_preprocess inputs: (pixels, records), laid out as pack_ycc lays the pixels out"""
    return P.pack_host([c[5] for c in cases], preset, align=4)[:2]


def test_chain_into_the_three_consumers(golden, tiny_net):
    """tf2_ycc_to_rgb -> tf2_preprocess_aa == preprocess.reference_aa on Pillow's RGB of the same JPEGs (so the device path from
    decoder planes equals the reference's Pillow pipeline from the decoded image); the same pixels into tf2_preprocess and, with
    whole-image ROIs, into tf2_roi_crop"""
    import torch
    cases = [c for c in golden if c[2] == (2, 2) and c[3] * c[4] > 1][:8] + [c for c in golden if c[2] == (2, 1)][:4]
    for sub in ((2, 2), (2, 1)):
        part = [c for c in cases if c[2] == sub]
        frames = [G.case_planes(seed, kind, G.SUBS.index(sub), h, w) for seed, kind, _, h, w, _, _ in part]
        src, ycc, srcs, pixels = Y.pack_ycc(frames, Y.PLANAR, sub, "cuda:0", preset=TINY_PIL)
        st = Y.DeviceConverter(Y.Desc(sub=sub)).run(src, ycc, pixels, srcs)
        rgb_pixels, rgb_recs = _rgb_records(part, TINY_PIL)
        assert np.array_equal(Y.records_to_words(rgb_recs, P.SRC_WORDS), srcs.cpu().numpy())
        for preset in (TINY_PIL, TINY_PLAIN):
            pp = P.Preprocessor(tiny_net, preset, "RGB")
            for out in ("q", "f32"):
                got, pst = pp(pixels, srcs, out=out)
                want, wst = pp.reference(rgb_pixels, Y.records_to_words(rgb_recs, P.SRC_WORDS), out=out)
                torch.cuda.synchronize()
                assert (st.cpu() == 0).all() and (pst.cpu().numpy() == wst).all() and (wst == 0).all()
                assert np.array_equal(got.cpu().numpy().view(np.uint8), want.view(np.uint8)), (sub, preset.name, out)
        crop = R.DeviceCropper(tiny_net, TINY_PLAIN, "RGB")
        rois = R.whole_image_rois(rgb_recs)
        got, cst = crop.crop(pixels, srcs, R.rois_to_device(rois, "cuda:0"), out="f32")
        want, wst = crop.reference_crop(rgb_pixels, Y.records_to_words(rgb_recs, P.SRC_WORDS), rois, out="f32")
        torch.cuda.synchronize()
        assert (cst.cpu().numpy() == wst).all() and (wst == 0).all()
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_one_graph_planes_to_labels_and_two_streams(tiny_net):
    """convert + tf2_preprocess_aa + network + classify captured ONCE; planes and both record tables refilled with frames of other
    sizes between replays; outputs and statuses equal the statement each time.  Then two streams with their own buffers, side by
    side."""
    import torch
    net, B, k = tiny_net, 4, 3
    rng = np.random.default_rng(9)
    sub = (2, 2)
    desc = Y.Desc(layout=Y.SEMI_CBCR, sub=sub)
    conv, pp = Y.DeviceConverter(desc), P.Preprocessor(net, TINY_PIL, "RGB")

    def frames_of(n):
        out = []
        for _ in range(n):
            h, w = int(rng.integers(20, 3 * Y.TILE_H)), int(rng.integers(20, Y.TILE_W + 40))
            out.append(Y.subsample_box(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), sub))
        return out
    sets = [frames_of(B) for _ in range(3)]
    hosts = [Y.pack_ycc_host(s, desc.layout, sub, 3, TINY_PIL) for s in sets]
    runner, cls = Runner(None, net), K.DeviceClassifier(net, k)

    def expected(host):
        src, yrec, srec, need = host
        px, st = Y.reference(src, yrec, srec, desc, need)
        xq, pst = pp.reference(px, Y.records_to_words(srec, P.SRC_WORDS), out="q")
        assert (st == 0).all() and (pst == 0).all()
        logits = runner.run_batch(torch.from_numpy(xq).to("cuda:0")).clone()
        torch.cuda.synchronize()
        return xq, K.reference(logits.cpu().numpy(), net.q[net.num_layer], k)
    wants = [expected(h) for h in hosts]
    src = torch.zeros(max(h[0].size for h in hosts), dtype=torch.uint8, device="cuda:0")
    pixels = torch.zeros(max(h[3] for h in hosts), dtype=torch.uint8, device="cuda:0")
    ycc = torch.zeros(B, Y.YCC_WORDS, dtype=torch.int32, device="cuda:0")
    srcs = torch.zeros(B, P.SRC_WORDS, dtype=torch.int32, device="cuda:0")
    status = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    fill = lambda i: Y.pack_ycc(sets[i], desc.layout, sub, "cuda:0", 3, TINY_PIL, src=src, ycc=ycc, srcs=srcs, pixels=pixels)
    fill(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        conv.run(src, ycc, pixels, srcs, status=status)
        cls.run(runner.run_batch(pp(pixels, srcs, out="q")[0]))                    # warm the launch plan of this stream's workspace
        torch.cuda.current_stream().synchronize()
        with torch.cuda.graph(g, stream=side):
            conv.run(src, ycc, pixels, srcs, status=status)
            xq, pst = pp(pixels, srcs, out="q")
            res = cls.run(runner.run_batch(xq))
    torch.cuda.current_stream().wait_stream(side)
    for i in (1, 2, 0, 1):
        fill(i)
        g.replay()
        torch.cuda.synchronize()
        wq, want = wants[i]
        assert (status.cpu() == 0).all() and (pst.cpu() == 0).all()
        assert np.array_equal(xq.cpu().numpy(), wq)
        assert np.array_equal(res.labels.cpu().numpy(), want.labels)
        assert np.array_equal(res.features.cpu().numpy().view(np.uint32), want.features.view(np.uint32))
    # two streams, their own buffers, runners and classifiers, side by side
    ins = [Y.pack_ycc(sets[i], desc.layout, sub, "cuda:0", 3, TINY_PIL) for i in range(2)]
    runner2, cls2 = Runner(None, net), K.DeviceClassifier(net, k)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream()); s2.wait_stream(torch.cuda.current_stream())
    outs = []
    for _ in range(3):
        pair = []
        for (sr, yc, sc, px), s, rn, c in ((ins[0], s1, runner, cls), (ins[1], s2, runner2, cls2)):
            with torch.cuda.stream(s):
                st = conv.run(sr, yc, px, sc, stream=s)
                x, _ = pp(px, sc, out="q", stream=s)
                pair.append((st, x.clone(), c.run(rn.run_batch(x), stream=s)))
        outs.append(pair)
    torch.cuda.synchronize()
    for pair in outs:
        for (st, x, r), (wq, want) in zip(pair, wants[:2]):
            assert (st.cpu() == 0).all() and np.array_equal(x.cpu().numpy(), wq)
            assert np.array_equal(r.labels.cpu().numpy(), want.labels)
