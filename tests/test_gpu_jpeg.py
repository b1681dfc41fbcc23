"""JPEG reconstruction on the MI355X (tf2_jpeg_idct, jpeg_idct.hip): the whole plane buffer after the call, and the statuses,
bit-identical to the statement jpeg.reference -- mixed batches of the smallest sizes that can go wrong (1 x 1, one block, one chroma
column, one chroma row, odd sizes, one below, at and one above the kernel's tile of blocks for the Y plane and for a subsampled
chroma plane) per layout and subsampling, the fixture's own coefficients where the size exists, plane offsets of every residue mod 4,
padded pitches (the dword and the byte paths in one batch), guard bytes, blocks_per_image 1, 3 and the default; the wrap regime;
all-zero and DC-only blocks; malformed records; Pillow's own RGB of the fixture's files through decode_host -> tf2_jpeg_idct ->
tf2_ycc_to_rgb; and idct + convert + tf2_preprocess_aa + network + classify in one captured graph replayed on refilled
coefficients."""
import os
import sys
from dataclasses import replace

import numpy as np
import pytest

from tf2_amd import classify as K, config as cfg, jpeg as J, preprocess as P, synth, ycc as Y
from tf2_amd.network import NetWork, Runner

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_jpeg_golden as G  # noqa: E402

TH, TW = 8 * J.TILE_BH, 8 * J.TILE_BW            # the kernel's tile in samples of a plane
SIZES = [(1, 1), (8, 8), (2, 9), (9, 2), (15, 15), (16, 16), (17, 17), (17, 33), (37, 53),
         (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1),                     # the Y plane around one tile, both directions together
         (TH + 1, TW - 1), (TH - 1, TW + 1),                               # and each direction alone: a tail in x only, in y only
         (2 * TH - 1, 2 * TW - 1), (2 * TH, 2 * TW), (2 * TH + 1, 2 * TW + 1),   # a 4:2:0 / 4:2:2 chroma plane around one tile
         (2 * TH + 1, 2 * TW - 1), (2 * TH - 1, 2 * TW + 1)]
GROUPS = [(Y.GRAY, (1, 1)), (Y.PLANAR, (1, 1)), (Y.PLANAR, (2, 1)), (Y.PLANAR, (2, 2))]


@pytest.fixture(scope="module")
def golden():
    return G.load()[0]


@pytest.fixture(scope="module")
def decoded(golden):
    """{(layout, sub, h, w): (Info, coef)} of the supported fixture files, decoded by the host library"""
    out = {}
    for c, (info, coef, st) in zip(golden, J.decode_host([c["file"] for c in golden])):
        if G.supported(c):
            assert st == 0
            out[J.group_key(info)[:2] + (c["h"], c["w"])] = (info, coef)
    return out


def items_of(rng, sizes, layout, sub, decoded):
    """(Info, coef) per size: the fixture's file of that size and group where there is one, else seeded random coefficients within
    +-1024 with quantisers 1..255"""
    out = []
    for h, w in sizes:
        hit = decoded.get((layout, tuple(sub) if layout != Y.GRAY else (1, 1), h, w)) if decoded else None
        if hit is None:
            info = J.make_info(h, w, layout, sub, rng.integers(1, 256, (3, 64)))
            hit = (info, rng.integers(-1024, 1025, (info.total_blocks, 64)).astype(np.int16))
        out.append(hit)
    return out


def mixed(rng, items, layout, sub, rot=0):
    """The device inputs of `items` laid out to be awkward: image i's plane offsets are (i + rot) mod 4 modulo 4; where that is 0
    the pitches are multiples of 4 (the dword path), elsewhere any pitch from the row's bytes up.  Gaps of guard bytes lie before
    every plane and behind every row, gaps of blocks between the components' coefficient runs."""
    sub = (1, 1) if layout == Y.GRAY else tuple(sub)
    n = len(items)
    jrec, yrec, srec = np.zeros(n, J.JPEG_DTYPE), np.zeros(n, Y.YCC_DTYPE), np.zeros(n, P.SRC_DTYPE)
    quant = np.zeros((n, 3, 64), np.uint16)
    blocks, at, nb = [], 0, 0
    for i, (info, coef) in enumerate(items):
        slot = (i + rot) % 4
        offs, pitches, taken = [0, 0, 0], [0, 0, 0], 0
        for c in range(info.components):
            ph, pw = info.ph[c], info.pw[c]
            pitch = pitches[1] if c == 2 else pw + int(rng.integers(0, 9))
            if slot == 0 and c != 2:
                pitch = -(-pitch // 4) * 4 + 4 * int(rng.integers(0, 2))
            off = -(-(at + int(rng.integers(1, 20))) // 4) * 4 + slot
            offs[c], pitches[c], at = off, pitch, off + (ph - 1) * pitch + pw
            gap, nc_blocks = int(rng.integers(0, 3)), info.bw[c] * info.bh[c]
            blocks += [np.full((gap, 64), 0x5A5A, np.int16), np.asarray(coef, np.int16).reshape(-1, 64)[taken:taken + nc_blocks]]
            jrec[i]["block_off"][c], jrec[i]["bw"][c], jrec[i]["bh"][c] = nb + gap, info.bw[c], info.bh[c]
            nb, taken = nb + gap + nc_blocks, taken + nc_blocks
        yrec[i] = (offs[0], offs[1], offs[2], pitches[0], pitches[1])
        srec[i] = (0, info.h, info.w, 3 * info.w, info.h, info.w, 0, 0, 0)
        quant[i] = info.quant
    return np.concatenate(blocks), jrec, quant, yrec, srec, at + int(rng.integers(0, 9))


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr)).to("cuda:0")


def run_and_check(desc, coef, jrec, quant, yrec, srec, before, want_status=None):
    """the device on host inputs: the whole plane buffer and the statuses equal the statement; returns (planes, status)"""
    import torch
    planes = _dev(before)
    st = J.DeviceDecoder(desc).run(_dev(coef), _dev(Y.records_to_words(jrec, J.JPEG_WORDS)), _dev(quant.view(np.int16)), planes,
                                   _dev(Y.records_to_words(yrec, Y.YCC_WORDS)), _dev(Y.records_to_words(srec, P.SRC_WORDS)))
    torch.cuda.synchronize()
    want, wst = J.reference(coef, jrec, quant, yrec, srec, desc, before)
    got, gst = planes.cpu().numpy(), st.cpu().numpy()
    assert np.array_equal(gst, wst), (gst, wst)
    if want_status is not None:
        assert gst.tolist() == list(want_status), gst
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (desc, len(bad), bad[:8], got[bad[:8]], want[bad[:8]])
    return got, gst


@pytest.mark.parametrize("layout,sub", GROUPS)
def test_mixed_batches_bit_identical(layout, sub, decoded):
    """every size of SIZES in one batch, four times: the rotation moves every image over all four residues (and so over the dword
    and the byte path), the grid is one block, three blocks and the default an image.  The reference leaves every byte outside the
    planes' ph x pw as it was, so equality of the whole buffer is also the guard-byte check."""
    rng = np.random.default_rng(300 + GROUPS.index((layout, sub)))
    items = items_of(rng, SIZES, layout, sub, decoded)
    assert sum(it[0].raw is not None for it in items) >= 8           # the fixture's files are in the batch
    for rot, bpi in enumerate((1, 3, 0, 0)):
        coef, jrec, quant, yrec, srec, nbytes = mixed(rng, items, layout, sub, rot)
        before = rng.integers(0, 256, nbytes, dtype=np.uint8)
        got, _ = run_and_check(J.Desc(layout, sub, bpi), coef, jrec, quant, yrec, srec, before, [0] * len(items))
        assert (got != before).any()


@pytest.mark.parametrize("layout,sub", [(Y.GRAY, (1, 1)), (Y.PLANAR, (2, 2))])
def test_the_wrap_regime_and_trivial_blocks(layout, sub):
    """full-range int16 coefficients with quantisers up to 65535: every sum wraps, and the device equals reference_idct as bytes;
    in the same batch all-zero blocks, DC-only blocks and DC-only blocks that clamp"""
    rng = np.random.default_rng(41)
    items = []
    for k, (h, w) in enumerate([(17, 33), (TH + 1, TW + 1), (8, 8), (40, 24)]):
        info = J.make_info(h, w, layout, sub, rng.integers(1, 65536, (3, 64)) if k < 3 else np.ones((3, 64)))
        coef = rng.integers(-32768, 32768, (info.total_blocks, 64)).astype(np.int16)
        if k == 3:
            coef[:, 1:] = 0
            coef[::3] = 0
            coef[1::3, 0] = rng.integers(-2000, 2000, coef[1::3].shape[0])
        items.append((info, coef))
    coef, jrec, quant, yrec, srec, nbytes = mixed(rng, items, layout, sub)
    before = rng.integers(0, 256, nbytes, dtype=np.uint8)
    got, _ = run_and_check(J.Desc(layout, sub), coef, jrec, quant, yrec, srec, before, [0] * 4)
    info, c0 = items[0]
    want = J.plane_of(J.reference_idct(c0[:info.bw[0] * info.bh[0]], info.quant[0]), info.bw[0], info.bh[0], info.h, info.w)
    off, pitch = int(yrec[0]["off_y"]), int(yrec[0]["pitch_y"])
    assert np.array_equal(np.stack([got[off + y * pitch:][:info.w] for y in range(info.h)]), want)
    assert 0 < (want == 0).mean() < 1 and (want == 255).any()          # both clamps and values between


@pytest.mark.parametrize("layout,sub", [(Y.PLANAR, (2, 2)), (Y.GRAY, (1, 1))])
def test_malformed_records(layout, sub):
    """one record per status bit and combinations, between valid ones: the statuses of the statement, the malformed images' bytes
    untouched, the valid neighbours exact.  The extent cases end exactly one unit past their buffer."""
    rng = np.random.default_rng(23)
    sizes = [SIZES[i % len(SIZES)] for i in range(2, 12)]
    items = items_of(rng, sizes, layout, sub, None)
    coef, jrec, quant, yrec, srec, nbytes = mixed(rng, items, layout, sub)
    nblocks, nc = len(coef), (1 if layout == Y.GRAY else 3)
    last, lastp = nc - 1, ("off_y" if nc == 1 else "off_cr")
    srec[1]["w"] = 0                                                   # BAD_SIZE
    jrec[2]["bw"][last] = -(-items[2][0].pw[last] // 8) - 1            # BAD_GRID by one block column
    yrec[3]["pitch_y" if nc == 1 else "pitch_c"] = items[3][0].pw[last] - 1    # BAD_PITCH by one byte
    jrec[4]["block_off"][0] = -1                                       # BAD_OFFSET
    i5 = items[5][0]
    jrec[5]["block_off"][last] = nblocks - i5.bw[last] * i5.bh[last] + 1       # OUT_OF_COEF by one block
    i6 = items[6][0]
    pitch6 = int(yrec[6]["pitch_y" if nc == 1 else "pitch_c"])
    yrec[6][lastp] = nbytes - ((i6.ph[last] - 1) * pitch6 + i6.pw[last]) + 1   # OUT_OF_PLANES by one byte
    srec[7]["h"], yrec[7]["pitch_y"], yrec[7]["off_y"], jrec[7]["bh"][0] = 40000, 0, -8, 0     # SIZE | GRID | PITCH | OFFSET
    jrec[8]["block_off"][0], yrec[8]["off_y"] = nblocks, nbytes                                # both extents
    desc = J.Desc(layout, sub)
    want = [0, J.REC_BAD_SIZE, J.REC_BAD_GRID, J.REC_BAD_PITCH, J.REC_BAD_OFFSET, J.REC_OUT_OF_COEF, J.REC_OUT_OF_PLANES,
            J.REC_BAD_SIZE | J.REC_BAD_GRID | J.REC_BAD_PITCH | J.REC_BAD_OFFSET, J.REC_OUT_OF_COEF | J.REC_OUT_OF_PLANES, 0]
    assert J.record_status(jrec, yrec, srec, desc, nblocks, nbytes).tolist() == want
    before = rng.integers(0, 256, nbytes, dtype=np.uint8)
    got, _ = run_and_check(desc, coef, jrec, quant, yrec, srec, before, want)
    alone, _ = J.reference(coef, jrec[[0, 9]], quant[[0, 9]], yrec[[0, 9]], srec[[0, 9]], desc, before)
    assert np.array_equal(got, alone) and (got != before).any()        # the malformed ones changed nothing


def test_fixture_files_give_pillows_rgb_on_the_device(golden):
    """fixture files -> decode_host -> tf2_jpeg_idct -> tf2_ycc_to_rgb, one batch per group_key (REPLICATE for the narrow group):
    Pillow's own RGB bytes out of the device"""
    import torch
    cases = [c for c in golden if G.supported(c)]
    groups = {}
    for c, (info, coef, st) in zip(cases, J.decode_host([c["file"] for c in cases], threads=4)):
        assert st == 0
        groups.setdefault(J.group_key(info), []).append((c, info, coef))
    assert len(groups) == 6 and {k[2] for k in groups} == {Y.FANCY, Y.REPLICATE}
    for (layout, sub, upsample), members in groups.items():
        items = [(info, coef) for _, info, coef in members]
        coef, jpeg, quant, planes, ycc, srcs, pixels = J.pack(items, layout, sub, "cuda:0")
        st = J.DeviceDecoder(J.Desc(layout, sub)).run(coef, jpeg, quant, planes, ycc, srcs)
        st2 = Y.DeviceConverter(Y.Desc(layout=layout, sub=sub, upsample=upsample)).run(planes, ycc, pixels, srcs)
        torch.cuda.synchronize()
        assert (st.cpu() == 0).all() and (st2.cpu() == 0).all()
        out = pixels.cpu().numpy()
        for (c, _, _), r in zip(members, J.pack_host(items, layout, sub)[4]):
            h, w = c["h"], c["w"]
            got = np.stack([out[int(r["offset"]) + y * int(r["row_pitch"]):][:3 * w] for y in range(h)]).reshape(h, w, 3)
            assert np.array_equal(got, c["rgb"]), (c["seed"], c["mode"], h, w)


# TORCHVISION_PIL (Resize(256), CenterCrop(224)) scaled to the 24 x 24 test net: Resize(28), CenterCrop(24) -- as tests/test_gpu_ycc.py
TINY_HW = 24
TINY_PIL = replace(P.TORCHVISION_PIL, name="torchvision_pil_tiny", out_hw=(TINY_HW, TINY_HW), short_side=28)


@pytest.fixture(scope="module")
def tiny_net():
    t = cfg.tiny_tables(hw=TINY_HW)
    q = synth.synth_q_values(t, 2, spread=2)
    net = NetWork(t)
    net.Init(synth.synth_model(t, q, 2), synth.q_text(q), device="cuda:0")
    return net


def test_one_graph_coefficients_to_labels(tiny_net):
    """idct + convert + tf2_preprocess_aa + network + classify captured ONCE; coefficients, quantisers and all three record tables
    refilled with images of other sizes between replays; every intermediate buffer and the labels equal the host statements chained"""
    import torch
    net, B, k = tiny_net, 4, 3
    rng = np.random.default_rng(11)
    layout, sub = Y.PLANAR, (2, 2)
    jdesc, ydesc = J.Desc(layout, sub), Y.Desc(layout=layout, sub=sub)
    dec, conv, pp = J.DeviceDecoder(jdesc), Y.DeviceConverter(ydesc), P.Preprocessor(net, TINY_PIL, "RGB")

    def items_of_set():
        out = []
        for _ in range(B):
            h, w = int(rng.integers(20, 3 * TH)), int(rng.integers(20, TW + 40))
            info = J.make_info(h, w, layout, sub, rng.integers(1, 32, (3, 64)))
            coef = (rng.integers(-1024, 1025, (info.total_blocks, 64)) >> rng.integers(0, 8, (1, 64))).astype(np.int16)
            out.append((info, coef))
        return out
    sets = [items_of_set() for _ in range(3)]
    hosts = [J.pack_host(s, layout, sub, 3, TINY_PIL) for s in sets]
    runner, cls = Runner(None, net), K.DeviceClassifier(net, k)

    def expected(host):
        coef, jrec, quant, yrec, srec, pbytes, need = host
        pl, st = J.reference(coef, jrec, quant, yrec, srec, jdesc, pbytes)
        px, st2 = Y.reference(pl, yrec, srec, ydesc, need)
        xq, pst = pp.reference(px, Y.records_to_words(srec, P.SRC_WORDS), out="q")
        assert (st == 0).all() and (st2 == 0).all() and (pst == 0).all()
        logits = runner.run_batch(torch.from_numpy(xq).to("cuda:0")).clone()
        torch.cuda.synchronize()
        return pl, px, xq, K.reference(logits.cpu().numpy(), net.q[net.num_layer], k)
    wants = [expected(h) for h in hosts]
    dev = "cuda:0"
    coef = torch.zeros(max(len(h[0]) for h in hosts), 64, dtype=torch.int16, device=dev)
    planes = torch.zeros(max(h[5] for h in hosts), dtype=torch.uint8, device=dev)
    pixels = torch.zeros(max(h[6] for h in hosts), dtype=torch.uint8, device=dev)
    jpeg = torch.zeros(B, J.JPEG_WORDS, dtype=torch.int32, device=dev)
    quant = torch.zeros(B, 3, 64, dtype=torch.int16, device=dev)
    ycc = torch.zeros(B, Y.YCC_WORDS, dtype=torch.int32, device=dev)
    srcs = torch.zeros(B, P.SRC_WORDS, dtype=torch.int32, device=dev)
    status, status2 = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)

    def fill(i):
        planes.zero_()
        pixels.zero_()
        J.pack(sets[i], layout, sub, dev, 3, TINY_PIL, coef=coef, jpeg=jpeg, quant=quant, planes=planes, ycc=ycc, srcs=srcs, pixels=pixels)
    fill(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dec.run(coef, jpeg, quant, planes, ycc, srcs, status=status)
        conv.run(planes, ycc, pixels, srcs, status=status2)
        cls.run(runner.run_batch(pp(pixels, srcs, out="q")[0]))                    # warm the launch plan of this stream's workspace
        torch.cuda.current_stream().synchronize()
        with torch.cuda.graph(g, stream=side):
            dec.run(coef, jpeg, quant, planes, ycc, srcs, status=status)
            conv.run(planes, ycc, pixels, srcs, status=status2)
            xq, pst = pp(pixels, srcs, out="q")
            res = cls.run(runner.run_batch(xq))
    torch.cuda.current_stream().wait_stream(side)
    for i in (1, 2, 0, 1):
        fill(i)
        g.replay()
        torch.cuda.synchronize()
        wpl, wpx, wq, want = wants[i]
        assert (status.cpu() == 0).all() and (status2.cpu() == 0).all() and (pst.cpu() == 0).all()
        assert np.array_equal(planes.cpu().numpy()[:wpl.size], wpl)
        assert np.array_equal(pixels.cpu().numpy()[:wpx.size], wpx)
        assert np.array_equal(xq.cpu().numpy(), wq)
        assert np.array_equal(res.labels.cpu().numpy(), want.labels)
        assert np.array_equal(res.features.cpu().numpy().view(np.uint32), want.features.view(np.uint32))
