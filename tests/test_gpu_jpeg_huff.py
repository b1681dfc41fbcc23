"""JPEG entropy decoding on the MI355X (tf2_jpeg_huff, jpeg_huff.hip): the whole coefficient buffer, the statuses and the rounds used,
bit-identical to the statement jpeg.reference_huff and, for files the host decodes, to jpeg.entropy -- mixed batches of the fixture's
files per layout and subsampling (restart intervals included) at 16 bytes a subsequence and at the default, with guard words behind
every buffer the call writes; a file of more subsequences than a workgroup has lanes (the carry between chunks); truncated and
bit-flipped scans beside a good one, a byte range cut inside a stuffed pair and inside a restart marker; malformed records; Pillow's
own RGB of the fixture's files through tf2_jpeg_huff -> tf2_jpeg_idct -> tf2_ycc_to_rgb; and the three calls in one captured graph
replayed on refilled bytes of other files and sizes."""
import os
import sys

import numpy as np
import pytest

from tf2_amd import jpeg as J, preprocess as P, ycc as Y
from tests.test_jpeg_huff import synth_file

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_jpeg_golden as G  # noqa: E402

GROUPS = [(Y.GRAY, (1, 1)), (Y.PLANAR, (1, 1)), (Y.PLANAR, (2, 1)), (Y.PLANAR, (2, 2))]
GUARD = 0x5A5A


@pytest.fixture(scope="module")
def parsed():
    """[(case, file, Info, host coefficients)] of the supported fixture files"""
    out = []
    for c in G.load()[0]:
        if G.supported(c):
            info = J.parse(c["file"])
            coef, st = J.entropy(c["file"], info)
            assert st == 0
            out.append((c, c["file"], info, coef))
    return out


def group_of(parsed, layout, sub):
    return [f for f in parsed if J.group_key(f[2])[:2] == (layout, sub)]


def lay_out(rng, items, layout, sub):
    """(bytes, scan, jrec, coef_blocks) of [(file, Info)] laid out to be awkward: 1..5 guard bytes between the scans (byte offsets
    of every residue), 0..2 guard blocks between the components' coefficient runs"""
    parts, at, nb = [], 0, 0
    scan, jrec = np.zeros(len(items), J.SCAN_DTYPE), np.zeros(len(items), J.JPEG_DTYPE)
    for i, (data, info) in enumerate(items):
        gap = int(rng.integers(1, 6))
        parts += [np.full(gap, 0xA5, np.uint8), np.frombuffer(data, np.uint8)[info.scan_offset:]]
        scan[i] = J.scan_record(data, info, at + gap)
        at += gap + parts[-1].size
        for c in range(info.components):
            nb += int(rng.integers(0, 3))
            jrec[i]["block_off"][c], jrec[i]["bw"][c], jrec[i]["bh"][c] = nb, info.bw[c], info.bh[c]
            nb += info.bw[c] * info.bh[c]
    return np.concatenate(parts + [np.full(3, 0xA5, np.uint8)]), scan, jrec, nb + 1


def run_and_check(desc, hb, scan, jrec, nb, work_bytes=None, want_status=None):
    """the device on host inputs: the whole coefficient buffer (guard blocks between and behind the extents included), the statuses
    and the rounds equal the statement; the guard words behind the workspace and the statuses are intact.  Returns (coef, status)."""
    import torch
    B = len(scan)
    if work_bytes is None:
        work_bytes = J.huff_work_bytes(desc, B, int(scan["byte_len"].max()))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    before = np.full((nb + 2, 64), GUARD, np.int16)
    coef, work, status = dev(before), dev(np.full(work_bytes + 16, 0x5A, np.uint8)), dev(np.full(B + 4, GUARD, np.int32))
    data = dev(hb)
    J.DeviceEntropy(desc).run(data, dev(Y.records_to_words(scan, J.SCAN_WORDS)), dev(Y.records_to_words(jrec, J.JPEG_WORDS)),
                              coef[:nb], work[:work_bytes], status=status[:B])
    torch.cuda.synchronize()
    want, wst, wrounds = J.reference_huff(hb, scan, jrec, desc, nb, before[:nb], work_bytes)
    got, gst, gwork = coef.cpu().numpy(), status.cpu().numpy(), work.cpu().numpy()
    assert np.array_equal(gst[:B], wst), (gst[:B], wst)
    if want_status is not None:
        assert gst[:B].tolist() == list(want_status), gst[:B]
    bad = np.flatnonzero((got[:nb] != want).any(axis=1))
    assert bad.size == 0, (desc, len(bad), bad[:8])
    assert (got[nb:] == GUARD).all() and (gst[B:] == GUARD).all() and (gwork[work_bytes:] == 0x5A).all()
    slice_ = (work_bytes // B) & ~7
    for b in range(B):
        head = gwork[b * slice_: b * slice_ + 16].view(np.int32)
        if wst[b] & ~(J.TRUNCATED | J.BAD_CODE):                    # an image with a record bit: its slice is untouched
            assert (gwork[b * slice_:(b + 1) * slice_] == 0x5A).all()
        elif wst[b] == 0:
            assert head[0] == wrounds[b] and head[1] == max(1, -(-int(scan[b]["byte_len"]) // desc.subseq)), (b, head, wrounds[b])
    return got[:nb], gst[:B]


def host_extent(coef, j, info):
    return np.concatenate([coef[int(j["block_off"][c]):][:info.bw[c] * info.bh[c]] for c in range(info.components)])


@pytest.mark.parametrize("layout,sub", GROUPS)
def test_mixed_batches_bit_identical(layout, sub, parsed):
    """seven files of the group from 1 x 1 to 50 x 75, the restart-interval files among them, at 16 bytes a subsequence (up to a few
    hundred subsequences; past a chunk's lanes: test_more_subsequences_than_lanes) and at the default"""
    rng = np.random.default_rng(500 + GROUPS.index((layout, sub)))
    members = sorted(group_of(parsed, layout, sub), key=lambda f: f[0]["h"] * f[0]["w"])
    with_rst = [f for f in members if f[2].restart_interval]
    pick = [members[0], members[-1]] + with_rst[:3]
    pick += [f for f in members[1:-1] if f not in pick][:7 - len(pick)]
    assert 5 <= len(pick) <= 7 and (pick[0][0]["h"], pick[0][0]["w"]) == (1, 1) and (pick[1][0]["h"], pick[1][0]["w"]) == (50, 75)
    assert {f[2].restart_interval for f in pick} >= {0, 1, 3}
    for subseq in (16, 0):
        hb, scan, jrec, nb = lay_out(rng, [(f[1], f[2]) for f in pick], layout, sub)
        got, _ = run_and_check(J.HuffDesc(layout, sub, subseq), hb, scan, jrec, nb, want_status=[0] * len(pick))
        for (c, data, info, hcoef), j in zip(pick, jrec):
            assert np.array_equal(host_extent(got, j, info), hcoef), (c["h"], c["w"], subseq)


def test_more_subsequences_than_lanes():
    """one 96 x 128 4:2:0 file at 16 bytes a subsequence: the second chunk starts from the first one's converged exit"""
    data = synth_file(96, 128, fine=True)
    info = J.parse(data)
    assert info.status == 0 and (info.h, info.w, info.sub) == (96, 128, (2, 2))
    hb, scan, jrec, nb = lay_out(np.random.default_rng(3), [(data, info)], Y.PLANAR, (2, 2))
    assert -(-int(scan[0]["byte_len"]) // 16) > J.huff_chunk_lanes(16) == 256
    got, _ = run_and_check(J.HuffDesc(Y.PLANAR, (2, 2), 16), hb, scan, jrec, nb, want_status=[0])
    want, hst = J.entropy(data, info)
    assert hst == 0 and np.array_equal(host_extent(got, jrec[0], info), want)


def test_hostile_scans(parsed):
    """a good file between a truncated and a bit-flipped one; byte ranges that end inside a stuffed pair and inside a restart marker"""
    rng = np.random.default_rng(9)
    members = group_of(parsed, Y.PLANAR, (2, 2))
    good = max(members, key=lambda f: len(f[1]))
    stuffed = next(f for f in members if b"\xff\x00" in f[1][f[2].scan_offset:])
    rst = max((f for f in members if f[2].restart_interval), key=lambda f: len(f[1]))
    cut = good[1][:good[2].scan_offset + (len(good[1]) - good[2].scan_offset) // 2]
    flipped = bytearray(good[1])
    flipped[good[2].scan_offset + 40] ^= 0x10
    flipped[good[2].scan_offset + 41] = 0xFF
    flipped = bytes(flipped)
    items = [(cut, good[2]), (good[1], good[2]), (flipped, good[2]), (stuffed[1], stuffed[2]), (rst[1], rst[2])]
    hb, scan, jrec, nb = lay_out(rng, items, Y.PLANAR, (2, 2))
    at = stuffed[1].index(b"\xff\x00", stuffed[2].scan_offset) - stuffed[2].scan_offset
    scan[3]["byte_len"] = at + 1                                   # ... FF | 00
    at = rst[1].index(b"\xff\xd0", rst[2].scan_offset) - rst[2].scan_offset
    scan[4]["byte_len"] = at + 1                                   # ... FF | D0
    for subseq in (16, 0):
        got, st = run_and_check(J.HuffDesc(Y.PLANAR, (2, 2), subseq), hb, scan, jrec, nb)
        assert st[1] == 0 and np.array_equal(host_extent(got, jrec[1], good[2]), good[3])
        for i, (data, info) in enumerate(items):
            if i == 1:
                continue
            n = int(scan[i]["byte_len"])
            _, hst = J.entropy(data[:info.scan_offset + n], info)
            assert hst in (J.TRUNCATED, J.BAD_CODE) and st[i] in (J.TRUNCATED, J.BAD_CODE), (i, hst, st[i])
            assert not host_extent(got, jrec[i], info).any()


@pytest.mark.parametrize("layout,sub", [(Y.PLANAR, (2, 2)), (Y.GRAY, (1, 1))])
def test_malformed_records(layout, sub, parsed):
    """one image per new status bit between valid ones: each sets its bit alone and nothing of it is read or written"""
    rng = np.random.default_rng(31)
    members = sorted(group_of(parsed, layout, sub), key=lambda f: len(f[1]))
    pick = [members[3], members[4], members[5], members[-1], members[6], members[7]]     # the longest scan is image 3
    hb, scan, jrec, nb = lay_out(rng, [(f[1], f[2]) for f in pick], layout, sub)
    desc = J.HuffDesc(layout, sub, 16)
    scan[1]["byte_off"] = len(hb) - int(scan[1]["byte_len"]) + 1                           # BAD_RANGE by one byte
    scan[2]["tab"][0]["dc_counts"][0] = 3                                                  # BAD_TABLE: three codes of one bit
    others = max(int(s["byte_len"]) for i, s in enumerate(scan) if i != 3)
    assert int(scan[3]["byte_len"]) > others + 16
    work_bytes = J.huff_work_bytes(desc, len(pick), others)                                # WORK_TOO_SMALL for image 3 alone
    scan[4]["components"] = 4 - desc.components                                            # BAD_SCAN: not the desc's
    want = [0, J.REC_BAD_RANGE, J.REC_BAD_TABLE, J.REC_WORK_TOO_SMALL, J.REC_BAD_SCAN, 0]
    got, st = run_and_check(desc, hb, scan, jrec, nb, work_bytes, want)
    alone, _, _ = J.reference_huff(hb, scan[[0, 5]], jrec[[0, 5]], desc, nb, np.full((nb, 64), GUARD, np.int16))
    assert np.array_equal(got, alone)                                                      # the malformed ones changed nothing
    for i in (0, 5):
        assert np.array_equal(host_extent(got, jrec[i], pick[i][2]), pick[i][3])
    jrec[0]["bh"][0] = 0                                                                   # the tf2_jpeg_src record's own bits
    jrec[5]["block_off"][0] = -1
    jrec[3]["block_off"][desc.components - 1] = nb - 1
    run_and_check(desc, hb, scan, jrec, nb, None,
                  [J.REC_BAD_GRID, J.REC_BAD_RANGE, J.REC_BAD_TABLE, J.REC_OUT_OF_COEF, J.REC_BAD_SCAN, J.REC_BAD_OFFSET])


def test_fixture_files_give_pillows_rgb_from_their_bytes(parsed):
    """fixture files -> tf2_jpeg_huff -> tf2_jpeg_idct -> tf2_ycc_to_rgb, one batch per group_key: Pillow's own RGB bytes out of
    the device, the host having parsed headers only"""
    import torch
    groups = {}
    for f in parsed:
        groups.setdefault(J.group_key(f[2]), []).append(f)
    assert len(groups) == 6 and {k[2] for k in groups} == {Y.FANCY, Y.REPLICATE}
    for (layout, sub, upsample), members in groups.items():
        items = [(f[1], f[2]) for f in members]
        data, scan, coef, jpeg, quant, planes, ycc, srcs, pixels, work = J.pack_bytes(items, layout, sub, "cuda:0")
        st0 = J.DeviceEntropy(J.HuffDesc(layout, sub)).run(data, scan, jpeg, coef, work)
        st1 = J.DeviceDecoder(J.Desc(layout, sub)).run(coef, jpeg, quant, planes, ycc, srcs)
        st2 = Y.DeviceConverter(Y.Desc(layout=layout, sub=sub, upsample=upsample)).run(planes, ycc, pixels, srcs)
        torch.cuda.synchronize()
        assert (st0.cpu() == 0).all() and (st1.cpu() == 0).all() and (st2.cpu() == 0).all()
        out = pixels.cpu().numpy()
        for (c, _, _, _), r in zip(members, J.pack_bytes_host(items, layout, sub)[5]):
            h, w = c["h"], c["w"]
            got = np.stack([out[int(r["offset"]) + y * int(r["row_pitch"]):][:3 * w] for y in range(h)]).reshape(h, w, 3)
            assert np.array_equal(got, c["rgb"]), (c["seed"], c["mode"], h, w)


def test_one_graph_bytes_to_pixels(parsed):
    """tf2_jpeg_huff + tf2_jpeg_idct + tf2_ycc_to_rgb captured ONCE; the bytes and every record table refilled with other files of
    other sizes between replays: Pillow's RGB each time"""
    import torch
    layout, sub, B, dev = Y.PLANAR, (2, 2), 3, "cuda:0"
    members = [f for f in group_of(parsed, layout, sub) if J.group_key(f[2])[2] == Y.FANCY]
    assert len(members) == 10
    sets = [members[0:3], members[3:6], members[6:9], [members[9], members[0], members[7]]]
    hosts = [J.pack_bytes_host([(f[1], f[2]) for f in s], layout, sub) for s in sets]
    hdesc = J.HuffDesc(layout, sub)
    data = torch.zeros(max(h[0].size for h in hosts), dtype=torch.uint8, device=dev)
    coef = torch.zeros(max(h[6] for h in hosts), 64, dtype=torch.int16, device=dev)
    planes = torch.zeros(max(h[7] for h in hosts), dtype=torch.uint8, device=dev)
    pixels = torch.zeros(max(h[8] for h in hosts), dtype=torch.uint8, device=dev)
    work = torch.zeros(J.huff_work_bytes(hdesc, B, max(int(h[1]["byte_len"].max()) for h in hosts)), dtype=torch.uint8, device=dev)
    scan = torch.zeros(B, J.SCAN_WORDS, dtype=torch.int32, device=dev)
    jpeg = torch.zeros(B, J.JPEG_WORDS, dtype=torch.int32, device=dev)
    quant = torch.zeros(B, 3, 64, dtype=torch.int16, device=dev)
    ycc = torch.zeros(B, Y.YCC_WORDS, dtype=torch.int32, device=dev)
    srcs = torch.zeros(B, P.SRC_WORDS, dtype=torch.int32, device=dev)
    sts = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3)]
    ent, dec, conv = J.DeviceEntropy(hdesc), J.DeviceDecoder(J.Desc(layout, sub)), Y.DeviceConverter(Y.Desc(layout=layout, sub=sub))

    def fill(i):
        coef.fill_(GUARD)
        pixels.zero_()
        J.pack_bytes([(f[1], f[2]) for f in sets[i]], layout, sub, dev, data=data, scan=scan, coef=coef, jpeg=jpeg, quant=quant,
                     planes=planes, ycc=ycc, srcs=srcs, pixels=pixels, work=work)

    def calls():
        ent.run(data, scan, jpeg, coef, work, status=sts[0])
        dec.run(coef, jpeg, quant, planes, ycc, srcs, status=sts[1])
        conv.run(planes, ycc, pixels, srcs, status=sts[2])
    fill(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        calls()
        torch.cuda.current_stream().synchronize()
        with torch.cuda.graph(g, stream=side):
            calls()
    torch.cuda.current_stream().wait_stream(side)
    for i in (1, 2, 3, 0, 2):
        fill(i)
        g.replay()
        torch.cuda.synchronize()
        assert all((s.cpu() == 0).all() for s in sts)
        out = pixels.cpu().numpy()
        for f, r in zip(sets[i], hosts[i][5]):
            h, w = f[0]["h"], f[0]["w"]
            got = np.stack([out[int(r["offset"]) + y * int(r["row_pitch"]):][:3 * w] for y in range(h)]).reshape(h, w, 3)
            assert np.array_equal(got, f[0]["rgb"]), (i, h, w)
