"""Parallel JPEG entropy decoding, on the CPU: jpeg.reference_huff -- the statement of tf2_jpeg_huff (csrc/jpeg_huff.hip), which runs
the parallel algorithm itself: subsequences, tolerant rounds, prefix sums, strict pass -- against the host decoder jpeg.entropy on the
fixture's files (restart intervals 1 and 3 included), on a larger 4:2:0 file at three subsequence sizes, on files cut at every byte
of the scan and with seeded bit flips (nonzero status exactly when the host's is, coefficients zero then); why the rounds are
tolerant (without the rule they degenerate to one round a subsequence); and the host fill call tf2_jpeg_scan_fill against an
independent parse of the DHT segments."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

from tf2_amd import _lib, jpeg as J, ycc as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_jpeg_golden as G  # noqa: E402
import jpeg_time as T  # noqa: E402


@pytest.fixture(scope="module")
def files():
    """[(case, file bytes, Info, host coefficients)] of the fixture's decodable files"""
    out = []
    for c in G.load()[0]:
        if G.supported(c):
            info = J.parse(c["file"])
            coef, st = J.entropy(c["file"], info)
            assert st == 0
            out.append((c, c["file"], info, coef))
    assert len(out) == 56
    return out


def huff(data, info, subseq, tolerant=True):
    """reference_huff of one file: (coef [total_blocks, 64], status, rounds, subsequences)"""
    layout, sub, _ = J.group_key(info)
    hb, scan, jrec, _, _, _, nb, _, _ = J.pack_bytes_host([(data, info)], layout, sub)
    coef, st, rounds = J.reference_huff(hb, scan, jrec, J.HuffDesc(layout, sub, subseq), nb, tolerant=tolerant)
    return coef, int(st[0]), int(rounds[0]), max(1, -(-int(scan[0]["byte_len"]) // subseq))


def synth_file(h, w, fine=False):
    """one 4:2:0 file of tools/jpeg_time.py's synth_frame content: Pillow's encoding (quality 90; fine: 95) where Pillow is
    importable, the tool's own encoder otherwise (its quantiser; fine: half of it)"""
    frame = T.synth_frame(np.random.default_rng(5), h, w)
    try:
        from PIL import Image
    except ImportError:
        keep = T.QUANT
        try:
            T.QUANT = np.maximum(1, keep // 2) if fine else keep
            return T.encode(frame, (2, 2), J.ZIGZAG)
        finally:
            T.QUANT = keep
    out = io.BytesIO()
    Image.fromarray(frame, "YCbCr").convert("RGB").save(out, "JPEG", quality=95 if fine else 90, subsampling=2)
    return out.getvalue()


@pytest.mark.parametrize("subseq", [16, 128])
def test_reference_equals_the_host_decoder_on_the_fixture(files, subseq):
    restarts = set()
    for c, data, info, want in files:
        got, st, rounds, n = huff(data, info, subseq)
        assert st == 0 and np.array_equal(got, want), (c["seed"], c["mode"], c["h"], c["w"], subseq, st)
        assert 1 <= rounds <= n + (n - 1) // J.huff_chunk_lanes(subseq)
        restarts.add(info.restart_interval)
    assert restarts == {0, 1, 3}


def test_without_the_tolerant_rule_the_rounds_degenerate():
    """a 96 x 128 4:2:0 file at 16 bytes a subsequence: a lane that stops at the first impossible event never meets the right
    chain, so little more than the induction's one subsequence a round is left"""
    data = synth_file(96, 128)
    info = J.parse(data)
    want, _ = J.entropy(data, info)
    got, st, tolerant, n = huff(data, info, 16)
    got2, st2, strict, n2 = huff(data, info, 16, tolerant=False)
    assert n == n2 and 16 < n <= J.huff_chunk_lanes(16)
    assert st == 0 and st2 == 0 and np.array_equal(got, want) and np.array_equal(got2, want)    # (both are exact: rounds alone differ)
    print(f"subsequences {n}, rounds: tolerant {tolerant}, without the rule {strict}")
    assert tolerant < strict <= n
    assert strict > n // 2 and tolerant < n // 2


def independent_tables(data):
    """{(class, id): (counts [16], symbols)} of a file's DHT segments and the scan's (dc id, ac id) per component"""
    d, pos, tabs = bytes(data), 2, {}
    while True:
        assert d[pos] == 0xFF
        m, ln = d[pos + 1], (d[pos + 2] << 8) | d[pos + 3]
        seg = d[pos + 4:pos + 2 + ln]
        pos += 2 + ln
        if m == 0xC4:
            at = 0
            while at < len(seg):
                n = sum(seg[at + 1:at + 17])
                tabs[(seg[at] >> 4, seg[at] & 15)] = (list(seg[at + 1:at + 17]), list(seg[at + 17:at + 17 + n]))
                at += 17 + n
        elif m == 0xDA:
            return tabs, [(seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(seg[0])], pos


def test_scan_record_holds_the_files_own_tables(files):
    for c, data, info, _ in files:
        rec = J.scan_record(data, info, 1234)
        tabs, ids, scan_at = independent_tables(data)
        assert scan_at == info.scan_offset
        assert (int(rec["byte_off"]), int(rec["byte_len"])) == (1234, len(data) - scan_at)
        assert (int(rec["components"]), int(rec["sub_x"]), int(rec["sub_y"])) == (info.components,) + tuple(info.sub)
        assert int(rec["restart_interval"]) == info.restart_interval == (0 if c["restart"] == 0 else int(rec["restart_interval"]))
        for k, (td, ta) in enumerate(ids):
            for name, (counts, syms) in (("dc", tabs[(0, td)]), ("ac", tabs[(1, ta)])):
                assert rec["tab"][k][name + "_counts"].tolist() == counts
                assert rec["tab"][k][name + "_vals"].tolist() == syms + [0] * (256 - len(syms))
        for k in range(info.components, 3):
            assert not rec["tab"][k]["dc_counts"].any() and not rec["tab"][k]["ac_vals"].any()
    assert C.sizeof(_lib.JpegScan) == J.SCAN_DTYPE.itemsize == 1664 and C.sizeof(_lib.JpegHuffDesc) == 20


def test_scan_fill_refuses_null_arguments_and_foreign_infos(files):
    _, data, info, _ = files[5]
    buf = np.frombuffer(data, np.uint8)
    L, raw = _lib.lib(), _lib.JpegScan()
    assert L.tf2_jpeg_scan_fill(buf.ctypes.data, buf.size, C.byref(info.raw), 0, C.byref(raw)) == 0
    assert L.tf2_jpeg_scan_fill(None, buf.size, C.byref(info.raw), 0, C.byref(raw)) == -1
    assert L.tf2_jpeg_scan_fill(buf.ctypes.data, buf.size, None, 0, C.byref(raw)) == -1
    assert L.tf2_jpeg_scan_fill(buf.ctypes.data, buf.size, C.byref(info.raw), 0, None) == -1
    other = files[20][2]
    assert other.key() != info.key()
    assert L.tf2_jpeg_scan_fill(buf.ctypes.data, buf.size, C.byref(other.raw), 0, C.byref(raw)) == -1     # not this file's info
    bad = J.parse(data[:40])
    assert bad.status != 0
    assert L.tf2_jpeg_scan_fill(buf.ctypes.data, buf.size, C.byref(bad.raw), 0, C.byref(raw)) == -1


def small_files(files):
    """three small files: a 4:2:0 one with a restart interval, a 4:4:4 one, a grey one with a restart interval"""
    pick = []
    for want in (lambda c, i: c["mode"] == 2 and i.restart_interval and len(c["file"]) > 700,
                 lambda c, i: c["mode"] == 0 and not i.restart_interval and 16 * 16 <= c["h"] * c["w"] <= 17 * 33,
                 lambda c, i: c["mode"] == -1 and i.restart_interval and c["h"] * c["w"] >= 15 * 15):
        pick.append(min((f for f in files if want(f[0], f[2])), key=lambda f: len(f[1])))
    return pick


def check_damaged(data, info, subseq):
    """the statement against the host decoder on a damaged file: (host status, statement's status)"""
    want, hst = J.entropy(data, info)
    got, st, _, _ = huff(data, info, subseq)
    assert (st != 0) == (hst != 0), (hst, st)
    if st:
        assert st in (J.TRUNCATED, J.BAD_CODE) and hst in (J.TRUNCATED, J.BAD_CODE) and not got.any()
    else:
        assert np.array_equal(got, want)
    return hst, st


def test_files_cut_at_every_byte_of_the_scan(files):
    seen = set()
    for c, data, info, _ in small_files(files):
        for cut in range(info.scan_offset, len(data)):
            seen.add(check_damaged(data[:cut], info, 16 if cut % 2 else 64))
    assert {s[0] for s in seen} >= {0, J.TRUNCATED}                # (cut inside the EOI marker: the host still decodes)


def test_files_with_seeded_bit_flips(files):
    rng = np.random.default_rng(77)
    seen = set()
    for c, data, info, _ in small_files(files):
        for trial in range(150):
            d = bytearray(data)
            for _ in range(1 + trial % 3):
                at = int(rng.integers(info.scan_offset, len(d)))
                d[at] ^= 1 << int(rng.integers(0, 8))
            seen.add(check_damaged(bytes(d), info, (16, 32, 128)[trial % 3])[0])
    assert seen >= {0, J.TRUNCATED, J.BAD_CODE}


def test_synchronisation_over_many_subsequences():
    """a 96 x 128 4:2:0 file of synth_frame content: a few KB, so more than a hundred subsequences at 16 bytes and a handful at
    256 (past a chunk's lanes: tests/test_gpu_jpeg_huff.py's finer file, against this statement)"""
    data = synth_file(96, 128)
    info = J.parse(data)
    assert info.status == 0 and info.sub == (2, 2) and (info.h, info.w) == (96, 128)
    want, hst = J.entropy(data, info)
    assert hst == 0
    for subseq in (16, 64, 256):
        got, st, rounds, n = huff(data, info, subseq)
        print(f"subseq_bytes {subseq}: {n} subsequences, {rounds} rounds")
        assert st == 0 and np.array_equal(got, want)
        assert rounds < n or n <= 2


def test_host_checks_refuse_before_any_device_call():
    """every refusal is TF2_ERR_ARG with a "tf2_jpeg_huff:" message; the pointers are never followed (they point nowhere)"""
    L = _lib.lib()
    desc = J.HuffDesc(Y.PLANAR, (2, 2), 64)
    B, need = 2, J.huff_work_bytes(desc, 2, 0)
    assert need == 2 * (16 + 8) == L.tf2_jpeg_huff_work_bytes(C.byref(desc.c()), B, 0)
    assert L.tf2_jpeg_huff_work_bytes(C.byref(desc.c()), B, 1000) == J.huff_work_bytes(desc, B, 1000) == 2 * (16 + 8 * 16)
    assert L.tf2_jpeg_huff_work_bytes(C.byref(J.HuffDesc(Y.PLANAR, (2, 2), 48).c()), B, 1000) == 0
    good = dict(d=desc, data=0x10000, n=4096, scan=0x20000, jpeg=0x30000, coef=0x40000, blocks=16, work=0x50000, wb=need, batch=B,
                status=0x60000)

    def call(**kw):
        a = dict(good, **kw)
        d = a["d"] if isinstance(a["d"], (_lib.JpegHuffDesc, type(None))) else a["d"].c()
        rc = L.tf2_jpeg_huff(None if d is None else C.byref(d), a["data"], a["n"], a["scan"], a["jpeg"], a["coef"], a["blocks"], a["work"],
                             a["wb"], a["batch"], a["status"], None)
        return rc, L.tf2_last_error().decode()
    small = desc.c()
    small.size -= 4
    for kw, text in [(dict(d=None), "null desc"), (dict(d=small), "desc size"), (dict(d=J.HuffDesc(7, (2, 2))), "layout"),
                     (dict(d=J.HuffDesc(Y.PLANAR, (1, 2))), "sub_x, sub_y"), (dict(d=J.HuffDesc(Y.PLANAR, (2, 2), 48)), "subseq_bytes"),
                     (dict(d=J.HuffDesc(Y.PLANAR, (2, 2), 512)), "subseq_bytes"), (dict(batch=0), "batch"), (dict(data=0), "null"),
                     (dict(scan=0), "null"), (dict(jpeg=0), "null"), (dict(coef=0), "null"), (dict(work=0), "null"),
                     (dict(status=0), "null"), (dict(coef=0x40008), "16-byte"), (dict(work=0x50004), "8-byte"),
                     (dict(blocks=1 << 62), "wraps"), (dict(wb=need - 1), "work_bytes"),
                     (dict(data=0x40000 - 100), "byte and the coefficient"), (dict(work=0x40000 + 16 * 128 - 8), "coefficient and the workspace"),
                     (dict(status=0x50000 + need - 4), "workspace and the status"), (dict(status=0x10000 + 4092), "byte and the status")]:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("tf2_jpeg_huff: ") and text in msg, (kw, rc, msg)
