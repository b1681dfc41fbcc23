"""Second-stage crops on the MI355X (tf2_roi_select / tf2_roi_crop, roi_crop.hip): the ROI table bit-identical to
roi.reference_select at every det layout, batch and max_rois (random rows, all scores equal, no detections, more candidates than
slots and fewer, boxes outside [0, 1], degenerate / NaN / inf boxes, a malformed source record, and tables whose winners all come
from one thread's rows, so that its four-key cache is refilled again and again); the crops bit-identical to
roi.reference_crop in float32 and int8 on a 227 x 227 net (byte stores) and a 224 x 224 net (vector stores) over sources with
offsets, padded rows, 3- and 4-byte pixels and 1 x N images, with ROIs that upscale, downscale, are one pixel wide, leave the image
or cover it, and empty / bad-image / bad-box / bad-source slots between good ones; a misaligned output; the whole-image identity with
tf2_preprocess on the device; the detect -> crop -> embed -> match cascade against the statements applied to the device's own det;
the cascade captured in one graph and replayed on refilled buffers, and two streams side by side."""
import numpy as np
import pytest

from tf2_amd import config as cfg, embed as E, preprocess as P, roi as R, ssd, synth
from tf2_amd.network import NetWork, Runner

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _host_net(tables, seed=1):
    """a net handle with a q table (all tf2_roi_crop reads of it: image size, Q0)"""
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


def _same_table(rois, counts, want_rois, want_counts, where):
    got = rois.cpu().numpy()
    want = np.ascontiguousarray(want_rois).view(np.int32).reshape(-1, R.ROI_WORDS)
    assert np.array_equal(counts.cpu().numpy(), want_counts), (where, counts.cpu().numpy(), want_counts)
    bad = np.argwhere((got != want).any(axis=1))
    assert bad.size == 0, (where, len(bad), R.rois_to_host(got)[bad[0]], want_rois[bad[0]])


def _det_case(kind, rng, B, Cn, K):
    """det [B, Cn, K, 5], counts [B, Cn] and source records of one input family"""
    det = np.zeros((B, Cn, K, 5), np.float32)
    det[..., 0] = rng.uniform(0, 1, (B, Cn, K))
    x1, y1 = rng.uniform(-0.3, 1.0, (B, Cn, K)), rng.uniform(-0.3, 1.0, (B, Cn, K))
    det[..., 1], det[..., 2] = x1, y1
    det[..., 3], det[..., 4] = x1 + rng.uniform(-0.05, 0.6, (B, Cn, K)), y1 + rng.uniform(-0.05, 0.6, (B, Cn, K))   # some x2 < x1
    odd = rng.uniform(0, 1, (B, Cn, K))
    det[..., 1][odd < 0.02] = np.nan
    det[..., 4][(odd >= 0.02) & (odd < 0.04)] = np.inf
    det[..., 3][(odd >= 0.04) & (odd < 0.06)] = det[..., 1][(odd >= 0.04) & (odd < 0.06)]          # zero width
    det[..., 0][(odd >= 0.06) & (odd < 0.08)] = np.nan
    counts = rng.integers(-2, K + 6, (B, Cn)).astype(np.int32)                                      # below 0 and above top_k too
    if kind == "equal":                       # every score the same: the order is (class, rank) alone
        det[..., 0] = 0.5
    elif kind == "none":                      # every count 0
        counts[:] = 0
    elif kind == "few":                       # at most two candidates an image
        counts[:] = 0
        counts[:, Cn - 1] = rng.integers(0, 2, B)
        counts[:, 1] = 1
    srcs = np.zeros(B, P.SRC_DTYPE)
    for b in range(B):
        h, w = int(rng.integers(1, 700)), int(rng.integers(1, 700))
        srcs[b] = (0, h, w, 3 * w, h, w, 0, 0, 0)
    if B > 1:
        srcs[B // 2]["h"] = 0                 # a malformed record: its image gets no ROI
        srcs[B - 1]["w"] = 40000
    return det, counts, srcs


@pytest.mark.parametrize("max_rois", [1, 3, 64])
@pytest.mark.parametrize("B,Cn,K", [(1, 2, 1), (5, 2, 1), (1, 21, 200), (5, 21, 200), (1, 256, 256)])
def test_select_bit_identical(nets, B, Cn, K, max_rois):
    import torch
    rng = np.random.default_rng(B * 100000 + Cn * 300 + K + max_rois)
    more = fewer = 0
    for k, kind in enumerate(("random", "equal", "none", "few")):
        det, counts, srcs = _det_case(kind, rng, B, Cn, K)
        classes = (1,) if Cn == 2 else tuple(sorted(set(int(c) for c in rng.integers(1, Cn, 6)) | {1, Cn - 1}))
        c = R.DeviceCropper(nets[227], P.SQUEEZENET, "RGB", num_classes=Cn, top_k=K, classes=classes, min_score=(0.3, 0.25, 0.0, 0.0)[k],
                            max_rois=max_rois, expand=((1.0, 1.0), (1.25, 1.5), (1.0, 1.0), (0.5, 2.0))[k], square=bool(k & 1),
                            clip=kind != "equal")
        want_rois, want_n = c.reference_select(det, counts, srcs)
        # the candidates of the statement without the slot limit: both "more than the slots" and "fewer" occur over the cases
        all_n = R.reference_select(det, counts, srcs, classes, c.min_score, 64 if Cn * K < 64 else 4096, c.expand, c.square, c.clip)[1]
        more += int((all_n > max_rois).sum())
        fewer += int((all_n < max_rois).sum())
        rois, n = c.select(_dev(det), _dev(counts), _src_words(srcs))
        torch.cuda.synchronize()
        _same_table(rois, n, want_rois, want_n, kind)
        if kind == "none":
            assert (want_n == 0).all() and (want_rois["image"] == -1).all()
        if B > 1:
            assert want_n[B // 2] == 0 and want_n[B - 1] == 0
    assert fewer > 0 and (more > 0 or (Cn == 2 and K <= max_rois))      # (class 1 alone of two: at most K candidates)


def _owners(rois, K):
    """winners per thread of roi_select: row (cls, rank) belongs to thread (cls * K + rank) % 256"""
    taken = rois[rois["image"] >= 0]
    return np.bincount((taken["cls"].astype(np.int64) * K + taken["rank"]) % 256, minlength=256)


@pytest.mark.parametrize("kind", ["equal", "scores", "ten", "eight", "spread"])
def test_select_many_winners_of_one_thread(nets, kind):
    """(256, 256) with counts of 1: every candidate is a row (c, 0), row index c * 256, and so belongs to thread 0 of the block, which
    keeps four keys at a time -- 64 winners make it refill its cache fifteen times.  equal: every score the same (the keys differ in
    the row alone); scores: random scores, a tenth of the boxes unusable; ten / eight: only ten / eight usable boxes (a refill that
    finds two keys, a refill that finds none after a full one); spread: counts of 3, so three threads give a third of the winners each"""
    import torch
    B, Cn, K, M = 2, 256, 256, 64
    rng = np.random.default_rng(len(kind))
    det = np.zeros((B, Cn, K, 5), np.float32)
    det[..., 0] = 0.5 if kind == "equal" else rng.uniform(0.1, 1.0, (B, Cn, K))
    det[..., 1:3], det[..., 3:5] = 0.25, 0.75
    counts = np.full((B, Cn), 3 if kind == "spread" else 1, np.int32)
    if kind == "scores":
        det[..., 3][rng.uniform(0, 1, (B, Cn, K)) < 0.1] = 0.25                # zero width
    elif kind in ("ten", "eight"):
        keep = 10 if kind == "ten" else 8
        det[..., 3] = 0.25
        for b in range(B):
            det[b, rng.choice(np.arange(1, Cn), keep, replace=False), 0, 3] = 0.75
    srcs = np.zeros(B, P.SRC_DTYPE)
    srcs[0], srcs[1] = (0, 375, 500, 1500, 1, 1, 0, 0, 0), (0, 64, 48, 144, 1, 1, 0, 0, 0)
    c = R.DeviceCropper(nets[227], P.SQUEEZENET, "RGB", num_classes=Cn, top_k=K, classes=tuple(range(1, Cn)), min_score=0.05, max_rois=M)
    want_rois, want_n = c.reference_select(det, counts, srcs)
    most = max(_owners(want_rois[b * M:(b + 1) * M], K).max() for b in range(B))
    assert want_n.tolist() == {"ten": [10, 10], "eight": [8, 8]}.get(kind, [M, M])
    assert most == {"ten": 10, "eight": 8, "spread": most}.get(kind, M) and most >= 8      # one thread gives two caches or more
    assert kind != "spread" or most > 16
    rois, n = c.select(_dev(det), _dev(counts), _src_words(srcs))
    torch.cuda.synchronize()
    _same_table(rois, n, want_rois, want_n, kind)


def _sources(rng, pb):
    """a pixel buffer and records: gaps before each image (nonzero offsets), rows padded past w * pb, a large image, small and
    1 x N / N x 1 images, and a last record that points past the buffer"""
    sizes = [(1000, 800), (40, 33), (1, 257), (300, 1), (227, 227), (224, 224)]
    recs = np.zeros(len(sizes) + 1, P.SRC_DTYPE)
    at = int(rng.integers(1, 64))
    for i, (h, w) in enumerate(sizes):
        pitch = w * pb + (i % 3) * int(rng.integers(1, 33))
        recs[i] = (at, h, w, pitch, 0, 0, -7, 0, 0)               # resize_* / crop_* are not read
        at += (h - 1) * pitch + w * pb + int(rng.integers(0, 100))
    recs[len(sizes)] = (at - 100, 50, 50, 50 * pb, 50, 50, 0, 0, 0)   # ends past the buffer
    return rng.integers(0, 256, at, dtype=np.uint8), recs


def _rois_for(recs):
    """(record, expected status) per slot: good ROIs of every kind with empty and malformed slots between them"""
    rows = [
        (0, 100.25, 50.5, 800.0, 950.5, 0),          # 900 x ~700 px of the large image: downscale
        (-1, 0.0, 0.0, 0.0, 0.0, R.EMPTY),
        (1, 10.3, 7.7, 17.3, 12.7, 0),               # 5 x 7 px: upscale
        (7, 0.0, 0.0, 10.0, 10.0, R.BAD_IMAGE),      # the batch has 7 records
        (0, 400.0, 300.0, 401.0, 301.0, 0),          # exactly one pixel
        (1, 5.0, 5.0, 5.5, 30.0, R.BAD_BOX),
        (1, -20.5, -10.25, 20.0, 25.0, 0),           # partly outside (a table of clip = False)
        (6, 0.0, 0.0, 50.0, 50.0, R.BAD_SRC),
        (1, 100.0, 200.0, 140.0, 260.0, 0),          # wholly outside: the corner pixel
        (2, np.nan, 0.0, 100.0, 1.0, R.BAD_BOX),
        (2, 0.0, 0.0, 257.0, 1.0, 0),                # 1 x N whole
        (-5, 0.0, 0.0, 10.0, 10.0, R.BAD_IMAGE),
        (3, -0.5, 10.0, 1.5, 290.0, 0),              # N x 1
        (6, 0.0, 0.0, np.inf, 50.0, R.BAD_SRC | R.BAD_BOX),
        (4, 0.0, 0.0, 227.0, 227.0, 0),              # whole images: identity at 227 / 224
        (5, 0.0, 0.0, 224.0, 224.0, 0),
        (0, 0.0, 0.0, 800.0, 1000.0, 0),
        (-1, 1.0, 2.0, 3.0, 4.0, R.EMPTY),
    ]
    rois = np.zeros(len(rows), R.ROI_DTYPE)
    for k, (image, x0, y0, x1, y1, _) in enumerate(rows):
        rois[k] = (image, 15, k, 0.5, x0, y0, x1, y1)
    return rois, [r[-1] for r in rows]


def _check_crop(c, pixels, srcs, rois, want_status, misalign=False):
    import torch
    S, (oh, ow) = rois.shape[0], c.out_hw
    for out in ("f32", "q"):
        images = None
        if misalign:                          # one element past the allocation's start: no 4- / 16-byte stores
            flat = torch.zeros(S * 3 * oh * ow + 1, dtype=torch.int8 if out == "q" else torch.float32, device=DEV)
            images = flat[1:].view(S, 3, oh, ow)
            assert images.data_ptr() % (4 if out == "q" else 16) != 0
        got, st = c.crop(pixels, srcs, rois, out=out, images=images)
        torch.cuda.synchronize()
        want, wst = c.reference_crop(pixels, srcs, rois, out=out)
        assert wst.tolist() == want_status and st.cpu().numpy().tolist() == want_status
        g = got.cpu().numpy()
        assert g.dtype == want.dtype and g.shape == want.shape
        view = np.uint8 if out == "q" else np.uint32
        bad = np.argwhere(g.view(view) != want.view(view))
        assert bad.size == 0, (out, len(bad), bad[:5], g[tuple(bad[0])], want[tuple(bad[0])])
        assert all((g[s] == 0).all() for s, bits in enumerate(want_status) if bits) and len(np.unique(g)) > 4


@pytest.mark.parametrize("hw,preset,src_order", [(227, P.SQUEEZENET, "RGB"), (227, P.GOOGLENET, "BGRA"), (224, P.RESNET50, "RGBA"),
                                                 (224, P.TORCHVISION, "BGR")])
def test_crop_bit_identical(nets, hw, preset, src_order):
    rng = np.random.default_rng(hw + len(src_order))
    pixels, recs = _sources(rng, len(src_order))
    rois, want_status = _rois_for(recs)
    assert R.roi_status(rois, recs, len(src_order), pixels.size).tolist() == want_status
    c = R.DeviceCropper(nets[hw], preset, src_order)
    assert c.out_hw == (hw, hw)
    _check_crop(c, _dev(pixels), _src_words(recs), R.rois_to_device(rois, DEV), want_status)


def test_crop_into_a_misaligned_output(nets):
    rng = np.random.default_rng(12)
    pixels, recs = _sources(rng, 3)
    rois, want_status = _rois_for(recs)
    c = R.DeviceCropper(nets[224], P.RESNET50, "RGB")
    _check_crop(c, _dev(pixels), _src_words(recs), R.rois_to_device(rois[:6], DEV), want_status[:6], misalign=True)


@pytest.mark.parametrize("hw,preset", [(227, P.GOOGLENET), (224, P.TORCHVISION)])
def test_whole_image_rois_equal_tf2_preprocess(nets, hw, preset):
    """roi_crop on (0, 0, w, h) == tf2_preprocess with resize = (hw, hw) and crop (0, 0), on the device, float32 and int8"""
    import torch
    rng = np.random.default_rng(hw)
    sizes = [(375, 500), (500, 333), (hw, hw), (97, 131), (1, 40), (33, 1), (640, 479)]
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
    pixels, recs, pb = P.pack_host(imgs, preset, align=16)
    recs["resize_h"], recs["resize_w"], recs["crop_y"], recs["crop_x"] = hw, hw, 0, 0
    px, sr = _dev(pixels), _src_words(recs)
    pp, c = P.Preprocessor(nets[hw], preset, "RGB"), R.DeviceCropper(nets[hw], preset, "RGB")
    rois = R.rois_to_device(R.whole_image_rois(recs), DEV)
    for out in ("f32", "q"):
        want, wst = pp(px, sr, out=out)
        got, st = c.crop(px, sr, rois, out=out)
        torch.cuda.synchronize()
        assert (wst.cpu() == 0).all() and (st.cpu() == 0).all()
        assert torch.equal(got.cpu().view(torch.uint8), want.cpu().view(torch.uint8))
        assert len(torch.unique(got.cpu())) > 4


# ---- the cascade: SSD300 (quarter width, synthetic weights) -> select -> crop -> SqueezeNet 1.1 -> match ----------------------------
# min_score was chosen on roi.reference_select applied to the detector's det of _image_sets()[0]: the best scores of its two images
# are 0.7209, 0.6958, 0.6898, 0.6574.. and 0.7363, 0.6477.., so 0.68 takes three rows of image 0 and one of image 1 -- ROIs to crop,
# and fewer of them than slots (the synthetic SSD's softmax is wide: nothing scores above 0.74)
CASCADE_MIN_SCORE, CASCADE_MAX_ROIS, CASCADE_CLASSES = 0.68, 8, tuple(range(1, 21))


class _Cascade:
    def __init__(self, ssd_net, face_net, gallery):
        self.pp = P.Preprocessor(ssd_net, P.SSD300, "RGB")
        self.det = ssd.DeviceDetector(ssd_net, ssd_net.plan, ssd.VOC)
        self.crop = R.DeviceCropper(face_net, P.SQUEEZENET, "RGB", classes=CASCADE_CLASSES, min_score=CASCADE_MIN_SCORE,
                                    max_rois=CASCADE_MAX_ROIS, expand=(1.25, 1.25), square=True)
        self.runner = Runner(None, face_net)
        self.matcher = E.DeviceMatcher(face_net, 3)
        self.gallery = gallery

    def __call__(self, pixels, srcs):
        x, _ = self.pp(pixels, srcs, out="q")
        det, counts = self.det.run(x)
        crops, status, rois, n = self.crop(det, counts, pixels, srcs, out="q")
        outputs = self.runner.run_batch(crops)
        res = self.matcher.match(outputs, self.gallery)
        return dict(det=det, counts=counts, rois=rois, n=n, crops=crops, status=status, outputs=outputs, idx=res.idx, dist=res.dist,
                    ids=res.ids, emb=res.embeddings)


@pytest.fixture(scope="module")
def cascade_nets():
    from tests.test_gpu_ssd_detect import _ssd_net
    _, _, ssd_net = _ssd_net(4)
    t = cfg.squeezenet11_tables()
    q = synth.synth_q_values(t, 21, spread=2)
    face = NetWork(t)
    face.Init(synth.synth_model(t, q, 21), synth.q_text(q), device=DEV)
    rng = np.random.default_rng(31)
    g = rng.normal(0, 1, (10, 128)).astype(np.float32)
    return ssd_net, face, _dev(g / np.linalg.norm(g, axis=1, keepdims=True).astype(np.float32))


def _image_sets():
    rng = np.random.default_rng(8)
    return [[rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in pair]
            for pair in (((375, 500), (300, 300)), ((120, 90), (640, 480)), ((333, 500), (227, 227)))]


def _host(out):
    return {k: v.cpu().clone() for k, v in out.items()}


def _equal(a, b, where):
    import torch
    for k in a:
        assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                           b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), (where, k)


def test_cascade_equals_the_statements(cascade_nets):
    import torch
    ssd_net, face, gallery = cascade_nets
    cas = _Cascade(ssd_net, face, gallery)
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
    ref, _ = cas.matcher.reference(out["outputs"], gallery)
    assert np.array_equal(out["idx"].cpu().numpy(), ref.idx) and np.array_equal(out["ids"].cpu().numpy(), ref.ids)
    assert np.array_equal(out["dist"].cpu().numpy().view(np.uint32), ref.dist.view(np.uint32))
    assert np.array_equal(out["emb"].cpu().numpy().view(np.uint32), ref.embeddings.view(np.uint32))
    assert out["outputs"].shape == (2 * CASCADE_MAX_ROIS, 128)


def test_cascade_graph_replay_with_refilled_buffers_and_two_streams(cascade_nets):
    """capture preprocess -> detect -> select -> crop -> SqueezeNet -> match once, refill the pixel buffer and the records with other
    images of other sizes, replay: equal to eager execution.  Then two streams with their own buffers side by side."""
    import torch
    ssd_net, face, gallery = cascade_nets
    sets = _image_sets()
    cas = _Cascade(ssd_net, face, gallery)
    refs = []
    for s in sets:
        out = cas(*P.pack(s, P.SSD300, DEV))
        torch.cuda.synchronize()
        refs.append(_host(out))
    assert not torch.equal(refs[0]["rois"], refs[1]["rois"])
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
    for k in (1, 2, 0, 1):
        P.pack(sets[k], P.SSD300, DEV, pixels=pixels, srcs=srcs)
        g.replay()
        torch.cuda.synchronize()
        _equal(_host(out), refs[k], f"replay of set {k}")
    # two streams, their own cascades (workspaces) and inputs, side by side
    both = [cas, _Cascade(ssd_net, face, gallery)]
    ins = [P.pack(s, P.SSD300, DEV) for s in sets[:2]]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    outs = []
    for _ in range(3):
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                o = both[i](*ins[i])
                outs.append((i, {k: v.clone() for k, v in o.items()}))
    torch.cuda.synchronize()
    for i, o in outs:
        _equal(_host(o), refs[i], f"stream {i}")
