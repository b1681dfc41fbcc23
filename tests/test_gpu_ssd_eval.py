"""Detection accuracy on the MI355X (tf2_det_eval_*, ssd_eval.hip): the store bit-identical to the host statement
ssd.match_reference at the shapes where the kernel changes path, every status bit raised alone with the store untouched, detect +
update in one captured graph replayed over refilled records, two streams into one store, and SSD300 (quarter width) end to end
against the independent statement ssd.voc_eval_reference."""
import numpy as np
import pytest

from tf2_amd import config as cfg, ssd, synth
from tf2_amd.network import NetWork
from tests.test_ssd_eval import KINDS, _same_result, census, make_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A
# (batch, C, top_k, max_gt): one lane's worth of ground truths (64), one past it, four per lane (256); the ends of top_k and C
SHAPES = [(1, 2, 1, 1), (5, 21, 200, 64), (5, 21, 200, 65), (32, 21, 200, 42), (3, 201, 256, 256)]


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32).reshape(a.shape + (6,)) if a.dtype == ssd.GT_DTYPE else a).to(DEV)


def _evaluator(C, K, cap, G, thresh=0.5):
    """an evaluator whose store is prefilled with a sentinel (then `seen` zeroed, as every epoch starts)"""
    ev = ssd.DeviceEvaluator(C, K, cap, G, thresh, device=DEV)
    ev.store.fill_(SENTINEL)
    ev.reset()
    return ev


def _check_store(ev, matches, slots):
    """the device store against the statement: written slots bit for bit, every other byte still the sentinel, seen exact"""
    got, want = ev.views(ev.store_host()), ev.views(ev.store_from(matches, slots))
    np.testing.assert_array_equal(got["seen"], want["seen"])
    on = want["seen"] != 0
    np.testing.assert_array_equal(got["npos"][on], want["npos"][on])
    np.testing.assert_array_equal(got["flags"][on], want["flags"][on])
    np.testing.assert_array_equal(got["scores"][on].view(np.uint32), want["scores"][on].view(np.uint32))
    for key in ("npos", "flags", "scores"):
        assert (got[key][~on].view(np.uint8) == SENTINEL).all(), key


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_store_bit_identical(kind, shape):
    """Flags, scores, npos and seen of the store, and flags_out, against match_reference.  Every case must contain true positives,
    duplicates and ignored rows, asserted on the statement's output (a run of the fill path alone cannot pass).  The smallest shape
    has one row and one ground truth an image: it runs 48 seeded images, one a step, and asserts true positives, ignored rows and
    false positives over them -- a duplicate needs two rows of one class."""
    import torch
    B, C, K, G = shape
    tiny = K == 1
    steps = 48 if tiny else 1
    cap = steps * B + 5
    ev = _evaluator(C, K, cap, G)
    rng = np.random.default_rng(B * 1000 + G)
    free = rng.permutation(cap)
    matches, all_slots, total = [], [], np.zeros(4, np.int64)
    for step in range(steps):
        case = make_case(kind, B, C, K, G, seed=step)
        slots = free[step * B:(step + 1) * B].astype(np.int32)
        if kind == "sparse" and B > 2:
            slots[B // 2] = -1                                        # padding of a last batch
        want = ssd.match_reference(*case, 0.5, slots=slots, capacity=cap)
        assert (want.status == 0).all()
        total += census(want)
        status, flags = ev.update(_dev(case[0]), _dev(case[1]), _dev(case[2]), _dev(case[3]), _dev(slots), flags=True)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(status.cpu().numpy(), want.status)
        np.testing.assert_array_equal(flags.cpu().numpy(), want.flags)
        matches.append(want); all_slots.append(slots)
    tp, dup, ign, fp = total
    assert tp > 0 and ign > 0 and fp > 0 and (dup > 0 or tiny), total
    _check_store(ev, matches, all_slots)
    if not tiny:                                                      # rows beyond the first 64 of a class took part
        assert (matches[0].flags[:, :, 64:] >= 0).any()


BAD = {
    "slot": (ssd.EVAL_BAD_SLOT, lambda det, counts, gt, cnt, slots, cap, C, K, G: slots.__setitem__(2, cap)),
    "slot_huge": (ssd.EVAL_BAD_SLOT, lambda det, counts, gt, cnt, slots, cap, C, K, G: slots.__setitem__(2, 2 ** 31 - 1)),
    "count_over": (ssd.EVAL_BAD_COUNT, lambda det, counts, gt, cnt, slots, cap, C, K, G: cnt.__setitem__(2, G + 1)),
    "count_negative": (ssd.EVAL_BAD_COUNT, lambda det, counts, gt, cnt, slots, cap, C, K, G: cnt.__setitem__(2, -1)),
    "label_over": (ssd.EVAL_BAD_LABEL, lambda det, counts, gt, cnt, slots, cap, C, K, G: gt["label"].__setitem__((2, 1), C)),
    "label_zero": (ssd.EVAL_BAD_LABEL, lambda det, counts, gt, cnt, slots, cap, C, K, G: gt["label"].__setitem__((2, 0), 0)),
    "box_nan": (ssd.EVAL_BAD_BOX, lambda det, counts, gt, cnt, slots, cap, C, K, G: gt["box"].__setitem__((2, 3, 1), np.nan)),
    "box_inverted": (ssd.EVAL_BAD_BOX, lambda det, counts, gt, cnt, slots, cap, C, K, G: gt["box"].__setitem__((2, 0), (.5, .1, .25, .3))),
    "det_over": (ssd.EVAL_BAD_DET, lambda det, counts, gt, cnt, slots, cap, C, K, G: counts.__setitem__((2, 7), K + 1)),
    "det_negative": (ssd.EVAL_BAD_DET, lambda det, counts, gt, cnt, slots, cap, C, K, G: counts.__setitem__((2, 0), -1)),
}


@pytest.mark.parametrize("which", list(BAD))
def test_status_bits_and_store_safety(which):
    """One malformed image (image 2) in a batch of good ones raises its bit alone; its slot (where it has a valid one) keeps the
    sentinel and its seen stays 0; the good images are exact.  Nothing is read or written through a malformed record: every record is
    validated before it indexes anything."""
    import torch
    B, C, K, G, cap = 6, 21, 200, 64, 9
    bit, spoil = BAD[which]
    det, counts, gt, cnt = make_case("jitter", B, C, K, G, seed=5)
    assert cnt[2] >= 4
    slots = np.array([4, 0, 7, 1, 8, 3], np.int32)
    spoil(det, counts, gt, cnt, slots, cap, C, K, G)
    want = ssd.match_reference(det, counts, gt, cnt, 0.5, slots=slots, capacity=cap)
    assert want.status.tolist() == [0, 0, bit, 0, 0, 0] and census(want)[0] > 0
    ev = _evaluator(C, K, cap, G)
    status, flags = ev.update(_dev(det), _dev(counts), _dev(gt), _dev(cnt), _dev(slots), flags=True)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0, bit, 0, 0, 0]
    np.testing.assert_array_equal(flags.cpu().numpy(), want.flags)
    assert (flags[2].cpu().numpy() == -2).all()
    _check_store(ev, [want], [slots])
    seen = ev.views(ev.store_host())["seen"]
    assert seen.sum() == 5 and seen[7] == 0
    r = ev.result()
    assert r["images"] == 5


def _ssd_net(width_div, seed=3, loc_q=6, conf_q=3):
    """SSD300 at `width_div` with head Qs that keep dequantised loc within +-2 (int8 / 2^6) and conf within +-16 (the net of
    tests/test_gpu_ssd_detect.py, restated)"""
    t = cfg.ssd300_tables(width_div=width_div)
    plan = cfg.build_plan(t)
    q = np.array(synth.synth_q_values(t, seed, spread=1))
    at, pos = {}, 3
    for L in plan:                                # file-order Q positions per table row
        if not L.ipool:
            at[L.index] = pos; pos += L.N
        elif L.ipool == 2:
            pos += L.N
    for lr, cr in ssd.head_rows(plan):
        q[at[lr]:at[lr] + plan[lr].N] = loc_q
        q[at[cr]:at[cr] + plan[cr].N] = conf_q
    net = NetWork(t)
    net.Init(synth.synth_model(t, q, seed), synth.q_text(q), device=DEV)
    return t, net


@pytest.fixture(scope="module")
def small_net():
    return _ssd_net(4)


def _enclosed_pair(det, counts, b):
    """(class, box) of the first class of image b with two rows whose enclosing box has IoU > 0.6 with each of them, or None.  The
    detector's NMS leaves rows of one class with IoU <= 0.45, so no ground truth cut from one row is matched by a second one; a ground
    truth around two of them is: alone in its class, it is the earlier row's true positive and the later row's duplicate."""
    for c in range(1, counts.shape[1]):
        bx = det[b, c, :int(counts[b, c]), 1:].astype(np.float64)
        lo = np.minimum(bx[:, None, :2], bx[None, :, :2])
        hi = np.maximum(bx[:, None, 2:], bx[None, :, 2:])
        area = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
        around = (hi - lo).prod(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            ok = np.triu(np.minimum(area[:, None], area[None, :]) / around > 0.6, 1)      # (a row lies inside the box: IoU = area ratio)
        if ok.any():
            i, j = np.argwhere(ok)[0]
            return c, (*lo[i, j], *hi[i, j])
    return None


def _gt_from_detections(det, counts, rng, max_gt, per_image=12):
    """ground truth made of a subset of an image's own detections, jittered (true positives exist), one in five difficult, and one box
    around two rows of a class that gets no other ground truth (_enclosed_pair: a duplicate exists)"""
    images = []
    B, C = counts.shape
    for b in range(B):
        pair = _enclosed_pair(det, counts, b)
        rows = [(*pair[1], pair[0], False)] if pair else []
        for _ in range(per_image):
            c = int(rng.integers(1, C))
            if counts[b, c] == 0 or (pair and c == pair[0]):
                continue
            r = int(rng.integers(0, min(int(counts[b, c]), 6)))
            box = det[b, c, r, 1:].astype(np.float64) + rng.normal(0, 0.004, 4)
            x1, x2 = sorted((box[0], box[2]))
            y1, y2 = sorted((box[1], box[3]))
            rows.append((x1, y1, x2, y2, c, rng.random() < 0.2))
        images.append(np.asarray(rows[:max_gt], np.float64).reshape(-1, 6))
    return ssd.pack_ground_truth(images, max_gt)


def _detect_inputs(rng, batch):
    """decoded boxes [B, 8732, 4] and peaked class probabilities [B, 8732, 21] for DeviceDetector.detect"""
    import torch
    pri = ssd.prior_boxes(ssd.VOC)
    loc = torch.from_numpy(rng.normal(0, 1.0, (batch, 8732, 4)).astype(np.float32))
    boxes = torch.stack([ssd.decode(loc[b], pri, ssd.VOC["variance"]) for b in range(batch)])
    probs = torch.softmax(torch.from_numpy(rng.normal(0, 4.0, (batch, 8732, 21)).astype(np.float32)), -1)
    return boxes.contiguous().to(DEV), probs.contiguous().to(DEV)


def test_graph_replay_refilled_records_and_idempotence(small_net):
    """detect + update captured once on one stream; three replays with new boxes, ground truth and slots leave the statement's
    store; replaying the first batch again changes no byte of it"""
    import torch
    t, net = small_net
    B, C, K, G, cap = 3, 21, 200, 64, 12
    detector = ssd.DeviceDetector(net, net.plan, ssd.VOC)
    ev = _evaluator(C, K, cap, G)
    rng = np.random.default_rng(8)
    fills = []
    for i in range(3):
        boxes, probs = _detect_inputs(rng, B)
        det, counts = detector.detect(boxes, probs)
        torch.cuda.synchronize()
        det, counts = det.cpu().numpy(), counts.cpu().numpy()
        gt, cnt = _gt_from_detections(det, counts, rng, G)
        slots = np.array([[5, 0, 9], [2, -1, 11], [7, 1, 4]], np.int32)[i]
        fills.append((boxes, probs, _dev(gt), _dev(cnt), _dev(slots), slots, ssd.match_reference(det, counts, gt, cnt, 0.5, slots=slots, capacity=cap)))
    tp, dup, ign, fp = map(sum, zip(*(census(f[6]) for f in fills)))
    assert tp > 0 and dup > 0 and ign > 0 and fp > 0, (tp, dup, ign, fp)
    s_boxes, s_probs, s_gt, s_cnt, s_slots = (torch.empty_like(v) for v in fills[0][:5])
    s_slots.fill_(-1)
    status = torch.empty(B, dtype=torch.int32, device=DEV)
    for dst, src in zip((s_boxes, s_probs, s_gt, s_cnt), fills[0][:4]):
        dst.copy_(src)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ev.update(*detector.detect(s_boxes, s_probs), s_gt, s_cnt, s_slots, status=status)      # warm up (every image skipped)
        torch.cuda.current_stream().synchronize()
        with torch.cuda.graph(g, stream=side):
            ev.update(*detector.detect(s_boxes, s_probs), s_gt, s_cnt, s_slots, status=status)
    torch.cuda.current_stream().wait_stream(side)

    def replay(fill):
        for dst, src in zip((s_boxes, s_probs, s_gt, s_cnt, s_slots), fill[:5]):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0] * B
    for fill in fills:
        replay(fill)
    _check_store(ev, [f[6] for f in fills], [f[5] for f in fills])
    before = ev.store.clone()
    replay(fills[0])
    assert torch.equal(ev.store, before)
    assert ev.result()["images"] == 8


def test_two_streams_into_one_store():
    import torch
    B, C, K, G, cap = 5, 21, 200, 42, 16
    ev = _evaluator(C, K, cap, G)
    cases = [make_case(kind, B, C, K, G, seed=9) for kind in ("jitter", "ties")]
    slots = [np.array([0, 2, 4, 6, 8], np.int32), np.array([15, 1, 3, 13, 5], np.int32)]
    wants = [ssd.match_reference(*c, 0.5, slots=s, capacity=cap) for c, s in zip(cases, slots)]
    ins = [[_dev(v) for v in c] + [_dev(s)] for c, s in zip(cases, slots)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream()); s2.wait_stream(torch.cuda.current_stream())
    outs = []
    for _ in range(3):
        outs.append((ev.update(*ins[0], stream=s1), ev.update(*ins[1], stream=s2)))
    torch.cuda.synchronize()
    for a, b in outs:
        assert a.cpu().tolist() == [0] * B and b.cpu().tolist() == [0] * B
    _check_store(ev, wants, slots)
    got = ev.result()
    whole = [np.concatenate([c[i] for c in cases]) for i in range(4)]
    _same_result(got, ssd.voc_eval_reference(*whole, image_ids=np.concatenate(slots)))


def test_end_to_end_quarter_width(small_net):
    """DeviceDetector.run on two batches, ground truth from the first run's own detections, DeviceEvaluator.update behind each run,
    result() for both metrics against voc_eval_reference on the detections copied to the host"""
    import torch
    t, net = small_net
    B, G = 2, 64
    detector = ssd.DeviceDetector(net, net.plan, ssd.VOC)
    ev = ssd.DeviceEvaluator(21, 200, 6, G, 0.5, device=DEV)
    rng = np.random.default_rng(4)
    xs = [torch.from_numpy(np.ascontiguousarray(synth.synth_images(t, B, seed))).to(DEV) for seed in (31, 32)]
    first = [tuple(v.cpu().numpy() for v in detector.run(x)) for x in xs]
    torch.cuda.synchronize()
    gts = [_gt_from_detections(d, c, rng, G) for d, c in first]
    slots = [np.array([3, 0], np.int32), np.array([5, 2], np.int32)]
    host = []
    for x, (gt, cnt), sl in zip(xs, gts, slots):
        det, counts = detector.run(x)
        status = ev.update(det, counts, gt, cnt, sl)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0, 0]
        host.append((det.cpu().numpy(), counts.cpu().numpy()))
    for (d, c), (d0, c0) in zip(host, first):                          # a run repeats bit for bit
        assert np.array_equal(d, d0) and np.array_equal(c, c0)
    whole = [np.concatenate([h[0] for h in host]), np.concatenate([h[1] for h in host]), np.concatenate([g[0] for g in gts]),
             np.concatenate([g[1] for g in gts])]
    for use_07 in (False, True):
        want = ssd.voc_eval_reference(*whole, image_ids=np.concatenate(slots), iou_thresh=0.5, use_07_metric=use_07)
        got = ev.result(use_07)
        assert want["tp"].sum() > 0 and want["fp"].sum() > 0 and want["images"] == 4
        _same_result(got, want)
    ev.reset()
    torch.cuda.synchronize()
    assert ev.result()["images"] == 0
