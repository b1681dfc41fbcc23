"""Detection accuracy, CPU side: the matching statement ssd.match_reference on hand-worked cases, tf2_det_eval_summarise on a
hand-worked precision / recall curve, match_reference + tf2_det_eval_summarise against the independent global-form statement
ssd.voc_eval_reference on seeded data, the host refusals of tf2_det_eval_create / _run, and the scratch-free ISA of ssd_eval.hip.
The device itself is checked in tests/test_gpu_ssd_eval.py, which takes its inputs from `make_case` below."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tf2_amd import _lib, ssd

FAKE = 0x1000        # a non-null "device pointer" for calls that must be refused before they touch it
KINDS = ["jitter", "ties", "sparse", "difficult"]


def _one_image(rows_by_class, gts, num_classes=3, top_k=4, max_gt=4, thresh=0.5):
    """match_reference on one image: rows_by_class {c: [(score, x1, y1, x2, y2), ...]}, gts [(x1, y1, x2, y2, label, difficult)]"""
    det = np.zeros((1, num_classes, top_k, 5), np.float32)
    counts = np.zeros((1, num_classes), np.int32)
    for c, rows in rows_by_class.items():
        det[0, c, :len(rows)] = rows
        counts[0, c] = len(rows)
    gt, cnt = ssd.pack_ground_truth([np.asarray(gts, np.float64).reshape(-1, 6)], max_gt)
    m = ssd.match_reference(det, counts, gt, cnt, thresh)
    assert m.status[0] == 0
    return m


def test_two_rows_on_one_ground_truth_tp_then_fp():
    m = _one_image({1: [(.9, 0, 0, .5, .5), (.8, 0, 0, .5, .5)]}, [(0, 0, .5, .5, 1, 0)])
    assert m.flags[0, 1].tolist() == [1, 0, -2, -2] and m.npos[0].tolist() == [0, 1, 0] and m.duplicates[0, 1] == 1
    assert m.scores[0, 1].tolist() == [np.float32(.9), np.float32(.8), 0, 0]
    assert (m.flags[0, 0] == -2).all() and (m.flags[0, 2] == -2).all()


def test_difficult_ground_truth_is_ignored_and_not_in_npos():
    m = _one_image({1: [(.9, 0, 0, .5, .5), (.8, .5, .5, 1, 1)]}, [(0, 0, .5, .5, 1, 1), (.5, .5, 1, 1, 1, 0)])
    assert m.flags[0, 1].tolist() == [-1, 1, -2, -2] and m.npos[0, 1] == 1
    # every row on a difficult box is ignored: it is never "taken"
    m = _one_image({1: [(.9, 0, 0, .5, .5), (.8, 0, 0, .5, .5)]}, [(0, 0, .5, .5, 1, 1)])
    assert m.flags[0, 1].tolist() == [-1, -1, -2, -2] and m.npos[0, 1] == 0


def test_iou_exactly_at_the_threshold_is_a_false_positive():
    """det (0, 0, .5, .5) against gt (0, 0, .5, 1): inter .25, union .5, IoU 0.5 exactly in float32 -- not > 0.5"""
    m = _one_image({1: [(.9, 0, 0, .5, .5)]}, [(0, 0, .5, 1, 1, 0)])
    assert m.flags[0, 1, 0] == 0 and m.duplicates[0, 1] == 0
    m = _one_image({1: [(.9, 0, 0, .5, .5)]}, [(0, 0, .5, .75, 1, 0)])
    assert m.flags[0, 1, 0] == 1
    m = _one_image({1: [(.9, 0, 0, .5, .5)]}, [(0, 0, .5, 1, 1, 0)], thresh=0.25)
    assert m.flags[0, 1, 0] == 1


def test_equal_iou_the_lower_index_wins_and_no_fall_back():
    """two identical ground truths: row 0 takes index 0; row 1's winner is index 0 again (taken): FP although index 1 is free"""
    m = _one_image({1: [(.9, 0, 0, .5, .5), (.8, 0, 0, .5, .5)]}, [(0, 0, .5, .5, 1, 0), (0, 0, .5, .5, 1, 0)])
    assert m.flags[0, 1].tolist() == [1, 0, -2, -2] and m.npos[0, 1] == 2 and m.duplicates[0, 1] == 1
    # the lower index is the difficult one: ignored, whatever the other is
    m = _one_image({1: [(.9, 0, 0, .5, .5)]}, [(0, 0, .5, .5, 1, 1), (0, 0, .5, .5, 1, 0)])
    assert m.flags[0, 1, 0] == -1


def test_class_without_ground_truth_is_all_false_positives():
    m = _one_image({1: [(.9, 0, 0, .5, .5)], 2: [(.9, 0, 0, .5, .5), (.8, 0, 0, .5, .5), (.1, .1, .1, .2, .2)]}, [(0, 0, .5, .5, 1, 0)])
    assert m.flags[0, 2].tolist() == [0, 0, 0, -2] and m.flags[0, 1].tolist() == [1, -2, -2, -2] and m.npos[0].tolist() == [0, 1, 0]


def test_nan_iou_is_a_false_positive_and_never_wins():
    m = _one_image({1: [(.9, .5, .5, .5, .5)]}, [(.5, .5, .5, .5, 1, 0)])           # 0 / 0
    assert m.flags[0, 1, 0] == 0 and m.npos[0, 1] == 1
    # a NaN in front of a real overlap does not hide it: the second ground truth wins
    m = _one_image({1: [(.9, .5, .5, .5, .5)]}, [(.5, .5, .5, .5, 1, 0), (.25, .25, .75, .75, 1, 0)], thresh=0.0)
    assert m.flags[0, 1, 0] == 0                                                      # (IoU 0 is not > 0)
    m = _one_image({1: [(.9, .25, .25, .75, .75)]}, [(.5, .5, .5, .5, 1, 0), (.25, .25, .75, .75, 1, 0)])
    assert m.flags[0, 1, 0] == 1


def test_statement_status_bits():
    det = np.zeros((6, 3, 4, 5), np.float32)
    counts = np.zeros((6, 3), np.int32)
    gt, cnt = ssd.pack_ground_truth([[[0, 0, .5, .5, 1, 0]]] * 6, 4)
    cnt[1] = 5
    gt[2, 0]["label"] = 3
    gt[3, 0]["box"] = (0, 0, np.inf, .5)
    counts[4, 2] = 5
    m = ssd.match_reference(det, counts, gt, cnt, slots=[0, 1, 2, 3, 4, 9], capacity=9)
    assert m.status.tolist() == [0, ssd.EVAL_BAD_COUNT, ssd.EVAL_BAD_LABEL, ssd.EVAL_BAD_BOX, ssd.EVAL_BAD_DET, ssd.EVAL_BAD_SLOT]
    gt[3, 0]["box"] = (.5, 0, .25, .5)
    cnt[3] = -1
    counts[3, 0] = -1
    m = ssd.match_reference(det, counts, gt, cnt, slots=[0, 1, 2, -1, 4, 8], capacity=9)
    assert m.status.tolist() == [0, 2, 4, 0, 16, 0] and (m.flags[3] == -2).all()
    m = ssd.match_reference(det, counts, gt, cnt, slots=[0, 1, 2, 9, 4, 8], capacity=9)
    assert m.status[3] == 1 | 2 | 16                                                  # a bad count: the box is not looked at


def _store_of_flags(flags, scores, npos):
    """a one-class (+ background) store of one image per (flags, scores) row set"""
    k = max(len(f) for f in flags)
    H = ssd.EvalHandle(2, k, len(flags) + 2, 4, 0.5)
    store = np.zeros(H.store_size, np.uint8)
    v = H.views(store)
    v["flags"][:] = -2
    for s, (f, sc, n) in enumerate(zip(flags, scores, npos)):
        v["seen"][s + 1] = 1
        v["npos"][s + 1, 1] = n
        v["flags"][s + 1, 1, :len(f)] = f
        v["scores"][s + 1, 1, :len(f)] = sc
    return H, store


def test_hand_worked_ap():
    """TP, FP, TP with npos 2: recall .5, .5, 1; precision 1, .5, 2/3"""
    H, store = _store_of_flags([[1, 0, 1]], [[.9, .8, .7]], [2])
    r = H.summarise(store)
    assert abs(r["ap"][1] - (0.5 * 1 + 0.5 * (2 / 3))) < 1e-15 and r["map"] == r["ap"][1] and np.isnan(r["ap"][0])
    assert (r["npos"][1], r["tp"][1], r["fp"][1], r["images"]) == (2, 2, 1, 1)
    r = H.summarise(store, use_07_metric=True)
    assert abs(r["ap"][1] - (6 * 1 + 5 * (2 / 3)) / 11) < 1e-15
    # the same three rows spread over two images, an ignored row in between: the same curve
    H, store = _store_of_flags([[1, -1, 1], [0]], [[.9, .85, .7], [.8]], [1, 1])
    r = H.summarise(store)
    assert abs(r["ap"][1] - (0.5 + 0.5 * 2 / 3)) < 1e-15 and (r["tp"][1], r["fp"][1], r["images"]) == (2, 1, 2)
    # the pinned order on equal scores: slot ascending, then rank -- FP (slot 1) before TP (slot 2) gives precision 1/2 at recall 1
    H, store = _store_of_flags([[0], [1]], [[.5], [.5]], [0, 1])
    assert H.summarise(store)["ap"][1] == 0.5
    H, store = _store_of_flags([[1], [0]], [[.5], [.5]], [1, 0])
    assert H.summarise(store)["ap"][1] == 1.0
    assert ssd.voc_ap([.5, .5, 1], [1, .5, 2 / 3]) == pytest.approx(0.5 + 0.5 * 2 / 3, abs=1e-15)
    assert ssd.voc_ap([.5, .5, 1], [1, .5, 2 / 3], True) == pytest.approx((6 + 5 * 2 / 3) / 11, abs=1e-15)


def test_npos_zero_is_nan_and_left_out_of_the_mean():
    H = ssd.EvalHandle(4, 2, 3, 4, 0.5)
    det = np.zeros((1, 4, 2, 5), np.float32)
    counts = np.zeros((1, 4), np.int32)
    det[0, 1, 0] = (.9, 0, 0, .5, .5); counts[0, 1] = 1         # class 1: one TP
    det[0, 2, 0] = (.9, 0, 0, .5, .5); counts[0, 2] = 1         # class 2: a detection, no ground truth: npos 0
    det[0, 3, 0] = (.9, 0, 0, .5, .5); counts[0, 3] = 1         # class 3: only a difficult ground truth: npos 0, row ignored
    gt, cnt = ssd.pack_ground_truth([[[0, 0, .5, .5, 1, 0], [0, 0, .5, .5, 3, 1]]], 4)
    m = ssd.match_reference(det, counts, gt, cnt)
    r = H.summarise(H.store_from([m], [[2]]))
    assert r["ap"][1] == 1.0 and np.isnan(r["ap"][[0, 2, 3]]).all() and r["map"] == 1.0
    assert r["npos"].tolist() == [0, 1, 0, 0] and r["tp"].tolist() == [0, 1, 0, 0] and r["fp"].tolist() == [0, 0, 1, 0]
    w = ssd.voc_eval_reference(det, counts, gt, cnt, [2])
    assert w["map"] == 1.0 and np.isnan(w["ap"][[0, 2, 3]]).all() and w["fp"].tolist() == [0, 0, 1, 0]
    # nothing seen: every class NaN, and so is the mean
    r = H.summarise(np.zeros(H.store_size, np.uint8))
    assert np.isnan(r["ap"]).all() and np.isnan(r["map"]) and r["images"] == 0


def make_case(kind, batch, num_classes, top_k, max_gt, seed):
    """Seeded (det [B, C, K, 5], counts [B, C], gt records [B, max_gt], gt_count [B]) for the evaluator:
      jitter     detections are perturbed ground truths (some twice: duplicates) plus noise boxes, continuous scores
      ties       dyadic coordinates, duplicated ground truths and detections, detections of IoU exactly 0.5, four score levels
      sparse     half the images without ground truth, ground truth in at most three classes, half the other classes without rows
      difficult  jitter with four of five ground truths difficult
    Image 0 has max_gt ground truths (every lane's last register in use); class 1 has top_k rows and class 2 up to 70 and more (rows
    beyond the first 64 of a class).  Rows are best first; rows past counts hold garbage the
    evaluator must not look at."""
    rng = np.random.default_rng([seed, batch, num_classes, top_k, max_gt])
    B, Cn, K = batch, num_classes, top_k
    det = rng.uniform(-5, 5, (B, Cn, K, 5)).astype(np.float32)
    counts = np.zeros((B, Cn), np.int32)
    images = []
    levels = np.float32([0.9, 0.6, 0.3, 0.05])
    for b in range(B):
        n_gt = max_gt if b == 0 else int(rng.integers(1, max_gt + 1))
        if kind == "sparse" and b % 2 == 1:
            n_gt = 0
        pool = np.arange(1, Cn) if kind != "sparse" else rng.choice(np.arange(1, Cn), min(3, Cn - 1), replace=False)
        label = rng.choice(pool, n_gt)
        if kind == "ties":
            xy = rng.integers(0, 6, (n_gt, 2)) / 8.0
            wh = rng.integers(1, 3, (n_gt, 2)) / 8.0
        else:
            xy = rng.uniform(0, 0.7, (n_gt, 2))
            wh = rng.uniform(0.05, 0.3, (n_gt, 2))
        box = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        if kind == "ties":                        # duplicated ground truths: a later one repeats an earlier one of its class
            for i in range(1, n_gt):
                same = np.flatnonzero(label[:i] == label[i])
                if same.size and rng.random() < 0.3:
                    box[i] = box[same[0]]
        difficult = rng.random(n_gt) < (0.8 if kind == "difficult" else 0.2)
        images.append(np.concatenate([box.astype(np.float64), label[:, None], difficult[:, None]], 1))
        for c in range(1, Cn):
            rows = []
            for i in np.flatnonzero(label == c):
                u = rng.random()
                if u < 0.85:
                    if kind == "ties":
                        half = box[i].copy()
                        half[2] = half[0] + (half[2] - half[0]) / 2            # half the box: IoU 0.5 exactly
                        rows.append(half if rng.random() < 0.3 else box[i])
                    else:
                        rows.append(box[i] + rng.normal(0, 0.01, 4).astype(np.float32))
                if u < 0.45:
                    rows.append(box[i] if kind == "ties" else box[i] + rng.normal(0, 0.01, 4).astype(np.float32))
            if not (kind == "sparse" and not (label == c).any() and rng.random() < 0.5):
                for _ in range(K if c == 1 else 70 if c == 2 else int(rng.integers(0, 4))):
                    xy0 = rng.integers(0, 6, 2) / 8.0 if kind == "ties" else rng.uniform(0, 0.7, 2)
                    wh0 = rng.integers(1, 3, 2) / 8.0 if kind == "ties" else rng.uniform(0.05, 0.3, 2)
                    rows.append(np.concatenate([xy0, xy0 + wh0]).astype(np.float32))
            if not rows:
                continue
            rows = np.stack(rows)[rng.permutation(len(rows))][:K]
            n = rows.shape[0]
            score = levels[rng.integers(0, 4, n)] if kind == "ties" else rng.uniform(0.01, 1, n).astype(np.float32)
            det[b, c, :n, 0] = -np.sort(-score)
            det[b, c, :n, 1:] = rows
            counts[b, c] = n
    gt, cnt = ssd.pack_ground_truth(images, max_gt)
    return det, counts, gt, cnt


def census(m):
    """(true positives, duplicates, ignored rows, false positives) of a MatchResult"""
    return int((m.flags == 1).sum()), int(m.duplicates.sum()), int((m.flags == -1).sum()), int((m.flags == 0).sum())


def _same_result(got, want):
    for key in ("npos", "tp", "fp"):
        np.testing.assert_array_equal(got[key], want[key], key)
    assert got["images"] == want["images"]
    assert np.array_equal(np.isnan(got["ap"]), np.isnan(want["ap"]))
    have = ~np.isnan(want["ap"])
    # 1e-9 absolute: at most ~1e6 terms in [0, 1] in double, any summation order stays within n 2^-53 sum < 1.2e-10
    assert np.abs(got["ap"][have] - want["ap"][have]).max(initial=0.0) <= 1e-9
    assert abs(got["map"] - want["map"]) <= 1e-9


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("use_07", [False, True])
def test_per_image_matching_is_the_global_protocol(kind, use_07):
    """match_reference (per image) + tf2_det_eval_summarise == voc_eval_reference (one global sorted list per class) over three
    batches whose slots are shuffled with gaps, one image skipped; ties and duplicates cross images in the "ties" kind"""
    Cn, K, G, cap = 6, 12, 10, 40
    rng = np.random.default_rng(17)
    slots = rng.choice(cap, 15, replace=False).astype(np.int32).reshape(3, 5)
    slots[1, 3] = -1
    H = ssd.EvalHandle(Cn, K, cap, G, 0.5)
    cases = [make_case(kind, 5, Cn, K, G, seed) for seed in (1, 2, 3)]
    matches = [ssd.match_reference(*case, 0.5, slots=sl, capacity=cap) for case, sl in zip(cases, slots)]
    tp, dup, ign, fp = map(sum, zip(*(census(m) for m in matches)))
    assert tp > 0 and dup > 0 and ign > 0 and fp > 0, (tp, dup, ign, fp)
    assert any((case[3] == 0).any() for case in cases) or kind != "sparse"          # empty images
    got = H.summarise(H.store_from(matches, slots), use_07)
    whole = [np.concatenate([case[i] for case in cases]) for i in range(4)]
    want = ssd.voc_eval_reference(*whole, image_ids=slots.reshape(-1), iou_thresh=0.5, use_07_metric=use_07)
    assert want["images"] == 14 and 0 < want["map"] < 1
    _same_result(got, want)
    # the store is a function of the (slot, image) pairs: the batches in another order give the same bytes
    assert np.array_equal(H.store_from(matches[::-1], slots[::-1]), H.store_from(matches, slots))


def _create(**kw):
    d = _lib.DetEvalDesc(C.sizeof(_lib.DetEvalDesc), 21, 200, 64, 100, 0.5)
    for k, v in kw.items():
        if k != "desc":
            setattr(d, k, v)
    h = C.c_void_p()
    st = _lib.lib().tf2_det_eval_create(C.byref(d) if kw.get("desc", True) else None, C.byref(h))
    err = _lib.lib().tf2_last_error().decode()
    assert (st == 0) == bool(h.value)
    if h.value:
        _lib.lib().tf2_det_eval_destroy(h)
    return st, err


def test_create_refusals():
    assert C.sizeof(_lib.DetEvalDesc) == 24 and ssd.GT_DTYPE.itemsize == 24 and C.sizeof(_lib.DetEvalClass) == 32
    assert _create()[0] == 0
    for kw, message in ((dict(size=20), "desc size"), (dict(size=28), "desc size"), (dict(desc=False), "desc size"),
                        (dict(num_classes=1), "num_classes must be in 2..256"), (dict(num_classes=257), "num_classes"),
                        (dict(top_k=0), "top_k must be in 1..256"), (dict(top_k=257), "top_k"),
                        (dict(max_gt=0), "max_gt must be in 1..256"), (dict(max_gt=257), "max_gt"),
                        (dict(capacity=0), "capacity"), (dict(capacity=-4), "capacity"),
                        (dict(iou_thresh=-0.1), "iou_thresh"), (dict(iou_thresh=float("nan")), "iou_thresh"),
                        (dict(iou_thresh=float("inf")), "iou_thresh")):
        st, err = _create(**kw)
        assert st == -1 and message in err, (kw, st, err)
    for kw in (dict(num_classes=2, top_k=1, max_gt=1, capacity=1, iou_thresh=0.0), dict(num_classes=256, top_k=256, max_gt=256)):
        assert _create(**kw)[0] == 0
    assert _lib.lib().tf2_det_eval_create(C.byref(_lib.DetEvalDesc()), None) == -1
    assert _lib.lib().tf2_abi_version() == 1


def test_store_size_and_layout():
    H = ssd.EvalHandle(21, 200, 7, 64, 0.5)
    assert H.store_size == 7 * 4 * (1 + 21 + 21 * 200) + 7 * 21 * 200
    v = H.views(np.zeros(H.store_size, np.uint8))
    assert v["seen"].shape == (7,) and v["npos"].shape == (7, 21) and v["scores"].shape == (7, 21, 200) and v["flags"].shape == (7, 21, 200)
    assert _lib.lib().tf2_det_eval_store_size(None) == 0


def test_run_refusals():
    """every refusal of tf2_det_eval_run / _store_init / _summarise comes before any device call: the pointers are fakes and there is
    no device here"""
    L = _lib.lib()
    H = ssd.EvalHandle(21, 200, 10, 64, 0.5)
    good = dict(h=H._h, det=FAKE, counts=FAKE, gt=FAKE, gt_count=FAKE, slot=FAKE, batch=2, store=FAKE, bytes=H.store_size, status=FAKE)
    for kw, message in ((dict(batch=0), "batch must be >= 1"), (dict(batch=-2), "batch must be >= 1"),
                        (dict(det=None), "null det_dev / counts_dev"), (dict(counts=None), "null det_dev / counts_dev"),
                        (dict(gt=None), "null gt_dev"), (dict(gt_count=None), "null gt_dev / gt_count_dev"),
                        (dict(slot=None), "slot_dev"), (dict(store=None), "null store_dev"), (dict(status=None), "status_dev"),
                        (dict(h=None), "null tf2_det_eval handle"), (dict(bytes=H.store_size - 1), "tf2_det_eval_store_size is"),
                        (dict(bytes=0), "tf2_det_eval_store_size is")):
        a = dict(good, **kw)
        st = L.tf2_det_eval_run(a["h"], a["det"], a["counts"], a["gt"], a["gt_count"], a["slot"], a["batch"], a["store"], a["bytes"],
                                a["status"], None, None)
        err = L.tf2_last_error().decode()
        assert st == -1 and message in err, (kw, st, err)
    for args, message in (((None, FAKE, H.store_size, None), "null tf2_det_eval handle"), ((H._h, None, H.store_size, None), "null store_dev"),
                          ((H._h, FAKE, H.store_size - 1, None), "tf2_det_eval_store_size is")):
        assert L.tf2_det_eval_store_init(*args) == -1 and message in L.tf2_last_error().decode()
    per = (_lib.DetEvalClass * 21)()
    host = np.zeros(H.store_size, np.uint8)
    for args, message in (((None, host.ctypes.data, host.size, 0, per, None, None), "null tf2_det_eval handle"),
                          ((H._h, None, host.size, 0, per, None, None), "null store_host"),
                          ((H._h, host.ctypes.data, host.size, 0, None, None, None), "per_class"),
                          ((H._h, host.ctypes.data, host.size - 1, 0, per, None, None), "tf2_det_eval_store_size is")):
        assert L.tf2_det_eval_summarise(*args) == -1 and message in L.tf2_last_error().decode()
    assert L.tf2_det_eval_summarise(H._h, host.ctypes.data, host.size, 0, per, None, None) == 0        # images / map are optional


def test_pack_ground_truth():
    gt, cnt = ssd.pack_ground_truth([np.zeros((0, 6)), [[.1, .2, .3, .4, 7, 1]]], 3)
    assert gt.shape == (2, 3) and cnt.tolist() == [0, 1] and gt.view(np.int32).reshape(2, 3, 6)[1, 0, 4:].tolist() == [7, 1]
    assert gt[1, 0]["box"].tolist() == [np.float32(.1), np.float32(.2), np.float32(.3), np.float32(.4)]
    again, _ = ssd.pack_ground_truth([gt[0, :0], gt[1, :1]], 3)
    assert again.tobytes() == gt.tobytes()
    with pytest.raises(ValueError):
        ssd.pack_ground_truth([np.zeros((4, 6))], 3)


def test_eval_kernel_compiles_without_scratch():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import vmcnt_check
    seg, lds, txt = vmcnt_check.kernel_segments("ssd_eval")
    names = [k for k in seg if "det_eval_kernel" in k]
    assert len(names) == 1 and len(seg) == 1, seg
    assert seg[names[0]] == 0, seg
    assert "scratch_" not in txt.split("amdhsa.kernels")[0]
