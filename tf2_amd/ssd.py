"""SSD300 around the integer engine.

The convolutional part of SSD300-VGG runs as one TF2 table program (`config.ssd300_tables`: VGG base with the
ceil-mode pool, stride-1 pool5, dilated conv6, conv7, the extras and the twelve multibox head convolutions) on the
integer kernels.  What the reference keeps in float on the host side of the detector is restated here with PyTorch
(GPU when available) and pinned to the reference's own functions executed in the build container
(tests/golden/ref_ssd.npz, oracle/gen_golden.py gen_ssd):

  prior boxes   TransForm_Kit/Quantization/models/SSD/layers/functions/prior_box.py:28-57
  decode        .../layers/box_utils.py:140-158
  nms           .../layers/box_utils.py:175-239   (greedy, top_k highest scores first)
  Detect        .../layers/functions/detection.py:27-62
  L2Norm        .../layers/modules/l2norm.py:19-24

The VOC / COCO prior-box configurations are the data of TransForm_Kit/Quantization/data/SSD/config.py:15-45.
No trained SSD weights or datasets ship with the reference, so the mAP of its README cannot be re-measured here.
"""
from __future__ import annotations

from math import sqrt
from typing import Dict, List, Sequence, Tuple

import numpy as np

VOC = dict(num_classes=21, feature_maps=[38, 19, 10, 5, 3, 1], min_dim=300, steps=[8, 16, 32, 64, 100, 300],
           min_sizes=[30, 60, 111, 162, 213, 264], max_sizes=[60, 111, 162, 213, 264, 315],
           aspect_ratios=[[2], [2, 3], [2, 3], [2, 3], [2], [2]], variance=[0.1, 0.2], clip=True, name="VOC")
COCO = dict(num_classes=201, feature_maps=[38, 19, 10, 5, 3, 1], min_dim=300, steps=[8, 16, 32, 64, 100, 300],
            min_sizes=[21, 45, 99, 153, 207, 261], max_sizes=[45, 99, 153, 207, 261, 315],
            aspect_ratios=[[2], [2, 3], [2, 3], [2, 3], [2], [2]], variance=[0.1, 0.2], clip=True, name="COCO")


def prior_boxes(cfg: dict = VOC):
    """Default boxes in centre form, [sum_k f_k^2 * boxes_k, 4] (8732 rows for SSD300), in the reference's order
    (prior_box.py:28-57): per source map k, per cell (row i, column j): the min-size square, the sqrt(min*max) square,
    then for every aspect ratio a the (w, h) pairs (s*sqrt(a), s/sqrt(a)) and (s/sqrt(a), s*sqrt(a)); clipped to
    [0, 1] when cfg['clip'].  Computed per map as a grid of centres times a small table of shapes, in float64 like the
    reference's Python arithmetic, then stored as float32."""
    import torch
    size = float(cfg["min_dim"])
    blocks = []
    for f, step, smin, smax, ratios in zip(cfg["feature_maps"], cfg["steps"], cfg["min_sizes"], cfg["max_sizes"],
                                            cfg["aspect_ratios"]):
        cells = size / step                                   # the reference divides by image_size / step
        centres = (np.arange(f, dtype=np.float64) + 0.5) / cells
        cy, cx = np.meshgrid(centres, centres, indexing="ij")
        s = smin / size
        shapes = [(s, s), (sqrt(s * (smax / size)),) * 2]
        for a_r in ratios:
            shapes += [(s * sqrt(a_r), s / sqrt(a_r)), (s / sqrt(a_r), s * sqrt(a_r))]
        wh = np.asarray(shapes, np.float64)                   # [boxes_k, 2]
        grid = np.stack([cx, cy], -1).reshape(f * f, 1, 2)    # [cells, 1, (cx, cy)]
        blocks.append(np.concatenate([np.broadcast_to(grid, (f * f, len(shapes), 2)),
                                      np.broadcast_to(wh[None], (f * f, len(shapes), 2))], -1).reshape(-1, 4))
    out = torch.from_numpy(np.concatenate(blocks, 0).astype(np.float32))
    return out.clamp_(0, 1) if cfg["clip"] else out


def decode(loc, priors, variances: Sequence[float]):
    """Regression offsets -> boxes (semantics of box_utils.py:140-158).  A prior is (cx, cy, w, h); the network predicts the
    centre shift in units of variance[0] * prior size and the log of the size ratio in units of variance[1]:
        centre = prior_centre + t_xy * v0 * prior_wh,   size = prior_wh * exp(t_wh * v1),
    returned in corner form (centre -+ size / 2)."""
    import torch
    v_centre, v_size = float(variances[0]), float(variances[1])
    p_centre, p_size = priors[:, :2], priors[:, 2:]
    centre = p_centre + loc[:, :2] * v_centre * p_size
    size = p_size * torch.exp(loc[:, 2:] * v_size)
    top_left = centre - size / 2
    return torch.cat((top_left, top_left + size), 1)      # x2 = x1 + w: the reference's own rounding of the far corner


def _iou_one_to_many(box, area_box, others, area_others):
    """IoU of one corner-form box with each row of `others`."""
    import torch
    lo = torch.maximum(others[:, :2], box[:2])
    hi = torch.minimum(others[:, 2:], box[2:])
    wh = (hi - lo).clamp(min=0.0)
    inter = wh[:, 0] * wh[:, 1]
    return inter / ((area_others - inter) + area_box)


def nms(boxes, scores, overlap: float = 0.5, top_k: int = 200):
    """Greedy non-maximum suppression (semantics of box_utils.py:175-239): among the top_k highest scores, repeatedly keep the best
    remaining box and drop every remaining box whose IoU with it exceeds `overlap` (IoU <= overlap survives).  Returns the kept
    indices, best first.  Candidates are walked in ascending-score order from the back, as the reference's sort leaves them,
    so ties resolve the same way."""
    import torch
    if boxes.numel() == 0:
        return torch.zeros(0, dtype=torch.long, device=boxes.device)
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    order = scores.sort(0).indices[-top_k:]                # ascending; the best candidate is the last element
    kept: List[int] = []
    while order.numel() > 0:
        best = order[-1]
        kept.append(int(best))
        order = order[:-1]
        if order.numel() == 0:
            break
        iou = _iou_one_to_many(boxes[best], area[best], boxes[order], area[order])
        order = order[iou <= overlap]
    return torch.tensor(kept, dtype=torch.long, device=boxes.device)


def l2norm(x, weight, eps: float = 1e-10):
    """l2norm.py:19-24: x / (||x||_2 over channels + eps) * weight[c]."""
    norm = x.pow(2).sum(dim=1, keepdim=True).sqrt() + eps
    return weight.view(1, -1, 1, 1) * (x / norm)


def detect(loc, conf, priors, num_classes: int, top_k: int = 200, conf_thresh: float = 0.01, nms_thresh: float = 0.45,
           variance: Sequence[float] = (0.1, 0.2)):
    """Per-image, per-class detection list (semantics of detection.py:27-62).  loc [B, P, 4] offsets, conf [B, P, classes]
    class probabilities -> [B, classes, top_k, 5] rows (score, x1, y1, x2, y2); class 0 is background and stays empty; unused
    rows are zero.  For every foreground class: candidates above conf_thresh, decoded boxes, NMS, best first."""
    import torch
    n_img = loc.size(0)
    result = torch.zeros(n_img, num_classes, top_k, 5, device=loc.device)
    for b in range(n_img):
        boxes_b = decode(loc[b], priors, variance)
        for cls in range(1, num_classes):
            p = conf[b, :, cls]
            sel = p > conf_thresh
            if not bool(sel.any()):
                continue
            cand_scores, cand_boxes = p[sel], boxes_b[sel]
            keep = nms(cand_boxes, cand_scores, nms_thresh, top_k)
            result[b, cls, :keep.numel(), 0] = cand_scores[keep]
            result[b, cls, :keep.numel(), 1:] = cand_boxes[keep]
    return result


def head_rows(plan) -> List[Tuple[int, int]]:
    """(loc row, conf row) per source map of a `config.ssd300_tables` program: the last twelve rows."""
    n = len(plan)
    return [(n - 12 + 2 * i, n - 12 + 2 * i + 1) for i in range(6)]


def gather_heads(read_layer, plan, q_rows: Dict[int, np.ndarray], batch: int, num_classes: int):
    """Engine outputs -> (loc [B, P, 4], conf [B, P, num_classes]) float32 as SSD.forward builds them
    (SSD.py:62-70: permute(0, 2, 3, 1), flatten, concatenate over the six sources).  read_layer(l) returns the int8
    NCHW output of row l; q_rows[l] is that row's file Q (value = int8 / 2^Q)."""
    import torch
    locs, confs = [], []
    for lrow, crow in head_rows(plan):
        for row, dst in ((lrow, locs), (crow, confs)):
            y = np.asarray(read_layer(row), np.float32) / np.exp2(np.asarray(q_rows[row], np.float32))[None, :, None, None]
            dst.append(torch.from_numpy(y).permute(0, 2, 3, 1).contiguous().view(batch, -1))
    loc = torch.cat(locs, 1).view(batch, -1, 4)
    conf = torch.cat(confs, 1).view(batch, -1, num_classes)
    return loc, conf


def nms_ordered(boxes, scores, overlap: float = 0.45, top_k: int = 200):
    """Greedy NMS in the engine's stated order (the device's, tf2_ssd_detect): candidates by score descending, then index
    ascending (a stable order, unlike nms's torch.sort), the first top_k of them; walking that order, keep the best remaining
    candidate and drop every remaining one whose IoU with it is not <= overlap.  IoU in float32 (_iou_one_to_many), overlap
    rounded to float32 as the device holds it.  Returns the kept indices into `boxes`, best first."""
    import torch
    boxes = torch.as_tensor(boxes, dtype=torch.float32)
    scores = np.asarray(scores, np.float32)
    if scores.size == 0:
        return torch.zeros(0, dtype=torch.long)
    order = np.lexsort((np.arange(scores.size), -scores))[:top_k]        # score descending, index ascending
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    thr = float(np.float32(overlap))
    rest = torch.from_numpy(order)
    kept: List[int] = []
    while rest.numel() > 0:
        best = int(rest[0])
        kept.append(best)
        rest = rest[1:]
        if rest.numel() == 0:
            break
        iou = _iou_one_to_many(boxes[best], area[best], boxes[rest], area[rest])
        rest = rest[iou <= thr]
    return torch.tensor(kept, dtype=torch.long)


def detect_ordered(boxes, probs, num_classes: int, top_k: int = 200, conf_thresh: float = 0.01, nms_thresh: float = 0.45):
    """The host statement of the device's selection (tf2_ssd_detect / the second stage of tf2_ssd_run), its yardstick.
    boxes [B, P, 4] corner form, probs [B, P, num_classes] float32 -> (det [B, num_classes, top_k, 5] float32 rows (score, x1, y1,
    x2, y2), counts [B, num_classes] int32).  Per image and class >= 1:
      candidates   p > conf_thresh (strict, in float32)
      order        score descending, then prior index ascending (an explicit stable order: the reference's nms walks
                   torch.sort's unstable order, which is not defined on ties -- and int8 heads tie often)
      top_k        the first top_k of that order
      suppression  walking the order, keep a candidate unless its IoU with a kept box is not <= nms_thresh (IoU.le, as nms)
    (nms_ordered); IoU is _iou_one_to_many's float32 arithmetic.  Rows best first, zero past counts[b, c]; class 0 stays empty; no cross-class cap."""
    import torch
    boxes = torch.as_tensor(boxes, dtype=torch.float32).detach().cpu().contiguous()
    probs = torch.as_tensor(probs, dtype=torch.float32).detach().cpu().contiguous()
    n_img, n_pri = probs.shape[0], probs.shape[1]
    det = torch.zeros(n_img, num_classes, top_k, 5, dtype=torch.float32)
    counts = torch.zeros(n_img, num_classes, dtype=torch.int32)
    ct = np.float32(conf_thresh)
    idx = np.arange(n_pri)
    for b in range(n_img):
        bx = boxes[b]
        pb = probs[b].numpy()
        for cls in range(1, num_classes):
            p = pb[:, cls]
            cand = idx[p > ct]
            if cand.size == 0:
                continue
            keep = cand[nms_ordered(bx[cand], p[cand], nms_thresh, top_k).numpy()]
            det[b, cls, :keep.size, 0] = torch.from_numpy(p[keep])
            det[b, cls, :keep.size, 1:] = bx[torch.from_numpy(keep)]
            counts[b, cls] = keep.size
    return det, counts


class DeviceDetector:
    """SSD detection on the device (tf2_ssd_*, include/tf2_amd.h) for a `config.ssd300_tables`-style program on `net`
    (a tf2_amd.network.NetWork, packed and bound): the heads are `head_rows(plan)`, the priors `prior_boxes(cfg)`.
      run(images)      one step -- network on the outputs-kept plan, heads -> boxes + probabilities, select + NMS -- enqueued
                       on `stream` (default: the current one).  Returns (det [B, C, top_k, 5], counts [B, C]) and, with
                       decoded=True, also (boxes [B, P, 4], probs [B, P, C]); logits= an int8 device tensor receives the
                       network's logits as Runner.run_batch returns them; mark= a torch.cuda.Event recorded between the
                       network's launches and the detector's.
      detect(b, p)     the selection alone on device boxes [B, P, 4] and probabilities [B, P, C].
    One workspace per batch size is kept; detectors that run side by side on several streams are separate objects."""

    def __init__(self, net, plan, cfg: dict = VOC, top_k: int = 200, conf_thresh: float = 0.01, nms_thresh: float = 0.45):
        import ctypes as C
        from . import _lib
        self.net, self.num_classes, self.top_k = net, int(cfg["num_classes"]), int(top_k)
        self.conf_thresh, self.nms_thresh = conf_thresh, nms_thresh
        pri = np.ascontiguousarray(prior_boxes(cfg).numpy(), np.float32)
        self.n_priors = pri.shape[0]
        rows = head_rows(plan)
        d = _lib.SsdDesc()
        d.size = C.sizeof(_lib.SsdDesc)
        d.num_classes, d.top_k, d.conf_thresh, d.nms_thresh = self.num_classes, self.top_k, conf_thresh, nms_thresh
        d.variance[0], d.variance[1] = cfg["variance"]
        d.n_sources = len(rows)
        for i, (lr, cr) in enumerate(rows):
            d.loc_row[i], d.conf_row[i] = lr, cr
        d.priors, d.n_priors = pri.ctypes.data, self.n_priors
        h = C.c_void_p()
        _lib.check(_lib.lib().tf2_ssd_create(net._h, C.byref(d), C.byref(h)))
        self._h = h
        self._ws = {}
        self._scratch = {}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            from . import _lib
            _lib.lib().tf2_ssd_destroy(h)
            self._h = None

    def workspace_size(self, batch: int) -> int:
        from . import _lib
        return int(_lib.lib().tf2_ssd_workspace_size(self._h, batch))

    def _buffer(self, cache, batch, size):
        import torch
        if batch not in cache:
            cache[batch] = torch.empty(max(size, 256), dtype=torch.uint8, device=self.net.device)
        return cache[batch]

    def run(self, images, stream=None, decoded: bool = False, logits=None, mark=None):
        import torch
        from . import _lib
        assert images.is_contiguous() and images.device == self.net.device and images.dtype in (torch.float32, torch.int8)
        dev, B, C, P = self.net.device, images.shape[0], self.num_classes, self.n_priors
        stream = stream or torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            ws = self._buffer(self._ws, B, self.workspace_size(B))
            det = torch.empty(B, C, self.top_k, 5, dtype=torch.float32, device=dev)
            counts = torch.empty(B, C, dtype=torch.int32, device=dev)
            boxes = torch.empty(B, P, 4, dtype=torch.float32, device=dev) if decoded else None
            probs = torch.empty(B, P, C, dtype=torch.float32, device=dev) if decoded else None
            ptr = lambda t: t.data_ptr() if t is not None else None
            if mark is not None:
                mark.record(stream)             # creates the underlying hipEvent_t; re-recorded by the library
            _lib.check(_lib.lib().tf2_ssd_run(self._h, images.data_ptr(), int(images.dtype == torch.int8), B, ws.data_ptr(), ws.numel(),
                                              det.data_ptr(), counts.data_ptr(), ptr(boxes), ptr(probs), ptr(logits),
                                              mark.cuda_event if mark is not None else None, stream.cuda_stream))
        return (det, counts, boxes, probs) if decoded else (det, counts)

    def detect(self, boxes, probs, stream=None):
        import torch
        from . import _lib
        dev = self.net.device
        boxes = boxes.to(dev, torch.float32).contiguous()
        probs = probs.to(dev, torch.float32).contiguous()
        B, P, C = probs.shape
        assert P == self.n_priors and C == self.num_classes and tuple(boxes.shape) == (B, P, 4)
        stream = stream or torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            scratch = self._buffer(self._scratch, B, int(_lib.lib().tf2_ssd_detect_scratch_size(self._h, B)))
            det = torch.empty(B, C, self.top_k, 5, dtype=torch.float32, device=dev)
            counts = torch.empty(B, C, dtype=torch.int32, device=dev)
            _lib.check(_lib.lib().tf2_ssd_detect(self._h, boxes.data_ptr(), probs.data_ptr(), B, scratch.data_ptr(), scratch.numel(),
                                                 det.data_ptr(), counts.data_ptr(), stream.cuda_stream))
        return det, counts

    def poll_error(self, batch: int, stream=None) -> None:
        """tf2_net_poll_error on this detector's workspace of `batch` images (synchronises the stream)."""
        import torch
        from . import _lib
        ws = self._ws[batch]
        stream = stream or torch.cuda.current_stream(self.net.device)
        _lib.check(_lib.lib().tf2_net_poll_error(self.net._h, batch, ws.data_ptr(), ws.numel(), stream.cuda_stream))


# ---- detection accuracy: ground-truth matching and VOC mAP (tf2_det_eval_*, include/tf2_amd.h; csrc/ssd_eval.hip) ----------------
# The reference ships no evaluation code, so the statement below is the canonical one: the PASCAL VOC devkit protocol behind the
# README's mAP, with plain IoU on normalised coordinates (no "+1 pixel") and the devkit's undefined tie order pinned.

GT_DTYPE = np.dtype([("box", np.float32, 4), ("label", np.int32), ("difficult", np.int32)])       # tf2_gt_box, 24 bytes
EVAL_BAD_SLOT, EVAL_BAD_COUNT, EVAL_BAD_LABEL, EVAL_BAD_BOX, EVAL_BAD_DET = 1, 2, 4, 8, 16       # TF2_EVAL_*


def pack_ground_truth(per_image, max_gt: int):
    """Per-image ground truth -> the padded records of tf2_det_eval_run: (gt [B, max_gt] of GT_DTYPE, gt_count [B] int32).  An image
    is an array [n, 6] of rows (x1, y1, x2, y2, label, difficult) in the normalised corner form of `det` (or a GT_DTYPE array [n]);
    n = 0 is an image without objects."""
    gt = np.zeros((len(per_image), max_gt), GT_DTYPE)
    cnt = np.zeros(len(per_image), np.int32)
    for b, rows in enumerate(per_image):
        rows = np.asarray(rows)
        if rows.dtype != GT_DTYPE:
            rows = rows.reshape(-1, 6)
            rec = np.zeros(rows.shape[0], GT_DTYPE)
            rec["box"], rec["label"], rec["difficult"] = rows[:, :4], rows[:, 4], rows[:, 5]
            rows = rec
        if rows.shape[0] > max_gt:
            raise ValueError(f"image {b} has {rows.shape[0]} ground truths, max_gt is {max_gt}")
        gt[b, :rows.shape[0]] = rows
        cnt[b] = rows.shape[0]
    return gt, cnt


def _gt_records(gt):
    """GT_DTYPE view [B, max_gt] of ground-truth records given as such, or as their int32 words [B, max_gt, 6] (numpy / torch)"""
    if hasattr(gt, "detach"):
        gt = gt.detach().cpu().numpy()
    gt = np.ascontiguousarray(gt)
    return gt if gt.dtype == GT_DTYPE else gt.view(GT_DTYPE).reshape(gt.shape[0], gt.shape[1])


def _host(a, dtype):
    return np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype)


class MatchResult:
    """flags int8 [B, C, K], scores float32 [B, C, K], npos int32 [B, C], status int32 [B]; duplicates int32 [B, C]: the rows among
    the flag-0 ones whose winner passed the threshold but was taken (what the device does not record: for tests' censuses)"""

    def __init__(self, flags, scores, npos, status, duplicates):
        self.flags, self.scores, self.npos, self.status, self.duplicates = flags, scores, npos, status, duplicates


def match_reference(det, counts, gt, gt_count, iou_thresh: float = 0.5, slots=None, capacity=None) -> MatchResult:
    """The host statement of tf2_det_eval_run's kernel, its yardstick, per image: det [B, C, K, 5] rows (score, x1, y1, x2, y2) best
    first, counts [B, C], gt [B, max_gt] records (pack_ground_truth), gt_count [B].  Per image and class c >= 1, for row r = 0 ..
    counts-1: among the image's ground truths of class c in index order (difficult ones included) the one with the largest IoU,
    strict '>' from none (the lowest index wins a tie, a NaN IoU never wins); flag 0 if there is none or its IoU is not >
    iou_thresh (float32, strict), -1 if it is difficult, 1 if it is not yet taken (it is taken now), 0 if it is (a duplicate: no
    fall-back to the second best).  Rows past counts and all of class 0: flag -2, score 0.  npos[b, c] = non-difficult ground truths.
    IoU is _iou_one_to_many's float32 arithmetic, inter / ((area_gt - inter) + area_det), with the device's min / max (a NaN operand
    is ignored: np.fmax / np.fmin; the same values for every non-NaN box).
    status[b] is 0 or an OR of EVAL_BAD_*: gt_count outside 0..max_gt (labels and boxes are then not looked at), a label outside
    1..C-1, a non-finite or inverted box, a count outside 0..K, and, with `slots` / `capacity`, a slot >= capacity; slot < 0 skips the
    image (status 0).  A skipped or malformed image has flag -2 everywhere, scores and npos 0."""
    det, counts = _host(det, np.float32), _host(counts, np.int32)
    gt, gt_count = _gt_records(gt), _host(gt_count, np.int32)
    B, C, K = det.shape[:3]
    max_gt = gt.shape[1]
    thr = np.float32(iou_thresh)
    flags = np.full((B, C, K), -2, np.int8)
    scores = np.zeros((B, C, K), np.float32)
    npos = np.zeros((B, C), np.int32)
    status = np.zeros(B, np.int32)
    duplicates = np.zeros((B, C), np.int32)
    for b in range(B):
        if slots is not None:
            if int(slots[b]) < 0:
                continue
            if capacity is not None and int(slots[b]) >= capacity:
                status[b] |= EVAL_BAD_SLOT
        n_gt = int(gt_count[b])
        if n_gt < 0 or n_gt > max_gt:
            status[b] |= EVAL_BAD_COUNT
            n_gt = 0
        g = gt[b, :n_gt]
        box, label, difficult = g["box"], g["label"], g["difficult"] != 0
        if ((label < 1) | (label >= C)).any():
            status[b] |= EVAL_BAD_LABEL
        if (~np.isfinite(box).all(axis=1) | (box[:, 2] < box[:, 0]) | (box[:, 3] < box[:, 1])).any():
            status[b] |= EVAL_BAD_BOX
        if ((counts[b] < 0) | (counts[b] > K)).any():
            status[b] |= EVAL_BAD_DET
        if status[b]:
            continue
        area_gt = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
        for c in range(1, C):
            n = int(counts[b, c])
            of_c = np.flatnonzero(label == c)
            npos[b, c] = int((~difficult[of_c]).sum())
            flags[b, c, :n] = 0
            scores[b, c, :n] = det[b, c, :n, 0]
            if n == 0 or of_c.size == 0:
                continue
            d = det[b, c, :n, 1:]
            area_det = (d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1])
            gb = box[of_c]
            lo_x, lo_y = np.fmax(gb[None, :, 0], d[:, None, 0]), np.fmax(gb[None, :, 1], d[:, None, 1])
            hi_x, hi_y = np.fmin(gb[None, :, 2], d[:, None, 2]), np.fmin(gb[None, :, 3], d[:, None, 3])
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                inter = np.fmax(hi_x - lo_x, np.float32(0)) * np.fmax(hi_y - lo_y, np.float32(0))
                iou = inter / ((area_gt[of_c][None, :] - inter) + area_det[:, None])          # [rows, ground truths of c]
            assert iou.dtype == np.float32
            iou = np.where(np.isnan(iou), -np.inf, iou)
            win = iou.argmax(axis=1)                                                          # the first of the largest
            best = iou[np.arange(n), win]
            taken = np.zeros(of_c.size, bool)
            for r in range(n):
                if not best[r] > thr:
                    continue
                w = win[r]
                if difficult[of_c[w]]:
                    flags[b, c, r] = -1
                elif not taken[w]:
                    flags[b, c, r] = 1
                    taken[w] = True
                else:
                    duplicates[b, c] += 1
    return MatchResult(flags, scores, npos, status, duplicates)


def voc_ap(rec, prec, use_07_metric: bool = False) -> float:
    """The devkit's voc_ap: the 11-point metric (maximum precision at recall >= k * 0.1, k = 0..10, 0 where there is none, their
    mean) or the all-point one (recall bracketed by 0 and 1, the monotone precision envelope from the right, sum of delta recall x
    precision), in float64."""
    rec, prec = np.asarray(rec, np.float64), np.asarray(prec, np.float64)
    if use_07_metric:
        ap = 0.0
        for k in range(11):
            t = k * 0.1
            p = float(prec[rec >= t].max()) if (rec >= t).any() else 0.0
            ap += p / 11.0
        return ap
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = max(mpre[i - 1], mpre[i])
    i = np.flatnonzero(mrec[1:] != mrec[:-1])
    return float(((mrec[i + 1] - mrec[i]) * mpre[i + 1]).sum())


def voc_eval_reference(det, counts, gt, gt_count, image_ids=None, iou_thresh: float = 0.5, use_07_metric: bool = False) -> dict:
    """The same protocol written independently of match_reference, in the devkit's global form (voc_eval): per class, every image's
    detections in ONE list, sorted by (score descending, image id ascending, rank ascending -- the pinned order), walked once with
    per-image taken flags, then voc_ap.  Within one image the global order restricted to that image is the row order (rows are best
    first and ties keep the rank order), so per-image matching is the same protocol; tests/test_ssd_eval.py shows the two agree.
    image_ids [B]: the images' positions in the dataset (the evaluator's slots; default 0..B-1), ids < 0 are left out.
    Returns dict(ap [C] (NaN where npos == 0), npos, tp, fp [C], images, map: the mean AP over classes with npos > 0)."""
    det, counts = _host(det, np.float32), _host(counts, np.int32)
    gt, gt_count = _gt_records(gt), _host(gt_count, np.int32)
    B, C, K = det.shape[:3]
    ids = np.arange(B) if image_ids is None else np.asarray(image_ids, np.int64)
    thr = np.float32(iou_thresh)
    ap = np.full(C, np.nan)
    npos, tps, fps = np.zeros(C, np.int64), np.zeros(C, np.int64), np.zeros(C, np.int64)
    use = [b for b in range(B) if ids[b] >= 0]
    for c in range(1, C):
        class_recs = {}
        for b in use:
            g = gt[b, :gt_count[b]]
            g = g[g["label"] == c]
            class_recs[b] = dict(bbox=g["box"], difficult=g["difficult"] != 0, det=np.zeros(g.size, bool))
            npos[c] += int((g["difficult"] == 0).sum())
        img = np.concatenate([np.full(counts[b, c], b, np.int64) for b in use] + [np.zeros(0, np.int64)])
        rank = np.concatenate([np.arange(counts[b, c]) for b in use] + [np.zeros(0, np.int64)])
        conf = np.concatenate([det[b, c, :counts[b, c], 0] for b in use] + [np.zeros(0, np.float32)])
        bbs = np.concatenate([det[b, c, :counts[b, c], 1:] for b in use] + [np.zeros((0, 4), np.float32)])
        order = np.lexsort((rank, ids[img], -conf.astype(np.float64)))
        tp, fp = np.zeros(order.size), np.zeros(order.size)
        for at, d in enumerate(order):
            R = class_recs[int(img[d])]
            bb, BBGT = bbs[d], R["bbox"]
            ovmax, jmax = -np.inf, -1
            if BBGT.shape[0] > 0:
                ixmin, iymin = np.fmax(BBGT[:, 0], bb[0]), np.fmax(BBGT[:, 1], bb[1])
                ixmax, iymax = np.fmin(BBGT[:, 2], bb[2]), np.fmin(BBGT[:, 3], bb[3])
                iw, ih = np.fmax(ixmax - ixmin, np.float32(0)), np.fmax(iymax - iymin, np.float32(0))
                inters = iw * ih
                with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                    uni = ((BBGT[:, 2] - BBGT[:, 0]) * (BBGT[:, 3] - BBGT[:, 1]) - inters) + (bb[2] - bb[0]) * (bb[3] - bb[1])
                    overlaps = inters / uni
                overlaps = np.where(np.isnan(overlaps), -np.inf, overlaps)
                ovmax, jmax = overlaps.max(), int(overlaps.argmax())
            if ovmax > thr:
                if not R["difficult"][jmax]:
                    if not R["det"][jmax]:
                        tp[at] = 1.0
                        R["det"][jmax] = True
                    else:
                        fp[at] = 1.0
            else:
                fp[at] = 1.0
        tps[c], fps[c] = int(tp.sum()), int(fp.sum())
        if npos[c] == 0:
            continue
        ctp, cfp = np.cumsum(tp), np.cumsum(fp)
        keep = (tp + fp) > 0                                  # ignored rows are no points of the curve
        rec = ctp[keep] / float(npos[c])
        prec = ctp[keep] / np.maximum(ctp[keep] + cfp[keep], np.finfo(np.float64).eps)
        ap[c] = voc_ap(rec, prec, use_07_metric)
    have = npos > 0
    return dict(ap=ap, npos=npos, tp=tps, fp=fps, images=len(use), map=float(ap[have].mean()) if have.any() else float("nan"))


def _summarise(h, store: np.ndarray, num_classes: int, use_07_metric: bool) -> dict:
    import ctypes as C
    from . import _lib
    per = (_lib.DetEvalClass * num_classes)()
    images, mean = C.c_int64(), C.c_double()
    _lib.check(_lib.lib().tf2_det_eval_summarise(h, store.ctypes.data, store.size, int(bool(use_07_metric)), per, C.byref(images),
                                                 C.byref(mean)))
    return dict(ap=np.array([p.ap for p in per]), npos=np.array([p.npos for p in per], np.int64),
                tp=np.array([p.tp for p in per], np.int64), fp=np.array([p.fp for p in per], np.int64), images=int(images.value),
                map=float(mean.value))


class EvalHandle:
    """A tf2_det_eval handle (host constants only: usable without a device) and the layout of its store."""

    def __init__(self, num_classes: int, top_k: int, capacity: int, max_gt: int = 64, iou_thresh: float = 0.5):
        import ctypes as C
        from . import _lib
        self.num_classes, self.top_k, self.capacity, self.max_gt, self.iou_thresh = num_classes, top_k, capacity, max_gt, iou_thresh
        d = _lib.DetEvalDesc(C.sizeof(_lib.DetEvalDesc), num_classes, top_k, max_gt, capacity, iou_thresh)
        h = C.c_void_p()
        _lib.check(_lib.lib().tf2_det_eval_create(C.byref(d), C.byref(h)))
        self._h, self._destroy = h, _lib.lib().tf2_det_eval_destroy
        self.store_size = int(_lib.lib().tf2_det_eval_store_size(h))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._destroy(h)
            self._h = None

    def views(self, store: np.ndarray) -> dict:
        """seen [cap], npos [cap, C], scores [cap, C, K], flags [cap, C, K] of a host copy of the store (uint8 [store_size])"""
        cap, C, K = self.capacity, self.num_classes, self.top_k
        o1, o2, o3 = cap * 4, cap * 4 * (1 + C), cap * 4 * (1 + C + C * K)
        return dict(seen=store[:o1].view(np.int32), npos=store[o1:o2].view(np.int32).reshape(cap, C),
                    scores=store[o2:o3].view(np.float32).reshape(cap, C, K), flags=store[o3:o3 + cap * C * K].view(np.int8).reshape(cap, C, K))

    def store_from(self, matches, slots) -> np.ndarray:
        """the host image of a store that holds MatchResult(s) `matches` at `slots` (what the device leaves; unwritten bytes zero)"""
        store = np.zeros(self.store_size, np.uint8)
        v = self.views(store)
        for m, sl in zip(matches, slots):
            for b, s in enumerate(np.asarray(sl)):
                if s >= 0 and m.status[b] == 0:
                    v["seen"][s] = 1
                    v["npos"][s], v["scores"][s], v["flags"][s] = m.npos[b], m.scores[b], m.flags[b]
        return store

    def summarise(self, store: np.ndarray, use_07_metric: bool = False) -> dict:
        """tf2_det_eval_summarise on a host copy of the store: dict(ap, npos, tp, fp [C], images, map)"""
        store = np.ascontiguousarray(store, np.uint8)
        return _summarise(self._h, store, self.num_classes, use_07_metric)


class DeviceEvaluator(EvalHandle):
    """Detection accuracy on the device (tf2_det_eval_*, include/tf2_amd.h): the store of `capacity` image slots lives on `device`.
      update(det, counts, gt, gt_count, slots)   one step behind DeviceDetector.run / .detect on `stream` (default: the current one):
                       det / counts as the detector returns them, gt int32 [B, max_gt, 6] (the words of pack_ground_truth's records;
                       a numpy record array is copied to the device), gt_count and slots int32 [B]; slots[b] is the image's place in
                       the dataset, < 0 skips it.  Returns status int32 [B] on the device (0, or EVAL_BAD_* bits: the image was
                       left out); flags=True returns (status, flags int8 [B, C, K]) as well.  No allocation happens inside a captured
                       graph if status= (and flags_out=) are passed.
      reset()          a new epoch: `seen` is zeroed, nothing else needs to be.
      result()         one copy of the store to the host, then tf2_det_eval_summarise: dict(ap, npos, tp, fp [C], images, map)."""

    def __init__(self, num_classes: int, top_k: int, capacity: int, max_gt: int = 64, iou_thresh: float = 0.5, device="cuda:0"):
        import torch
        super().__init__(num_classes, top_k, capacity, max_gt, iou_thresh)
        self.device = torch.device(device)
        self.store = torch.empty(self.store_size, dtype=torch.uint8, device=self.device)
        self.reset()

    def _dev(self, a, shape):
        import torch
        if not hasattr(a, "data_ptr"):
            a = np.ascontiguousarray(a)
            a = torch.from_numpy(a.view(np.int32).reshape(shape) if a.dtype == GT_DTYPE else a.astype(np.int32).reshape(shape))
        a = a.to(self.device)
        assert a.dtype == torch.int32 and a.is_contiguous() and tuple(a.shape) == shape, (a.dtype, tuple(a.shape), shape)
        return a

    def reset(self, stream=None) -> None:
        import torch
        from . import _lib
        stream = stream or torch.cuda.current_stream(self.device)
        _lib.check(_lib.lib().tf2_det_eval_store_init(self._h, self.store.data_ptr(), self.store.numel(), stream.cuda_stream))

    def update(self, det, counts, gt, gt_count, slots, stream=None, flags: bool = False, status=None, flags_out=None):
        import torch
        from . import _lib
        B, C, K = det.shape[0], self.num_classes, self.top_k
        assert tuple(det.shape) == (B, C, K, 5) and det.dtype == torch.float32 and det.is_contiguous() and det.device == self.device
        assert tuple(counts.shape) == (B, C) and counts.dtype == torch.int32 and counts.is_contiguous() and counts.device == self.device
        stream = stream or torch.cuda.current_stream(self.device)
        with torch.cuda.stream(stream):
            gt, gt_count, slots = self._dev(gt, (B, self.max_gt, 6)), self._dev(gt_count, (B,)), self._dev(slots, (B,))
            if status is None:
                status = torch.empty(B, dtype=torch.int32, device=self.device)
            if flags and flags_out is None:
                flags_out = torch.empty(B, C, K, dtype=torch.int8, device=self.device)
            _lib.check(_lib.lib().tf2_det_eval_run(self._h, det.data_ptr(), counts.data_ptr(), gt.data_ptr(), gt_count.data_ptr(),
                                                   slots.data_ptr(), B, self.store.data_ptr(), self.store.numel(), status.data_ptr(),
                                                   flags_out.data_ptr() if flags_out is not None else None, stream.cuda_stream))
        return (status, flags_out) if flags else status

    def store_host(self) -> np.ndarray:
        return self.store.cpu().numpy()

    def result(self, use_07_metric: bool = False) -> dict:
        return self.summarise(self.store_host(), use_07_metric)
