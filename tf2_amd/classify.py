"""Classification on the device (tf2_cls_*, include/tf2_amd.h; csrc/classify.hip): the int8 logits [B, n] of a run in, top-k
labels and features with Evaluation's tie rule (network_helper.cpp:143-207), softmax probabilities, the rank of a ground-truth
label and running top-1 / top-k tallies out.

`reference` is the one host statement of the arithmetic and the yardstick of the device.  Per image, with the runtime Q row of the
last layer's output (the row tf2_topk's callers pass, q[NUM_LAYER]; sh[i] = -q[i] in 0..30):
  features        f[i] = float32(logit[i]) / float32(1 << sh[i])                                      (exact)
  top-k           the first k entries by (feature descending, index descending on equal features): the closed form of the
                  reference's k bubble passes with a strict '>' (tests/test_classify.py holds it against tf2_topk)
  probabilities   d[i] = f[i] - max(f) as ONE float32 subtraction, p[i] = exp(d[i]) / sum_j exp(d[j]); the statement evaluates
                  exp and the sum in float64 on the float32 d, the device in float32 with a fixed summation order.  The
                  reference's text (network.Evaluation keeps it) does not subtract the maximum: exp overflows float32 once a
                  feature passes ~88 and the result is inf / inf; mathematically the two agree.
  rank, tally     truth < 0: unlabelled, rank -1, not counted; 0 <= truth < n: rank = position of the label among the top k
                  (0 = best) or -1; truth >= n: a bad label, rank -1.  tally = [images with truth >= 0 (bad labels included:
                  they are misses), rank == 0, rank >= 0, bad labels].

`DeviceClassifier(net, top_k)` runs the device path on the logits tensor Runner.run_batch returns."""
import ctypes as C
from typing import NamedTuple, Optional

import numpy as np

MAX_N, MAX_TOP_K = 4096, 64          # kClsMaxN, kClsMaxTopK (csrc/classify.h)


class Result(NamedTuple):
    labels: object                   # int32 [B, k]
    features: object                 # float32 [B, k]
    probs: object                    # [B, k]: float64 from `reference`, float32 from the device
    all_probs: object                # [B, n] (the device: None unless asked for)
    rank: object                     # int32 [B] (None without truth)
    tally: object                    # [4]: this call's counts from `reference`; the classifier's running tally from the device


def features_of(logits, q_last) -> np.ndarray:
    """float32 [B, n]: logit / (1 << sh), sh = -q_last (the runtime row) in 0..30"""
    logits = np.asarray(logits, np.int8)
    logits = logits.reshape(-1, logits.shape[-1])
    n = logits.shape[1]
    sh = -np.asarray(q_last).reshape(-1)[:n].astype(np.int64)
    if sh.size != n:
        raise ValueError(f"q row has {sh.size} channels, the output {n}")
    if (sh < 0).any() or (sh > 30).any():
        raise ValueError("Q of the last layer must be in 0..30 (network_helper.cpp:181)")
    return logits.astype(np.float32) / (np.int64(1) << sh).astype(np.float32)[None, :]


def reference(logits, q_last, top_k: int, truth=None) -> Result:
    """The statement on int8 logits [B, n] (or [n]) and the runtime Q row q_last; truth: int [B] or None"""
    f = features_of(logits, q_last)
    B, n = f.shape
    if not 1 <= top_k <= n:
        raise ValueError(f"top_k must be in 1..{n}")
    idx = np.broadcast_to(np.arange(n, dtype=np.int64), (B, n))
    order = np.lexsort((-idx, -f.astype(np.float64)), axis=-1)[:, :top_k]          # feature descending, then index descending
    labels = order.astype(np.int32)
    feats = np.take_along_axis(f, order, axis=1)
    d = (f - f.max(axis=1, keepdims=True)).astype(np.float32)                     # one float32 rounding
    e = np.exp(d.astype(np.float64))
    all_probs = e / e.sum(axis=1, keepdims=True)
    probs = np.take_along_axis(all_probs, order, axis=1)
    rank, tally = None, np.zeros(4, np.uint64)
    if truth is not None:
        t = np.asarray(truth).reshape(B).astype(np.int64)
        hit = labels.astype(np.int64) == t[:, None]
        rank = np.where(hit.any(axis=1) & (t >= 0) & (t < n), hit.argmax(axis=1), -1).astype(np.int32)
        tally[:] = [(t >= 0).sum(), (rank == 0).sum(), (rank >= 0).sum(), (t >= n).sum()]
    return Result(labels, feats, probs, all_probs, rank, tally)


class DeviceClassifier:
    """tf2_cls_* for `net` (a tf2_amd.network.NetWork with its q table set and a 1 x 1 final map).
      run(logits, truth=None, all_probs=False, stream=None) -> Result of device tensors
    logits: the int8 device tensor [B, n] Runner.run_batch returns; truth: an int32 device tensor [B] (refill it between the replays
    of a captured graph).  Enqueued on `stream` (default: the current one); nothing synchronises.  With truth the counts are added
    to `self.tally` (int64 [4] on the device: labelled, top-1 hits, top-k hits, bad labels) -- it keeps accumulating over runs and
    graph replays until reset().  accuracy() is the only method that synchronises.  Classifiers that tally side by side on several
    streams may share one object (integer atomics) or be separate objects with their own tallies."""

    def __init__(self, net, top_k: int = 5):
        from . import _lib
        self.net, self.top_k, self.n = net, int(top_k), int(net.plan[-1].N)
        d = _lib.ClsDesc(C.sizeof(_lib.ClsDesc), self.top_k)
        h = C.c_void_p()
        _lib.check(_lib.lib().tf2_cls_create(net._h, C.byref(d), C.byref(h)))
        self._h = h
        self.tally = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            from . import _lib
            _lib.lib().tf2_cls_destroy(h)
            self._h = None

    def _tally(self, dev):
        import torch
        if self.tally is None:
            self.tally = torch.zeros(4, dtype=torch.int64, device=dev)
        return self.tally

    def run(self, logits, truth=None, all_probs: bool = False, stream=None) -> Result:
        import torch
        from . import _lib
        dev = logits.device
        assert logits.dtype == torch.int8 and logits.is_contiguous() and dev.type == "cuda" and logits.dim() == 2 and logits.shape[1] == self.n
        B, k = logits.shape[0], self.top_k
        if truth is not None:
            assert truth.dtype == torch.int32 and truth.is_contiguous() and truth.device == dev and tuple(truth.shape) == (B,)
            self._tally(dev)                                      # (allocated and zeroed outside the enqueue below)
        stream = stream or torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            labels = torch.empty(B, k, dtype=torch.int32, device=dev)
            feats = torch.empty(B, k, dtype=torch.float32, device=dev)
            probs = torch.empty(B, k, dtype=torch.float32, device=dev)
            allp = torch.empty(B, self.n, dtype=torch.float32, device=dev) if all_probs else None
            rank = torch.empty(B, dtype=torch.int32, device=dev) if truth is not None else None
            ptr = lambda t: t.data_ptr() if t is not None else None
            _lib.check(_lib.lib().tf2_cls_run(self._h, logits.data_ptr(), B, labels.data_ptr(), feats.data_ptr(), probs.data_ptr(), ptr(allp),
                                              ptr(truth), ptr(rank), ptr(self.tally) if truth is not None else None, stream.cuda_stream))
        return Result(labels, feats, probs, allp, rank, self.tally)

    def reset(self, stream=None):
        """zero the running tally (enqueued on `stream`, default the current one)"""
        import torch
        if self.tally is not None:
            with torch.cuda.stream(stream or torch.cuda.current_stream(self.tally.device)):
                self.tally.zero_()

    def accuracy(self) -> dict:
        """{labelled, bad, top1, topk}: the running counts and the top-1 / top-k fractions of the labelled images (None before any).
        Synchronises the device."""
        import torch
        if self.tally is None:
            return dict(labelled=0, bad=0, top1=None, topk=None)
        torch.cuda.synchronize(self.tally.device)
        n, h1, hk, bad = (int(v) for v in self.tally.cpu().tolist())
        return dict(labelled=n, bad=bad, top1=h1 / n if n else None, topk=hk / n if n else None)

    def reference(self, logits, truth=None) -> Result:
        """The statement on host copies of the same inputs, with the net's last Q row"""
        lg = logits.cpu().numpy() if hasattr(logits, "cpu") else np.asarray(logits)
        tr = truth.cpu().numpy() if hasattr(truth, "cpu") else truth
        return reference(lg, self.net.q[self.net.num_layer], self.top_k, tr)
