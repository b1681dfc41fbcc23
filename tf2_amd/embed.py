"""Face matching on the device (tf2_emb_*, include/tf2_amd.h; csrc/embed_match.hip): the int8 outputs [B, D] of an embedding network
(SqueezeNet 1.1 with its 1000 -> 128 row: D = 128) in, unit embeddings, the k nearest rows of a float32 gallery [N, D] and running
accept / identify tallies out -- the 1:N search of a feature library the reference's face demo does in closed binaries.

The reference gives no program text for the matching, so the three functions below ARE the statement and the yardstick of the
device; all arithmetic is float32, every operation rounded separately (no fused multiply-add), every sum taken for c ascending:
  reference_embed  f[c] = float32(out[c]) / float32(1 << sh[c]), sh = -q_last_row in 0..30 (classify.features_of: exact);
                   s = sum_c f[c] * f[c] from 0.0f;  e[c] = f[c] / sqrt(s);  s == 0 gives the zero vector, with no division
  reference_match  d(b, n) = sum_c (e[b, c] - g[n, c])^2 from 0.0f; a NaN distance (a caller's gallery row only) counts and is
                   reported as +inf; the first k rows by (distance ascending, row index ascending); slots past N read idx -1,
                   dist +inf, id -1; id = ids[idx], or idx without ids
  reference_tally  truth[b] < 0: unlabelled, nothing counted; else [labelled, id[b, 0] == truth, any of the k ids == truth,
                   true accepts: dist[b, 0] < threshold and id[b, 0] == truth, false accepts: dist[b, 0] < threshold and
                   id[b, 0] != truth] -- a strict float32 '<'; a truth no gallery row carries is an impostor: it can only be
                   rejected or falsely accepted

`DeviceMatcher(net, top_k)` runs the device path on the int8 tensor Runner.run_batch returns; `Gallery` holds the rows.

Where the matcher's `threshold` comes from (tf2_emb_roc_*; csrc/embed_roc.hip): the genuine and impostor distance histograms of a
labelled set, with the matcher's own distances and its own strict '<', again stated here and bit-identical on the device:
  roc_thresholds      thr[t] = float32(t + 1) * float32(step), t < T;  roc_bin: bin(d) = #{t : thr[t] <= d} in 0..T, NaN as +inf;
                      a pair is accepted at threshold t iff d < thr[t] iff bin(d) <= t
  reference_roc_hist  hist[same][bin] over all pairs i < j of one labelled set, or all (i, j) of two; ids < 0 take no part
  reference_pairs     listed pairs (a, b, same, fold): their distances and per-fold histograms; invalid pairs counted, dist -1
  roc_summary         TA / FA / TAR / FAR per threshold, best accuracy, EER, the threshold for each FAR target (tie rules there)
  fold_protocol       the LFW ten-fold accuracy from per-fold histograms
`DeviceRoc(n_thr, step, n_folds)` runs the device path and keeps the histograms on the device."""
import ctypes as C
from typing import NamedTuple

import numpy as np

from .classify import features_of

MAX_D, MAX_TOP_K = 512, 16           # kEmbMaxD, kEmbMaxTopK (csrc/embed_match.h)
SLAB, GROUP = 64, 32                 # kEmbSlab, kEmbGroup: gallery rows and queries of one stage-1 block
TALLY = ("labelled", "identified", "among_k", "true_accepts", "false_accepts")
ROC_MAX_THR, ROC_MAX_FOLDS = 4096, 16  # kRocMaxThr, kRocMaxFolds (csrc/embed_roc.h)
ROC_TILE = 256                       # kRocTile: rows of one block's tile on either side of the all-pairs kernel
FAR_TARGETS = (1e-1, 1e-2, 1e-3, 1e-4, 1e-5)


class Result(NamedTuple):
    idx: object                      # int32 [B, k]: gallery rows, nearest first (-1 past N)
    dist: object                     # float32 [B, k]: squared distances (+inf past N)
    ids: object                      # int32 [B, k]: the rows' ids (-1 past N)
    embeddings: object               # float32 [B, D]: the queries' unit embeddings


def reference_embed(out_i8, q_last_row) -> np.ndarray:
    """float32 [B, D]: the unit embeddings of int8 outputs [B, D] (or [D]) under the runtime Q row of the last layer's output"""
    f = features_of(out_i8, q_last_row)
    B, D = f.shape
    s = np.zeros(B, np.float32)
    for c in range(D):
        s = s + f[:, c] * f[:, c]                                  # float32 product, float32 sum: two roundings
    norm = np.sqrt(s)
    e = np.zeros((B, D), np.float32)
    nz = s != 0
    e[nz] = f[nz] / norm[nz, None]
    return e


def _distances(e, g) -> np.ndarray:
    """float32 [B, N]: THE distance loop of the statement, d(b, n) of float32 e [B, D] and g [N, D]; NaN reads +inf"""
    d = np.zeros((e.shape[0], g.shape[0]), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(e.shape[1]):
            t = e[:, c, None] - g[None, :, c]
            d = d + t * t
    return np.where(np.isnan(d), np.float32(np.inf), d)


def reference_match(e, gallery, ids=None, top_k: int = 1):
    """(idx int32 [B, k], dist float32 [B, k], id int32 [B, k]) of embeddings e [B, D] against gallery [N, D]"""
    e = np.asarray(e, np.float32)
    g = np.asarray(gallery, np.float32)
    e = e.reshape(-1, e.shape[-1])
    B, D = e.shape
    N = g.shape[0]
    if g.ndim != 2 or g.shape[1] != D or N < 1:
        raise ValueError(f"gallery must be [N >= 1, {D}]")
    if top_k < 1:
        raise ValueError("top_k must be >= 1")
    d = _distances(e, g)
    rows = np.broadcast_to(np.arange(N, dtype=np.int64), (B, N))
    order = np.lexsort((rows, d), axis=-1)[:, :top_k]              # distance ascending, then row index ascending
    k = order.shape[1]
    idx = np.full((B, top_k), -1, np.int32)
    dist = np.full((B, top_k), np.inf, np.float32)
    idx[:, :k] = order
    dist[:, :k] = np.take_along_axis(d, order, axis=1)
    out_ids = idx.copy()
    if ids is not None:
        ids = np.asarray(ids).reshape(-1).astype(np.int32)
        if ids.size < N:
            raise ValueError("ids has fewer entries than the gallery rows")
        out_ids[:, :k] = ids[order]
    return idx, dist, out_ids


def reference_tally(idx, dist, ids, truth, threshold) -> np.ndarray:
    """uint64 [5]: this call's counts (TALLY names them)"""
    ids = np.asarray(ids).astype(np.int64)
    t = np.asarray(truth).reshape(ids.shape[0]).astype(np.int64)
    lab = t >= 0
    first = ids[:, 0] == t
    accept = np.asarray(dist, np.float32)[:, 0] < np.float32(threshold)
    among = (ids == t[:, None]).any(axis=1)
    return np.array([lab.sum(), (lab & first).sum(), (lab & among).sum(), (lab & accept & first).sum(),
                     (lab & accept & ~first).sum()], np.uint64)


def roc_thresholds(n_thr: int = 400, step: float = 0.01) -> np.ndarray:
    """float32 [T]: the threshold grid thr[t] = float32(t + 1) * float32(step), one float32 multiply each; T in 1..4096, step
    (as a float32) finite and > 0.  FaceNet's arange(0, 4, 0.01) on squared distances is T = 400, step = 0.01."""
    n_thr, s = int(n_thr), np.float32(step)
    if not 1 <= n_thr <= ROC_MAX_THR:
        raise ValueError(f"n_thr must be in 1..{ROC_MAX_THR}")
    if not (np.isfinite(s) and s > 0):
        raise ValueError("step must be finite and > 0 as a float32")
    return np.arange(1, n_thr + 1, dtype=np.float32) * s


def roc_bin(d, thr) -> np.ndarray:
    """bin(d) = #{t : thr[t] <= d} in 0..T of float32 distances (any shape); a NaN distance counts as +inf (bin T).  A pair is
    accepted at threshold t iff d < thr[t] iff bin(d) <= t: reference_tally's strict '<'."""
    d = np.asarray(d, np.float32)
    d = np.where(np.isnan(d), np.float32(np.inf), d)
    return np.searchsorted(np.asarray(thr, np.float32), d, side="right")


def _labelled(rows, ids, D=None):
    rows = np.asarray(rows, np.float32)
    if rows.ndim != 2 or rows.shape[0] < 1 or (D is not None and rows.shape[1] != D):
        raise ValueError("rows must be float32 [n >= 1, D]")
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    if ids.size != rows.shape[0]:
        raise ValueError("one id a row")
    return rows, ids


def reference_roc_hist(rows_a, ids_a, rows_b=None, ids_b=None, n_thr: int = 400, step: float = 0.01) -> np.ndarray:
    """int64 [2][T + 1]: hist[same][bin] over the pairs of labelled rows, same = (ids_a[i] == ids_b[j]), the distance exactly
    reference_match's.  Self mode (rows_b is None): every pair i < j of one set; cross mode: every (i, j).  A row whose id is < 0
    takes part in no pair."""
    thr = roc_thresholds(n_thr, step)
    a, ia = _labelled(rows_a, ids_a)
    self_mode = rows_b is None
    b, ib = (a, ia) if self_mode else _labelled(rows_b, ids_b, a.shape[1])
    hist = np.zeros((2, n_thr + 1), np.int64)
    cols = np.arange(b.shape[0])
    for i0 in range(0, a.shape[0], 256):                                # (256 rows of the matrix at a time: memory only)
        sl = slice(i0, min(i0 + 256, a.shape[0]))
        bins = roc_bin(_distances(a[sl], b), thr)
        ok = (ia[sl, None] >= 0) & (ib[None, :] >= 0)
        if self_mode:
            ok &= np.arange(sl.start, sl.stop)[:, None] < cols[None, :]
        same = ia[sl, None] == ib[None, :]
        for s in (0, 1):
            hist[s] += np.bincount(bins[ok & (same == bool(s))], minlength=n_thr + 1)
    return hist


def reference_pairs(rows, pairs, n_folds: int = 1, n_thr: int = 400, step: float = 0.01):
    """(dist float32 [P], hist int64 [n_folds][2][T + 1], invalid int) of listed pairs, int32 [P][4] = (a, b, same, fold): dist[p] is
    reference_match's d of rows a and b (NaN reads +inf) and counts in hist[fold][same][bin].  A pair with a or b outside 0..n-1,
    same not in {0, 1} or fold outside 0..n_folds-1 is invalid: it reads no row, gets dist -1.0, adds 1 to `invalid` and nothing to
    hist.  n_folds in 1..16."""
    thr = roc_thresholds(n_thr, step)
    if not 1 <= int(n_folds) <= ROC_MAX_FOLDS:
        raise ValueError(f"n_folds must be in 1..{ROC_MAX_FOLDS}")
    rows = np.asarray(rows, np.float32)
    pairs = np.asarray(pairs, np.int32).reshape(-1, 4)
    n = rows.shape[0]
    a, b, same, fold = (pairs[:, i].astype(np.int64) for i in range(4))
    valid = (a >= 0) & (a < n) & (b >= 0) & (b < n) & ((same == 0) | (same == 1)) & (fold >= 0) & (fold < n_folds)
    dist = np.full(pairs.shape[0], -1.0, np.float32)
    for r in np.unique(a[valid]):                                       # one row of the distance matrix per distinct a
        sel = np.flatnonzero(valid & (a == r))
        dist[sel] = _distances(rows[r:r + 1], rows[b[sel]])[0]
    hist = np.zeros((int(n_folds), 2, n_thr + 1), np.int64)
    np.add.at(hist, (fold[valid], same[valid], roc_bin(dist[valid], thr)), 1)
    return dist, hist, int((~valid).sum())


def _curves(hist):
    """(TA, FA int64 [T], genuine, impostors): accepts at every threshold t, the pairs with bin <= t"""
    hist = np.asarray(hist, np.int64)
    if hist.ndim != 2 or hist.shape[0] != 2 or hist.shape[1] < 2:
        raise ValueError("hist must be [2][T + 1]")
    return np.cumsum(hist[1])[:-1], np.cumsum(hist[0])[:-1], int(hist[1].sum()), int(hist[0].sum())


def roc_summary(hist, step: float = 0.01, far_targets=FAR_TARGETS) -> dict:
    """The verification curve of a histogram int64 [2][T + 1] (hist[0] impostor, hist[1] genuine pairs) on roc_thresholds(T, step):
      thresholds float32 [T];  TA, FA int64 [T]: genuine / impostor pairs accepted at thr[t] (d < thr[t]);  genuine, impostors: the
      totals;  TAR, FAR float64 [T]: TA / genuine, FA / impostors (0.0 where the total is 0);  accuracy float64 [T]:
      (TA + impostors - FA) / (genuine + impostors)
      best_accuracy  {t, threshold, accuracy}: the FIRST t of the maximum of the integer TA + impostors - FA (np.argmax's rule)
      eer            {t, threshold, far, frr}: the FIRST t with FAR[t] >= 1 - TAR[t], compared in integers (FA[t] * genuine >=
                     (genuine - TA[t]) * impostors), both rates at that t, nothing interpolated; None when no t has it, or a total
                     is 0
      far            {target: {t, threshold, fa, ta, far, tar}} for every FAR target: the LARGEST t with FA[t] <= target *
                     impostors, compared as exact rationals (FA is non-decreasing in t; equality meets the target).  A float
                     target stands for the decimal it prints as (1e-3 is 1/1000); a Fraction or an int is taken as it is.  Where
                     even t = 0 exceeds the target, or there is no impostor pair: t None, threshold None ("none").
    Every `threshold` is the float32 thr[t] itself, ready for DeviceMatcher.match(threshold=): the matcher accepts d < thr[t], which
    is what TA and FA counted.  These tie rules are this project's pinning of what the usual scripts leave to argmax and to
    interpolation."""
    from fractions import Fraction
    TA, FA, G, I = _curves(hist)
    T = TA.size
    thr = roc_thresholds(T, step)
    rate = lambda x, n: x / n if n else np.zeros(T)
    correct = TA + (I - FA)
    tb = int(np.argmax(correct))
    res = dict(thresholds=thr, TA=TA, FA=FA, genuine=G, impostors=I, TAR=rate(TA, G), FAR=rate(FA, I), accuracy=rate(correct, G + I),
               best_accuracy=dict(t=tb, threshold=thr[tb], accuracy=float(rate(correct, G + I)[tb])), eer=None, far={})
    if G and I:
        for t in range(T):
            if int(FA[t]) * G >= (G - int(TA[t])) * I:
                res["eer"] = dict(t=t, threshold=thr[t], far=int(FA[t]) / I, frr=(G - int(TA[t])) / G)
                break
    for target in far_targets:
        frac = target if isinstance(target, (int, Fraction)) else Fraction(repr(float(target)))
        meets = [t for t in range(T) if I and Fraction(int(FA[t])) <= frac * I]
        if meets:
            t = meets[-1]
            res["far"][target] = dict(t=t, threshold=thr[t], fa=int(FA[t]), ta=int(TA[t]), far=int(FA[t]) / I, tar=int(TA[t]) / G if G else 0.0)
        else:
            res["far"][target] = dict(t=None, threshold=None, fa=None, ta=None, far=None, tar=None)
    return res


def fold_protocol(hist_folds) -> dict:
    """The LFW protocol on per-fold histograms int64 [K][2][T + 1]: for fold k, t* is the first argmax of the accuracy (the integer
    TA + impostors - FA) over the OTHER folds' summed histograms, and the fold's accuracy is its own at t*.
    {t: int [K], accuracy: float64 [K], mean, std (np.std, ddof 0)}; a fold without pairs has accuracy NaN."""
    h = np.asarray(hist_folds, np.int64)
    if h.ndim != 3 or h.shape[1] != 2:
        raise ValueError("hist_folds must be [K][2][T + 1]")
    total = h.sum(axis=0)
    ts, acc = [], []
    for k in range(h.shape[0]):
        TA, FA, G, I = _curves(total - h[k])
        t = int(np.argmax(TA + (I - FA)))
        TA, FA, G, I = _curves(h[k])
        ts.append(t)
        acc.append((int(TA[t]) + I - int(FA[t])) / (G + I) if G + I else float("nan"))
    acc = np.array(acc, np.float64)
    return dict(t=np.array(ts), accuracy=acc, mean=float(np.mean(acc)), std=float(np.std(acc)))


class Gallery:
    """The feature library on the device: `rows` float32 [capacity, D] and `ids` int32 [capacity], of which the first `count` (a
    host-side number) are enrolled.  A library read from a file goes in with `load`; `enrol` appends the embeddings of a batch."""

    def __init__(self, capacity: int, D: int, device="cuda:0"):
        import torch
        self.capacity, self.D, self.count = int(capacity), int(D), 0
        self.rows = torch.zeros(self.capacity, self.D, dtype=torch.float32, device=device)
        self.ids = torch.full((self.capacity,), -1, dtype=torch.int32, device=device)

    def load(self, rows, ids=None):
        """append float32 rows [n, D] (numpy or tensor) with their ids (default: their row indices)"""
        import torch
        rows = torch.as_tensor(np.asarray(rows, np.float32) if not hasattr(rows, "device") else rows).reshape(-1, self.D)
        n = rows.shape[0]
        if self.count + n > self.capacity:
            raise ValueError(f"gallery is full: {self.count} + {n} > {self.capacity}")
        sl = slice(self.count, self.count + n)
        self.rows[sl].copy_(rows)
        new = torch.arange(self.count, self.count + n, dtype=torch.int32) if ids is None else torch.as_tensor(np.asarray(ids, np.int32)).reshape(n)
        self.ids[sl].copy_(new)
        self.count += n

    def enrol(self, matcher, outputs, ids=None, stream=None):
        """append the embeddings of `outputs` (int8 [B, D], the tensor Runner.run_batch returns): the embed kernel writes them
        straight into the gallery's rows.  A captured graph of match() fixes n: enrolling more rows needs a re-capture, or a
        capture at the final n."""
        import torch
        B = outputs.shape[0]
        if self.count + B > self.capacity:
            raise ValueError(f"gallery is full: {self.count} + {B} > {self.capacity}")
        sl = slice(self.count, self.count + B)
        matcher.embed(outputs, out=self.rows[sl], stream=stream)
        new = torch.arange(self.count, self.count + B, dtype=torch.int32) if ids is None else torch.as_tensor(np.asarray(ids, np.int32)).reshape(B)
        with torch.cuda.stream(stream or torch.cuda.current_stream(self.rows.device)):
            self.ids[sl].copy_(new, non_blocking=True)
        self.count += B


class DeviceMatcher:
    """tf2_emb_* for `net` (a tf2_amd.network.NetWork with its q table set, whose only output is a 1 x 1 map of D = 2..512 channels).
      embed(outputs, out=None, stream=None) -> float32 [B, D] unit embeddings (written into `out` when given: a slice of a gallery)
      match(outputs, gallery, ids=None, n=None, threshold=1.0, truth=None, stream=None) -> Result of device tensors
    outputs: the int8 device tensor [B, D] Runner.run_batch returns; gallery: a Gallery, or a float32 device tensor [N, D] with
    ids int32 [N] or None (the id is then the row index); n: rows to search (default: all enrolled); truth: an int32 device tensor
    [B] (refill it between the replays of a captured graph).  Enqueued on `stream` (default: the current one); nothing
    synchronises.  With truth the counts are added to `self.tally` (int64 [5] on the device, TALLY names them), which keeps
    accumulating over runs and graph replays until reset(); accuracy() is the only method that synchronises.  The scratch of a
    call is allocated per call from torch's caching allocator (inside a captured graph: from the graph's pool); matchers that tally
    side by side on several streams may share one object (integer atomics).  A captured graph fixes n: enrolling more rows needs a
    re-capture, or a capture at the final n."""

    def __init__(self, net, top_k: int = 5):
        from . import _lib
        self.net, self.top_k, self.D = net, int(top_k), int(net.plan[-1].N)
        d = _lib.EmbDesc(C.sizeof(_lib.EmbDesc), self.top_k)
        h = C.c_void_p()
        _lib.check(_lib.lib().tf2_emb_create(net._h, C.byref(d), C.byref(h)))
        self._h = h
        self.tally = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            from . import _lib
            _lib.lib().tf2_emb_destroy(h)
            self._h = None

    def _check(self, outputs):
        import torch
        assert outputs.dtype == torch.int8 and outputs.is_contiguous() and outputs.device.type == "cuda"
        assert outputs.dim() == 2 and outputs.shape[1] == self.D

    def scratch_size(self, batch: int, n: int) -> int:
        from . import _lib
        return int(_lib.lib().tf2_emb_scratch_size(self._h, int(batch), int(n)))

    def embed(self, outputs, out=None, stream=None):
        import torch
        from . import _lib
        self._check(outputs)
        dev, B = outputs.device, outputs.shape[0]
        stream = stream or torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            if out is None:
                out = torch.empty(B, self.D, dtype=torch.float32, device=dev)
            assert out.dtype == torch.float32 and out.is_contiguous() and out.device == dev and tuple(out.shape) == (B, self.D)
            _lib.check(_lib.lib().tf2_emb_embed(self._h, outputs.data_ptr(), B, out.data_ptr(), stream.cuda_stream))
        return out

    def match(self, outputs, gallery, ids=None, n=None, threshold: float = 1.0, truth=None, stream=None) -> Result:
        import torch
        from . import _lib
        self._check(outputs)
        dev, B, k = outputs.device, outputs.shape[0], self.top_k
        if isinstance(gallery, Gallery):
            n = gallery.count if n is None else int(n)
            assert n <= gallery.count, "n exceeds the enrolled rows"
            gallery, ids = gallery.rows, gallery.ids
        n = gallery.shape[0] if n is None else int(n)
        assert gallery.dtype == torch.float32 and gallery.is_contiguous() and gallery.device == dev and gallery.dim() == 2
        assert gallery.shape[1] == self.D and 1 <= n <= gallery.shape[0]
        if ids is not None:
            assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.device == dev and ids.dim() == 1 and ids.shape[0] >= n
        if truth is not None:
            assert truth.dtype == torch.int32 and truth.is_contiguous() and truth.device == dev and tuple(truth.shape) == (B,)
            if self.tally is None:                                # (allocated and zeroed outside the enqueue below)
                self.tally = torch.zeros(5, dtype=torch.int64, device=dev)
        stream = stream or torch.cuda.current_stream(dev)
        nbytes = self.scratch_size(B, n)
        with torch.cuda.stream(stream):
            scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
            idx = torch.empty(B, k, dtype=torch.int32, device=dev)
            dist = torch.empty(B, k, dtype=torch.float32, device=dev)
            out_ids = torch.empty(B, k, dtype=torch.int32, device=dev)
            emb = torch.empty(B, self.D, dtype=torch.float32, device=dev)
            ptr = lambda t: t.data_ptr() if t is not None else None
            _lib.check(_lib.lib().tf2_emb_match(self._h, outputs.data_ptr(), B, gallery.data_ptr(), ptr(ids), n, float(threshold),
                                                scratch.data_ptr(), scratch.numel() * 8, idx.data_ptr(), dist.data_ptr(),
                                                out_ids.data_ptr(), emb.data_ptr(), ptr(truth),
                                                ptr(self.tally) if truth is not None else None, stream.cuda_stream))
        return Result(idx, dist, out_ids, emb)

    def reset(self, stream=None):
        """zero the running tally (enqueued on `stream`, default the current one)"""
        import torch
        if self.tally is not None:
            with torch.cuda.stream(stream or torch.cuda.current_stream(self.tally.device)):
                self.tally.zero_()

    def accuracy(self) -> dict:
        """the five running counters by name (TALLY).  Synchronises the device."""
        import torch
        if self.tally is None:
            return dict.fromkeys(TALLY, 0)
        torch.cuda.synchronize(self.tally.device)
        return dict(zip(TALLY, (int(v) for v in self.tally.cpu().tolist())))

    def reference(self, outputs, gallery, ids=None, n=None, threshold: float = 1.0, truth=None):
        """The statement on host copies of the same inputs, with the net's last Q row: (Result, tally or None)"""
        host = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else (None if t is None else np.asarray(t))
        if isinstance(gallery, Gallery):
            n = gallery.count if n is None else int(n)
            gallery, ids = gallery.rows, gallery.ids
        g = host(gallery)
        n = g.shape[0] if n is None else int(n)
        i = host(ids)
        e = reference_embed(host(outputs), self.net.q[self.net.num_layer])
        idx, dist, out_ids = reference_match(e, g[:n], None if i is None else i[:n], self.top_k)
        tally = None if truth is None else reference_tally(idx, dist, out_ids, host(truth), threshold)
        return Result(idx, dist, out_ids, e), tally


class DeviceRoc:
    """tf2_emb_roc_*: the distance histograms behind a verification curve, kept on the device.
      add(gallery_or_rows, ids=None, other=None, other_ids=None, n=None, stream=None)   all pairs: self mode (i < j of one set), or
          cross mode against `other` (every (i, j)).  A set is a Gallery (its rows[:count], ids[:count]; n: the first n of the first
          set instead) or a float32 device tensor [N, D] with ids int32 [N].  Needs n_folds == 1.
      add_pairs(rows, pairs, stream=None) -> dist   listed pairs, int32 device tensor [P, 4] = (a, b, same, fold), of float32 device
          rows [N, D] (or a Gallery): float32 device tensor [P], -1.0 for an invalid pair; invalid pairs are counted in `invalid`
    `hist` is an int64 device tensor [n_folds, 2, n_thr + 1], zeroed at construction, and `invalid` int64 [1]; both keep
    accumulating over calls and graph replays until reset().  The calls are enqueued on `stream` (default: the current one), allocate
    nothing but add_pairs' result, never synchronise and are graph-capturable (a captured graph fixes the row counts).  summary()
    (roc_summary of the histogram, summed over the folds) and folds() (fold_protocol) synchronise and make one host copy."""

    def __init__(self, n_thr: int = 400, step: float = 0.01, n_folds: int = 1, device="cuda:0"):
        import torch
        roc_thresholds(n_thr, step)                                # (the checks)
        if not 1 <= int(n_folds) <= ROC_MAX_FOLDS:
            raise ValueError(f"n_folds must be in 1..{ROC_MAX_FOLDS}")
        self.n_thr, self.step, self.n_folds = int(n_thr), float(np.float32(step)), int(n_folds)
        self.hist = torch.zeros(self.n_folds, 2, self.n_thr + 1, dtype=torch.int64, device=device)
        self.invalid = torch.zeros(1, dtype=torch.int64, device=device)

    @staticmethod
    def _set(rows, ids, n):
        """(rows tensor, ids tensor, n) of a Gallery or a tensor with ids"""
        import torch
        if isinstance(rows, Gallery):
            n = rows.count if n is None else int(n)
            assert n <= rows.count, "n exceeds the enrolled rows"
            rows, ids = rows.rows, rows.ids
        n = rows.shape[0] if n is None else int(n)
        assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.device.type == "cuda" and rows.dim() == 2
        assert 1 <= n <= rows.shape[0]
        if ids is not None:
            assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.device == rows.device and ids.dim() == 1 and ids.shape[0] >= n
        return rows, ids, n

    def add(self, gallery_or_rows, ids=None, other=None, other_ids=None, n=None, stream=None):
        import torch
        from . import _lib
        if self.n_folds != 1:
            raise ValueError("add() counts into one histogram: n_folds must be 1")
        a, ia, na = self._set(gallery_or_rows, ids, n)
        assert ia is not None, "a raw tensor of rows needs its ids"
        b, ib, nb = (None, None, 0) if other is None else self._set(other, other_ids, None)
        assert other is None or (ib is not None and b.device == a.device and b.shape[1] == a.shape[1])
        assert a.device == self.hist.device
        stream = stream or torch.cuda.current_stream(a.device)
        ptr = lambda t: t.data_ptr() if t is not None else None
        _lib.check(_lib.lib().tf2_emb_roc_hist(a.data_ptr(), ia.data_ptr(), na, ptr(b), ptr(ib), nb, a.shape[1], self.n_thr, self.step,
                                               self.hist.data_ptr(), stream.cuda_stream))

    def add_pairs(self, rows, pairs, stream=None):
        import torch
        from . import _lib
        rows, _, n = self._set(rows, None, None)
        assert pairs.dtype == torch.int32 and pairs.is_contiguous() and pairs.device == rows.device and pairs.dim() == 2 and pairs.shape[1] == 4
        assert rows.device == self.hist.device
        stream = stream or torch.cuda.current_stream(rows.device)
        with torch.cuda.stream(stream):
            dist = torch.empty(pairs.shape[0], dtype=torch.float32, device=rows.device)
            _lib.check(_lib.lib().tf2_emb_roc_pairs(rows.data_ptr(), n, rows.shape[1], pairs.data_ptr(), pairs.shape[0], self.n_folds,
                                                    self.n_thr, self.step, dist.data_ptr(), self.hist.data_ptr(),
                                                    self.invalid.data_ptr(), stream.cuda_stream))
        return dist

    def reset(self, stream=None):
        """zero the histograms and the invalid counter (enqueued on `stream`, default the current one)"""
        import torch
        with torch.cuda.stream(stream or torch.cuda.current_stream(self.hist.device)):
            self.hist.zero_()
            self.invalid.zero_()

    def _host(self) -> np.ndarray:
        import torch
        torch.cuda.synchronize(self.hist.device)
        return self.hist.cpu().numpy()

    def summary(self, far_targets=FAR_TARGETS) -> dict:
        """roc_summary of the histogram (summed over the folds).  Synchronises the device."""
        return roc_summary(self._host().sum(axis=0), self.step, far_targets)

    def folds(self) -> dict:
        """fold_protocol of the per-fold histograms.  Synchronises the device."""
        return fold_protocol(self._host())

    def reference(self, gallery_or_rows, ids=None, other=None, other_ids=None, n=None) -> np.ndarray:
        """The statement on host copies of add()'s inputs: int64 [2][n_thr + 1]"""
        def host(rows, ids, n):
            if isinstance(rows, Gallery):
                n = rows.count if n is None else int(n)
                rows, ids = rows.rows, rows.ids
            h = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
            n = rows.shape[0] if n is None else int(n)
            return h(rows)[:n], h(ids)[:n]
        a, ia = host(gallery_or_rows, ids, n)
        b, ib = (None, None) if other is None else host(other, other_ids, None)
        return reference_roc_hist(a, ia, b, ib, self.n_thr, self.step)

    def reference_pairs(self, rows, pairs):
        """The statement on host copies of add_pairs()'s inputs: (dist, hist, invalid)"""
        h = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
        if isinstance(rows, Gallery):
            rows = rows.rows
        return reference_pairs(h(rows), h(pairs), self.n_folds, self.n_thr, self.step)
