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

`DeviceMatcher(net, top_k)` runs the device path on the int8 tensor Runner.run_batch returns; `Gallery` holds the rows."""
import ctypes as C
from typing import NamedTuple

import numpy as np

from .classify import features_of

MAX_D, MAX_TOP_K = 512, 16           # kEmbMaxD, kEmbMaxTopK (csrc/embed_match.h)
SLAB, GROUP = 64, 32                 # kEmbSlab, kEmbGroup: gallery rows and queries of one stage-1 block
TALLY = ("labelled", "identified", "among_k", "true_accepts", "false_accepts")


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
    d = np.zeros((B, N), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(D):
            t = e[:, c, None] - g[None, :, c]
            d = d + t * t
    d = np.where(np.isnan(d), np.float32(np.inf), d)
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
