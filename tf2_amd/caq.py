"""CAQ calibration on the device: float maps to per-channel Q rows  (tf2_caq_*, include/tf2_amd.h; csrc/act_caq.hip)

The reference makes its Q file with Quantization/feature_write.py (a float forward over calibration images keeping the maximum of
|feature|) and quantization.py (QuantizeForShift per channel, QuantizeChannel's mean clamp); `calibrate.Calibrator` restates that with
torch ops and a Python loop per channel.  This module is the same step on the device: `DeviceCalibrator` reads the float maps that
`fidelity.float_refs` produces, once per pass, into exact per-channel integer stores; `reference_range` / `reference_error` state the
same numbers in numpy (the device stores equal them as integers); `q_max` turns a RANGE store into the reference's Q, bit for bit, and
`q_clip` / `q_mse` are two rules the reference lacks.  Nothing here needs a packed net or a Q table: this runs before either exists.

fit(f) of a finite non-zero float32: the largest integer q with |f| * 2^q <= 127, on the bit pattern: e the unbiased exponent, m the
24-bit significand (a denormal normalised first), fit = 6 - e where m <= 0xFE0000, else 5 - e.  QuantizeForShift on a non-negative
channel is fit of its peak: its `round` branch with the `while` loop and its `floor` branch both land there, and no float32 sits close
enough to 127 * 2^k for the double log2 to fall on the wrong side (tests/test_caq.py sweeps every exponent: no exception found).

RANGE record, 70 int64 a channel (pass 1): n (finite values), nonfinite (NaN, +-inf: nothing else is recorded for these), zeros (+-0),
negatives (finite, < 0), peak_pos / peak_neg (the magnitude bit pattern of the largest positive / most negative value, 0 when none),
hist[b], b = clamp(fit(f), -32, 31) + 32, over the non-zero finite values.  The peaks are maxima, every other slot a sum.  The sum of
hist[b] over b < Q + 32 counts the values beyond the rail at exponent Q.

ERROR record, 12 int64 a channel (pass 2), against a base exponent Qb per record (-64 .. 64); the candidates are Q = Qb + j, j = 0..3.
Per value, in this order:
  1. f is NaN or +-inf: nonfinite += 1, nothing else.
  2. t = f * 2^(Qb + 7), one float32 multiplication.
  3. |t| >= 2^18: e = +-2^18 with t's sign, ref_clamped += 1; otherwise e = rint(t), half to even.
  4. for each j, s = 7 - j: u = (e + (1 << (s - 1))) >> s (arithmetic), v = clamp(u, -128, 127), clipped_j += (u != v),
     d = e - (v << s), sum_d2_j += d^2.
Slots: n, nonfinite, ref_clamped, sum_e2, clipped[4], sum_d2[4].  |d| < 2^18 + 2^14, d^2 < 2^37: a slot holds 2^26 values a channel.

A store is [records][slots]: the network input's channels first ("row -1": the float images), then the table rows in order.
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np

from . import config as cfg
from ._observe import capture_graph, checked_refs, keeping, listed, store_rows

RANGE_SLOTS = 70                     # kCaqRangeSlots
ERROR_SLOTS = 12                     # kCaqErrorSlots
N, NONFINITE, ZEROS, NEGATIVES, PEAK_POS, PEAK_NEG, HIST = 0, 1, 2, 3, 4, 5, 6
BINS = 64                            # kCaqBins
E_N, E_NONFINITE, E_REF_CLAMPED, E_SUM_E2, E_CLIPPED, E_SUM_D2 = 0, 1, 2, 3, 4, 8
FRAC = 7                             # kCaqFrac
CANDS = 4                            # kCaqCands
E_LIMIT = 1 << 18                    # kCaqELimit
SLAB = 32768                         # kCaqSlab: values of one channel a block of the kernels walks (a quarter a wave)
GROUP = 4                            # kCaqGroup: values of a 16-byte load
ROWS_PER_LAUNCH = 64                 # kCaqRowsPerLaunch
QB_MIN, QB_MAX = -64, 64


# ---- the statement ---------------------------------------------------------------------------------------------------------
def fit(f) -> np.ndarray:
    """int64, of float32 values (any shape): the largest q with |f| * 2^q <= 127.  0 where f is zero or not finite (undefined there)."""
    bits = np.ascontiguousarray(np.asarray(f, np.float32)).view(np.uint32).astype(np.int64)
    mag = bits & 0x7fffffff
    E, frac = mag >> 23, mag & 0x7fffff
    length = np.frexp(frac.astype(np.float64))[1].astype(np.int64)            # bit length of the denormal's fraction
    den = E == 0
    e = np.where(den, length - 1 - 149, E - 127)
    m = np.where(den, frac << np.clip(24 - length, 0, 24), frac | 0x800000)
    q = 6 - e - (m > 0xFE0000)
    return np.where((mag == 0) | (mag >= 0x7f800000), 0, q)


def empty_range(n_records: int) -> np.ndarray:
    """[n_records, 70] int64 as tf2_caq_store_init leaves it: zeros"""
    return np.zeros((int(n_records), RANGE_SLOTS), np.int64)


def empty_error(n_records: int) -> np.ndarray:
    return np.zeros((int(n_records), ERROR_SLOTS), np.int64)


def combine_range(a, b) -> np.ndarray:
    """The RANGE store after both sets of batches: every slot adds, the two peaks take the maximum"""
    a, b = np.asarray(a, np.int64).reshape(-1, RANGE_SLOTS), np.asarray(b, np.int64).reshape(-1, RANGE_SLOTS)
    out = a + b
    out[:, PEAK_POS:PEAK_NEG + 1] = np.maximum(a[:, PEAK_POS:PEAK_NEG + 1], b[:, PEAK_POS:PEAK_NEG + 1])
    return out


def combine_error(a, b) -> np.ndarray:
    """The ERROR store after both sets of batches (taken against the same base exponents): every slot adds"""
    return np.asarray(a, np.int64).reshape(-1, ERROR_SLOTS) + np.asarray(b, np.int64).reshape(-1, ERROR_SLOTS)


def scale_of(qb) -> np.ndarray:
    """2^(Qb + 7) as float32, Qb clamped to -64 .. 64: the table tf2_caq_error reads"""
    return np.ldexp(np.float32(1), np.clip(np.asarray(qb, np.int64), QB_MIN, QB_MAX) + FRAC).astype(np.float32)


def _planes(x) -> np.ndarray:
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim >= 2, (x.dtype, x.shape)
    return np.ascontiguousarray(x).reshape(x.shape[0], x.shape[1], -1)


def range_records(x) -> np.ndarray:
    """[C, 70] int64 of a float32 tensor [B, C, ...]"""
    x = _planes(x)
    C = x.shape[1]
    rec = empty_range(C)
    if x.size == 0:
        return rec
    bits = x.view(np.uint32).astype(np.int64)
    mag = bits & 0x7fffffff
    fin = mag < 0x7f800000
    nz = fin & (mag != 0)
    neg = nz & (bits >> 31 != 0)
    s = lambda m: m.sum(axis=(0, 2), dtype=np.int64)
    rec[:, N], rec[:, NONFINITE], rec[:, ZEROS], rec[:, NEGATIVES] = s(fin), s(~fin), s(fin & ~nz), s(neg)
    rec[:, PEAK_POS] = np.where(nz & ~neg, mag, 0).max(axis=(0, 2))
    rec[:, PEAK_NEG] = np.where(neg, mag, 0).max(axis=(0, 2))
    b = np.clip(fit(x), -32, 31) + 32
    for k in np.unique(b[nz]):
        rec[:, HIST + int(k)] = s(nz & (b == k))
    return rec


def error_records(x, qb) -> np.ndarray:
    """[C, 12] int64 of a float32 tensor [B, C, ...] against the base exponents qb [C]"""
    x = _planes(x)
    C = x.shape[1]
    rec = empty_error(C)
    if x.size == 0:
        return rec
    qb = np.asarray(qb, np.int64).reshape(-1)
    assert qb.size == C, (qb.size, C)
    fin = np.isfinite(x)
    with np.errstate(over="ignore", under="ignore"):
        t = (np.where(fin, x, np.float32(0)) * scale_of(qb).reshape(1, C, 1)).astype(np.float32)
    big = fin & (np.abs(t) >= np.float32(E_LIMIT))
    e = np.where(big, np.where(t < 0, -E_LIMIT, E_LIMIT), np.rint(np.where(big, np.float32(0), t))).astype(np.int64)
    s = lambda m: m.sum(axis=(0, 2), dtype=np.int64)
    rec[:, E_N], rec[:, E_NONFINITE], rec[:, E_REF_CLAMPED], rec[:, E_SUM_E2] = s(fin), s(~fin), s(big), s(e * e)
    for j in range(CANDS):
        sh = FRAC - j
        u = (e + (1 << (sh - 1))) >> sh
        v = np.clip(u, -128, 127)
        d = e - (v << sh)
        rec[:, E_CLIPPED + j], rec[:, E_SUM_D2 + j] = s(fin & (u != v)), s(d * d)
    return rec


def reference_range(maps, images=None) -> np.ndarray:
    """The RANGE store [records, 70] int64 of one observed batch.  maps: the rows' float32 maps in table order, [B][C][H][W] or [B][C]
    -- a sequence, or a dict {row: map} (its key -1 is not used).  images: the float32 images [B, C, H, W], whose channels lead the
    store; None: the input's records are left out."""
    parts = [] if images is None else [range_records(np.asarray(images, np.float32))]
    parts += [range_records(np.asarray(m, np.float32)) for m in listed(maps)]
    return np.concatenate(parts, axis=0)


def reference_error(maps, images, qb) -> np.ndarray:
    """The ERROR store [records, 12] int64 of one observed batch against qb [records], one base exponent a record in the store's order
    (the images' channels first unless images is None)"""
    tensors = ([] if images is None else [np.asarray(images, np.float32)]) + [np.asarray(m, np.float32) for m in listed(maps)]
    qb = np.asarray(qb, np.int64).reshape(-1)
    parts, at = [], 0
    for x in tensors:
        parts.append(error_records(x, qb[at:at + x.shape[1]]))
        at += x.shape[1]
    assert at == qb.size, (at, qb.size)
    return np.concatenate(parts, axis=0)


# ---- the rules, from host copies of the stores -----------------------------------------------------------------------------
def q_max(rng) -> np.ndarray:
    """[records] int64, the reference's rule: fit of the channel's largest magnitude; 0 for an empty or all-zero channel"""
    r = np.asarray(rng, np.int64).reshape(-1, RANGE_SLOTS)
    peak = np.maximum(r[:, PEAK_POS], r[:, PEAK_NEG])
    return np.where(peak > 0, fit(peak.astype(np.uint32).view(np.float32)), 0)


def q_clip(rng, num: int, den: int) -> np.ndarray:
    """[records] int64: the largest Q <= 31 that sends at most num / den of the channel's finite values beyond the rail --
    over(Q) * den <= num * n with over(Q) = sum of hist[b < Q + 32], Q from -31 (below it bin 0 no longer tells the values apart) -- and
    never below q_max.  q_clip(rng, 0, 1) is q_max.  A channel without a non-zero value keeps q_max's 0."""
    assert den > 0 and num >= 0
    r = np.asarray(rng, np.int64).reshape(-1, RANGE_SLOTS)
    hist = r[:, HIST:HIST + BINS]
    over = np.cumsum(hist, axis=1)[:, :-1]                                        # over[:, k]: Q = k - 31
    ok = over * int(den) <= int(num) * r[:, N:N + 1]
    best = (BINS - 2 - np.argmax(ok[:, ::-1], axis=1)) - 31
    qm = q_max(r)
    return np.where(ok.any(axis=1) & (hist.sum(axis=1) > 0), np.maximum(qm, best), qm)


def q_mse(err, qb) -> np.ndarray:
    """[records] int64: Qb + argmin_j sum_d2_j, ties to the smaller j"""
    e = np.asarray(err, np.int64).reshape(-1, ERROR_SLOTS)
    return np.asarray(qb, np.int64).reshape(-1) + np.argmin(e[:, E_SUM_D2:E_SUM_D2 + CANDS], axis=1)


def mean_clamp(row) -> np.ndarray:
    """QuantizeChannel's clamp on integers: with S the sum of the row's C entries, a positive q with q C > S becomes floor(S / C), then a
    negative q with q C < S becomes ceil(S / C) -- the second rule on the result of the first, as calibrate.quantize_channels"""
    q = np.asarray(row, np.int64).reshape(-1).copy()
    C, S = int(q.size), int(q.sum())
    if C == 0:
        return q
    lo, hi = S // C, -((-S) // C)
    q = np.where((q > 0) & (q * C > S), lo, q)
    q = np.where((q < 0) & (q * C < S), hi, q)
    return q


def record_spans(plan, image_c: int) -> Dict[int, tuple]:
    """{-1: (0, image_c), l: (first record, C)} of the store"""
    spans, at = {-1: (0, int(image_c))}, int(image_c)
    for L in plan:
        spans[L.index] = (at, int(L.N))
        at += int(L.N)
    return spans


def q_rows(plan, q_records, clamp: bool = True) -> Dict[int, np.ndarray]:
    """{-1: image row, l: row of conv l} from one Q a record (q_max / q_clip / q_mse of a store whose input has
    len(q_records) - sum of N channels), as calibrate.Calibrator.q_rows: the mean clamp per row (clamp=False: left out), pooling rows
    (ipool == 1) skipped, residual partners share the element-wise minimum"""
    q = np.asarray(q_records, np.int64).reshape(-1)
    spans = record_spans(plan, q.size - sum(int(L.N) for L in plan))
    rows = {}
    for k, (first, C) in spans.items():
        if k >= 0 and plan[k].ipool == 1:
            continue
        rows[k] = mean_clamp(q[first:first + C]) if clamp else q[first:first + C].copy()
    for L in plan:
        if L.add_src >= 0 and L.add_src in rows and L.index in rows and rows[L.add_src].size == rows[L.index].size:
            m = np.minimum(rows[L.index], rows[L.add_src])
            rows[L.index] = m.copy(); rows[L.add_src] = m.copy()
    return rows


def q_file_text(tables, rows: Dict[int, np.ndarray]) -> str:
    """The combined Q file of Calibrator.q_file_text: the image row, then one line per output channel of every conv row"""
    vals: List[int] = [int(v) for v in rows[-1]]
    for L in cfg.build_plan(tables):
        if L.ipool != 1:
            vals += [int(v) for v in rows[L.index]]
    assert len(vals) == cfg.q_value_count(tables)
    return "".join(f"{v}\n" for v in vals)


# ---- the device -------------------------------------------------------------------------------------------------------------------
def rows_of(plan, image_chw) -> List[dict]:
    """[{layer, C, HW, first}] of the store, row -1 first"""
    return [dict(layer=r["layer"], C=r["C"], HW=r["H"] * r["W"], first=r["first"]) for r in store_rows(plan, image_chw)]


class DeviceCalibrator:
    """Both passes of the tables' program on `device`: owns the two int64 stores and the scale table as torch tensors; needs no NetWork.
      observe(images, refs)        pass 1 (tf2_caq_range) of one batch, enqueued on the current stream with no synchronisation,
                                   accumulating into the RANGE store.  images: float32 [batch, C, H, W] on the device, or None.  refs: a
                                   list in row order (fidelity.float_refs) or a dict {row: tensor} of contiguous float32 device tensors
                                   [batch, C, H, W] ([batch, C] for an end-pool row); None or a missing row: not observed.
      set_base(qb)                 the base exponents of pass 2, one a record (clamped to -64 .. 64); empties the ERROR store.
      observe_error(images, refs)  pass 2 (tf2_caq_error) of one batch into the ERROR store.
      capture(images, refs, error=False)   a pass as a HIP graph over the static buffers; returns the replay function.
      reset()                      both stores empty (enqueued);  range_store() / error_store(): host copies [records, 70 / 12] int64.
    range_store= / error_store=: the store tensors of another calibrator of the same program -- calibrators that run side by side on
    several streams may accumulate into one store: the adds are atomic."""

    def __init__(self, tables, image_chw, device="cuda:0", range_store=None, error_store=None):
        import torch
        self.tables, self.device = tables, torch.device(device)
        self.plan = cfg.build_plan(tables)
        self.image_chw = tuple(int(v) for v in image_chw)
        self.rows = rows_of(self.plan, self.image_chw)
        self.records = self.rows[-1]["first"] + self.rows[-1]["C"]
        self.range_dev = self._store(range_store, RANGE_SLOTS)
        self.error_dev = self._store(error_store, ERROR_SLOTS)
        self.qb = np.zeros(self.records, np.int64)
        self._scales = torch.from_numpy(scale_of(self.qb)).to(self.device)
        if range_store is None:
            self._init(self.range_dev)
        if error_store is None:
            self._init(self.error_dev)

    def _store(self, given, slots):
        import torch
        if given is None:
            return torch.empty(self.records * slots, dtype=torch.int64, device=self.device)
        assert given.dtype == torch.int64 and given.numel() >= self.records * slots and given.device == self.device
        return given

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def _init(self, store) -> None:
        from . import _lib
        _lib.check(_lib.lib().tf2_caq_store_init(store.data_ptr(), store.numel() * 8, self._stream()))

    def reset(self) -> None:
        self._init(self.range_dev)
        self._init(self.error_dev)

    def set_base(self, qb) -> None:
        import torch
        qb = np.clip(np.asarray(qb, np.int64).reshape(-1), QB_MIN, QB_MAX)
        assert qb.size == self.records, (qb.size, self.records)
        self.qb = qb
        self._scales.copy_(torch.from_numpy(scale_of(qb)).to(self.device))
        self._init(self.error_dev)

    def _tables(self, images, refs):
        """the host arrays tf2_caq_* read at enqueue (and the batch); every tensor checked against its row"""
        from . import _lib
        tensors = [images] + listed(refs, len(self.plan))
        batch = next((int(t.shape[0]) for t in tensors if t is not None), 0)
        ptrs = checked_refs(self.rows, tensors, batch, self.device)
        desc = (_lib.CaqRow * len(self.rows))()
        for d, r in zip(desc, self.rows):
            d.C, d.HW, d.first_record = r["C"], r["HW"], r["first"]
        return desc, ptrs, len(self.rows), batch

    def observe(self, images, refs) -> None:
        from . import _lib
        desc, ptrs, n, batch = self._tables(images, refs)
        _lib.check(_lib.lib().tf2_caq_range(desc, ptrs, n, batch, self.range_dev.data_ptr(), self.range_dev.numel() * 8, self._stream()))

    def observe_error(self, images, refs) -> None:
        from . import _lib
        desc, ptrs, n, batch = self._tables(images, refs)
        _lib.check(_lib.lib().tf2_caq_error(desc, ptrs, n, batch, self._scales.data_ptr(), self.error_dev.data_ptr(),
                                            self.error_dev.numel() * 8, self._stream()))

    def capture(self, images, refs, error: bool = False):
        """observe(images, refs) -- error=True: observe_error -- as a HIP graph: refill the buffers, replay"""
        step = (lambda: self.observe_error(images, refs)) if error else (lambda: self.observe(images, refs))
        # warm-up outside the capture; the store is put back
        self._graph = capture_graph(step, self.device, keeping(self.error_dev if error else self.range_dev, step))
        return self._graph.replay

    def range_store(self) -> np.ndarray:
        return self.range_dev.cpu().numpy()[:self.records * RANGE_SLOTS].reshape(-1, RANGE_SLOTS).copy()

    def error_store(self) -> np.ndarray:
        return self.error_dev.cpu().numpy()[:self.records * ERROR_SLOTS].reshape(-1, ERROR_SLOTS).copy()


def calibrate(tables, model, batches, rule="max", device="cuda:0", bn_eps: float = 1e-5, clamp: bool = True) -> str:
    """The Q file text of `tables` with the float32 LoadModel stream `model` over `batches` (an iterable of float32 image batches
    [B, C, H, W], numpy or torch; a sequence for rule "mse", which reads them twice): fidelity.float_refs per batch, pass 1 on the
    device -- and pass 2 against Qb = q_max for "mse" -- then the rule on the host copy of the store, the mean clamp and the residual
    pairs of q_rows.  rule: "max" (the reference's), ("clip", num, den), "mse"."""
    import torch
    from . import fidelity
    dev = torch.device(device)
    if rule == "mse":
        batches = list(batches)
    cal = None

    def each():
        nonlocal cal
        for x in batches:
            x = torch.as_tensor(np.asarray(x, np.float32) if not torch.is_tensor(x) else x, dtype=torch.float32, device=dev).contiguous()
            if cal is None:
                cal = DeviceCalibrator(tables, tuple(x.shape[1:]), dev)
            yield x, fidelity.float_refs(tables, model, x, device=dev, bn_eps=bn_eps)

    for x, refs in each():
        cal.observe(x, refs)
    assert cal is not None, "calibrate: no batches"
    rng = cal.range_store()
    if rule == "max":
        q = q_max(rng)
    elif rule == "mse":
        cal.set_base(q_max(rng))
        for x, refs in each():
            cal.observe_error(x, refs)
        q = q_mse(cal.error_store(), cal.qb)
    elif isinstance(rule, (tuple, list)) and len(rule) == 3 and rule[0] == "clip":
        q = q_clip(rng, int(rule[1]), int(rule[2]))
    else:
        raise ValueError(f"calibrate: unknown rule {rule!r}")
    return q_file_text(tables, q_rows(cal.plan, q, clamp=clamp))
