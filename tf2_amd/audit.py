"""Activation audit: does a Q file fit the integer engine?  (tf2_audit_*, include/tf2_amd.h; csrc/act_audit.hip)

`calibrate.Calibrator` derives Q rows from a float forward (the reference's feature_write.py + quantization.py); the reference then
checks the result with Quantization/debug/CompareError.py, which dumps every layer of the integer run.  This module is the integer half
of that check without the dump: `DeviceAuditor` reduces every kept map of a step to exact per-channel statistics on the device,
`reference_audit` states the same numbers in numpy (the device store equals it as integers), `summary` turns a store into a per-channel
verdict and `q_delta` / `apply_delta` into a corrected Q file by the reference's own rule (QuantizeForShift, quantization.py:33-46).

The record of a channel is 16 int64 (SLOTS): n, neg, lo_rail (v == -128), hi_rail (v == 127), min, max, sum, sumsq, hist[8] with
hist[b] counting the values whose |v| has bit length b (0 for 0, 1 for 1, 2 for 2..3, ... 7 for 64..127); |v| = 128 is in lo_rail alone.
A store is [records][16]: the network input's channels first ("row -1"), then the table rows in order, each row's channels contiguous.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

from . import config as cfg
from ._observe import DeviceObserver, Handle, described_rows
from .preprocess import quant_input, trans_of

SLOTS = 16
N, NEG, LO_RAIL, HI_RAIL, MIN, MAX, SUM, SUMSQ, HIST = 0, 1, 2, 3, 4, 5, 6, 7, 8
SLAB = 1024                          # kAuditSlab: pixels of a row one block of the kernel walks
CHANS = 256                          # kAuditChans: channels of a block
IMG_SLAB = 16384                     # kAuditImgSlab: values of an image plane one block of the input kernel walks
ROWS_PER_LAUNCH = 64                 # kAuditRowsPerLaunch


# ---- the statement ---------------------------------------------------------------------------------------------------------
def empty_store(n_records: int) -> np.ndarray:
    """[n_records, 16] int64 as tf2_audit_store_init leaves it: zeros, min = 127, max = -128"""
    s = np.zeros((int(n_records), SLOTS), np.int64)
    s[:, MIN], s[:, MAX] = 127, -128
    return s


def combine(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The store after both sets of batches were observed: counters add, min / max take the extreme"""
    a, b = np.asarray(a, np.int64).reshape(-1, SLOTS), np.asarray(b, np.int64).reshape(-1, SLOTS)
    out = a + b
    out[:, MIN] = np.minimum(a[:, MIN], b[:, MIN])
    out[:, MAX] = np.maximum(a[:, MAX], b[:, MAX])
    return out


def channel_records(x) -> np.ndarray:
    """[C, 16] int64 of an int8 tensor [B, C, ...] ([B, C] for an end-pool row): every value of channel c over batch and pixels"""
    x = np.asarray(x)
    assert x.dtype == np.int8 and x.ndim >= 2, (x.dtype, x.shape)
    C = x.shape[1]
    rec = empty_store(C)
    if x.size == 0:
        return rec
    v = np.moveaxis(x.reshape(x.shape[0], C, -1), 1, 0).reshape(C, -1).astype(np.int64)
    rec[:, N] = v.shape[1]
    rec[:, NEG] = (v < 0).sum(1)
    rec[:, LO_RAIL] = (v == -128).sum(1)
    rec[:, HI_RAIL] = (v == 127).sum(1)
    rec[:, MIN], rec[:, MAX] = v.min(1), v.max(1)
    rec[:, SUM], rec[:, SUMSQ] = v.sum(1), (v * v).sum(1)
    a = np.abs(v)
    bits = np.zeros_like(a)
    for k in range(7):
        bits += a >= (1 << k)
    counted = v != -128
    for b in range(8):
        rec[:, HIST + b] = ((bits == b) & counted).sum(1)
    return rec


def reference_audit(maps, images_q=None) -> np.ndarray:
    """The store [records, 16] int64 of one observed batch.  maps: the rows' outputs in table order, NCHW int8 ([B][N] or [B][N][1][1]
    for an end-pool row) -- a sequence, or a dict {row: map} such as oracle.netref.RefNet.run returns (its key -1, the prepared input, is
    not used: it may be the conv1-rewrite form).  images_q: the int8 images [B, C, H, W] the step received (float images: through
    reference_input_quant); None leaves the input's records out of the result."""
    if isinstance(maps, dict):
        maps = [maps[l] for l in sorted(k for k in maps if k >= 0)]
    parts = [] if images_q is None else [channel_records(images_q)]
    parts += [channel_records(m) for m in maps]
    return np.concatenate(parts, axis=0)


def reference_input_quant(images, q0: int) -> np.ndarray:
    """float images -> the int8 values the engine's input rule makes of them (csrc/input_quant.h; q0 = the runtime value net.q[0, 0])"""
    return quant_input(np.asarray(images, np.float32), trans_of(q0))


def rows_of(plan, image_chw) -> List[dict]:
    """What tf2_audit_describe reports, from the plan alone (n_doubled is the packed image's business: None here)"""
    return described_rows(plan, image_chw, SLOTS)


# ---- verdicts -----------------------------------------------------------------------------------------------------------------
def summary(store, rows) -> Dict[int, dict]:
    """{layer: arrays over the row's channels} from a store and its rows (DeviceAuditor.rows() / rows_of): n, neg, lo_rail, hi_rail, min,
    max (int64), mean, rms (float64, from sum and sumsq; 0 for an unobserved channel), bits_used (bit length of the largest |v| seen, 8
    when -128 was seen) and clip_rate = (lo_rail + hi_rail) / n."""
    s = np.asarray(store, np.int64).reshape(-1, SLOTS)
    out = {}
    for r in rows:
        first = int(r["offset"]) // (SLOTS * 8)
        rec = s[first:first + int(r["C"])]
        n = rec[:, N]
        nz = np.maximum(n, 1).astype(np.float64)
        hist = rec[:, HIST:HIST + 8]
        bits = np.where(hist.any(1), 7 - np.argmax(hist[:, ::-1] > 0, axis=1), 0)
        bits = np.where(rec[:, LO_RAIL] > 0, 8, bits)
        out[int(r["layer"])] = dict(
            n=n.copy(), neg=rec[:, NEG].copy(), lo_rail=rec[:, LO_RAIL].copy(), hi_rail=rec[:, HI_RAIL].copy(), min=rec[:, MIN].copy(),
            max=rec[:, MAX].copy(), mean=rec[:, SUM] / nz, rms=np.sqrt(rec[:, SUMSQ] / nz), bits_used=bits.astype(np.int64),
            clip_rate=(rec[:, LO_RAIL] + rec[:, HI_RAIL]) / nz)
    return out


def q_delta(summary_row: dict) -> np.ndarray:
    """Per channel, how far the row's Q can move (the integer form of QuantizeForShift, quantization.py:33-46, applied to the integer
    activations): -1 where a rail value was seen (the channel clipped: its true range is unknown, give it one bit back), 0 for an
    all-zero or unobserved channel, else the largest h >= 0 with max * 2^h <= 127 and min * 2^h >= -128.  For integer data without rail
    values this is calibrate.quantize_for_shift exactly (tests/test_audit.py).  The mean clamp of quantize_channels is not applied."""
    mn, mx = np.asarray(summary_row["min"], np.int64), np.asarray(summary_row["max"], np.int64)
    h = np.zeros(mn.shape, np.int64)
    for k in range(1, 9):
        h += ((mx << k) <= 127) & ((mn << k) >= -128)          # (monotone in k: the count is the largest k that fits)
    idle = (np.asarray(summary_row["n"]) == 0) | ((mn == 0) & (mx == 0))
    h = np.where(idle, 0, h)
    clipped = (np.asarray(summary_row["lo_rail"]) + np.asarray(summary_row["hi_rail"])) > 0
    return np.where(clipped, -1, h).astype(np.int64)


def q_rows_of(plan, q_values) -> Dict[int, np.ndarray]:
    """Q-file ints in file order (quantization.cpp:36-53: three image values, then every row that is no pooling row) -> {-1: image row,
    l: row l}, the form of Calibrator.q_rows (non-negated)"""
    q = np.asarray(q_values, np.int64).ravel()
    rows, pos = {-1: q[:3].copy()}, 3
    for L in plan:
        if L.ipool == 1:
            continue
        rows[L.index] = q[pos:pos + L.N].copy()
        pos += L.N
    assert pos == q.size, (pos, q.size)
    return rows


def apply_delta(plan, q_rows: Dict[int, np.ndarray], deltas: Dict[int, np.ndarray]) -> Dict[int, np.ndarray]:
    """New Q rows (non-negated, the Q file's convention): row l plus deltas[l] (q_delta of the row's summary) per channel.  The image row
    moves by the smallest delta of the input's channels, all three values alike: the engine quantises the whole image with the row's
    first value.  Pooling rows (ipool == 1) have no row of their own and keep their source's.  Tensors that are added together share one
    Q vector, the element-wise minimum, as in Calibrator.q_rows -- repeated until nothing changes, so that a chain of residual blocks
    ends with one vector too."""
    out = {k: np.asarray(v, np.int64).copy() for k, v in q_rows.items()}
    for l, row in out.items():
        if l not in deltas:
            continue
        d = np.asarray(deltas[l], np.int64)
        if l == -1:
            out[l] = row + (int(d.min()) if d.size else 0)
        else:
            assert d.size == row.size, (l, d.size, row.size)
            out[l] = row + d
    changed = True
    while changed:
        changed = False
        for L in plan:
            if L.add_src >= 0 and L.add_src in out and L.index in out and out[L.add_src].size == out[L.index].size:
                m = np.minimum(out[L.index], out[L.add_src])
                if not (np.array_equal(m, out[L.index]) and np.array_equal(m, out[L.add_src])):
                    out[L.index], out[L.add_src] = m.copy(), m.copy()
                    changed = True
    return out


def q_file_text(plan, tables, q_rows: Dict[int, np.ndarray]) -> str:
    """The Q file of the rows, in Calibrator.q_file_text's order: loads through NetWork.Quantization"""
    vals: List[int] = [int(v) for v in q_rows[-1]]
    for L in plan:
        if L.ipool != 1:
            vals += [int(v) for v in q_rows[L.index]]
    assert len(vals) == cfg.q_value_count(tables), (len(vals), cfg.q_value_count(tables))
    return "".join(f"{v}\n" for v in vals)


def report(summ: Dict[int, dict], top: int = 10) -> str:
    """For people: per row the clipped and the idle channels, and the `top` worst channels over all rows by clip rate and by unused bits
    (q_delta: bits of headroom the channel never used)."""
    lines, clip, slack = [], [], []
    for l in sorted(summ):
        r = summ[l]
        d = q_delta(r)
        nclip, nslack = int((d < 0).sum()), int((d > 0).sum())
        lines.append(f"row {l:3d}  C {r['n'].size:5d}  n/ch {int(r['n'].max(initial=0)):9d}  min {int(r['min'].min(initial=127)):4d}  "
                     f"max {int(r['max'].max(initial=-128)):4d}  clipped ch {nclip:5d}  ch with spare bits {nslack:5d}  "
                     f"worst clip rate {float(r['clip_rate'].max(initial=0.0)):.4f}")
        clip += [(float(r["clip_rate"][c]), l, c) for c in np.nonzero(d < 0)[0]]
        slack += [(int(d[c]), l, c, int(r["bits_used"][c])) for c in np.nonzero(d > 0)[0]]
    lines.append(f"-- worst {top} channels by clip rate")
    for rate, l, c in sorted(clip, key=lambda t: (-t[0], t[1], t[2]))[:top]:
        lines.append(f"   row {l:3d} ch {c:5d}  clip rate {rate:.4f}")
    lines.append(f"-- worst {top} channels by unused bits")
    for d, l, c, b in sorted(slack, key=lambda t: (-t[0], t[1], t[2]))[:top]:
        lines.append(f"   row {l:3d} ch {c:5d}  spare bits {d}  bits used {b}")
    return "\n".join(lines)


# ---- the device -------------------------------------------------------------------------------------------------------------------
class AuditHandle(Handle):
    """tf2_audit_create on a packed NetWork (no device needed): rows(), store_size"""
    PREFIX, SLOTS = "audit", SLOTS


class DeviceAuditor(DeviceObserver, AuditHandle):
    """The audit of `network` (a NetWork, packed and bound) at one batch size: owns the handle, the keep_all workspace, the logits and the
    int64 store as torch tensors.
      observe(images)   one keep_all step and the audit of every row behind it, enqueued on the current stream, accumulating into the
                        store; returns the int8 logits tensor (device), the same as Runner.run_batch's.  images: float32 or int8
                        [batch, C, H, W] on the network's device.
      capture(images)   the same as a HIP graph over the static buffer `images`; returns the replay function (refill, replay).
      audit_kept(images) the audit kernels alone on the maps the last observe(images) left (timing; capture(images, kept_only=True)).
      reset()           the empty store (enqueued);  store() one host copy [records, 16] int64;  rows() as AuditHandle.
    store=: the store tensor of another auditor of the same network -- auditors that run side by side on several streams are separate
    objects (one workspace each) and may accumulate into one store: the adds are atomic."""

    def observe(self, images):
        import torch
        from . import _lib
        self._check_images(images)
        _lib.check(_lib.lib().tf2_audit_run(self._h, images.data_ptr(), int(images.dtype == torch.int8), self.batch, self._ws.data_ptr(),
                                            self._ws.numel(), self._logits.data_ptr(), self.store_dev.data_ptr(), self.store_dev.numel() * 8,
                                            self._stream()))
        return self._logits

    def audit_kept(self, images) -> None:
        """The audit kernels alone (tf2_audit_kept) on what the last observe(images) left in the workspace: the same maps are counted
        once more.  `images` must be the batch that step received."""
        import torch
        from . import _lib
        self._check_images(images, typed=False)
        _lib.check(_lib.lib().tf2_audit_kept(self._h, images.data_ptr(), int(images.dtype == torch.int8), self.batch, self._ws.data_ptr(),
                                             self._ws.numel(), self.store_dev.data_ptr(), self.store_dev.numel() * 8, self._stream()))

    def capture(self, images, kept_only: bool = False):
        """kept_only: capture audit_kept(images) instead of observe(images)"""
        step = (lambda: self.audit_kept(images)) if kept_only else (lambda: self.observe(images))
        return self._capture(step, lambda: self.observe(images))        # warm-up outside the capture; the store is put back
