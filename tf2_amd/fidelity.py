"""Layer fidelity: how far is each channel of each layer from the float network?  (tf2_fid_*, include/tf2_amd.h; csrc/act_fidelity.hip)

The reference closes its quantisation work with Quantization/debug/CompareError.py: every float feature map scaled by 2^Q[c] per
channel against the integer run's map, 100 * sum|int8 - q*float| / sum|q*float| per layer; Verify() (network_helper.cpp:18-141) does the
same for the last row.  `calibrate.float_forward` is the float side, `audit.DeviceAuditor` the integer side; this module is the
comparison between them, on the device: `DeviceComparator` sets every kept int8 map of a step against the float map of the same row
and keeps exact per-channel integer statistics, `reference_compare` states the same numbers in numpy (the device store equals it as
integers), `summary` / `layer_summary` turn a store into rel_l1 (CompareError's figure), SQNR, bias, cosine, `report` prints them.

The comparison is made in fixed point, FRAC = 8 fractional bits of an int8 LSB.  For an int8 value v, its float32 reference f and the
channel's scale exponent Q (the scale is 2^Q: Verify's 1 << -q[l + 1][c] of the runtime table), in this order:
  1. f is NaN or +-inf: nonfinite += 1, nothing else.
  2. t = f * 2^(Q + 8), one float32 multiplication (exact unless it overflows to +-inf, which step 3 takes).
  3. |t| >= 65536: e = +-65536 with t's sign, ref_clamped += 1.
  4. otherwise e = rint(t), half to even (65535.5 -> 65536, not clamped).
  5. d = 256 v - e, |d| < 2^17.
  6. k = min(7, bit_length((|d| + 128) >> 8)): the error in whole LSBs after rounding; k = 0: v is the nearest int8 to the scaled float.
The record of a channel is 18 int64 (SLOTS): n, nonfinite, ref_clamped, max_abs_d, sum_d, sum_abs_d, sum_d2, sum_abs_e, sum_e2,
sum_q2 = sum (256 v)^2, hist[8].  d^2 < 2^34: sum_d2 holds 2^29 values a channel whatever they are.  A store is [records][18]: the
network input's channels first ("row -1": float images against their own quantisation), then the table rows in order.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np

from . import calibrate
from ._observe import DeviceObserver, Handle, checked_refs, described_rows, listed
from .preprocess import quant_input

SLOTS = 18
N, NONFINITE, REF_CLAMPED, MAX_ABS_D, SUM_D, SUM_ABS_D, SUM_D2, SUM_ABS_E, SUM_E2, SUM_Q2, HIST = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
SLOT_NAMES = ("n", "nonfinite", "ref_clamped", "max_abs_d", "sum_d", "sum_abs_d", "sum_d2", "sum_abs_e", "sum_e2", "sum_q2") + \
    tuple(f"hist{k}" for k in range(8))
FRAC = 8                             # kFidFrac
E_LIMIT = 65536                      # |e| <= 2^16: 256 int8 LSBs
SLAB = 1024                          # kFidSlab: pixels of a row one block of the kernel walks
CHANS = 64                           # kFidChans: channels of a block
TILE = 64                            # kFidTile: pixels of the float tile transposed through LDS at a time
IMG_SLAB = 16384                     # kFidImgSlab
ROWS_PER_LAUNCH = 64                 # kFidRowsPerLaunch


# ---- the statement ---------------------------------------------------------------------------------------------------------
def empty_store(n_records: int) -> np.ndarray:
    """[n_records, 18] int64 as tf2_fid_store_init leaves it: zeros"""
    return np.zeros((int(n_records), SLOTS), np.int64)


def combine(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The store after both sets of batches were compared: every slot adds, max_abs_d takes the maximum"""
    a, b = np.asarray(a, np.int64).reshape(-1, SLOTS), np.asarray(b, np.int64).reshape(-1, SLOTS)
    out = a + b
    out[:, MAX_ABS_D] = np.maximum(a[:, MAX_ABS_D], b[:, MAX_ABS_D])
    return out


def scale_of(q) -> np.ndarray:
    """2^(Q + 8) as float32"""
    return np.ldexp(np.float32(1), np.asarray(q, np.int64) + FRAC).astype(np.float32)


def fixed_ref(f, q):
    """(e, finite, clamped) of float32 references f with scale exponents q (broadcast against f): steps 1-4 of the rule.  e is int64, 0
    where f is not finite."""
    f = np.asarray(f, np.float32)
    fin = np.isfinite(f)
    with np.errstate(over="ignore"):
        t = (np.where(fin, f, np.float32(0)) * scale_of(q)).astype(np.float32)
    big = np.abs(t) >= np.float32(E_LIMIT)
    e = np.where(big, np.where(t < 0, -E_LIMIT, E_LIMIT), np.rint(np.where(big, np.float32(0), t))).astype(np.int64)
    return np.where(fin, e, 0), fin, fin & big


def bit_length(m: np.ndarray) -> np.ndarray:
    """of values below 2^10 ((|d| + 128) >> 8 <= 384)"""
    m = np.asarray(m, np.int64)
    out = np.zeros(m.shape, np.int64)
    for k in range(10):
        out += m >= (1 << k)
    return out


def channel_records(v, f, q) -> np.ndarray:
    """[C, 18] int64 of an int8 tensor v [B, C, ...] against its float32 reference f of the same shape, q: [C] scale exponents"""
    v, f = np.asarray(v), np.asarray(f)
    assert v.dtype == np.int8 and v.ndim >= 2 and f.dtype == np.float32, (v.dtype, v.shape, f.dtype)
    C = v.shape[1]
    rec = empty_store(C)
    if v.size == 0:
        return rec
    f = f.reshape(f.shape[0], C, -1)
    v = v.reshape(v.shape[0], C, -1)
    assert v.shape == f.shape, (v.shape, f.shape)
    q = np.asarray(q, np.int64).reshape(-1)
    assert q.size == C, (q.size, C)
    e, fin, big = fixed_ref(f, q.reshape(1, C, 1))
    v256 = np.where(fin, v.astype(np.int64) * 256, 0)
    d = v256 - e
    ad = np.abs(d)
    k = np.minimum(7, bit_length((ad + 128) >> 8))
    s = lambda x: x.sum(axis=(0, 2), dtype=np.int64)
    rec[:, N], rec[:, NONFINITE], rec[:, REF_CLAMPED] = s(fin), s(~fin), s(big)
    rec[:, MAX_ABS_D] = ad.max(axis=(0, 2))
    rec[:, SUM_D], rec[:, SUM_ABS_D], rec[:, SUM_D2] = s(d), s(ad), s(d * d)
    rec[:, SUM_ABS_E], rec[:, SUM_E2], rec[:, SUM_Q2] = s(np.abs(e)), s(e * e), s(v256 * v256)
    for b in range(8):
        rec[:, HIST + b] = s((k == b) & fin)
    return rec


def reference_compare(maps, refs, q_rows, images=None, q0=None) -> np.ndarray:
    """The store [records, 18] int64 of one compared batch.  maps: the rows' int8 outputs in table order, NCHW ([B][N] or [B][N][1][1] for
    an end-pool row) -- a sequence, or a dict {row: map} such as oracle.netref.RefNet.run returns (its key -1 is not used).  refs: the
    float32 references of the same rows (sequence or dict; a None entry: the row is not compared, its records stay empty).  q_rows: per
    row the channels' scale exponents Q (scale 2^Q; q_rows_of_net).  images, q0: the float32 images [B, C, H, W] the step received and
    the input's exponent Q0 -- row -1 leads the result, v = quant_input(images, 2^Q0) against the same floats; int8 images: a row of
    empty records; None: the input's records are left out."""
    maps = listed(maps)
    refs, q_rows = listed(refs, len(maps)), listed(q_rows, len(maps))
    assert len(refs) == len(maps) == len(q_rows), (len(maps), len(refs), len(q_rows))
    parts = []
    if images is not None:
        images = np.asarray(images)
        if images.dtype == np.int8:
            parts.append(empty_store(images.shape[1]))
        else:
            images = images.astype(np.float32, copy=False)
            trans = np.ldexp(np.float32(1), int(q0))
            parts.append(channel_records(quant_input(images, trans), images, np.full(images.shape[1], int(q0))))
    for m, r, q in zip(maps, refs, q_rows):
        m = np.asarray(m)
        parts.append(empty_store(m.shape[1]) if r is None else channel_records(m, np.asarray(r, np.float32).reshape(m.shape), np.asarray(q)[:m.shape[1]]))
    return np.concatenate(parts, axis=0)


def q_rows_of_net(network) -> Dict[int, np.ndarray]:
    """{-1: the input's Q0 per image channel, l: row l's scale exponents} from a NetWork's runtime table: Verify's 1 << -q[l + 1][c]; a
    pooling row (ipool == 1) carries its source's values there (quantization.cpp:42-43), as in audit.apply_delta"""
    q = np.asarray(network.q, np.int64)
    rows = {-1: np.full(int(network._nd.image_c), -int(q[0, 0]), np.int64)}
    for L in network.plan:
        rows[L.index] = -q[L.index + 1, :L.N]
    return rows


def rows_of(plan, image_chw) -> List[dict]:
    """What tf2_fid_describe reports, from the plan alone (n_doubled is the packed image's business: None here)"""
    return described_rows(plan, image_chw, SLOTS)


def float_refs(tables, model, images, device=None, bn_eps: float = 1e-5) -> list:
    """calibrate.float_forward as a list in row order of contiguous float32 tensors on `device`: [B][C][H][W], a concat member its own
    slice, an end-pool row [B][C]"""
    outs = calibrate.float_forward(tables, model, images, device, bn_eps)
    refs = []
    for l in sorted(k for k in outs if k >= 0):
        y = outs[l]
        if y.dim() == 4 and y.shape[2] == 1 and y.shape[3] == 1:
            y = y.reshape(y.shape[0], y.shape[1])
        refs.append(y.float().contiguous())
    return refs


# ---- verdicts -----------------------------------------------------------------------------------------------------------------
def _figures(rec: np.ndarray) -> dict:
    """The quantities of summary from records [..., 18] (int64): one value a leading index"""
    g = lambda s: rec[..., s].astype(np.float64)
    n, sd2, se2, sq2 = g(N), g(SUM_D2), g(SUM_E2), g(SUM_Q2)
    nz = np.maximum(n, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(g(SUM_ABS_E) > 0, g(SUM_ABS_D) / g(SUM_ABS_E), np.where(g(SUM_ABS_D) > 0, np.inf, 0.0))
        sqnr = np.where(sd2 > 0, np.where(se2 > 0, 10.0 * np.log10(se2 / np.where(sd2 > 0, sd2, 1.0)), -np.inf), np.inf)
        den = 2.0 * np.sqrt(sq2 * se2)
        cos = np.where(den > 0, (sq2 + se2 - sd2) / np.where(den > 0, den, 1.0), np.where((sq2 == 0) & (se2 == 0), 1.0, 0.0))
    return dict(n=rec[..., N].copy(), nonfinite=rec[..., NONFINITE].copy(), ref_clamped=rec[..., REF_CLAMPED].copy(), rel_l1=rel,
                sqnr_db=sqnr, bias_lsb=g(SUM_D) / (256.0 * nz), max_err_lsb=g(MAX_ABS_D) / 256.0, cosine=cos,
                nearest=np.where(n > 0, g(HIST) / nz, 1.0))


def summary(store, rows) -> Dict[int, dict]:
    """{layer: arrays over the row's channels} from a store and its rows (DeviceComparator.rows() / rows_of): n, nonfinite, ref_clamped
    (int64) and, float64,
      rel_l1 = sum_abs_d / sum_abs_e            (CompareError's figure / 100, per channel)
      sqnr_db = 10 log10(sum_e2 / sum_d2)
      bias_lsb = sum_d / (256 n)
      max_err_lsb = max_abs_d / 256
      cosine = (sum_q2 + sum_e2 - sum_d2) / (2 sqrt(sum_q2 sum_e2))       (2 <q, e> = |q|^2 + |e|^2 - |q - e|^2)
      nearest = hist[0] / n
    Pinned: an empty channel (n = 0) has rel_l1 0, sqnr_db +inf, bias_lsb 0, max_err_lsb 0, cosine 1, nearest 1.  sum_abs_e = 0 (an
    all-zero reference): rel_l1 0 where sum_abs_d is 0 too, else +inf.  sum_d2 = 0: sqnr_db +inf; sum_e2 = 0 < sum_d2: -inf.  One of
    sum_q2, sum_e2 zero: cosine 0; both: 1."""
    s = np.asarray(store, np.int64).reshape(-1, SLOTS)
    out = {}
    for r in rows:
        first = int(r["offset"]) // (SLOTS * 8)
        out[int(r["layer"])] = _figures(s[first:first + int(r["C"])])
    return out


def layer_summary(store, rows) -> Dict[int, dict]:
    """{layer: the quantities of summary, one value a row} from each row's integer totals over its channels (max_abs_d: the maximum).
    rel_l1 * 100 is the figure CompareError.py prints for the row; for the last row it is Verify()'s (times 100)."""
    s = np.asarray(store, np.int64).reshape(-1, SLOTS)
    out = {}
    for r in rows:
        first = int(r["offset"]) // (SLOTS * 8)
        rec = s[first:first + int(r["C"])]
        tot = rec.sum(axis=0)
        tot[MAX_ABS_D] = rec[:, MAX_ABS_D].max(initial=0)
        out[int(r["layer"])] = {k: v[()] for k, v in _figures(tot).items()}
    return out


def report(summ: Dict[int, dict], top: int = 10, layers: Optional[Dict[int, dict]] = None) -> str:
    """For people: one line a row (its figures over all channels: `layers` = layer_summary of the same store; without it the rows'
    figures are the means of the channels'), the first row whose rel_l1 exceeds twice its predecessor's marked with '<<', then the `top`
    worst channels over all rows by rel_l1 and by |bias_lsb|."""
    lines, by_rel, by_bias, prev = [], [], [], None
    marked = False
    for l in sorted(summ):
        r = summ[l]
        n = int(np.asarray(r["n"]).sum())
        if layers is not None:
            g = {k: float(layers[l][k]) for k in ("rel_l1", "sqnr_db", "bias_lsb", "max_err_lsb", "cosine", "nearest")}
        else:
            seen = np.asarray(r["n"]) > 0
            with np.errstate(invalid="ignore"):
                g = {k: float(np.asarray(r[k])[seen].mean()) if seen.any() else 0.0 for k in ("rel_l1", "sqnr_db", "bias_lsb", "cosine", "nearest")}
            g["max_err_lsb"] = float(np.asarray(r["max_err_lsb"]).max(initial=0.0))
        mark = ""
        if n and l >= 0:
            if not marked and prev is not None and g["rel_l1"] > 2.0 * prev:
                mark, marked = "  << first row above twice its predecessor", True
            prev = g["rel_l1"]
        lines.append(f"row {l:3d}  C {np.asarray(r['n']).size:5d}  n {n:10d}  rel_l1 {100.0 * g['rel_l1']:8.3f} %  sqnr {g['sqnr_db']:7.2f} dB  "
                     f"bias {g['bias_lsb']:+7.3f}  max {g['max_err_lsb']:7.2f}  cos {g['cosine']:.5f}  nearest {g['nearest']:.3f}  "
                     f"clamped {int(np.asarray(r['ref_clamped']).sum())}  nonfinite {int(np.asarray(r['nonfinite']).sum())}{mark}")
        for c in np.nonzero(np.asarray(r["n"]) > 0)[0]:
            by_rel.append((float(r["rel_l1"][c]), l, int(c)))
            by_bias.append((abs(float(r["bias_lsb"][c])), l, int(c), float(r["bias_lsb"][c])))
    lines.append(f"-- worst {top} channels by rel_l1")
    for rel, l, c in sorted(by_rel, key=lambda t: (-t[0], t[1], t[2]))[:top]:
        lines.append(f"   row {l:3d} ch {c:5d}  rel_l1 {100.0 * rel:8.3f} %")
    lines.append(f"-- worst {top} channels by |bias_lsb|")
    for _, l, c, b in sorted(by_bias, key=lambda t: (-t[0], t[1], t[2]))[:top]:
        lines.append(f"   row {l:3d} ch {c:5d}  bias {b:+8.3f} LSB")
    return "\n".join(lines)


# ---- the device -------------------------------------------------------------------------------------------------------------------
class FidelityHandle(Handle):
    """tf2_fid_create on a packed NetWork with its Q table (no device needed): rows(), scales(), store_size"""
    PREFIX, SLOTS = "fid", SLOTS

    def scales(self) -> np.ndarray:
        """[records] float32: 2^(Q + 8) of every record (tf2_fid_scales), the table the kernels read"""
        import ctypes as C
        from . import _lib
        cap = self.store_size // (SLOTS * 8)
        out = np.zeros(cap, np.float32)
        n = C.c_int(0)
        _lib.check(_lib.lib().tf2_fid_scales(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n)))
        assert n.value == cap
        return out


class DeviceComparator(DeviceObserver, FidelityHandle):
    """The comparison of `network` (a NetWork, packed and bound) at one batch size: owns the handle, the keep_all workspace, the logits,
    the scale table and the int64 store as torch tensors.
      observe(images, refs)   one keep_all step and the comparison of every row behind it, enqueued on the current stream with no
                        synchronisation, accumulating into the store; returns the int8 logits tensor (device), the same as
                        Runner.run_batch's.  images: float32 or int8 [batch, C, H, W] on the network's device.  refs: a list in row
                        order (float_refs) or a dict {row: tensor} of contiguous float32 device tensors [batch, C, H, W] ([batch, C]
                        for an end-pool row); None or a missing row: not compared.
      capture(images, refs)   the same as a HIP graph over the static buffers `images` and `refs`; returns the replay function (refill
                        the buffers, replay).
      compare_kept(images, refs)  the comparison kernels alone on the maps the last observe(images, ...) left (capture(..., kept_only=True)).
      reset()           the empty store (enqueued);  store() one host copy [records, 18] int64;  rows() as FidelityHandle.
    store=: the store tensor of another comparator of the same network -- comparators that run side by side on several streams are
    separate objects (one workspace each) and may accumulate into one store: the adds are atomic."""

    def __init__(self, network, batch: int, store=None):
        import torch
        super().__init__(network, batch, store)
        self._scales = torch.from_numpy(self.scales()).to(network.device)
        self._rows = self.rows()

    def _ref_array(self, refs):
        """the host array of device pointers tf2_fid_run reads at enqueue; every tensor checked against its row"""
        return checked_refs(self._rows[1:], refs, self.batch, self.net.device)

    def _call(self, images, refs, kept: bool):
        import torch
        from . import _lib
        self._check_images(images)
        arr = self._ref_array(refs)
        L = _lib.lib()
        head = (self._h, images.data_ptr(), int(images.dtype == torch.int8), self.batch, self._ws.data_ptr(), self._ws.numel())
        tail = (arr, self._scales.data_ptr(), self.store_dev.data_ptr(), self.store_dev.numel() * 8, self._stream())
        _lib.check(L.tf2_fid_kept(*head, *tail) if kept else L.tf2_fid_run(*head, self._logits.data_ptr(), *tail))

    def observe(self, images, refs):
        self._call(images, refs, False)
        return self._logits

    def compare_kept(self, images, refs) -> None:
        """The comparison kernels alone (tf2_fid_kept) on what the last observe(images, ...) left in the workspace: the same maps are
        compared once more.  `images` must be the batch that step received."""
        self._call(images, refs, True)

    def capture(self, images, refs, kept_only: bool = False):
        """kept_only: capture compare_kept(images, refs) instead of observe(images, refs)"""
        step = (lambda: self.compare_kept(images, refs)) if kept_only else (lambda: self.observe(images, refs))
        return self._capture(step, lambda: self.observe(images, refs))  # warm-up outside the capture; the store is put back
