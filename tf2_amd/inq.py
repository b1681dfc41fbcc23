"""INQ weight quantisation: float weights to 0 / +-2^e  (tf2_inq_*, include/tf2_amd.h; csrc/weight_inq.hip)

The engine computes on weights that are 0 or +-2^-i, i = 0..14 (`tf2_get_real` reads anything else as +-1 or 0, without a word).  The
reference makes such weights with TransForm_Kit/Compression/compress_net (incremental network quantisation): per conv / FC weight and
bias, `ComputeQuantumRange` and `ShapeIntoTwoPower` (core/compress_core.py) turn the largest still-float weights into powers of two, the
rest is retrained, and the portion grows until everything is quantised.  This module is that rule:

  reference_range / reference_step   the statement, in numpy, on float32 BIT PATTERNS (no logarithm): bit-identical to the reference's two
                                     functions (tests/golden/ref_inq.npz, tools/gen_inq_golden.py) with one stated deviation (exp_of)
  reference_model_step               the same over a LoadModel stream: filters and conv / FC biases are segments, BN and L2Norm never
  DeviceQuantizer                    tf2_inq_step on torch tensors, in place, every segment in one call; equals reference_* as bits
  quantize_model / engine_check / report   float stream in, engine-ready stream out, and what `tf2_get_real` makes of a stream

The record of a segment is 32 int64 (STATE_DTYPE): n1, n0 (still-float / quantised weights), max1, max0 (their largest magnitude
patterns), nonfinite, max_exp, min_exp, n_keep, n_update, thr (pattern), status, flushed_min, flushed_floor, over_one, hist[16], and two
zero words.  The mask is 1 (any non-zero byte) for a weight that is still float and 0 for a quantised one.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import config as cfg
from .model4bit import split_model

RANGE_GREW, ALL_ZERO, NONFINITE = 1, 2, 4          # status bits (TF2_INQ_*)
NO_EXP = -1000                                     # the "exponent" of zero
N_VALUES = 7                                       # magnitudes of a tensor (compress_train_eval.py:54)
WORDS = 32
STATE_DTYPE = np.dtype([(n, "<i8") for n in ("n1", "n0", "max1", "max0", "nonfinite", "max_exp", "min_exp", "n_keep", "n_update", "thr",
                                             "status", "flushed_min", "flushed_floor", "over_one")] + [("hist", "<i8", (16,)), ("reserved", "<i8", (2,))])
assert STATE_DTYPE.itemsize == WORDS * 8
_MAG = np.uint32(0x7fffffff)


# ---- the statement ---------------------------------------------------------------------------------------------------------
def _bits(w) -> np.ndarray:
    return np.ascontiguousarray(w, np.float32).ravel().view(np.uint32)


def _leading_bit(m: np.ndarray) -> np.ndarray:
    """position of the highest set bit of m (int64, 0 < m < 2^31); 0 for m == 0"""
    return np.frexp(np.maximum(m, 1).astype(np.float64))[1].astype(np.int64) - 1


def exp2_of_bits(mag) -> np.ndarray:
    """floor(log2 a) of float32 magnitude patterns (the exponent of the leading bit, denormals included); NO_EXP for zero"""
    mag = np.asarray(mag).astype(np.int64)
    E = mag >> 23
    e = np.where(E > 0, E - 127, _leading_bit(mag) - 149)
    return np.where(mag == 0, NO_EXP, e)


def exp_of_bits(mag) -> np.ndarray:
    """exp_of on float32 magnitude patterns (bits & 0x7fffffff): the e with 0.75 * 2^e <= a < 1.5 * 2^e, that is the reference's
    floor(log(4a/3) / log 2): E + 1 where the mantissa field is >= 0x400000, else E; a denormal is normalised from its leading bit first.
    NO_EXP for zero.  (The reference's double log returns E at a = 1.5 * 2^E exactly for 20 values of E, all <= -30, where 4a/3 is a
    power of two and log / log rounds under the integer; this rule gives E + 1 there as at every other E.)"""
    mag = np.asarray(mag).astype(np.int64)
    E, m = mag >> 23, mag & 0x7fffff
    p = _leading_bit(m)
    den = E == 0
    e = np.where(den, p - 149, E - 127)
    m = np.where(den, (m << (23 - p)) & 0x7fffff, m)
    return np.where(mag == 0, NO_EXP, e + (m >= 0x400000))


def exp_of(a) -> np.ndarray:
    """exp_of of float32 values (their magnitudes)"""
    return exp_of_bits(_bits(a) & _MAG).reshape(np.shape(a))


def pow2_bits(e) -> np.ndarray:
    """float32 pattern of 2^e, e in -149..127"""
    e = np.asarray(e, np.int64)
    return np.where(e >= -126, (e + 127) << 23, np.int64(1) << np.maximum(e + 149, 0)).astype(np.uint32)


def _check_portions(prev: float, cur: float, n_values: int) -> None:
    if not 0.0 <= prev < 1.0:
        raise ValueError(f"prev = {prev} is not in [0, 1)")
    if not prev <= cur <= 1.0:
        raise ValueError(f"cur = {cur} is not in [prev = {prev}, 1]")
    if n_values < 1:
        raise ValueError("n_values must be >= 1")


def reference_range(w, mask, n_values: int = N_VALUES) -> dict:
    """ComputeQuantumRange on bit patterns: dict(n1, n0, max1, max0, nonfinite, max_exp, min_exp, status)."""
    mag = _bits(w) & _MAG
    one = np.asarray(mask).ravel() != 0
    assert one.size == mag.size, (one.size, mag.size)
    n1, n0 = int(one.sum()), int((~one).sum())
    max1 = int(mag[one].max(initial=0))
    max0 = int(mag[~one].max(initial=0))
    nonfinite = int((mag >= 0x7f800000).sum())
    status = 0
    max_exp = -100
    if nonfinite:
        status = NONFINITE                                      # the patterns say nothing about a range
    elif n1 == 0:
        pass                                                    # every weight is quantised: nothing to do
    elif max0 == 0:                                             # nothing, or only zeros, fixed so far: the float weights set the range
        if max1 == 0:
            status |= ALL_ZERO
        else:
            max_exp = int(exp_of_bits(max1))
    else:
        max_exp = int(exp2_of_bits(max0))                       # a power of two: the reference's round(log2)
        if max1 != 0 and int(exp_of_bits(max1)) > max_exp:
            status |= RANGE_GREW                                # the reference exits here
    return dict(n1=n1, n0=n0, max1=max1, max0=max0, nonfinite=nonfinite, max_exp=max_exp, min_exp=max_exp - int(n_values) + 1, status=status)


def codes_of(bits, one, min_exp: int) -> np.ndarray:
    """The 4-bit file's code per weight relative to min_exp (model4bit._codes_for): 15 still float, 7 zero, k = e - min_exp for a
    negative, k + 8 for a positive power of two; 15 where k is outside 0..6."""
    bits = np.asarray(bits, np.uint32)
    mag = bits & _MAG
    k = exp2_of_bits(mag) - int(min_exp)
    c = np.where(mag == 0, 7, np.where((k >= 0) & (k <= 6), k + np.where(bits >> 31, 0, 8), 15))
    return np.where(one, 15, c).astype(np.uint8)


def reference_step(w, mask, prev: float, cur: float, n_values: int = N_VALUES, exp_floor: int = -127):
    """One INQ step of one tensor: (weights float32, mask uint8, record STATE_DTYPE scalar, codes uint8), inputs untouched.
    ShapeIntoTwoPower behind ComputeQuantumRange, with the additions of the ABI: exp_floor, +0.0 for a selected zero, status bits that
    leave the tensor as it is, 2^127 for magnitudes of 1.5 * 2^127 and more."""
    _check_portions(prev, cur, n_values)
    shape = np.shape(w)
    bits = _bits(w).copy()
    mk = np.asarray(mask).ravel().astype(np.uint8).copy()
    one = mk != 0
    r = reference_range(bits.view(np.float32), mk, n_values)
    rec = np.zeros((), STATE_DTYPE)
    for k, v in r.items():
        rec[k] = v
    n1, min_exp = r["n1"], r["min_exp"]
    n_keep, n_update = n1, 0
    if not r["status"]:
        n_init = round(float(n1) / (1.0 - prev))               # Python's round: half to even, as rint
        n_keep = round(float(n_init) * (1.0 - cur))
        n_update = n1 - n_keep
    rec["n_keep"], rec["n_update"] = n_keep, n_update
    mag = bits & _MAG
    if not r["status"] and n_update > 0:
        thr = np.sort(mag[one])[n_keep]
        rec["thr"] = int(thr)
        sel = one & (mag >= thr)
        e = np.minimum(exp_of_bits(mag), 127)
        nz = sel & (mag != 0)
        fmin = nz & (e < min_exp)
        ffloor = nz & ~fmin & (e < exp_floor)
        emit = nz & ~fmin & ~ffloor
        rec["flushed_min"], rec["flushed_floor"], rec["over_one"] = int(fmin.sum()), int(ffloor.sum()), int((emit & (e > 0)).sum())
        sign = bits & np.uint32(0x80000000)
        bits[sel] = 0
        bits[emit] = sign[emit] | pow2_bits(e[emit])
        mk[sel] = 0
        one = mk != 0
    codes = codes_of(bits, one, min_exp)
    rec["hist"] = np.bincount(codes, minlength=16)
    return bits.view(np.float32).reshape(shape), mk.reshape(shape), rec, codes.reshape(shape)


# ---- a model stream ------------------------------------------------------------------------------------------------------------
def segments_of(tables, which: Sequence[str] = ("filter", "bias")) -> List[Tuple[str, int, int]]:
    """[(name, offset, count)] of the tensors INQ works on in a LoadModel stream: conv / FC filters and, as in the reference
    (compress_train_eval.py:64-76), their biases.  BN tensors and L2Norm weights are never segments."""
    bad = set(which) - {"filter", "bias"}
    if bad:
        raise ValueError(f"which: unknown kinds {sorted(bad)}")
    out, pos = [], 0
    for name, t, _ in split_model(tables, np.zeros(cfg.model_float_count(tables), np.float32)):
        if name.rsplit(".", 1)[1] in which:
            out.append((name, pos, int(t.size)))
        pos += int(t.size)
    return out


def reference_model_step(tables, model, mask, prev: float, cur: float, n_values: int = N_VALUES, exp_floor: int = -127,
                         which: Sequence[str] = ("filter", "bias")):
    """reference_step on every segment of a LoadModel stream: (stream, mask uint8 over the whole stream, records [n_segs], codes uint8
    over the whole stream, 0 outside the segments).  mask: uint8 over the stream, or None for "everything still float"."""
    model = np.ascontiguousarray(model, np.float32).ravel().copy()
    segs = segments_of(tables, which)
    mk = np.zeros(model.size, np.uint8)
    if mask is None:
        for _, o, n in segs:
            mk[o:o + n] = 1
    else:
        mk[:] = np.asarray(mask).ravel()
    codes = np.zeros(model.size, np.uint8)
    recs = np.zeros(len(segs), STATE_DTYPE)
    for i, (_, o, n) in enumerate(segs):
        model[o:o + n], mk[o:o + n], recs[i], codes[o:o + n] = reference_step(model[o:o + n], mk[o:o + n], prev, cur, n_values, exp_floor)
    return model, mk, recs, codes


# ---- the device -----------------------------------------------------------------------------------------------------------------
class DeviceQuantizer:
    """tf2_inq_step over the segments of a LoadModel stream (tables, which) or over an explicit table (segs = [(offset, count)],
    n_total): owns the state and scratch buffers, allocated on the first step's device.
      step(stream_dev, mask_dev, prev, cur, exp_floor=-127, codes=None, n_values=7)
                  one INQ step of every segment, in place, enqueued on the current stream.  stream_dev: float32 [n_total], mask_dev:
                  uint8 [n_total] (non-zero: still float), codes: uint8 [n_total] or None; contiguous torch tensors on one device.
      capture(...) the same call as a HIP graph over these buffers; returns the replay function (refill, replay).
      state()     one host copy of the records, a structured array [n_segs] of STATE_DTYPE."""

    def __init__(self, tables=None, which: Sequence[str] = ("filter", "bias"), segs=None, n_total: Optional[int] = None):
        from . import _lib
        if segs is None:
            named = segments_of(tables, which)
            self.names = [n for n, _, _ in named]
            segs = [(o, c) for _, o, c in named]
            n_total = cfg.model_float_count(tables)
        else:
            self.names = [f"seg{i}" for i in range(len(segs))]
        self.segs = [(int(o), int(c)) for o, c in segs]
        self.n_total = int(n_total)
        self._table = (_lib.InqSeg * max(len(self.segs), 1))(*[_lib.InqSeg(o, c) for o, c in self.segs])
        self.state_size = int(_lib.lib().tf2_inq_state_size(len(self.segs)))
        self.scratch_size = int(_lib.lib().tf2_inq_scratch_size(len(self.segs)))
        self.state_dev = self._scratch = None

    def step(self, stream_dev, mask_dev, prev: float, cur: float, exp_floor: int = -127, codes=None, n_values: int = N_VALUES) -> None:
        import torch
        from . import _lib
        dev = stream_dev.device
        assert stream_dev.dtype == torch.float32 and stream_dev.is_contiguous() and stream_dev.numel() == self.n_total, "stream_dev"
        assert mask_dev.dtype == torch.uint8 and mask_dev.is_contiguous() and mask_dev.numel() == self.n_total and mask_dev.device == dev, "mask_dev"
        if codes is not None:
            assert codes.dtype == torch.uint8 and codes.is_contiguous() and codes.numel() == self.n_total and codes.device == dev, "codes"
        if self.state_dev is None or self.state_dev.device != dev:
            self.state_dev = torch.zeros(max(self.state_size // 8, 1), dtype=torch.int64, device=dev)
            self._scratch = torch.empty(max(self.scratch_size // 8, 1), dtype=torch.int64, device=dev)
        hip_stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.lib().tf2_inq_step(stream_dev.data_ptr(), mask_dev.data_ptr(), self.n_total, self._table, len(self.segs),
                                           float(prev), float(cur), int(n_values), int(exp_floor),
                                           codes.data_ptr() if codes is not None else None, self.state_dev.data_ptr(),
                                           self._scratch.data_ptr(), self._scratch.numel() * 8, hip_stream))

    def capture(self, stream_dev, mask_dev, prev: float, cur: float, exp_floor: int = -127, codes=None, n_values: int = N_VALUES):
        """A HIP graph of step(...) on these buffers.  The warm-up call outside the capture is a real step: it changes stream_dev and
        mask_dev, so fill them before every replay."""
        from ._observe import capture_graph
        # (the warm-up: buffers allocated, kernels loaded)
        self._graph = capture_graph(lambda: self.step(stream_dev, mask_dev, prev, cur, exp_floor, codes, n_values), stream_dev.device)
        return self._graph.replay

    def state(self) -> np.ndarray:
        assert self.state_dev is not None, "no step yet"
        return self.state_dev.cpu().numpy()[:self.state_size // 8].view(STATE_DTYPE).copy()


# ---- a model in, a model out ------------------------------------------------------------------------------------------------------
def quantize_model(tables, model, schedule: Sequence[float] = (1.0,), exp_floor: int = -127, which: Sequence[str] = ("filter", "bias"),
                   device="cuda:0", between=None):
    """Float LoadModel stream -> (quantised stream float32, per-tensor report) on the device: one DeviceQuantizer.step per portion of
    `schedule` (ascending, ending at 1.0), prev = the portion before (0 at first).  between(stream_dev, mask_dev, step): the caller's
    retraining of the still-float weights between steps, on the device (None: the weights stay).  Raises if a tensor reports a status
    bit or the final mask is not all zero.  The report: [dict(name, offset, count, codes = the codes of the tensor, record fields)]."""
    import torch
    schedule = [float(p) for p in schedule]
    if not schedule or schedule[-1] != 1.0 or any(b < a for a, b in zip(schedule, schedule[1:])):
        raise ValueError(f"schedule {schedule} must ascend and end at 1.0")
    model = np.ascontiguousarray(model, np.float32).ravel()
    dq = DeviceQuantizer(tables, which)
    if model.size != dq.n_total:
        raise ValueError(f"model stream has {model.size} floats, the tables need {dq.n_total}")
    mk = np.zeros(model.size, np.uint8)
    for o, c in dq.segs:
        mk[o:o + c] = 1
    w_dev = torch.from_numpy(model.copy()).to(device)
    m_dev = torch.from_numpy(mk).to(device)
    c_dev = torch.zeros(model.size, dtype=torch.uint8, device=device)
    totals = np.zeros((len(dq.segs), 3), np.int64)
    prev = 0.0
    for i, cur in enumerate(schedule):
        dq.step(w_dev, m_dev, prev, cur, exp_floor=exp_floor, codes=c_dev)
        st = dq.state()
        bad = [(dq.names[j], int(s)) for j, s in enumerate(st["status"]) if s]
        if bad:
            raise ValueError(f"quantize_model: step {i} (portion {cur}): status bits set (1 range grew, 2 all zero, 4 non-finite): {bad}")
        totals += np.stack([st["flushed_min"], st["flushed_floor"], st["over_one"]], 1)
        prev = cur
        if between is not None and cur < 1.0:
            between(w_dev, m_dev, i)
    left = int(m_dev.count_nonzero().item())
    if left:
        raise ValueError(f"quantize_model: {left} weights are still float after the schedule {schedule}")
    out, codes = w_dev.cpu().numpy(), c_dev.cpu().numpy()
    rep = []
    for j, ((o, c), name) in enumerate(zip(dq.segs, dq.names)):
        r = {k: (st[k][j].copy() if k in ("hist", "reserved") else int(st[k][j])) for k in STATE_DTYPE.names}
        r.update(name=name, offset=o, count=c, codes=codes[o:o + c].copy(), flushed_min=int(totals[j, 0]), flushed_floor=int(totals[j, 1]),
                 over_one=int(totals[j, 2]))
        rep.append(r)
    return out, rep


def engine_check(tables, model) -> List[dict]:
    """What the engine's loader makes of a LoadModel stream, per filter: [dict(name, count, misfit, flushed, examples)].  misfit: weights
    `tf2_get_real` (the library's own, through the C ABI) decodes to another value -- non-zero weights that are not +-2^0 .. +-2^-14 are
    read as +-1; flushed: the misfits among them with |w| < 1e-5, read as 0.  examples: up to five misread values with what they become."""
    from . import _lib
    L = _lib.lib()
    out = []
    for name, t, is_filter in split_model(tables, model):
        if not is_filter:
            continue
        vals, counts = np.unique(t.ravel().view(np.uint32), return_counts=True)
        misfit = flushed = 0
        examples = []
        for b, n in zip(vals, counts):
            v = np.uint32(b).view(np.float32)
            code = int(L.tf2_get_real(float(v), 14))
            read = np.float32(0.0) if code == 0x40 else np.float32(np.ldexp(-1.0 if code & 0x80 else 1.0, (code & 0x3f) - 14))
            if not (read == v):                                  # (a NaN is a misfit too)
                misfit += int(n)
                flushed += int(n) if code == 0x40 else 0
                if len(examples) < 5:
                    examples.append((float(v), float(read)))
        out.append(dict(name=name, count=int(t.size), misfit=misfit, flushed=flushed, examples=examples))
    return out


def report(rep: Sequence[dict], check: Optional[Sequence[dict]] = None) -> str:
    """For people: per tensor max_exp, min_exp, the code histogram (codes 0..6 negative, 7 zero, 8..14 positive, 15 none), the share
    flushed to zero under min_exp / under exp_floor, the weights above 1, and (check = engine_check's result) the engine's misfits."""
    mis = {c["name"]: c for c in (check or [])}
    lines = []
    for r in rep:
        n = max(int(r["count"]), 1)
        h = " ".join(f"{int(v)}" for v in r["hist"])
        line = (f"{r['name']:<18s} n {r['count']:9d}  exp {int(r['max_exp']):4d}..{int(r['min_exp']):4d}  flushed {100.0 * r['flushed_min'] / n:6.2f}% min "
                f"{100.0 * r['flushed_floor'] / n:6.2f}% floor  >1: {int(r['over_one'])}  codes [{h}]")
        if r["name"] in mis:
            line += f"  engine misfits {mis[r['name']]['misfit']}"
        lines.append(line)
    return "\n".join(lines)
