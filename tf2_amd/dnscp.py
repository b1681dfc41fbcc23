"""DNS channel pruning: keep bytes per input channel, statistics, the pruned stream  (tf2_dnscp_*, include/tf2_amd.h; csrc/weight_dnscp.hip)

The reference makes a pruned network with TransForm_Kit/DnsChannelpruning: per iteration and conv `DnscpCore.maskChannelCalc`
(dnscp_core.py) prunes the INPUT channels whose mean magnitude lies under a threshold from the conv's own mean and deviation
(`cal_mean_std`), revives them above a higher one, and forces the kept count to a multiple of 16; `model_convert.py` then drops the
pruned input channels and the matching output channels of the conv in front.  This module is that rule:

  reference_stats / reference_step   the statement, in numpy, on float32 BIT PATTERNS with exact integer sums (torch's float32 sums
                                     have no defined order): equal to the reference's own masks on tests/golden/ref_dnscp.npz
                                     (tools/gen_dnscp_golden.py), whose inputs stay a relative 2^-10 clear of both thresholds
  thresholds                         mu, std and the two thresholds from the exact sums, in double, on the host
  reference_model_step               the same over a LoadModel stream
  prunable_rows / pruned_tables / pruned_q / reference_compact / kept_ratio / report    from keep bytes to an engine-ready network
  DevicePruner                       tf2_dnscp_stats / tf2_dnscp_step on torch tensors; equals reference_* as bits
  prune_model                        the export through tf2_dnscp_compact

Deviations from the reference, all stated in include/tf2_amd.h: a pruned weight is written as +0.0 (the reference's multiply by a zero
mask leaves -0.0 for a negative weight; `tf2_get_real` reads both as zero); sums are integers in a per-conv fixed point (m(a) =
floor(a * 2^(31 - E)), so a weight under 2^(E - 31) counts as 0 in S1, A1, A2 -- it still counts in nz); `kept_ratio` is N*C*k^2 and
that times OH*OW over the conv rows of the tables, not torchsummary's figures.

The record of a conv is 16 int64 (STATE_DTYPE): n, nz, nonfinite, max (pattern), E, A1, A2_hi, A2_lo, kept_before, pruned, revived,
fixup (+ revived, - pruned), kept_after, status, B_lo, B_hi.
"""
from __future__ import annotations

import math
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import config as cfg
from .inq import NO_EXP, exp2_of_bits
from .model4bit import split_model

UPDATE = 1                                         # flags (TF2_DNSCP_UPDATE)
ALL_ZERO, NONFINITE, NAN_THRESHOLD = 1, 2, 4       # status bits (TF2_DNSCP_*)
MAX_C = 4096
WORDS = 16
STATE_DTYPE = np.dtype([(n, "<i8") for n in ("n", "nz", "nonfinite", "max", "E", "A1", "A2_hi", "A2_lo", "kept_before", "pruned", "revived",
                                             "fixup", "kept_after", "status", "B_lo", "B_hi")])
assert STATE_DTYPE.itemsize == WORDS * 8
_MAG = np.uint32(0x7fffffff)
_INF = 0x7f800000
I64_MAX = (1 << 63) - 1


# ---- the statement ---------------------------------------------------------------------------------------------------------
def _conv_bits(w) -> np.ndarray:
    """[N, C, kk] uint32 patterns of a conv [N, C, k, k] (or [N, C, kk])"""
    w = np.ascontiguousarray(w, np.float32)
    if w.ndim not in (3, 4):
        raise ValueError(f"a conv is [N, C, k, k] or [N, C, kk], not {w.shape}")
    b = w.reshape(w.shape[0], w.shape[1], -1).view(np.uint32)
    N, C, kk = b.shape
    if C > MAX_C or N * kk >= 1 << 22 or N * C * kk >= 1 << 28:
        raise ValueError(f"conv {w.shape}: C <= 4096, N * kk < 2^22 and N * C * kk < 2^28 (exact sums)")
    return b


def fixed_of_bits(mag, E: int) -> np.ndarray:
    """m(a) = floor(a * 2^(31 - E)) of float32 magnitude patterns under the conv's E, int64 in 0 .. 2^32 - 1: a shift of the 24-bit
    significand (a denormal's by the same inequality); 0 for zero and for a non-finite pattern"""
    mag = np.asarray(mag).astype(np.int64)
    e = mag >> 23
    sig = np.where(e > 0, (mag & 0x7fffff) | 0x800000, mag)
    sh = np.where(e > 0, e - 127, -126) + 8 - int(E)
    m = np.where(sh >= 0, sig << np.clip(sh, 0, 31), sig >> np.clip(-sh, 0, 63))
    return np.where((mag == 0) | (mag >= _INF), 0, m)


def _keep_of(keep, C: int) -> np.ndarray:
    if keep is None:
        return np.ones(C, bool)
    k = np.asarray(keep).ravel() != 0
    assert k.size == C, (k.size, C)
    return k


def reference_stats(w, keep=None):
    """(S1 int64 [C], record) of one conv: the sums of tf2_dnscp_stats.  keep: bytes per input channel, None for all kept."""
    b = _conv_bits(w)
    N, C, kk = b.shape
    kp = _keep_of(keep, C)
    mag = b & _MAG
    fin = mag < _INF
    rec = np.zeros((), STATE_DTYPE)
    mx = int(mag[fin].max(initial=0))
    E = int(exp2_of_bits(mx))
    m = fixed_of_bits(mag, E)
    S1 = m.sum(axis=(0, 2)).astype(np.int64)
    mk = m[:, kp, :].astype(np.uint64)
    sq = mk * mk
    rec["n"], rec["nz"], rec["nonfinite"], rec["max"], rec["E"] = N * C * kk, int((mag[:, kp, :] != 0).sum()), int((~fin).sum()), mx, E
    rec["A1"], rec["A2_hi"], rec["A2_lo"] = int(mk.sum()), int((sq >> np.uint64(32)).sum()), int((sq & np.uint64(0xffffffff)).sum())
    rec["kept_before"] = rec["kept_after"] = int(kp.sum())
    rec["status"] = NONFINITE if rec["nonfinite"] else (ALL_ZERO if mx == 0 else 0)
    return S1, rec


def _thresholds_one(rec, c_rate: float, alpha_low: float, alpha_high: float) -> Tuple[float, float, float, float]:
    n, nz, E = int(rec["n"]), int(rec["nz"]), int(rec["E"])
    A1, A2 = int(rec["A1"]), (int(rec["A2_hi"]) << 32) + int(rec["A2_lo"])
    if nz == 0:
        return math.nan, math.nan, math.nan, math.nan              # the reference's 0 / 0
    k = max(E, -149) - 31                                           # the fixed point's unit is 2^k
    mu_i = float(Fraction(A1, nz))                                  # one rounding
    var_i = float((Fraction(A2) - n * Fraction(mu_i) ** 2) / n)     # one rounding, on the rounded mu as the reference's
    mu, var = math.ldexp(mu_i, k), math.ldexp(var_i, 2 * k)         # exact scalings
    std = math.sqrt(var) if var >= 0 else math.nan
    T = max(mu + float(c_rate) * std, 0.0)                          # Python's max: a NaN first argument stays
    return float(alpha_low) * T, float(alpha_high) * T, mu, std


def thresholds(stats, c_rate: float = 0.1, alpha_low: float = 0.95, alpha_high: float = 1.05, with_moments: bool = False):
    """(t_lo, t_hi) of a record or of an array of records -- cal_mean_std and the two products of maskChannelCalc, in the weights' units:
    mu = A1 / nz, var = (A2 - n mu^2) / n, std = sqrt(var) (NaN under 0), T = max(mu + c_rate * std, 0), t_lo = alpha_low * T, t_hi =
    alpha_high * T.  Double precision on the exact integers as Python ints, one rounding at each of mu, var, sqrt, the products and
    the sum.  with_moments: (t_lo, t_hi, mu, std)."""
    stats = np.asarray(stats)
    if stats.ndim == 0:
        r = _thresholds_one(stats, c_rate, alpha_low, alpha_high)
        return r if with_moments else r[:2]
    r = np.asarray([_thresholds_one(s, c_rate, alpha_low, alpha_high) for s in stats], np.float64).reshape(-1, 4)
    return tuple(r[:, i] for i in range(4 if with_moments else 2))


def bound_of(t: float, nkk: int, E: int, nan: int) -> int:
    """B = floor(t * double(N kk) * 2^(31 - max(E, -149))) clamped to [-1, 2^63 - 1]; `nan` for a NaN t"""
    t = float(t)
    if t != t:
        return int(nan)
    with np.errstate(over="ignore"):
        x = np.float64(t) * np.float64(nkk)                         # one IEEE multiply
        x = np.floor(x * np.float64(2.0) ** (31 - max(int(E), -149)))   # an exact scaling (or a result under 1, or inf)
    if x >= 9223372036854775808.0:
        return I64_MAX
    if x < -1.0:
        return -1
    return int(x)


def reference_step(w, keep, t_lo: float, t_hi: float, update: bool = True):
    """One DNS-CP step of one conv: (keep uint8 [C] as 0 / 1 where decided, masked weights float32, S1, record), inputs untouched."""
    b = _conv_bits(w)
    N, C, kk = b.shape
    shape = np.shape(w)
    if update and (t_lo < 0 or t_hi < 0):
        raise ValueError("thresholds must be >= 0 or NaN")
    S1, rec = reference_stats(w, keep)
    kp = np.asarray(keep, np.uint8).ravel().copy() if keep is not None else np.ones(C, np.uint8)
    old = kp != 0
    if update:
        rec["B_lo"], rec["B_hi"] = bound_of(t_lo, N * kk, int(rec["E"]), -1), bound_of(t_hi, N * kk, int(rec["E"]), I64_MAX)
        if t_lo != t_lo or t_hi != t_hi:
            rec["status"] |= NAN_THRESHOLD
    if int(rec["status"]) & NONFINITE:
        return kp, b.view(np.float32).reshape(shape).copy(), S1, rec     # left as it was (the caller's out keeps what it held)
    if update:
        prune = old & (S1 <= int(rec["B_lo"]))
        revive = ~old & (S1 > int(rec["B_hi"]))
        k1 = (old & ~prune) | revive
        nzc = int(k1.sum())
        target = 16 * round(nzc / 16) or 16                         # Python's round: half to even
        k2 = k1.copy()
        fix = 0
        if target > nzc:
            idx = np.flatnonzero(~k1)[:target - nzc]                # the loops simply run out where C is too small
            k2[idx] = True
            fix = int(idx.size)
        elif target < nzc:
            idx = np.flatnonzero(k1)[:nzc - target]
            k2[idx] = False
            fix = -int(idx.size)
        rec["pruned"], rec["revived"], rec["fixup"], rec["kept_after"] = int(prune.sum()), int(revive.sum()), fix, int(k2.sum())
        kp = k2.astype(np.uint8)
    out = np.where((kp != 0)[None, :, None], b, np.uint32(0))
    return kp, out.view(np.float32).reshape(shape), S1, rec


# ---- tables ----------------------------------------------------------------------------------------------------------------
def prunable_rows(tables) -> List[int]:
    """The consumer rows l whose input channels DNS-CP may prune -- find_dnscp_conv.py's flag rule on the tables: l is a conv row whose
    input is row p's output, and p is a conv row with no residual add that is no concat member, not the last row, and read (as data or
    as residual) by l alone.  Pruning l's input channel c then removes p's output channel c and nothing else."""
    plan = cfg.build_plan(tables)
    readers: Dict[int, List[int]] = {}
    for L in plan:
        for s in (L.src, L.add_src):
            if s >= 0:
                readers.setdefault(s, []).append(L.index)
    out = []
    for L in plan:
        p = L.src
        if L.ipool or p < 0:
            continue
        P = plan[p]
        if P.ipool or P.add_src >= 0 or P.concat >= 0 or p == len(plan) - 1 or readers.get(p) != [L.index]:
            continue
        out.append(L.index)
    return out


def _filter_layout(tables) -> Dict[int, Tuple[int, int, int, int]]:
    """{row: (offset, N, C, kk)} of the filters in the LoadModel stream"""
    out, pos = {}, 0
    for name, t, is_filter in split_model(tables, np.zeros(cfg.model_float_count(tables), np.float32)):
        if is_filter:
            out[int(name[5:].split(".")[0])] = (pos, t.shape[0], t.shape[1], t.shape[2] * t.shape[3])
        pos += int(t.size)
    return out


def _check_keeps(tables, keeps) -> Dict[int, np.ndarray]:
    plan = cfg.build_plan(tables)
    ok = set(prunable_rows(tables))
    out = {}
    for l, k in keeps.items():
        k = np.asarray(k).ravel() != 0
        if int(l) not in ok:
            raise ValueError(f"row {l} is not prunable (prunable_rows)")
        if k.size != plan[int(l)].C or not k.any():
            raise ValueError(f"row {l}: {k.size} keep bytes for {plan[int(l)].C} input channels, or none kept")
        out[int(l)] = k
    return out


def reference_model_step(tables, model, keeps, th, update: Optional[Sequence[int]] = None):
    """reference_step on the filter of every prunable row of a LoadModel stream: (masked stream, keeps {row: uint8 [C]}, S1 {row: int64},
    records [n_rows]).  keeps: {row: bytes} or None (all kept); th: {row: (t_lo, t_hi)}; update: the rows decided (None: all)."""
    model = np.ascontiguousarray(model, np.float32).ravel()
    out = model.copy()
    rows = prunable_rows(tables)
    lay = _filter_layout(tables)
    recs = np.zeros(len(rows), STATE_DTYPE)
    new, sums = {}, {}
    for i, l in enumerate(rows):
        o, N, C, kk = lay[l]
        upd = update is None or l in update
        t_lo, t_hi = th[l] if upd else (0.0, 0.0)
        new[l], w, sums[l], recs[i] = reference_step(model[o:o + N * C * kk].reshape(N, C, kk), None if keeps is None else keeps[l], t_lo, t_hi, upd)
        out[o:o + N * C * kk] = w.ravel()
    return out, new, sums, recs


def pruned_tables(tables, keeps):
    """A copy of the tables with kInputChannels[l] and kOutputChannels[p] = kNEnd[p] (p the row in front of l) set to the kept counts;
    everything else is unchanged."""
    keeps = _check_keeps(tables, keeps)
    plan = cfg.build_plan(tables)
    out = cfg.NetTables({k: (list(v) if isinstance(v, list) else v) for k, v in tables.items()})
    for l, k in keeps.items():
        n = int(k.sum())
        p = plan[l].src
        out["kInputChannels"][l] = n
        out["kOutputChannels"][p] = n
        out["kNEnd"][p] = n
    return out.validate()


def pruned_q(tables, keeps, q_vals) -> np.ndarray:
    """The Q file's values without those of the removed output channels."""
    keeps = _check_keeps(tables, keeps)
    plan = cfg.build_plan(tables)
    q_vals = np.asarray(q_vals).ravel()
    if q_vals.size != cfg.q_value_count(tables):
        raise ValueError(f"{q_vals.size} Q values, the tables need {cfg.q_value_count(tables)}")
    out_keep = {plan[l].src: k for l, k in keeps.items()}
    sel = np.ones(q_vals.size, bool)
    pos = 3
    for L in plan:
        if L.ipool == 1:
            continue
        if L.index in out_keep:
            sel[pos:pos + L.N] = out_keep[L.index]
        pos += L.N
    return q_vals[sel]


def compact_plan(tables, keeps) -> List[Tuple[str, int, Tuple[int, int, int], Optional[np.ndarray], Optional[np.ndarray]]]:
    """Per tensor of the LoadModel stream: (name, offset, (N, C, kk), kept n indices or None, kept c indices or None) --
    model_convert.py's clip_cin_channel on the pruned convs, clip_cout_channel on the conv in front and its bias, mean, var, gamma and
    beta; scale_factor and every other tensor whole."""
    keeps = _check_keeps(tables, keeps)
    plan = cfg.build_plan(tables)
    out_keep = {plan[l].src: np.flatnonzero(k).astype(np.int32) for l, k in keeps.items()}
    in_keep = {l: np.flatnonzero(k).astype(np.int32) for l, k in keeps.items()}
    out, pos = [], 0
    for name, t, is_filter in split_model(tables, np.zeros(cfg.model_float_count(tables), np.float32)):
        row, kind = int(name[5:].split(".")[0]), name.rsplit(".", 1)[1]
        n_idx = out_keep.get(row) if kind in ("filter", "bias", "mean", "var", "gamma", "beta") else None
        c_idx = in_keep.get(row) if is_filter else None
        out.append((name, pos, (t.shape[0], t.shape[1], t.shape[2] * t.shape[3]), n_idx, c_idx))
        pos += int(t.size)
    return out


def reference_compact(tables, keeps, model) -> np.ndarray:
    """The pruned LoadModel stream of pruned_tables(tables, keeps), in numpy."""
    model = np.ascontiguousarray(model, np.float32).ravel()
    if model.size != cfg.model_float_count(tables):
        raise ValueError(f"model stream has {model.size} floats, the tables need {cfg.model_float_count(tables)}")
    parts = []
    for _, o, (N, C, kk), n_idx, c_idx in compact_plan(tables, keeps):
        t = model[o:o + N * C * kk].reshape(N, C, kk)
        if n_idx is not None:
            t = t[n_idx]
        if c_idx is not None:
            t = t[:, c_idx]
        parts.append(t.ravel())
    return np.concatenate(parts)


def kept_ratio(tables, keeps) -> Tuple[float, float]:
    """(params kept, MACs kept) of the pruned network over the conv rows of the tables: params = N * C * k^2 and macs = params * OH * OW
    per row.  This project's definition, not torchsummary's (which the reference's calculate_compress_rate prints)."""
    def tot(t):
        rows = [L for L in cfg.build_plan(t) if not L.ipool]
        return (sum(L.N * L.model_C * L.model_k ** 2 for L in rows), sum(L.N * L.model_C * L.model_k ** 2 * L.OH * L.OW for L in rows))
    (p0, m0), (p1, m1) = tot(tables), tot(pruned_tables(tables, keeps))
    return p1 / p0, m1 / m0


def report(tables, keeps, recs=None) -> str:
    """For people: per pruned row the input width before and after, the row in front, and the network's kept ratios; recs (records in
    prunable_rows order) adds what the last step did."""
    plan = cfg.build_plan(tables)
    rows = prunable_rows(tables)
    lines = []
    for l in sorted(keeps):
        k = np.asarray(keeps[l]).ravel() != 0
        line = f"row {l:3d} (in front: row {plan[l].src:3d})  C {k.size:5d} -> {int(k.sum()):5d}  {100.0 * k.sum() / k.size:6.2f}%"
        if recs is not None and l in rows:
            r = recs[rows.index(l)]
            line += f"  pruned {int(r['pruned'])} revived {int(r['revived'])} fix-up {int(r['fixup']):+d} status {int(r['status'])}"
        lines.append(line)
    p, m = kept_ratio(tables, keeps)
    lines.append(f"conv params kept {100.0 * p:.2f}%  conv MACs kept {100.0 * m:.2f}%  (N*C*k^2 and that times OH*OW, over the tables' conv rows)")
    return "\n".join(lines)


# ---- the device -----------------------------------------------------------------------------------------------------------------
class DevicePruner:
    """tf2_dnscp_stats / tf2_dnscp_step over the prunable filters of a LoadModel stream (tables) or over an explicit table
    (convs = [(offset, N, C, kk)], n_total): owns the keep bytes (all kept at first), S1, the records and the thresholds.
      stats(weights_dev)          the record and S1 of every conv under the current keep bytes
      thresholds(c_rate, alpha_low, alpha_high)   reads the records once and sets (t_lo, t_hi) of every conv from them; returns them
      set_thresholds(t_lo, t_hi)  the same from the caller's own numbers (arrays over the convs)
      step(dense_dev, out_dev, update=None)   one step, enqueued on the current stream: the convs in `update` (conv ids: table rows, or
                                  indices of an explicit table; None: all) are decided, every conv's keep bytes applied.  out_dev may be dense_dev.
      capture(dense_dev, out_dev, update=None)   the same call as a HIP graph over these buffers; returns the replay function
      keeps() / set_keep(keeps)   {conv id: uint8 [C]} from / to the device;  sums()  {conv id: int64 [C]};  state()  records [n_convs]"""

    def __init__(self, tables=None, convs=None, n_total: Optional[int] = None):
        from . import _lib
        if convs is None:
            lay = _filter_layout(tables)
            self.ids = prunable_rows(tables)
            convs = [lay[l] for l in self.ids]
            n_total = cfg.model_float_count(tables)
        else:
            self.ids = list(range(len(convs)))
        self.convs = [tuple(int(v) for v in c) for c in convs]
        self.n_total = int(n_total)
        self.keep_off = np.concatenate([[0], np.cumsum([c[2] for c in self.convs])]).astype(np.int64)
        self.n_channels = int(self.keep_off[-1])
        self._table = (_lib.DnscpConv * max(len(self.convs), 1))(*[_lib.DnscpConv(o, N, C, kk, 0, int(ko), 0.0, 0.0)
                                                                  for (o, N, C, kk), ko in zip(self.convs, self.keep_off)])
        self.state_size = int(_lib.lib().tf2_dnscp_state_size(len(self.convs)))
        self.keep_dev = self.sums_dev = self.state_dev = None

    def _buffers(self, dev):
        import torch
        if self.state_dev is None or self.state_dev.device != dev:
            self.keep_dev = torch.ones(max(self.n_channels, 1), dtype=torch.uint8, device=dev)
            self.sums_dev = torch.zeros(max(self.n_channels, 1), dtype=torch.int64, device=dev)
            self.state_dev = torch.zeros(max(self.state_size // 8, 1), dtype=torch.int64, device=dev)

    def _check(self, t, name):
        import torch
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == self.n_total, name

    def stats(self, weights_dev) -> None:
        import torch
        from . import _lib
        self._check(weights_dev, "weights_dev")
        self._buffers(weights_dev.device)
        for d in self._table:
            d.flags = 0
        _lib.check(_lib.lib().tf2_dnscp_stats(weights_dev.data_ptr(), self.n_total, self._table, len(self.convs), self.keep_dev.data_ptr(),
                                              self.n_channels, self.sums_dev.data_ptr(), self.state_dev.data_ptr(), None, 0,
                                              torch.cuda.current_stream(weights_dev.device).cuda_stream))

    def thresholds(self, c_rate: float = 0.1, alpha_low: float = 0.95, alpha_high: float = 1.05):
        t_lo, t_hi = thresholds(self.state(), c_rate, alpha_low, alpha_high)
        self.set_thresholds(t_lo, t_hi)
        return t_lo, t_hi

    def set_thresholds(self, t_lo, t_hi) -> None:
        for d, a, b in zip(self._table, np.asarray(t_lo, np.float64).ravel(), np.asarray(t_hi, np.float64).ravel()):
            d.t_lo, d.t_hi = float(a), float(b)

    def step(self, dense_dev, out_dev, update: Optional[Sequence[int]] = None) -> None:
        import torch
        from . import _lib
        self._check(dense_dev, "dense_dev")
        self._check(out_dev, "out_dev")
        assert out_dev.device == dense_dev.device, "out_dev"
        self._buffers(dense_dev.device)
        if update is not None and set(update) - set(self.ids):
            raise ValueError(f"update: unknown conv ids {sorted(set(update) - set(self.ids))}")
        for d, i in zip(self._table, self.ids):
            d.flags = UPDATE if update is None or i in update else 0
        _lib.check(_lib.lib().tf2_dnscp_step(dense_dev.data_ptr(), out_dev.data_ptr(), self.n_total, self._table, len(self.convs),
                                             self.keep_dev.data_ptr(), self.n_channels, self.sums_dev.data_ptr(), self.state_dev.data_ptr(),
                                             None, 0, torch.cuda.current_stream(dense_dev.device).cuda_stream))

    def capture(self, dense_dev, out_dev, update: Optional[Sequence[int]] = None):
        """A HIP graph of step(...) on these buffers.  The warm-up call outside the capture is a real step: it changes the keep bytes
        (and dense_dev where out_dev is dense_dev), so set them before every replay."""
        from ._observe import capture_graph
        # (the warm-up: buffers allocated, kernels loaded)
        self._graph = capture_graph(lambda: self.step(dense_dev, out_dev, update), dense_dev.device)
        return self._graph.replay

    def _split(self, flat) -> dict:
        return {i: flat[a:b].copy() for i, a, b in zip(self.ids, self.keep_off[:-1], self.keep_off[1:])}

    def keeps(self) -> Dict[int, np.ndarray]:
        assert self.keep_dev is not None, "no call yet"
        return self._split(self.keep_dev.cpu().numpy())

    def sums(self) -> Dict[int, np.ndarray]:
        assert self.sums_dev is not None, "no call yet"
        return self._split(self.sums_dev.cpu().numpy())

    def set_keep(self, keeps, device="cuda:0") -> None:
        import torch
        self._buffers(torch.device(device) if self.state_dev is None else self.state_dev.device)
        flat = self.keep_dev.cpu().numpy()
        for i, k in keeps.items():
            j = self.ids.index(i)
            k = np.asarray(k, np.uint8).ravel()
            assert k.size == self.convs[j][2], (i, k.size)
            flat[self.keep_off[j]:self.keep_off[j + 1]] = k
        self.keep_dev.copy_(torch.from_numpy(flat))

    def state(self) -> np.ndarray:
        assert self.state_dev is not None, "no call yet"
        return self.state_dev.cpu().numpy()[:self.state_size // 8].view(STATE_DTYPE).copy()


def compact_segments(plan):
    """(segment tuples (src_off, dst_off, n_src, c_src, n_out, c_out, kk, n_idx, c_idx), index list int32, n_dst) of a compact_plan for
    tf2_dnscp_compact; neighbouring whole tensors travel as one segment"""
    segs, idx, dst = [], [], 0
    n_at = 0
    for _, o, (N, C, kk), n_idx, c_idx in plan:
        if n_idx is None and c_idx is None:
            cnt = N * C * kk                                        # a whole tensor travels as [cnt][1][1]
            s = segs[-1] if segs else None
            if s is not None and s[7] < 0 and s[8] < 0 and s[0] + s[2] == o and s[2] + cnt < 1 << 30:
                segs[-1] = (s[0], s[1], s[2] + cnt, 1, s[4] + cnt, 1, 1, -1, -1)
            else:
                segs.append((o, dst, cnt, 1, cnt, 1, 1, -1, -1))
            dst += cnt
            continue
        n_o = c_o = -1
        if n_idx is not None:
            n_o = n_at; idx.append(n_idx); n_at += n_idx.size
        if c_idx is not None:
            c_o = n_at; idx.append(c_idx); n_at += c_idx.size
        n_out, c_out = (N if n_idx is None else n_idx.size), (C if c_idx is None else c_idx.size)
        segs.append((o, dst, N, C, n_out, c_out, kk, n_o, c_o))
        dst += n_out * c_out * kk
    return segs, (np.concatenate(idx).astype(np.int32) if idx else np.zeros(0, np.int32)), dst


def prune_model(tables, model, q_vals, keeps, device="cuda:0"):
    """(pruned tables, pruned LoadModel stream float32, pruned Q values) -- the export on the device through tf2_dnscp_compact.
    keeps: {row: keep bytes}, or a DevicePruner built from these tables (its keep bytes are read once)."""
    import torch
    from . import _lib
    if isinstance(keeps, DevicePruner):
        keeps = keeps.keeps()
    keeps = {l: k for l, k in _check_keeps(tables, keeps).items()}
    model = np.ascontiguousarray(model, np.float32).ravel()
    if model.size != cfg.model_float_count(tables):
        raise ValueError(f"model stream has {model.size} floats, the tables need {cfg.model_float_count(tables)}")
    t2 = pruned_tables(tables, keeps)
    segs, idx, n_dst = compact_segments(compact_plan(tables, keeps))
    assert n_dst == cfg.model_float_count(t2), (n_dst, cfg.model_float_count(t2))
    src = torch.from_numpy(model).to(device)
    dst = torch.empty(n_dst, dtype=torch.float32, device=device)
    idx_dev = torch.from_numpy(idx).to(device) if idx.size else None
    table = (_lib.DnscpSeg * len(segs))(*[_lib.DnscpSeg(s[0], s[1], s[2], s[3], s[4], s[5], s[6], 0, s[7], s[8]) for s in segs])
    _lib.check(_lib.lib().tf2_dnscp_compact(src.data_ptr(), src.numel(), dst.data_ptr(), n_dst, table, len(segs),
                                            idx_dev.data_ptr() if idx_dev is not None else None, int(idx.size),
                                            torch.cuda.current_stream(src.device).cuda_stream))
    return t2, dst.cpu().numpy(), pruned_q(tables, keeps, q_vals)
