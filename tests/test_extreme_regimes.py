"""The extreme-regime models (tf2_amd/synth.py synth_extreme) reach the edges they are named after, and the packed image computes the
oracle's layers there.

The plain high-precision reference: every targeted layer's accumulator in int64 (numpy, from the oracle's own filter codes and the
oracle's input to that layer: x * (+-2^shift), the -128 negate quirk of pe.cl:32-37 kept), then the reference's requantisation steps
without any clamp.  From it, per layer: the share of accumulators outside int32 (wrapped), of outputs clipped at 127 / -128, of
generic-form x + 2^14 that saturates -- and from the packed image (tests/emu_packed.parse) the exponent windows, the epilogue form
(fast: 0 generic, 1 FAST, 2 SEMI) and the dual form, and for a two-window row the per-channel dshift and the share of outputs whose
int64 high-window sum shifted by it leaves int32 (two_window_stats).  The assertions pin each regime to its target, so that an edit to
a generator cannot quietly make it benign again."""
import hashlib
import os

import numpy as np
import pytest

from oracle import netref, oracle as O
from tf2_amd import config as cfg, network, synth
from tests import emu_packed as emu
from tests.test_pack_emulation import check_net


def conv_int64(x, codes, stride, pad, dil=1):
    """x int8 [B, C, H, W], codes uint8 [N, C, k, k] -> exact sum of MUL terms, int64 [B, N, OH, OW] (no bias)."""
    B, C, H, W = x.shape
    N, _, k, _ = codes.shape
    OH = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    zero = (codes & 0x40) != 0
    mag = np.where(zero, 0, np.left_shift(np.int64(1), (codes & 0x1f).astype(np.int64)))
    neg = (codes & 0x80) != 0
    wp = np.where(neg, 0, mag).reshape(N, -1)                      # [N, C*k*k]
    wn = np.where(neg, mag, 0).reshape(N, -1)
    xp = np.zeros((B, C, H + 2 * pad, W + 2 * pad), np.int64)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    xn = (-xp).astype(np.int8).astype(np.int64)                    # (int8)(-x): -(-128) stays -128
    cols, ncols = [], []
    for c in range(C):
        for fh in range(k):
            for fw in range(k):
                sl = (slice(None), c, slice(fh * dil, fh * dil + stride * OH, stride), slice(fw * dil, fw * dil + stride * OW, stride))
                cols.append(xp[sl][:, :OH, :OW].reshape(B, -1)); ncols.append(xn[sl][:, :OH, :OW].reshape(B, -1))
    X = np.stack(cols, 1)                                          # [B, K, P]
    XN = np.stack(ncols, 1)
    acc = np.einsum("nk,bkp->bnp", wp, X) + np.einsum("nk,bkp->bnp", wn, XN)
    return acc.reshape(B, N, OH, OW)


def wrap32(a):
    return (a + 2 ** 31) % 2 ** 32 - 2 ** 31


def layer_stats(R, outs, pls, L, blob=None):
    """Exact int64 statistics of one conv row (plain form: no rewritten first layer); with the packed image `blob`, a two-window MFMA
    row's statistics too (two_window_stats)."""
    x = outs[L.src]
    codes = R.codes[L.index]
    bias, alpha, beta = (v.astype(np.int64) for v in R.bn[L.index])
    acc64 = conv_int64(x, codes, L.stride, L.pad_h, L.dil) + bias[None, :, None, None]
    got = np.stack([O.conv(xi, codes, R.bn[L.index][0], L.stride, L.pad_h, L.dil) for xi in x])
    np.testing.assert_array_equal(got, wrap32(acc64), err_msg=f"oracle conv vs wrap32(int64) at layer {L.index}")
    v = wrap32(acc64)
    xq = wrap32(((v * alpha[None, :, None, None]) >> 20) + beta[None, :, None, None])
    y = ((xq >> 14) + 1) >> 1                                      # the reference's rounding, before the clamp
    pl = pls[L.index]
    st = dict(wrapped=float((acc64 != v).mean()), hi=float((y > 127).mean()), lo=float((y < -128).mean()),
              sat14=float((xq + 2 ** 14 > 2 ** 31 - 1).mean()), windows=int(pl["n_phases"]), fast=int(pl["fast"]),
              dual=int(pl["dual"]), max_shift=int(pl["max_shift"]), kind=int(pl["kind"]))
    if blob is not None and st["kind"] == 1 and st["windows"] == 2:
        st.update(two_window_stats(blob, pl, x, codes, L))
    return st


def two_window_stats(blob, pl, x, codes, L):
    """A two-window row: the per-channel dshift of the packed image (dshift[1][n]: what the kernels shift the high window's sum by)
    and the share of outputs whose EXACT int64 high-window sum, shifted by it, leaves int32 (hi << dshift wraps before the low window
    is added).  The window split is restated from the codes (head of weight_pack.cpp): per output channel a window covers 7 exponents,
    taken from the top down -- the high window is [top - 6, top] for the channel's largest shift `top`, the low one [top2 - 6, top2]
    for the largest shift below it, values are relative to the window's base, dshift is the distance of the bases."""
    N = L.N
    sh = (codes & 0x1f).astype(np.int64).reshape(N, -1)
    nz = ((codes & 0x40) == 0).reshape(N, -1)
    top = np.where(nz, sh, -1).max(1)                               # (-1: an all-zero row)
    lo0 = np.maximum(top - 6, 0)
    in_hi = nz & (sh >= lo0[:, None])
    top2 = np.where(nz & ~in_hi, sh, -1).max(1)
    lo1 = np.where(top2 >= 0, np.maximum(top2 - 6, 0), lo0)         # (a row with one window repeats it: shift 0)
    dsh = emu.i32(blob, int(pl["off_dshift"]), 2 * int(pl["Np"])).reshape(2, -1)[1, :N].astype(np.int64)
    np.testing.assert_array_equal(dsh, np.where(top >= 0, lo0 - lo1, 0), err_msg=f"dshift of the packed image vs the codes' windows, layer {L.index}")
    rel = np.where(in_hi, sh - lo0[:, None], 0).reshape(codes.shape).astype(np.uint8)
    hi_codes = np.where(in_hi.reshape(codes.shape), (codes & 0xc0) | rel, 0x40).astype(np.uint8)      # the high window alone, shifts relative to its base
    hi64 = conv_int64(x, hi_codes, L.stride, L.pad_h, L.dil)
    assert np.abs(hi64).max() < 2 ** 31                             # (the sum itself is an int32: only the shift takes it out)
    sh64 = hi64 << dsh[None, :, None, None]
    return dict(dshift=dsh, hi_shift_wraps=float((sh64 != wrap32(sh64)).mean()), hi_sum_log2=float(np.log2(max(1, np.abs(hi64).max()))))


def regime_stats(t, q, model, x, rows, mode=0):
    net = network.NetWork(t)
    net.Quantization(synth.q_text(q)); net.LoadModel(model); net.Pack(mode)
    blob = net.packed_host()
    _, pls = emu.parse(blob)
    R = netref.RefNet(t, q, model)
    outs = R.run(x)
    return {l: layer_stats(R, outs, pls, R.plan[l], blob) for l in rows}, R, outs


TINY_ROWS = [1, 2, 3, 4, 5, 6, 7]


def _tiny(regime, seed=5):
    t = cfg.tiny_tables()
    q, model = synth.synth_extreme(t, seed, regime)
    return t, q, model, synth.synth_extreme_images(t, 3, seed)


def test_generators_leave_the_plain_ones_alone():
    """synth_model / synth_q_values are what bench.py, the goldens and the other tests are built on: the extreme generators add, they do
    not change them (the same seed gives the same bytes before and after a synth_extreme call)."""
    t = cfg.tiny_tables()
    q0 = synth.synth_q_values(t, 5, spread=2); m0 = synth.synth_model(t, q0, 5)
    synth.synth_extreme(t, 5, "wrap")
    assert (synth.synth_q_values(t, 5, spread=2) == q0).all() and synth.synth_model(t, q0, 5).tobytes() == m0.tobytes()
    a = synth.synth_extreme(t, 5, "spread"); b = synth.synth_extreme(t, 5, "spread")
    assert (a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes()
    # a regime added later leaves the earlier ones alone: the wrap model's bytes (Q values, then the float32 stream) as they were before
    # wrap2 joined EXTREME_REGIMES -- the digest was taken from the generator of that commit -- and unchanged by a wrap2 call in between
    before = "6e2a27924d5046be69333505169c31a27967c75655036f04a1a0162d270faeb9"
    for _ in range(2):
        w = synth.synth_extreme(t, 5, "wrap")
        assert hashlib.sha256(w[0].tobytes() + w[1].tobytes()).hexdigest() == before
        synth.synth_extreme(t, 5, "wrap2")


def test_wrap2_regime_wraps_two_window_rows():
    """The tiny net in the wrap2 regime: every targeted row packs as a two-window dual row; the boosted ones (rows 1, 2, 4, 6: shifts of 20
    and more, the others read a boosted tensor and drop their Q) have their windows 9 and more exponents apart on most channels, and a
    generic (row 1) and a SEMI one (row 2) wrap the final accumulator.  (Measured: 0.104 / 0.189 of the outputs of rows 1 / 2; dshift
    11 .. 14 on every channel of the boosted rows.  The tiny net's K is too short for hi << dshift itself to leave int32: that is
    pinned on ResNet-50 below.)"""
    t, q, model, x = _tiny("wrap2")
    st, _, _ = regime_stats(t, q, model, x, TINY_ROWS)
    boosted = [l for l in TINY_ROWS if st[l]["max_shift"] >= 20]
    assert boosted == [1, 2, 4, 6], st
    for l in TINY_ROWS:
        assert st[l]["windows"] == 2 and st[l]["dual"] == 1, (l, st[l])
    for l in boosted:
        assert (st[l]["dshift"] >= 9).mean() >= 0.9, (l, st[l]["dshift"])
    assert st[1]["fast"] == 0 and st[2]["fast"] == 2, st
    assert st[1]["wrapped"] >= 0.1 and st[2]["wrapped"] >= 0.1, st


def test_wrap_regime_wraps_and_takes_semi_and_generic():
    t, q, model, x = _tiny("wrap")
    st, R, _ = regime_stats(t, q, model, x, TINY_ROWS)
    # rows whose input Q is not itself boosted: shifts of 22-26, the accumulator wraps on a large share of the outputs -- row 1 (odd:
    # scales >= 1) in the generic form, row 2 (even: scales 2^-9 .. 2^-7 on every channel) in the SEMI form
    assert st[1]["wrapped"] >= 0.1 and st[2]["wrapped"] >= 0.1, st
    assert st[1]["fast"] == 0 and st[2]["fast"] == 2, st
    assert any(s["hi"] > 0.05 and s["lo"] > 0.05 for s in st.values()), st


def test_expand32_regime_masks_the_shift():
    """expand = 32 on channel 0 of the targeted rows: magnitude-1 weights encode as 0x20 (shift 0 after pe.cl's & 0x1f), and the packed
    image computes the oracle's layers (tests/test_pack_emulation.check_net, modes 0 and 2)."""
    t, q, model, x = _tiny("expand32")
    R = netref.RefNet(t, q, model)
    codes = R.codes[2]
    c0 = codes[:, 0][(codes[:, 0] & 0x40) == 0]
    assert ((c0 & 0x3f) == 0x20).any(), np.unique(c0)                 # (levels 1-3 give codes 31 .. 29)
    for mode in (0, 2):
        check_net(t, q, model, x, mode)


def test_saturate_regime_clips_both_ends_and_saturates_x():
    t, q, model, x = _tiny("saturate")
    st, R, outs = regime_stats(t, q, model, x, TINY_ROWS)
    for l in TINY_ROWS:
        assert st[l]["hi"] > 0.1, (l, st[l])
        assert st[l]["sat14"] > 0.05, (l, st[l])                  # the all-zero rows with beta at 2^31 - 2^13
    assert all(st[l]["lo"] > 0.1 for l in (1, 4, 7)), st          # rows without ReLU
    assert all(s["fast"] == 0 for s in st.values()), st            # beta near 2^31: neither FAST nor SEMI
    # residual sums clip at both ends: y far below -128 on the RNN rows (4 and 7: no ReLU, post-ReLU residual, add_relu)
    for l in (4, 7):
        L = R.plan[l]
        y = outs[l].astype(np.int64)
        assert (y == 0).mean() > 0.3 and (y == 127).mean() > 0.02, (l, (y == 0).mean(), (y == 127).mean())
    assert sum((outs[l] == 127).mean() for l in TINY_ROWS) / len(TINY_ROWS) > 0.1


def test_spread_regime_needs_three_to_five_windows():
    t, q, model, x = _tiny("spread")
    st, R, _ = regime_stats(t, q, model, x, TINY_ROWS)
    w = [s["windows"] for s in st.values()]
    assert max(w) >= 4 and sum(3 <= v <= 5 for v in w) >= 3, st
    codes = R.codes[3]
    assert ((codes[1] & 0x40) != 0).all() and ((codes[0] & 0x40) == 0).sum() == 1    # all-zero row, one-tap row


def test_spread_regime_dual_and_empty_phases_on_resnet50(golden_dir):
    """ResNet-50 rows 14 and 30 (3x3; rows 64..127 low levels only: rows with fewer windows than their layer): 3-5 windows; the row
    behind a targeted one keeps two windows (dual form)."""
    t = cfg.resnet50_tables()
    q, model = synth.synth_extreme(t, 0, "spread", rows={14, 30})
    net = network.NetWork(t)
    net.Quantization(synth.q_text(q)); net.LoadModel(model); net.Pack(0)
    _, pls = emu.parse(net.packed_host())
    assert 3 <= int(pls[14]["n_phases"]) <= 5 and 3 <= int(pls[30]["n_phases"]) <= 5, (pls[14]["n_phases"], pls[30]["n_phases"])
    assert int(pls[15]["n_phases"]) == 2 and int(pls[15]["dual"]) == 1


@pytest.mark.parametrize("regime,top", [("shift22", 22), ("shift23", 23)])
def test_shift_boundary_regimes(regime, top):
    """conv_shift.hip switches from v_mad_i32_i24 to a 32-bit multiply above max_shift 22 (net_plan.hip): the layers' largest shift is
    exactly 22 / 23 in mode 2."""
    t, q, model, x = _tiny(regime)
    st, _, _ = regime_stats(t, q, model, x, TINY_ROWS, mode=2)
    assert all(s["kind"] == 2 for s in st.values())
    assert sum(s["max_shift"] == top for s in st.values()) >= 3, {l: s["max_shift"] for l, s in st.items()}


def r50_all_rows():
    return {L.index for L in cfg.build_plan(cfg.resnet50_tables()) if not L.ipool}


def test_resnet50_wrap_rows_semi_and_generic(golden_dir):
    """ResNet-50 with every row in the wrap regime: layers with an even index take the SEMI form, odd ones the generic form, and both
    wrap the accumulator on a large share of the outputs -- on rows the ring, split-K, pointwise and fused kernels run (R50_ROUTES).
    oracle.conv equals wrap32 of the int64 sums there."""
    t = cfg.resnet50_tables()
    q, model = synth.synth_extreme(t, 0, "wrap", rows=r50_all_rows())
    x = synth.synth_extreme_images(t, 1, 0)
    rows = [3, 8, 14, 16, 19, 28, 31]
    st, _, _ = regime_stats(t, q, model, x, rows)
    for l in rows:
        assert st[l]["wrapped"] >= 0.01 and st[l]["fast"] == (2 if l % 2 == 0 else 0), (l, st[l])
    assert sum(st[l]["wrapped"] > 0.1 for l in rows) >= 5, st


# ResNet-50 routes of the GPU cases (tests/test_gpu_extremes.py), per regime: options, batch, concurrency and {kernel name prefix: rows
# of the extreme model that launches of that kernel must cover}.  Wrap rows with an even index are SEMI rows (above).  Routes a regime
# lacks select no launch of their kernel for that model: see SATURATE_NOT_SELECTED / SPREAD_NOT_SELECTED.
_BGROUP = dict(bgroup="1", bgroup_min7="1", bgroup_min14="1", bgroup_min28="1", bgroup_min56f="1", bfirst="1", alt_conc="0")
_WRAP = {
    "default": (dict(), 2, 0, {"conv_stem": {0}, "conv_mfma2_kernel": {3, 8}, "conv_mfma2_pair": {11, 12}, "conv_mfma_sk_kernel": {16, 19}}),
    "bneck": (dict(bneck_min="1"), 2, 0, {"conv_bneck": {16, 19}}),
    "bgroup": (_BGROUP, 2, 0, {"conv_bgroup56f": {3}, "conv_bgroup28": {16, 19}, "conv_bgroup_kernel": {28, 31}, "conv_bgroup7": {48}}),
    "bgroup_chain1": (dict(_BGROUP, bgroup_chain="1"), 2, 0, {"conv_bgroup_kernel": {28, 31}}),
    "bband": (dict(bband="2", bband_min="1"), 2, 0, {"conv_bband": {28, 31}}),
    "bfirst": (dict(bfirst="2", bfirst_min="1", alt_conc="0"), 2, 0, {"conv_bfirst": {3}}),
    "pwk": (dict(pwk="2", pwk_minpix="0", pwk_units="0", pwk_slabs="8", alt_conc="0"), 2, 0, {"conv_pwk_kernel": {5, 8}, "conv_pwk_pair": {11, 12}}),
    "pw": (dict(pw_slabs="2", pw_minpix="0"), 2, 0, {"conv_pw_kernel": {14}}),
    "sk": (dict(sk="1"), 2, 0, {"conv_mfma_sk_kernel": {3, 8, 14}}),
    "nofuse": (dict(nofuse="1"), 2, 0, {"conv_mfma2_kernel": {3, 5, 8}}),
    # conv_img.hip one batch at a time (its default is batches in flight, from batch 8 on): stage 5's 3x3 rows; batch 3 = one full
    # two-image block and the one-image tail block
    "img": (dict(img="2", img_min="1", alt_conc="0"), 3, 0, {"conv_img_kernel": {48, 51}}),
}
SATURATE_NOT_SELECTED = ("bband", "bfirst", "bgroup_chain1")      # (and the 56 x 56 / 14 x 14 group kernels of the bgroup route)
_BBAND28 = dict(bband="2", bband_min="1", bband_rows_alone="7")   # (stage 3's 28 x 28 bands come in 7 or 4 rows: conv_bband_shape_ok)
# wrap2: a route's fifth entry names the model (R50_MODELS) whose rows= set places wrapped two-window rows where that kernel's
# eligibility function (net_plan.hip) accepts them; every row named below is a boosted dual row (asserted), its shares of wrapped
# outputs are pinned in test_resnet50_wrap2_rows_wrap_in_both_windows.
#   all      every row: the boosted rows alternate with rows that read a boosted tensor (two windows as well, benign magnitudes), so the
#            group, band and conv_bfirst launches find no one-window 3x3 / expand row and are not selected; row 3 goes to split-K
#   groups   {1, 2, 4 | 15, 16, 18, 19 | 47, 50}, the other rows plain one-window rows (q_spread = 0): shortcut, reduce and expand of
#            the first bottleneck (bgroup_first_at: "return n_dual == 0 || n_dual == 3", its 3x3 one-window), the reduces of two 28 x 28
#            bottlenecks (rows 16 / 19 read them: dual, not boosted) and of the 7 x 7 ones
#   body     {5, 8, 14 | 15, 16, 18, 19 | 48, 51}: row 14 boosts stage 3's residual tensor, so the reduces 15 / 18 drop their Q and the
#            3x3 rows 16 / 19 are the boosted ones (a band's or group's dual 3x3 needs a dual reduce: conv_bband_windows_ok "return dual1
#            || !dual2"); the pointwise rows 5, 8, 14 and stage 5's 3x3 rows 48 / 51 for the batch-8 in-flight plan
_WRAP2 = {
    "default": (dict(), 2, 0, {"conv_mfma2_kernel": {5, 8}, "conv_mfma2_pair": {11, 12}, "conv_mfma_sk_kernel": {3, 16, 19}}, "all"),
    "bneck": (dict(bneck_min="1"), 2, 0, {"conv_bneck": {16, 19}}, "all"),
    "pwk": _WRAP["pwk"] + ("all",),
    "pw": _WRAP["pw"] + ("all",),
    "sk": (dict(sk="1"), 2, 0, {"conv_mfma_sk_kernel": {3, 8, 14}}, "all"),
    "img": _WRAP["img"] + ("all",),
    "bgroup": (_BGROUP, 2, 0, {"conv_bgroup56f": {1, 2}, "conv_bgroup28": {15, 18}, "conv_bgroup7": {47, 50}}, "groups"),
    "bfirst": (dict(bfirst="2", bfirst_min="1", alt_conc="0"), 2, 0, {"conv_bfirst": {1, 2}}, "groups"),
    "bband": (_BBAND28, 2, 0, {"conv_bband": {15, 18}}, "groups"),
    "bgroup_3x3": (_BGROUP, 2, 0, {"conv_bgroup28": {16, 19}}, "body"),
    "bband_3x3": (_BBAND28, 2, 0, {"conv_bband": {16, 19}}, "body"),
}
# Kernels that cannot take a wrap2 row:
#   conv_stem              weight_pack.cpp writes its image only when "Np == 64 && TM == 64 && P <= 2 && C <= 32 && !L.endpool": row 0 in
#                          wrap2 has three windows (its two level clusters and the rewrite's unit taps at shift 0).  The stem's
#                          two-window form is (high window, unit taps), which the wrap model's row 0 is, 19 exponents apart.
#   conv_bgroup_kernel     (14 x 14, with or without bgroup_chain) bgroup_at: "if (!(one_window || (k == l && A.H == 7 && dual))) return false;"
#   conv_bband, 14 x 14    conv_bband_windows_ok: "if (M == 256) return !dual1 && !dual2;"
#   the expand of a group, band or conv_bfirst launch: one-window only (bband_at: "if (!one_window && !(dual && k < l + 2)) return false;")
#                          -- but conv_bgroup56f's, which is dual with its shortcut and reduce
WRAP2_NOT_SELECTED = ("conv_stem", "conv_bgroup_kernel")
R50_ROUTES = {
    "wrap": _WRAP,
    "saturate": dict({k: v for k, v in _WRAP.items() if k not in SATURATE_NOT_SELECTED},
                     bgroup=(_BGROUP, 2, 0, {"conv_bgroup28": {16, 19}, "conv_bgroup7": {48}})),
    # the spread model (3-5 windows on rows 14 and 30): only the ring and split-K kernels take rows of more than two windows; conv_img
    # gets the two-window rows 48 / 51 behind the targeted rows 47 / 50
    "spread": {"default": (dict(), 2, 0, {"conv_mfma2_kernel": {14, 30}}), "sk": (dict(sk="1"), 2, 0, {"conv_mfma_sk_kernel": {14, 30}}),
               "img": _WRAP["img"] + ("img",)},
    "wrap2": _WRAP2,
}
R50_SPREAD_ROWS = {14, 30}
SEMI_EXEMPT = ("conv_bfirst", "conv_bgroup56f")          # (rows 1-4: the extreme row among them, row 3, is a generic one)
# (regime, model name) -> (rows, q_spread) of synth_extreme; a route without a model name takes (regime, None)
R50_MODELS = {("spread", None): (R50_SPREAD_ROWS, 1), ("spread", "img"): (R50_SPREAD_ROWS | {47, 50}, 1),
              ("wrap2", "groups"): ({1, 2, 4, 15, 16, 18, 19, 47, 50}, 0), ("wrap2", "body"): ({5, 8, 14, 15, 16, 18, 19, 48, 51}, 0)}


def route(regime, name):
    """(options, batch, concurrency, {kernel: rows}, model name or None) of one route."""
    r = R50_ROUTES[regime][name]
    return r if len(r) == 5 else r + (None,)


def covered_rows(launches, prefix):
    """Rows computed by launches whose kernel name starts with `prefix`: a launch covers its own row and the rows up to the next
    launch's (a fused pair's expand, a group's inner rows, a pair launch's second row)."""
    starts = sorted({r["layer"] for r in launches if r["layer"] >= 0})
    out = set()
    for r in launches:
        if r["layer"] < 0 or not r["kernel"].startswith(prefix):
            continue
        nxt = [s for s in starts if s > r["layer"]]
        out.update(range(r["layer"], nxt[0] if nxt else r["layer"] + 1))
    return out


def r50_rows(regime, model=None):
    """(rows, q_spread) of the ResNet-50 extreme model `model` of a regime (default: every row)."""
    if model == "all":
        model = None
    return R50_MODELS.get((regime, model), (r50_all_rows(), 1))


def r50_extreme(regime, model=None):
    t = cfg.resnet50_tables()
    rows, q_spread = r50_rows(regime, model)
    return (t,) + synth.synth_extreme(t, 0, regime, rows=rows, q_spread=q_spread)


# wrap2 on ResNet-50, per model the rows the routes name: row -> (pin, measured) of the share of outputs whose final int64 accumulator
# leaves int32, and of the share whose int64 hi << dshift alone does (0 where the row's K is too short for that).  A pin is at most half
# of what the int64 reference measured.  Images: one synth_extreme_images image (seed 0); the body model takes the first plain float
# image of the in-flight GPU case instead (synth_images, seed 900: _in_flight's inputs), which leaves the rows as wrapped.
_WRAP2_PINS = {
    "all": {3: ((0.25, 0.549), (0, 0.0)), 5: ((0.2, 0.434), (0, 0.0)), 8: ((0.45, 0.972), (0, 0.0)), 11: ((0.45, 0.928), (0, 0.0)),
            12: ((0.45, 0.955), (0, 0.0)), 14: ((0.25, 0.576), (0, 0.0)), 16: ((0.25, 0.576), (0.02, 0.040)),
            19: ((0.35, 0.742), (0.15, 0.369)), 48: ((0.45, 0.905), (0.15, 0.378)), 51: ((0.45, 0.929), (0.15, 0.382))},
    "groups": {1: ((0.2, 0.441), (0, 0.0)), 2: ((0.2, 0.436), (0, 0.0)), 15: ((0.15, 0.367), (0, 0.0)), 18: ((0.3, 0.688), (0, 0.0)),
               47: ((0.45, 0.949), (0.15, 0.375)), 50: ((0.45, 0.932), (0.15, 0.375))},
    "body": {5: ((0.2, 0.458), (0, 0.0)), 8: ((0.2, 0.445), (0, 0.0)), 14: ((0.15, 0.331), (0, 0.0)), 16: ((0.3, 0.693), (0.03, 0.060)),
             19: ((0.35, 0.724), (0.15, 0.333)), 48: ((0.4, 0.867), (0.1, 0.375)), 51: ((0.4, 0.886), (0.1, 0.239))},
}


@pytest.mark.parametrize("mname", sorted(_WRAP2_PINS))
def test_resnet50_wrap2_rows_wrap_in_both_windows(mname):
    """The wrap2 rows that the routes put on each kernel (R50_ROUTES["wrap2"], the in-flight case's rows): two-window dual rows, even
    ones SEMI and odd ones generic, windows 13 exponents apart, and wrapped -- the final accumulator on a large share of the outputs,
    and on the long-K rows (stages 3 and 5's 3x3 rows, stage 5's reduces) hi << dshift on its own: a combination done in a wider type,
    or a dshift read for another row, changes those outputs."""
    t = cfg.resnet50_tables()
    _, q, model = r50_extreme("wrap2", mname)
    x = synth.synth_images(t, 1, 900) if mname == "body" else synth.synth_extreme_images(t, 1, 0)
    pins = _WRAP2_PINS[mname]
    named = set().union(*(rows for r in R50_ROUTES["wrap2"] for rows in route("wrap2", r)[3].values() if route("wrap2", r)[4] == mname))
    assert named <= set(pins), named - set(pins)
    st, _, _ = regime_stats(t, q, model, x, sorted(pins))
    for l, ((pin_w, meas_w), (pin_h, meas_h)) in pins.items():
        s = st[l]
        assert pin_w <= meas_w / 2 + 1e-9 and pin_h <= meas_h / 2 + 1e-9
        assert s["windows"] == 2 and s["dual"] == 1 and s["fast"] == (2 if l % 2 == 0 else 0), (l, s)
        assert (s["dshift"] >= 9).all(), (l, s["dshift"])
        assert s["wrapped"] >= pin_w and s["hi_shift_wraps"] >= pin_h, (l, s["wrapped"], s["hi_shift_wraps"])


# the kernel families that have a two-window form: each must get a boosted dual row from some wrap2 route
WRAP2_FAMILIES = ("conv_mfma2_kernel", "conv_mfma2_pair", "conv_mfma_sk_kernel", "conv_pw_kernel", "conv_pwk_kernel", "conv_pwk_pair",
                  "conv_bneck", "conv_bband", "conv_bgroup56f", "conv_bgroup28", "conv_bgroup7", "conv_bfirst", "conv_img_kernel")


@pytest.mark.parametrize("regime", ["wrap", "saturate", "spread", "wrap2"])
def test_resnet50_extreme_routes_reach_their_kernels(regime, monkeypatch):
    """The launch plans of the GPU cases (no device): every route runs the named rows of the extreme model on the named kernel, and in
    the wrap model each of the ring, split-K, pointwise and fused kernels gets at least one SEMI row and the stem a wrapped SEMI row.
    In the wrap2 models every named row is a boosted two-window (dual) row, every family of WRAP2_FAMILIES gets one, and a SEMI and a
    generic one are among them."""
    from tests.conftest import set_opts
    nets, seen = {}, {}
    for name in R50_ROUTES[regime]:
        opts, B, conc, want, mname = route(regime, name)
        if mname not in nets:
            t, q, model = r50_extreme(regime, mname)
            net = network.NetWork(t)
            net.Quantization(synth.q_text(q)); net.LoadModel(model); net.Pack(0)
            nets[mname] = (net, emu.parse(net.packed_host())[1])
        net, pls = nets[mname]
        targets = r50_rows(regime, mname)[0]
        monkeypatch.delenv("TF2_AMD_OPTS", raising=False)
        set_opts(monkeypatch, **opts)
        net.reload_options()
        launches = net.describe_launches(B, conc)
        for prefix, rows in want.items():
            got = covered_rows(launches, prefix)
            assert rows <= got, (regime, name, prefix, rows, got)
            if regime == "wrap":
                assert prefix in SEMI_EXEMPT or any(int(pls[l]["fast"]) == 2 and int(pls[l]["max_shift"]) >= 20 for l in rows), (name, prefix)
            if regime == "spread":
                assert all(3 <= int(pls[l]["n_phases"]) <= 5 for l in rows & targets)
                assert all(int(pls[l]["n_phases"]) == 2 and int(pls[l]["dual"]) == 1 for l in rows - targets)      # (the row behind a targeted one)
            if regime == "wrap2":
                for l in rows:
                    assert int(pls[l]["n_phases"]) == 2 and int(pls[l]["dual"]) == 1 and int(pls[l]["max_shift"]) >= 20, (name, prefix, l, pls[l])
                seen.setdefault(prefix, set()).update(int(pls[l]["fast"]) for l in rows)
        if regime == "wrap2":
            for prefix in WRAP2_NOT_SELECTED:
                assert not covered_rows(launches, prefix) & targets, (name, prefix)
    if regime == "wrap2":
        assert set(WRAP2_FAMILIES) <= set(seen), set(WRAP2_FAMILIES) - set(seen)
        forms = set().union(*seen.values())
        assert {0, 2} <= forms, seen                     # generic and SEMI dual rows


# ---- wrap2 on the other families of the GPU cases: small VGG16 (conv_c3, conv_fc), fire programs (conv_fire), body programs -------------
# {kernel prefix: rows} per option set, as the GPU cases assert them; per model the rows pinned: row -> ((pin, measured) wrapped,
# (pin, measured) hi << dshift), pins at most half of the int64 reference's figures (two synth_extreme_images images of the model's seed)
VGG16_WRAP2 = [(dict(c3="1", c3_min="1", c3_min256="1", fc="1", fc4="1", fc_min="8"), {"conv_c3_kernel": {1, 2, 3, 4, 5, 6}, "fc_partial": {13, 14}}),
               (dict(c3="0", fc="1", fc4="0", fc_min="8"), {"fc_partial": {13, 14}, "conv_mfma_sk": {1, 3, 5}}),
               (dict(c3="1", c3_min="1", c3_w9="2", fc="0", no4bit="1"), {"conv_c3_kernel": {1, 3, 4, 5, 6}})]
FIRE_WRAP2_ROWS = {1, 4}             # the squeezes of the first two fire modules (row 4 reads a concat tensor: its shares are not measured here)
# the same launches as the wrap model's, but the whole-window rows on conv_fc's int8 form (two-window rows do not fit the 4-bit codes);
# seed 2's third pair (rows 11 | 12) has the generic boosted 3x3 whose hi << dshift leaves int32
BODY_WANT_WRAP2 = {2: {"conv_bneck": {5, 6, 8, 9, 11, 12}, "conv_c3_kernel": {1, 2}},
                   5: {"conv_c3_kernel": {1, 2}, "fc_partial": {5}},
                   9: {"conv_bneck": {4, 5}, "conv_c3_kernel": {1}, "fc_partial": {6}}}


def _family_cases():
    from tests import test_fuzz_programs as F
    yield ("vgg16", lambda: cfg.vgg16_tables(64, 40), 4, {}, [o for o, _ in VGG16_WRAP2], [w for _, w in VGG16_WRAP2],
           {3: ((0.3, 0.696), (0.12, 0.294)), 5: ((0.4, 0.847), (0.15, 0.375)), 13: ((0.4, 0.892), (0.15, 0.375))})      # (row 1: 0.573 | 0)
    yield ("fire4", lambda: F.random_fire_program(4), 4, dict(rows=FIRE_WRAP2_ROWS, q_spread=0), [dict(fire="1")], [{"conv_fire": FIRE_WRAP2_ROWS}],
           {1: ((0.1, 0.262), (0, 0.0))})
    yield ("fire1", lambda: F.random_fire_program(1), 1, dict(rows=FIRE_WRAP2_ROWS, q_spread=0), [dict(fire="1")], [{"conv_fire": FIRE_WRAP2_ROWS}], {})
    yield ("body2", lambda: F.random_body_program(2), 2, {}, [F._BODY_OPTS], [BODY_WANT_WRAP2[2]],
           {1: ((0.3, 0.622), (0, 0.0)), 6: ((0.25, 0.557), (0, 0.0)), 8: ((0.3, 0.634), (0, 0.003)), 11: ((0.4, 0.811), (0.15, 0.337))})
    yield ("body5", lambda: F.random_body_program(5), 5, {}, [F._BODY_OPTS], [BODY_WANT_WRAP2[5]],
           {1: ((0.25, 0.537), (0, 0.0)), 5: ((0.35, 0.738), (0.15, 0.375))})
    yield ("body9", lambda: F.random_body_program(9), 9, {}, [F._BODY_OPTS], [BODY_WANT_WRAP2[9]],
           {1: ((0.2, 0.49), (0, 0.0)), 6: ((0.45, 0.973), (0.25, 0.543))})


@pytest.mark.parametrize("case", list(_family_cases()), ids=lambda c: c[0])
def test_wrap2_family_models_reach_their_kernels_and_wrap(case, monkeypatch):
    """The launch plans of the GPU cases' wrap2 models outside ResNet-50 (no device): the named kernels run the named rows, those are
    two-window dual rows, a boosted one among them per kernel except where noted, and the pinned rows wrap."""
    from tests.conftest import set_opts
    _, mk, seed, kw, opt_sets, wants, pins = case
    t = mk()
    q, model = synth.synth_extreme(t, seed, "wrap2", **kw)
    for opts, want in zip(opt_sets, wants):
        monkeypatch.delenv("TF2_AMD_OPTS", raising=False)
        set_opts(monkeypatch, **opts)
        net = network.NetWork(t)
        net.Quantization(synth.q_text(q)); net.LoadModel(model); net.Pack(0)
        _, pls = emu.parse(net.packed_host())
        launches = net.describe_launches(2, 0)
        for prefix, rows in want.items():
            assert rows <= covered_rows(launches, prefix), (prefix, rows, [(r["layer"], r["kernel"]) for r in launches])
            assert all(int(pls[l]["n_phases"]) == 2 and int(pls[l]["dual"]) == 1 for l in rows), (prefix, rows)
            # (body program 9's pair, rows 4 | 5, reads a boosted tensor: two-window rows of benign magnitudes)
            assert any(int(pls[l]["max_shift"]) >= 20 for l in rows) or (seed == 9 and prefix == "conv_bneck"), (prefix, rows)
    if pins:
        st, _, _ = regime_stats(t, q, model, synth.synth_extreme_images(t, 2, seed), sorted(pins))
        for l, ((pin_w, meas_w), (pin_h, meas_h)) in pins.items():
            assert pin_w <= meas_w / 2 + 1e-9 and pin_h <= meas_h / 2 + 1e-9
            assert st[l]["dual"] == 1 and (st[l]["dshift"] >= 9).all(), (l, st[l])
            assert st[l]["wrapped"] >= pin_w and st[l]["hi_shift_wraps"] >= pin_h, (l, st[l]["wrapped"], st[l]["hi_shift_wraps"])


# ---- the packed image at the extremes (CPU emulation of the kernels' data flow, tests/emu_packed.py) ----------------------------------
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("regime", synth.EXTREME_REGIMES)
def test_tiny_packed_image_at_the_extremes(regime, mode):
    t, q, model, x = _tiny(regime)
    check_net(t, q, model, x, mode)


def _no_concat_rows(t):
    plan = cfg.build_plan(t)
    return {L.index for L in plan if not (L.src >= 0 and plan[L.src].concat >= 0)}


@pytest.mark.parametrize("family,seed", [("free", 3), ("free", 11), ("body", 2), ("body", 5), ("fire", 1), ("inception", 4)])
@pytest.mark.parametrize("regime", ["wrap", "saturate", "spread", "wrap2"])
def test_random_programs_packed_image_at_the_extremes(family, seed, regime, monkeypatch):
    from tests import test_fuzz_programs as F
    from tests.conftest import set_opts
    if family == "body":
        set_opts(monkeypatch, **F._BODY_OPTS)
    gen = dict(free=F.random_program, body=F.random_body_program, fire=F.random_fire_program, inception=F.random_inception_program)[family]
    t = gen(seed)
    q, model = synth.synth_extreme(t, seed, regime)
    x = synth.synth_extreme_images(t, 2, seed)
    for mode in (0, 2):
        check_net(t, q, model, x, mode, layers=_no_concat_rows(t))
