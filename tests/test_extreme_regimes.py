"""The extreme-regime models (tf2_amd/synth.py synth_extreme) reach the edges they are named after, and the packed image computes the
oracle's layers there.

The plain high-precision reference: every targeted layer's accumulator in int64 (numpy, from the oracle's own filter codes and the
oracle's input to that layer: x * (+-2^shift), the -128 negate quirk of pe.cl:32-37 kept), then the reference's requantisation steps
without any clamp.  From it, per layer: the share of accumulators outside int32 (wrapped), of outputs clipped at 127 / -128, of
generic-form x + 2^14 that saturates -- and from the packed image (tests/emu_packed.parse) the exponent windows, the epilogue form
(fast: 0 generic, 1 FAST, 2 SEMI) and the dual form.  The assertions pin each regime to its target, so that an edit to a generator
cannot quietly make it benign again."""
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


def layer_stats(R, outs, pls, L):
    """Exact int64 statistics of one conv row (plain form: no rewritten first layer)."""
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
    return dict(wrapped=float((acc64 != v).mean()), hi=float((y > 127).mean()), lo=float((y < -128).mean()),
                sat14=float((xq + 2 ** 14 > 2 ** 31 - 1).mean()), windows=int(pl["n_phases"]), fast=int(pl["fast"]),
                dual=int(pl["dual"]), max_shift=int(pl["max_shift"]), kind=int(pl["kind"]))


def regime_stats(t, q, model, x, rows, mode=0):
    net = network.NetWork(t)
    net.Quantization(synth.q_text(q)); net.LoadModel(model); net.Pack(mode)
    _, pls = emu.parse(net.packed_host())
    R = netref.RefNet(t, q, model)
    outs = R.run(x)
    return {l: layer_stats(R, outs, pls, R.plan[l]) for l in rows}, R, outs


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
}
SATURATE_NOT_SELECTED = ("bband", "bfirst", "bgroup_chain1")      # (and the 56 x 56 / 14 x 14 group kernels of the bgroup route)
R50_ROUTES = {
    "wrap": _WRAP,
    "saturate": dict({k: v for k, v in _WRAP.items() if k not in SATURATE_NOT_SELECTED},
                     bgroup=(_BGROUP, 2, 0, {"conv_bgroup28": {16, 19}, "conv_bgroup7": {48}})),
    # the spread model (3-5 windows on rows 14 and 30): only the ring and split-K kernels take rows of more than two windows
    "spread": {"default": (dict(), 2, 0, {"conv_mfma2_kernel": {14, 30}}), "sk": (dict(sk="1"), 2, 0, {"conv_mfma_sk_kernel": {14, 30}})},
}
R50_SPREAD_ROWS = {14, 30}
SEMI_EXEMPT = ("conv_bfirst", "conv_bgroup56f")          # (rows 1-4: the extreme row among them, row 3, is a generic one)


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


def r50_extreme(regime):
    t = cfg.resnet50_tables()
    rows = R50_SPREAD_ROWS if regime == "spread" else r50_all_rows()
    return (t,) + synth.synth_extreme(t, 0, regime, rows=rows)


@pytest.mark.parametrize("regime", ["wrap", "saturate", "spread"])
def test_resnet50_extreme_routes_reach_their_kernels(regime, monkeypatch):
    """The launch plans of the GPU cases (no device): every route runs the named rows of the extreme model on the named kernel, and in
    the wrap model each of the ring, split-K, pointwise and fused kernels gets at least one SEMI row and the stem a wrapped SEMI row."""
    from tests.conftest import set_opts
    t, q, model = r50_extreme(regime)
    net = network.NetWork(t)
    net.Quantization(synth.q_text(q)); net.LoadModel(model); net.Pack(0)
    _, pls = emu.parse(net.packed_host())
    for name, (opts, B, conc, want) in R50_ROUTES[regime].items():
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
                assert all(3 <= int(pls[l]["n_phases"]) <= 5 for l in rows)


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
@pytest.mark.parametrize("regime", ["wrap", "saturate", "spread"])
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
