"""Max pools and global averages at their extremes (no device): the post-op regimes of tf2_amd/synth.py (synth_postop "signed_pool",
"avg_extreme") on the post-op programs of tf2_amd/config.py, and the launch plans that decide which kernel pools or averages a row.

The plain reference here is numpy, restated from the reference's device code and not from oracle/tf2_oracle.c:
- max pool: out[ph, pw] = max over the S x S window at (ph * st - pad, pw * st - pad) of the map extended by zeros -- taps beyond the
  valid map read 0 (pool.cl:115-140) -- and, for S < 3, of the window slots s >= S that stay 0 (pool.cl:177-186);
- global average: an int16 sum of the H x W map (full_size_pool.cl:95-106, Sreal: wraps), then ((s * mult) >> 14) + 1 >> 1 with an
  arithmetic shift (:118), then the clip to int8 (:119).
oracle.tf2o_maxpool / tf2o_global_avg and the post-ops inside tf2o_layer are checked against it on the regime data, and the regimes are
shown to reach their targets from the oracle's own maps.  The GPU cases are tests/test_gpu_postop_extremes.py."""
import numpy as np
import pytest

from oracle import netref, oracle as O
from tf2_amd import config as cfg, network, synth
from tests.conftest import set_opts


# ---- the numpy restatements ------------------------------------------------------------------------------------------------------------
def np_maxpool(x, S, st, pad, PH, PW):
    """x int8 [C, H, W] -> int8 [C, PH, PW]."""
    C, H, W = x.shape
    hz, wz = max(H + 2 * pad, (PH - 1) * st + S), max(W + 2 * pad, (PW - 1) * st + S)
    xz = np.zeros((C, hz, wz), np.int16)
    xz[:, pad:pad + H, pad:pad + W] = x
    out = np.full((C, PH, PW), 0 if S < 3 else -128, np.int16)
    for i in range(S):
        for j in range(S):
            out = np.maximum(out, xz[:, i:i + st * (PH - 1) + 1:st, j:j + st * (PW - 1) + 1:st])
    return out.astype(np.int8)


def np_global_avg(x, mult):
    """x int8 [C, H, W] -> int8 [C]."""
    s = x.reshape(x.shape[0], -1).astype(np.int64).sum(axis=1)
    s = (s + 32768) % 65536 - 32768
    m = (((s * mult) >> 14) + 1) >> 1
    return np.clip(m, -128, 127).astype(np.int8)


def pool_windows(x, S, st, pad, PH, PW):
    """Per window of x int8 [C, H, W]: (max of the taps inside the map, whether a tap lies outside it), each [C, PH, PW]."""
    C, H, W = x.shape
    inside = np.full((C, PH, PW), -129, np.int16)
    outside = np.zeros((PH, PW), bool)
    for ph in range(PH):
        for pw in range(PW):
            h0, w0 = ph * st - pad, pw * st - pad
            h1, w1 = max(h0, 0), max(w0, 0)
            h2, w2 = min(h0 + S, H), min(w0 + S, W)
            outside[ph, pw] = (h1, w1, h2, w2) != (h0, w0, h0 + S, w0 + S)
            inside[:, ph, pw] = x[:, h1:h2, w1:w2].reshape(C, -1).max(axis=1)
    return inside, np.broadcast_to(outside, inside.shape)


def pre_post_op(R, outs, L):
    """Row L's map in front of its pool / global average (the oracle's layer with those post-ops off), int8 [B, N, OH, OW]."""
    spec = L.oracle_spec()
    spec.update(pool_en=0, PH=L.OH, PW=L.OW, endpool=0)
    res = outs[L.add_src] if L.add_src >= 0 else None
    b, a, be = R.bn[L.index]
    return O.layer(spec, outs[L.src], R.codes[L.index], b, a, be, res)


def _run(t, q, model, B, seed):
    R = netref.RefNet(t, q, model)
    x = synth.synth_extreme_images(t, B, seed)
    return R, R.run(x)


# ---- the programs of the regimes -------------------------------------------------------------------------------------------------------
def signed_pool_cases():
    """(name, tables, pooled rows, pooling rows): the four pool geometries behind a row without ReLU, each with a 3/1/1 pooling row on a
    signed tensor; conv_c3's ceil-mode 2x2 pool on the odd 31 x 31 map without ReLU."""
    out = [(f"geom_{g}", cfg.signed_pool_tables(g), [1], [3]) for g in cfg.POOL_GEOMS]
    out.append(("c3_odd_relu0", cfg.c3_pool_tables(31, relu=0), [1], []))
    return out


# averaged rows: {name: (tables, averaged row, categories that must occur)}.  Which categories a map admits is a matter of its size and
# multiplier (synth.avg_level_targets): with mult = round(2^15 / HW) no average clips, on 8 x 8 no int16 sum wraps, 669 is odd.
AVG_CASES = {
    "avg22": (lambda: cfg.avg_tables(22), 3, ("wrap+", "wrap-", "half+", "half-", "neg")),
    "avg22_m669": (lambda: cfg.avg_tables(22, mult=669), 3, ("wrap+", "wrap-", "clip+", "clip-", "neg")),
    "avg8": (lambda: cfg.avg_tables(8), 3, ("half+", "half-", "neg")),
    "avg8_m669": (lambda: cfg.avg_tables(8, mult=669), 3, ("clip+", "clip-", "neg")),
}


def avg_categories(pre, mult):
    """Counts per category of the (image, channel) averages of pre int8 [B, N, H, W], from the exact sums."""
    B, N = pre.shape[:2]
    st = pre.reshape(B, N, -1).astype(np.int64).sum(axis=2)
    s = (st + 32768) % 65536 - 32768
    m = (((s * mult) >> 14) + 1) >> 1
    half = (s * mult) % 32768 == 16384
    return {"wrap+": int(((st != s) & (st > 0)).sum()), "wrap-": int(((st != s) & (st < 0)).sum()),
            "half+": int((half & (s > 0)).sum()), "half-": int((half & (s < 0)).sum()),
            "clip+": int((m > 127).sum()), "clip-": int((m < -128).sum()),
            "neg": int(((m < 0) & (m >= -128) & ((s * mult) % 16384 != 0)).sum())}


# ---- the restatements against the oracle, on the regime data ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(5))
def test_maxpool_restatement_matches_the_oracle(case):
    name, t, pooled, pooling = signed_pool_cases()[case]
    q, model = synth.synth_postop(t, 3, "signed_pool")
    R, outs = _run(t, q, model, 2, 3)
    plan = cfg.build_plan(t)
    for l in pooled:
        L = plan[l]
        pre = pre_post_op(R, outs, L)
        for b in range(pre.shape[0]):
            want = np_maxpool(pre[b], L.pool_S, L.pool_st, L.pool_pad, L.PH, L.PW)
            np.testing.assert_array_equal(outs[l][b], want, err_msg=f"{name}: tf2o_layer's pool, row {l}")
            np.testing.assert_array_equal(O.maxpool(pre[b], L.pool_S, L.pool_st, L.pool_pad, L.PH, L.PW), want, err_msg=f"{name}: tf2o_maxpool")
    for l in pooling:
        L = plan[l]
        for b in range(outs[l].shape[0]):
            np.testing.assert_array_equal(outs[l][b], np_maxpool(outs[L.src][b], L.pool_S, L.pool_st, L.pool_pad, L.PH, L.PW),
                                          err_msg=f"{name}: pooling row {l}")


@pytest.mark.parametrize("name", sorted(AVG_CASES))
def test_global_avg_restatement_matches_the_oracle(name):
    mk, l, _ = AVG_CASES[name]
    t = mk()
    q, model = synth.synth_postop(t, 4, "avg_extreme")
    R, outs = _run(t, q, model, 2, 4)
    L = cfg.build_plan(t)[l]
    pre = pre_post_op(R, outs, L)
    for b in range(pre.shape[0]):
        want = np_global_avg(pre[b], L.endpool_mult)
        np.testing.assert_array_equal(outs[l][b].ravel(), want, err_msg=f"{name}: tf2o_layer's average")
        np.testing.assert_array_equal(O.global_avg(pre[b].reshape(L.N, -1), L.endpool_mult).ravel(), want, err_msg=f"{name}: tf2o_global_avg")


def test_restatements_at_hand_made_edges():
    """A few maps written out by hand: the zero slot of S = 2, the zero tap at pad 1 and at the ceil-mode edge, -128; an int16 wrap, both
    rounding halves, both clips."""
    x = np.full((1, 4, 4), -5, np.int8); x[0, 1, 1] = -128; x[0, 2, 2] = -1
    np.testing.assert_array_equal(np_maxpool(x, 2, 2, 0, 2, 2), np.zeros((1, 2, 2), np.int8))            # slot 0 wins for S = 2
    np.testing.assert_array_equal(np_maxpool(x, 3, 2, 1, 2, 2), [[[0, 0], [0, -1]]])                     # the pad decides but at (1, 1)
    np.testing.assert_array_equal(np_maxpool(x, 3, 1, 0, 2, 2), [[[-1, -1], [-1, -1]]])                  # inside only: no zero tap
    np.testing.assert_array_equal(np_maxpool(x, 3, 2, 0, 2, 2), [[[-1, 0], [0, 0]]])                     # ceil edge: zero taps
    for s, mult, want in ((127 * 289, 113, _avg(127 * 289 - 65536, 113)), (32, 512, 1), (-32, 512, 0), (96, 512, 2), (-96, 512, -1),
                          (127 * 64, 669, 127), (-128 * 64, 669, -128)):
        m = np.zeros(64 if mult != 113 else 289, np.int64)
        m[:] = s // m.size; m[: s - m.sum()] += 1 if s > m.sum() else 0; m[: m.sum() - s] -= 1 if m.sum() > s else 0
        assert m.sum() == s and np.abs(m).max() <= 128
        np.testing.assert_array_equal(np_global_avg(m.astype(np.int8).reshape(1, 1, -1), mult), [want])
        np.testing.assert_array_equal(O.global_avg(m.astype(np.int8).reshape(1, -1), mult).ravel(), [want])


def _avg(s, mult):
    return int(np.clip((((s * mult) >> 14) + 1) >> 1, -128, 127))


# ---- the regimes reach their targets ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(5))
def test_signed_pool_regime_reaches_its_windows(case):
    """Per targeted pooled row (and pooling row): windows whose inside is all negative and whose result the zero tap (pad 1, the
    ceil-mode edge) or the zero slot of S < 3 decides; for S = 3 windows wholly inside the map with a negative maximum; -128 and 127 in
    the map; channels negative everywhere."""
    name, t, pooled, pooling = signed_pool_cases()[case]
    q, model = synth.synth_postop(t, 3, "signed_pool")
    R, outs = _run(t, q, model, 2, 3)
    plan = cfg.build_plan(t)
    for l in pooled + pooling:
        L = plan[l]
        pre = pre_post_op(R, outs, L) if not L.ipool else outs[L.src]
        n_zero_tap = n_slot = n_neg_inside = n_neg_chan = 0
        for b in range(pre.shape[0]):
            inside, outside = pool_windows(pre[b], L.pool_S, L.pool_st, L.pool_pad, L.PH, L.PW)
            n_zero_tap += int(((inside < 0) & outside).sum())
            n_slot += int(((inside < 0) & ~outside).sum()) if L.pool_S < 3 else 0
            n_neg_inside += int(((inside < 0) & ~outside).sum()) if L.pool_S >= 3 else 0
            n_neg_chan += int((pre[b].reshape(L.N, -1).max(axis=1) < 0).sum())
        assert n_zero_tap + n_slot > 0, (name, l)
        if L.pool_pad or (L.PH - 1) * L.pool_st + L.pool_S > L.OH:
            assert n_zero_tap > 0, (name, l)
        if L.pool_S < 3:
            assert n_slot > 0, (name, l)
        else:
            assert n_neg_inside > 0, (name, l)
        assert n_neg_chan > 0 and (pre == -128).any() and (pre == 127).any(), (name, l)


@pytest.mark.parametrize("name", sorted(AVG_CASES))
def test_avg_extreme_regime_reaches_its_edges(name):
    mk, l, want = AVG_CASES[name]
    t = mk()
    q, model = synth.synth_postop(t, 4, "avg_extreme")
    R, outs = _run(t, q, model, 2, 4)
    L = cfg.build_plan(t)[l]
    got = avg_categories(pre_post_op(R, outs, L), L.endpool_mult)
    assert all(got[k] > 0 for k in want), (name, got)
    lv = synth.avg_level_targets(L.H, L.W, L.endpool_mult)
    assert all(bool(lv[k]) == (k in want) for k in lv), (name, {k: len(v) for k, v in lv.items()})      # (nothing the map admits is left out)


def test_avg_extreme_on_resnet50_row52_signed():
    """kAdditionReluEnable[52] = 0: the 7 x 7 average (conv_mfma_sk AVG) of a signed map -- negative averages (the only edge a 7 x 7 map
    with 669 admits: no wrap, no half, no clip) on every image."""
    t = r50_signed_avg_tables()
    q, model = synth.synth_postop(t, 0, "avg_extreme", rows=[52])
    R, outs = _run(t, q, model, 1, 0)
    L = cfg.build_plan(t)[52]
    got = avg_categories(pre_post_op(R, outs, L), L.endpool_mult)
    assert got["neg"] >= 64 and not any(got[k] for k in ("wrap+", "wrap-", "half+", "half-", "clip+", "clip-")), got
    assert (outs[52] == 127).any() and (outs[52] < 0).any()


def r50_relu0_tables():
    """ResNet-50 with kReluEnable[0] = 0: conv_stem_pool_kernel's non-ReLU branch pools a signed map."""
    return cfg.with_flags(cfg.resnet50_tables(), "kReluEnable", [0], 0)


def r50_signed_avg_tables():
    """ResNet-50 with kAdditionReluEnable[52] = 0: the global average inside row 52's split-K launch reads a signed map."""
    return cfg.with_flags(cfg.resnet50_tables(), "kAdditionReluEnable", [52], 0)


# ---- launch plans --------------------------------------------------------------------------------------------------------------------
def _cover(raw, r):
    """Rows a launch computes: a separate pool / average launch its own row; another launch its row and those up to the next launch's
    (a fused launch's inner rows: tests/test_extreme_regimes.py covered_rows)."""
    if r["layer"] < 0:
        return set()
    if r["kernel"] in ("maxpool_kernel", "global_avg_kernel"):
        return {r["layer"]}
    nxt = [x["layer"] for x in raw if x["layer"] > r["layer"]]
    return set(range(r["layer"], min(nxt) if nxt else r["layer"] + 1))


def _pooling(raw, row):
    return [r["kernel"] for r in raw if "pool" in r["kernel"] and row in _cover(raw, r)]


def _averaging(raw, row):
    return [r["kernel"] for r in raw if ("global average" in r["kernel"] or r["kernel"] == "global_avg_kernel") and row in _cover(raw, r)]


def _plan(t, q, model, B, conc, mode=0):
    net = network.NetWork(t)
    net.Quantization(synth.q_text(q)); net.LoadModel(model); net.Pack(mode)
    return net, [(r["layer"], r["kernel"]) for r in net.describe_launches(B, conc)], net.describe_launches(B, conc)


def _qm(t, seed=1):
    q = synth.synth_q_values(t, seed, spread=1)
    return q, synth.synth_model(t, q, seed)


def _fire_tables(relu):
    from tests.test_fuzz_programs import random_fire_program
    t = random_fire_program(0)                      # (fire modules 2 and 3 pool behind the expands, rows 5 and 6)
    return t if relu else cfg.with_flags(t, "kReluEnable", [5, 6], 0)


def _sq_tables(relu):
    t = cfg.squeezenet11_tables(image_hw=67)
    return t if relu else cfg.with_flags(t, "kReluEnable", [0], 0)


# ReLU-only fused pools: (tables(relu), options, pooled row, fused kernel prefix).  With ReLU the fused pool takes the row; without it
# the row's pool must run on maxpool_kernel (the fused pools take an unsigned maximum: v_pk_max_u16).
RELU_ONLY_POOLS = {
    "c3": (lambda r: cfg.c3_pool_tables(31, r), dict(c3="1", c3_min="1", c3_min256="1"), 1, "conv_c3_kernel"),
    "c3_w9": (lambda r: cfg.c3_pool_tables(31, r), dict(c3="1", c3_min="1", c3_w9="2"), 1, "conv_c3_w9"),
    "fire": (_fire_tables, dict(fire="1", fire_pool="4"), 5, "conv_fire"),
    "first_pool": (_sq_tables, dict(), 0, "conv_first_pool"),
}


@pytest.mark.parametrize("name", sorted(RELU_ONLY_POOLS))
def test_relu_only_fused_pools_refuse_rows_without_relu(name, monkeypatch):
    mk, opts, row, prefix = RELU_ONLY_POOLS[name]
    set_opts(monkeypatch, **opts)
    for relu in (1, 0):
        t = mk(relu)
        _, launches, raw = _plan(t, *_qm(t), 2, 0)
        pooling = _pooling(raw, row)
        if relu:
            assert any(k.startswith(prefix) for k in pooling) and not any(k.startswith("maxpool") for k in pooling), (name, launches)
        else:
            assert pooling and all(k.startswith("maxpool_kernel") for k in pooling), (name, launches)
            assert (row, "maxpool_kernel") in launches, (name, launches)


def test_stem_pools_both_branches():
    """ResNet-50's row 0 runs on conv_stem_pool_kernel with and without ReLU (the kernel's signed branch), and rows 1-2 then read a
    signed tensor (conv_shift_kernel); stem_pool=0 moves the pool onto maxpool_kernel."""
    for relu in (1, 0):
        t = cfg.resnet50_tables() if relu else r50_relu0_tables()
        q, model = synth.synth_postop(t, 0, "signed_pool", rows=[0])
        net, launches, _ = _plan(t, q, model, 2, 0)
        assert launches[1][0] == 0 and launches[1][1].startswith("conv_stem_pool_kernel"), launches[:4]
        if not relu:
            assert {1, 2} <= {l for l, k in launches if k.startswith("conv_shift_kernel")}, launches[:6]


def test_stem_pool_off_runs_maxpool(monkeypatch):
    set_opts(monkeypatch, stem_pool="0")
    t = r50_relu0_tables()
    _, launches, _ = _plan(t, *synth.synth_postop(t, 0, "signed_pool", rows=[0]), 2, 0)
    assert (0, "maxpool_kernel") in launches and not any("pool" in k for l, k in launches if l == 0 and k != "maxpool_kernel"), launches[:4]


def test_resnet50_signed_average_stays_fused():
    t = r50_signed_avg_tables()
    _, launches, _ = _plan(t, *synth.synth_postop(t, 0, "avg_extreme", rows=[52]), 2, 0)
    assert any(l == 52 and k.startswith("conv_mfma_sk") and "global average" in k for l, k in launches), launches[-4:]


# a row that pools AND averages: the pool into its own PH x PW tensor, then the average of it (never the pool into the 1 x 1 output)
POOL_AVG_ROUTES = {
    "default": (lambda: cfg.pool_avg_tables(12, 1), dict(), 0, "conv_mfma2"),
    "signed": (lambda: cfg.pool_avg_tables(12, 0), dict(), 0, "conv_mfma2"),
    "sk": (lambda: cfg.pool_avg_tables(12, 0), dict(sk="1", avg_fuse="1"), 0, "conv_mfma_sk"),
    "shift": (lambda: cfg.pool_avg_tables(12, 0), dict(), 2, "conv_shift"),
    "first_row": (lambda: cfg.stem_pool_avg_tables(0), dict(), 0, "conv_mfma_sk"),
}


@pytest.mark.parametrize("route", sorted(POOL_AVG_ROUTES))
@pytest.mark.parametrize("conc", [0, 1])
def test_pool_and_average_row_plans_both(route, conc, monkeypatch):
    mk, opts, mode, conv = POOL_AVG_ROUTES[route]
    set_opts(monkeypatch, **opts)
    t = mk()
    row = [L.index for L in cfg.build_plan(t) if L.pool_en and L.endpool][0]
    net, launches, _ = _plan(t, *_qm(t), 2, conc, mode)
    mine = [k for l, k in launches if l == row]
    assert len(mine) == 3 and mine[0].startswith(conv) and mine[1] == "maxpool_kernel" and mine[2] == "global_avg_kernel", (route, launches)
    # the pooled map has a tensor of its own: one tensor more than the rows name, batch x PH x PW x Cp bytes
    tensors, rows = net.describe_workspace(2, False)
    named = {r[k] for r in rows for k in ("in_tensor", "out_tensor", "conv_tensor", "res_tensor") if r[k] >= 0}
    extra = [i for i in range(len(tensors)) if i not in named]
    L = cfg.build_plan(t)[row]
    assert len(extra) == 1 and tensors[extra[0]]["bytes"] >= 2 * L.PH * L.PW * 64, (extra, tensors)
    assert tensors[rows[row]["out_tensor"]]["bytes"] < 2 * L.PH * L.PW * 64


def test_pooling_row_with_an_average_is_refused():
    t = cfg.signed_pool_tables("3s2p1")
    t["kEndPoolEnable"][3] = 1
    with pytest.raises(Exception, match="pool-only row with a global average"):
        _plan(t, *_qm(t), 1, 0)


SHIPPED = ("resnet50", "resnet50_pruned", "googlenet", "squeezenet", "vgg16", "ssd300")


@pytest.mark.parametrize("name", SHIPPED)
def test_shipped_plans_keep_their_post_op_shape(name):
    """The shipped networks have no row that pools and averages: their launch plans and workspaces are those of before pool + average
    rows were planned.  Per batch 1 / 32 and one batch at a time / in flight: every tensor of the workspace is some row's input, output,
    conv map or residual (no extra pooled map); every pooling row is covered by exactly one pooling launch (maxpool_kernel or a fused
    pool), every averaged row by exactly one averaging launch (global_avg_kernel or a fused average); no other row has a maxpool_kernel
    or global_avg_kernel launch."""
    t, qv, seed, _, _ = synth.bench_network(name)
    plan = cfg.build_plan(t)
    assert not any(L.pool_en and L.endpool for L in plan)
    net = network.NetWork(t)
    net.Quantization(synth.q_text(qv)); net.LoadModel(synth.synth_model(t, qv, seed)); net.Pack(0)
    for B in (1, 32):
        tensors, rows = net.describe_workspace(B, False)
        named = {r[k] for r in rows for k in ("in_tensor", "out_tensor", "conv_tensor", "res_tensor") if r[k] >= 0}
        assert named == set(range(len(tensors))), (name, B, sorted(set(range(len(tensors))) - named))
        for conc in (0, 1):
            raw = net.describe_launches(B, conc)
            for L in plan:
                # (a merged row -- the 3x3 expand behind a 1x1 one, weight_pack.cpp merge_next -- is pooled with the row it is merged into)
                own = min(m for m in range(L.index + 1) if rows[m]["conv_tensor"] == rows[L.index]["conv_tensor"])
                npool, navg = len(_pooling(raw, own)), len(_averaging(raw, own))
                assert npool == (1 if L.pool_en or L.ipool == 1 else npool), (name, B, conc, L.index, _pooling(raw, L.index))
                assert navg == (1 if L.endpool else navg), (name, B, conc, L.index, _averaging(raw, L.index))
            for r in raw:
                if r["kernel"] == "maxpool_kernel":
                    assert plan[r["layer"]].pool_en or plan[r["layer"]].ipool == 1, (name, B, conc, r)
                if r["kernel"] == "global_avg_kernel":
                    assert plan[r["layer"]].endpool and not plan[r["layer"]].pool_en, (name, B, conc, r)


# ---- the routes of the GPU cases (tests/test_gpu_postop_extremes.py) ---------------------------------------------------------------------
# {name: (tables(), regime, targeted rows (None: the regime's default), pack mode, options, batch, concurrency, {kernel prefix: rows})}
_C3 = dict(c3="1", c3_min="1", c3_min256="1")
_C3W9 = dict(c3="1", c3_min="1", c3_w9="2")
_FIRE = dict(fire="1", fire_pool="4")
_BGROUP = dict(bgroup="1", bgroup_min7="1", bgroup_min14="1", bgroup_min28="1", bgroup_min56f="1", bfirst="1", alt_conc="0")
_POOL_AVG = {"maxpool_kernel": {2}, "global_avg_kernel": {2}}
POSTOP_ROUTES = {
    **{f"maxpool_{g}": (lambda g=g: cfg.signed_pool_tables(g), "signed_pool", None, 0, {}, 2, 0, {"maxpool_kernel": {1, 3}})
       for g in cfg.POOL_GEOMS},
    "c3_pool_odd": (lambda: cfg.c3_pool_tables(31, 1), "signed_pool", None, 0, _C3, 2, 0, {"conv_c3_kernel": {1}}),
    "c3_w9_pool_odd": (lambda: cfg.c3_pool_tables(31, 1), "signed_pool", None, 0, _C3W9, 2, 0, {"conv_c3_w9": {1}}),
    "c3_relu0": (lambda: cfg.c3_pool_tables(31, 0), "signed_pool", None, 0, _C3, 2, 0, {"conv_c3_kernel": {1}, "maxpool_kernel": {1}}),
    "stem_pool": (cfg.resnet50_tables, "signed_pool", [0], 0, {}, 2, 0, {"conv_stem_pool": {0}}),
    "r50_stem_relu0": (r50_relu0_tables, "signed_pool", [0], 0, {}, 2, 0, {"conv_stem_pool": {0}, "conv_shift_kernel": {1, 2}}),
    "r50_stem_relu0_pool_off": (r50_relu0_tables, "signed_pool", [0], 0, dict(stem_pool="0"), 2, 0,
                                {"conv_stem": {0}, "maxpool_kernel": {0}}),
    "first_pool": (lambda: _sq_tables(1), "signed_pool", [0], 0, {}, 2, 0, {"conv_first_pool": {0}}),
    "first_pool_relu0": (lambda: _sq_tables(0), "signed_pool", [0], 0, {}, 2, 0, {"maxpool_kernel": {0}}),
    "fire_pool": (lambda: _fire_tables(1), "signed_pool", [5, 6], 0, _FIRE, 2, 0, {"conv_fire": {5, 6}}),
    "fire_pool_relu0": (lambda: _fire_tables(0), "signed_pool", [5, 6], 0, _FIRE, 2, 0, {"maxpool_kernel": {5}}),
    "global_avg_22": (lambda: cfg.avg_tables(22), "avg_extreme", None, 0, {}, 2, 0, {"global_avg_kernel": {3}}),
    "global_avg_22_m669": (lambda: cfg.avg_tables(22, mult=669), "avg_extreme", None, 0, {}, 2, 0, {"global_avg_kernel": {3}}),
    "sk_avg_8": (lambda: cfg.avg_tables(8), "avg_extreme", None, 0, dict(avg_fuse="1"), 2, 0, {"conv_mfma_sk": {3}}),
    "sk_avg_8_m669": (lambda: cfg.avg_tables(8, mult=669), "avg_extreme", None, 0, dict(avg_fuse="1"), 2, 0, {"conv_mfma_sk": {3}}),
    "r50_sk_avg_signed": (r50_signed_avg_tables, "avg_extreme", [52], 0, {}, 2, 0, {"conv_mfma_sk": {52}}),
    "r50_bgroup7_avg": (cfg.resnet50_tables, "avg_extreme", [52], 0, _BGROUP, 2, 0, {"conv_bgroup7": {52}}),
    "pool_avg_default": (lambda: cfg.pool_avg_tables(12, 1), "signed_pool", None, 0, {}, 3, 0, dict(_POOL_AVG, conv_mfma2={2})),
    "pool_avg_signed": (lambda: cfg.pool_avg_tables(12, 0), "signed_pool", None, 0, {}, 3, 0, dict(_POOL_AVG, conv_mfma2={2})),
    "pool_avg_sk": (lambda: cfg.pool_avg_tables(12, 0), "signed_pool", None, 0, dict(sk="1", avg_fuse="1"), 3, 0,
                    dict(_POOL_AVG, conv_mfma_sk={2})),
    "pool_avg_shift": (lambda: cfg.pool_avg_tables(12, 0), "signed_pool", None, 2, {}, 3, 0, dict(_POOL_AVG, conv_shift={2})),
    "pool_avg_in_flight": (lambda: cfg.pool_avg_tables(12, 0), "signed_pool", None, 0, {}, 3, 1, _POOL_AVG),
    "pool_avg_first_row": (lambda: cfg.stem_pool_avg_tables(0), "signed_pool", None, 0, {}, 1, 0,
                           {"maxpool_kernel": {0}, "global_avg_kernel": {0}}),
}
_MODELS = {}


def postop_model(route):
    """(tables, q, model) of a route: synth_postop(seed 2) of its regime on its rows."""
    if route not in _MODELS:
        mk, regime, rows = POSTOP_ROUTES[route][:3]
        t = mk()
        _MODELS[route] = (t,) + synth.synth_postop(t, 2, regime, rows)
    return _MODELS[route]


def test_postop_routes_reach_their_kernels(monkeypatch):
    """The launch plans of the GPU cases, with their models: every route runs its rows on its kernels; the split-K and group routes
    average inside the launch; on the pool + average routes the row's own launches are conv, maxpool_kernel, global_avg_kernel."""
    for name, (mk, regime, rows, mode, opts, B, conc, want) in POSTOP_ROUTES.items():
        monkeypatch.delenv("TF2_AMD_OPTS", raising=False)
        set_opts(monkeypatch, **opts)
        t, q, model = postop_model(name)
        net = network.NetWork(t)
        net.Quantization(synth.q_text(q)); net.LoadModel(model); net.Pack(mode)
        raw = net.describe_launches(B, conc)
        for prefix, rs in want.items():
            got = {l for r in raw if r["kernel"].startswith(prefix) for l in _cover(raw, r)}
            assert rs <= got, (name, prefix, rs, sorted(got), [(r["layer"], r["kernel"]) for r in raw])
        if name.startswith(("sk_avg", "r50_sk_avg", "r50_bgroup7")):
            l = max(max(v) for v in want.values())
            assert any("global average" in k for k in _averaging(raw, l)), (name, raw)
        if name.startswith("pool_avg"):
            row = min(want["maxpool_kernel"])
            mine = [r["kernel"] for r in raw if r["layer"] == row]
            assert mine[-2:] == ["maxpool_kernel", "global_avg_kernel"], (name, mine)
