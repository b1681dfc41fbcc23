"""DNS channel pruning on the device (tf2_dnscp_stats / tf2_dnscp_step / tf2_dnscp_compact, csrc/weight_dnscp.hip) against the numpy
statement tf2_amd.dnscp.reference_stats / reference_step / reference_compact: keep bytes, the output stream, S1 and every word of the
record as bits -- conv geometry, knife-edge sums, status bits, the fix-up, partial updates, graph replay, and a pruned network against
the masked one through the engine."""
import os

import numpy as np
import pytest

from tf2_amd import config as cfg, dnscp, network, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_dnscp.npz")
GAP_W, GAP_OUT = np.float32(123.456), np.float32(-77.25)       # between the convs, and what out_dev holds before a step


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch


class Buf:
    """convs [(offset, weights [N, C, kk])] laid into one flat buffer with marked gaps"""

    def __init__(self, parts, n_total=None):
        self.convs = [(int(o),) + tuple(np.shape(w)) for o, w in parts]
        last = self.convs[-1]
        self.n_total = int(n_total if n_total is not None else last[0] + last[1] * last[2] * last[3] + 3)
        self.w = np.full(self.n_total, GAP_W, np.float32)
        for o, w in parts:
            w = np.asarray(w, np.float32).ravel()
            self.w[o:o + w.size] = w

    def conv(self, i, w=None):
        o, N, C, kk = self.convs[i]
        return (self.w if w is None else w)[o:o + N * C * kk].reshape(N, C, kk)

    def stats(self, keeps=None):
        r = [dnscp.reference_stats(self.conv(i), None if keeps is None else keeps[i]) for i in range(len(self.convs))]
        return [s for s, _ in r], np.asarray([rec for _, rec in r], dnscp.STATE_DTYPE)

    def expect(self, keeps, t_lo, t_hi, update, before):
        """the statement's step: (keeps, out stream, S1, records); before: what the output buffer held"""
        out = before.copy()
        new, sums, recs = [], [], np.zeros(len(self.convs), dnscp.STATE_DTYPE)
        for i, (o, N, C, kk) in enumerate(self.convs):
            upd = update is None or i in update
            k, w, s, recs[i] = dnscp.reference_step(self.conv(i), keeps[i], t_lo[i] if upd else 0.0, t_hi[i] if upd else 0.0, upd)
            if not int(recs[i]["status"]) & dnscp.NONFINITE:
                out[o:o + N * C * kk] = w.ravel()
            new.append(k); sums.append(s)
        return new, out, sums, recs


def assert_state(got, want):
    for f in dnscp.STATE_DTYPE.names:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"record word {f}")
    assert got.tobytes() == want.tobytes()


def step_and_check(buf, keeps, t_lo, t_hi, update=None, shift=0, inplace=False, pruner=None):
    """one device step of `buf` against the statement; shift: elements the buffers are moved off their 16-byte alignment"""
    torch = _torch()
    dp = pruner or dnscp.DevicePruner(convs=buf.convs, n_total=buf.n_total)
    dense = torch.zeros(buf.n_total + 8, dtype=torch.float32, device="cuda:0")[shift:shift + buf.n_total]
    dense.copy_(torch.from_numpy(buf.w))
    out = dense if inplace else torch.full((buf.n_total + 8,), float(GAP_OUT), dtype=torch.float32, device="cuda:0")[shift:shift + buf.n_total]
    before = out.cpu().numpy()
    dp.set_keep(dict(enumerate(keeps)))
    dp.set_thresholds(t_lo, t_hi)
    dp.step(dense, out, update)
    torch.cuda.synchronize()
    wk, wout, ws, recs = buf.expect(keeps, t_lo, t_hi, update, before)
    got_k, got_s = dp.keeps(), dp.sums()
    for i in range(len(buf.convs)):
        np.testing.assert_array_equal(got_k[i], wk[i], err_msg=f"keep bytes of conv {i}")
        np.testing.assert_array_equal(got_s[i], ws[i], err_msg=f"S1 of conv {i}")
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), wout.view(np.uint32), err_msg="output stream")
    if not inplace:
        np.testing.assert_array_equal(dense.cpu().numpy().view(np.uint32), buf.w.view(np.uint32), err_msg="dense weights")
    assert_state(dp.state(), recs)
    return wk, recs


def mixed(rng, N, C, kk, low_frac=0.3):
    """a conv whose channels are a texture times a high or a low scale, signs mixed"""
    scale = np.where(rng.random(C) < low_frac, rng.uniform(0.01, 0.2, C), rng.uniform(0.7, 1.3, C))
    return (rng.standard_normal((N, C, kk)) * scale[None, :, None]).astype(np.float32)


def own_thresholds(buf, keeps=None):
    _, recs = buf.stats(keeps)
    return dnscp.thresholds(recs)


def ones(buf):
    return [np.ones(c[2], np.uint8) for c in buf.convs]


def test_conv_geometry_gaps_and_alignment():
    """5x16x1 (smaller than a block), 7x48x9 (straddles two blocks), 3x33x9, 64x4096x1 (the widest conv: 64 blocks, every LDS slot)
    and 1x16x49, at offsets off the 16-byte grid with marked gaps; stats first, then a step, with and without 16-byte accesses."""
    torch = _torch()
    rng = np.random.default_rng(1)
    parts, o = [], 1
    for N, C, kk in ((5, 16, 1), (7, 48, 9), (3, 33, 9), (64, 4096, 1), (1, 16, 49)):
        if (N, C, kk) == (7, 48, 9):
            o = 4000 - 1                                                        # [3999, 7023): both sides of element 4096
        assert o % 4
        parts.append((o, mixed(rng, N, C, kk)))
        o += N * C * kk + 5 + (o + N * C * kk + 5) % 2
        o += 1 - o % 2
    buf = Buf(parts)
    assert buf.convs[1][0] < 4096 < buf.convs[1][0] + 7 * 48 * 9
    dp = dnscp.DevicePruner(convs=buf.convs, n_total=buf.n_total)
    for shift in (0, 1):
        w = torch.zeros(buf.n_total + 8, dtype=torch.float32, device="cuda:0")[shift:shift + buf.n_total]
        w.copy_(torch.from_numpy(buf.w))
        dp.stats(w)
        torch.cuda.synchronize()
        sums, recs = buf.stats()
        assert_state(dp.state(), recs)
        for i, s in dp.sums().items():
            np.testing.assert_array_equal(s, sums[i])
        np.testing.assert_array_equal(w.cpu().numpy().view(np.uint32), buf.w.view(np.uint32))
        t_lo, t_hi = dp.thresholds()
        np.testing.assert_array_equal(t_lo, dnscp.thresholds(recs)[0])
        keeps, r = step_and_check(buf, ones(buf), t_lo, t_hi, shift=shift)
        assert (r["pruned"] > 0).any() and (r["kept_after"] % 16 == 0).all() and not r["status"].any()
    # a second step on other weights from the first one's keep bytes: pruned channels are revived, kept ones pruned
    rng2 = np.random.default_rng(2)
    buf2 = Buf([(c[0], mixed(rng2, *c[1:])) for c in buf.convs], buf.n_total)
    _, r2 = step_and_check(buf2, keeps, t_lo, t_hi)
    assert (r2["revived"] > 0).any() and (r2["pruned"] > 0).any()
    step_and_check(buf2, keeps, t_lo, t_hi, inplace=True, shift=1)


def test_sums_on_the_thresholds():
    """Four weights of 0.25 under a maximum of 1 make S1 = 2^31 exactly: a kept channel goes at S1 == B_lo and stays at S1 == B_lo + 1; a
    pruned one stays at S1 == B_hi and comes back at S1 == B_hi + 1."""
    w = np.full((4, 32, 1), 0.25, np.float32)
    w[0, 31, 0] = 1.0                                                           # E = 0; channel 31 stands apart
    buf = Buf([(3, w), (150, w), (300, w), (450, w)])
    S = 1 << 31
    assert int(buf.stats()[0][0][0]) == S
    t_on, t_under = 0.25, (S - 0.5) / (4.0 * 2.0 ** 31)                         # B = S and B = S - 1
    assert dnscp.bound_of(t_on, 4, 0, -1) == S and dnscp.bound_of(t_under, 4, 0, -1) == S - 1
    keeps = [np.ones(32, np.uint8), np.ones(32, np.uint8), np.zeros(32, np.uint8), np.zeros(32, np.uint8)]
    for k in keeps:
        k[31] = 1
    big = 1e30
    _, recs = step_and_check(buf, keeps, [t_on, t_under, 0.0, 0.0], [big, big, t_on, t_under])
    assert recs["B_lo"].tolist()[:2] == [S, S - 1] and recs["B_hi"].tolist()[2:] == [S, S - 1]
    assert recs["pruned"].tolist() == [31, 0, 0, 0] and recs["revived"].tolist() == [0, 0, 0, 31]
    assert int(recs["B_hi"][0]) == dnscp.I64_MAX                                # the clamp


def test_denormals_zeros_nonfinite_and_nan_thresholds():
    rng = np.random.default_rng(3)
    den = rng.integers(1, 1 << 20, (6, 20, 9)).astype(np.uint32).view(np.float32)      # denormals only: E from a leading bit
    den[:, :7, :] = (den[:, :7, :].view(np.uint32) >> 9).view(np.float32)
    zero = np.zeros((4, 24, 1), np.float32)
    zero[1, 3, 0] = -0.0
    bad = mixed(rng, 5, 32, 9)
    bad[2, 5, 1], bad[4, 30, 8] = np.nan, -np.inf
    fine = mixed(rng, 6, 48, 1)
    sparse = mixed(rng, 8, 40, 9, low_frac=0.0) * (rng.random((8, 40, 9)) < 0.1)       # negative variance: thresholds() gives NaN
    buf = Buf([(2, den), (1090, zero), (1201, bad), (2650, fine), (2950, fine), (4090, sparse.astype(np.float32))])
    t_lo, t_hi = own_thresholds(buf)
    assert np.isnan(t_lo[1]) and np.isnan(t_lo[5]) and not np.isnan(t_lo[[0, 3]]).any()
    t_lo[4], t_hi[4] = t_lo[3], np.nan                                          # one NaN of the two: only the revival is switched off
    keeps = ones(buf)
    keeps[4][::3] = 0
    keeps[5][:11] = 0
    _, recs = step_and_check(buf, keeps, t_lo, t_hi)
    assert recs["status"].tolist() == [0, dnscp.ALL_ZERO | dnscp.NAN_THRESHOLD, dnscp.NONFINITE, 0, dnscp.NAN_THRESHOLD, dnscp.NAN_THRESHOLD]
    assert int(recs["E"][0]) < -126 and int(recs["E"][1]) == dnscp.NO_EXP and int(recs["nonfinite"][2]) == 2
    assert int(recs["pruned"][0]) > 0 and int(recs["pruned"][4]) > 0 and int(recs["revived"][4]) == 0
    assert (int(recs["kept_before"][5]), int(recs["fixup"][5]), int(recs["kept_after"][5])) == (29, 3, 32)   # NaN: only the fix-up runs
    # an all-zero conv under real thresholds: every sum is 0 <= B_lo, everything goes, the floor brings 16 back
    t_lo[1], t_hi[1] = 0.5, 0.6
    _, recs = step_and_check(buf, keeps, t_lo, t_hi, shift=1)
    assert (int(recs["pruned"][1]), int(recs["fixup"][1]), int(recs["kept_after"][1])) == (24, 16, 16)


def test_recorded_reference_iterations_on_the_device():
    """The fixture's convs as one buffer: stats and thresholds from iteration 0's weights, then two steps in sequence.  After each the
    reference's own recorded masks (both hysteresis branches, both fix-up directions, the tie at 2.5, the floor at 16 with and without
    room for it, NaN thresholds from a negative variance)."""
    z = np.load(GOLDEN)
    n = int(z["n_cases"])
    bufs = []
    for it in (0, 1):
        parts, o = [], 1
        for c in range(n):
            w = z[f"c{c:02d}_s{it}_w"]
            parts.append((o, w.reshape(w.shape[0], w.shape[1], -1)))
            o += w.size + 3
        bufs.append(Buf(parts))
    t_lo, t_hi = own_thresholds(bufs[0])
    keeps = ones(bufs[0])
    seen = np.zeros(5, bool)
    for it in (0, 1):
        keeps, recs = step_and_check(bufs[it], keeps, t_lo, t_hi)
        for c in range(n):
            np.testing.assert_array_equal(keeps[c], z[f"c{c:02d}_s{it}_keep"], err_msg=f"case {c} iteration {it}")
        seen |= [(recs["pruned"] > 0).any(), (recs["revived"] > 0).any(), (recs["fixup"] > 0).any(), (recs["fixup"] < 0).any(),
                 (recs["status"] == dnscp.NAN_THRESHOLD).any()]
    assert seen.all()


def test_update_for_some_convs_only():
    rng = np.random.default_rng(5)
    buf = Buf([(4, mixed(rng, 8, 64, 9)), (4700, mixed(rng, 16, 48, 1)), (5500, mixed(rng, 4, 80, 9))])
    t_lo, t_hi = own_thresholds(buf)
    keeps = ones(buf)
    keeps[1][5:20] = 0
    keeps[1][7] = 200                                                           # any non-zero byte keeps, and stays as it is
    new, recs = step_and_check(buf, keeps, t_lo, t_hi, update=[0, 2])
    np.testing.assert_array_equal(new[1], keeps[1])
    assert recs["pruned"].tolist()[1] == 0 and recs["B_lo"].tolist()[1] == 0 and int(recs["kept_after"][1]) == 48 - 14
    assert int(recs["pruned"][0]) > 0 and int(recs["pruned"][2]) > 0
    step_and_check(buf, keeps, t_lo, t_hi, update=[], inplace=True)
    step_and_check(buf, keeps, t_lo, t_hi, update=[1], inplace=True)


def test_graph_replay_on_refilled_weights_equals_fresh_calls():
    torch = _torch()
    rng = np.random.default_rng(6)
    shapes = ((2, 12, 40, 9), (4400, 32, 64, 1), (6500, 3, 16, 49))
    fills = [Buf([(o, mixed(rng, N, C, kk)) for o, N, C, kk in shapes]) for _ in range(2)]
    t_lo, t_hi = own_thresholds(fills[0])
    dp = dnscp.DevicePruner(convs=fills[0].convs, n_total=fills[0].n_total)
    dense = torch.from_numpy(fills[0].w).to("cuda:0")
    out = torch.full_like(dense, float(GAP_OUT))
    dp.set_thresholds(t_lo, t_hi)
    replay = dp.capture(dense, out, update=[0, 1])
    start = ones(fills[0])
    start[2][3] = 0
    for b in (fills[1], fills[0], fills[1]):
        dense.copy_(torch.from_numpy(b.w)); out.fill_(float(GAP_OUT))
        dp.set_keep(dict(enumerate(start)))
        replay()
        torch.cuda.synchronize()
        wk, wout, ws, recs = b.expect(start, t_lo, t_hi, [0, 1], np.full(b.n_total, GAP_OUT, np.float32))
        for i, k in dp.keeps().items():
            np.testing.assert_array_equal(k, wk[i])
        for i, s in dp.sums().items():
            np.testing.assert_array_equal(s, ws[i])
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), wout.view(np.uint32))
        assert_state(dp.state(), recs)


def _tiny():
    t = cfg.tiny_tables(widths=(48, 64))
    q = synth.synth_q_values(t, 5, spread=2)
    return t, q, synth.synth_model(t, q, 5).copy()


def test_compact_equals_reference_compact():
    _torch()
    t, q, model = _tiny()
    model = (model + np.arange(model.size, dtype=np.float32) * np.float32(2.0 ** -20)).astype(np.float32)   # every element its own value
    rng = np.random.default_rng(7)
    plan = cfg.build_plan(t)
    keeps = {}
    for l, n in zip(dnscp.prunable_rows(t), (16, 32, 48, 1)):
        k = np.zeros(plan[l].C, np.uint8)
        k[rng.permutation(plan[l].C)[:n]] = 1
        keeps[l] = k
    t2, stream, q2 = dnscp.prune_model(t, model, q, keeps)
    np.testing.assert_array_equal(stream.view(np.uint32), dnscp.reference_compact(t, keeps, model).view(np.uint32))
    assert stream.size == cfg.model_float_count(t2) and q2.size == cfg.q_value_count(t2)
    assert [t2["kInputChannels"][l] for l in keeps] == [16, 32, 48, 1]


def test_pruned_network_equals_the_masked_network_through_the_engine():
    """tiny (48, 64): some input channels of the prunable rows scaled down, stats -> thresholds -> step prunes them.  The engine on the
    full tables with the masked stream and on prune_model's tables, stream and Q: the logits and every kept channel of every row are
    bit-identical (integer accumulations; a zero weight adds nothing)."""
    torch = _torch()
    t, q, model = _tiny()
    rows = dnscp.prunable_rows(t)
    assert rows == [3, 4, 6, 7]
    plan = cfg.build_plan(t)
    rng = np.random.default_rng(8)
    dp = dnscp.DevicePruner(t)
    low = {}
    for (o, N, C, kk), l in zip(dp.convs, rows):
        low[l] = np.sort(rng.permutation(C)[:16])
        w = model[o:o + N * C * kk].reshape(N, C, kk)
        w[:, low[l], :] *= np.float32(2.0 ** -6)                                # still powers of two for the engine
    dense = torch.from_numpy(model).to("cuda:0")
    masked = dense.clone()                                                      # (a step writes the prunable filters only)
    dp.stats(dense)
    dp.thresholds()
    dp.step(dense, masked)
    torch.cuda.synchronize()
    keeps = dp.keeps()
    for l in (3, 6):                                                            # (the 1x1 rows' 64 weights a channel scatter more: the fix-up decides there)
        np.testing.assert_array_equal(np.flatnonzero(keeps[l] == 0), low[l])
    assert all(int(k.sum()) == 32 for k in keeps.values())
    want, wk, _, recs = dnscp.reference_model_step(t, model, None, {l: dnscp.thresholds(r) for l, r in zip(rows, dp.state())})
    np.testing.assert_array_equal(masked.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert_state(dp.state(), recs)
    t2, stream, q2 = dnscp.prune_model(t, masked.cpu().numpy(), q, dp)
    assert t2["kInputChannels"][3] == 32 and "MACs kept" in dnscp.report(t, keeps, recs)
    x = torch.from_numpy(synth.synth_images(t, 4, 5)).to("cuda:0")
    full = network.NetWork(t)
    full.Init(masked.cpu().numpy(), synth.q_text(q), device="cuda:0", pack_mode=0)
    small = network.NetWork(t2)
    small.Init(stream, synth.q_text(q2), device="cuda:0", pack_mode=0)
    ra, rb = network.Runner(None, full), network.Runner(None, small)
    np.testing.assert_array_equal(ra.run_batch(x, keep_all=True).cpu().numpy(), rb.run_batch(x, keep_all=True).cpu().numpy())
    out_keep = {plan[l].src: keeps[l] != 0 for l in rows}
    for L in plan:
        a, b = ra.read_layer(L.index, 4), rb.read_layer(L.index, 4)
        a = np.asarray(a)[:, out_keep[L.index]] if L.index in out_keep else np.asarray(a)
        np.testing.assert_array_equal(a, np.asarray(b), err_msg=f"row {L.index}")
