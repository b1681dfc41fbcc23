"""INQ weight quantisation on the device (tf2_inq_step, csrc/weight_inq.hip) against the numpy statement tf2_amd.inq.reference_step:
weights, masks, codes and every word of the state as bits -- segment geometry, the select's passes, rounding and flushing, status
bits, the recorded reference schedules, graph replay, and a float stream through quantize_model into the engine."""
import os

import numpy as np
import pytest

from oracle import netref
from tf2_amd import config as cfg, inq, network, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_inq.npz")
GAP_W, GAP_M, GAP_C = np.float32(123.456), 1, 0xAA          # what lies between the segments: must come back untouched


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch


class Buf:
    """segments [(offset, weights, mask)] laid into one flat buffer with marked gaps"""

    def __init__(self, parts, n_total=None):
        self.segs = [(int(o), int(np.size(w))) for o, w, _ in parts]
        self.n_total = int(n_total if n_total is not None else self.segs[-1][0] + self.segs[-1][1] + 3)
        self.w = np.full(self.n_total, GAP_W, np.float32)
        self.m = np.full(self.n_total, GAP_M, np.uint8)
        for o, w, m in parts:
            w = np.asarray(w, np.float32).ravel()
            self.w[o:o + w.size] = w
            self.m[o:o + w.size] = np.asarray(m, np.uint8).ravel()

    def expect(self, prev, cur, n_values=7, exp_floor=-127):
        w, m = self.w.copy(), self.m.copy()
        c = np.full(self.n_total, GAP_C, np.uint8)
        recs = np.zeros(len(self.segs), inq.STATE_DTYPE)
        for i, (o, n) in enumerate(self.segs):
            w[o:o + n], m[o:o + n], recs[i], c[o:o + n] = inq.reference_step(self.w[o:o + n], self.m[o:o + n], prev, cur, n_values, exp_floor)
        return w, m, c, recs


def assert_state(got, want, names=None):
    for f in inq.STATE_DTYPE.names:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"state word {f}" + (f" {names}" if names else ""))
    assert got.tobytes() == want.tobytes()


def run_and_check(buf, prev, cur, n_values=7, exp_floor=-127, with_codes=True, shift=0):
    """one device step of `buf` against the statement; shift: elements the buffers are moved off their 16-byte alignment"""
    torch = _torch()
    dq = inq.DeviceQuantizer(segs=buf.segs, n_total=buf.n_total)
    w = torch.zeros(buf.n_total + 8, dtype=torch.float32, device="cuda:0")[shift:shift + buf.n_total]
    m = torch.zeros(buf.n_total + 8, dtype=torch.uint8, device="cuda:0")[shift:shift + buf.n_total]
    c = torch.zeros(buf.n_total + 8, dtype=torch.uint8, device="cuda:0")[shift:shift + buf.n_total]
    w.copy_(torch.from_numpy(buf.w)); m.copy_(torch.from_numpy(buf.m)); c.fill_(GAP_C)
    dq.step(w, m, prev, cur, exp_floor=exp_floor, codes=c if with_codes else None, n_values=n_values)
    torch.cuda.synchronize()
    ww, wm, wc, recs = buf.expect(prev, cur, n_values, exp_floor)
    np.testing.assert_array_equal(w.cpu().numpy().view(np.uint32), ww.view(np.uint32), err_msg="weights")
    np.testing.assert_array_equal(m.cpu().numpy(), wm, err_msg="mask")
    if with_codes:
        np.testing.assert_array_equal(c.cpu().numpy(), wc, err_msg="codes")
    else:
        assert (c.cpu().numpy() == GAP_C).all()
    assert_state(dq.state(), recs)
    return recs, ww, wm


def test_segment_geometry_and_masks():
    rng = np.random.default_rng(1)
    parts = []
    for o, n in ((1, 1), (5, 3), (10, 255), (267, 257), (4094, 4099)):          # offsets off the 16-byte grid, gaps, chunk boundaries crossed
        assert o % 4
        parts.append((o, rng.standard_normal(n) * 0.1, np.ones(n)))
    q = np.ldexp(1.0, -rng.integers(1, 7, 50)) * np.where(rng.random(50) < 0.5, -1, 1)
    parts.append((8195, q, np.zeros(50)))                                       # already all quantised
    parts.append((8250, np.zeros(33), np.ones(33)))                             # all zero
    half = rng.standard_normal(700) * 0.3                                       # half quantised before: the range comes from mask 0
    hm = np.ones(700)
    big = np.abs(half) >= np.sort(np.abs(half))[350]
    half[big] = inq.reference_step(half, hm, 0.0, 1.0)[0][big]
    hm[big] = 0
    parts.append((8301, half, hm))
    buf = Buf(parts)
    for shift in (0, 1):                                                        # 16-byte path, and buffers that allow none
        recs, _, wm = run_and_check(buf, 0.5, 0.75, shift=shift)
        assert recs["status"].tolist() == [0, 0, 0, 0, 0, 0, inq.ALL_ZERO, 0]
        assert int(recs["max_exp"][5]) == -100 and int(recs["n_update"][7]) > 0 and int(recs["n_update"][4]) > 0
    run_and_check(buf, 0.0, 1.0, with_codes=False)
    recs, _, wm = run_and_check(buf, 0.0, 1.0)
    assert not wm[4094:4094 + 4099].any()


def test_selection_and_threshold():
    rng = np.random.default_rng(2)
    f = np.float32
    ties = rng.choice(np.asarray([0.3, 0.11, 0.07, 0.02, 0.004], f), 1000) * np.where(rng.random(1000) < 0.5, -1, 1)
    sparse = rng.standard_normal(500) * 0.2
    sparse[rng.permutation(500)[:300]] = 0.0                                    # 60 % zeros: thr = 0
    zeros = rng.standard_normal(64) * 0.2
    zeros[:40:2], zeros[1:40:2] = 0.0, -0.0                                     # both zeros, selected
    base = np.float32(0.1).view(np.uint32) & ~np.uint32(0xff)
    low8 = (base + rng.permutation(256).astype(np.uint32)).view(f)              # differ in the lowest 8 mantissa bits only: the last pass decides
    low8 = np.concatenate([low8, low8[:77]]) * np.where(rng.random(333) < 0.5, -1, 1).astype(f)
    expo = np.ldexp(1.0, -rng.integers(0, 40, 600)).astype(f)                   # differ in the exponent only: the first pass decides
    mid = ((np.float32(0.2).view(np.uint32) & ~np.uint32(0x7fff80)) | (rng.integers(0, 1 << 16, 900).astype(np.uint32) << 7)).view(f)
    parts, o = [], 3
    for w in (ties, sparse, zeros, low8, expo, mid):
        parts.append((o, w, np.ones(w.size)))
        o += w.size + 5
    buf = Buf(parts)
    recs, ww, wm = run_and_check(buf, 0.0, 0.5)
    assert int(recs["n1"][0] - wm[3:1003].sum()) > int(recs["n_update"][0]) > 0  # ties: more selected than n_update
    assert int(recs["thr"][1]) == 0 and int(recs["thr"][2]) == 0 and int(recs["n_update"][1]) > 0
    assert int(recs["hist"][2][7]) >= 40
    assert int(recs["thr"][3]) & 0xff and int(recs["thr"][3]) >> 8 == int(base) >> 8
    for prev, cur in ((0.5, 0.8), (0.3, 0.37), (0.0, 1.0)):
        run_and_check(buf, prev, cur)


def _triplets(lo, hi):
    out = []
    for E in range(lo, hi + 1):
        b = np.float32(np.ldexp(1.5, E)).view(np.uint32)
        out += [np.uint32(b - 1).view(np.float32), np.uint32(b).view(np.float32), np.uint32(b + 1).view(np.float32)]
    return np.asarray(out, np.float32)


def test_rounding_and_flushing():
    rng = np.random.default_rng(3)
    f = np.float32
    wide = _triplets(-126, 3)                                                   # every normal boundary under a large maximum
    den = np.asarray([1, 2, 3, 5, 6, 7, 0x2fffff, 0x300000, 0x300001, 0x5fffff, 0x600000, 0x600001, 0x7fffff], np.uint32).view(f)
    seg_a = np.concatenate([wide, den, -den, f([12.0])]) * np.where(np.arange(wide.size + 2 * den.size + 1) % 2, -1, 1).astype(f)
    near = _triplets(-13, 0)                                                    # inside a 15-magnitude window: every triplet is emitted
    small = np.concatenate([rng.standard_normal(400) * 3e-4, rng.standard_normal(400) * 1e-7, ldexp_tail()])   # max_exp about -10
    tiny = np.asarray([2.0 ** -125, -1.5 * 2.0 ** -126, 2.0 ** -127, 3 * 2.0 ** -129, 2.0 ** -149], f)   # a denormal window
    huge = np.asarray([3.4e38, -2.6e38, 1e38], f)                               # e = 128 is emitted as 2^127
    parts, o = [], 2
    for w in (seg_a, near, small, tiny, huge):
        parts.append((o, w, np.ones(w.size)))
        o += w.size + 6
    buf = Buf(parts)
    recs, ww, _ = run_and_check(buf, 0.0, 1.0)
    assert int(recs["flushed_min"][0]) > 300 and int(recs["max_exp"][0]) == 4 and int(recs["over_one"][0]) > 0
    assert int(recs["flushed_min"][2]) > 300 and int(recs["flushed_floor"][2]) == 0
    o2 = buf.segs[2][0]
    flushed = ww[o2:o2 + buf.segs[2][1]]
    assert (flushed.view(np.uint32)[flushed == 0] == 0).all()                   # +0.0, never -0.0
    assert int(recs["max_exp"][4]) == 128 and np.isfinite(ww).all()
    recs15, _, _ = run_and_check(buf, 0.0, 1.0, n_values=15)
    assert int(recs15["flushed_min"][1]) == 0 and int(recs15["hist"][1][15]) > 0  # k > 6 has no 4-bit code
    recs14, _, _ = run_and_check(buf, 0.0, 1.0, exp_floor=-14)                  # the same segments under the engine's floor
    assert int(recs14["min_exp"][2]) < -14 and int(recs14["flushed_floor"][2]) > 0 and int(recs14["flushed_floor"][3]) == 4
    assert int(recs14["flushed_min"][2]) < int(recs["flushed_min"][2]) + 1 and int(recs14["flushed_floor"][0]) == 0
    run_and_check(buf, 0.0, 0.5, exp_floor=-14)
    run_and_check(buf, 0.0, 1.0, exp_floor=-150)


def ldexp_tail():
    return np.asarray([2.0 ** -15, -2.0 ** -16, 2.0 ** -14, 1.49 * 2.0 ** -15, 1.5 * 2.0 ** -15], np.float32)


def test_status_bits_leave_their_tensor_alone():
    rng = np.random.default_rng(4)
    ok = rng.standard_normal(300) * 0.2
    grew = np.concatenate([[0.25, -0.125, 0.0], rng.standard_normal(97) * 0.05, [0.9]])
    gm = np.ones(101); gm[:3] = 0
    fine = np.concatenate([[0.25, -0.125], rng.uniform(-0.37, 0.37, 98)])       # up to the quantised maximum's own band: no growth
    fm = np.ones(100); fm[:2] = 0
    bad = rng.standard_normal(200) * 0.2
    bad[17], bad[150] = np.nan, -np.inf
    bm = np.ones(200); bm[150] = 0
    buf = Buf([(1, ok, np.ones(300)), (307, grew, gm), (413, fine, fm), (518, bad, bm), (4090, ok[:99], np.ones(99))])
    recs, ww, wm = run_and_check(buf, 0.5, 0.75)
    assert recs["status"].tolist() == [0, inq.RANGE_GREW, 0, inq.NONFINITE, 0]
    assert int(recs["nonfinite"][3]) == 2 and recs["n_update"].tolist()[1] == 0 and recs["n_update"].tolist()[3] == 0
    assert all(int(recs["n_update"][i]) > 0 for i in (0, 2, 4))
    np.testing.assert_array_equal(ww[307:408].view(np.uint32), buf.w[307:408].view(np.uint32))
    np.testing.assert_array_equal(wm[518:718], buf.m[518:718])


def test_recorded_reference_schedules_on_the_device():
    """The fixture's tensors as the segments of one buffer per schedule, stepped on the device; between steps the still-float weights
    are replaced ON THE DEVICE by the fixture's perturbed ones.  After every step: the reference's own recorded output."""
    torch = _torch()
    z = np.load(GOLDEN)
    groups = {}
    for c in range(int(z["n_cases"])):
        tag = f"c{c:02d}"
        steps = int(z[tag + "_steps"])
        if int(z[tag + "_s0_exp"][2]) != 7:
            continue
        sched = tuple(float(z[f"{tag}_s{k}_par"][1]) for k in range(steps))
        key = next((g for g in groups if g[:len(sched)] == sched or sched[:len(g)] == g), None)
        if key is not None and len(sched) > len(key):
            groups[sched] = groups.pop(key)
            key = sched
        groups.setdefault(key or sched, []).append((tag, steps))
    assert len(groups) >= 2
    for sched, cases in groups.items():
        parts, o = [], 1
        for tag, steps in cases:
            w = z[tag + "_s0_w_in"].ravel()
            parts.append((o, w, np.ones(w.size)))
            o += w.size + 3
        buf = Buf(parts)
        dq = inq.DeviceQuantizer(segs=buf.segs, n_total=buf.n_total)
        w_dev, m_dev = torch.from_numpy(buf.w).to("cuda:0"), torch.from_numpy(buf.m).to("cuda:0")
        prev = 0.0
        for k, cur in enumerate(sched):
            fresh = np.zeros(buf.n_total, np.float32)
            for (tag, steps), (so, n) in zip(cases, buf.segs):
                if k < steps:
                    fresh[so:so + n] = z[f"{tag}_s{k}_w_in"].ravel()
            in_seg = torch.zeros(buf.n_total, dtype=torch.bool, device="cuda:0")
            for (tag, steps), (so, n) in zip(cases, buf.segs):
                if k < steps:
                    in_seg[so:so + n] = True
            w_dev = torch.where(in_seg & (m_dev != 0), torch.from_numpy(fresh).to("cuda:0"), w_dev).contiguous()
            before_w, before_m = w_dev.cpu().numpy(), m_dev.cpu().numpy()
            dq.step(w_dev, m_dev, prev, cur)
            torch.cuda.synchronize()
            got_w, got_m, st = w_dev.cpu().numpy(), m_dev.cpu().numpy(), dq.state()
            for i, ((tag, steps), (so, n)) in enumerate(zip(cases, buf.segs)):
                if k < steps:
                    p = f"{tag}_s{k}_"
                    np.testing.assert_array_equal(before_w[so:so + n].view(np.uint32), z[p + "w_in"].ravel().view(np.uint32), err_msg=p + "input")
                    np.testing.assert_array_equal(got_w[so:so + n].view(np.uint32), z[p + "w_out"].ravel().view(np.uint32), err_msg=p)
                    np.testing.assert_array_equal(got_m[so:so + n], z[p + "mask_out"].ravel(), err_msg=p)
                    assert (int(st["max_exp"][i]), int(st["min_exp"][i])) == tuple(int(v) for v in z[p + "exp"][:2]), p
                want = inq.reference_step(before_w[so:so + n], before_m[so:so + n], prev, cur)
                np.testing.assert_array_equal(got_w[so:so + n].view(np.uint32), want[0].view(np.uint32))
                assert st[i].tobytes() == want[2].tobytes(), (tag, k)
            prev = cur
        assert not any(got_m[so:so + n].any() for so, n in buf.segs)


def test_graph_replay_on_refilled_buffers_equals_fresh_calls():
    torch = _torch()
    rng = np.random.default_rng(6)
    fills = []
    for seed in (0, 1):
        parts = [(2, rng.standard_normal(5000) * 0.1, rng.random(5000) < 0.8), (5003, rng.standard_normal(77), np.ones(77)),
                 (5090, rng.choice([0.5, 0.25, -0.125, 0.0], 640), rng.random(640) < 0.5)]
        fills.append(Buf(parts))
    # the quantised part of a segment must hold powers of two under the float part's range for a clean step: make it so
    for b in fills:
        for o, n in b.segs:
            q = b.m[o:o + n] == 0
            b.w[o:o + n][q] = np.ldexp(1.0, np.minimum(inq.exp_of(b.w[o:o + n][q]), 3)).astype(np.float32) * (b.w[o:o + n][q] != 0)
            b.w[o + int(np.argmax(q))] = 8.0
    n_total = fills[0].n_total
    dq = inq.DeviceQuantizer(segs=fills[0].segs, n_total=n_total)
    w = torch.zeros(n_total, dtype=torch.float32, device="cuda:0")
    m = torch.ones(n_total, dtype=torch.uint8, device="cuda:0")
    c = torch.zeros(n_total, dtype=torch.uint8, device="cuda:0")
    w.copy_(torch.from_numpy(fills[0].w)); m.copy_(torch.from_numpy(fills[0].m))
    replay = dq.capture(w, m, 0.25, 0.625, exp_floor=-14, codes=c)
    for b in (fills[1], fills[0], fills[1]):
        w.copy_(torch.from_numpy(b.w)); m.copy_(torch.from_numpy(b.m)); c.fill_(GAP_C)
        replay()
        torch.cuda.synchronize()
        ww, wm, wc, recs = b.expect(0.25, 0.625, exp_floor=-14)
        assert not recs["status"].any() and (recs["n_update"] > 0).all()
        np.testing.assert_array_equal(w.cpu().numpy().view(np.uint32), ww.view(np.uint32))
        np.testing.assert_array_equal(m.cpu().numpy(), wm)
        np.testing.assert_array_equal(c.cpu().numpy(), wc)
        assert_state(dq.state(), recs)


def test_float_stream_to_correct_logits():
    """The smallest network of the parity tests: Gaussian float filters -> quantize_model on the device -> no misfit left -> the
    engine's logits equal the oracle's on the quantised stream.  The float stream itself is what the engine misreads in silence."""
    torch = _torch()
    t = cfg.tiny_tables()
    q = synth.synth_q_values(t, 5, spread=2)
    model = synth.synth_model(t, q, 5).copy()
    rng = np.random.default_rng(11)
    for name, o, n in inq.segments_of(t, ("filter",)):
        model[o:o + n] = np.clip(rng.standard_normal(n) * 0.25, -0.95, 0.95).astype(np.float32)
    before = inq.engine_check(t, model)
    assert all(r["misfit"] > 0.9 * r["count"] for r in before)
    for schedule in ((1.0,), (0.5, 0.75, 0.875, 1.0)):
        out, rep = inq.quantize_model(t, model, schedule=schedule, exp_floor=-14)
        want = model.copy()
        mk = None
        prev = 0.0
        for cur in schedule:
            want, mk, recs, codes = inq.reference_model_step(t, want, mk, prev, cur, exp_floor=-14)
            prev = cur
        np.testing.assert_array_equal(out.view(np.uint32), want.view(np.uint32))
        for r, rec, (name, o, n) in zip(rep, recs, inq.segments_of(t)):
            assert r["name"] == name and int(r["max_exp"]) == int(rec["max_exp"]) and (r["hist"] == rec["hist"]).all()
            np.testing.assert_array_equal(r["codes"], codes[o:o + n])
        check = inq.engine_check(t, out)
        assert all(r["misfit"] == 0 for r in check), check
        assert "engine misfits 0" in inq.report(rep, check)
    x = synth.synth_images(t, 4, 5)
    net = network.NetWork(t)
    net.Init(out, synth.q_text(q), device="cuda:0", pack_mode=0)
    got = network.Runner(None, net).run_batch(torch.from_numpy(x).to("cuda:0")).cpu().numpy()
    ref = netref.RefNet(t, q, out)
    np.testing.assert_array_equal(got, ref.logits(ref.run(x)))
    with pytest.raises(ValueError):
        inq.quantize_model(t, model, schedule=(0.5, 0.9))
    nan = model.copy()
    nan[inq.segments_of(t)[0][1]] = np.nan
    with pytest.raises(ValueError, match="status"):
        inq.quantize_model(t, nan)
