"""CAQ calibration on the device (tf2_caq_*, csrc/act_caq.hip): the stores of caq.DeviceCalibrator -- and of bare tf2_caq_range /
tf2_caq_error calls on rows that belong to no network -- equal caq.reference_range / reference_error as integers, one assertion over
the whole store, on the float maps of fidelity.float_refs on the device (copied to the host for the statement).  The regimes come from
tests/test_audit.py, the poisoned values from tests/test_caq.py."""
import ctypes as C
import os

import numpy as np
import pytest

from tf2_amd import _lib, caq as Q, config as cfg, fidelity as F, network, synth
from tests.test_audit import case_inputs
from tests.test_caq import POISON, tie

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPECIAL = np.array(POISON + [tie(j) for j in range(4)], np.float32)


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).to(DEV)


def poison(a: np.ndarray, seed: int) -> np.ndarray:
    """a copy with the values of the CPU test at seeded positions (as many as fit)"""
    out = np.array(a, np.float32)
    flat = out.reshape(-1)
    pos = np.random.default_rng(seed).choice(flat.size, size=min(flat.size, SPECIAL.size), replace=False)
    flat[pos] = SPECIAL[:pos.size]
    return out


def check_program(t, model, x, cal=None, poisoned=False, error=True):
    """one observed batch on empty stores against the statement, both passes; returns (calibrator, range store, error store)"""
    torch = _torch()
    xf = np.asarray(x, np.float32)                           # int8 images go in as the floats of their values
    xd = _dev(xf)
    refs = F.float_refs(t, model, xd, device=DEV)
    if poisoned:
        refs = [_dev(poison(r.cpu().numpy(), 100 + l)) for l, r in enumerate(refs)]
        xd = _dev(poison(xf, 99))
    host = [r.cpu().numpy() for r in refs]
    xh = xd.cpu().numpy()
    cal = cal or Q.DeviceCalibrator(t, xf.shape[1:], DEV)
    cal.reset()
    cal.observe(xd, refs)
    got = cal.range_store()
    np.testing.assert_array_equal(got, Q.reference_range(host, xh), err_msg="RANGE store against the statement")
    assert got.shape == (cal.records, 70) and (got[:, Q.HIST:].sum(1) == got[:, Q.N] - got[:, Q.ZEROS]).all()
    err = None
    if error:
        cal.set_base(Q.q_max(got))
        cal.observe_error(xd, refs)
        err = cal.error_store()
        np.testing.assert_array_equal(err, Q.reference_error(host, xh, cal.qb), err_msg="ERROR store against the statement")
        assert (err[:, Q.E_N] == got[:, Q.N]).all() and (err[:, Q.E_NONFINITE] == got[:, Q.NONFINITE]).all()
    torch.cuda.synchronize()
    return cal, got, err


# ---- 1. the small programs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tiny_benign", "tiny_saturate", "fire_float", "fire_int8"])
@pytest.mark.parametrize("batch", [3, 1])
def test_small_programs(case, batch):
    t, q, model, x = case_inputs(case, batch)
    cal, got, err = check_program(t, model, x)
    rows = cal.rows
    values = np.concatenate([np.full(r["C"], batch * r["HW"]) for r in rows])
    assert (got[:, Q.N] + got[:, Q.NONFINITE] == values).all()
    assert err[:, Q.E_CLIPPED].sum() == 0 and err[:, Q.E_CLIPPED + 1].sum() > 0          # Qb = fit(peak): nothing clips at j = 0
    if case.startswith("tiny"):
        assert {r["HW"] for r in rows[1:]} >= {36, 9, 1} and sorted({r["C"] for r in rows}) == [3, 10, 16, 32]
    clean = got[:, Q.NONFINITE].copy()
    # the same program with the poisoned values in every map
    _, got, err = check_program(t, model, x, cal=cal, poisoned=True)
    for r in rows:
        if batch * r["C"] * r["HW"] >= SPECIAL.size:
            part = slice(r["first"], r["first"] + r["C"])
            assert got[part, Q.NONFINITE].sum() - clean[part].sum() in (1, 2, 3) and got[part, Q.NEGATIVES].sum() >= 1, r


# ---- 2. bare rows: no network, buffers that start one float into their allocation ----------------------------------------------------
class Bare:
    """rows (C, HW) at one batch behind tf2_caq_range / tf2_caq_error themselves; record ranges in row order"""

    def __init__(self, shapes, batch, seed, qb=None):
        torch = _torch()
        self.shapes, self.batch = list(shapes), batch
        rng = np.random.default_rng(seed)
        self.host, self.dev, self.keep = [], [], []
        firsts, at = [], 0
        for i, (c, hw) in enumerate(self.shapes):
            a = rng.standard_normal((batch, c, hw)) * 10.0 ** rng.integers(-3, 4, (1, c, 1))
            a = poison(np.where(rng.random(a.shape) < 0.3, 0.0, a), seed * 1000 + i)
            whole = torch.empty(a.size + 5, dtype=torch.float32, device=DEV)
            view = whole[1:1 + a.size]                                  # no plane starts 16-byte aligned where C * HW is odd too
            view.copy_(torch.from_numpy(a.reshape(-1)))
            assert view.data_ptr() % 16 == 4
            self.host.append(a); self.dev.append(view); self.keep.append(whole)
            firsts.append(at)
            at += c
        self.records = at
        self.desc = (_lib.CaqRow * len(self.shapes))()
        for d, (c, hw), f in zip(self.desc, self.shapes, firsts):
            d.C, d.HW, d.first_record = c, hw, f
        self.firsts = firsts
        self.qb = np.zeros(at, np.int64) if qb is None else np.asarray(qb, np.int64)
        self.scales = _dev(Q.scale_of(self.qb))
        self.rng = torch.zeros(at * 70, dtype=torch.int64, device=DEV)
        self.err = torch.zeros(at * 12, dtype=torch.int64, device=DEV)

    def ptrs(self, skip=()):
        return (C.c_void_p * len(self.shapes))(*[None if i in skip else v.data_ptr() for i, v in enumerate(self.dev)])

    def run(self, skip=()):
        torch = _torch()
        L, s = _lib.lib(), torch.cuda.current_stream(DEV).cuda_stream
        p, n = self.ptrs(skip), len(self.shapes)
        _lib.check(L.tf2_caq_range(self.desc, p, n, self.batch, self.rng.data_ptr(), self.rng.numel() * 8, s))
        _lib.check(L.tf2_caq_error(self.desc, p, n, self.batch, self.scales.data_ptr(), self.err.data_ptr(), self.err.numel() * 8, s))
        torch.cuda.synchronize()
        return self.rng.cpu().numpy().reshape(-1, 70), self.err.cpu().numpy().reshape(-1, 12)

    def statement(self, skip=()):
        r = np.concatenate([Q.empty_range(a.shape[1]) if i in skip else Q.range_records(a) for i, a in enumerate(self.host)])
        e = np.concatenate([Q.empty_error(a.shape[1]) if i in skip else Q.error_records(a, self.qb[f:f + a.shape[1]])
                            for i, (a, f) in enumerate(zip(self.host, self.firsts))])
        return r, e


# the shapes of the issue, one pixel past the slab (a plane, and two planes together), a wave's share of it and a 16-byte group, and
# both sides of every change in how a wave's lanes are dealt over planes ((HW + 6) / 4 groups a plane: 64 at HW = 250, 32 at HW = 122)
BARE = [(1, 1), (3, 1), (5, 49), (64, 1025), (65, 4097), (2, Q.SLAB + 1), (3, Q.SLAB // 2 + 1), (3, Q.SLAB // 4 + 1), (3, Q.SLAB // 8 + 1),
        (3, Q.GROUP + 1), (3, Q.GROUP), (2, 249), (2, 250), (3, 125), (3, 126), (7, 2), (5, 3), (3, 196)]


def test_bare_rows_on_unaligned_buffers():
    b = Bare(BARE, 2, seed=1)
    got_r, got_e = b.run()
    want_r, want_e = b.statement()
    np.testing.assert_array_equal(got_r, want_r)
    np.testing.assert_array_equal(got_e, want_e)
    assert got_r[:, Q.NONFINITE].sum() >= 3 * (len(BARE) - 2) and got_e[:, Q.E_REF_CLAMPED].sum() >= len(BARE) - 2


def test_more_rows_than_one_launch_takes():
    shapes = [(1 + i % 3, 1 + i % 7) for i in range(Q.ROWS_PER_LAUNCH + 1)] + [(4, 300)]
    b = Bare(shapes, 2, seed=2)
    got_r, got_e = b.run()
    want_r, want_e = b.statement()
    np.testing.assert_array_equal(got_r, want_r)
    np.testing.assert_array_equal(got_e, want_e)


def test_base_exponents_from_minus_64_to_64():
    qb = np.array([-64, 0, 64, -64, 0, 64, 13, -7])
    b = Bare([(8, 49), (8, 1)], 2, seed=3, qb=np.concatenate([qb, qb[::-1]]))
    for a, f in zip(b.host, b.firsts):                        # values around each channel's own rail: some clip at every candidate
        c = a.shape[1]
        a[...] = (np.random.default_rng(f).uniform(-200, 200, a.shape) * 2.0 ** -b.qb[f:f + c].astype(np.float64).reshape(1, c, 1)).astype(np.float32)
        a[...] = poison(a, 7 + f)
    for a, v in zip(b.host, b.dev):
        v.copy_(_torch().from_numpy(a.reshape(-1)))
    got_r, got_e = b.run()
    want_r, want_e = b.statement()
    np.testing.assert_array_equal(got_r, want_r)
    np.testing.assert_array_equal(got_e, want_e)
    assert (got_e[:8, Q.E_CLIPPED:Q.E_CLIPPED + 4] > 0).all() and (got_e[:8, Q.E_SUM_D2] > 0).all()


def test_null_rows_keep_their_records():
    b = Bare([(3, 49), (5, 1), (2, 300), (4, 10)], 2, seed=4)
    r1, e1 = b.run()
    skip = {1, 2}
    r2, e2 = b.run(skip=skip)
    sr, se = b.statement(skip=skip)
    np.testing.assert_array_equal(r2, Q.combine_range(r1, sr))
    np.testing.assert_array_equal(e2, Q.combine_error(e1, se))
    np.testing.assert_array_equal(r2[3:10], r1[3:10])


# ---- 3. accumulation and order ---------------------------------------------------------------------------------------------------------
def test_graph_replays_accumulate_over_refilled_buffers():
    torch = _torch()
    t, q, model, _ = case_inputs("tiny_benign", 3)
    xs = [synth.synth_images(t, 3, s).astype(np.float32) for s in (1, 4, 5)]
    sets = [F.float_refs(t, model, _dev(x), device=DEV) for x in xs]
    cal = Q.DeviceCalibrator(t, xs[0].shape[1:], DEV)
    buf = _dev(xs[0]).clone()
    rbuf = [r.clone() for r in sets[0]]
    qb = np.arange(cal.records) % 9 - 2
    cal.set_base(qb)
    replay_r = cal.capture(buf, rbuf)
    replay_e = cal.capture(buf, rbuf, error=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(cal.range_store(), Q.empty_range(cal.records))          # capture itself observed nothing
    np.testing.assert_array_equal(cal.error_store(), Q.empty_error(cal.records))
    want_r, want_e = Q.empty_range(cal.records), Q.empty_error(cal.records)
    for x, refs in zip(xs, sets):
        buf.copy_(_dev(x))
        for dst, src in zip(rbuf, refs):
            dst.copy_(src)
        replay_r()
        replay_e()
        host = [r.cpu().numpy() for r in refs]
        want_r = Q.combine_range(want_r, Q.reference_range(host, x))
        want_e = Q.combine_error(want_e, Q.reference_error(host, x, qb))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(cal.range_store(), want_r)
    np.testing.assert_array_equal(cal.error_store(), want_e)
    # three observed batches give the same stores
    cal.reset()
    for x, refs in zip(xs, sets):
        cal.observe(_dev(x), refs)
        cal.observe_error(_dev(x), refs)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(cal.range_store(), want_r)
    np.testing.assert_array_equal(cal.error_store(), want_e)


def test_two_streams_into_one_store():
    torch = _torch()
    t, q, model, x1 = case_inputs("fire_float", 3)
    x1 = x1.astype(np.float32)
    x2 = synth.synth_images(t, 3, 7).astype(np.float32)
    cal = Q.DeviceCalibrator(t, x1.shape[1:], DEV)
    other = Q.DeviceCalibrator(t, x1.shape[1:], DEV, range_store=cal.range_dev, error_store=cal.error_dev)
    d1, d2 = _dev(x1), _dev(x2)
    r1, r2 = F.float_refs(t, model, d1, device=DEV), F.float_refs(t, model, d2, device=DEV)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s1):
        cal.observe(d1, r1)
        cal.observe_error(d1, r1)
    with torch.cuda.stream(s2):
        other.observe(d2, r2)
        other.observe_error(d2, r2)
    torch.cuda.synchronize()
    h1, h2 = [r.cpu().numpy() for r in r1], [r.cpu().numpy() for r in r2]
    np.testing.assert_array_equal(cal.range_store(), Q.combine_range(Q.reference_range(h1, x1), Q.reference_range(h2, x2)))
    np.testing.assert_array_equal(cal.error_store(), Q.combine_error(Q.reference_error(h1, x1, cal.qb), Q.reference_error(h2, x2, cal.qb)))


# ---- 4. refusals on real buffers ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_stream_usable():
    torch = _torch()
    b = Bare([(3, 49), (5, 1)], 2, seed=5)
    L, s = _lib.lib(), torch.cuda.current_stream(DEV).cuda_stream
    p = b.ptrs()
    rng = lambda batch=2, store=b.rng.data_ptr(), size=b.rng.numel() * 8, maps=p: L.tf2_caq_range(b.desc, maps, 2, batch, store, size, s)
    err = lambda batch=2, sc=b.scales.data_ptr(), size=b.err.numel() * 8: L.tf2_caq_error(b.desc, p, 2, batch, sc, b.err.data_ptr(), size, s)
    assert rng(batch=0) == -1 and rng(store=None) == -1 and rng(maps=None) == -1
    assert rng(size=b.rng.numel() * 8 - 8) == -3 and "store too small" in L.tf2_last_error().decode()
    assert err(batch=-1) == -1 and err(sc=None) == -1 and err(size=8) == -3
    torch.cuda.synchronize()
    assert not b.rng.any().item() and not b.err.any().item()                              # nothing was enqueued
    got_r, got_e = b.run()
    want_r, want_e = b.statement()
    np.testing.assert_array_equal(got_r, want_r)
    np.testing.assert_array_equal(got_e, want_e)
    assert L.tf2_caq_store_init(b.rng.data_ptr(), b.rng.numel() * 8, s) == 0
    torch.cuda.synchronize()
    assert not b.rng.any().item()


# ---- 5. the rules end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["max", ("clip", 1, 1000), "mse"])
def test_calibrate_returns_a_loadable_q_file(monkeypatch, rule):
    t, q, model, _ = case_inputs("tiny_benign", 3)
    batches = [synth.synth_images(t, 3, s).astype(np.float32) for s in (1, 2)]
    seen = []
    real = F.float_refs

    def recording(*a, **k):
        refs = real(*a, **k)
        seen.append([r.cpu().numpy() for r in refs])           # host copies of the very maps the passes read
        return refs

    monkeypatch.setattr(F, "float_refs", recording)
    text = Q.calibrate(t, model, batches, rule=rule, device=DEV)
    monkeypatch.undo()
    assert len(seen) == (4 if rule == "mse" else 2)
    store = Q.combine_range(Q.reference_range(seen[0], batches[0]), Q.reference_range(seen[1], batches[1]))
    plan = cfg.build_plan(t)
    if rule == "max":
        want = Q.q_max(store)
    elif rule == "mse":
        qb = np.clip(Q.q_max(store), -64, 64)
        want = Q.q_mse(Q.combine_error(Q.reference_error(seen[2], batches[0], qb), Q.reference_error(seen[3], batches[1], qb)), qb)
        assert (want >= qb).all()
    else:
        want = Q.q_clip(store, 1, 1000)
        assert (want >= Q.q_max(store)).all()
    assert text == Q.q_file_text(t, Q.q_rows(plan, want))
    net = network.NetWork(t)
    net.Quantization(text.encode())                              # the engine's own parser accepts it
    assert net.q_values_read == len(text.split()) == cfg.q_value_count(t)


# ---- 6. ResNet-50: C up to 2048, HW = 1, 49, 196, 784, 3136, 12544 and the 224 x 224 input, pass 1 ---------------------------------------
def test_resnet50_batch2(golden_dir):
    t = cfg.resnet50_tables()
    q = np.loadtxt(os.path.join(golden_dir, "resnet50_Q"), dtype=np.int32)
    model = synth.synth_model(t, q, 0)
    x = synth.synth_images(t, 2, 0)
    cal, got, _ = check_program(t, model, x, error=False)
    assert max(r["C"] for r in cal.rows) == 2048 and {1, 49, 196, 784, 3136} <= {r["HW"] for r in cal.rows[1:]}
    assert cal.rows[0]["HW"] == 224 * 224
