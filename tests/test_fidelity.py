"""Layer fidelity, CPU side: the statement (fidelity.reference_compare) against records counted by hand, its accumulation rule,
layer_summary against CompareError.py's formula and against network.Verify on the oracle's maps and calibrate.float_forward, the regimes
the GPU tests run, the host refusals of tf2_fid_*, the header's constants and the scratch-free ISA of act_fidelity.hip.  The device is
checked in tests/test_gpu_fidelity.py, which takes its cases from `oracle_case` below."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from oracle import netref
from tf2_amd import _lib, calibrate, config as cfg, fidelity as F, network, synth
from tests.test_audit import case_inputs

_CASES = {}


def oracle_case(name: str, batch: int):
    """(tables, q values, model, images, RefNet, oracle maps {l: int8 NCHW}, float refs [numpy per row], q_rows {l: Q}) of a regime of
    tests/test_audit.py -- computed once, shared, never changed"""
    key = (name, batch)
    if key not in _CASES:
        t, q, model, x = case_inputs(name, batch)
        R = netref.RefNet(t, q, model)
        maps = R.run(x)
        rq = np.asarray(R.q, np.int64)
        refs = [r.numpy() for r in F.float_refs(t, model, x, device="cpu")]      # (int8 images go in as the floats of their values)
        q_rows = {-1: np.full(x.shape[1], -int(rq[0][0]), np.int64)}
        for L in R.plan:
            q_rows[L.index] = -rq[L.index + 1][:L.N]
        _CASES[key] = (t, q, model, x, R, maps, refs, q_rows)
    return _CASES[key]


def oracle_store(name: str, batch: int):
    t, q, model, x, R, maps, refs, q_rows = oracle_case(name, batch)
    store = F.reference_compare(maps, refs, q_rows, images=x, q0=int(q_rows[-1][0]))
    return store, F.rows_of(R.plan, x.shape[1:])


def scalar_record(vs, fs, q):
    """one channel's record in Python integers: the rule of the issue, value by value"""
    rec = [0] * 18
    scale = np.float32(2.0) ** np.float32(q + 8)
    for v, f in zip(vs, fs):
        f = np.float32(f)
        if not math.isfinite(float(f)):
            rec[1] += 1
            continue
        with np.errstate(over="ignore"):
            t = float(np.float32(f * scale))
        if abs(t) >= 65536:
            e = -65536 if t < 0 else 65536
            rec[2] += 1
        else:
            e = int(round(t))                         # Python rounds half to even
        d = 256 * int(v) - e
        k = min(7, ((abs(d) + 128) >> 8).bit_length())
        rec[0] += 1
        rec[3] = max(rec[3], abs(d))
        rec[4] += d; rec[5] += abs(d); rec[6] += d * d; rec[7] += abs(e); rec[8] += e * e; rec[9] += (256 * int(v)) ** 2
        rec[10 + k] += 1
    return rec


# ---- 1. records by hand ------------------------------------------------------------------------------------------------------------
def test_records_by_hand():
    f32 = np.float32
    # channel 0, Q = 0 (t = 256 f): ties, the clamp's edge, overflow, the values that are no numbers, zeros
    f0 = [0.5 / 256, 1.5 / 256, 2.5 / 256, -0.5 / 256, 65535.5 / 256, 256.0, -256.0, 3e38, -3e38, np.nan, np.inf, -np.inf, -0.0, 1e-40]
    v0 = [0, 0, 0, 0, 127, 127, -128, 127, -128, 5, 5, 5, 0, 0]
    e, fin, big = F.fixed_ref(np.array(f0, f32), 0)
    assert e[:5].tolist() == [0, 2, 2, 0, 65536] and not big[:5].any()                   # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> -0
    assert e[5:9].tolist() == [65536, -65536, 65536, -65536] and big[5:9].all()         # +-65536 and +-inf by overflow: clamped
    assert (~fin[9:12]).all() and e[9:12].tolist() == [0, 0, 0] and not big[9:12].any()
    assert e[12:].tolist() == [0, 0] and fin[12:].all() and np.float32(1e-40) != 0      # -0.0 and a denormal
    # channel 1, Q = 0, v = 0 and e = j: every histogram bin at both of its edges, and the cap (|d| = 98304: bit length 9)
    edges = [0, 127, 128, 383, 384, 895, 896, 1919, 1920, 3967, 3968, 8063, 8064, 16255, 16256, 65535]
    f1 = [j / 256 for j in edges] + [-300.0, 300.0]
    v1 = [0] * len(edges) + [127, -128]
    # channel 2, Q = -3 (t = 32 f); channel 3, Q = 5 (t = 8192 f)
    f2 = [1.0, -7.96875, 1000.0, 2047.99, 2048.0, 0.015625, -0.046875]
    v2 = [0, -1, 125, 127, 127, 0, 0]
    f3 = [0.01, -0.0155, 3.9, 7.99993896484375, 8.0, 0.00006103515625, -2.0]
    v3 = [0, 0, 125, 127, 127, 0, -64]
    n = len(f1)
    pad = lambda a, fill: list(a) + [fill] * (n - len(a))
    f = np.array([pad(f0, np.nan), f1, pad(f2, np.nan), pad(f3, np.nan)], f32).reshape(1, 4, n)
    v = np.array([pad(v0, 0), v1, pad(v2, 0), pad(v3, 0)], np.int8).reshape(1, 4, n)
    q = [0, 0, -3, 5]
    rec = F.channel_records(v, f, q)
    assert rec.shape == (4, 18) and rec.dtype == np.int64
    for c in range(4):
        assert rec[c].tolist() == scalar_record(v[0, c], f[0, c], q[c]), c
    # channel 0 by hand: 11 finite of 14 (+ 4 NaN of the padding), 4 clamped
    assert rec[0, :3].tolist() == [11, 3 + (n - len(f0)), 4]
    d0 = [0, -2, -2, 0, 127 * 256 - 65536, 127 * 256 - 65536, -32768 + 65536, 127 * 256 - 65536, -32768 + 65536, 0, 0]
    assert rec[0, 3] == 33024 and rec[0, 4] == sum(d0) and rec[0, 5] == sum(abs(u) for u in d0) and rec[0, 6] == sum(u * u for u in d0)
    assert rec[0, 7] == 4 + 5 * 65536 and rec[0, 8] == 8 + 5 * 65536 ** 2 and rec[0, 9] == 3 * (127 * 256) ** 2 + 2 * 32768 ** 2
    assert rec[0, 10:].tolist() == [6, 0, 0, 0, 0, 0, 0, 5]
    # channel 1: two values a bin, the last bin with the cap: 16256, 65535 and the two |d| = 127 * 256 + 65536, 32768 + 65536
    assert rec[1, 10:].tolist() == [2, 2, 2, 2, 2, 2, 2, 4] and rec[1, 3] == 98304 and rec[1, 2] == 2 and rec[1, 0] == n
    # Q negative and positive: 2047.99 * 32 = 65535.68 rounds to 65536 unclamped, 2048 * 32 is clamped; 7.99993896484375 * 8192 = 65535.5
    assert rec[2, :3].tolist() == [7, n - 7, 1] and rec[3, :3].tolist() == [7, n - 7, 1]
    e3, _, big3 = F.fixed_ref(np.array(f3, f32), 5)
    assert e3[3] == 65536 and not big3[3] and big3[4] and e3[5] == 0 and e3[6] == -16384        # 0.5 -> 0 (tie to even)
    assert F.scale_of([-64, 64]).tolist() == [2.0 ** -56, 2.0 ** 72]
    # brute force over random maps, an end-pool row [B][N] among them, extreme Q at both ends
    rng = np.random.default_rng(0)
    maps = [rng.integers(-128, 128, (3, 5, 4, 7)).astype(np.int8), rng.integers(-128, 128, (3, 6)).astype(np.int8)]
    qs = [np.array([-64, -2, 0, 3, 64]), rng.integers(-4, 5, 6)]
    refs = [(m.astype(np.float64) + rng.uniform(-3, 3, m.shape)) * 2.0 ** -np.asarray(qq).reshape((1, -1) + (1,) * (m.ndim - 2))
            for m, qq in zip(maps, qs)]
    refs = [r.astype(f32) for r in refs]
    imgs = rng.uniform(-30, 30, (3, 3, 4, 4)).astype(f32)
    s = F.reference_compare(maps, refs, qs, images=imgs, q0=2)
    assert s.shape == (3 + 5 + 6, 18)
    for c in range(5):
        assert s[3 + c].tolist() == scalar_record(maps[0][:, c].ravel(), refs[0][:, c].ravel(), int(qs[0][c]))
    for c in range(6):
        assert s[8 + c].tolist() == scalar_record(maps[1][:, c], refs[1][:, c], int(qs[1][c]))
    from tf2_amd.preprocess import quant_input
    for c in range(3):
        assert s[c].tolist() == scalar_record(quant_input(imgs[:, c], 4.0).ravel(), imgs[:, c].ravel(), 2)
    assert (s[:, 10:].sum(1) == s[:, 0]).all() and (s[:3, F.MAX_ABS_D] <= 128).all()          # the input against itself: half an LSB
    # int8 images: row -1 stays empty; a None reference: that row stays empty
    s2 = F.reference_compare(maps, [None, refs[1]], qs, images=np.zeros((3, 3, 4, 4), np.int8), q0=2)
    assert not s2[:8].any() and (s2[8:] == s[8:]).all()


# ---- 2. combining ----------------------------------------------------------------------------------------------------------------------
def test_two_batches_combined_equal_their_concatenation():
    rng = np.random.default_rng(1)
    qs = [rng.integers(-3, 4, 4), rng.integers(-3, 4, 7)]

    def batch(B, noise):
        maps = [rng.integers(-128, 128, (B, 4, 3, 3)).astype(np.int8), rng.integers(-128, 128, (B, 7)).astype(np.int8)]
        refs = [((m + rng.uniform(-noise, noise, m.shape)) * 2.0 ** -qq.reshape((1, -1) + (1,) * (m.ndim - 2))).astype(np.float32) for m, qq in zip(maps, qs)]
        refs[0][0, 1, 0, 0] = np.nan
        return maps, refs

    (ma, ra), (mb, rb) = batch(2, 0.4), batch(3, 9.0)
    a, b = F.reference_compare(ma, ra, qs), F.reference_compare(mb, rb, qs)
    both = F.reference_compare([np.concatenate(p) for p in zip(ma, mb)], [np.concatenate(p) for p in zip(ra, rb)], qs)
    np.testing.assert_array_equal(F.combine(a, b), both)
    assert (both[:, F.MAX_ABS_D] == np.maximum(a[:, F.MAX_ABS_D], b[:, F.MAX_ABS_D])).all() and (a[:, F.MAX_ABS_D] < b[:, F.MAX_ABS_D]).any()
    assert both[1, F.NONFINITE] == 2
    e = F.empty_store(11)
    assert e.shape == (11, 18) and not e.any()
    np.testing.assert_array_equal(F.combine(e, a), a)
    np.testing.assert_array_equal(F.reference_compare([np.zeros((0, 3, 2, 2), np.int8)], [np.zeros((0, 3, 2, 2), np.float32)], [[0, 0, 0]]), F.empty_store(3))
    # the pinned values of empty and of all-zero channels
    s = F.summary(F.empty_store(3), F.rows_of([], (3, 2, 2)))[-1]
    assert s["rel_l1"].tolist() == [0.0] * 3 and s["cosine"].tolist() == [1.0] * 3 and s["nearest"].tolist() == [1.0] * 3
    assert np.isposinf(s["sqnr_db"]).all() and s["bias_lsb"].tolist() == [0.0] * 3 and s["max_err_lsb"].tolist() == [0.0] * 3
    z = F.channel_records(np.array([[[0, 0]], [[1, -1]]], np.int8).reshape(1, 2, 2), np.zeros((1, 2, 2), np.float32), [0, 0])
    s = F.summary(z, [dict(layer=0, C=2, offset=0)])[0]
    assert s["rel_l1"].tolist() == [0.0, np.inf] and np.isposinf(s["sqnr_db"][0]) and np.isneginf(s["sqnr_db"][1])
    assert s["cosine"].tolist() == [1.0, 0.0] and s["nearest"].tolist() == [1.0, 0.0] and s["max_err_lsb"].tolist() == [0.0, 1.0]


# ---- 3. CompareError's formula and Verify ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tiny_benign", "fire_float"])
def test_layer_rel_l1_is_compare_errors_formula(case):
    """CompareError.py prints 100 * sum|int8 - q float| / sum|q float| per layer.  With N = sum|v - f 2^Q| and D = sum|f 2^Q| in float64
    over the n values of a row (no reference clamped: |f 2^Q| < 256, asserted), every |d| / 256 is within 1/512 of |v - f 2^Q| (e / 256
    is f 2^Q rounded to 1/256: off by at most 1/512) and every |e| / 256 within 1/512 of |f 2^Q|: the statement's numerator lies in
    N -+ n/512, its denominator in D -+ n/512, so with D > n/512
        |rel_l1 - N/D| <= (N + n/512) / (D - n/512) - N/D
    (the upper side is the wider one).  The float64 evaluation of N and D adds at most n 2^-52 relative, covered by a factor 1 + 1e-9."""
    t, q, model, x, R, maps, refs, q_rows = oracle_case(case, 3)
    store, rows = oracle_store(case, 3)
    lay = F.layer_summary(store, rows)
    for L in R.plan:
        l = L.index
        v = maps[l].astype(np.float64).reshape(3, L.N, -1)
        sf = refs[l].astype(np.float64).reshape(3, L.N, -1) * 2.0 ** q_rows[l].astype(np.float64).reshape(1, -1, 1)
        assert np.abs(sf).max() < 256
        n, N, D = v.size, np.abs(v - sf).sum(), np.abs(sf).sum()
        assert D > n / 512, (l, D, n)
        bound = ((N + n / 512) / (D - n / 512) - N / D) * (1 + 1e-9) + 1e-12
        got = float(lay[l]["rel_l1"])
        print(f"{case} row {l}: rel_l1 {got:.6f}, CompareError {N / D:.6f}, |diff| {abs(got - N / D):.3e}, bound {bound:.3e}")
        assert abs(got - N / D) <= bound, (l, got, N / D, bound)
        assert lay[l]["n"] == n and lay[l]["ref_clamped"] == 0 and lay[l]["nonfinite"] == 0


@pytest.mark.parametrize("case", ["tiny_benign", "fire_float"])
def test_last_rows_figure_is_verifys(case):
    """network.Verify (network_helper.cpp:18-141) on one frame: float32 throughout.  Its terms et = f * 2^Q are exact (a power of two),
    |et - v| and |et| carry one rounding each (u = 2^-24), and a float32 sum of n terms in any order is within g = n u / (1 - n u) of
    the exact sum of its (rounded) terms: numerator and denominator are each within G = (1 + u)(1 + g) - 1 of N and D, the division adds
    one rounding, so |Verify - N/D| <= N/D ((1 + G)(1 + u) / (1 - G) - 1).  The statement's figure for the same frame is within
    (N + n/512) / (D - n/512) - N/D of N/D (test_layer_rel_l1_is_compare_errors_formula); the two bounds add."""
    t, q, model, x, R, maps, refs, q_rows = oracle_case(case, 3)
    last = len(R.plan) - 1
    Nc = R.plan[last].N
    u = 2.0 ** -24
    for frame in range(3):
        v = maps[last][frame:frame + 1]
        f = refs[last][frame:frame + 1].reshape(v.shape)
        store = F.reference_compare([v], [f], [q_rows[last]])
        got = float(F.layer_summary(store, [dict(layer=last, C=Nc, offset=0)])[last]["rel_l1"])
        out = np.moveaxis(v.reshape(1, Nc, -1), 1, 2)                         # [1][hw][N]: the engine's output of a frame
        ver = network.Verify(0, f.reshape(Nc, -1).ravel(), np.asarray(R.q), out, num_layer=len(R.plan))
        sf = f.astype(np.float64).reshape(Nc, -1) * 2.0 ** q_rows[last].astype(np.float64).reshape(-1, 1)
        n, N, D = sf.size, np.abs(v.astype(np.float64).reshape(Nc, -1) - sf).sum(), np.abs(sf).sum()
        assert D > n / 512
        g = n * u / (1 - n * u)
        G = (1 + u) * (1 + g) - 1
        bound = ((N + n / 512) / (D - n / 512) - N / D) + N / D * ((1 + G) * (1 + u) / (1 - G) - 1) + 1e-12
        print(f"{case} frame {frame}: rel_l1 {got:.6f}, Verify {ver:.6f}, |diff| {abs(got - ver):.3e}, bound {bound:.3e}")
        assert abs(got - ver) <= bound, (frame, got, ver, bound)


# ---- 4. the regimes of the GPU tests are not vacuous -------------------------------------------------------------------------------------
def test_the_benign_regimes_clamp_nothing_and_the_saturate_regime_clamps_every_row():
    for case in ("tiny_benign", "fire_float"):
        store, rows = oracle_store(case, 3)
        assert store[3:, F.REF_CLAMPED].sum() == 0 and store[:, F.NONFINITE].sum() == 0, case      # (every table row)
        s = F.summary(store, rows)
        assert all((s[l]["n"] == 3 * r["H"] * r["W"]).all() for l, r in zip(sorted(s), rows)), case
        assert "worst" in F.report(s, top=3, layers=F.layer_summary(store, rows)) and "worst" in F.report(s, top=3)
    # (tiny_benign's float images reach +-150 and Q0 = 2 makes +-600 of them: the INPUT's records say so, as the audit's do)
    assert oracle_store("tiny_benign", 3)[0][:3, F.REF_CLAMPED].min() > 0
    store, rows = oracle_store("tiny_saturate", 3)
    lay = F.layer_summary(store, rows)
    for l in lay:
        if l >= 0:
            assert lay[l]["ref_clamped"] >= 0.09 * lay[l]["n"] > 0, (l, lay[l]["ref_clamped"], lay[l]["n"])
    assert sorted({r["C"] for r in rows}) == [3, 10, 16, 32]


# ---- 5. host refusals (no device: a refusal touches none) -----------------------------------------------------------------------------
def test_fid_abi_refusals_and_sizes_without_a_device():
    L = _lib.lib()
    t = cfg.tiny_tables()
    q = synth.synth_q_values(t, 1)
    net = network.NetWork(t)
    net.Quantization(synth.q_text(q)); net.LoadModel(synth.synth_model(t, q, 1))
    h = C.c_void_p()
    assert L.tf2_fid_create(net._h, C.byref(h)) == -2 and "packed" in L.tf2_last_error().decode()          # TF2_ERR_STATE
    assert L.tf2_fid_create(None, C.byref(h)) == -1 and L.tf2_fid_create(net._h, None) == -1
    net.Pack(0)
    a = F.FidelityHandle(net)
    plan = cfg.build_plan(t)
    records = 3 + sum(P.N for P in plan)
    assert a.store_size == 144 * records == L.tf2_fid_store_size(a._h)
    assert L.tf2_fid_store_size(None) == 0 and L.tf2_fid_workspace_size(None, 1) == 0
    assert L.tf2_fid_workspace_size(a._h, 0) == 0 and L.tf2_fid_workspace_size(a._h, 3) == net.workspace_size(3, True)
    rows = a.rows()
    want = F.rows_of(plan, (3, 12, 12))
    keys = ("layer", "C", "H", "W", "offset")
    assert [{k: r[k] for k in keys} for r in rows] == [{k: r[k] for k in keys} for r in want]
    arr = (_lib.AuditRow * len(rows))()
    n = C.c_int(-7)
    assert L.tf2_fid_describe(a._h, arr, len(rows) - 1, C.byref(n)) == -3 and n.value == len(rows)        # TF2_ERR_SIZE, *n set
    assert L.tf2_fid_describe(a._h, arr, len(rows), None) == -1 and L.tf2_fid_describe(None, arr, len(rows), C.byref(n)) == -1
    # the scale table is 2^(Q + 8) of q_rows_of_net, record by record
    qr = F.q_rows_of_net(net)
    want_scales = np.concatenate([F.scale_of(qr[r["layer"]]) for r in rows])
    np.testing.assert_array_equal(a.scales(), want_scales)
    buf = (C.c_float * records)()
    n = C.c_int(-7)
    assert L.tf2_fid_scales(a._h, buf, records - 1, C.byref(n)) == -3 and n.value == records
    assert L.tf2_fid_scales(None, buf, records, C.byref(n)) == -1 and L.tf2_fid_scales(a._h, buf, records, None) == -1
    # run, kept and store_init refuse before any device call: null pointers, batch, sizes, a net that is not bound
    one = C.c_void_p(256)                                    # never dereferenced
    refs = (C.c_void_p * len(plan))()
    big = 1 << 30

    def run(img=one, b=3, ws=one, wsz=big, lg=one, rf=refs, sc=one, st=one, ssz=a.store_size):
        return L.tf2_fid_run(a._h, img, 1, b, ws, wsz, lg, rf, sc, st, ssz, None)

    def kept(img=one, b=3, ws=one, wsz=big, rf=refs, sc=one, st=one, ssz=a.store_size):
        return L.tf2_fid_kept(a._h, img, 1, b, ws, wsz, rf, sc, st, ssz, None)

    assert run(img=None) == -1 and run(ws=None) == -1 and run(lg=None) == -1 and run(st=None) == -1 and run(rf=None) == -1 and run(sc=None) == -1
    assert run(b=0) == -1 and run(b=-2) == -1
    assert kept(img=None) == -1 and kept(ws=None) == -1 and kept(st=None) == -1 and kept(rf=None) == -1 and kept(b=0) == -1
    assert L.tf2_fid_run(None, one, 1, 3, one, big, one, refs, one, one, a.store_size, None) == -1
    assert run() == -2 and "not bound" in L.tf2_last_error().decode()
    assert kept() == -2 and "not bound" in L.tf2_last_error().decode()
    assert L.tf2_fid_store_init(a._h, None, a.store_size, None) == -1
    assert L.tf2_fid_store_init(a._h, one, a.store_size - 1, None) == -3
    assert L.tf2_fid_store_init(None, one, a.store_size, None) == -1
    # a net without its Q table has no scales to compare with
    bare = network.NetWork(t)
    assert L.tf2_fid_create(bare._h, C.byref(h)) == -2


def test_the_headers_constants_are_the_modules():
    src = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "act_fidelity.h")).read()
    for name, value in (("kFidSlots", F.SLOTS), ("kFidFrac", F.FRAC), ("kFidSlab", F.SLAB), ("kFidChans", F.CHANS), ("kFidTile", F.TILE),
                        ("kFidImgSlab", F.IMG_SLAB), ("kFidRowsPerLaunch", F.ROWS_PER_LAUNCH)):
        assert re.search(rf"constexpr int {name} = {value};", src), name
    assert len(F.SLOT_NAMES) == F.SLOTS == F.HIST + 8 and F.E_LIMIT == 256 << F.FRAC
    assert "d^2 < 2^34" in src and (128 * 256 + F.E_LIMIT) ** 2 < 2 ** 34 and 2 ** 34 * 2 ** 29 <= 2 ** 63
    pub = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tf2_amd.h")).read()
    for name in _lib.EXPORTED:
        if name.startswith("tf2_fid_"):
            assert re.search(rf"\b{name}\(", pub), name
    assert sum(name.startswith("tf2_fid_") for name in _lib.EXPORTED) == 9


def test_act_fidelity_kernels_compile_without_scratch():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import vmcnt_check
    seg, lds, txt = vmcnt_check.kernel_segments("act_fidelity")
    assert len(seg) == 2, seg
    for kernel in ("fid_rows_kernel", "fid_image_kernel"):
        names = [k for k in seg if kernel in k]
        assert len(names) == 1 and seg[names[0]] == 0, (kernel, seg)
    assert "scratch_" not in txt.split("amdhsa.kernels")[0]
