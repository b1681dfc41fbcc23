"""Activation audit, CPU side: the statement (audit.reference_audit) against values counted by hand, its accumulation rule, q_delta
against the reference's QuantizeForShift (calibrate.quantize_for_shift), apply_delta / q_file_text through NetWork.Quantization, the
regimes the GPU tests run (on the oracle: they must reach the rails, or stay clear of them, for those tests to mean anything), the host
refusals of tf2_audit_* and the scratch-free ISA of act_audit.hip.  The device is checked in tests/test_gpu_audit.py, which takes its
cases from `case_inputs` below."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import netref
from tf2_amd import _lib, audit as A, calibrate, config as cfg, network, synth

FIRE = dict(image_hw=31, conv1=(16, 3, 2, 0, True), fires=((8, 16, False), (8, 16, True)), classes=12, fc_out=8, name="f")


def fire_tables():
    return cfg.fire_net_tables(FIRE["image_hw"], FIRE["conv1"], FIRE["fires"], FIRE["classes"], FIRE["fc_out"], FIRE["name"])


def long_tables(expand=8):
    """69 table rows (70 store rows; 461 records with expand 8): more than ROWS_PER_LAUNCH, so an observer's second launch really
    happens.  expand=16 (813 records) is the form the engine runs: tf2_net_create refuses a concat slice that does not start at a
    multiple of 16 channels, which the second expand of a fire module with expand 8 does; the oracle and the row walk take both."""
    return cfg.fire_net_tables(15, (8, 3, 1, 0, False), ((4, expand, False),) * 22, 6, 4, "long")


def case_inputs(name: str, batch: int):
    """(tables, q values, model stream, images) of a named regime: what the GPU tests run and the oracle statement below audits"""
    if name == "tiny_benign":
        t = cfg.tiny_tables()
        q = synth.synth_q_values(t, 1)
        return t, q, synth.synth_model(t, q, 1), synth.synth_images(t, batch, 1)
    if name == "tiny_saturate":
        t = cfg.tiny_tables()
        q, model = synth.synth_extreme(t, 3, "saturate")
        return t, q, model, synth.synth_extreme_images(t, batch, seed=3)
    if name in ("fire_float", "fire_int8"):
        t = fire_tables()
        q = synth.synth_q_values(t, 1)
        return t, q, synth.synth_model(t, q, 1), synth.synth_images(t, batch, 1, kind="float" if name == "fire_float" else "int8")
    if name == "long":
        t = long_tables(expand=16)
        q = synth.synth_q_values(t, 1)
        return t, q, synth.synth_model(t, q, 1), synth.synth_images(t, batch, 1)
    raise KeyError(name)


def oracle_store(t, q, model, images):
    """reference_audit of the oracle's maps; float images quantised by the statement of the engine's input rule"""
    R = netref.RefNet(t, q, model)
    outs = R.run(images)
    xq = images if images.dtype == np.int8 else A.reference_input_quant(images, int(R.q[0, 0]))
    return A.reference_audit(outs, xq), R


def bit_length(v: int) -> int:
    return int(abs(int(v))).bit_length()


# ---- 1. the statement on hand-made maps ------------------------------------------------------------------------------------------
def test_reference_audit_counts_by_hand():
    # channel 0: the values the record singles out; channel 1: all zero; two images of 2 x 3 pixels
    ch0 = np.array([[-128, 127, 0, 1, -1, 64], [-64, 127, 3, -2, 100, -128]], np.int8)
    x = np.zeros((2, 2, 2, 3), np.int8)
    x[:, 0] = ch0.reshape(2, 2, 3)
    s = A.reference_audit([x])
    assert s.shape == (2, 16) and s.dtype == np.int64
    #        n  neg lo hi  min   max  sum                               sumsq
    want0 = [12, 5, 2, 2, -128, 127, int(ch0.astype(np.int64).sum()), int((ch0.astype(np.int64) ** 2).sum())]
    assert s[0, :8].tolist() == want0
    assert want0[6] == -128 + 127 + 0 + 1 - 1 + 64 - 64 + 127 + 3 - 2 + 100 - 128 and want0[7] == 2 * 16384 + 2 * 16129 + 2 + 2 * 4096 + 9 + 4 + 10000
    # hist by bit length of |v|: 0 -> {0}; 1 -> {1, -1}; 2 -> {3, -2}; 7 -> {127, 127, 64, -64, 100}; the two -128 in none
    assert s[0, 8:].tolist() == [1, 2, 2, 0, 0, 0, 0, 5]
    assert s[0, 8:].sum() == s[0, 0] - s[0, 2]
    assert s[1].tolist() == [12, 0, 0, 0, 0, 0, 0, 0, 12, 0, 0, 0, 0, 0, 0, 0]
    # brute force over random maps, an end-pool row [B][N] among them
    rng = np.random.default_rng(0)
    maps = [rng.integers(-128, 128, (3, 5, 4, 7)).astype(np.int8), rng.integers(-128, 128, (3, 6)).astype(np.int8)]
    s = A.reference_audit(maps, rng.integers(-128, 128, (3, 3, 4, 4)).astype(np.int8))
    assert s.shape == (3 + 5 + 6, 16)
    m = maps[0]
    for c in range(5):
        v = [int(u) for u in m[:, c].ravel()]
        rec = [len(v), sum(u < 0 for u in v), v.count(-128), v.count(127), min(v), max(v), sum(v), sum(u * u for u in v)]
        rec += [sum(1 for u in v if u != -128 and bit_length(u) == b) for b in range(8)]
        assert s[3 + c].tolist() == rec
    assert s[8:, 0].tolist() == [3] * 6 and s[8:, A.SUM].tolist() == maps[1].astype(np.int64).sum(0).tolist()
    assert (s[:, 8:].sum(1) == s[:, 0] - s[:, 2]).all()


def test_two_batches_added_equal_their_concatenation_and_an_unobserved_channel_keeps_its_initial_extremes():
    rng = np.random.default_rng(1)
    a = [rng.integers(-128, 128, (2, 4, 3, 3)).astype(np.int8), rng.integers(-5, 6, (2, 7)).astype(np.int8)]
    b = [rng.integers(-128, 128, (3, 4, 3, 3)).astype(np.int8), rng.integers(-90, 3, (3, 7)).astype(np.int8)]
    both = [np.concatenate([u, v]) for u, v in zip(a, b)]
    np.testing.assert_array_equal(A.combine(A.reference_audit(a), A.reference_audit(b)), A.reference_audit(both))
    e = A.empty_store(11)
    assert (e[:, A.MIN] == 127).all() and (e[:, A.MAX] == -128).all() and e.sum() == 11 * (127 - 128)
    np.testing.assert_array_equal(A.combine(e, A.reference_audit(a)), A.reference_audit(a))
    empty = A.reference_audit([np.zeros((0, 3, 2, 2), np.int8)])
    np.testing.assert_array_equal(empty, A.empty_store(3))
    s = A.summary(empty, A.rows_of([], (3, 2, 2)))[-1]
    assert s["min"].tolist() == [127] * 3 and s["max"].tolist() == [-128] * 3 and A.q_delta(s).tolist() == [0, 0, 0]


# ---- 2. q_delta is the reference's QuantizeForShift on integer data without rail values ----------------------------------------------
def _row_of(channels):
    """summary row of a list of int8 vectors, one a channel"""
    store = np.concatenate([A.channel_records(np.asarray(c, np.int8).reshape(-1, 1)) for c in channels])
    return A.summary(store, [dict(layer=0, C=len(channels), offset=0)])[0]


def test_q_delta_is_quantize_for_shift():
    rng = np.random.default_rng(2)
    chans = []
    for peak in range(1, 127):                              # every peak, on either side and on both
        body = rng.integers(-peak, peak + 1, 40)
        chans += [np.append(body, peak), np.append(body, -peak), np.append(np.abs(body), peak), np.append(-np.abs(body), -peak)]
    for k in range(7):                                      # one-sided negative channels with peak 2^k: -2^k * 2^(7-k) = -128 still fits
        chans.append(-rng.integers(0, (1 << k) + 1, 30))
        chans[-1][0] = -(1 << k)
    chans.append(np.array([-127, 126, 0]))
    for c in chans:
        assert c.min() > -128 and c.max() < 127
    got = A.q_delta(_row_of(chans))
    want = [int(calibrate.quantize_for_shift(c.astype(np.float64))) for c in chans]
    assert got.tolist() == want
    assert got.min() == 0 and got.max() == 7 and A.q_delta(_row_of([[-1, 0]])).tolist() == [7] and A.q_delta(_row_of([[1, 0]])).tolist() == [6]


def test_q_delta_on_rails_and_idle_channels():
    row = _row_of([[127, 1], [-128, 1], [0, 0, 0], [5, -128, 127], [3, -3]])
    assert A.q_delta(row).tolist() == [-1, -1, 0, -1, 5]
    assert row["bits_used"].tolist() == [7, 8, 0, 8, 2] and row["clip_rate"].tolist() == [0.5, 0.5, 0.0, 2 / 3, 0.0]
    assert row["mean"].tolist() == [64.0, -63.5, 0.0, 4 / 3, 0.0] and row["rms"][4] == 3.0


# ---- 3. apply_delta and the Q file ----------------------------------------------------------------------------------------------------
def test_apply_delta_keeps_residual_partners_together_and_writes_a_loadable_q_file():
    t = cfg.tiny_tables()
    plan = cfg.build_plan(t)
    q = synth.synth_q_values(t, 1)
    rows = A.q_rows_of(plan, q)
    assert sorted(rows) == [-1] + [L.index for L in plan if L.ipool != 1]
    rng = np.random.default_rng(3)
    deltas = {l: rng.integers(-1, 3, r.size) for l, r in rows.items()}
    new = A.apply_delta(plan, rows, deltas)
    pairs = [(L.index, L.add_src) for L in plan if L.add_src >= 0]
    assert pairs
    for l, s in pairs:
        np.testing.assert_array_equal(new[l], new[s])
        assert (new[l] <= np.minimum(rows[l] + deltas[l], rows[s] + deltas[s])).all()
    free = [l for l in rows if l >= 0 and not any(l in p for p in pairs)]
    for l in free:
        np.testing.assert_array_equal(new[l], rows[l] + deltas[l])
    assert new[-1].tolist() == (rows[-1] + deltas[-1].min()).tolist()
    text = A.q_file_text(plan, t, new)
    assert len(text.splitlines()) == cfg.q_value_count(t)
    net = network.NetWork(t)
    net.Quantization(text.encode())
    assert net.q_values_read == cfg.q_value_count(t)
    net.LoadModel(synth.synth_model(t, q, 1))
    # no deltas: the file comes back as it went in
    assert A.q_file_text(plan, t, A.apply_delta(plan, rows, {})) == synth.q_text(q).decode()


# ---- 4. the regimes of the GPU tests are not vacuous -----------------------------------------------------------------------------------
def test_the_saturate_regime_reaches_both_rails_and_the_benign_ones_reach_none():
    t, q, model, x = case_inputs("tiny_saturate", 3)
    store, R = oracle_store(t, q, model, x)
    rows = A.rows_of(R.plan, x.shape[1:])
    assert store.shape[0] * 128 == 128 * (3 + sum(L.N for L in R.plan))
    s = A.summary(store, rows)
    for l in s:
        assert s[l]["hi_rail"].sum() > 0, l
    assert s[1]["lo_rail"].sum() > 0 and s[8]["lo_rail"].sum() > 0
    assert sorted({r["C"] for r in rows}) == [3, 10, 16, 32]

    t, q, model, x = case_inputs("tiny_benign", 3)
    store, R = oracle_store(t, q, model, x)
    s = A.summary(store, A.rows_of(R.plan, x.shape[1:]))
    for l in s:
        if l >= 0:
            assert s[l]["lo_rail"].sum() == 0 and s[l]["hi_rail"].sum() == 0, l
            assert (A.q_delta(s[l]) >= 1).any(), l
    # (the float images reach +-150 and Q0 = 2 clips them: the input record says so)
    assert (A.q_delta(s[-1]) == -1).all() and s[-1]["lo_rail"].sum() > 0 and s[-1]["hi_rail"].sum() > 0
    assert "worst" in A.report(s, top=3)

    t, q, model, x = case_inputs("fire_float", 3)
    store, R = oracle_store(t, q, model, x)
    s = A.summary(store, A.rows_of(R.plan, x.shape[1:]))
    assert all(s[l]["lo_rail"].sum() == 0 and s[l]["hi_rail"].sum() == 0 for l in s if l >= 0)
    assert any(L.concat >= 0 and L.n_start > 0 for L in R.plan)


# ---- 5. host refusals (no device: a refusal touches none) ---------------------------------------------------------------------------
def test_audit_abi_refusals_and_sizes_without_a_device():
    L = _lib.lib()
    t = cfg.tiny_tables()
    q = synth.synth_q_values(t, 1)
    net = network.NetWork(t)
    net.Quantization(synth.q_text(q)); net.LoadModel(synth.synth_model(t, q, 1))
    h = C.c_void_p()
    assert L.tf2_audit_create(net._h, C.byref(h)) == -2 and "packed" in L.tf2_last_error().decode()          # TF2_ERR_STATE
    assert L.tf2_audit_create(None, C.byref(h)) == -1 and L.tf2_audit_create(net._h, None) == -1
    net.Pack(0)
    a = A.AuditHandle(net)
    plan = cfg.build_plan(t)
    assert a.store_size == 128 * (3 + sum(P.N for P in plan)) == L.tf2_audit_store_size(a._h)
    assert L.tf2_audit_store_size(None) == 0 and L.tf2_audit_workspace_size(None, 1) == 0
    assert L.tf2_audit_workspace_size(a._h, 0) == 0 and L.tf2_audit_workspace_size(a._h, 3) == net.workspace_size(3, True)
    rows = a.rows()
    want = A.rows_of(plan, (3, 12, 12))
    assert [{k: r[k] for k in ("layer", "C", "H", "W", "offset")} for r in rows] == [{k: r[k] for k in ("layer", "C", "H", "W", "offset")} for r in want]
    assert rows[0]["n_doubled"] == 0 and all(0 <= r["n_doubled"] <= r["C"] for r in rows)
    arr = (_lib.AuditRow * len(rows))()
    n = C.c_int(-7)
    assert L.tf2_audit_describe(a._h, arr, len(rows) - 1, C.byref(n)) == -3 and n.value == len(rows)        # TF2_ERR_SIZE, *n set
    assert L.tf2_audit_describe(a._h, arr, len(rows), None) == -1 and L.tf2_audit_describe(None, arr, len(rows), C.byref(n)) == -1
    # run and store_init refuse before any device call: null pointers, batch, sizes, a net that is not bound
    one = C.c_void_p(256)                                    # never dereferenced
    run = lambda img=one, b=3, ws=one, wsz=1 << 30, lg=one, st=one, ssz=a.store_size: L.tf2_audit_run(a._h, img, 1, b, ws, wsz, lg, st, ssz, None)
    assert run(img=None) == -1 and run(ws=None) == -1 and run(lg=None) == -1 and run(st=None) == -1 and run(b=0) == -1 and run(b=-2) == -1
    assert run() == -2 and "not bound" in L.tf2_last_error().decode()
    assert L.tf2_audit_store_init(a._h, None, a.store_size, None) == -1
    assert L.tf2_audit_store_init(a._h, one, a.store_size - 1, None) == -3


# ---- 6. the rows of a store: one walk (_observe.store_rows) behind the three modules' rows_of ------------------------------------------------
@pytest.mark.parametrize("tables", [cfg.tiny_tables, fire_tables, lambda: cfg.ssd300_tables(width_div=4), long_tables],
                         ids=["tiny", "fire", "ssd300_div4", "long"])
def test_the_three_modules_lay_out_the_same_rows(tables):
    from tf2_amd import caq as Q, fidelity as F
    plan = cfg.build_plan(tables())
    chw = (plan[0].C, plan[0].H, plan[0].W)
    a, f, c = A.rows_of(plan, chw), F.rows_of(plan, chw), Q.rows_of(plan, chw)
    assert len(a) == len(f) == len(c) == len(plan) + 1
    assert [r["layer"] for r in c] == [-1] + [L.index for L in plan] and (c[0]["C"], c[0]["HW"], c[0]["first"]) == (chw[0], chw[1] * chw[2], 0)
    for ra, rf, rc in zip(a, f, c):
        assert ra["layer"] == rf["layer"] == rc["layer"] and ra["C"] == rf["C"] == rc["C"] > 0, (ra, rf, rc)
        assert ra["H"] * ra["W"] == rf["H"] * rf["W"] == rc["HW"] > 0, (ra, rf, rc)
        assert ra["offset"] == rc["first"] * A.SLOTS * 8 and rf["offset"] == rc["first"] * F.SLOTS * 8, (ra, rf, rc)
    for prev, cur in zip(c, c[1:]):
        assert cur["first"] == prev["first"] + prev["C"]                     # a row's channels are contiguous, the rows in order
    records = chw[0] + sum(L.N for L in plan)
    assert c[-1]["first"] + c[-1]["C"] == records                            # the last row ends at the store size
    assert a[-1]["offset"] + a[-1]["C"] * A.SLOTS * 8 == records * A.SLOTS * 8 and f[-1]["offset"] + f[-1]["C"] * F.SLOTS * 8 == records * F.SLOTS * 8
    assert _lib.lib().tf2_caq_range_store_size(records) == records * Q.RANGE_SLOTS * 8
    assert _lib.lib().tf2_caq_error_store_size(records) == records * Q.ERROR_SLOTS * 8
    if tables is long_tables:
        assert len(c) == 70 > max(A.ROWS_PER_LAUNCH, F.ROWS_PER_LAUNCH, Q.ROWS_PER_LAUNCH) and records == 461


def test_the_engine_takes_the_long_program_of_the_gpu_tests():
    """case_inputs("long") on a handle without a device: 70 rows as rows_of lays them out, more than one launch takes"""
    from tf2_amd import fidelity as F
    t, q, model, _ = case_inputs("long", 2)
    net = network.NetWork(t)
    net.Quantization(synth.q_text(q)); net.LoadModel(model); net.Pack(0)
    plan = cfg.build_plan(t)
    for mod, handle in ((A, A.AuditHandle(net)), (F, F.FidelityHandle(net))):
        rows, want = handle.rows(), mod.rows_of(plan, (3, 15, 15))
        assert len(rows) == 70 > mod.ROWS_PER_LAUNCH and handle.store_size == 813 * mod.SLOTS * 8
        assert [(r["layer"], r["C"], r["H"], r["W"], r["offset"]) for r in rows] == [(r["layer"], r["C"], r["H"], r["W"], r["offset"]) for r in want]


def test_the_kernel_constants_are_the_modules():
    src = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "act_audit.h")).read()
    for name, value in (("kAuditSlots", A.SLOTS), ("kAuditSlab", A.SLAB), ("kAuditChans", A.CHANS), ("kAuditImgSlab", A.IMG_SLAB),
                        ("kAuditRowsPerLaunch", A.ROWS_PER_LAUNCH)):
        assert re.search(rf"constexpr int {name} = {value};", src), name
    assert A.SLAB * 16384 < 2 ** 31 and A.IMG_SLAB * 16384 < 2 ** 31         # a block's sumsq counter


def test_act_audit_kernels_compile_without_scratch():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import vmcnt_check
    seg, lds, txt = vmcnt_check.kernel_segments("act_audit")
    assert len(seg) == 3, seg
    for kernel in ("audit_rows_kernel", "audit_image_kernel", "audit_init_kernel"):
        names = [k for k in seg if kernel in k]
        assert len(names) == 1 and seg[names[0]] == 0, (kernel, seg)
    assert "scratch_" not in txt.split("amdhsa.kernels")[0]
    assert "v_dot4" in txt and "v_mfma" not in txt
