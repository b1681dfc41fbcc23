"""CAQ calibration, CPU side: `caq.fit` against the reference's QuantizeForShift (calibrate.quantize_for_shift) over every exponent, the
rules against calibrate.Calibrator fed the very same float maps, mean_clamp against quantize_channels, records counted by hand, the
accumulation rule, the two rules the reference lacks, the host refusals of tf2_caq_*, the header's constants and the scratch-free ISA of
act_caq.hip.  The device is checked in tests/test_gpu_caq.py, which takes its poisoned values from `POISON` below."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tf2_amd import _lib, calibrate, caq as Q, config as cfg, synth
from tests.test_audit import fire_tables

f32 = np.float32
UP, DOWN = f32(np.inf), f32(0)
# the values every hand-counted channel holds: what is no number, both zeros, a denormal, 127 * 2^k with its neighbours, -128 * 2^k, and a
# value whose product passes 2^18 at Qb = 0
POISON = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, 127.0, float(np.nextafter(f32(127), UP)), float(np.nextafter(f32(127), DOWN)),
          -128.0, 3000.0]


def tie(j: int) -> float:
    """(v + 1/2) * 2^-Q at Q = Qb + j, Qb = 0, v = 5: a rounding tie of candidate j"""
    return 5.5 * 2.0 ** -j


def poisoned_channels() -> np.ndarray:
    """[1, 4, 12] float32: channel j holds POISON and the tie of candidate j"""
    return np.array([[POISON + [tie(j)] for j in range(4)]], f32)


def scalar_range(fs):
    """one channel's RANGE record in Python integers, value by value"""
    rec = [0] * 70
    for f in fs:
        f = float(f32(f))
        if not math.isfinite(f):
            rec[1] += 1
            continue
        rec[0] += 1
        if f == 0:
            rec[2] += 1
            continue
        pattern = int(np.array([abs(f)], f32).view(np.uint32)[0])
        if f < 0:
            rec[3] += 1
            rec[5] = max(rec[5], pattern)
        else:
            rec[4] = max(rec[4], pattern)
        q = 200
        while abs(f) * 2.0 ** q > 127:                 # the definition: the largest q with |f| 2^q <= 127 (exact in double)
            q -= 1
        rec[6 + min(max(q, -32), 31) + 32] += 1
    return rec


def scalar_error(fs, qb):
    """one channel's ERROR record in Python integers: the rule of the module's docstring, value by value"""
    rec = [0] * 12
    scale = f32(2.0 ** (qb + 7))
    for f in fs:
        f = f32(f)
        if not math.isfinite(float(f)):
            rec[1] += 1
            continue
        with np.errstate(over="ignore", under="ignore"):
            t = float(f32(f * scale))
        if abs(t) >= 2 ** 18:
            e = -2 ** 18 if t < 0 else 2 ** 18
            rec[2] += 1
        else:
            e = int(round(t))                          # Python rounds half to even
        rec[0] += 1
        rec[3] += e * e
        for j in range(4):
            s = 7 - j
            u = (e + (1 << (s - 1))) >> s
            v = min(max(u, -128), 127)
            rec[4 + j] += u != v
            rec[8 + j] += (e - (v << s)) ** 2
    return rec


# ---- 1. fit is QuantizeForShift --------------------------------------------------------------------------------------------------------
def boundary_sweep() -> np.ndarray:
    """every float32 127 * 2^k and 2^k with both neighbours, over all exponents, and 20,000 random finite non-zero patterns"""
    vals = []
    for k in range(-160, 130):
        for x in (127.0 * 2.0 ** k, 2.0 ** k):
            with np.errstate(over="ignore"):
                v = f32(x)
            if float(v) == x and np.isfinite(v) and v > 0:
                vals += [v, np.nextafter(v, UP), np.nextafter(v, DOWN)]
    rng = np.random.default_rng(0)
    pat = rng.integers(1, 0x7f800000, 20000, dtype=np.int64).astype(np.uint32)
    out = np.concatenate([np.array(vals, f32), pat.view(f32)])
    return out[np.isfinite(out) & (out > 0)]


def test_fit_is_quantize_for_shift_over_every_exponent():
    x = boundary_sweep()
    assert x.size > 21000 and (x < f32(1.2e-38)).any() and (x > f32(1e38)).any()          # denormals and the top exponent are in
    got = Q.fit(x)
    want = np.array([calibrate.quantize_for_shift(np.array([v], np.float64)) for v in x.astype(np.float64)])
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(float(x[i]), int(got[i]), float(want[i])) for i in bad[:10]]   # no exception found: none to document
    # the definition itself, in exact double arithmetic
    with np.errstate(over="ignore"):
        assert (x.astype(np.float64) * 2.0 ** got <= 127).all() and (x.astype(np.float64) * 2.0 ** (got + 1) > 127).all()
    assert Q.fit(-x).tolist() == got.tolist() and Q.fit(np.array([0.0, -0.0, np.nan, np.inf], f32)).tolist() == [0, 0, 0, 0]
    # the kernel's form of a normal value's fit: 133 - ((mag + 0x1ffff) >> 23); a denormal's is at least 132 either way
    mag = x.view(np.uint32).astype(np.int64)
    kern = 133 - ((mag + 0x1ffff) >> 23)
    normal = mag >= 0x800000
    assert (kern[normal] == got[normal]).all() and (kern[~normal] >= 132).all() and (got[~normal] >= 132).all()


def test_fit_on_the_references_own_arrays(golden_dir):
    z = np.load(os.path.join(golden_dir, "ref_caq.npz"))
    x = np.abs(z["fs_x"].astype(f32)).reshape(-1)
    x = x[x > 0]
    want = np.array([calibrate.quantize_for_shift(np.array([v], np.float64)) for v in x.astype(np.float64)])
    assert x.size > 1000 and (Q.fit(x) == want).all()
    # and array by array, against what the reference's function returned: a non-negative array's Q is fit of its peak
    for a, q in zip(np.abs(z["fs_x"]).astype(f32), z["fs_q"]):
        if a.max() > 0 and float(f32(a.max())) == float(np.abs(a).max()):
            assert calibrate.quantize_for_shift(a.astype(np.float64)) == Q.fit(a.max())


# ---- 2. the reference's rule, from the store ---------------------------------------------------------------------------------------------
def _calibrated_both_ways(monkeypatch, t, seeds, batch):
    q = synth.synth_q_values(t, 1)
    model = synth.synth_model(t, q, 1)
    cal = calibrate.Calibrator(t, model, device="cpu")
    store = None
    for s in seeds:
        x = synth.synth_images(t, batch, s, kind="float")
        outs = calibrate.float_forward(t, model, x, "cpu")                    # once: both sides get these very tensors
        monkeypatch.setattr(calibrate, "float_forward", lambda *a, **k: outs)
        cal.observe(x)
        monkeypatch.undo()
        maps = [outs[l].numpy() for l in sorted(k for k in outs if k >= 0)]
        one = Q.reference_range(maps, x)
        store = one if store is None else Q.combine_range(store, one)
    return cal, store


@pytest.mark.parametrize("tables", ["tiny", "fire"])
def test_q_max_rows_are_the_calibrators(monkeypatch, tables):
    t = cfg.tiny_tables() if tables == "tiny" else fire_tables()
    cal, store = _calibrated_both_ways(monkeypatch, t, (1, 2), 3)
    want = cal.q_rows()
    got = Q.q_rows(cal.plan, Q.q_max(store))
    assert sorted(got) == sorted(want) and len(got) > 3
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"row {k}")
    assert Q.q_file_text(t, got) == cal.q_file_text()
    assert any(np.unique(r).size > 1 for r in got.values())                              # not one value everywhere
    rows = Q.rows_of(cal.plan, (3, 1, 1))
    assert store.shape == (3 + sum(L.N for L in cal.plan), 70) == (rows[-1]["first"] + rows[-1]["C"], 70)


def _float_clamp(q):
    """calibrate.quantize_channels behind its per-channel rule"""
    q = np.asarray(q, np.float64)
    m = q.mean()
    q = np.where((q > 0) & (q > m), float(math.floor(m)), q)
    return np.where((q < 0) & (q < m), float(math.ceil(m)), q)


def test_mean_clamp_is_quantize_channels(golden_dir):
    z = np.load(os.path.join(golden_dir, "ref_caq.npz"))
    for i in range(5):
        x = z[f"qc{i}_x"]
        per = [x[c] for c in range(x.shape[0])] if x.ndim == 1 else [x[:, c] for c in range(x.shape[1])]
        q = np.array([calibrate.quantize_for_shift(c) for c in per]).astype(np.int64)
        got = Q.mean_clamp(q)
        np.testing.assert_array_equal(got, calibrate.quantize_channels(x).astype(np.int64))
        np.testing.assert_array_equal(got, z[f"qc{i}_q"].astype(np.int64))
    rng = np.random.default_rng(5)
    under = 0
    for _ in range(20000):
        n = int(rng.integers(1, 40))
        q = rng.integers(-12, 13, n) - int(rng.integers(0, 9)) * int(rng.integers(0, 2))
        under += bool(q.mean() < 0 and (q > 0).any())
        np.testing.assert_array_equal(Q.mean_clamp(q), _float_clamp(q).astype(np.int64))
    assert under > 1000                                                                    # positive entries under a negative mean
    # mean -11/3: 5 -> floor = -4, and the second rule takes that -4 (below the mean) on to ceil = -3
    assert Q.mean_clamp([5, -20, 4]).tolist() == [-3, -3, -3] and Q.mean_clamp([]).size == 0


# ---- 3. records by hand --------------------------------------------------------------------------------------------------------------
def test_records_by_hand():
    x = poisoned_channels()
    assert x.shape == (1, 4, 12) and f32(1e-40) != 0 and float(x[0, 0, 7]) > 127 > float(x[0, 0, 8])
    rng = Q.reference_range([x])
    err = Q.reference_error([x], None, np.zeros(4, np.int64))
    bits = lambda v: int(np.array([v], f32).view(np.uint32)[0])
    # channel 0, counted by hand.  fit: 1e-40 -> bin 63; 127 and its lower neighbour 0, the upper neighbour and -128 -1; 5.5 -> 4
    # (5.5 * 16 = 88); 3000 -> -5 (3000 / 32 = 93.75)
    want = [0] * 70
    want[:6] = [9, 3, 2, 1, bits(3000.0), bits(128.0)]
    for b, n in ((63, 1), (32, 2), (31, 2), (36, 1), (27, 1)):
        want[6 + b] = n
    assert rng[0].tolist() == want
    # Qb = 0: e = 0, 0, 0 (zeros, denormal), 16256 three times (127 and both neighbours round to it), -16384, 704, and 2^18 for 3000
    es = [0, 0, 0, 16256, 16256, 16256, -16384, 704, 2 ** 18]
    d = {0: [0, 0, 0, 0, 0, 0, 0, -64, 2 ** 18 - 127 * 128],              # 704 + 64 = 768 = 6 * 128: the tie goes up, d = -64
         1: [0, 0, 0, 8128, 8128, 8128, -8192, 0, 2 ** 18 - 127 * 64],
         2: [0, 0, 0, 12192, 12192, 12192, -12288, 0, 2 ** 18 - 127 * 32],
         3: [0, 0, 0, 14224, 14224, 14224, -14336, 0, 2 ** 18 - 127 * 16]}
    want = [9, 3, 1, sum(e * e for e in es), 1, 5, 5, 5] + [sum(v * v for v in d[j]) for j in range(4)]
    assert err[0].tolist() == want
    # every channel against the scalar statement; channel j's tie is one of candidate j: it adds (2^(6 - j))^2 there
    for j in range(4):
        assert rng[j].tolist() == scalar_range(x[0, j]) and err[j].tolist() == scalar_error(x[0, j], 0), j
        without = scalar_error(x[0, j, :11], 0)
        assert err[j, 8 + j] - without[8 + j] == (1 << (6 - j)) ** 2 and 704 >> j == int(tie(j) * 128)
    # other base exponents, and the denormal at the largest scale: e = 0
    for qb in (-64, -3, 5, 64):
        got = Q.reference_error([x], None, np.full(4, qb))
        assert got[2].tolist() == scalar_error(x[0, 2], qb), qb
    assert Q.reference_error([np.array([[1e-40, -1e-45]], f32)], None, [64, 64])[:, 3].tolist() == [0, 0]
    np.testing.assert_array_equal(Q.scale_of([-70, 0, 70]), np.array([2.0 ** -57, 128.0, 2.0 ** 71], f32))       # Qb clamps to -64 .. 64


def test_the_budget_of_a_record():
    worst = 2 ** 18 + 2 ** 14                                        # |e| <= 2^18, |v << s| <= 128 * 2^7
    assert Q.E_LIMIT == 2 ** 18 and 128 << Q.FRAC == 2 ** 14 and worst ** 2 < 2 ** 37 and 2 ** 37 * 2 ** 26 <= 2 ** 63
    x = np.array([[[3e38, -3e38, 1e30]]], f32)                       # the worst value at every candidate: clamped and clipped
    e = Q.reference_error([x], None, [64])
    assert e[0, Q.E_REF_CLAMPED] == 3 and (e[0, Q.E_CLIPPED:Q.E_CLIPPED + 4] == 3).all()
    assert e[0, Q.E_SUM_D2] == 2 * (2 ** 18 - 127 * 128) ** 2 + (2 ** 18 - 128 * 128) ** 2 and e[0, Q.E_SUM_D2 + 3] < 3 * worst ** 2


def test_two_batches_combined_equal_their_concatenation():
    rng = np.random.default_rng(7)
    mk = lambda b: [(rng.standard_normal((b, 5, 3, 3)) * 10.0 ** rng.integers(-3, 4, (1, 5, 1, 1))).astype(f32), rng.standard_normal((b, 7)).astype(f32)]
    a, b = mk(2), mk(3)
    a[0][0, 1], b[0][1, 2, 0, 0], a[1][:, 3], b[1][:, 3] = 0.0, np.nan, -np.abs(a[1][:, 3]), -np.abs(b[1][:, 3])
    ia, ib = rng.standard_normal((2, 3, 4, 4)).astype(f32), rng.standard_normal((3, 3, 4, 4)).astype(f32)
    both = [np.concatenate([p, q]) for p, q in zip(a, b)]
    whole = Q.reference_range(both, np.concatenate([ia, ib]))
    np.testing.assert_array_equal(Q.combine_range(Q.reference_range(a, ia), Q.reference_range(b, ib)), whole)
    np.testing.assert_array_equal(Q.combine_range(whole, Q.empty_range(15)), whole)
    assert whole.shape == (15, 70) and whole[3 + 2, Q.NONFINITE] == 1 and whole[3 + 5 + 3, Q.PEAK_POS] == 0 < whole[3 + 5 + 3, Q.PEAK_NEG]
    qb = Q.q_max(whole)
    np.testing.assert_array_equal(Q.combine_error(Q.reference_error(a, ia, qb), Q.reference_error(b, ib, qb)),
                                  Q.reference_error(both, np.concatenate([ia, ib]), qb))
    assert (whole[:, Q.HIST:].sum(1) == whole[:, Q.N] - whole[:, Q.ZEROS]).all()
    # images left out: the rows' records alone
    np.testing.assert_array_equal(Q.reference_range(both), whole[3:])


# ---- 4. the rules the reference lacks ---------------------------------------------------------------------------------------------------
def test_q_mse_and_q_clip_on_an_outlier_and_a_uniform_channel():
    rng = np.random.default_rng(11)
    x = np.zeros((1, 4, 4001), f32)
    x[0, 0] = rng.uniform(0, 100, 4001)                               # uniform up to the rail
    x[0, 1, :4000], x[0, 1, 4000] = rng.uniform(0, 1, 4000), 70.0     # one outlier in 4001
    x[0, 2] = 0.0                                                     # all zeros
    x[0, 3] = np.nan                                                  # nothing finite
    store = Q.reference_range([x])
    qm = Q.q_max(store)
    assert qm.tolist() == [0, 0, 0, 0]
    err = Q.reference_error([x], None, qm)
    got = Q.q_mse(err, qm)
    assert got[0] == 0 and got[1] > 0 and got[2] == 0 and got[3] == 0          # (ties, all zeros: the smaller j)
    assert err[1, Q.E_CLIPPED:Q.E_CLIPPED + 4].tolist() == [0, 1, 1, 1] and err[0, Q.E_CLIPPED] == 0 < err[0, Q.E_CLIPPED + 1]
    np.testing.assert_array_equal(Q.q_clip(store, 0, 1), qm)
    clip = Q.q_clip(store, 1, 1000)                                    # one value in a thousand may clip
    assert clip[0] == 0 and clip[1] == 6 and clip[2] == 0 and clip[3] == 0      # fit(1.0) = 6: everything but the outlier fits
    assert Q.q_clip(store, 1, 1).tolist()[:2] == [31, 31]
    # q_clip(0, 1) is q_max on anything, peaks beyond the histogram's clamp included
    y = (rng.standard_normal((2, 9, 50)) * 10.0 ** rng.integers(-30, 30, (1, 9, 1))).astype(f32)
    y[:, 4] = 1e-30
    s2 = Q.reference_range([y])
    np.testing.assert_array_equal(Q.q_clip(s2, 0, 1), Q.q_max(s2))
    assert Q.q_max(s2)[4] == Q.fit(f32(1e-30)) > 31 and Q.q_max(Q.empty_range(2)).tolist() == [0, 0]


def test_q_rows_skips_pooling_rows_and_pairs_residual_partners():
    t = cfg.tiny_tables()
    plan = cfg.build_plan(t)
    n = 3 + sum(L.N for L in plan)
    q = np.random.default_rng(2).integers(-3, 9, n)
    rows = Q.q_rows(plan, q)
    raw = Q.q_rows(plan, q, clamp=False)
    spans = Q.record_spans(plan, 3)
    pairs = [L for L in plan if L.add_src >= 0 and L.add_src in rows and rows[L.add_src].size == rows[L.index].size]
    assert len(pairs) == 2                       # (1, 4) then (4, 7), in the Calibrator's order: the last pair ends equal, the chain descends
    assert (rows[pairs[-1].index] == rows[pairs[-1].add_src]).all() and (rows[pairs[0].add_src] >= rows[pairs[0].index]).all()
    part = lambda l, f: f(q[spans[l][0]:spans[l][0] + spans[l][1]])
    np.testing.assert_array_equal(rows[7], np.minimum(np.minimum(part(1, Q.mean_clamp), part(4, Q.mean_clamp)), part(7, Q.mean_clamp)))
    np.testing.assert_array_equal(raw[7], np.minimum(np.minimum(part(1, np.array), part(4, np.array)), part(7, np.array)))
    assert all((L.index in rows) == (L.ipool != 1) for L in plan)
    first, c = spans[-1]
    np.testing.assert_array_equal(raw[-1], q[first:first + c])
    np.testing.assert_array_equal(rows[-1], Q.mean_clamp(q[:3]))
    text = Q.q_file_text(t, rows)
    assert len(text.split()) == cfg.q_value_count(t)


# ---- 5. host refusals (no device: a refusal touches none) -----------------------------------------------------------------------------
def test_caq_abi_refusals_and_sizes_without_a_device():
    L = _lib.lib()
    assert L.tf2_caq_range_store_size(3) == 3 * 70 * 8 and L.tf2_caq_error_store_size(3) == 3 * 12 * 8
    assert L.tf2_caq_range_store_size(0) == 0 and L.tf2_caq_error_store_size(-1) == 0
    one = C.c_void_p(256)                                    # never dereferenced

    def call(error=False, rows=((3, 4, 0), (5, 1, 3)), maps="ok", batch=2, store=one, records=8, scales=one, nullrows=False):
        desc = (_lib.CaqRow * len(rows))()
        for d, (c, hw, first) in zip(desc, rows):
            d.C, d.HW, d.first_record = c, hw, first
        ptrs = (C.c_void_p * len(rows))(*([256] * len(rows))) if maps == "ok" else maps
        size = records * (96 if error else 560)
        if error:
            return L.tf2_caq_error(None if nullrows else desc, ptrs, len(rows), batch, scales, store, size, None)
        return L.tf2_caq_range(None if nullrows else desc, ptrs, len(rows), batch, store, size, None)

    for error in (False, True):
        assert call(error, nullrows=True) == -1 and call(error, maps=None) == -1 and call(error, store=None) == -1
        assert call(error, batch=0) == -1 and call(error, batch=-3) == -1 and "batch" in L.tf2_last_error().decode()
        assert call(error, rows=((0, 4, 0),)) == -1 and call(error, rows=((3, 0, 0),)) == -1 and call(error, rows=((3, -1, 0),)) == -1
        assert call(error, rows=((3, 4, -1),)) == -1 and call(error, rows=()) == -1
        assert call(error, rows=((3, 4, 0), (5, 1, 2))) == -1 and "overlap" in L.tf2_last_error().decode()
        assert call(error, rows=((5, 1, 3), (4, 4, 0))) == -1                              # in any order
        assert call(error, records=7) == -3 and "store too small" in L.tf2_last_error().decode()
        assert call(error, rows=((3, 4, 6),)) == -3                                          # a range out of the store
        assert call(error, store=C.c_void_p(260)) == -1
        assert call(error, rows=((1, 1 << 30, 0),), batch=4) == -5
    assert call(True, scales=None) == -1
    assert L.tf2_caq_store_init(None, 560, None) == -1 and L.tf2_caq_store_init(one, 0, None) == -1 and L.tf2_caq_store_init(one, 12, None) == -1


def test_the_headers_constants_are_the_modules():
    here = os.path.dirname(os.path.abspath(_lib.__file__))
    src = open(os.path.join(here, "csrc", "act_caq.h")).read()
    for name, value in (("kCaqRangeSlots", Q.RANGE_SLOTS), ("kCaqErrorSlots", Q.ERROR_SLOTS), ("kCaqBins", Q.BINS), ("kCaqFrac", Q.FRAC),
                        ("kCaqCands", Q.CANDS), ("kCaqSlab", Q.SLAB), ("kCaqGroup", Q.GROUP), ("kCaqRowsPerLaunch", Q.ROWS_PER_LAUNCH)):
        assert re.search(rf"constexpr int {name} = {value};", src), name
    assert re.search(r"constexpr int kCaqELimit = 1 << 18;", src) and Q.E_LIMIT == 1 << 18
    assert Q.RANGE_SLOTS == Q.HIST + Q.BINS and Q.ERROR_SLOTS == Q.E_SUM_D2 + Q.CANDS and Q.E_CLIPPED + Q.CANDS == Q.E_SUM_D2
    assert "d^2 < 2^37" in src and "2^26 values" in src and "e = 0 whether" in src
    pub = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tf2_amd.h")).read()
    for name in _lib.EXPORTED:
        if name.startswith("tf2_caq_"):
            assert re.search(rf"\b{name}\(", pub), name
    assert sum(name.startswith("tf2_caq_") for name in _lib.EXPORTED) == 5
    assert "d^2 < 2^37" in pub and "either flush mode" in pub and C.sizeof(_lib.CaqRow) == 16


def test_act_caq_kernels_compile_without_a_private_segment():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import vmcnt_check
    seg, lds, txt = vmcnt_check.kernel_segments("act_caq")
    assert len(seg) == 2, seg
    for kernel in ("caq_range_kernel", "caq_error_kernel"):
        names = [k for k in seg if kernel in k]
        assert len(names) == 1 and seg[names[0]] == 0, (kernel, seg)
