"""INQ weight quantisation, host side (tf2_amd/inq.py, tf2_inq_* of include/tf2_amd.h): the numpy statement against the recorded outputs
of the reference's own ComputeQuantumRange / ShapeIntoTwoPower (tests/golden/ref_inq.npz, tools/gen_inq_golden.py), exp_of against exact
rational arithmetic, the ABI's refusals (no device), engine_check, and the 4-bit file of a quantised stream."""
import ctypes as C
import os
import struct
import sys
from fractions import Fraction

import numpy as np
import pytest

from tf2_amd import _lib, config as cfg, inq, model4bit, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_inq.npz")


def fixture_steps():
    z = np.load(GOLDEN)
    for c in range(int(z["n_cases"])):
        for k in range(int(z[f"c{c:02d}_steps"])):
            p = f"c{c:02d}_s{k}_"
            yield p, {n: z[p + n] for n in ("w_in", "mask_in", "w_out", "mask_out", "par", "exp")}


def test_reference_equals_the_recorded_reference_as_bits():
    n = 0
    for p, s in fixture_steps():
        prev, cur = (float(v) for v in s["par"])
        mx, mn, nv = (int(v) for v in s["exp"])
        r = inq.reference_range(s["w_in"], s["mask_in"], nv)
        assert (r["max_exp"], r["min_exp"]) == (mx, mn), p
        w, m, rec, _ = inq.reference_step(s["w_in"], s["mask_in"], prev, cur, nv)
        np.testing.assert_array_equal(w.view(np.uint32), s["w_out"].view(np.uint32), err_msg=p)
        np.testing.assert_array_equal(m, s["mask_out"], err_msg=p)
        assert (int(rec["max_exp"]), int(rec["min_exp"]), int(rec["status"])) == (mx, mn, 0), p
        assert w.shape == s["w_in"].shape
        n += 1
    assert n >= 40


def test_fixture_holds_what_it_should():
    steps = dict(fixture_steps())
    sizes = {s["w_in"].size for s in steps.values()}
    assert 1 in sizes and 400 in sizes
    # the half-to-even case: n1 = 5, prev = 0.5, cur = 0.75 -> n_init = 10, n_keep = 2
    hits = [(p, s) for p, s in steps.items() if int(s["mask_in"].sum()) == 5 and tuple(s["par"]) == (0.5, 0.75)]
    assert hits
    for p, s in hits:
        _, _, rec, _ = inq.reference_step(s["w_in"], s["mask_in"], 0.5, 0.75)
        assert (int(rec["n_keep"]), int(rec["n_update"])) == (2, 3), p
    # 1.5 * 2^E and both neighbours, E = -20 .. 0
    trip = [s for s in steps.values() if int(s["exp"][2]) == 24]
    assert trip
    mags = set((trip[0]["w_in"].view(np.uint32) & 0x7fffffff).tolist())
    for E in range(-20, 1):
        b = int(np.float32(1.5 * 2.0 ** E).view(np.uint32))
        assert {b - 1, b, b + 1} <= mags, E
    # a tie-heavy tensor: more weights selected than n_update
    more = 0
    for s in steps.values():
        _, m, rec, _ = inq.reference_step(s["w_in"], s["mask_in"], *(float(v) for v in s["par"]), int(s["exp"][2]))
        more += int(s["mask_in"].sum() - m.sum()) > int(rec["n_update"])
    assert more


def _floor_log2(x: Fraction) -> int:
    e = x.numerator.bit_length() - x.denominator.bit_length()
    while Fraction(2) ** e > x:
        e -= 1
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    return e


def test_exp_of_is_floor_log2_of_four_thirds_a_exactly():
    ms = (0, 1, 0x3fffff, 0x400000, 0x400001, 0x7fffff)
    pats, want = [], []
    for E in range(0, 255):
        for m in ms + ((2, 3, 5, 6, 7, 0x300000, 0x5fffff, 0x600000) if E == 0 else ()):
            if E == 0 and m == 0:
                continue
            a = Fraction(m, 1 << 23) * Fraction(2) ** -126 if E == 0 else (1 + Fraction(m, 1 << 23)) * Fraction(2) ** (E - 127)
            pats.append((E << 23) | m)
            want.append(_floor_log2(4 * a / 3))
    got = inq.exp_of_bits(np.asarray(pats, np.uint32))
    np.testing.assert_array_equal(got, np.asarray(want))
    assert int(inq.exp_of_bits(np.uint32(0))) == inq.NO_EXP
    np.testing.assert_array_equal(inq.exp_of(np.asarray([1.0, -1.49, 1.5, 0.75, -0.7499], np.float32)), [0, 0, 1, 0, -1])
    # pow2_bits is 2^e for every e a float32 holds, denormals included
    e = np.arange(-149, 128)
    np.testing.assert_array_equal(inq.pow2_bits(e).view(np.float32).astype(np.float64), np.ldexp(1.0, e))


def test_statement_edges():
    f = np.float32
    # a selected +-0 becomes +0.0 with mask 0; thr = 0 selects everything
    w = np.asarray([0.0, -0.0, 0.5, 0.0, -0.0, 0.0, 0.0, 0.25], f)
    out, m, rec, codes = inq.reference_step(w, np.ones(8, np.uint8), 0.0, 0.5)
    assert int(rec["thr"]) == 0 and not m.any() and (out.view(np.uint32)[[0, 1, 3, 4, 5, 6]] == 0).all()
    assert codes.tolist() == [7, 7, 14, 7, 7, 7, 7, 13] and int(rec["hist"][7]) == 6
    # flushed under min_exp and under exp_floor; 2^1 counted as over one
    w = np.asarray([2.0, 2.0 ** -4, 2.0 ** -5, -2.0 ** -6, 2.0 ** -20], f)
    out, m, rec, _ = inq.reference_step(w, np.ones(5, np.uint8), 0.0, 1.0, exp_floor=-4)
    assert out.tolist() == [2.0, 2.0 ** -4, 0.0, 0.0, 0.0] and not np.signbit(out).any()
    assert (int(rec["flushed_min"]), int(rec["flushed_floor"]), int(rec["over_one"]), int(rec["max_exp"]), int(rec["min_exp"])) == (2, 1, 1, 1, -5)
    # status bits leave the tensor untouched
    w = np.asarray([0.5, 4.0, 0.1], f)
    out, m, rec, _ = inq.reference_step(w, np.asarray([0, 1, 1], np.uint8), 0.5, 1.0)
    assert int(rec["status"]) == inq.RANGE_GREW and (out == w).all() and m.tolist() == [0, 1, 1] and int(rec["n_update"]) == 0
    out, m, rec, _ = inq.reference_step(np.zeros(4, f), np.ones(4, np.uint8), 0.0, 1.0)
    assert int(rec["status"]) == inq.ALL_ZERO and int(rec["max_exp"]) == -100 and m.all()
    out, m, rec, _ = inq.reference_step(np.asarray([np.nan, 1.0, np.inf], f), np.ones(3, np.uint8), 0.0, 1.0)
    assert int(rec["status"]) == inq.NONFINITE and int(rec["nonfinite"]) == 2 and m.all()
    out, m, rec, _ = inq.reference_step(np.asarray([0.5, -0.25], f), np.zeros(2, np.uint8), 0.5, 1.0)
    assert int(rec["max_exp"]) == -100 and int(rec["status"]) == 0 and (out == [0.5, -0.25]).all()
    with pytest.raises(ValueError):
        inq.reference_step(w, np.ones(3), 0.5, 0.25)
    with pytest.raises(ValueError):
        inq.reference_step(w, np.ones(3), 1.0, 1.0)


def _step(w=0x1000, mask=0x2000, n_total=100, segs=((0, 10), (20, 30)), n_segs=None, prev=0.0, cur=1.0, n_values=7, exp_floor=-127,
          state=0x3000, scratch=0x4000, scratch_bytes=None):
    """tf2_inq_step with made-up device pointers: every refusal below is made on the host before anything touches them"""
    L = _lib.lib()
    table = (_lib.InqSeg * max(len(segs), 1))(*[_lib.InqSeg(o, c) for o, c in segs]) if segs is not None else None
    n_segs = len(segs) if n_segs is None else n_segs
    if scratch_bytes is None:
        scratch_bytes = L.tf2_inq_scratch_size(max(n_segs, 1))
    return L.tf2_inq_step(w, mask, n_total, table, n_segs, prev, cur, n_values, exp_floor, None, state, scratch, scratch_bytes, None)


def test_abi_refusals_need_no_device():
    L = _lib.lib()
    ARG, SIZE = -1, -3
    assert L.tf2_inq_state_size(3) == 3 * 256 and L.tf2_inq_state_size(0) == 0
    assert L.tf2_inq_scratch_size(3) == 3 * (4 * 256 * 4 + 16) and L.tf2_inq_scratch_size(-1) == 0
    assert inq.STATE_DTYPE.itemsize == L.tf2_inq_state_size(1)
    for kw in (dict(w=None), dict(mask=None), dict(segs=None, n_segs=2), dict(state=None), dict(scratch=None),
               dict(n_segs=0), dict(n_segs=-1),
               dict(segs=((20, 30), (0, 10))),                   # not ascending
               dict(segs=((0, 10), (9, 5))),                     # overlap
               dict(segs=((0, 10), (95, 6))),                    # past n_total
               dict(segs=((0, 10), (20, 0))),                    # empty
               dict(segs=((-1, 10),)),
               dict(prev=-0.1), dict(prev=1.0, cur=1.0), dict(prev=float("nan")),
               dict(prev=0.5, cur=0.25), dict(cur=1.5), dict(cur=float("nan")),
               dict(n_values=0), dict(n_values=16), dict(exp_floor=-151), dict(exp_floor=128),
               dict(state=0x3004), dict(scratch=0x4001)):
        assert _step(**kw) == ARG, kw
        assert L.tf2_last_error()
    assert _step(scratch_bytes=L.tf2_inq_scratch_size(2) - 1) == SIZE
    assert b"tf2_inq_scratch_size" in L.tf2_last_error()
    assert L.tf2_abi_version() == 1


def _tiny_float_stream(seed=3):
    t = cfg.tiny_tables()
    q = synth.synth_q_values(t, 5, spread=2)
    model = synth.synth_model(t, q, 5).copy()
    rng = np.random.default_rng(seed)
    for name, o, n in inq.segments_of(t, ("filter",)):
        model[o:o + n] = np.clip(rng.standard_normal(n) * 0.25, -0.95, 0.95).astype(np.float32)
    return t, q, model


def test_segments_are_filters_and_biases_only():
    t = cfg.ssd300_tables(width_div=8)
    names = [n for n, _, _ in inq.segments_of(t)]
    assert names and all(n.endswith((".filter", ".bias")) for n in names) and any(n.endswith(".bias") for n in names)
    parts = model4bit.split_model(t, np.zeros(cfg.model_float_count(t), np.float32))
    assert any(n.endswith(".l2w") for n, _, _ in parts)
    assert len(names) == sum(n.endswith((".filter", ".bias")) for n, _, _ in parts)
    assert [n for n, _, _ in inq.segments_of(t, ("filter",))] == [n for n, _, f in parts if f]
    segs = inq.segments_of(t)
    assert all(a[1] + a[2] <= b[1] for a, b in zip(segs, segs[1:]))


def test_engine_check_flags_what_get_real_misreads():
    t, q, model = _tiny_float_stream()
    (name, o, n), = inq.segments_of(t, ("filter",))[:1]
    ok = np.asarray([s * 2.0 ** -i for i in range(15) for s in (1, -1)] + [0.0, -0.0], np.float32)
    model[o:o + n] = np.resize(ok, n)
    good = inq.reference_model_step(t, model, None, 0.0, 1.0, exp_floor=-14)[0]
    good[o:o + n] = np.resize(ok, n)
    rows = inq.engine_check(t, good)
    assert [r["name"] for r in rows] == [s[0] for s in inq.segments_of(t, ("filter",))]
    assert all(r["misfit"] == 0 and r["flushed"] == 0 for r in rows), rows
    bad = good.copy()
    bad[o:o + 4] = [2.0 ** -15, 2.0 ** -16, 3 * 2.0 ** -4, 2.0]
    r = inq.engine_check(t, bad)[0]
    assert (r["misfit"], r["flushed"]) == (4, 0) and sorted(v for v, _ in r["examples"]) == sorted([2.0 ** -15, 2.0 ** -16, 3 * 2.0 ** -4, 2.0])
    assert all(abs(read) == 1.0 for _, read in r["examples"])         # the silent failure: each is read as +-1
    bad[o + 4] = -2.0 ** -17                                          # under 1e-5: read as zero
    r = inq.engine_check(t, bad)[0]
    assert (r["misfit"], r["flushed"]) == (5, 1)
    # the float stream itself: nearly every weight is a misfit
    r = inq.engine_check(t, model)
    assert all(x["misfit"] > 0.9 * x["count"] for x in r[1:])


def test_quantised_stream_writes_a_4bit_file_of_codes():
    t, q, model = _tiny_float_stream()
    out, mask, recs, codes = inq.reference_model_step(t, model, None, 0.0, 1.0, exp_floor=-14)
    segs = inq.segments_of(t)
    assert not mask.any() and not recs["status"].any() and len(recs) == len(segs)
    data = model4bit.write_model_4bit(t, out)
    pos = 0
    for (name, arr, is_filter) in model4bit.split_model(t, out):
        min_exp, dtype, N, Cc, H, W = struct.unpack_from("<bbhhhh", data, pos)
        assert dtype == (0 if is_filter else 1), name
        enc = model4bit.encode_tensor(arr, is_filter)
        pos += len(enc)
        if is_filter:
            # the step's own codes are the file's: same window, same nibbles
            i = [s[0] for s in segs].index(name)
            lo, want = model4bit._codes_for(arr)
            o, n = segs[i][1], segs[i][2]
            if lo == int(recs["min_exp"][i]):
                np.testing.assert_array_equal(codes[o:o + n], want)
            np.testing.assert_array_equal(np.bincount(codes[o:o + n], minlength=16), recs["hist"][i])
    assert pos == len(data)
    back = model4bit.read_model_4bit(data)
    np.testing.assert_array_equal(back.view(np.uint32), out.view(np.uint32))
    assert all(r["misfit"] == 0 for r in inq.engine_check(t, out))
    # a two-step schedule with the weights left alone ends in the same place as one step
    a, m, _, _ = inq.reference_model_step(t, model, None, 0.0, 0.5, exp_floor=-14)
    b, m, _, _ = inq.reference_model_step(t, a, m, 0.5, 1.0, exp_floor=-14)
    assert not m.any()
    np.testing.assert_array_equal(b.view(np.uint32), out.view(np.uint32))


def test_kernels_compile_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import vmcnt_check
    sizes = list(vmcnt_check.kernel_segments("weight_inq")[0].values())
    assert len(sizes) == 6 and all(int(s) == 0 for s in sizes), sizes
