"""DNS channel pruning, the host side (tf2_amd/dnscp.py): the numpy statement against the reference's own recorded masks and clipped
tensors (tests/golden/ref_dnscp.npz, tools/gen_dnscp_golden.py), the thresholds, the table rule, the shipped pruned ResNet-50, the
export's lengths, the oracle on the masked and on the compacted network, and every refusal of the C ABI (no device)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import netref
from tf2_amd import _lib, config as cfg, dnscp, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "ref_dnscp.npz"))


def _cases(z):
    return [f"c{c:02d}_" for c in range(int(z["n_cases"]))]


def test_statement_equals_the_reference_masks(z):
    """Every case, both iterations: the keep bytes EQUAL the reference's mask.  The fixture keeps every channel mean a relative 2^-10
    clear of both thresholds (asserted), so the order of the reference's float32 sums decides nothing."""
    assert len(_cases(z)) == 8
    seen = np.zeros(7, bool)
    for t in _cases(z):
        assert float(z[t + "margin"]) >= 2.0 ** -10, t
        _, rec = dnscp.reference_stats(z[t + "s0_w"])
        t_lo, t_hi = dnscp.thresholds(rec)
        keep = None
        for it in (0, 1):
            w = z[t + f"s{it}_w"]
            keep, out, S1, r = dnscp.reference_step(w, keep, t_lo, t_hi)
            np.testing.assert_array_equal(keep, z[t + f"s{it}_keep"], err_msg=f"{t} iteration {it}")
            kept = (keep != 0)[None, :, None, None]
            np.testing.assert_array_equal(out.view(np.uint32), np.where(kept, w.view(np.uint32), 0))     # +0.0 where the reference leaves -0.0
            assert (out == w * kept).all()                                                              # the same values
            nzc = int(r["kept_before"] - r["pruned"] + r["revived"])
            seen |= [r["pruned"] > 0 and it == 1, r["revived"] > 0, r["fixup"] > 0, r["fixup"] < 0, nzc == 40 and r["kept_after"] == 32,
                     nzc < 8 and r["kept_after"] == min(16, w.shape[1]), r["status"] == dnscp.NAN_THRESHOLD]
    assert seen.all(), seen


def _pair_tables(Cc, N, k):
    """a conv image -> Cc channels with BN, and the conv [N, Cc, k, k] with a bias that reads it: the smallest prunable pair"""
    b = cfg._B("pair", image=(5, 8, 8), first_filter=k)
    b.conv(-1, 5, 8, 8, Cc, k, 1, k // 2, bn=1)
    b.conv(0, Cc, 8, 8, N, k, 1, k // 2, bn=0, bias=1)
    return b.tables()


def test_compacted_tensors_equal_the_reference_clips(z):
    for t in _cases(z):
        w = z[t + "s1_w"]
        N, Cc, k, _ = w.shape
        tab = _pair_tables(Cc, N, k)
        assert dnscp.prunable_rows(tab) == [1]
        pv, bias = z[t + "pv"], np.arange(N, dtype=np.float32)
        model = np.concatenate([z[t + "pw"].ravel(), pv, pv + 1, [0.5], pv + 2, pv + 3, w.ravel(), bias]).astype(np.float32)
        keeps = {1: z[t + "s1_keep"]}
        np.testing.assert_array_equal(np.flatnonzero(keeps[1]), z[t + "idx"])
        got = dnscp.reference_compact(tab, keeps, model)
        kv = z[t + "pv_kept"]
        want = np.concatenate([z[t + "pw_kept"].ravel(), kv, (pv + 1)[z[t + "idx"]], [0.5], (pv + 2)[z[t + "idx"]], (pv + 3)[z[t + "idx"]],
                               z[t + "w_kept"].ravel(), bias]).astype(np.float32)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=t)
        t2 = dnscp.pruned_tables(tab, keeps)
        assert got.size == cfg.model_float_count(t2) and t2["kInputChannels"][1] == t2["kOutputChannels"][0] == t2["kNEnd"][0] == kv.size


def test_thresholds_against_the_recorded_moments(z):
    """mu and std of thresholds() against the reference's cal_mean_std.  The reference sums float32 (up to 4 032 terms here) and forms
    the variance as a difference of two float32 numbers of which 60 .. 85 % cancels; this side is exact up to four double roundings.
    Measured on the fixture: mu within 8.5e-8 (1.4 float32 ulp), std within 5.6e-7.  The bounds are those of the float32 side: 2^-21
    (4 ulp) for a float32 sum and quotient, and eight times that for std, whose cancellation and square root pass up to (mu^2 + var) /
    (2 var) < 4 times the relative error of both sums on."""
    worst = [0.0, 0.0]
    for t in _cases(z):
        _, rec = dnscp.reference_stats(z[t + "s0_w"])
        t_lo, t_hi, mu, std = dnscp.thresholds(rec, with_moments=True)
        worst[0] = max(worst[0], abs(mu / float(z[t + "mu"]) - 1.0))
        if np.isnan(z[t + "std"]):
            assert np.isnan(std) and np.isnan(t_lo) and np.isnan(t_hi), t           # negative variance; max(NaN, 0) stays NaN
            continue
        worst[1] = max(worst[1], abs(std / float(z[t + "std"]) - 1.0))
        T = max(mu + 0.1 * std, 0.0)
        assert (t_lo, t_hi) == (0.95 * T, 1.05 * T)
    print("worst relative difference: mu %.3g, std %.3g" % tuple(worst))
    assert worst[0] <= 2.0 ** -21 and worst[1] <= 2.0 ** -18, worst
    # other parameters, arrays of records, nothing kept that is non-zero
    recs = np.asarray([dnscp.reference_stats(z[t + "s0_w"])[1] for t in _cases(z)], dnscp.STATE_DTYPE)
    a = dnscp.thresholds(recs, c_rate=0.0, alpha_low=1.0, alpha_high=2.0, with_moments=True)
    ok = ~np.isnan(a[3])
    np.testing.assert_array_equal(a[0][ok], a[2][ok])
    np.testing.assert_array_equal(a[1][ok], 2.0 * a[2][ok])
    _, rec = dnscp.reference_stats(np.zeros((2, 16, 1, 1), np.float32))
    assert int(rec["status"]) == dnscp.ALL_ZERO and int(rec["E"]) == dnscp.NO_EXP and np.isnan(dnscp.thresholds(rec)[0])


def test_fixed_point_is_a_floor_of_the_scaled_magnitude():
    rng = np.random.default_rng(0)
    bits = np.concatenate([rng.integers(0, 0x7f800000, 4000), [0, 1, 2, 0x7fffff, 0x800000, 0x7f7fffff, 0x7f800000, 0x7fc00000]]).astype(np.uint32)
    a = bits.view(np.float32).astype(np.float64)
    for E in (127, 0, -126, -149, int(dnscp.exp2_of_bits(0x3f000000))):
        fits = (bits < 0x7f800000) & (dnscp.exp2_of_bits(bits) <= E)
        m = dnscp.fixed_of_bits(bits, E)
        want = np.floor(np.ldexp(a[fits], 31 - E))                                  # exact in double: 24 significant bits
        np.testing.assert_array_equal(m[fits], want.astype(np.int64))
        assert (m[fits] < 1 << 32).all() and (m[bits >= 0x7f800000] == 0).all()


def _resnet50_rows():
    want, idx = [], 1
    for nblk in (3, 4, 6, 3):
        for blk in range(nblk):
            idx += blk == 0                                                          # the shortcut row of a stage's first block
            want += [idx + 1, idx + 2]                                               # the 3x3 and the expand row of the bottleneck
            idx += 3
    return want


def test_prunable_rows_of_the_table_programs():
    assert dnscp.prunable_rows(cfg.resnet50_tables()) == _resnet50_rows() and len(_resnet50_rows()) == 32
    assert dnscp.prunable_rows(cfg.tiny_tables(widths=(48, 64))) == [3, 4, 6, 7]
    assert dnscp.prunable_rows(cfg.vgg16_tables()) == list(range(1, 16))             # a chain: every row but the first
    assert dnscp.prunable_rows(cfg.squeezenet11_tables()) == [1, 26]                 # squeeze rows feed two expands, expands a concat
    ssd = cfg.ssd300_tables()
    rows = dnscp.prunable_rows(ssd)
    assert rows == [1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 14, 15, 16, 18, 20, 22, 24]
    plan = cfg.build_plan(ssd)
    for l in rows:                                                                  # the rule itself, row by row
        p = plan[l].src
        readers = [L.index for L in plan if p in (L.src, L.add_src)]
        assert readers == [l] and not plan[p].ipool and not plan[l].ipool and plan[p].concat < 0 and plan[p].add_src < 0
    for L in plan:                                                                  # sources with a head or an L2Norm row on them are left out
        if L.index not in rows and L.src >= 0 and not L.ipool and not plan[L.src].ipool and plan[L.src].concat < 0:
            assert len([M.index for M in plan if L.src in (M.src, M.add_src)]) > 1 or plan[L.src].add_src >= 0


def test_shipped_pruned_resnet50_is_what_pruned_tables_makes():
    full = cfg.NetTables(json.load(open(os.path.join(GOLDEN, "tables_resnet50.json"))))
    ship = cfg.NetTables(json.load(open(os.path.join(GOLDEN, "tables_resnet50_pruned.json"))))
    base = cfg.resnet50_tables()
    rows = [l for l in range(54) if full["kInputChannels"][l] != ship["kInputChannels"][l]]
    assert len(rows) == 31 and set(rows) <= set(dnscp.prunable_rows(base))
    assert all(ship["kInputChannels"][l] % 16 == 0 and 0 < ship["kInputChannels"][l] < full["kInputChannels"][l] for l in rows)
    keeps = {l: np.arange(full["kInputChannels"][l]) < ship["kInputChannels"][l] for l in rows}
    got = dnscp.pruned_tables(base, keeps)
    for k in ("kInputChannels", "kOutputChannels", "kNEnd"):
        assert got[k] == ship[k], k
    assert all(got[k] == base[k] for k in base if k not in ("kInputChannels", "kOutputChannels", "kNEnd"))
    # lengths of the export: the shipped Q file has exactly pruned_q's length, the stream model_float_count's
    q_full = np.loadtxt(os.path.join(GOLDEN, "resnet50_Q"), dtype=np.int32)
    q_ship = np.loadtxt(os.path.join(GOLDEN, "resnet50_pruned_Q"), dtype=np.int32)
    q2 = dnscp.pruned_q(base, keeps, q_full)
    assert q2.size == cfg.q_value_count(got) == q_ship.size
    segs, idx, n_dst = dnscp.compact_segments(dnscp.compact_plan(base, keeps))
    assert n_dst == cfg.model_float_count(got) < cfg.model_float_count(base) and idx.size == 6 * sum(int(k.sum()) for k in keeps.values())   # filter, mean, var, gamma, beta in front; the filter itself
    p, m = dnscp.kept_ratio(base, keeps)
    assert 0.3 < p < 0.6 and 0.3 < m < 0.6
    with pytest.raises(ValueError):
        dnscp.pruned_tables(base, {2: np.ones(64)})                                 # row 2 reads the stem beside the shortcut
    with pytest.raises(ValueError):
        dnscp.pruned_tables(base, {3: np.zeros(64)})                                # nothing kept


def _tiny_pruned(seed=8):
    t = cfg.tiny_tables(widths=(48, 64))
    q = synth.synth_q_values(t, 5, spread=2)
    model = synth.synth_model(t, q, 5).copy()
    rng = np.random.default_rng(seed)
    rows = dnscp.prunable_rows(t)
    lay = dnscp._filter_layout(t)
    for l in rows:
        o, N, Cc, kk = lay[l]
        model[o:o + N * Cc * kk].reshape(N, Cc, kk)[:, np.sort(rng.permutation(Cc)[:16]), :] *= np.float32(2.0 ** -6)
    th = {l: dnscp.thresholds(dnscp.reference_stats(model[lay[l][0]:lay[l][0] + lay[l][1] * lay[l][2] * lay[l][3]].reshape(lay[l][1:]))[1]) for l in rows}
    masked, keeps, _, recs = dnscp.reference_model_step(t, model, None, th)
    return t, q, model, masked, keeps, recs


def test_oracle_on_masked_and_compacted_network_agrees():
    t, q, model, masked, keeps, recs = _tiny_pruned()
    assert [int(k.sum()) for k in keeps.values()] == [32, 32, 32, 32] and not recs["status"].any()
    assert (masked != model).any()
    t2 = dnscp.pruned_tables(t, keeps)
    stream, q2 = dnscp.reference_compact(t, keeps, masked), dnscp.pruned_q(t, keeps, q)
    assert stream.size == cfg.model_float_count(t2) and q2.size == cfg.q_value_count(t2)
    np.testing.assert_array_equal(stream, dnscp.reference_compact(t, keeps, model))      # the export drops exactly what the mask zeroed
    x = synth.synth_images(t, 3, 5)
    a, b = netref.RefNet(t, q, masked), netref.RefNet(t2, q2, stream)
    la, lb = a.logits(a.run(x)), b.logits(b.run(x))
    np.testing.assert_array_equal(la, lb)
    full = netref.RefNet(t, q, model)
    assert (full.logits(full.run(x)) != la).any()                                   # the pruned channels did carry something
    assert "conv MACs kept" in dnscp.report(t, keeps, recs)
    # a second step with only some rows updated: the others keep their bytes
    _, k2, _, r2 = dnscp.reference_model_step(t, model, keeps, {l: (0.0, 0.0) for l in keeps}, update=[4])
    assert all((k2[l] == keeps[l]).all() for l in (3, 6, 7)) and int(r2["revived"][1]) == 16 and int(r2["kept_after"][1]) == 48


def _conv(o=0, N=4, Cc=16, kk=9, flags=1, ko=0, t_lo=0.1, t_hi=0.2):
    return _lib.DnscpConv(o, N, Cc, kk, flags, ko, t_lo, t_hi)


def _step(fn="step", dense=0x10000, out=0x20000, n_total=4096, convs=(None,), n_convs=None, keep=0x30000, n_channels=64, sums=0x40000,
          state=0x50000):
    L = _lib.lib()
    convs = [_conv() if c is None else c for c in convs] if convs is not None else None
    table = (_lib.DnscpConv * len(convs))(*convs) if convs else None
    n = len(convs) if n_convs is None and convs is not None else (n_convs or 0)
    if fn == "stats":
        return L.tf2_dnscp_stats(dense, n_total, table, n, keep, n_channels, sums, state, None, 0, None)
    return L.tf2_dnscp_step(dense, out, n_total, table, n, keep, n_channels, sums, state, None, 0, None)


def _compact(src=0x10000, n_src=4096, dst=0x80000, n_dst=4096, segs=((0, 0, 4, 16, 4, 8, 9, 0, -1, 0),), n_segs=None, idx=0x90000, n_idx=8):
    L = _lib.lib()
    table = (_lib.DnscpSeg * len(segs))(*[_lib.DnscpSeg(*s) for s in segs]) if segs is not None else None
    return L.tf2_dnscp_compact(src, n_src, dst, n_dst, table, len(segs) if n_segs is None and segs is not None else (n_segs or 0), idx, n_idx, None)


def test_abi_refusals_need_no_device():
    """Every refusal comes before anything is enqueued: the pointers here are numbers, and no device is touched."""
    L = _lib.lib()
    ARG, UNSUPPORTED = -1, -5
    assert L.tf2_dnscp_state_size(3) == 3 * 128 and L.tf2_dnscp_state_size(0) == 0 and L.tf2_dnscp_scratch_size(3) == 0
    assert dnscp.STATE_DTYPE.itemsize == L.tf2_dnscp_state_size(1)
    assert C.sizeof(_lib.DnscpConv) == 48 and C.sizeof(_lib.DnscpSeg) == 56
    nan = float("nan")
    for kw in (dict(dense=None), dict(out=None), dict(keep=None), dict(sums=None), dict(state=None), dict(convs=None, n_convs=1),
               dict(n_convs=0), dict(n_convs=-1), dict(n_total=0), dict(n_channels=0),
               dict(convs=(_conv(N=0),)), dict(convs=(_conv(Cc=0),)), dict(convs=(_conv(kk=0),)),
               dict(convs=(_conv(o=600, ko=0), _conv(o=0, ko=16))),          # not ascending
               dict(convs=(_conv(o=0), _conv(o=575, ko=16))),                # overlap
               dict(convs=(_conv(o=4096 - 575),)),                           # past n_total
               dict(convs=(_conv(o=-1),)),
               dict(convs=(_conv(), _conv(o=600, ko=15))),                   # keep ranges overlap
               dict(convs=(_conv(ko=49),)),                                  # past n_channels
               dict(convs=(_conv(ko=-1),)),
               dict(convs=(_conv(flags=2),)), dict(convs=(_conv(t_lo=-0.5),)), dict(convs=(_conv(t_hi=-1e-300),)),
               dict(fn="stats", convs=(_conv(flags=1),)),
               dict(out=0x10000 + 4 * 100),                                  # overlaps dense without being it
               dict(state=0x50004), dict(sums=0x40001)):
        assert _step(**kw) == ARG, kw
        assert L.tf2_last_error()
    for kw in (dict(convs=(_conv(Cc=4097, kk=1, N=1),), n_total=1 << 20, n_channels=8192),
               dict(convs=(_conv(N=1 << 20, Cc=1, kk=4),), n_total=1 << 30),
               dict(convs=(_conv(N=1 << 12, Cc=4096, kk=16),), n_total=1 << 30, n_channels=4096)):
        assert _step(**kw) == UNSUPPORTED, kw
    assert b"2^28" in L.tf2_last_error()
    for kw in (dict(src=None), dict(dst=None), dict(segs=None, n_segs=1), dict(n_segs=0), dict(n_src=0), dict(n_dst=0), dict(n_idx=-1),
               dict(segs=((0, 0, 0, 16, 4, 8, 9, 0, -1, 0),)), dict(segs=((0, 0, 4, 16, 4, 8, 0, 0, -1, 0),)),
               dict(segs=((4096 - 575, 0, 4, 16, 4, 8, 9, 0, -1, 0),)),      # the source leaves src
               dict(segs=((0, 4096 - 287, 4, 16, 4, 8, 9, 0, -1, 0),)),      # the destination leaves dst
               dict(segs=((0, 300, 4, 16, 4, 8, 9, 0, -1, 0), (0, 0, 4, 16, 4, 8, 9, 0, -1, 0))),   # destinations not ascending
               dict(segs=((0, 0, 4, 16, 3, 8, 9, 0, -1, 0),)),               # identity between unequal sizes
               dict(segs=((0, 0, 4, 16, 4, 8, 9, 0, -1, 1),)),               # the index list leaves idx
               dict(segs=((0, 0, 4, 16, 4, 8, 9, 0, -1, 0),), idx=None),
               dict(dst=0x10000 + 4 * 1000)):
        assert _compact(**kw) == ARG, kw
        assert L.tf2_last_error()
    # NaN thresholds are no refusal; with every check passed the call would go on to the device, so stop at a refused sibling
    assert _step(convs=(_conv(t_lo=nan, t_hi=nan), _conv(o=10)), n_channels=64) == ARG and b"conv 1" in L.tf2_last_error()
    assert L.tf2_abi_version() == 1
    with pytest.raises(ValueError):
        dnscp.reference_step(np.ones((2, 16, 1, 1), np.float32), None, -1.0, 0.0)
    with pytest.raises(ValueError):
        dnscp.reference_stats(np.ones((1, 4097, 1, 1), np.float32))


def test_kernels_compile_without_scratch():
    import re
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import vmcnt_check
    sizes = list(vmcnt_check.kernel_segments("weight_dnscp")[0].values())
    assert len(sizes) == 7 and all(int(s) == 0 for s in sizes), sizes
