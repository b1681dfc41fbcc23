"""Classification head, CPU side: the statement classify.reference against tf2_topk (labels and features, exactly) over the input
families and the (n, k) grid the device is held to, its probabilities against network.Evaluation within a derived bound, the rank
and tally rules, the host refusals of tf2_cls_create / tf2_cls_run (no device: a refusal touches none) and the scratch-free ISA of
classify.hip.  The device itself is checked in tests/test_gpu_classify.py, which takes its inputs from `family` below."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tf2_amd import _lib, classify as K, config as cfg, network, synth
from tf2_amd.network import NetWork

NS = [2, 10, 63, 64, 65, 1000, 1001, 4096]
FAMILIES = ["random", "equal", "two_valued", "extreme_sh0", "extreme_sh30", "mixed_sh"]


def ks_of(n):
    return sorted({1, min(5, n), min(n, 64)})


GRID = [(n, k) for n in NS for k in ks_of(n)]


def family(kind: str, n: int, batch: int, seed: int):
    """(int8 logits [batch, n], runtime Q row int8 [n] = -sh) of one input family; the Q row depends on (kind, n, seed) alone"""
    rng = np.random.default_rng([seed, n, batch, FAMILIES.index(kind)])
    rng_q = np.random.default_rng([seed, n, FAMILIES.index(kind)])
    sh = np.zeros(n, np.int64)
    if kind == "random":                       # every logit value, per-channel sh 0..7
        lg = rng.integers(-128, 128, (batch, n))
        sh = rng_q.integers(0, 8, n)
    elif kind == "equal":                      # the tie rule alone
        lg = np.repeat(rng.integers(-128, 128, (batch, 1)), n, axis=1)
        sh[:] = 4
    elif kind == "two_valued":
        vals = rng.integers(-128, 128, (batch, 2))
        lg = np.take_along_axis(vals, rng.integers(0, 2, (batch, n)), axis=1)
        sh[:] = 2
    elif kind in ("extreme_sh0", "extreme_sh30"):
        lg = np.where(rng.integers(0, 2, (batch, n)) == 1, 127, -128)
        sh[:] = 0 if kind == "extreme_sh0" else 30
    else:                                      # different logits, equal features: v << sh with sh in {0, 3, 6} per channel (64 at 6 == 1 at 0)
        sh = rng_q.choice([0, 3, 6], n)
        lg = rng.integers(-1, 2, (batch, n)) << sh[None, :]
    return lg.astype(np.int8), (-sh).astype(np.int8)


def topk_host(logits, q_last, k):
    """tf2_topk per image: (labels [B, k], features [B, k])"""
    B, n = logits.shape
    labels, feats = np.empty((B, k), np.int32), np.empty((B, k), np.float32)
    for b in range(B):
        row = np.ascontiguousarray(logits[b])
        _lib.check(_lib.lib().tf2_topk(row.ctypes.data, q_last.ctypes.data, n, k, labels[b].ctypes.data, feats[b].ctypes.data))
    return labels, feats


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("n,k", GRID)
def test_reference_equals_topk(kind, n, k):
    lg, q = family(kind, n, 3, seed=1)
    ref = K.reference(lg, q, k)
    labels, feats = topk_host(lg, q, k)
    assert np.array_equal(ref.labels, labels)
    assert np.array_equal(ref.features.view(np.uint32), feats.view(np.uint32))
    if kind == "equal":
        assert (ref.labels == np.arange(n - 1, n - 1 - k, -1)[None, :]).all()
    if kind == "mixed_sh" and n >= 63 and k == 5:
        raw = np.take_along_axis(lg, ref.labels.astype(np.int64), axis=1)
        assert (ref.features == 1.0).all() and len(np.unique(raw)) > 1          # 1, 8 and 64 side by side, ordered by index alone
        assert (np.diff(ref.labels, axis=1) < 0).all()


@pytest.mark.parametrize("n,sh", [(10, 3), (1000, 1), (1000, None), (4096, 2)])
def test_reference_probabilities_against_evaluation(n, sh):
    """Relative difference of the top-5 probabilities at most (n + 4 + 2 max|d|) 2^-24: n for Evaluation's sequential float32 sum of
    n positive terms (the worst case of that order), 4 for its float32 exp, division and rounding, 2 max|d| for the one float32
    rounding of d = f - fmax in numerator and sum (an error of |d| 2^-24 in an exponent is a relative error of that size), which
    Evaluation does not have.  Features stay within +-64 (sh >= 1), so Evaluation's float32 exp neither overflows nor underflows on
    the top five."""
    rng = np.random.default_rng(n)
    lg = rng.integers(-128, 128, (4, n)).astype(np.int8)
    q = (-(rng.integers(1, 8, n) if sh is None else np.full(n, sh))).astype(np.int8)
    ref = K.reference(lg, q, 5)
    f = K.features_of(lg, q)
    assert np.abs(f).max() <= 80
    for b in range(4):
        labels, probs = network.Evaluation(b, q, lg, k=5)
        assert labels == ref.labels[b].tolist()
        bound = (n + 4 + 2 * float(f[b].max() - f[b].min())) * 2.0 ** -24
        rel = np.abs(np.float64(probs) - ref.probs[b]) / ref.probs[b]
        print(f"n={n} sh={sh} image {b}: max relative difference {rel.max():.3e}, bound {bound:.3e}")
        assert rel.max() <= bound
    assert np.allclose(ref.all_probs.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert np.array_equal(np.take_along_axis(ref.all_probs, ref.labels.astype(np.int64), axis=1), ref.probs)


def test_probabilities_stay_finite_where_evaluation_overflows():
    lg = np.array([[127, 100, -128, 127]], np.int8)
    q = np.zeros(4, np.int8)                                   # features up to 127: exp overflows float32
    _, probs = network.Evaluation(0, q, lg, k=2)
    assert not np.isfinite(probs).all()
    ref = K.reference(lg, q, 2)
    assert ref.labels.tolist() == [[3, 0]] and np.allclose(ref.probs, 0.5)


def test_rank_and_tally_rules():
    n, k = 12, 5
    lg = np.tile(np.arange(n, dtype=np.int8) * 3, (k + 5, 1))          # label i has feature 3 i: the top five are 11, 10, 9, 8, 7
    q = np.zeros(n, np.int8)
    truth = np.array([11, 10, 9, 8, 7, 6, -1, n, 1 << 20, 0], np.int32)  # every position, absent, unlabelled, bad, bad, absent
    ref = K.reference(lg, q, k, truth)
    assert ref.labels[0].tolist() == [11, 10, 9, 8, 7]
    assert ref.rank.tolist() == [0, 1, 2, 3, 4, -1, -1, -1, -1, -1]
    assert ref.tally.tolist() == [9, 1, 5, 2]                           # nine labelled (two of them bad), one top-1, five top-5
    none = K.reference(lg, q, k, np.full(k + 5, -1, np.int32))
    assert none.tally.tolist() == [0, 0, 0, 0] and (none.rank == -1).all()
    assert K.reference(lg, q, k).rank is None
    # a tie at the boundary: the label of the smaller index loses
    tie = np.zeros((1, 8), np.int8)
    assert K.reference(tie, np.zeros(8, np.int8), 3, np.int32([4])).rank.tolist() == [-1]
    assert K.reference(tie, np.zeros(8, np.int8), 3, np.int32([5])).rank.tolist() == [2]
    with pytest.raises(ValueError):
        K.reference(tie, np.zeros(8, np.int8), 9)
    with pytest.raises(ValueError):
        K.reference(tie, np.ones(8, np.int8), 3)                       # sh = -1


FAKE = 0x7f0000001000      # never dereferenced: every case is refused before a device call


def _net(tables, q_set=True, edit=None):
    net = NetWork(tables)
    if q_set:
        q = net.Quantization(synth.q_text(synth.synth_q_values(tables, 1)))
        q[net.num_layer] = np.minimum(q[net.num_layer], 0)               # a legal last row whatever the seed gave
        if edit:
            edit(q[net.num_layer])
        _lib.check(_lib.lib().tf2_net_set_q(net._h, q.ctypes.data, q.size))
    return net


def _create(net, top_k=5, size=None, desc=True):
    d = _lib.ClsDesc(C.sizeof(_lib.ClsDesc) if size is None else size, top_k)
    h = C.c_void_p()
    st = _lib.lib().tf2_cls_create(net._h if net is not None else None, C.byref(d) if desc else None, C.byref(h))
    err = _lib.lib().tf2_last_error().decode()
    assert (st == 0) == bool(h.value)
    if h.value:
        _lib.lib().tf2_cls_destroy(h)
    return st, err


def test_create_refusals():
    assert C.sizeof(_lib.ClsDesc) == 8
    tiny = _net(cfg.tiny_tables())                                       # 10 classes
    for kw, message in ((dict(size=4), "desc size"), (dict(size=16), "desc size"), (dict(desc=False), "desc size"),
                        (dict(top_k=0), "top_k"), (dict(top_k=-3), "top_k"), (dict(top_k=11), "top_k must be in 1..10")):
        st, err = _create(tiny, **kw)
        assert st == -1 and message in err, (kw, st, err)
    st, err = _create(_net(cfg.tiny_tables(classes=1000)), top_k=65)
    assert st == -1 and "top_k must be in 1..64" in err
    st, err = _create(None)
    assert st == -1 and "null tf2_net" in err
    st, err = _create(_net(cfg.tiny_tables(), q_set=False))
    assert st == -2 and "q table" in err
    for tables in (cfg.ssd300_tables(width_div=4), cfg.vgg16_tables(64, 10, with_fc=False)):
        st, err = _create(_net(tables))
        assert st == -1 and "1 x 1" in err, (st, err)
    # the measured networks pass every host check (what is left is the device allocation: refused here without a device)
    import json
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    goog = cfg.NetTables(json.load(open(os.path.join(golden, "tables_googlenet.json"))))
    goog.setdefault("xConv1Rewrite", 1)
    for tables in (cfg.resnet50_tables(), goog, cfg.squeezenet11_tables(), cfg.vgg16_tables(32, 10), cfg.tiny_tables(classes=4096)):
        st, err = _create(_net(tables))
        assert st in (0, -4), (st, err)
    for bad in (1, -31, 127, -128):                                      # sh = -1, 31, -127, 128
        def edit(row, bad=bad):
            row[7] = bad
        st, err = _create(_net(cfg.tiny_tables(), edit=edit))
        assert st == -1 and "0..30" in err and "channel 7" in err, (bad, st, err)
    st, err = _create(_net(cfg.tiny_tables(classes=4097)))
    assert st == -5 and "4097 classes" in err


@pytest.mark.parametrize("batch,ptrs,message", [
    (0, (FAKE, FAKE), "batch"), (-1, (FAKE, FAKE), "batch"),
    (2, (None, FAKE), "null logits_dev / labels_dev"), (2, (FAKE, None), "null logits_dev / labels_dev"),
    (2, (FAKE, FAKE), "null tf2_cls handle"),
])
def test_run_refusals(batch, ptrs, message):
    """tf2_cls_run checks its arguments before it looks at the handle (a handle needs a device: tests/test_gpu_classify.py repeats
    these on a real one)"""
    st = _lib.lib().tf2_cls_run(None, ptrs[0], batch, ptrs[1], None, None, None, None, None, None, None)
    err = _lib.lib().tf2_last_error().decode()
    assert st == -1 and message in err, (st, err)


def test_classify_kernel_compiles_without_scratch():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import vmcnt_check
    seg, lds, txt = vmcnt_check.kernel_segments("classify")
    names = [k for k in seg if "classify_kernel" in k]
    assert len(names) == 1 and len(seg) == 1, seg
    assert seg[names[0]] == 0, seg
    assert "scratch_" not in txt.split("amdhsa.kernels")[0]
