"""Threshold calibration, CPU side: the statement (embed.roc_thresholds / roc_bin / reference_roc_hist / reference_pairs / roc_summary /
fold_protocol) against brute force and hand-made cases, its tie rules, the transfer of a returned threshold to the matcher's strict
'<', the host refusals of tf2_emb_roc_hist / tf2_emb_roc_pairs (no device: a refusal touches none) and the scratch-free ISA of
embed_roc.hip.  The device itself is checked in tests/test_gpu_embed_roc.py, which takes its inputs from `labelled_set` below."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tf2_amd import _lib, embed as E
from tests.test_classify import FAKE

INF, NAN = float("inf"), float("nan")


def labelled_set(n: int, D: int, seed: int, identities: int = 7):
    """(float32 unit rows [n, D], int32 ids [n]): the statement's embeddings of seeded int8 outputs; ids are a seeded mix of
    `identities` names with about 10 % negative ones (-1 and -5: unlabelled rows)"""
    rng = np.random.default_rng([seed, n, D])
    rows = E.reference_embed(rng.integers(-128, 128, (n, D)).astype(np.int8), (-rng.integers(0, 8, D)).astype(np.int8))
    ids = rng.integers(100, 100 + identities, n).astype(np.int32)
    ids[rng.random(n) < 0.1] = rng.choice([-1, -5])
    return rows, ids


def _matrix(a, b):
    """the full distance matrix as reference_match reports it: all N columns asked for, put back by row index"""
    idx, dist, _ = E.reference_match(a, b, None, b.shape[0])
    d = np.empty_like(dist)
    np.put_along_axis(d, idx.astype(np.int64), dist, axis=1)
    return d


@pytest.mark.parametrize("n_thr,step", [(1, 0.25), (400, 0.01), (4096, 0.001), (7, 3.0e37)])
def test_thresholds_are_one_float32_multiply(n_thr, step):
    thr = E.roc_thresholds(n_thr, step)
    assert thr.dtype == np.float32 and thr.shape == (n_thr,)
    with np.errstate(over="ignore"):
        for t in range(n_thr):
            assert thr[t] == np.float32(np.float32(t + 1) * np.float32(step)) or (np.isinf(thr[t]) and step > 1e37)
    assert (np.diff(thr) >= 0).all()


@pytest.mark.parametrize("n_thr,step", [(0, 0.01), (4097, 0.01), (-1, 0.01), (4, 0.0), (4, -0.5), (4, INF), (4, NAN), (4, 1e-50), (4, 1e39)])
def test_threshold_refusals(n_thr, step):
    with pytest.raises(ValueError), np.errstate(over="ignore"):
        E.roc_thresholds(n_thr, step)


def test_bin_is_searchsorted_right_with_nan_as_inf():
    thr = E.roc_thresholds(400, 0.01)
    rng = np.random.default_rng(1)
    below = np.nextafter(thr, np.float32(0)).astype(np.float32)
    above = np.nextafter(thr, np.float32(np.inf)).astype(np.float32)
    d = np.concatenate([thr, below, above, rng.random(500).astype(np.float32) * 5, np.float32([0.0, 4.0, 4.5, 1e30, INF])])
    got = E.roc_bin(d, thr)
    assert np.array_equal(got, np.searchsorted(thr, d, side="right"))
    assert np.array_equal(got, (thr[None, :] <= d[:, None]).sum(axis=1))          # the definition: #{t : thr[t] <= d}
    assert np.array_equal(got[:400], np.arange(1, 401))                              # exactly on thr[t]: t + 1 thresholds are <= d
    assert np.array_equal(got[400:800], np.arange(0, 400))                           # one ulp below
    assert got[-5:].tolist() == [0, 400, 400, 400, 400] and E.roc_bin(np.float32([4.0]), thr)[0] == 400
    assert E.roc_bin(np.float32([NAN, INF, -0.0]), thr).tolist() == [400, 400, 0]
    # accepted at threshold t iff d < thr[t] iff bin <= t
    for t in (0, 57, 399):
        assert np.array_equal(d < thr[t], got <= t)
    assert E.roc_bin(np.float32([[0.1, 0.3], [0.25, NAN]]), E.roc_thresholds(1, 0.25)).tolist() == [[0, 1], [1, 1]]


def _brute_hist(a, ia, b, ib, self_mode, n_thr, step):
    thr = E.roc_thresholds(n_thr, step)
    hist = np.zeros((2, n_thr + 1), np.int64)
    for i in range(a.shape[0]):
        for j in range(i + 1 if self_mode else 0, b.shape[0]):
            if ia[i] < 0 or ib[j] < 0:
                continue
            d = E.reference_match(a[i:i + 1], b[j:j + 1])[1][0, 0]
            hist[int(ia[i] == ib[j]), int(np.searchsorted(thr, d, side="right"))] += 1
    return hist


@pytest.mark.parametrize("D", [2, 20])
def test_reference_roc_hist_against_the_double_loop(D):
    rows, ids = labelled_set(40, D, seed=2)
    rows[5] = rows[3]                                                    # d = 0: bin 0
    rows[9, 0] = np.nan                                                  # every pair of row 9: bin T
    ids[[3, 5, 9]] = 100
    other, oids = labelled_set(23, D, seed=3)
    assert (ids < 0).any() and (oids < 0).any()
    for n_thr, step in ((400, 0.01), (5, 0.5)):
        h = E.reference_roc_hist(rows, ids, n_thr=n_thr, step=step)
        assert h.dtype == np.int64 and h.shape == (2, n_thr + 1)
        assert np.array_equal(h, _brute_hist(rows, ids, rows, ids, True, n_thr, step))
        lab = int((ids >= 0).sum())
        assert h.sum() == lab * (lab - 1) // 2 and h[1, 0] >= 1 and h[:, n_thr].sum() >= lab - 1
        x = E.reference_roc_hist(rows, ids, other, oids, n_thr=n_thr, step=step)
        assert np.array_equal(x, _brute_hist(rows, ids, other, oids, False, n_thr, step))
        assert x.sum() == lab * int((oids >= 0).sum())
    # the sums with every row labelled; rows that take no part change nothing
    pos = np.abs(ids)
    assert E.reference_roc_hist(rows, pos).sum() == 40 * 39 // 2 and E.reference_roc_hist(rows, pos, other, np.abs(oids)).sum() == 40 * 23
    keep = ids >= 0
    assert np.array_equal(E.reference_roc_hist(rows, ids), E.reference_roc_hist(rows[keep], ids[keep]))
    assert E.reference_roc_hist(rows[:1], ids[:1]).sum() == 0
    with pytest.raises(ValueError):
        E.reference_roc_hist(rows, ids[:-1])
    with pytest.raises(ValueError):
        E.reference_roc_hist(rows, ids, other[:, :1], oids)


def test_roc_summary_by_hand():
    #                 bin 0  1  2  3  4      thr = 0.25, 0.5, 0.75, 1.0
    hist = np.int64([[0, 1, 1, 3, 5],        # impostors: FA = 0, 1, 2, 5 of 10
                     [4, 3, 2, 1, 0]])       # genuine:   TA = 4, 7, 9, 10 of 10
    s = E.roc_summary(hist, 0.25, far_targets=(1e-1, 0.2, 1e-2, 0.3, Fraction(1, 2), 1))
    assert s["thresholds"].dtype == np.float32 and s["thresholds"].tolist() == [0.25, 0.5, 0.75, 1.0]
    assert s["TA"].tolist() == [4, 7, 9, 10] and s["FA"].tolist() == [0, 1, 2, 5] and (s["genuine"], s["impostors"]) == (10, 10)
    assert s["TAR"].tolist() == [0.4, 0.7, 0.9, 1.0] and s["FAR"].tolist() == [0.0, 0.1, 0.2, 0.5]
    assert s["accuracy"].tolist() == [0.7, 0.8, 0.85, 0.75]
    assert s["best_accuracy"] == dict(t=2, threshold=np.float32(0.75), accuracy=0.85)
    assert s["eer"] == dict(t=2, threshold=np.float32(0.75), far=0.2, frr=0.1)          # FAR 0.2 >= FRR 0.1 first at t = 2
    far = s["far"]
    assert far[1e-1] == dict(t=1, threshold=np.float32(0.5), fa=1, ta=7, far=0.1, tar=0.7)   # FA == target * impostors meets the target
    assert far[0.2]["t"] == 2 and far[1e-2]["t"] == 0 and far[1e-2]["fa"] == 0
    assert far[0.3]["t"] == 2                                            # 0.3 is 3/10, not the double below it: FA <= 3
    assert far[Fraction(1, 2)]["t"] == 3 and far[1]["t"] == 3 and far[1]["threshold"] == np.float32(1.0)
    assert type(far[1e-1]["threshold"]) is np.float32
    # 3/10 exactly: FA = 3 meets 0.3 although the double 0.3 times 10 is below 3
    eq = E.roc_summary(np.int64([[3, 0, 7], [1, 1, 1]]), 0.5, far_targets=(0.3,))
    assert eq["far"][0.3]["t"] == 1 and eq["far"][0.3]["fa"] == 3
    # "none": even t = 0 accepts more impostors than the target allows
    none = E.roc_summary(np.int64([[3, 0, 7], [1, 1, 1]]), 0.5, far_targets=(0.2, 1e-5))
    assert none["far"][0.2] == dict(t=None, threshold=None, fa=None, ta=None, far=None, tar=None) and none["far"][1e-5]["t"] is None
    # argmax ties: the first index of the maximum (correct = 12, 12, 11)
    tie = E.roc_summary(np.int64([[0, 1, 9], [2, 1, 1]]), 0.5)
    assert tie["best_accuracy"]["t"] == 0 and (tie["TA"] + tie["impostors"] - tie["FA"]).tolist() == [12, 12]
    assert set(tie["far"]) == set(E.FAR_TARGETS) and tie["far"][1e-1]["t"] == 1 and tie["far"][1e-2]["t"] == 0
    # no t with FAR >= FRR; empty halves
    assert E.roc_summary(np.int64([[0, 0, 5], [0, 0, 5]]), 0.5)["eer"] is None
    empty = E.roc_summary(np.int64([[0, 0, 0], [1, 1, 0]]), 0.5)
    assert empty["eer"] is None and empty["far"][1e-1]["t"] is None and empty["FAR"].tolist() == [0.0, 0.0]
    assert empty["best_accuracy"]["t"] == 1
    with pytest.raises(ValueError):
        E.roc_summary(np.zeros((3, 5), np.int64), 0.5)
    # counts beyond 2^32 (a 100 000-row set has 5e9 pairs): the comparisons are exact integers
    big = E.roc_summary(np.int64([[5 * 10 ** 4, 5 * 10 ** 9 - 5 * 10 ** 4, 0], [10 ** 6, 10 ** 6, 0]]), 0.5, far_targets=(1e-5,))
    assert big["far"][1e-5]["t"] == 0 and big["far"][1e-5]["fa"] == 5 * 10 ** 4


def test_fold_protocol_by_hand():
    # T = 2.  fold:            impostors         genuine
    h = np.int64([[[0, 2, 2], [3, 1, 0]],      # fold 0
                  [[1, 0, 3], [1, 3, 0]],      # fold 1
                  [[2, 0, 0], [0, 0, 2]]])     # fold 2
    # correct(t) = TA[t] + impostors - FA[t]:  fold 0: 3 + 4 - 0, 4 + 4 - 2 = 7, 6;  fold 1: 1 + 4 - 1, 4 + 4 - 1 = 4, 7;  fold 2: 0, 0
    # others of fold 0: 4, 7 -> t* = 1: 6 / 8;  others of fold 1: 7, 6 -> t* = 0: 4 / 8;  others of fold 2: 11, 13 -> t* = 1: 0 / 4
    p = E.fold_protocol(h)
    assert p["t"].tolist() == [1, 0, 1] and p["accuracy"].tolist() == [0.75, 0.5, 0.0]
    assert p["mean"] == np.mean([0.75, 0.5, 0.0]) and p["std"] == np.std([0.75, 0.5, 0.0])
    # a tie over the other folds takes the first t
    tie = E.fold_protocol(np.int64([[[0, 1, 0], [1, 0, 0]], [[0, 1, 0], [0, 1, 0]]]))
    assert tie["t"].tolist() == [0, 0] and tie["accuracy"].tolist() == [1.0, 0.5]
    with pytest.raises(ValueError):
        E.fold_protocol(h[0])


def test_reference_pairs_and_every_kind_of_invalid_pair():
    rows, _ = labelled_set(12, 20, seed=4)
    rows[7, 3] = np.nan
    pairs = np.int32([[0, 1, 1, 0], [2, 3, 0, 1], [4, 4, 1, 2], [5, 7, 0, 2], [1, 0, 0, 0],
                      [12, 1, 0, 0], [1, 12, 0, 0], [-1, 1, 0, 0], [1, -1, 1, 0], [1, 2, 2, 0], [1, 2, -1, 0], [1, 2, 0, 3], [1, 2, 0, -1]])
    dist, hist, invalid = E.reference_pairs(rows, pairs, n_folds=3, n_thr=8, step=0.5)
    assert dist.dtype == np.float32 and hist.shape == (3, 2, 9) and hist.dtype == np.int64 and invalid == 8
    assert (dist[5:] == -1.0).all() and hist.sum() == 5
    thr = E.roc_thresholds(8, 0.5)
    want = np.zeros_like(hist)
    for p in range(5):
        a, b, same, fold = pairs[p]
        d = E.reference_match(rows[a:a + 1], rows[b:b + 1])[1][0, 0]
        assert dist[p].tobytes() == d.tobytes()
        want[fold, same, np.searchsorted(thr, d, side="right")] += 1
    assert np.array_equal(hist, want)
    assert dist[2] == 0.0 and hist[2, 1, 0] == 1 and np.isposinf(dist[3]) and hist[2, 0, 8] == 1 and dist[0] == dist[4]
    with pytest.raises(ValueError):
        E.reference_pairs(rows, pairs, n_folds=17)
    with pytest.raises(ValueError):
        E.reference_pairs(rows, pairs, n_folds=0)


@pytest.mark.parametrize("target", [1e-1, 1e-2, 0.37])
def test_a_returned_threshold_means_the_same_to_the_matcher(target):
    """the threshold for a FAR target, handed to the matcher's rule (reference_match's distance, strict '<'), accepts no more than
    target * impostors impostor pairs, and the next threshold of the grid accepts more"""
    rows, ids = labelled_set(60, 8, seed=5, identities=6)
    s = E.roc_summary(E.reference_roc_hist(rows, ids, n_thr=400, step=0.01), 0.01, far_targets=(target,))
    got = s["far"][target]
    assert got["t"] is not None and got["t"] + 1 < 400
    d = _matrix(rows, rows)
    i, j = np.triu_indices(60, 1)
    impostor = (ids[i] >= 0) & (ids[j] >= 0) & (ids[i] != ids[j])
    assert impostor.sum() == s["impostors"]
    limit = Fraction(repr(target)) * int(impostor.sum())
    accepted = int((d[i, j][impostor] < got["threshold"]).sum())
    assert accepted == got["fa"] and accepted <= limit
    assert int((d[i, j][impostor] < s["thresholds"][got["t"] + 1]).sum()) > limit


HIST_OK = dict(a=FAKE, ia=FAKE, n_a=5, b=None, ib=None, n_b=0, d=128, n_thr=400, step=0.01, hist=FAKE)


@pytest.mark.parametrize("kw,message", [
    (dict(d=1), "d must be in 2..512"), (dict(d=513), "d must be in 2..512"), (dict(n_a=0), "n_a"), (dict(n_a=-3), "n_a"),
    (dict(b=FAKE, ib=FAKE, n_b=0), "n_b"), (dict(n_thr=0), "n_thr must be in 1..4096"), (dict(n_thr=4097), "n_thr must be in 1..4096"),
    (dict(step=0.0), "step"), (dict(step=-1.0), "step"), (dict(step=INF), "step"), (dict(step=NAN), "step"),
    (dict(a=None), "null rows_a_dev / ids_a_dev"), (dict(ia=None), "null rows_a_dev / ids_a_dev"),
    (dict(b=FAKE, n_b=3), "null ids_b_dev"), (dict(hist=None), "null hist_dev"),
])
def test_roc_hist_refusals(kw, message):
    """tf2_emb_roc_hist checks its arguments before any device call (tests/test_gpu_embed_roc.py shows the accepted calls)"""
    k = dict(HIST_OK, **kw)
    st = _lib.lib().tf2_emb_roc_hist(k["a"], k["ia"], k["n_a"], k["b"], k["ib"], k["n_b"], k["d"], k["n_thr"], k["step"], k["hist"], None)
    err = _lib.lib().tf2_last_error().decode()
    assert st == -1 and "tf2_emb_roc_hist" in err and message in err, (st, err)


PAIRS_OK = dict(rows=FAKE, n_rows=5, d=128, pairs=FAKE, n_pairs=3, n_folds=10, n_thr=400, step=0.01, dist=FAKE, hist=FAKE, invalid=FAKE)


@pytest.mark.parametrize("kw,message", [
    (dict(d=1), "d must be in 2..512"), (dict(d=600), "d must be in 2..512"), (dict(n_rows=0), "n_rows"), (dict(n_pairs=0), "n_pairs"),
    (dict(n_pairs=-1), "n_pairs"), (dict(n_folds=0), "n_folds must be in 1..16"), (dict(n_folds=17), "n_folds must be in 1..16"),
    (dict(n_thr=0), "n_thr"), (dict(n_thr=5000), "n_thr"), (dict(step=0.0), "step"), (dict(step=NAN), "step"), (dict(step=-INF), "step"),
    (dict(rows=None), "null rows_dev / pairs_dev"), (dict(pairs=None), "null rows_dev / pairs_dev"),
    (dict(dist=None), "null dist_dev / hist_dev / invalid_dev"), (dict(hist=None), "null dist_dev / hist_dev / invalid_dev"),
    (dict(invalid=None), "null dist_dev / hist_dev / invalid_dev"),
])
def test_roc_pairs_refusals(kw, message):
    k = dict(PAIRS_OK, **kw)
    st = _lib.lib().tf2_emb_roc_pairs(k["rows"], k["n_rows"], k["d"], k["pairs"], k["n_pairs"], k["n_folds"], k["n_thr"], k["step"],
                                      k["dist"], k["hist"], k["invalid"], None)
    err = _lib.lib().tf2_last_error().decode()
    assert st == -1 and "tf2_emb_roc_pairs" in err and message in err, (st, err)


def test_constants_and_the_tile_pair_limit():
    assert (E.ROC_MAX_THR, E.ROC_MAX_FOLDS, E.ROC_TILE) == (4096, 16, 256)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tf2_amd", "csrc", "embed_roc.h")).read()
    for name, value in (("kRocMaxThr", 4096), ("kRocMaxFolds", 16), ("kRocTile", E.ROC_TILE)):
        assert re.search(rf"constexpr int {name} = {value};", hdr), name
    # 2^31 - 1 rows a side in cross mode: 2^46 tile pairs, more than one grid holds (refused before any device call)
    n = 2 ** 31 - 1
    st = _lib.lib().tf2_emb_roc_hist(FAKE, FAKE, n, FAKE, FAKE, n, 128, 400, 0.01, FAKE, None)
    assert st == -5 and "too many tile pairs" in _lib.lib().tf2_last_error().decode()


def test_embed_roc_kernels_compile_without_scratch():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import vmcnt_check
    seg, lds, txt = vmcnt_check.kernel_segments("embed_roc")
    assert len(seg) == 2, seg
    for kernel in ("roc_hist_kernel", "roc_pairs_kernel"):
        names = [k for k in seg if kernel in k]
        assert len(names) == 1 and seg[names[0]] == 0, (kernel, seg)
    assert "scratch_" not in txt.split("amdhsa.kernels")[0]
    assert "v_mfma" not in txt and "v_dot" not in txt and "v_fma_f32" not in txt and "v_fmac_f32" not in txt and "v_pk_fma_f32" not in txt
