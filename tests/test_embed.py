"""Face matching, CPU side: the statement (embed.reference_embed / reference_match / reference_tally) against independent
restatements and derived bounds, its tie, padding and NaN rules, the tally rules, the host refusals of tf2_emb_create / tf2_emb_embed /
tf2_emb_match (no device: a refusal touches none) and the scratch-free ISA of embed_match.hip.  The device itself is checked in
tests/test_gpu_embed.py, which takes its inputs from `family` below."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tf2_amd import _lib, classify as K, config as cfg, embed as E
from tests.test_classify import FAKE, _net

FAMILIES = ["random", "two_valued", "extreme_sh0", "extreme_sh30", "copies", "dup_within", "dup_across"]
TIE_FAMILIES = ("dup_within", "dup_across")


def outputs_of(kind: str, rng, rows: int, D: int):
    """int8 network outputs [rows, D] of one family"""
    if kind == "two_valued":
        vals = rng.integers(-128, 128, (rows, 2))
        return np.take_along_axis(vals, rng.integers(0, 2, (rows, D)), axis=1).astype(np.int8)
    if kind in ("extreme_sh0", "extreme_sh30"):
        return np.where(rng.integers(0, 2, (rows, D)) == 1, 127, -128).astype(np.int8)
    return rng.integers(-128, 128, (rows, D)).astype(np.int8)


def family(kind: str, D: int, B: int, N: int, k: int, seed: int):
    """(int8 outputs [B, D], runtime Q row int8 [D] = -sh, gallery float32 [N, D], ids int32 [N]) of one input family; the Q row
    depends on (kind, D, seed) alone.  Gallery rows are the statement's embeddings of int8 outputs of the same family (what enrolling
    writes); ids repeat, so that several rows carry one identity.
      copies      query b is gallery row (b * 37) % N's own int8 output: distance exactly 0.0
      dup_within  every distinct row stands k + 2 times in a run of consecutive rows (runs cross the slab boundaries as well)
      dup_across  row n equals row n % P, P = max(1, N // (k + 2)): at least k + 2 copies of every row, P rows apart"""
    rng = np.random.default_rng([seed, D, B, N, FAMILIES.index(kind)])
    rng_q = np.random.default_rng([seed, D, FAMILIES.index(kind)])
    sh = np.zeros(D, np.int64)
    if kind in ("random", "copies", "dup_within", "dup_across"):
        sh = rng_q.integers(0, 8, D)
    elif kind == "two_valued":
        sh[:] = 2
    elif kind == "extreme_sh30":
        sh[:] = 30
    q = (-sh).astype(np.int8)
    out = outputs_of(kind, rng, B, D)
    gal_out = outputs_of(kind, rng, N, D)
    if kind == "dup_within":
        gal_out = gal_out[np.arange(N) // (k + 2)]
    elif kind == "dup_across":
        gal_out = gal_out[np.arange(N) % max(1, N // (k + 2))]
    elif kind == "copies":
        out = gal_out[(np.arange(B) * 37) % N].copy()
    gallery = E.reference_embed(gal_out, q)
    ids = (rng.permutation(N) // 3 + 100).astype(np.int32)               # three rows an identity, none below 100
    return out, q, gallery, ids


def _embed_scalar(out, q):
    """reference_embed restated one float32 operation at a time on classify's features"""
    f = K.features_of(out, q)
    e = np.zeros_like(f)
    for b in range(f.shape[0]):
        s = np.float32(0.0)
        for c in range(f.shape[1]):
            s = np.float32(s + np.float32(f[b, c] * f[b, c]))
        if s != 0:
            norm = np.float32(np.sqrt(np.float64(s)))                    # |s| < 2^53: the float64 root rounded again is the correctly rounded float32 root
            for c in range(f.shape[1]):
                e[b, c] = np.float32(f[b, c] / norm)
    return e


@pytest.mark.parametrize("kind", ["random", "two_valued", "extreme_sh0", "extreme_sh30", "mixed"])
@pytest.mark.parametrize("D", [2, 5, 128, 512])
def test_reference_embed(kind, D):
    """bit-identical to the scalar restatement on classify.features_of's features; a unit norm within (D + 2) 2^-24: the sum of D
    rounded products rounded D times is within (D + 1) 2^-24 relative of the exact one (first order), the root halves that and
    rounds once more, each division rounds once (a relative 2^-24 of every e[c], so 2^-24 of the norm): (D + 1) / 2 + 2 <= D + 2"""
    rng = np.random.default_rng([D, len(kind)])
    if kind == "mixed":
        sh = rng.choice([0, 3, 6, 30], D)
        out = (rng.integers(-1, 2, (6, D)) << np.minimum(sh, 6)[None, :]).astype(np.int8)
        q = (-sh).astype(np.int8)
    else:
        out, q, _, _ = family(kind, D, 6, 1, 1, seed=1)
    out[0] = 0                                                           # the zero embedding
    e = E.reference_embed(out, q)
    assert e.dtype == np.float32 and e.shape == (6, D)
    assert np.array_equal(e.view(np.uint32), _embed_scalar(out, q).view(np.uint32))
    assert (e[0] == 0).all() and not np.signbit(e[0]).any()
    norms = np.sqrt((e[1:].astype(np.float64) ** 2).sum(axis=1))
    live = (out[1:] != 0).any(axis=1)
    print(f"{kind} D={D}: |norm - 1| <= {np.abs(norms[live] - 1).max() if live.any() else 0:.3e}, bound {(D + 2) * 2.0 ** -24:.3e}")
    assert (np.abs(norms[live] - 1) <= (D + 2) * 2.0 ** -24).all()
    assert (norms[~live] == 0).all()
    # the features are classify's: one channel alone gives exactly +-1 there
    one = np.zeros((2, D), np.int8)
    one[0, D - 1], one[1, 0] = -128, 127
    e1 = E.reference_embed(one, q)
    assert e1[0, D - 1] == -1.0 and e1[1, 0] == 1.0 and np.count_nonzero(e1) == 2
    with pytest.raises(ValueError):
        E.reference_embed(out, np.ones(D, np.int8))                      # sh = -1
    with pytest.raises(ValueError):
        E.reference_embed(out, np.full(D, -31, np.int8))                 # sh = 31


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("D,k,B,N", [(2, 1, 3, 1), (5, 5, 4, 3), (128, 5, 8, 65), (128, 16, 5, 200), (512, 5, 3, 130)])
def test_reference_match_against_float64(kind, D, k, B, N):
    """every reported distance within (D + 2) 2^-24 max(d, 1) of the float64 brute force on the same float32 operands (D
    subtractions, products and sums, each a relative 2^-24 of a partial sum of non-negative terms: first order (D + 2) 2^-24 d),
    the reported rows in an order the float64 distances contradict by no more than that, the tie and padding rules exactly"""
    out, q, g, ids = family(kind, D, B, N, k, seed=2)
    e = E.reference_embed(out, q)
    idx, dist, rid = E.reference_match(e, g, ids, k)
    assert idx.dtype == np.int32 and dist.dtype == np.float32 and rid.dtype == np.int32 and idx.shape == dist.shape == rid.shape == (B, k)
    d64 = ((e.astype(np.float64)[:, None, :] - g.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    m = min(k, N)
    got64 = np.take_along_axis(d64, idx[:, :m].astype(np.int64), axis=1)
    tol = (D + 2) * 2.0 ** -24 * np.maximum(got64, 1.0)
    assert (np.abs(dist[:, :m] - got64) <= tol).all()
    assert (np.sort(d64, axis=1)[:, :m] >= got64 - 2 * tol).all() and (np.sort(d64, axis=1)[:, :m] <= got64 + 2 * tol).all()
    assert (idx[:, m:] == -1).all() and np.isposinf(dist[:, m:]).all() and (rid[:, m:] == -1).all()
    assert np.array_equal(rid[:, :m], ids[idx[:, :m]])
    # ordered by (distance, row); rows never repeat
    for b in range(B):
        pairs = list(zip(dist[b, :m].tolist(), idx[b, :m].tolist()))
        assert pairs == sorted(pairs) and len(set(idx[b, :m].tolist())) == m
    plain = E.reference_match(e, g, None, k)
    assert np.array_equal(plain[0], idx) and np.array_equal(plain[2], idx)
    if kind == "copies":
        want = (np.arange(B) * 37) % N
        assert (dist[:, 0] == 0.0).all() and not np.signbit(dist[:, 0]).any()
        assert (g[idx[:, 0]] == g[want]).all() and (idx[:, 0] <= want).all()
    if kind in TIE_FAMILIES and N >= k + 2:
        wider = E.reference_match(e, g, ids, k + 1)[1]
        assert (wider[:, k - 1] == wider[:, k]).any()


def test_duplicates_come_out_in_index_order_and_nan_sorts_last():
    rng = np.random.default_rng(3)
    q = np.zeros(8, np.int8)
    rows = E.reference_embed(rng.integers(-128, 128, (4, 8)).astype(np.int8), q)
    g = rows[[0, 1, 0, 2, 0, 1, 3, 0]]                                   # row 0 at 0, 2, 4, 7
    idx, dist, rid = E.reference_match(rows[:1], g, None, 6)
    assert idx[0, :4].tolist() == [0, 2, 4, 7] and (dist[0, :4] == 0.0).all() and dist[0, 4] > 0
    bad = g.copy()
    bad[0, 3] = np.nan                                                    # the best row turns into the worst
    bad[2, 0] = np.inf                                                    # inf - x = inf: a real +inf distance, before the NaN row by index only
    idx, dist, rid = E.reference_match(rows[:1], bad, None, 8)
    assert idx[0, :2].tolist() == [4, 7] and idx[0, -2:].tolist() == [0, 2]
    assert np.isposinf(dist[0, -2:]).all() and not np.isnan(dist).any()
    # N < k
    idx, dist, rid = E.reference_match(rows[:2], g[:3], np.int32([7, 8, 9]), 5)
    assert (idx[:, 3:] == -1).all() and np.isposinf(dist[:, 3:]).all() and (rid[:, 3:] == -1).all()
    assert idx[0, :3].tolist() == [0, 2, 1] and rid[0, :3].tolist() == [7, 9, 8]
    with pytest.raises(ValueError):
        E.reference_match(rows, g[:, :4], None, 2)
    with pytest.raises(ValueError):
        E.reference_match(rows, g, None, 0)


def test_tally_rules():
    idx = np.int32([[0, 1, 2]] * 8)
    ids = np.int32([[10, 11, 12]] * 8)
    dist = np.float32([[0.5, 0.7, 0.9]] * 8)
    dist[6, 0] = 0.25                                                     # exactly the threshold: rejected
    dist[7, 0] = np.float32(0.25) - np.float32(2.0 ** -26)                # one ulp below: accepted
    truth = np.int32([10, 11, 12, 13, -1, -7, 10, 10])
    #        first, second, third, impostor, unlabelled, unlabelled, first, first
    assert E.reference_tally(idx, dist, ids, truth, 0.6).tolist() == [6, 3, 5, 3, 3]      # every first row accepted: the impostor and the two others falsely
    assert E.reference_tally(idx, dist, ids, truth, 0.25).tolist() == [6, 3, 5, 1, 0]     # strict '<': 0.25 is not below 0.25
    assert E.reference_tally(idx, dist, ids, truth, 0.0).tolist() == [6, 3, 5, 0, 0]
    assert E.reference_tally(idx, dist, ids, truth, np.inf).tolist() == [6, 3, 5, 3, 3]
    assert E.reference_tally(idx, dist, ids, np.full(8, -1), 0.6).tolist() == [0, 0, 0, 0, 0]
    assert E.reference_tally(idx, dist, ids, truth, 0.6).dtype == np.uint64
    # padded slots (id -1) match no label; an empty first slot cannot occur (N >= 1), +inf is never below a finite threshold
    pad_ids = np.int32([[10, -1, -1]])
    pad_dist = np.float32([[np.inf, np.inf, np.inf]])
    assert E.reference_tally(idx[:1], pad_dist, pad_ids, np.int32([10]), 1e30).tolist() == [1, 1, 1, 0, 0]
    assert E.reference_tally(idx[:1], pad_dist, pad_ids, np.int32([3]), 1e30).tolist() == [1, 0, 0, 0, 0]


def _create(net, top_k=5, size=None, desc=True):
    d = _lib.EmbDesc(C.sizeof(_lib.EmbDesc) if size is None else size, top_k)
    h = C.c_void_p()
    st = _lib.lib().tf2_emb_create(net._h if net is not None else None, C.byref(d) if desc else None, C.byref(h))
    err = _lib.lib().tf2_last_error().decode()
    assert (st == 0) == bool(h.value)
    if h.value:
        _lib.lib().tf2_emb_destroy(h)
    return st, err


def test_create_refusals():
    assert C.sizeof(_lib.EmbDesc) == 8
    assert (E.MAX_D, E.MAX_TOP_K, E.SLAB, E.GROUP) == (512, 16, 64, 32)
    tiny = _net(cfg.tiny_tables())                                       # D = 10
    for kw, message in ((dict(size=4), "desc size"), (dict(size=16), "desc size"), (dict(desc=False), "desc size"),
                        (dict(top_k=0), "top_k must be in 1..16"), (dict(top_k=-3), "top_k"), (dict(top_k=17), "top_k must be in 1..16")):
        st, err = _create(tiny, **kw)
        assert st == -1 and message in err, (kw, st, err)
    st, err = _create(None)
    assert st == -1 and "null tf2_net" in err
    st, err = _create(_net(cfg.tiny_tables(), q_set=False))
    assert st == -2 and "q table" in err
    for tables in (cfg.ssd300_tables(width_div=4), cfg.vgg16_tables(64, 10, with_fc=False)):
        st, err = _create(_net(tables))
        assert st == -1 and "1 x 1" in err, (st, err)
    # the embedding network and every legal D pass the host checks (what is left is the device allocation: refused here without a device);
    # top_k may exceed D and the rows of a gallery
    for tables, k in ((cfg.squeezenet11_tables(), 5), (cfg.tiny_tables(classes=2), 16), (cfg.tiny_tables(classes=512), 1)):
        st, err = _create(_net(tables), top_k=k)
        assert st in (0, -4), (st, err)
    for bad in (1, -31, 127, -128):                                      # sh = -1, 31, -127, 128
        def edit(row, bad=bad):
            row[7] = bad
        st, err = _create(_net(cfg.tiny_tables(), edit=edit))
        assert st == -1 and "0..30" in err and "channel 7" in err, (bad, st, err)
    for classes in (513, 1000):
        st, err = _create(_net(cfg.tiny_tables(classes=classes)))
        assert st == -5 and f"{classes} values" in err, (st, err)


NAN = float("nan")


@pytest.mark.parametrize("batch,n_rows,thr,ptrs,message", [
    (0, 4, 1.0, (FAKE,) * 5, "batch"), (-1, 4, 1.0, (FAKE,) * 5, "batch"),
    (2, 0, 1.0, (FAKE,) * 5, "n_rows"), (2, -5, 1.0, (FAKE,) * 5, "n_rows"),
    (2, 4, 1.0, (None, FAKE, FAKE, FAKE, FAKE), "null out_i8_dev / gallery_dev"),
    (2, 4, 1.0, (FAKE, None, FAKE, FAKE, FAKE), "null out_i8_dev / gallery_dev"),
    (2, 4, 1.0, (FAKE, FAKE, None, FAKE, FAKE), "null scratch_dev"),
    (2, 4, 1.0, (FAKE, FAKE, FAKE, None, FAKE), "null idx_dev / dist_dev"),
    (2, 4, 1.0, (FAKE, FAKE, FAKE, FAKE, None), "null idx_dev / dist_dev"),
    (2, 4, NAN, (FAKE,) * 5, "threshold is NaN"),
    (2, 4, 1.0, (FAKE,) * 5, "null tf2_emb handle"),
])
def test_match_refusals(batch, n_rows, thr, ptrs, message):
    """tf2_emb_match checks its arguments before it looks at the handle (a handle needs a device: tests/test_gpu_embed.py repeats
    these, and the scratch size, on a real one)"""
    out, gal, scratch, idx, dist = ptrs
    st = _lib.lib().tf2_emb_match(None, out, batch, gal, None, n_rows, thr, scratch, 1 << 20, idx, dist, None, None, None, None, None)
    err = _lib.lib().tf2_last_error().decode()
    assert st == -1 and message in err, (st, err)


@pytest.mark.parametrize("batch,ptrs,message", [
    (0, (FAKE, FAKE), "batch"), (2, (None, FAKE), "null out_i8_dev / rows_dev"), (2, (FAKE, None), "null out_i8_dev / rows_dev"),
    (2, (FAKE, FAKE), "null tf2_emb handle"),
])
def test_embed_refusals(batch, ptrs, message):
    st = _lib.lib().tf2_emb_embed(None, ptrs[0], batch, ptrs[1], None)
    err = _lib.lib().tf2_last_error().decode()
    assert st == -1 and message in err, (st, err)
    assert _lib.lib().tf2_emb_scratch_size(None, 32, 1000) == 0


def test_embed_match_kernels_compile_without_scratch():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import vmcnt_check
    seg, lds, txt = vmcnt_check.kernel_segments("embed_match")
    assert len(seg) == 3, seg
    for kernel in ("embed_kernel", "match_slab_kernel", "match_merge_kernel"):
        names = [k for k in seg if kernel in k]
        assert len(names) == 1 and seg[names[0]] == 0, (kernel, seg)
    assert "scratch_" not in txt.split("amdhsa.kernels")[0]
    assert "v_mfma" not in txt and "v_dot" not in txt                     # the distances: plain float32 vector arithmetic in a fixed order
