"""Threshold calibration on the MI355X (tf2_emb_roc_*, embed_roc.hip): every histogram equal to the statement
(embed.reference_roc_hist / reference_pairs) as integers and every distance bitwise, at every row count where the all-pairs kernel
takes another path (no pair, one pair, the 64-row sub-tile and the 256-row tile with one row less and one more, diagonal and
off-diagonal tiles, ragged last tiles), every staging path (D % 4 != 0, 16-byte rows, an unaligned base), the grid sizes, the exact
edges of the binning, accumulation, listed pairs with every kind of invalid pair, and a captured graph of enrol + add."""
import numpy as np
import pytest

from tf2_amd import embed as E
from tests.test_embed_roc import labelled_set
from tests.test_gpu_embed import _bits, _dev, _matcher

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = E.ROC_TILE


def _hist(roc):
    import torch
    torch.cuda.synchronize()
    return roc.hist.cpu().numpy()


@pytest.mark.parametrize("D", [2, 20, 128, 512])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 130, 200, T - 1, T, T + 1, 2 * T + 9])
def test_self_mode(N, D):
    rows, ids = labelled_set(N, D, seed=11)
    roc = E.DeviceRoc(400, 0.01, device=DEV)
    roc.add(_dev(rows), _dev(ids))
    want = E.reference_roc_hist(rows, ids, n_thr=400, step=0.01)
    got = _hist(roc)
    assert got.shape == (1, 2, 401) and got.dtype == np.int64
    assert np.array_equal(got[0], want), (N, D, np.flatnonzero((got[0] != want).any(axis=0))[:8])
    lab = int((ids >= 0).sum())
    assert got.sum() == lab * (lab - 1) // 2
    if N >= 63:
        assert want[0].sum() > 0 and want[1].sum() > 0 and lab < N           # both halves and the skipping are exercised


@pytest.mark.parametrize("D", [2, 128])
@pytest.mark.parametrize("n_a,n_b", [(33, 70), (1, 1), (T + 44, T + 1)])
def test_cross_mode(n_a, n_b, D):
    a, ia = labelled_set(n_a, D, seed=12)
    b, ib = labelled_set(n_b, D, seed=13)
    ia[0], ib[0] = 103, 103
    roc = E.DeviceRoc(400, 0.01, device=DEV)
    roc.add(_dev(a), _dev(ia), other=_dev(b), other_ids=_dev(ib))
    want = E.reference_roc_hist(a, ia, b, ib, n_thr=400, step=0.01)
    assert np.array_equal(_hist(roc)[0], want) and want.sum() == int((ia >= 0).sum()) * int((ib >= 0).sum())
    # a set against itself in cross mode: every ordered pair, the diagonal included
    roc.reset()
    roc.add(_dev(a), _dev(ia), other=_dev(a), other_ids=_dev(ia))
    assert np.array_equal(_hist(roc)[0], E.reference_roc_hist(a, ia, a, ia, n_thr=400, step=0.01))


def test_gallery_the_first_n_rows_and_an_unaligned_base():
    """a Gallery's enrolled rows (not its capacity), n below them, and rows that start 4 bytes past a 16-byte boundary (D = 128 on the
    scalar staging)"""
    import torch
    D, N = 128, 150
    rows, ids = labelled_set(N, D, seed=14)
    gal = E.Gallery(N + 30, D, DEV)
    gal.load(rows, ids)
    roc = E.DeviceRoc(400, 0.01, device=DEV)
    roc.add(gal)
    assert np.array_equal(_hist(roc)[0], E.reference_roc_hist(rows, ids)) and np.array_equal(roc.reference(gal), E.reference_roc_hist(rows, ids))
    roc.reset()
    roc.add(gal, n=70)
    assert np.array_equal(_hist(roc)[0], E.reference_roc_hist(rows[:70], ids[:70]))
    buf = torch.zeros(N * D + 1, dtype=torch.float32, device=DEV)
    off = buf[1:].view(N, D)
    off.copy_(_dev(rows))
    assert off.data_ptr() % 16 == 4
    roc.reset()
    roc.add(off, _dev(ids), other=gal)
    assert np.array_equal(_hist(roc)[0], E.reference_roc_hist(rows, ids, rows, ids))


@pytest.mark.parametrize("n_thr,step", [(1, 2.0), (400, 0.01), (4096, 0.001), (4096, 3.0e-5)])
def test_grid_sizes(n_thr, step):
    rows, ids = labelled_set(130, 20, seed=15)
    roc = E.DeviceRoc(n_thr, step, device=DEV)
    roc.add(_dev(rows), _dev(ids))
    want = E.reference_roc_hist(rows, ids, n_thr=n_thr, step=step)
    assert np.array_equal(_hist(roc)[0], want)
    assert np.count_nonzero(want.sum(axis=0)) >= min(n_thr, 50)            # the pairs are spread over the grid


def test_exact_edges():
    """d == thr[0] lands in bin 1, duplicates in bin 0, a NaN row in bin T, a denormal square is kept; the listed-pairs distance of
    the last is the one DeviceMatcher.match reports for the same two rows"""
    import torch
    D = 4
    rows = np.zeros((7, D), np.float32)
    rows[0, 0] = 0.5                      # d(0, 1) = 0.25 = thr[0]
    rows[2, 0] = 0.5                      # d(0, 2) = 0
    rows[3, 1] = np.nan
    rows[4, 0] = 1.0                      # the embedding of the int8 output (64, 0, 0, 0)
    rows[5, 0], rows[5, 1] = 1.0, 2.0 ** -70                 # d(4, 5) = 2^-140, a denormal
    rows[6, 0] = np.float32(0.5) + np.float32(2.0 ** -24)    # d(6, 1) one step above 0.25; d(6, 0) = 2^-48
    ids = np.int32([1, 1, 1, 1, 2, 2, 1])
    roc = E.DeviceRoc(8, 0.25, device=DEV)
    roc.add(_dev(rows), _dev(ids))
    want = E.reference_roc_hist(rows, ids, n_thr=8, step=0.25)
    got = _hist(roc)[0]
    assert np.array_equal(got, want)
    assert got[1, 8] == 4 and got[0, 8] == 2                  # the NaN row against its 4 genuine and 2 impostor partners
    assert got[1, 1] == 3                                     # (0, 1), (1, 2), (1, 6): 0.25 and just above are not below thr[0]
    assert got[1, 0] == 4                                     # (0, 2), (0, 6), (2, 6), (4, 5)
    # a grid of denormal thresholds: 2^-140 lies between thr[0] = 3 * 2^-142 and thr[1] = 6 * 2^-142
    fine = E.DeviceRoc(2, 3 * 2.0 ** -142, device=DEV)
    pairs = np.int32([[4, 5, 1, 0], [5, 4, 1, 0], [0, 1, 1, 0], [0, 2, 1, 0], [3, 0, 0, 0], [0, 6, 1, 0]])
    dist = fine.add_pairs(_dev(rows), _dev(pairs))
    want_d, want_h, inv = fine.reference_pairs(rows, pairs)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dist), _bits(want_d)) and np.array_equal(_hist(fine), want_h) and inv == 0
    d = dist.cpu().numpy()
    assert d[0] == np.float32(2.0 ** -140) and d[1] == d[0] and d[2] == 0.25 and d[3] == 0.0 and np.isposinf(d[4]) and d[5] == np.float32(2.0 ** -48)
    assert want_h[0, 1].tolist() == [1, 2, 2] and want_h[0, 0].tolist() == [0, 0, 1]
    m = _matcher(D, 1, np.zeros(D, np.int8))
    res = m.match(_dev(np.int8([[64, 0, 0, 0]])), _dev(rows[5:6]))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(res.embeddings), _bits(rows[4:5])) and np.array_equal(_bits(res.dist)[0], _bits(dist)[:1])


def test_accumulation_and_reset():
    a, ia = labelled_set(200, 128, seed=16)
    b, ib = labelled_set(70, 128, seed=17)
    roc = E.DeviceRoc(400, 0.01, device=DEV)
    roc.add(_dev(a), _dev(ia))
    roc.add(_dev(b), _dev(ib), other=_dev(a), other_ids=_dev(ia))
    want = E.reference_roc_hist(a, ia) + E.reference_roc_hist(b, ib, a, ia)
    assert np.array_equal(_hist(roc)[0], want)
    s, ref = roc.summary(), E.roc_summary(want, 0.01)
    assert np.array_equal(s["TA"], ref["TA"]) and np.array_equal(s["FA"], ref["FA"]) and s["far"] == ref["far"] and s["eer"] == ref["eer"]
    assert s["far"][1e-2]["t"] is not None and type(s["far"][1e-2]["threshold"]) is np.float32
    roc.reset()
    assert not _hist(roc).any()
    roc.add(_dev(b), _dev(ib))
    assert np.array_equal(_hist(roc)[0], E.reference_roc_hist(b, ib))
    with pytest.raises(ValueError):
        E.DeviceRoc(400, 0.01, n_folds=2, device=DEV).add(_dev(b), _dev(ib))


@pytest.mark.parametrize("D", [2, 128, 512])
def test_listed_pairs(D):
    import torch
    N, P, K = 50, 403, 10
    rows, ids = labelled_set(N, D, seed=18)
    rng = np.random.default_rng(19)
    pairs = np.stack([rng.integers(0, N, P), rng.integers(0, N, P), rng.integers(0, 2, P), rng.integers(0, K, P)], axis=1).astype(np.int32)
    pairs[:, 2] = ids[pairs[:, 0]] == ids[pairs[:, 1]]
    bad = {3: (N, 1, 0, 0), 40: (1, N, 0, 0), 77: (-1, 1, 0, 0), 150: (1, -1, 1, 0), 151: (1, 2, 2, 0), 300: (1, 2, -1, 0),
           301: (1, 2, 0, K), 402: (1, 2, 0, -1), 200: (2 ** 31 - 1, 0, 0, 0), 201: (0, -2 ** 31, 1, 9)}
    for p, v in bad.items():
        pairs[p] = v
    roc = E.DeviceRoc(400, 0.01, n_folds=K, device=DEV)
    dist = roc.add_pairs(_dev(rows), _dev(pairs))
    want_d, want_h, want_inv = roc.reference_pairs(rows, pairs)
    torch.cuda.synchronize()
    assert want_inv == len(bad) and (want_d[list(bad)] == -1.0).all() and (want_h.sum(axis=(1, 2)) > 0).all()
    assert np.array_equal(_bits(dist), _bits(want_d))
    assert np.array_equal(_hist(roc), want_h) and int(roc.invalid.cpu()[0]) == want_inv
    f, ref = roc.folds(), E.fold_protocol(want_h)
    assert np.array_equal(f["t"], ref["t"]) and np.array_equal(f["accuracy"], ref["accuracy"]) and (f["mean"], f["std"]) == (ref["mean"], ref["std"])
    assert np.array_equal(roc.summary()["TA"], E.roc_summary(want_h.sum(axis=0), 0.01)["TA"])
    # invalid pairs alone: counted, dist -1, nothing added; the counter accumulates until reset()
    only = np.int32([bad[p] for p in sorted(bad)])
    dist = roc.add_pairs(_dev(rows), _dev(only))
    torch.cuda.synchronize()
    assert (dist.cpu().numpy() == -1.0).all() and np.array_equal(_hist(roc), want_h) and int(roc.invalid.cpu()[0]) == 2 * len(bad)
    roc.reset()
    torch.cuda.synchronize()
    assert int(roc.invalid.cpu()[0]) == 0 and not _hist(roc).any()


def test_listed_pairs_of_a_probe_batch_give_the_matchers_nearest_distance():
    import torch
    D, B, N = 128, 5, 70
    rng = np.random.default_rng(20)
    q = (-rng.integers(0, 8, D)).astype(np.int8)
    gal = E.reference_embed(rng.integers(-128, 128, (N, D)).astype(np.int8), q)
    out = rng.integers(-128, 128, (B, D)).astype(np.int8)
    m = _matcher(D, 1, q)
    rows = torch.empty(N + B, D, dtype=torch.float32, device=DEV)
    rows[:N].copy_(_dev(gal))
    m.embed(_dev(out), out=rows[N:])
    res = m.match(_dev(out), rows[:N])
    pairs = np.int32([[N + b, j, 0, 0] for b in range(B) for j in range(N)])
    roc = E.DeviceRoc(400, 0.01, device=DEV)
    dist = roc.add_pairs(rows, _dev(pairs))
    torch.cuda.synchronize()
    nearest = dist.cpu().numpy().reshape(B, N).min(axis=1)
    assert np.array_equal(_bits(nearest), _bits(res.dist)[:, 0])
    assert np.array_equal(_bits(dist), _bits(E.reference_pairs(rows.cpu().numpy(), pairs)[0]))


def test_enrol_and_add_in_one_captured_graph():
    """matcher.embed into the gallery's rows and DeviceRoc.add captured in ONE graph, replayed twice on refilled int8 outputs: the
    histogram is the sum of the two references"""
    import torch
    D, B = 128, 150
    rng = np.random.default_rng(21)
    q = (-rng.integers(0, 8, D)).astype(np.int8)
    outs = [rng.integers(-128, 128, (B, D)).astype(np.int8) for _ in range(3)]
    _, ids = labelled_set(B, D, seed=22)
    m = _matcher(D, 1, q)
    gal = E.Gallery(B, D, DEV)
    gal.ids.copy_(_dev(ids))
    gal.count = B
    out_dev = _dev(outs[2])
    roc = E.DeviceRoc(400, 0.01, device=DEV)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        m.embed(out_dev, out=gal.rows)                    # warm-up
        roc.add(gal)
        torch.cuda.current_stream().synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            m.embed(out_dev, out=gal.rows)
            roc.add(gal)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    roc.reset()
    want = np.zeros((2, 401), np.int64)
    for k in (0, 1):
        with torch.cuda.stream(st):
            out_dev.copy_(torch.from_numpy(outs[k]))
            g.replay()
        want += E.reference_roc_hist(E.reference_embed(outs[k], q), ids)
    assert np.array_equal(_hist(roc)[0], want) and want.sum() > 0
