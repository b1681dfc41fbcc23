"""Face matching on the MI355X (tf2_emb_*, embed_match.hip): embeddings, rows, distances, ids and tallies bit-identical to the
statement (embed.reference_embed / reference_match / reference_tally) over the input families of tests/test_embed.py, at every
D, k, batch and gallery size where the kernels take another path (the scalar and the 16-byte staging, one query group and several,
fewer rows than a slab, whole slabs, a ragged last slab, fewer rows than k), run-to-run identity, the refusals on a real handle,
SqueezeNet 1.1 end to end with enrolment, and preprocess + network + match captured in one graph a stream, two streams adding to
one tally."""
import numpy as np
import pytest

from tf2_amd import _lib, config as cfg, embed as E, preprocess as P, synth
from tf2_amd.network import NetWork, Runner
from tests.test_embed import FAMILIES, TIE_FAMILIES, family

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = E.SLAB
# (batch, gallery rows): every batch of {1, 7, 32, 65} and every N of {1, 3, 63, 64, 65, one slab - 1, one slab, one slab + 1, five slabs
# and a ragged tail, ~5 000} at least once
SHAPES = [(1, 1), (7, 3), (32, 63), (65, 64), (7, 65), (32, S - 1), (1, S), (65, S + 1), (65, 5 * S + 37), (1, 5 * S + 37), (32, 4999)]
_NETS = {}


def _matcher(D, k, q_last):
    """a matcher of a host-only net handle with a D-channel output (cfg.tiny_tables: any D cheaply) whose last Q row is q_last: the
    matcher reads nothing else of the net, and the int8 outputs of these tests are written straight into a device buffer"""
    if D not in _NETS:
        t = cfg.tiny_tables(classes=D)
        net = NetWork(t)
        net.Quantization(synth.q_text(synth.synth_q_values(t, 1)))
        _NETS[D] = net
    net = _NETS[D]
    net.q[net.num_layer, :D] = q_last
    _lib.check(_lib.lib().tf2_net_set_q(net._h, net.q.ctypes.data, net.q.size))
    return E.DeviceMatcher(net, k)


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return np.ascontiguousarray(a).view(np.uint32)


def _truth(ids_ref, B, k):
    """labels that are the first id, the last of the k, an impostor (no id is below 100), unlabelled (-1, -9) in turn"""
    t = np.empty(B, np.int32)
    for b in range(B):
        t[b] = (ids_ref[b, 0], ids_ref[b, k - 1], 5, -1, ids_ref[b, k // 2], -9, 99)[b % 7]
    return t


def _threshold(dist):
    """the median of the nearest distances: about half the queries accepted, and at an odd batch one of them sits exactly on it"""
    d0 = np.sort(dist[:, 0])
    m = float(d0[len(d0) // 2])
    return m if np.isfinite(m) else 0.5


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, want_idx, want_dist, want_ids, want_e, where):
    assert np.array_equal(got.idx.cpu().numpy(), want_idx), (where, got.idx.cpu().numpy()[:2], want_idx[:2])
    assert np.array_equal(_bits(got.dist), _bits(want_dist)), where
    assert np.array_equal(got.ids.cpu().numpy(), want_ids), where
    assert np.array_equal(_bits(got.embeddings), _bits(want_e)), where


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("D", [2, 5, 128, 512])
def test_bit_identical(kind, D, k):
    import torch
    total = np.zeros(5, np.uint64)
    m = None
    tied = False
    for B, N in SHAPES:
        out, q, g, ids = family(kind, D, B, N, k, seed=3)
        m = m or _matcher(D, k, q)                        # (the Q row of a family is the same at every shape)
        e = E.reference_embed(out, q)
        idx, dist, rid = E.reference_match(e, g, ids, k)
        if kind in TIE_FAMILIES and N >= k + 2:           # the tie rule is exercised: rank k and rank k + 1 at one distance
            wider = E.reference_match(e, g, ids, k + 1)[1]
            assert (wider[:, k - 1] == wider[:, k]).any(), (B, N)
            tied = True
        truth, thr = _truth(rid, B, k), _threshold(dist)
        want_tally = E.reference_tally(idx, dist, rid, truth, thr)
        o, gd, idd, td = _dev(out), _dev(g), _dev(ids), _dev(truth)
        got = m.match(o, gd, idd, threshold=thr, truth=td)
        torch.cuda.synchronize()
        _same(got, idx, dist, rid, e, (B, N))
        total += want_tally
        assert np.array_equal(m.tally.cpu().numpy().view(np.uint64), total), ((B, N), m.tally.cpu().numpy(), total)
        # without ids and truth: the id is the row, nothing is counted; the embed call alone writes the same rows
        plain = m.match(o, gd)
        alone = m.embed(o)
        torch.cuda.synchronize()
        _same(plain, idx, dist, idx, e, (B, N))
        assert np.array_equal(_bits(alone), _bits(e))
        assert np.array_equal(m.tally.cpu().numpy().view(np.uint64), total)
    assert tied or kind not in TIE_FAMILIES
    assert m.accuracy() == dict(zip(E.TALLY, (int(v) for v in total)))
    m.reset()
    assert m.accuracy() == dict.fromkeys(E.TALLY, 0)


@pytest.mark.parametrize("D", [36, 100])
def test_16_byte_staging_with_a_short_last_chunk(D):
    """D a multiple of 4 but not of the 32 columns staged at a time: the 16-byte staging with a last chunk of 4 columns"""
    import torch
    k = 5
    m = None
    for B, N in ((7, S - 1), (32, 5 * S + 37)):
        out, q, g, ids = family("dup_across", D, B, N, k, seed=9)
        m = m or _matcher(D, k, q)
        gd = _dev(g)
        assert gd.data_ptr() % 16 == 0
        e = E.reference_embed(out, q)
        got = m.match(_dev(out), gd, _dev(ids))
        torch.cuda.synchronize()
        _same(got, *E.reference_match(e, g, ids, k), e, (D, B, N))


def test_unaligned_gallery_nan_rows_and_a_search_of_the_first_n():
    """a gallery that starts 4 bytes past a 16-byte boundary (D = 128 on the scalar staging), rows holding NaN and inf (+inf
    distances, ordered by row), and n below the rows of the buffer"""
    import torch
    D, k, B, N = 128, 5, 7, 3 * S + 5
    out, q, g, ids = family("random", D, B, N, k, seed=4)
    g = g.copy()
    g[3, 7], g[S, 0], g[N - 1, D - 1] = np.nan, np.inf, np.nan
    m = _matcher(D, k, q)
    buf = torch.zeros(N * D + 1, dtype=torch.float32, device=DEV)
    gd = buf[1:].view(N, D)
    gd.copy_(_dev(g))
    assert gd.data_ptr() % 16 == 4
    e = E.reference_embed(out, q)
    for n in (N, S + 1, 4):
        idx, dist, rid = E.reference_match(e, g[:n], ids[:n], k)
        got = m.match(_dev(out), gd, _dev(ids), n=n)
        torch.cuda.synchronize()
        _same(got, idx, dist, rid, e, n)
    # k = 16 over all the rows of a small gallery: the NaN and the inf rows come last, by row, as +inf
    m16 = _matcher(D, 16, q)
    idx, dist, rid = E.reference_match(e, g[:10], None, 16)
    assert idx[0, 9] == 3 and np.isposinf(dist[0, 9]) and idx[0, 10] == -1
    got = m16.match(_dev(out), gd, None, n=10)
    torch.cuda.synchronize()
    _same(got, idx, dist, rid, e, "k16")


def test_two_runs_bit_identical_at_batch_256():
    import torch
    D, k, B, N = 128, 5, 256, 4999
    out, q, g, ids = family("dup_across", D, B, N, k, seed=5)
    m = _matcher(D, k, q)
    o, gd, idd = _dev(out), _dev(g), _dev(ids)
    runs = [m.match(o, gd, idd) for _ in range(2)]
    torch.cuda.synchronize()
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    e = E.reference_embed(out, q)
    _same(runs[0], *E.reference_match(e, g, ids, k), e, "batch 256")


def test_refusals_on_a_real_handle():
    import torch
    D, k, B, N = 10, 5, 2, 70
    out, q, g, ids = family("random", D, B, N, k, seed=6)
    m = _matcher(D, k, q)
    o, gd = _dev(out), _dev(g)
    need = m.scratch_size(B, N)
    assert need == D * E.GROUP * 4 + B * 2 * k * 8 and m.scratch_size(0, N) == 0 and m.scratch_size(B, 0) == 0
    scratch = torch.zeros(need // 8 + 1, dtype=torch.int64, device=DEV)
    idx = torch.full((B, k), -7, dtype=torch.int32, device=DEV)
    dist = torch.zeros(B, k, dtype=torch.float32, device=DEV)
    L = _lib.lib()

    def call(batch=B, n=N, thr=1.0, o_=o.data_ptr(), g_=gd.data_ptr(), s_=scratch.data_ptr(), nbytes=need, i_=idx.data_ptr(), d_=dist.data_ptr()):
        st = L.tf2_emb_match(m._h, o_, batch, g_, None, n, thr, s_, nbytes, i_, d_, None, None, None, None, None)
        return st, L.tf2_last_error().decode()
    for kw, status, message in ((dict(batch=0), -1, "batch"), (dict(n=0), -1, "n_rows"), (dict(o_=None), -1, "null out_i8_dev"),
                                (dict(g_=None), -1, "gallery_dev"), (dict(s_=None), -1, "null scratch_dev"), (dict(i_=None), -1, "idx_dev"),
                                (dict(d_=None), -1, "dist_dev"), (dict(thr=float("nan")), -1, "NaN"), (dict(nbytes=need - 1), -3, "scratch_bytes"),
                                (dict(s_=scratch.data_ptr() + 4), -1, "8-byte aligned")):
        st, err = call(**kw)
        assert st == status and message in err, (kw, st, err)
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == -7).all()                # a refusal enqueues nothing
    assert L.tf2_emb_embed(m._h, None, B, gd.data_ptr(), None) == -1 and "null out_i8_dev / rows_dev" in L.tf2_last_error().decode()
    # the required outputs alone: every other pointer is optional
    st, err = call()
    assert st == 0, err
    torch.cuda.synchronize()
    want = E.reference_match(E.reference_embed(out, q), g, None, k)
    assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(_bits(dist), _bits(want[1]))


def test_squeezenet_end_to_end_batch32():
    """raw pixels -> preprocess.SQUEEZENET -> SqueezeNet 1.1 (synthetic weights) -> enrol the first 16 images -> match all 32:
    everything equals the statement applied to the network's own int8 outputs, and an enrolled image finds its own row at 0.0"""
    import torch
    t = cfg.squeezenet11_tables()
    q = synth.synth_q_values(t, 21, spread=2)
    net = NetWork(t)
    net.Init(synth.synth_model(t, q, 21), synth.q_text(q), device=DEV)
    rng = np.random.default_rng(7)
    imgs = [rng.integers(0, 256, (227, 227, 3), dtype=np.uint8) for _ in range(32)]
    px, sr = P.pack(imgs, P.SQUEEZENET, DEV)
    outputs = Runner(None, net).run_batch(P.Preprocessor(net, P.SQUEEZENET, "RGB")(px, sr, out="q")[0]).clone()
    m = E.DeviceMatcher(net, 5)
    assert m.D == 128
    gal = E.Gallery(64, 128, DEV)
    names = np.arange(500, 516, dtype=np.int32)
    gal.enrol(m, outputs[:16], names)
    assert gal.count == 16
    truth = np.concatenate([names, np.full(8, 7, np.int32), np.full(8, -1, np.int32)])      # enrolled, impostors, unlabelled
    got = m.match(outputs, gal, threshold=0.5, truth=_dev(truth))
    torch.cuda.synchronize()
    out = outputs.cpu().numpy()
    assert out.shape == (32, 128) and len(np.unique(out)) > 4
    e = E.reference_embed(out, net.q[net.num_layer])
    assert np.array_equal(_bits(gal.rows[:16]), _bits(e[:16])) and (gal.ids.cpu().numpy()[:16] == names).all()
    idx, dist, rid = E.reference_match(e, e[:16], names, 5)
    _same(got, idx, dist, rid, e, "squeezenet")
    d0 = got.dist.cpu().numpy()[:16, 0]
    assert (d0 == 0.0).all() and (e[got.idx.cpu().numpy()[:16, 0]] == e[:16]).all()
    assert np.array_equal(m.tally.cpu().numpy().view(np.uint64), E.reference_tally(idx, dist, rid, truth, 0.5))
    ref, tally = m.reference(outputs, gal, threshold=0.5, truth=truth)
    assert np.array_equal(ref.idx, idx) and np.array_equal(tally, E.reference_tally(idx, dist, rid, truth, 0.5))
    assert m.accuracy()["labelled"] == 24 and m.accuracy()["false_accepts"] == int(tally[4])


def test_one_graph_a_stream_two_streams_one_tally():
    """Preprocessor -> run_batch -> DeviceMatcher.match with truth captured in ONE graph per stream; the two graphs are replayed side
    by side three times with refilled labels and add to ONE tally, which then equals the sum of the host tallies of all six batches"""
    import torch
    t = cfg.tiny_tables(hw=224)
    q = synth.synth_q_values(t, 2, spread=2)
    net = NetWork(t)
    net.Init(synth.synth_model(t, q, 2), synth.q_text(q), device=DEV)
    pp = P.Preprocessor(net, P.TORCHVISION, "RGB")
    rng = np.random.default_rng(8)
    B, k, D = 8, 3, net.plan[-1].N
    sets = [[rng.integers(0, 256, (int(rng.integers(100, 600)), int(rng.integers(100, 600)), 3), dtype=np.uint8) for _ in range(B)]
            for _ in range(3)]
    m = E.DeviceMatcher(net, k)
    runners = [Runner(None, net), Runner(None, net)]
    # the gallery: set 2 enrolled whole, then the first half of set 0 (n = 12 rows, fixed before the capture)
    gal = E.Gallery(16, D, DEV)
    outs = []
    for s in sets:
        px, sr = P.pack(s, P.TORCHVISION, DEV)
        outs.append(runners[0].run_batch(pp(px, sr, out="q")[0]).clone())
    gal.enrol(m, outs[2], np.arange(8, dtype=np.int32) // 2 + 40)
    gal.enrol(m, outs[0][:4].contiguous(), np.int32([50, 50, 51, 51]))
    torch.cuda.synchronize()
    thr = 0.05
    refs = [m.reference(outs[i], gal, threshold=thr)[0] for i in (0, 1)]
    truths = [[np.array([(r.ids[b, 0], r.ids[b, k - 1], 3, -1)[(b + rnd) % 4] for b in range(B)], np.int32) for rnd in range(3)] for r in refs]
    want = sum(E.reference_tally(refs[i].idx, refs[i].dist, refs[i].ids, truths[i][rnd], thr) for i in (0, 1) for rnd in range(3))
    assert want[0] == 6 * 6 and want[1] > 0 and want[2] > want[1]

    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    ins = [P.pack(sets[i], P.TORCHVISION, DEV) for i in (0, 1)]
    truth_dev = [torch.full((B,), -1, dtype=torch.int32, device=DEV) for _ in (0, 1)]
    graphs, results = [], []
    for i in (0, 1):
        streams[i].wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(streams[i]):
            m.match(runners[i].run_batch(pp(*ins[i], out="q")[0]), gal, threshold=thr, truth=truth_dev[i])   # warm-up, all unlabelled
            torch.cuda.current_stream().synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=streams[i]):
                results.append(m.match(runners[i].run_batch(pp(*ins[i], out="q")[0]), gal, threshold=thr, truth=truth_dev[i]))
        torch.cuda.current_stream().wait_stream(streams[i])
        graphs.append(g)
    torch.cuda.synchronize()
    m.reset()
    torch.cuda.synchronize()
    for rnd in range(3):
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                truth_dev[i].copy_(torch.from_numpy(truths[i][rnd]))
                graphs[i].replay()
    torch.cuda.synchronize()
    for i in (0, 1):
        _same(results[i], refs[i].idx, refs[i].dist, refs[i].ids, refs[i].embeddings, f"stream {i}")
    assert np.array_equal(m.tally.cpu().numpy().view(np.uint64), want), (m.tally.cpu().numpy(), want)
    assert (results[0].dist.cpu().numpy()[:4, 0] == 0.0).all()            # the enrolled half of set 0 finds itself
