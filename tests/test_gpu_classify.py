"""Classification on the MI355X (tf2_cls_*, classify.hip): labels, features, ranks and tallies bit-identical to the statement
classify.reference over the input families and the (n, k) grid of tests/test_classify.py at batches 1..256, probabilities within a
bound derived from the kernel's own summation, run-to-run identity, ResNet-50 end to end against network.Evaluation, preprocess +
network + classifier in one captured graph with refilled pixels and labels (and a second stream side by side), and the CLI's
--device-eval against its default output."""
import os

import numpy as np
import pytest

from tf2_amd import _lib, classify as K, config as cfg, network, preprocess as P, synth
from tf2_amd.network import NetWork, Runner
from tests.test_classify import FAMILIES, GRID, family

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = [1, 7, 32, 65, 256]
_NETS = {}


def _classifier(n, k, q_last):
    """a classifier of a host-only net handle of n classes (cfg.tiny_tables: any n cheaply) whose last Q row is q_last: the
    classifier reads nothing else of the net, and the logits of these tests are written straight into a device buffer"""
    if n not in _NETS:
        t = cfg.tiny_tables(classes=n)
        net = NetWork(t)
        net.Quantization(synth.q_text(synth.synth_q_values(t, 1)))
        _NETS[n] = net
    net = _NETS[n]
    net.q[net.num_layer, :n] = q_last
    _lib.check(_lib.lib().tf2_net_set_q(net._h, net.q.ctypes.data, net.q.size))
    return K.DeviceClassifier(net, k)


def _truth(rng, ref_labels, n):
    """labels that hit every position of the top k in turn, miss, are unlabelled (-1, -9) and bad (n, n + 1000)"""
    B, k = ref_labels.shape
    t = np.empty(B, np.int32)
    for b in range(B):
        kind = b % (k + 5)
        t[b] = ref_labels[b, kind] if kind < k else (int(rng.integers(0, n)), -1, n, -9, n + 1000)[kind - k]
    return t


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("n,k", GRID)
def test_selection_bit_identical(kind, n, k):
    import torch
    total = np.zeros(4, np.uint64)
    cls = None
    for batch in BATCHES:
        lg, q = family(kind, n, batch, seed=2)
        cls = cls or _classifier(n, k, q)                # (the Q row of a family is the same at every batch)
        rng = np.random.default_rng([n, k, batch])
        truth = _truth(rng, K.reference(lg, q, k).labels, n)
        want = K.reference(lg, q, k, truth)
        got = cls.run(torch.from_numpy(lg).to("cuda:0"), torch.from_numpy(truth).to("cuda:0"))
        torch.cuda.synchronize()
        assert np.array_equal(got.labels.cpu().numpy(), want.labels), (batch, got.labels.cpu().numpy()[:2], want.labels[:2])
        assert np.array_equal(_bits(got.features.cpu().numpy()), _bits(want.features)), batch
        assert np.array_equal(got.rank.cpu().numpy(), want.rank), batch
        total += want.tally
        assert np.array_equal(got.tally.cpu().numpy().view(np.uint64), total), (batch, got.tally.cpu().numpy(), total)
        # without ground truth: the same labels, nothing counted
        plain = cls.run(torch.from_numpy(lg).to("cuda:0"))
        torch.cuda.synchronize()
        assert plain.rank is None and np.array_equal(plain.labels.cpu().numpy(), want.labels)
        assert np.array_equal(cls.tally.cpu().numpy().view(np.uint64), total)
    acc = cls.accuracy()
    assert acc["labelled"] == int(total[0]) and acc["bad"] == int(total[3]) and acc["top1"] == int(total[1]) / int(total[0])
    cls.reset()
    assert cls.accuracy() == dict(labelled=0, bad=0, top1=None, topk=None)


def summation_depth(n):
    """float32 additions on the longest path of classify_kernel's sum: a lane adds its ceil(n / 64) strided exponentials one after
    the other, then the 6-step butterfly over the 64 lanes"""
    return -(-n // 64) + 6


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("n,k", GRID)
def test_probabilities_within_the_derived_bound(kind, n, k):
    """probs and all_probs against the float64 statement (on the same float32 d): relative tolerance (A + 4) 2^-24, A =
    summation_depth(n) (each addition rounds once, relative 2^-24 of a partial sum of positive terms, at most A of them on any
    path), the 4 covering expf (1 ulp each in numerator and sum, ROCm's documented accuracy), the division and the final rounding
    (n = 1000: (16 + 6 + 4) 2^-24 = 1.55e-6).  Entries whose exact value is below 2^-100 get an absolute tolerance of 2^-100
    (float32 underflow).  Each row of all_probs adds up to 1 within n 2^-24."""
    import torch
    lg, q = family(kind, n, 32, seed=3)
    cls = _classifier(n, k, q)
    want = K.reference(lg, q, k)
    got = cls.run(torch.from_numpy(lg).to("cuda:0"), all_probs=True)
    again = cls.run(torch.from_numpy(lg).to("cuda:0"), all_probs=True)
    torch.cuda.synchronize()
    rtol = (summation_depth(n) + 4) * 2.0 ** -24
    tiny = 2.0 ** -100
    for g, w in ((got.probs.cpu().numpy().astype(np.float64), want.probs), (got.all_probs.cpu().numpy().astype(np.float64), want.all_probs)):
        big = w >= tiny
        rel = float((np.abs(g - w)[big] / w[big]).max())
        print(f"{kind} n={n} k={k}: max relative difference {rel:.3e} (bound {rtol:.3e}), entries below 2^-100: {int((~big).sum())}")
        assert rel <= rtol
        assert (np.abs(g - w)[~big] <= tiny).all()
    sums = got.all_probs.cpu().numpy().astype(np.float64).sum(axis=1)
    print(f"{kind} n={n}: row sums within {np.abs(sums - 1).max():.3e} of 1 (bound {n * 2.0 ** -24:.3e})")
    assert np.abs(sums - 1).max() <= n * 2.0 ** -24
    # probs are the all_probs entries of the labels, bit for bit; two runs give the same bits (fixed summation order)
    picked = np.take_along_axis(got.all_probs.cpu().numpy(), got.labels.cpu().numpy().astype(np.int64), axis=1)
    assert np.array_equal(_bits(picked), _bits(got.probs.cpu().numpy()))
    assert np.array_equal(_bits(again.probs.cpu().numpy()), _bits(got.probs.cpu().numpy()))
    assert np.array_equal(_bits(again.all_probs.cpu().numpy()), _bits(got.all_probs.cpu().numpy()))


def test_two_runs_bit_identical_at_batch_256():
    import torch
    lg, q = family("random", 1000, 256, seed=4)
    cls = _classifier(1000, 5, q)
    x = torch.from_numpy(lg).to("cuda:0")
    runs = [cls.run(x, all_probs=True) for _ in range(4)]
    torch.cuda.synchronize()
    for r in runs[1:]:
        assert torch.equal(r.probs.view(torch.int32), runs[0].probs.view(torch.int32))
        assert torch.equal(r.all_probs.view(torch.int32), runs[0].all_probs.view(torch.int32))


def test_run_refusals_on_a_real_handle():
    import torch
    lg, q = family("random", 10, 2, seed=5)
    cls = _classifier(10, 5, q)
    x = torch.from_numpy(lg).to("cuda:0")
    lab = torch.empty(2, 5, dtype=torch.int32, device="cuda:0")
    L = _lib.lib()
    for batch, ptrs, message in ((0, (x.data_ptr(), lab.data_ptr()), "batch"), (2, (None, lab.data_ptr()), "null logits_dev"),
                                 (2, (x.data_ptr(), None), "null logits_dev / labels_dev")):
        st = L.tf2_cls_run(cls._h, ptrs[0], batch, ptrs[1], None, None, None, None, None, None, None)
        assert st == -1 and message in L.tf2_last_error().decode()
    # labels alone: every other output is optional
    assert L.tf2_cls_run(cls._h, x.data_ptr(), 2, lab.data_ptr(), None, None, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(lab.cpu().numpy(), K.reference(lg, q, 5).labels)


def _r50():
    t = cfg.resnet50_tables()
    qv = np.loadtxt(os.path.join(ROOT, "tests", "golden", "resnet50_Q"), dtype=np.int32)
    model = synth.synth_model(t, qv, 0)
    net = NetWork(t)
    net.Init(model, synth.q_text(qv), device="cuda:0")
    return t, qv, model, net


def test_resnet50_end_to_end_batch32():
    """run_batch then the classifier on its logits tensor: the labels of network.Evaluation for every image (the oracle pins the
    logits elsewhere; this pins the hand-over), everything else bit-identical to the statement"""
    import torch
    t, qv, model, net = _r50()
    x = torch.from_numpy(np.ascontiguousarray(synth.synth_images(t, 32, 9))).to("cuda:0")
    logits = Runner(None, net).run_batch(x)
    cls = K.DeviceClassifier(net, 5)
    got = cls.run(logits)
    torch.cuda.synchronize()
    out = logits.cpu().numpy()
    assert out.shape == (32, 1000) and len(np.unique(out)) > 20
    for b in range(32):
        labels, probs = network.Evaluation(b, net.q, out, num_layer=net.num_layer)
        assert got.labels[b].cpu().tolist() == labels
        # Evaluation against the exact value: the CPU test's bound (sh = 2: |d| <= 64); the device against it: the kernel's bound
        np.testing.assert_allclose(got.probs[b].cpu().numpy(), probs, rtol=((1000 + 4 + 2 * 64) + (summation_depth(1000) + 4)) * 2.0 ** -24)
    want = cls.reference(logits)
    assert np.array_equal(got.labels.cpu().numpy(), want.labels) and np.array_equal(_bits(got.features.cpu().numpy()), _bits(want.features))


def test_one_graph_pixels_to_tallies_and_two_streams():
    """Preprocessor -> run_batch -> DeviceClassifier.run captured in ONE graph; pixels and labels refilled between three replays;
    the tally on the device after the three replays is the sum of three host tallies.  Then a second stream with its own
    workspace, classifier and outputs side by side with the first."""
    import torch
    t = cfg.tiny_tables(hw=224)
    q = synth.synth_q_values(t, 2, spread=2)
    net = NetWork(t)
    net.Init(synth.synth_model(t, q, 2), synth.q_text(q), device="cuda:0")
    pp = P.Preprocessor(net, P.TORCHVISION, "RGB")
    rng = np.random.default_rng(6)
    B, k, n = 8, 3, net.plan[-1].N
    sets = [[rng.integers(0, 256, (int(rng.integers(100, 600)), int(rng.integers(100, 600)), 3), dtype=np.uint8) for _ in range(B)]
            for _ in range(3)]
    runner, cls = Runner(None, net), K.DeviceClassifier(net, k)

    def eager(imgs, rn, c, truth=None):
        px, sr = P.pack(imgs, P.TORCHVISION, "cuda:0")
        logits = rn.run_batch(pp(px, sr, out="q")[0]).clone()
        return logits, c.run(logits, truth)
    refs = []
    for i, s in enumerate(sets):
        logits, r = eager(s, runner, cls)
        torch.cuda.synchronize()
        labels = r.labels.cpu().numpy()
        truth = np.array([labels[b, (b + i) % (k + 1)] if (b + i) % (k + 1) < k else (-1, n, (int(labels[b, 0]) + 1) % n)[(b + i) % 3]
                          for b in range(B)], np.int32)
        want = K.reference(logits.cpu().numpy(), net.q[net.num_layer], k, truth)
        assert np.array_equal(want.labels, labels)
        refs.append((truth, want))
    assert sum(int(w.tally[1]) for _, w in refs) > 0 and sum(int(w.tally[2] - w.tally[1]) for _, w in refs) > 0
    cap = max(P.pack_host(s, P.TORCHVISION)[0].size for s in sets)
    pixels = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    srcs = torch.zeros(B, P.SRC_WORDS, dtype=torch.int32, device="cuda:0")
    truth_dev = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
    P.pack(sets[0], P.TORCHVISION, "cuda:0", pixels=pixels, srcs=srcs)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cls.run(runner.run_batch(pp(pixels, srcs, out="q")[0]), truth_dev)       # warm the launch plan and the tally buffer (all unlabelled)
        torch.cuda.current_stream().synchronize()
        with torch.cuda.graph(g, stream=side):
            out = cls.run(runner.run_batch(pp(pixels, srcs, out="q")[0]), truth_dev, all_probs=True)
    torch.cuda.current_stream().wait_stream(side)
    cls.reset()
    total = np.zeros(4, np.uint64)
    for i in (0, 1, 2):
        truth, want = refs[i]
        P.pack(sets[i], P.TORCHVISION, "cuda:0", pixels=pixels, srcs=srcs)
        truth_dev.copy_(torch.from_numpy(truth))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.labels.cpu().numpy(), want.labels) and np.array_equal(out.rank.cpu().numpy(), want.rank)
        assert np.array_equal(_bits(out.features.cpu().numpy()), _bits(want.features))
        total += want.tally
    assert np.array_equal(cls.tally.cpu().numpy().view(np.uint64), total), (cls.tally.cpu().numpy(), total)
    acc = cls.accuracy()
    assert acc["labelled"] == int(total[0]) and acc["topk"] == int(total[2]) / int(total[0])
    # two streams, their own runners (workspaces), classifiers and outputs, side by side
    runner2, cls2 = Runner(None, net), K.DeviceClassifier(net, k)
    cls.reset()
    ins = [P.pack(s, P.TORCHVISION, "cuda:0") for s in sets[:2]]
    tr = [torch.from_numpy(refs[i][0]).to("cuda:0") for i in range(2)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream()); s2.wait_stream(torch.cuda.current_stream())
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            a = cls.run(runner.run_batch(pp(*ins[0], out="q", stream=s1)[0]), tr[0], stream=s1)
        with torch.cuda.stream(s2):
            b = cls2.run(runner2.run_batch(pp(*ins[1], out="q", stream=s2)[0]), tr[1], stream=s2)
        outs.append((a, b))
    torch.cuda.synchronize()
    for pair in outs:
        for r, (truth, want) in zip(pair, refs[:2]):
            assert np.array_equal(r.labels.cpu().numpy(), want.labels) and np.array_equal(r.rank.cpu().numpy(), want.rank)
            assert np.array_equal(_bits(r.features.cpu().numpy()), _bits(want.features))
    assert np.array_equal(cls.tally.cpu().numpy().view(np.uint64), 3 * refs[0][1].tally)
    assert np.array_equal(cls2.tally.cpu().numpy().view(np.uint64), 3 * refs[1][1].tally)


def test_cli_device_eval_prints_the_default_lines(golden_dir, tmp_path, capsys):
    """--device-eval: the ranks and labels of the default output for the shipped test image (synthetic weights), and probabilities
    that, parsed back from the six printed decimals, differ by at most 2e-6 (one unit of the printed precision for each side's
    rounding)"""
    from tf2_amd import cli
    t = cfg.resnet50_tables()
    q = np.loadtxt(os.path.join(golden_dir, "resnet50_Q"), dtype=np.int32)
    mf = tmp_path / "param.bin"
    np.asarray(synth.synth_model(t, q, 0), np.float32).tofile(mf)
    args = [str(mf), os.path.join(golden_dir, "resnet50_Q"), os.path.join(golden_dir, "resnet50_data_label_100.bin"),
            os.path.join(golden_dir, "resnet50_fc1000_label_100.bin"), "2"]

    def lines(extra):
        assert cli.main(args + extra) == 0
        rows = [l for l in capsys.readouterr().out.splitlines() if l.startswith("rank=")]
        return [(int(l.split("rank=")[1].split()[0]), int(l.split("label=")[1].split()[0]), float(l.split("probability=")[1])) for l in rows]
    host, dev = lines([]), lines(["--device-eval"])
    assert len(host) == 10 and [r[:2] for r in host] == [r[:2] for r in dev]
    assert all(np.isfinite(r[2]) for r in host + dev)
    units = max(abs(round(a[2] * 1e6) - round(b[2] * 1e6)) for a, b in zip(host, dev))        # (in units of the last printed decimal: exact)
    print(f"largest difference of the printed probabilities: {units} x 1e-6")
    assert units <= 2
