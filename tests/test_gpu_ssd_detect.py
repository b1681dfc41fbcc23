"""On-device SSD detection on the MI355X (tf2_ssd_run / tf2_ssd_detect, ssd_detect.hip): the selection bit-identical to its host
statement ssd.detect_ordered, the head decode against a keep_all run taken through the host path (read_layer, gather_heads,
softmax, decode), graph replay and two streams side by side, and the ordinary / keep_all plans untouched by the new one."""
import numpy as np
import pytest

from tf2_amd import config as cfg, ssd, synth
from tf2_amd.network import NetWork, Runner

pytestmark = pytest.mark.gpu


def _q_rows(plan, q):
    """file-order Q values per table row (the qrows view of tests/test_ssd.py): {row: Q[N]} and {row: position in the file}"""
    rows, at, pos = {}, {}, 3
    for L in plan:
        if not L.ipool:
            rows[L.index] = q[pos:pos + L.N]; at[L.index] = pos; pos += L.N
        elif L.ipool == 2:
            pos += L.N
    return rows, at


def _ssd_net(width_div, seed=3, loc_q=6, conf_q=3):
    """SSD300 at `width_div` with head Qs that keep dequantised loc within +-2 (int8 / 2^6) and conf within +-16"""
    t = cfg.ssd300_tables(width_div=width_div)
    plan = cfg.build_plan(t)
    q = np.array(synth.synth_q_values(t, seed, spread=1))
    _, at = _q_rows(plan, q)
    for lr, cr in ssd.head_rows(plan):
        q[at[lr]:at[lr] + plan[lr].N] = loc_q
        q[at[cr]:at[cr] + plan[cr].N] = conf_q
    model = synth.synth_model(t, q, seed)
    net = NetWork(t)
    net.Init(model, synth.q_text(q), device="cuda:0")
    return t, q, net


@pytest.fixture(scope="module")
def small_net():
    return _ssd_net(4)


def _images(t, batch, seed):
    import torch
    return torch.from_numpy(np.ascontiguousarray(synth.synth_images(t, batch, seed))).to("cuda:0")


def _softmax_probs(rng, batch, classes, scale=1.0):
    import torch
    return torch.softmax(torch.from_numpy(rng.normal(0, scale, (batch, 8732, classes)).astype(np.float32)), -1)


def _decoded(rng, batch):
    import torch
    pri = ssd.prior_boxes(ssd.VOC)
    loc = torch.from_numpy(rng.normal(0, 1.0, (batch, 8732, 4)).astype(np.float32))
    return torch.stack([ssd.decode(loc[b], pri, ssd.VOC["variance"]) for b in range(batch)])


def _case(kind, batch, top_k, seed):
    import torch
    rng = np.random.default_rng(seed)
    boxes = _decoded(rng, batch)
    if kind == "random":                      # every prior passes 0.01 in most classes (21 classes of ~0.05)
        probs = _softmax_probs(rng, batch, 21)
    elif kind == "ties":                      # four score levels, duplicated boxes
        levels = np.float32([0.6, 0.3, 0.02, 0.005])
        probs = torch.from_numpy(levels[rng.integers(0, 4, (batch, 8732, 21))])
        dup = rng.choice(8732, 600, replace=False)
        boxes[:, dup[300:]] = boxes[:, dup[:300]]
    else:                                     # peaked: few candidates; class 3 none, class 4 exactly top_k, class 5 all 8732
        probs = _softmax_probs(rng, batch, 21, 4.0)
        probs[..., 3] = 0.001
        probs[..., 4] = 0.0
        for b in range(batch):
            probs[b, rng.choice(8732, top_k, replace=False), 4] = torch.from_numpy(rng.uniform(0.02, 0.9, top_k).astype(np.float32))
        probs[..., 5] = torch.from_numpy(rng.uniform(0.011, 0.99, (batch, 8732)).astype(np.float32))
    return boxes.contiguous(), probs.contiguous()


@pytest.mark.parametrize("kind,batch,top_k,nms", [
    ("random", 1, 200, 0.45), ("random", 5, 1, 0.45), ("random", 32, 200, 0.45), ("random", 5, 256, 0.45), ("random", 5, 200, 1.0),
    ("ties", 5, 200, 0.45), ("ties", 1, 256, 0.45), ("ties", 32, 1, 0.45), ("ties", 5, 200, 1.0),
    ("peaked", 5, 200, 0.45), ("peaked", 5, 256, 0.45), ("peaked", 32, 200, 0.45), ("peaked", 1, 1, 0.45),
])
def test_stage2_bit_identical_to_detect_ordered(small_net, kind, batch, top_k, nms):
    import torch
    t, q, net = small_net
    det = ssd.DeviceDetector(net, net.plan, ssd.VOC, top_k=top_k, conf_thresh=0.01, nms_thresh=nms)
    boxes, probs = _case(kind, batch, top_k, seed=batch * 7 + top_k)
    got, counts = det.detect(boxes, probs)
    torch.cuda.synchronize()
    want, want_counts = ssd.detect_ordered(boxes, probs, 21, top_k, 0.01, nms)
    np.testing.assert_array_equal(counts.cpu().numpy(), want_counts.numpy())
    np.testing.assert_array_equal(got.cpu().numpy(), want.numpy())
    if kind == "peaked":
        assert (want_counts[:, 3] == 0).all()
        assert (counts.cpu()[:, 5] > 0).all()


def _host_heads(net, t, q, x, batch):
    """heads of a keep_all run through the host path: read_layer, gather_heads, softmax, decode"""
    import torch
    r = Runner(None, net)
    r.run_batch(x, keep_all=True)
    torch.cuda.synchronize()
    qrows, _ = _q_rows(net.plan, q)
    loc, conf = ssd.gather_heads(lambda l: r.read_layer(l, batch), net.plan, qrows, batch, 21)
    pri = ssd.prior_boxes(ssd.VOC)
    boxes = torch.stack([ssd.decode(loc[b], pri, ssd.VOC["variance"]) for b in range(batch)])
    return loc, boxes, torch.softmax(conf, -1)


def _end_to_end(t, q, net, batch, seed):
    import torch
    x = _images(t, batch, seed)
    det = ssd.DeviceDetector(net, net.plan, ssd.VOC)
    logits = torch.empty(batch, net.plan[-1].N, dtype=torch.int8, device="cuda:0")
    d, c, boxes, probs = det.run(x, decoded=True, logits=logits)
    det.poll_error(batch)                     # (synchronises) the workspace's error word is where the outputs-kept plan put it
    loc, want_boxes, want_probs = _host_heads(net, t, q, x, batch)
    assert loc.abs().max() <= 2.0 and loc.abs().max() > 0.1
    # (a) decode and softmax: exact dequantisation; exp and the softmax sum may differ from torch by an ulp or two
    np.testing.assert_allclose(probs.cpu().numpy(), want_probs.numpy(), rtol=2e-6, atol=0)
    np.testing.assert_allclose(boxes.cpu().numpy(), want_boxes.numpy(), rtol=0, atol=2e-6)
    # (b) the selection on the run's own boxes / probabilities: bit-identical
    want_det, want_counts = ssd.detect_ordered(boxes.cpu(), probs.cpu(), 21, 200, 0.01, 0.45)
    np.testing.assert_array_equal(c.cpu().numpy(), want_counts.numpy())
    np.testing.assert_array_equal(d.cpu().numpy(), want_det.numpy())
    assert (want_counts[:, 1:] > 0).all()
    # (c) the network's logits are those of tf2_net_run
    plain = Runner(None, net).run_batch(x)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(logits.cpu().numpy(), plain.cpu().numpy().reshape(batch, -1))


@pytest.mark.parametrize("batch", [2, 5])
def test_end_to_end_quarter_width(small_net, batch):
    t, q, net = small_net
    _end_to_end(t, q, net, batch, seed=batch)


def test_end_to_end_full_width_batch32():
    t, q, net = _ssd_net(1, seed=5)
    _end_to_end(t, q, net, 32, seed=11)


def test_graph_replay_and_two_streams(small_net):
    import torch
    t, q, net = small_net
    det = ssd.DeviceDetector(net, net.plan, ssd.VOC)
    xa, xb = _images(t, 3, 21), _images(t, 3, 22)
    ref_a = [v.cpu() for v in det.run(xa, decoded=True)]
    ref_b = [v.cpu() for v in det.run(xb, decoded=True)]
    # capture one step on a static input, replay it on two fillings
    static = xa.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = det.run(static, decoded=True)
    torch.cuda.current_stream().wait_stream(side)
    for x, ref in ((xa, ref_a), (xb, ref_b), (xa, ref_a)):
        static.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(out, ref):
            assert torch.equal(got.cpu(), want)
    # two streams, two detectors (two workspaces), side by side
    det2 = ssd.DeviceDetector(net, net.plan, ssd.VOC)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream()); s2.wait_stream(torch.cuda.current_stream())
    outs = []
    for _ in range(3):
        oa = det.run(xa, stream=s1, decoded=True)
        ob = det2.run(xb, stream=s2, decoded=True)
        outs.append((oa, ob))
    torch.cuda.synchronize()
    for oa, ob in outs:
        for got, want in zip(oa, ref_a):
            assert torch.equal(got.cpu(), want)
        for got, want in zip(ob, ref_b):
            assert torch.equal(got.cpu(), want)


def _plans(net, batches):
    return [(b, k, net.workspace_size(b, k), net.describe_workspace(b, k)) for b in batches for k in (False, True)]


@pytest.mark.parametrize("which", ["ssd300", "resnet50"])
def test_ordinary_and_keep_all_plans_untouched(which):
    """The ordinary and keep_all plans of a handle that created a detector and ran the outputs-kept plan equal those of a handle
    that never did.  (ResNet-50 has no heads: its handle runs an SSD net's calls beside it, the plans are per handle.)"""
    import os
    import torch
    batches = (1, 2, 32)
    if which == "ssd300":
        t, q, a = _ssd_net(1, seed=5)
        _, _, b = _ssd_net(1, seed=5)
        before = _plans(a, batches)
        det = ssd.DeviceDetector(b, b.plan, ssd.VOC)
        for n in batches:
            assert det.workspace_size(n) > b.workspace_size(n, False)
        det.run(_images(t, 2, 1))
        torch.cuda.synchronize()
        assert _plans(b, batches) == before
    else:
        t = cfg.resnet50_tables()
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        qv = np.loadtxt(os.path.join(root, "tests", "golden", "resnet50_Q"), dtype=np.int32)
        model = synth.synth_model(t, qv, 0)
        a = NetWork(t); a.Init(model, synth.q_text(qv), device="cuda:0")
        before = _plans(a, batches)
        _, _, s = _ssd_net(4)
        det = ssd.DeviceDetector(s, s.plan, ssd.VOC)
        det.run(_images(cfg.ssd300_tables(width_div=4), 2, 1))
        Runner(None, a).run_batch(torch.from_numpy(synth.synth_images(t, 2, 0)).to("cuda:0"))
        torch.cuda.synchronize()
        assert _plans(a, batches) == before
