"""On-device SSD detection, CPU side: the host statement of the device's selection (ssd.detect_ordered / nms_ordered) against
ssd.detect and the reference's nms cases (tests/golden/ref_ssd.npz), its pinned tie order, the refusals of tf2_ssd_create and
the scratch-free ISA of ssd_detect.hip.  The device itself is checked in tests/test_gpu_ssd_detect.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tf2_amd import _lib, config as cfg, ssd, synth
from tf2_amd.network import NetWork

PRI = ssd.prior_boxes(ssd.VOC)
P = PRI.shape[0]


def _distinct_probs(rng, batch, classes):
    """[B, P, C] float32 with no two equal scores inside a class (a permutation of k / P): tie-free inputs."""
    out = np.empty((batch, P, classes), np.float32)
    for b in range(batch):
        for c in range(classes):
            out[b, :, c] = (rng.permutation(P) + 1) / P
    return torch.from_numpy(out)


def _boxes(rng, batch, scale=1.0):
    loc = torch.from_numpy(rng.normal(0, scale, (batch, P, 4)).astype(np.float32))
    return loc, torch.stack([ssd.decode(loc[b], PRI, ssd.VOC["variance"]) for b in range(batch)])


@pytest.mark.parametrize("top_k,conf,nms", [(200, 0.01, 0.45), (20, 0.5, 0.45), (5, 0.9, 0.3), (256, 0.0, 0.7), (1, 0.2, 0.45)])
def test_detect_ordered_equals_detect_on_tie_free_inputs(top_k, conf, nms):
    rng = np.random.default_rng(top_k)
    loc, boxes = _boxes(rng, 2)
    probs = _distinct_probs(rng, 2, 6)
    want = ssd.detect(loc, probs, PRI, 6, top_k=top_k, conf_thresh=conf, nms_thresh=nms)
    det, counts = ssd.detect_ordered(boxes, probs, 6, top_k, conf, nms)
    np.testing.assert_array_equal(det.numpy(), want.numpy())
    assert (counts.numpy() == (want[..., 0] > 0).sum(-1).numpy()).all()
    assert (counts[:, 0] == 0).all() and (counts[:, 1:] > 0).all()


def test_nms_ordered_keeps_the_reference_indices(golden_dir):
    G = np.load(os.path.join(golden_dir, "ref_ssd.npz"))
    for i in range(4):
        thr, topk = G[f"nms{i}_par"]
        keep = ssd.nms_ordered(G[f"nms{i}_boxes"], G[f"nms{i}_scores"], float(thr), int(topk))
        np.testing.assert_array_equal(keep.numpy(), G[f"nms{i}_keep"])


def _brute_force(boxes, scores, top_k, conf, nms):
    """The pinned order spelled out with Python's stable sort on (-score, index) and one IoU at a time."""
    cand = [i for i in range(len(scores)) if np.float32(scores[i]) > np.float32(conf)]
    order = sorted(cand, key=lambda i: (-np.float32(scores[i]), i))[:top_k]
    b = torch.as_tensor(boxes)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    kept = []
    for i in order:
        if all(bool(ssd._iou_one_to_many(b[k], area[k], b[i:i + 1], area[i:i + 1])[0] <= np.float32(nms)) for k in kept):
            kept.append(i)
    return kept


def test_tied_inputs_follow_the_stated_order():
    rng = np.random.default_rng(7)
    _, boxes = _boxes(rng, 1, 0.5)
    boxes = boxes.clone()
    # a few score levels; duplicated boxes (IoU 1) inside and across levels; 3 levels x many priors
    levels = np.float32([0.9, 0.5, 0.25, 0.05])
    probs = torch.zeros(1, P, 3)
    probs[0, :, 1] = torch.from_numpy(levels[rng.integers(0, 4, P)])
    probs[0, :, 2] = torch.from_numpy(levels[rng.integers(1, 3, P)])
    dup = rng.choice(P, 400, replace=False)
    boxes[0, dup[200:]] = boxes[0, dup[:200]]
    n_top = int((probs[0, :, 1] == levels[0]).sum())
    for top_k in (1, 7, 200, 256, n_top, n_top + 3):            # the cut inside a tie run, and at its edge
        for nms in (0.45, 1.0):
            det, counts = ssd.detect_ordered(boxes, probs, 3, top_k, 0.01, nms)
            for c in (1, 2):
                kept = _brute_force(boxes[0].numpy(), probs[0, :, c].numpy(), top_k, 0.01, nms)
                assert counts[0, c] == len(kept)
                np.testing.assert_array_equal(det[0, c, :len(kept), 1:].numpy(), boxes[0, kept].numpy())
                np.testing.assert_array_equal(det[0, c, :len(kept), 0].numpy(), probs[0, kept, c].numpy())
                assert (det[0, c, len(kept):] == 0).all()
    # all equal, disjoint boxes: the lowest indices win the cut
    grid = torch.tensor([[i, 0, i + 0.5, 0.5] for i in range(50)], dtype=torch.float32)
    keep = ssd.nms_ordered(grid, np.full(50, 0.3, np.float32), 0.45, 10)
    assert keep.tolist() == list(range(10))
    # duplicated boxes at one score: the lowest index survives, the copies are suppressed; nms_thresh 1.0 keeps them (IoU 1 <= 1)
    twin = torch.tensor([[0, 0, 1, 1]] * 4 + [[2, 2, 3, 3]], dtype=torch.float32)
    assert ssd.nms_ordered(twin, np.float32([0.5, 0.5, 0.5, 0.5, 0.5]), 0.45, 10).tolist() == [0, 4]
    assert ssd.nms_ordered(twin, np.float32([0.5, 0.5, 0.5, 0.5, 0.5]), 1.0, 10).tolist() == [0, 1, 2, 3, 4]


@pytest.fixture(scope="module")
def packed_ssd_net():
    t = cfg.ssd300_tables(width_div=16)
    q = synth.synth_q_values(t, 3, spread=1)
    net = NetWork(t)
    net.Quantization(synth.q_text(q))
    net.LoadModel(synth.synth_model(t, q, 3))
    net.Pack(0)
    return net


def _desc(plan, **kw):
    pri = np.ascontiguousarray(PRI.numpy())
    d = _lib.SsdDesc()
    d.size = C.sizeof(_lib.SsdDesc)
    d.num_classes, d.top_k, d.conf_thresh, d.nms_thresh = 21, 200, 0.01, 0.45
    d.variance[0], d.variance[1] = 0.1, 0.2
    rows = ssd.head_rows(plan)
    d.n_sources = len(rows)
    for i, (lr, cr) in enumerate(rows):
        d.loc_row[i], d.conf_row[i] = lr, cr
    d.priors, d.n_priors = pri.ctypes.data, P
    for k, v in kw.items():
        if k in ("loc_row", "conf_row"):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d, pri


@pytest.mark.parametrize("change,message", [
    (dict(num_classes=20), "conf row"),                                  # conf N != nb * num_classes
    (dict(loc_row=(0, 26)), "a head row is named twice"),
    (dict(loc_row=(2, 9)), "read by another row"),                       # conv4_3 feeds the L2Norm row and pool4
    (dict(n_priors=P - 1), "n_priors"),
    (dict(top_k=0), "top_k"), (dict(top_k=257), "top_k"),
    (dict(nms_thresh=0.0), "nms_thresh"), (dict(nms_thresh=-0.5), "nms_thresh"),
    (dict(num_classes=1), "num_classes"), (dict(num_classes=257), "num_classes"),
    (dict(n_sources=0), "n_sources"), (dict(n_sources=9), "n_sources"),
    (dict(conf_thresh=-0.1), "conf_thresh"),
    (dict(size=8), "desc"),
])
def test_create_refuses_malformed_descs(packed_ssd_net, change, message):
    net = packed_ssd_net
    d, _pri = _desc(net.plan, **change)
    h = C.c_void_p()
    st = _lib.lib().tf2_ssd_create(net._h, C.byref(d), C.byref(h))
    err = _lib.lib().tf2_last_error().decode()
    assert st == -1 and not h.value, (st, err)
    assert message in err, err


def test_create_refuses_rows_with_wrong_N(packed_ssd_net):
    """A loc row whose N is not 4 * boxes: source 0's conf row (84 channels = 4 * 21) named as loc makes nb = 21, so the conf
    check (N = 21 * 21) refuses; a conf row of the wrong width is refused by name."""
    net = packed_ssd_net
    plan = net.plan
    lr, cr = ssd.head_rows(plan)[0]
    assert plan[lr].N == 16 and plan[cr].N == 84
    d, _pri = _desc(plan, loc_row=(0, cr), conf_row=(0, lr))
    h = C.c_void_p()
    assert _lib.lib().tf2_ssd_create(net._h, C.byref(d), C.byref(h)) == -1
    assert "expected boxes * num_classes" in _lib.lib().tf2_last_error().decode()


def test_a_valid_desc_passes_the_host_checks(packed_ssd_net):
    net = packed_ssd_net
    d, _pri = _desc(net.plan)
    h = C.c_void_p()
    st = _lib.lib().tf2_ssd_create(net._h, C.byref(d), C.byref(h))
    assert st in (0, -4), _lib.lib().tf2_last_error()         # -4: no device to upload the constants to (a CPU-only host)
    if st == 0:
        _lib.lib().tf2_ssd_destroy(h)


def test_ssd_detect_kernels_compile_without_scratch():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import vmcnt_check
    seg, lds, txt = vmcnt_check.kernel_segments("ssd_detect")
    names = [k for k in seg if "ssd_" in k]
    assert {"heads", "select", "transpose"} <= {n.split("ssd_")[1].split("_kernel")[0] for n in names}, seg
    assert all(seg[k] == 0 for k in names), seg
    # the IoU division is the IEEE one (v_div_scale / v_div_fixup), not a bare reciprocal
    body = txt[txt.index("ssd_select_kernel"):]
    assert "v_div_fixup_f32" in body
