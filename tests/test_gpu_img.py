"""conv_img.hip on the GPU: ResNet-50's 7 x 7 x 512 3x3 rows (48, 51) computed from an LDS-resident whole-image tile, against the oracle
and against the library with the kernel off.  Whole-network runs at small batches are the smallest shapes that put exactly those rows
through the kernel: batch 1 = a lone one-image block per m-tile, 2 = one full block, 3 = a full block + a one-image tail, 5 = several
blocks + a tail."""
import os

import numpy as np
import pytest

from tf2_amd import config as cfg, network, synth
from tests.conftest import set_opts
from tests.test_gpu_parity import Rig, _torch

pytestmark = pytest.mark.gpu

IMG = "conv_img_kernel"
# form -> (options, Q values): the shipped Q file (rows 48 / 51 packed as one-window rows, FAST / SEMI requantisation) in flight and alone, generic
# requantisation, one Q value per tensor (one-window tiles everywhere), Q values spread over three exponents per tensor (two-window rows 48 / 51)
FORMS = {
    "inflight": (dict(img="1", img_min="1", alt_conc="1"), "shipped"),
    "alone": (dict(img="2", img_min="1", alt_conc="0"), "shipped"),
    "generic": (dict(img="1", img_min="1", alt_conc="1", nofast="1"), "shipped"),
    "onewindow": (dict(img="1", img_min="1", alt_conc="1"), "spread0"),
    "twowindow": (dict(img="1", img_min="1", alt_conc="1"), "spread2"),
}
WINDOWS = {"shipped": "one-window", "spread0": "one-window", "spread2": "two-window"}


@pytest.fixture(scope="module")
def r50(golden_dir):
    t = cfg.resnet50_tables()
    q = np.loadtxt(os.path.join(golden_dir, "resnet50_Q"), dtype=np.int32)
    return t, q, synth.synth_model(t, q, 0)


@pytest.fixture(scope="module")
def r50_synth_q(r50):
    t = r50[0]
    out = {"shipped": r50}
    for name, spread in (("spread0", 0), ("spread2", 2)):
        q = synth.synth_q_values(t, 0, spread=spread)
        out[name] = (t, q, synth.synth_model(t, q, 0))
    return out


_refs = {}


def _reference(rig, key, images):
    """every layer of the oracle on `images`, computed once per (Q values, input) and shared by the forms; never modified"""
    if key not in _refs:
        outs = rig.ref.run(images)
        _refs[key] = (outs, rig.ref.logits(outs))
    return _refs[key]


def _check_all_layers(rig, images, outs, want):
    B = images.shape[0]
    got = rig.run(images, keep_all=True)
    for L in rig.ref.plan:
        np.testing.assert_array_equal(rig.runner.read_layer(L.index, B), outs[L.index][:B], err_msg=f"batch {B}, layer {L.index}")
    np.testing.assert_array_equal(got, want[:B], err_msg=f"batch {B}, logits")


@pytest.mark.parametrize("form", list(FORMS))
def test_every_layer_against_the_oracle(form, r50_synth_q, monkeypatch):
    opts, qkind = FORMS[form]
    set_opts(monkeypatch, **opts)
    rig = Rig(*r50_synth_q[qkind], 0)
    conc = int(opts["alt_conc"])
    for b in (1, 2, 3, 5):
        mine = [r for r in rig.net.describe_launches(b, conc) if r["kernel"].startswith(IMG)]
        assert [r["layer"] for r in mine] == [48, 51], (form, b)
        assert all(WINDOWS[qkind] in r["kernel"] for r in mine), mine
    x = synth.synth_images(rig.t, 5, 48)
    outs, want = _reference(rig, ("float", qkind), x)
    for b in (1, 2, 3, 5):
        _check_all_layers(rig, x[:b], outs, want)
    x8 = synth.synth_images(rig.t, 2, 49, kind="int8")
    x8[0, :, 100:104, :] = -128                      # rows of -128 (the negate quirk of pe.cl:32-37)
    x8[1, 1, ::7, :] = -128
    outs8, want8 = _reference(rig, ("int8", qkind), x8)
    _check_all_layers(rig, x8, outs8, want8)


def test_logits_at_batch_33(r50, monkeypatch):
    """the liveness-planned workspace (tensors share memory): five repeated runs identical, three images against the oracle, every image
    against a second handle with the kernel off"""
    set_opts(monkeypatch, img="1", alt_conc="1")
    rig = Rig(*r50, 0)
    assert [r["layer"] for r in rig.net.describe_launches(33, 1) if r["kernel"].startswith(IMG)] == [48, 51]
    x = synth.synth_images(rig.t, 33, 51)
    runs = [rig.run(x, keep_all=False).copy() for _ in range(5)]
    for r in runs[1:]:
        np.testing.assert_array_equal(r, runs[0])
    sel = [0, 16, 32]                                # the first image, one of a middle block, the one-image tail block
    np.testing.assert_array_equal(runs[0][sel], rig.ref.logits(rig.ref.run(x[sel])))
    set_opts(monkeypatch, img="0")
    off = Rig(*r50, 0)
    assert not any(r["kernel"].startswith(IMG) for r in off.net.describe_launches(33, 1))
    np.testing.assert_array_equal(off.run(x, keep_all=False), runs[0])


def test_four_streams(r50, monkeypatch):
    """four Runners of one handle on four streams, batch 3 each, three rounds enqueued back to back with no synchronisation in between:
    every stream's logits equal the serial result (the short form of tests/test_gpu_configs.py's in-flight test)"""
    torch = _torch()
    set_opts(monkeypatch, img="1", img_min="1")
    rig = Rig(*r50, 0)
    assert [r["layer"] for r in rig.net.describe_launches(3, 1) if r["kernel"].startswith(IMG)] == [48, 51]
    xs = [synth.synth_images(rig.t, 3, 60 + i) for i in range(4)]
    xd = [torch.from_numpy(x).to("cuda:0") for x in xs]
    streams = [torch.cuda.Stream(device="cuda:0") for _ in range(4)]
    runners = [network.Runner(None, rig.net) for _ in range(4)]
    serial = []
    for x in xd:
        serial.append(rig.runner.run_batch(x, concurrency=1).cpu().numpy().copy())
    np.testing.assert_array_equal(serial[0], rig.ref.logits(rig.ref.run(xs[0])))
    torch.cuda.synchronize()
    for rnd in range(3):
        for i in range(4):
            with torch.cuda.stream(streams[i]):
                runners[i].run_batch(xd[(i + rnd) % 4], concurrency=1)
    torch.cuda.synchronize()
    for i in range(4):
        np.testing.assert_array_equal(runners[i]._logits.cpu().numpy(), serial[(i + 2) % 4], err_msg=f"stream {i}")


def test_graph_replay(r50, monkeypatch):
    """one captured graph of a batch-3 step replayed 20 times: identical logits every time, and the launched step's"""
    torch = _torch()
    set_opts(monkeypatch, img="1", img_min="1")
    rig = Rig(*r50, 0)
    x = synth.synth_images(rig.t, 3, 70)
    buf = torch.from_numpy(x).to("cuda:0")
    want = rig.runner.run_batch(buf, concurrency=1).cpu().numpy().copy()
    runner = network.Runner(None, rig.net)
    replay = runner.capture(buf, concurrency=1)
    for k in range(20):
        replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(runner._logits.cpu().numpy(), want, err_msg=f"replay {k}")
