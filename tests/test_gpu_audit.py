"""Activation audit on the device (tf2_audit_*, csrc/act_audit.hip): the store of audit.DeviceAuditor equals audit.reference_audit of
the oracle's maps (netref.RefNet.run) and of Runner.read_layer after a separate keep_all run on the same images -- as integers, one
assertion over the whole store.  The regimes come from tests/test_audit.py, which shows on the oracle that they reach the rails (or
stay clear of them)."""
import os

import numpy as np
import pytest

from oracle import netref
from tf2_amd import _lib, audit as A, config as cfg, network, synth
from tests.test_audit import case_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).to(DEV)


class Rig:
    def __init__(self, t, q, model, batch):
        self.t, self.batch = t, batch
        self.net = network.NetWork(t)
        self.net.Init(model, synth.q_text(q), device=DEV)
        self.ref = netref.RefNet(t, q, model)
        self.aud = A.DeviceAuditor(self.net, batch)
        self.runner = network.Runner(None, self.net)

    def images_q(self, x):
        return x if x.dtype == np.int8 else A.reference_input_quant(x, int(self.net.q[0, 0]))

    def oracle(self, x):
        return A.reference_audit(self.ref.run(x), self.images_q(x))

    def check(self, x, oracle=True):
        """one observed batch on an empty store against both statements; returns (store, rows)"""
        torch = _torch()
        B = x.shape[0]
        xd = _dev(x)
        self.aud.reset()
        logits = self.aud.observe(xd).cpu().numpy()
        got = self.aud.store()
        plain = self.runner.run_batch(xd, keep_all=True).cpu().numpy()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(logits, plain, err_msg="logits of tf2_audit_run against Runner.run_batch")
        maps = [self.runner.read_layer(l, B) for l in range(self.net.num_layer)]
        np.testing.assert_array_equal(got, A.reference_audit(maps, self.images_q(x)), err_msg="device store against read_layer")
        if oracle:
            np.testing.assert_array_equal(got, self.oracle(x), err_msg="device store against the oracle")
        rows = self.aud.rows()
        assert got.shape[0] * 128 == self.aud.store_size and (got[:, 8:].sum(1) == got[:, 0] - got[:, 2]).all()
        return got, rows


# ---- 6. the small programs: every channel width, both rails, concat slices, both image types -----------------------------------------
@pytest.mark.parametrize("case,batch", [("tiny_benign", 3), ("tiny_saturate", 3), ("tiny_benign", 1), ("tiny_saturate", 1),
                                        ("fire_float", 3), ("fire_int8", 3)])
def test_small_programs(case, batch):
    t, q, model, x = case_inputs(case, batch)
    rig = Rig(t, q, model, batch)
    got, rows = rig.check(x)
    s = A.summary(got, rows)
    if case == "tiny_saturate":
        assert all(s[l]["hi_rail"].sum() > 0 for l in s) and s[1]["lo_rail"].sum() > 0 and s[8]["lo_rail"].sum() > 0
    if case.startswith("tiny"):
        assert sorted({r["C"] for r in rows}) == [3, 10, 16, 32]
        assert rows[-2]["H"] == 1 and s[rig.net.num_layer - 2]["n"][0] == batch          # the end-pool row: one value an image
    if case.startswith("fire"):
        ws = rig.net.describe_workspace(batch, True)[1]
        assert any(L.concat >= 0 and L.n_start > 0 for L in rig.ref.plan)                # a slice with out_off != 0
        assert "im2col" in rig.net.describe_launches(batch, 0)[0]["kernel"]              # the input tensor is not the image
        assert len(ws) == rig.net.num_layer


def test_more_rows_than_one_launch_takes():
    """70 store rows: tf2_audit_run deals them to two launches of the rows kernel (64 and 5 table rows)"""
    t, q, model, x = case_inputs("long", 2)
    got, rows = Rig(t, q, model, 2).check(x)
    assert len(rows) == 70 > A.ROWS_PER_LAUNCH
    assert got.shape[0] == 813 and (got[:, A.N] > 0).all()


# ---- 7. SSD: L2Norm row, independent pooling row, dilated row, heads with C = 4 nb and 21 nb -----------------------------------------
def test_ssd_program():
    t = cfg.ssd300_tables(width_div=4)
    q = synth.synth_q_values(t, 3, spread=1)
    rig = Rig(t, q, synth.synth_model(t, q, 3), 2)
    got, rows = rig.check(synth.synth_images(t, 2, 3))
    plan = rig.ref.plan
    assert any(L.ipool == 2 for L in plan) and any(L.ipool == 1 for L in plan) and any(L.dil > 1 for L in plan)
    assert {16, 24, 84, 126} <= {r["C"] for r in rows}


# ---- 8. ResNet-50: C up to 2048, the x-only stem input, the doubled form ---------------------------------------------------------------
@pytest.fixture(scope="module")
def r50_rig(golden_dir):
    t = cfg.resnet50_tables()
    q = np.loadtxt(os.path.join(golden_dir, "resnet50_Q"), dtype=np.int32)
    return Rig(t, q, synth.synth_model(t, q, 0), 2)


def test_resnet50_batch2(r50_rig):
    x = synth.synth_images(r50_rig.t, 2, 0)
    got, rows = r50_rig.check(x)
    assert sum(r["n_doubled"] for r in rows) > 0                                          # the 2y - 128 form is really met
    assert max(r["C"] for r in rows) == 2048 and rows[0] == dict(layer=-1, C=3, H=224, W=224, offset=0, n_doubled=0)
    assert "stem" in r50_rig.net.describe_launches(2, 0)[0]["kernel"] or "stem" in r50_rig.net.describe_launches(2, 0)[1]["kernel"]


# ---- 9. accumulation and order ---------------------------------------------------------------------------------------------------------
def test_graph_replays_accumulate():
    torch = _torch()
    t, q, model, _ = case_inputs("tiny_saturate", 3)
    rig = Rig(t, q, model, 3)
    xs = [synth.synth_extreme_images(t, 3, seed=s) for s in (3, 4, 5)]
    buf = _dev(xs[0]).clone()
    rig.aud.reset()
    replay = rig.aud.capture(buf)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rig.aud.store(), A.empty_store(rig.aud.store_size // 128))      # capture itself observed nothing
    want = A.empty_store(rig.aud.store_size // 128)
    for x in xs:
        buf.copy_(_dev(x))
        replay()
        want = A.combine(want, rig.oracle(x))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rig.aud.store(), want)
    rig.aud.reset()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rig.aud.store(), A.empty_store(rig.aud.store_size // 128))


def test_two_streams_into_one_store():
    torch = _torch()
    t, q, model, x1 = case_inputs("tiny_benign", 3)
    rig = Rig(t, q, model, 3)
    x2 = synth.synth_images(t, 3, 7)
    other = A.DeviceAuditor(rig.net, 3, store=rig.aud.store_dev)
    d1, d2 = _dev(x1), _dev(x2)
    rig.aud.reset()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s1):
        rig.aud.observe(d1)
    with torch.cuda.stream(s2):
        other.observe(d2)
    torch.cuda.synchronize()
    two = rig.aud.store()
    rig.aud.reset()
    rig.aud.observe(d1)
    rig.aud.observe(d2)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(two, rig.aud.store())
    np.testing.assert_array_equal(two, A.combine(rig.oracle(x1), rig.oracle(x2)))


def test_one_pixel_past_a_slab():
    """41 images of the 10 x 10 tiny program: rows 0 and 2 hold 41 * 25 = 1025 pixels, one more than the kernel's slab"""
    t = cfg.tiny_tables(hw=10)
    q = synth.synth_q_values(t, 2)
    B = 41
    rig = Rig(t, q, synth.synth_model(t, q, 2), B)
    got, rows = rig.check(synth.synth_images(t, B, 2, kind="int8"))
    assert max(B * r["H"] * r["W"] for r in rows[1:]) == A.SLAB + 1


def test_the_audit_alone_counts_the_kept_maps_once_more():
    """tf2_audit_kept (what tools/act_audit_time.py times by itself), directly and as a captured graph"""
    torch = _torch()
    t, q, model, x = case_inputs("fire_float", 3)
    rig = Rig(t, q, model, 3)
    xd = _dev(x)
    want = rig.oracle(x)
    rig.aud.reset()
    rig.aud.observe(xd)
    rig.aud.audit_kept(xd)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rig.aud.store(), A.combine(want, want))
    replay = rig.aud.capture(xd, kept_only=True)
    rig.aud.reset()
    replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rig.aud.store(), want)


# ---- 11. refusals on a real handle -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_stream_usable():
    torch = _torch()
    t, q, model, x = case_inputs("tiny_benign", 3)
    rig = Rig(t, q, model, 3)
    a, L = rig.aud, _lib.lib()
    xd = _dev(x)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    need = int(L.tf2_audit_workspace_size(a._h, 3))
    assert need == rig.net.workspace_size(3, True) and a._ws.numel() >= need
    run = lambda ws_bytes=need, store=a.store_dev.data_ptr(), store_bytes=a.store_size: L.tf2_audit_run(
        a._h, xd.data_ptr(), 0, 3, a._ws.data_ptr(), ws_bytes, a._logits.data_ptr(), store, store_bytes, stream)
    a.reset()
    assert run(ws_bytes=need - 1) == -3 and "workspace too small" in L.tf2_last_error().decode()
    assert run(store_bytes=a.store_size - 1) == -3 and "store too small" in L.tf2_last_error().decode()
    assert run(store=None) == -1
    torch.cuda.synchronize()
    np.testing.assert_array_equal(a.store(), A.empty_store(a.store_size // 128))          # nothing was enqueued
    assert run() == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(a.store(), rig.oracle(x))
