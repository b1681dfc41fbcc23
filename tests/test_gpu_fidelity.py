"""Layer fidelity on the device (tf2_fid_*, csrc/act_fidelity.hip): the store of fidelity.DeviceComparator equals
fidelity.reference_compare -- as integers, one assertion over the whole store -- of the oracle's maps (netref.RefNet.run) and of
Runner.read_layer after a separate keep_all run on the same images, against the references of fidelity.float_refs on the device (copied
to the host for the statement), and the logits equal Runner.run_batch's.  The regimes come from tests/test_audit.py;
tests/test_fidelity.py shows on the oracle what they clamp."""
import os

import numpy as np
import pytest

from oracle import netref
from tf2_amd import _lib, config as cfg, fidelity as F, network, synth
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
        self.t, self.model, self.batch = t, model, batch
        self.net = network.NetWork(t)
        self.net.Init(model, synth.q_text(q), device=DEV)
        self.ref = netref.RefNet(t, q, model)
        self.cmp = F.DeviceComparator(self.net, batch)
        self.runner = network.Runner(None, self.net)
        self.q_rows = F.q_rows_of_net(self.net)
        self.q0 = int(self.q_rows[-1][0])
        self.records = self.cmp.store_size // 144

    def refs(self, x):
        """float_refs on the device (int8 images go in as the floats of their values, as in tests/test_fidelity.py)"""
        return F.float_refs(self.t, self.model, x, device=DEV)

    def statement(self, maps, refs_host, x):
        return F.reference_compare(maps, refs_host, self.q_rows, images=x, q0=self.q0)

    def oracle(self, x, refs_host):
        return self.statement(self.ref.run(x), refs_host, x)

    def check(self, x, refs, both=True):
        """one compared batch on an empty store against the statement; returns (store, rows, oracle maps)"""
        torch = _torch()
        B = x.shape[0]
        xd = _dev(x)
        self.cmp.reset()
        logits = self.cmp.observe(xd, refs).cpu().numpy()
        got = self.cmp.store()
        plain = self.runner.run_batch(xd, keep_all=True).cpu().numpy()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(logits, plain, err_msg="logits of tf2_fid_run against Runner.run_batch")
        host = [None if r is None else r.cpu().numpy() for r in refs]
        maps = self.ref.run(x)
        np.testing.assert_array_equal(got, self.statement(maps, host, x), err_msg="device store against the oracle")
        read = [self.runner.read_layer(l, B) for l in range(self.net.num_layer)]
        if both:
            np.testing.assert_array_equal(got, self.statement(read, host, x), err_msg="device store against read_layer")
        else:                                   # (large programs: the same maps give the same statement)
            for l, m in enumerate(read):
                np.testing.assert_array_equal(m.reshape(maps[l].shape), maps[l], err_msg=f"read_layer({l}) against the oracle")
        rows = self.cmp.rows()
        assert got.shape == (self.records, 18) and (got[:, 10:].sum(1) == got[:, 0]).all()
        return got, rows, maps


def poisoned(refs, maps, q_rows, seed):
    """A copy of the references with, in every row at seeded positions: NaN, +-inf, +-3e38 (t overflows), -0.0, a denormal, and
    (v + j/512) * 2^-Q -- e = 256 v + j/2 exactly, a tie for odd j -- with |j|/2 at both edges of every histogram bin"""
    torch = _torch()
    rng = np.random.default_rng(seed)
    special = [np.nan, np.inf, -np.inf, 3e38, -3e38, -0.0, 1e-40]
    js = [1, -1, 3, -3, 255, -255, 256, 257, 767, 768, 1791, -1792, 3839, 3840, 7935, -7936, 16127, 16128, 32511, 32512, -40001]
    out = []
    for l, r in enumerate(refs):
        h = r.cpu().numpy().copy()
        v = np.asarray(maps[l]).reshape(h.shape)
        flat, vflat = h.reshape(h.shape[0], h.shape[1], -1), v.reshape(h.shape[0], h.shape[1], -1)
        n = flat.size
        pos = rng.choice(n, size=min(n, len(special) + len(js)), replace=False)
        for i, p in enumerate(pos):
            b, c, s = np.unravel_index(p, flat.shape)
            if i < len(special):
                flat[b, c, s] = special[i]
            else:
                val = (float(vflat[b, c, s]) + js[i - len(special)] / 512.0) * 2.0 ** -float(q_rows[l][c])
                assert float(np.float32(val)) == val
                flat[b, c, s] = val
        out.append(torch.from_numpy(h).to(DEV))
    return out


# ---- 6. the small programs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tiny_benign", "tiny_saturate", "fire_float", "fire_int8"])
@pytest.mark.parametrize("batch", [3, 1])
def test_small_programs(case, batch):
    t, q, model, x = case_inputs(case, batch)
    rig = Rig(t, q, model, batch)
    refs = rig.refs(x)
    got, rows, maps = rig.check(x, refs)
    lay = F.layer_summary(got, rows)
    assert all(lay[l]["n"] == batch * r["C"] * r["H"] * r["W"] for l, r in zip(sorted(lay), rows) if l >= 0)
    assert (lay[-1]["n"] == 0) == (x.dtype == np.int8)                                 # int8 images: row -1 is not compared
    if case == "tiny_saturate":
        assert all(lay[l]["ref_clamped"] > 0 for l in lay if l >= 0)
    elif case != "fire_int8":
        assert got[3:, F.REF_CLAMPED].sum() == 0 and got[:, F.NONFINITE].sum() == 0
    if case.startswith("tiny"):
        assert sorted({r["C"] for r in rows}) == [3, 10, 16, 32] and {(r["H"], r["W"]) for r in rows[1:]} >= {(6, 6), (3, 3), (1, 1)}
        assert rows[-2]["H"] == 1 and lay[rig.net.num_layer - 2]["n"] == batch * rows[-2]["C"]      # the end-pool row: one value an image
    if case.startswith("fire"):
        assert any(L.concat >= 0 and L.n_start > 0 for L in rig.ref.plan)                # a slice with out_off != 0
        assert "im2col" in rig.net.describe_launches(batch, 0)[0]["kernel"]              # the input tensor is not the image
    # the same program against poisoned references
    bad = poisoned(refs, maps, rig.q_rows, seed=batch)
    got, rows, _ = rig.check(x, bad)
    lay = F.layer_summary(got, rows)
    for l, r in zip(sorted(lay), rows):
        if l >= 0 and batch * r["C"] * r["H"] * r["W"] >= 28:
            assert lay[l]["nonfinite"] >= 3 and lay[l]["ref_clamped"] >= 2, l
            first = r["offset"] // 144
            assert (got[first:first + r["C"], 10:].sum(0) > 0).all(), (l, got[first:first + r["C"], 10:].sum(0))     # every bin


def test_null_references_leave_their_rows_empty():
    t, q, model, x = case_inputs("fire_float", 3)
    rig = Rig(t, q, model, 3)
    refs = rig.refs(x)
    skip = {0, 3, rig.net.num_layer - 1}
    some = [None if l in skip else r for l, r in enumerate(refs)]
    got, rows, _ = rig.check(x, some)
    for r in rows[1:]:
        first = r["offset"] // 144
        assert (not got[first:first + r["C"]].any()) == (r["layer"] in skip), r
    # a dict names the rows that are compared
    rig.cmp.reset()
    rig.cmp.observe(_dev(x), {l: r for l, r in enumerate(refs) if l not in skip})
    np.testing.assert_array_equal(rig.cmp.store(), got)


def test_more_rows_than_one_launch_takes():
    """70 store rows: tf2_fid_run deals the 69 table rows to two launches (64 and 5); with rows 60 .. 68 not compared the 60 that are
    left fit one launch, the others' records stay empty"""
    t, q, model, x = case_inputs("long", 2)
    rig = Rig(t, q, model, 2)
    refs = rig.refs(x)
    got, rows, _ = rig.check(x, refs)
    assert len(rows) == 70 > F.ROWS_PER_LAUNCH and got.shape[0] == 813 and (got[:, F.N] > 0).all()
    part, _, _ = rig.check(x, [None if 60 <= l <= 68 else r for l, r in enumerate(refs)])
    for r in rows[1:]:
        rec = slice(r["offset"] // 144, r["offset"] // 144 + r["C"])
        if 60 <= r["layer"] <= 68:
            assert not part[rec].any(), r
        else:
            np.testing.assert_array_equal(part[rec], got[rec], err_msg=str(r))


def test_scale_exponents_from_minus_64_to_64():
    """Any integer Q in -64 .. 64: the comparator's scale table replaced by one whose rows run over the whole range (both ends in every
    row), the references built around the engine's own values, (v + noise) * 2^-Q, so that every channel has small and large errors"""
    torch = _torch()
    t, q, model, x = case_inputs("tiny_benign", 3)
    rig = Rig(t, q, model, 3)
    maps = rig.ref.run(x)
    rng = np.random.default_rng(64)
    rows = rig.cmp.rows()
    q_rows = {-1: rig.q_rows[-1]}
    refs = []
    for r in rows[1:]:
        qq = rng.integers(-64, 65, r["C"])
        qq[0], qq[-1] = -64, 64
        q_rows[r["layer"]] = qq
        m = np.asarray(maps[r["layer"]]).astype(np.float64)
        noise = rng.uniform(-3, 3, m.shape) * (rng.random(m.shape) < 0.5)
        f = ((m + noise) * 2.0 ** -qq.astype(np.float64).reshape((1, -1) + (1,) * (m.ndim - 2))).astype(np.float32)
        refs.append(_dev(f))
    rig.cmp._scales = _dev(np.concatenate([F.scale_of(q_rows[r["layer"]]) for r in rows]))
    rig.q_rows = q_rows
    got, _, _ = rig.check(x, refs)
    lay = F.layer_summary(got, rows)
    assert all(lay[l]["ref_clamped"] == 0 and lay[l]["nonfinite"] == 0 and 0 < lay[l]["max_err_lsb"] <= 3.01 for l in lay if l >= 0)


# ---- 7. SSD: L2Norm row, pooling row (its source's Q), dilated row, heads with C = 16, 24, 84, 126, maps larger than a slab -------------
def test_ssd_program():
    t = cfg.ssd300_tables(width_div=4)
    q = synth.synth_q_values(t, 3, spread=1)
    rig = Rig(t, q, synth.synth_model(t, q, 3), 2)
    x = synth.synth_images(t, 2, 3)
    got, rows, _ = rig.check(x, rig.refs(x), both=False)
    plan = rig.ref.plan
    assert any(L.ipool == 2 for L in plan) and any(L.ipool == 1 for L in plan) and any(L.dil > 1 for L in plan)
    assert {16, 24, 84, 126} <= {r["C"] for r in rows} and max(2 * r["H"] * r["W"] for r in rows[1:]) > F.SLAB


# ---- 8. ResNet-50: the doubled form, C up to 2048, HW = 49, 196, 784, 3136, the x-only stem input -----------------------------------------
def test_resnet50_batch2(golden_dir):
    t = cfg.resnet50_tables()
    q = np.loadtxt(os.path.join(golden_dir, "resnet50_Q"), dtype=np.int32)
    rig = Rig(t, q, synth.synth_model(t, q, 0), 2)
    x = synth.synth_images(t, 2, 0)
    got, rows, _ = rig.check(x, rig.refs(x), both=False)
    assert sum(r["n_doubled"] for r in rows) > 0                                          # the 2y - 128 form is really met
    assert max(r["C"] for r in rows) == 2048 and {49, 196, 784, 3136} <= {r["H"] * r["W"] for r in rows[1:]}
    assert "stem" in rig.net.describe_launches(2, 0)[0]["kernel"] or "stem" in rig.net.describe_launches(2, 0)[1]["kernel"]


# ---- 9. accumulation and order ---------------------------------------------------------------------------------------------------------
def test_graph_replays_accumulate_over_refilled_buffers():
    torch = _torch()
    t, q, model, _ = case_inputs("tiny_benign", 3)
    rig = Rig(t, q, model, 3)
    xs = [synth.synth_images(t, 3, s) for s in (1, 4, 5)]
    sets = [rig.refs(x) for x in xs]
    buf = _dev(xs[0]).clone()
    rbuf = [r.clone() for r in sets[0]]
    rig.cmp.reset()
    replay = rig.cmp.capture(buf, rbuf)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rig.cmp.store(), F.empty_store(rig.records))           # capture itself compared nothing
    want = F.empty_store(rig.records)
    for x, refs in zip(xs, sets):
        buf.copy_(_dev(x))
        for dst, src in zip(rbuf, refs):
            dst.copy_(src)
        replay()
        want = F.combine(want, rig.oracle(x, [r.cpu().numpy() for r in refs]))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rig.cmp.store(), want)
    rig.cmp.reset()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rig.cmp.store(), F.empty_store(rig.records))


def test_two_streams_into_one_store():
    torch = _torch()
    t, q, model, x1 = case_inputs("tiny_benign", 3)
    rig = Rig(t, q, model, 3)
    x2 = synth.synth_images(t, 3, 7)
    other = F.DeviceComparator(rig.net, 3, store=rig.cmp.store_dev)
    d1, d2, r1, r2 = _dev(x1), _dev(x2), rig.refs(x1), rig.refs(x2)
    rig.cmp.reset()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s1):
        rig.cmp.observe(d1, r1)
    with torch.cuda.stream(s2):
        other.observe(d2, r2)
    torch.cuda.synchronize()
    two = rig.cmp.store()
    want = F.combine(rig.oracle(x1, [r.cpu().numpy() for r in r1]), rig.oracle(x2, [r.cpu().numpy() for r in r2]))
    np.testing.assert_array_equal(two, want)


def test_one_pixel_past_a_slab_and_a_tile():
    """41 images of the 10 x 10 tiny program: rows 0 and 2 hold 41 * 25 = 1025 pixels, one more than the kernel's slab; HW = 25 is no
    multiple of four, so the 16-byte loads give way to per-pixel addresses inside a tile"""
    t = cfg.tiny_tables(hw=10)
    q = synth.synth_q_values(t, 2)
    B = 41
    rig = Rig(t, q, synth.synth_model(t, q, 2), B)
    x = synth.synth_images(t, B, 2, kind="int8")
    got, rows, _ = rig.check(x, rig.refs(x))
    assert max(B * r["H"] * r["W"] for r in rows[1:]) == F.SLAB + 1


def test_compare_kept_is_observe_on_a_fresh_store():
    """tf2_fid_kept (what tools/fidelity_time.py times by itself), directly and as a captured graph"""
    torch = _torch()
    t, q, model, x = case_inputs("fire_float", 3)
    rig = Rig(t, q, model, 3)
    xd, refs = _dev(x), rig.refs(x)
    want = rig.oracle(x, [r.cpu().numpy() for r in refs])
    rig.cmp.reset()
    rig.cmp.observe(xd, refs)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rig.cmp.store(), want)
    rig.cmp.reset()
    rig.cmp.compare_kept(xd, refs)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rig.cmp.store(), want)
    replay = rig.cmp.capture(xd, refs, kept_only=True)
    rig.cmp.reset()
    replay()
    replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rig.cmp.store(), F.combine(want, want))


# ---- 10. refusals on a real handle -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_stream_usable():
    import ctypes as C
    torch = _torch()
    t, q, model, x = case_inputs("tiny_benign", 3)
    rig = Rig(t, q, model, 3)
    a, L = rig.cmp, _lib.lib()
    xd, refs = _dev(x), rig.refs(x)
    arr = a._ref_array(refs)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    need = int(L.tf2_fid_workspace_size(a._h, 3))
    assert need == rig.net.workspace_size(3, True) and a._ws.numel() >= need
    run = lambda ws_bytes=need, rf=arr, sc=a._scales.data_ptr(), store=a.store_dev.data_ptr(), store_bytes=a.store_size: L.tf2_fid_run(
        a._h, xd.data_ptr(), 0, 3, a._ws.data_ptr(), ws_bytes, a._logits.data_ptr(), rf, sc, store, store_bytes, stream)
    a.reset()
    assert run(ws_bytes=need - 1) == -3 and "workspace too small" in L.tf2_last_error().decode()
    assert run(store_bytes=a.store_size - 1) == -3 and "store too small" in L.tf2_last_error().decode()
    assert run(store=None) == -1 and run(rf=None) == -1 and run(sc=None) == -1
    torch.cuda.synchronize()
    np.testing.assert_array_equal(a.store(), F.empty_store(rig.records))                  # nothing was enqueued
    assert run() == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(a.store(), rig.oracle(x, [r.cpu().numpy() for r in refs]))
