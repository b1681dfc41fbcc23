"""Launch plans at batches where a fused kernel's tensors cross 2^32 bytes (no device: plans only, nothing allocated or run).

Audit of the fused kernels' global addressing: conv_bfirst, conv_bband, conv_bgroup, conv_fire, conv_c3 and conv_stem form every tensor
address from a 64-bit pixel base (size_t / long long); conv_bneck's phase 2 addresses the expand's residual and output as kernel-argument
base + ONE 32-bit byte offset ((unsigned)pix_base * Cp + channel), and conv_pwk reads and writes through 32-bit offsets as well
(conv_pwk_eligible refuses tensors of 2^32 bytes or more).  So every launch of those two kernels must see tensors below 2^32 bytes; a
bottleneck pair whose tensors do not fit runs as its two separate launches (the planner's fuse eligibility, net_plan.hip)."""
import numpy as np
import pytest

from tf2_amd import config as cfg, network, synth
from tests.conftest import set_opts

OFFSET32 = ("conv_bneck", "conv_pwk")
FOUR_G = 1 << 32


def _net(t, q, model):
    net = network.NetWork(t)
    net.Quantization(synth.q_text(q)); net.LoadModel(model); net.Pack(0)
    return net


def _offset32_violations(net, batch, conc):
    """(row, kernel, tensor bytes) of every tensor >= 2^32 bytes that a 32-bit-offset launch reads or writes.  A launch covers its own
    row and the rows up to the next launch's (a fused pair's expand, a group's inner rows)."""
    launches = net.describe_launches(batch, conc)
    tensors, rows = net.describe_workspace(batch, False)
    starts = sorted({r["layer"] for r in launches if r["layer"] >= 0})
    bad = []
    for r in launches:
        if not r["kernel"].startswith(OFFSET32):
            continue
        nxt = [s for s in starts if s > r["layer"]]
        for row in range(r["layer"], nxt[0] if nxt else len(rows)):
            for key in ("in_tensor", "out_tensor", "conv_tensor", "res_tensor"):
                ti = rows[row][key]
                if ti >= 0 and tensors[ti]["bytes"] >= FOUR_G:
                    bad.append((row, r["kernel"], tensors[ti]["bytes"]))
    return bad, launches


@pytest.mark.parametrize("forced", [False, True])
def test_resnet50_plans_around_the_4g_tensor(golden_dir, monkeypatch, forced):
    """ResNet-50's 56 x 56 x 256 tensors cross 2^32 bytes between batch 5300 and 5400 (3.21 MB per image).  bneck_min=1 makes every
    bottleneck pair eligible for conv_bneck by grid size, as test_fused_bottleneck_pairs does; pwk: the conv_pwk rows as well."""
    import os
    set_opts(monkeypatch, bneck_min="1")
    if forced:
        set_opts(monkeypatch, pwk="2", pwk_minpix="0", pwk_units="0", pwk_slabs="8")
    t = cfg.resnet50_tables()
    q = np.loadtxt(os.path.join(golden_dir, "resnet50_Q"), dtype=np.int32)
    net = _net(t, q, synth.synth_model(t, q, 0))
    assert 56 * 56 * 256 * 5300 < FOUR_G <= 56 * 56 * 256 * 5400
    for batch in (5300, 5400, 8200):
        for conc in (0, 1):
            bad, launches = _offset32_violations(net, batch, conc)
            assert not bad, (batch, conc, bad)
            fused = {r["layer"] for r in launches if r["kernel"].startswith("conv_bneck")}
            if conc == 0:
                # the 28 x 28 pairs (2.2 GB tensors at batch 5400) stay fused at every one of these batches; the 56 x 56 pairs only below 2^32
                assert {16, 19, 22} <= fused, (batch, fused)
                assert ({6, 9} <= fused) == (batch == 5300), (batch, fused)


def test_body_programs_plans_around_the_4g_tensor(monkeypatch):
    """The drawn body programs (tests/test_fuzz_programs.py): per conv_bneck pair the batch just below and just above the point where its
    expand's output tensor reaches 2^32 bytes; no 32-bit-offset launch may see a tensor of 2^32 bytes or more, and below it the pair stays
    fused."""
    from tests.test_fuzz_programs import _BODY_OPTS, BODY_SEEDS, random_body_program, _q_and_model
    set_opts(monkeypatch, **_BODY_OPTS)
    checked = 0
    for seed in BODY_SEEDS[:6]:
        t = random_body_program(seed)
        q, model = _q_and_model(t, seed)
        net = _net(t, q, model)
        pairs = {r["layer"] for r in net.describe_launches(64, 0) if r["kernel"].startswith("conv_bneck")}
        for l in sorted(pairs):
            tensors, rows = net.describe_workspace(64, False)
            per_img = max(tensors[rows[l + 1][k]]["bytes"] for k in ("out_tensor", "res_tensor") if rows[l + 1][k] >= 0) / 64
            edge = int(FOUR_G // per_img)
            for batch in (edge - 1, edge + 2):
                bad, launches = _offset32_violations(net, batch, 0)
                assert not bad, (seed, batch, bad)
                big = max(tensors2["bytes"] for tensors2 in net.describe_workspace(batch, False)[0]) >= FOUR_G
                fused = any(r["layer"] == l and r["kernel"].startswith("conv_bneck") for r in launches)
                if batch == edge + 2:
                    assert big and not fused, (seed, l, batch)
                else:
                    assert fused, (seed, l, batch)
                checked += 1
    assert checked >= 4
