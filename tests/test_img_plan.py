"""Where conv_img.hip (stride-1 rows of small square maps, whole images per block: ResNet-50's 7 x 7 x 512 3x3 rows 48 and 51) appears in
the launch plans and where it must not, and what its launches need (no device: plans are described, nothing is allocated or run)."""
import json
import os
import struct

import numpy as np
import pytest

from tf2_amd import _lib, config as cfg, network, synth
from tests.conftest import set_opts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG = "conv_img_kernel"


def _net(t, q, model):
    net = network.NetWork(t)
    net.Quantization(synth.q_text(q)); net.LoadModel(model); net.Pack(0)
    return net


@pytest.fixture(scope="module")
def r50(golden_dir):
    t = cfg.resnet50_tables()
    q = np.loadtxt(os.path.join(golden_dir, "resnet50_Q"), dtype=np.int32)
    return t, q, synth.synth_model(t, q, 0)


def _img_rows(net, batch, conc):
    return sorted(r["layer"] for r in net.describe_launches(batch, conc) if r["kernel"].startswith(IMG))


def test_forced_on_in_flight_plan_takes_rows_48_and_51(r50, monkeypatch):
    set_opts(monkeypatch, img="1")
    net = _net(*r50)
    plan = cfg.build_plan(r50[0])
    launches = net.describe_launches(32, 1)
    mine = [r for r in launches if r["kernel"].startswith(IMG)]
    assert sorted(r["layer"] for r in mine) == [48, 51], [(r["layer"], r["kernel"]) for r in launches]
    for r in mine:
        L = plan[r["layer"]]
        assert (L.H, L.W, L.C, L.k, L.stride) == (7, 7, 512, 3, 1)
        # the name states map, C, k, windows and images per block; one block per (m-tile, image pair)
        assert r["kernel"].startswith("conv_img_kernel<7x7,C512,k3,") and "-window,2 images>" in r["kernel"], r["kernel"]
        assert r["grid"] == (512 // 64) * 16 and r["block"] == 512
    # row 45 (3x3 / stride 2) and every row of stages 1-4 (rows below 43) stay where they were
    off = _net_names(r50, monkeypatch, img="0")
    for r in launches:
        if r["layer"] not in (48, 51):
            assert not r["kernel"].startswith(IMG)
    assert [r["kernel"] for r in launches if r["layer"] not in (48, 51)] == [k for l, k in off if l not in (48, 51)]


def _net_names(r50, monkeypatch, batch=32, conc=1, **opts):
    set_opts(monkeypatch, **opts)
    return [(r["layer"], r["kernel"]) for r in _net(*r50).describe_launches(batch, conc)]


def test_off_is_the_recorded_plan(r50, monkeypatch):
    """img=0 gives the kernel names of the batch-32 in-flight plan as profiles/r06_trace_launches_b32_conc1.json recorded them (before the
    kernel existed); the default (img=1) differs from that in rows 48 and 51 alone."""
    rec = json.load(open(os.path.join(ROOT, "profiles", "r06_trace_launches_b32_conc1.json")))
    want = [(r["layer"], r["kernel"]) for r in rec["launches"]]
    assert _net_names(r50, monkeypatch, img="0") == want
    dflt = _net_names(r50, monkeypatch, img=None)
    assert [x for x in dflt if x[0] not in (48, 51)] == [x for x in want if x[0] not in (48, 51)]
    assert sorted(l for l, k in dflt if k.startswith(IMG)) == [48, 51]


def test_plans_that_keep_their_kernels(r50, monkeypatch):
    """img=1 is the in-flight plan only, from img_min on: the one-batch-at-a-time plan at batch 32 and both batch-1 plans never name the
    kernel unless img=2 / img_min=1 ask; with img=2 the group launches keep their rows (they are asked first)."""
    set_opts(monkeypatch, img="1")
    net = _net(*r50)
    assert _img_rows(net, 32, 0) == [] and _img_rows(net, 1, 0) == [] and _img_rows(net, 1, 1) == []
    assert _img_rows(net, 8, 1) == [48, 51] and _img_rows(net, 7, 1) == []                         # img_min = 8
    set_opts(monkeypatch, img="1", img_min="1")
    net = _net(*r50)
    assert _img_rows(net, 1, 1) == [48, 51] and _img_rows(net, 1, 0) == [] and _img_rows(net, 32, 0) == []
    set_opts(monkeypatch, img="2", img_min=None)
    net = _net(*r50)
    groups = [r["layer"] for r in net.describe_launches(32, 0) if "conv_bgroup" in r["kernel"]]
    assert 47 in groups and _img_rows(net, 32, 0) == []                                           # rows 47-52 are one chained group launch
    assert _img_rows(net, 8, 0) == [48, 51]                                                         # (below bgroup_min7 the rows are plain rows)
    set_opts(monkeypatch, img="2", bgroup="0")
    assert _img_rows(_net(*r50), 32, 0) == [48, 51]
    # the per-row masks (test-only) decide a row whatever img / img_min say
    set_opts(monkeypatch, img="0", bgroup=None, img_rows=str(1 << 48))
    assert _img_rows(_net(*r50), 32, 1) == [48]
    set_opts(monkeypatch, img="1", img_rows=None, noimg_rows=str(1 << 48))
    assert _img_rows(_net(*r50), 32, 1) == [51]


@pytest.mark.parametrize("name", ["googlenet", "vgg16", "ssd300"])
def test_other_networks_name_it_only_where_the_predicate_holds(name, monkeypatch):
    """Net::img_at restated on the tables: a 3x3 / stride 1 / pad 1 row on a 7 x 7 map of 512 input channels without pool, average,
    concat slice or residual, fed by a ReLU row's own tensor.  None of these networks has such a row."""
    set_opts(monkeypatch, img="2", img_min="1", bgroup="0")
    t, q, seed = synth.bench_network(name)[:3]
    net = _net(t, q, synth.synth_model(t, q, seed))
    plan = cfg.build_plan(t)
    for batch, conc in ((1, 0), (3, 1), (32, 1), (32, 0)):
        for r in net.describe_launches(batch, conc):
            if not r["kernel"].startswith(IMG):
                continue
            L = plan[r["layer"]]
            assert (L.H, L.W, L.C, L.k, L.stride, L.pad_h, L.pad_w) == (7, 7, 512, 3, 1, 1, 1), (name, r)
            assert not (L.ipool or L.pool_en or L.endpool or L.concat >= 0 or L.add_src >= 0) and L.src >= 0 and plan[L.src].relu, (name, r)
            assert r["layer"] != len(plan) - 1


# ---- resources -------------------------------------------------------------------------------------------------------------------
def _code_objects(path):
    """The gfx950 code objects (ELF images) of the offload bundles inside a HIP shared library."""
    blob = open(path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    pos = blob.find(magic)
    while pos >= 0:
        n, = struct.unpack_from("<Q", blob, pos + len(magic))
        at = pos + len(magic) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, at)
            triple = blob[at + 24:at + 24 + tlen].decode()
            at += 24 + tlen
            if "gfx950" in triple and size:
                yield blob[pos + off:pos + off + size]
        pos = blob.find(magic, pos + len(magic))


def _kernel_descriptors(elf):
    """{kernel symbol: (group_segment_fixed_size, private_segment_fixed_size)} from the `<kernel>.kd` symbols of a code object: the first
    two words of the 64-byte amdhsa kernel descriptor."""
    assert elf[:4] == b"\x7fELF" and elf[4] == 2
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for s in secs:
        if s[1] not in (2, 11):                              # SHT_SYMTAB, SHT_DYNSYM
            continue
        str_off = secs[s[6]][4]
        for k in range(s[5] // 24):
            st_name, _, _, shndx, value, _ = struct.unpack_from("<IBBHQQ", elf, s[4] + k * 24)
            name = elf[str_off + st_name:elf.index(b"\0", str_off + st_name)].decode()
            if name.endswith(".kd") and 0 < shndx < shnum:
                sec = secs[shndx]
                out[name[:-3]] = struct.unpack_from("<II", elf, sec[4] + value - sec[3])
    return out


def test_launch_resources(r50, monkeypatch):
    set_opts(monkeypatch, img="2", img_min="1", bgroup="0")
    t, q, _ = r50
    q2 = synth.synth_q_values(t, 0, spread=2)                                  # (the shipped Q file packs rows 48 / 51 as one-window rows; Q values spread over
    seen = set()                                                               #  three exponents per tensor make them two-window rows)
    for net in (_net(*r50), _net(t, q2, synth.synth_model(t, q2, 0))):
        for batch, conc in ((1, 0), (3, 1), (32, 1), (33, 0)):
            mine = [r for r in net.describe_launches(batch, conc) if r["kernel"].startswith(IMG)]
            assert len(mine) == 2
            for r in mine:
                assert 0 < r["lds_bytes"] <= 163840, r
                assert r["grid"] == 8 * ((batch + 1) // 2)
                seen.add("one-window" in r["kernel"])
    assert seen == {True, False}                                               # both instantiations are launched somewhere above
    kds = {}
    for elf in _code_objects(_lib.LIB_PATH):
        kds.update({k: v for k, v in _kernel_descriptors(elf).items() if "conv_img_kernel" in k})
    assert len(kds) == 2, sorted(kds)                                          # one- and two-window
    for name, (group, private) in kds.items():
        assert private == 0, (name, private)                                   # no scratch at eight waves per block
