"""GPU parity at the arithmetic extremes: the extreme-regime models of tf2_amd/synth.py (synth_extreme: int32 wrap of the accumulator,
in one-window rows and in two-window rows whose hi << dshift wraps on its own, requantisation that clips and saturates, 3-5 exponent
windows, shifts at conv_shift's mul24 boundary) and int8 images with -128 / 127
patches, every layer against the oracle, on the kernel families and epilogue forms the routing options select.  Each case also checks
in the launch plan that the kernel it is about really runs (a routing change must not silently skip it).  The regimes themselves are
shown to be reached on the CPU: tests/test_extreme_regimes.py."""
import pytest

from tf2_amd import config as cfg, synth
from tests.conftest import set_opts
from tests.test_extreme_regimes import BODY_WANT_WRAP2, FIRE_WRAP2_ROWS, R50_ROUTES, VGG16_WRAP2, covered_rows, r50_extreme, route
from tests.test_gpu_parity import Rig

pytestmark = pytest.mark.gpu


def _runs(rig, batch, prefix, rows, conc=0):
    """The rows `rows` are computed by launches of the kernel `prefix` (the targeted rows really run there)."""
    launches = rig.net.describe_launches(batch, conc)
    got = covered_rows(launches, prefix)
    assert set(rows) <= got, (prefix, sorted(rows), sorted(got), [(r["layer"], r["kernel"]) for r in launches])


# ---- the tiny net: every regime, ring / split-K kernels (mode 0) and the shift kernels (mode 2) -------------------------------------
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("regime", ["wrap", "saturate", "spread", "shift22", "shift23", "expand32", "wrap2"])
def test_tiny_net_at_the_extremes(regime, mode):
    t = cfg.tiny_tables()
    q, model = synth.synth_extreme(t, 5, regime)
    rig = Rig(t, q, model, mode)
    if mode == 2:
        _runs(rig, 3, "conv_shift", range(1, 9))
    rig.check_all_layers(synth.synth_extreme_images(t, 3, 5))


@pytest.mark.parametrize("opts", [dict(nofast="1"), dict(nosemi="1"), dict(nodual="1"), dict(no4bit="1")])
def test_tiny_net_at_the_extremes_other_packed_forms(opts, monkeypatch):
    set_opts(monkeypatch, **opts)
    t = cfg.tiny_tables()
    # (wrap2 under nodual = 1: the same rows in the Horner form, acc <<= dshift between the windows)
    for regime, mode in (("wrap", 0), ("saturate", 0), ("spread", 0), ("shift23", 2), ("wrap2", 0)):
        q, model = synth.synth_extreme(t, 7, regime)
        Rig(t, q, model, mode).check_all_layers(synth.synth_extreme_images(t, 2, 7))


# ---- ResNet-50: every row extreme (spread: rows 14 and 30; wrap2: a model per route), one route per kernel family (tests/test_extreme_regimes.py R50_ROUTES) --------
@pytest.fixture(scope="module")
def r50_models():
    return {}


def _r50(models, regime, model=None):
    if (regime, model) not in models:
        models[regime, model] = r50_extreme(regime, model)
    return models[regime, model]


@pytest.mark.parametrize("regime,name", [(g, r) for g in ("wrap", "saturate", "spread", "wrap2") for r in R50_ROUTES[g]])
def test_resnet50_extreme_rows(r50_models, regime, name, monkeypatch):
    opts, B, conc, want, mname = route(regime, name)
    set_opts(monkeypatch, **opts)
    rig = Rig(*_r50(r50_models, regime, mname), 0)
    for prefix, rows in want.items():
        _runs(rig, B, prefix, rows, conc)
    rig.check_all_layers(synth.synth_extreme_images(rig.t, B, 1))


@pytest.mark.parametrize("switch", ["nofast", "nosemi", "nodual"])
def test_resnet50_wrap_rows_epilogue_forms(r50_models, switch, monkeypatch):
    set_opts(monkeypatch, **{switch: "1"})
    rig = Rig(*_r50(r50_models, "wrap"), 0)
    rig.check_all_layers(synth.synth_extreme_images(rig.t, 2, 3))


@pytest.mark.parametrize("regime,mname", [("wrap", None), ("wrap2", "body")])
def test_resnet50_conv_img_epilogue_forms(r50_models, regime, mname, monkeypatch):
    """conv_img.hip's rows 48 / 51 (the SEMI and the generic one) with the SEMI / FAST proofs switched off at pack time: the wrapped
    one-window rows of the wrap model and the wrapped two-window rows of wrap2's body model in the generic six-instruction form and,
    under nofast alone, the SEMI one; batch 3 (a full two-image block and the one-image tail block)."""
    opts, B, conc, want, _ = route(regime, "img")
    for switch in ("nofast", "nosemi"):
        set_opts(monkeypatch, **dict(opts, nofast=None, nosemi=None))
        set_opts(monkeypatch, **{switch: "1"})
        rig = Rig(*_r50(r50_models, regime, mname), 0)
        for prefix, rows in want.items():
            _runs(rig, B, prefix, rows, conc)
        rig.check_all_layers(synth.synth_extreme_images(rig.t, B, 2))


@pytest.mark.parametrize("graph", [False, True])
def test_resnet50_wrap_four_batches_in_flight(r50_models, graph):
    """The bench configuration (four runners, four streams, HIP graph replay) on the wrap model: every logits row of the last steps
    against a serial run, the serial run against the oracle.  Stage 5's 3x3 rows run on conv_img.hip there (its default plan)."""
    from tests.test_gpu_configs import _in_flight
    rig = Rig(*_r50(r50_models, "wrap"), 0)
    _runs(rig, 8, "conv_img_kernel", {48, 51}, conc=1)
    _in_flight(rig, 8, 4, 12, graph, 900)


def test_resnet50_wrap2_four_batches_in_flight(r50_models, monkeypatch):
    """The same (graph replay) on wrap2's body model: wrapped two-window rows on conv_img (48, 51), in conv_bband's 3x3 phase (16, 19) and
    on conv_pwk (5, 8, 14; pwk_units = 0: at batch 8 the rows have fewer units than the default asks for), with other batches' kernels
    on the chip.  (Logits only: a replayed graph runs the ordinary plan, which keeps no inner row; the rows themselves are compared in
    test_resnet50_extreme_rows.)  _in_flight's plain images leave the rows wrapped: tests/test_extreme_regimes.py
    test_resnet50_wrap2_rows_wrap_in_both_windows[body] pins that for the first of them."""
    from tests.test_gpu_configs import _in_flight
    set_opts(monkeypatch, pwk_units="0")
    rig = Rig(*_r50(r50_models, "wrap2", "body"), 0)
    for prefix, rows in {"conv_img_kernel": {48, 51}, "conv_bband": {16, 19}, "conv_pwk_kernel": {5, 8, 14}}.items():
        _runs(rig, 8, prefix, rows, conc=1)
    _in_flight(rig, 8, 4, 12, True, 900)


# ---- SqueezeNet (fire modules, merged rows, the shift kernels' classifier), small VGG16 (conv_c3, conv_fc) ---------------------------
@pytest.mark.parametrize("regime", ["wrap", "saturate", "spread", "wrap2"])
@pytest.mark.parametrize("opts", [dict(fire="0"), dict(merge="0")])
def test_squeezenet_at_the_extremes(regime, opts, monkeypatch):
    set_opts(monkeypatch, **opts)
    t = cfg.squeezenet11_tables(image_hw=67)
    q, model = synth.synth_extreme(t, 6, regime)
    rig = Rig(t, q, model, 0)
    rig.check_all_layers(synth.synth_extreme_images(t, 2, 6))


@pytest.mark.parametrize("seed", [1, 4])
@pytest.mark.parametrize("regime", ["wrap", "saturate"])          # (spread rows need 3+ windows: conv_fire does not take them)
def test_fire_programs_at_the_extremes(seed, regime, monkeypatch):
    from tests.test_fuzz_programs import random_fire_program
    set_opts(monkeypatch, fire="1")
    t = random_fire_program(seed)
    q, model = synth.synth_extreme(t, seed, regime)
    rig = Rig(t, q, model, 0)
    _runs(rig, 2, "conv_fire", {1, 4})        # (squeeze + expand rows of the first two fire modules; every conv row is targeted)
    rig.check_all_layers(synth.synth_extreme_images(t, 2, seed))


@pytest.mark.parametrize("seed", [1, 4])
def test_fire_programs_wrap2_squeezes(seed, monkeypatch):
    """conv_fire takes a two-window squeeze but one-window expands only (fire_at: "if (p1->n_phases != 1 || p1->dual || ...) return
    false;"), so the wrap2 rows are the squeeze rows 1 (generic) and 4 (SEMI) of the first two fire modules, the expands plain
    one-window rows (q_spread = 0)."""
    from tests.test_fuzz_programs import random_fire_program
    set_opts(monkeypatch, fire="1")
    t = random_fire_program(seed)
    q, model = synth.synth_extreme(t, seed, "wrap2", rows=FIRE_WRAP2_ROWS, q_spread=0)
    rig = Rig(t, q, model, 0)
    _runs(rig, 2, "conv_fire", FIRE_WRAP2_ROWS)
    rig.check_all_layers(synth.synth_extreme_images(t, 2, seed))


@pytest.mark.parametrize("regime", ["wrap", "saturate"])          # (spread rows need 3+ windows: neither conv_c3 nor conv_fc takes them)
@pytest.mark.parametrize("opts,want", [(dict(c3="1", c3_min="1", c3_min256="1", fc="1", fc4="1", fc_min="8"),
                                        {"conv_c3_kernel": {1, 2, 3, 4, 5, 6}, "fc4_partial": {13, 14}}),
                                       (dict(c3="0", fc="1", fc4="0", fc_min="8"), {"fc_partial": {13, 14}}),
                                       (dict(c3="1", c3_min="1", c3_w9="2", fc="0", no4bit="1"), {"conv_c3_w9": {1}, "conv_c3_kernel": {3, 4, 5, 6}})])
def test_small_vgg16_at_the_extremes(regime, opts, want, monkeypatch):
    set_opts(monkeypatch, **opts)
    t = cfg.vgg16_tables(64, 40)
    q, model = synth.synth_extreme(t, 4, regime)
    rig = Rig(t, q, model, 0)
    for prefix, rows in want.items():
        _runs(rig, 2, prefix, rows)
    rig.check_all_layers(synth.synth_extreme_images(t, 2, 4))


# wrap2 on the small VGG16: conv_c3_kernel and conv_fc's int8 form take the two-window rows (rows 1, 3, 5 and 13 are the boosted ones).
# Not the 4-bit form -- a nibble holds one of 7 exponents per row and input class, wrap2's levels span 15 (weight_pack.cpp, fc4: "if (e <
# 0 || e > 6) { fits = false; break; }") -- so fc4 = 1 leaves rows 13 / 14 on fc_partial; and not conv_c3_w9 (conv_c3_takes_w9: "return
# mode && a.tmk == 64 && a.C == 64 && !a.dual && ..."), so row 1 stays on conv_c3_kernel under c3_w9 = 2.
@pytest.mark.parametrize("opts,want", VGG16_WRAP2)
def test_small_vgg16_wrap2(opts, want, monkeypatch):
    set_opts(monkeypatch, **opts)
    t = cfg.vgg16_tables(64, 40)
    q, model = synth.synth_extreme(t, 4, "wrap2")
    rig = Rig(t, q, model, 0)
    for prefix, rows in want.items():
        _runs(rig, 2, prefix, rows)
    rig.check_all_layers(synth.synth_extreme_images(t, 2, 4))


_BODY_WANT = {2: ({"conv_bneck": {5, 6, 8, 9}, "conv_c3_kernel": {1, 2}}, {"conv_mfma_sk": {1, 2, 5}}),
              5: ({"conv_c3_kernel": {1, 2}, "fc4_partial": {5}}, {"conv_mfma_sk": {1, 2}}),
              9: ({"conv_bneck": {4, 5}, "conv_c3_kernel": {1}, "fc4_partial": {6}}, {"conv_mfma_sk": {1, 2, 4}})}
# (wrap2: tests/test_extreme_regimes.py BODY_WANT_WRAP2)


@pytest.mark.parametrize("seed", [2, 5, 9])
@pytest.mark.parametrize("regime", ["wrap", "saturate", "spread", "wrap2"])
def test_body_programs_at_the_extremes(seed, regime, monkeypatch):
    from tests.test_fuzz_programs import _BODY_OPTS, random_body_program
    set_opts(monkeypatch, **_BODY_OPTS)
    t = random_body_program(seed)
    q, model = synth.synth_extreme(t, seed, regime)
    rig = Rig(t, q, model, 0)
    want = BODY_WANT_WRAP2[seed] if regime == "wrap2" else _BODY_WANT[seed][regime == "spread"]      # (spread rows: the split-K kernel)
    for prefix, rows in want.items():
        _runs(rig, 2, prefix, rows)
    rig.check_all_layers(synth.synth_extreme_images(t, 2, seed))
