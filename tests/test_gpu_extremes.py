"""GPU parity at the arithmetic extremes: the extreme-regime models of tf2_amd/synth.py (synth_extreme: int32 wrap of the accumulator,
requantisation that clips and saturates, 3-5 exponent windows, shifts at conv_shift's mul24 boundary) and int8 images with -128 / 127
patches, every layer against the oracle, on the kernel families and epilogue forms the routing options select.  Each case also checks
in the launch plan that the kernel it is about really runs (a routing change must not silently skip it).  The regimes themselves are
shown to be reached on the CPU: tests/test_extreme_regimes.py."""
import pytest

from tf2_amd import config as cfg, synth
from tests.conftest import set_opts
from tests.test_extreme_regimes import R50_ROUTES, covered_rows, r50_extreme
from tests.test_gpu_parity import Rig

pytestmark = pytest.mark.gpu


def _runs(rig, batch, prefix, rows, conc=0):
    """The rows `rows` are computed by launches of the kernel `prefix` (the targeted rows really run there)."""
    launches = rig.net.describe_launches(batch, conc)
    got = covered_rows(launches, prefix)
    assert set(rows) <= got, (prefix, sorted(rows), sorted(got), [(r["layer"], r["kernel"]) for r in launches])


# ---- the tiny net: every regime, ring / split-K kernels (mode 0) and the shift kernels (mode 2) -------------------------------------
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("regime", ["wrap", "saturate", "spread", "shift22", "shift23", "expand32"])
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
    for regime, mode in (("wrap", 0), ("saturate", 0), ("spread", 0), ("shift23", 2)):
        q, model = synth.synth_extreme(t, 7, regime)
        Rig(t, q, model, mode).check_all_layers(synth.synth_extreme_images(t, 2, 7))


# ---- ResNet-50: every row extreme (spread: rows 14 and 30), one route per kernel family (tests/test_extreme_regimes.py R50_ROUTES) --------
@pytest.fixture(scope="module")
def r50_models():
    return {}


def _r50(models, regime):
    if regime not in models:
        models[regime] = r50_extreme(regime)
    return models[regime]


@pytest.mark.parametrize("regime,route", [(g, r) for g in ("wrap", "saturate", "spread") for r in R50_ROUTES[g]])
def test_resnet50_extreme_rows(r50_models, regime, route, monkeypatch):
    opts, B, conc, want = R50_ROUTES[regime][route]
    set_opts(monkeypatch, **opts)
    rig = Rig(*_r50(r50_models, regime), 0)
    for prefix, rows in want.items():
        _runs(rig, B, prefix, rows, conc)
    rig.check_all_layers(synth.synth_extreme_images(rig.t, B, 1))


@pytest.mark.parametrize("switch", ["nofast", "nosemi", "nodual"])
def test_resnet50_wrap_rows_epilogue_forms(r50_models, switch, monkeypatch):
    set_opts(monkeypatch, **{switch: "1"})
    rig = Rig(*_r50(r50_models, "wrap"), 0)
    rig.check_all_layers(synth.synth_extreme_images(rig.t, 2, 3))


@pytest.mark.parametrize("graph", [False, True])
def test_resnet50_wrap_four_batches_in_flight(r50_models, graph):
    """The bench configuration (four runners, four streams, HIP graph replay) on the wrap model: every logits row of the last steps
    against a serial run, the serial run against the oracle."""
    from tests.test_gpu_configs import _in_flight
    rig = Rig(*_r50(r50_models, "wrap"), 0)
    _in_flight(rig, 8, 4, 12, graph, 900)


# ---- SqueezeNet (fire modules, merged rows, the shift kernels' classifier), small VGG16 (conv_c3, conv_fc) ---------------------------
@pytest.mark.parametrize("regime", ["wrap", "saturate", "spread"])
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


_BODY_WANT = {2: ({"conv_bneck": {5, 6, 8, 9}, "conv_c3_kernel": {1, 2}}, {"conv_mfma_sk": {1, 2, 5}}),
              5: ({"conv_c3_kernel": {1, 2}, "fc4_partial": {5}}, {"conv_mfma_sk": {1, 2}}),
              9: ({"conv_bneck": {4, 5}, "conv_c3_kernel": {1}, "fc4_partial": {6}}, {"conv_mfma_sk": {1, 2, 4}})}


@pytest.mark.parametrize("seed", [2, 5, 9])
@pytest.mark.parametrize("regime", ["wrap", "saturate", "spread"])
def test_body_programs_at_the_extremes(seed, regime, monkeypatch):
    from tests.test_fuzz_programs import _BODY_OPTS, random_body_program
    set_opts(monkeypatch, **_BODY_OPTS)
    t = random_body_program(seed)
    q, model = synth.synth_extreme(t, seed, regime)
    rig = Rig(t, q, model, 0)
    for prefix, rows in _BODY_WANT[seed][regime == "spread"].items():       # (spread rows: the split-K kernel)
        _runs(rig, 2, prefix, rows)
    rig.check_all_layers(synth.synth_extreme_images(t, 2, seed))
