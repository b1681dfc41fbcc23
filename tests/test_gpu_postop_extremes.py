"""GPU parity of the max pools and global averages at their extremes: the post-op regimes of tf2_amd/synth.py (synth_postop) on the
post-op programs of tf2_amd/config.py, every layer and the logits against the oracle, on each kernel that pools or averages.  Each case
first checks in the launch plan that its rows run on the kernel it is about (tests/test_postop_extremes.py POSTOP_ROUTES, where the plans
are also checked without a device).  Batches of 1-3 keep the oracle fast."""
import pytest

from tf2_amd import synth
from tests.conftest import set_opts
from tests.test_gpu_extremes import _runs
from tests.test_gpu_parity import Rig
from tests.test_postop_extremes import POSTOP_ROUTES, postop_model

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("route", sorted(POSTOP_ROUTES))
def test_postop_route_at_the_extremes(route, monkeypatch):
    mk, regime, rows, mode, opts, B, conc, want = POSTOP_ROUTES[route]
    set_opts(monkeypatch, **opts)
    t, q, model = postop_model(route)
    rig = Rig(t, q, model, mode)
    for prefix, r in want.items():
        _runs(rig, B, prefix, r, conc)
    rig.check_all_layers(synth.synth_extreme_images(t, B, 2))


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("route", ["r50_stem_relu0", "r50_sk_avg_signed"])
def test_signed_stem_and_sk_average_in_flight(route, graph, monkeypatch):
    """Four runners on four streams, batches in flight (launched, or replayed from captured HIP graphs): the signed stem pool and the
    signed split-K average (avg_fuse=1 keeps it fused in flight) against a serial run, the serial run against the oracle."""
    from tests.test_gpu_configs import _in_flight
    mk, regime, rows, mode, opts, B, conc, want = POSTOP_ROUTES[route]
    set_opts(monkeypatch, avg_fuse="1", **opts)
    rig = Rig(*postop_model(route), mode)
    for prefix, r in want.items():
        _runs(rig, 2, prefix, r, 1)
    _in_flight(rig, 2, 4, 12, graph, 910)
