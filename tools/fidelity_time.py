#!/usr/bin/env python3
"""Cost of the layer comparison (tf2_fid_run / tf2_fid_kept, csrc/act_fidelity.hip) behind a ResNet-50 keep_all step (synthetic weights,
shipped resnet50_Q, float32 images), batch 32 by default: four HIP graphs captured in one process over the same static image and
reference buffers, each replay between its own pair of HIP events, in interleaved rounds so that clock and thermal drift fall on all of
them equally,
  keep_all      the keep_all step alone (Runner.run_batch(keep_all=True))
  audit         tf2_audit_kept: the audit kernels alone on the maps the step left -- the yardstick: comparable counting per value
  fid           tf2_fid_kept: the comparison kernels alone on the same maps against the float references
  with_fid      tf2_fid_run: the step, then the comparison
and once, in wall time, what the tree could do before: Runner.read_layer of every row to the host plus fidelity.reference_compare --
which is also the check that the store of the timed replays is the statement times the number of replays (--no-host leaves it out).
Medians and minima over --rounds x --replays replays after --warmup replays of each graph.  The bytes are the values
tf2_fid_describe lists: one byte a value of an int8 row plus four of its float reference; the input row reads its floats once (the
audit: one byte a row value, four an image value).  Prints one JSON line and writes it to --out (default
profiles/fidelity_time_b<batch>.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the host path (read_layer + reference_compare) and the store check")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tf2_amd import audit as A, config as cfg, fidelity as F, synth
    from tf2_amd._observe import capture_graph
    from tf2_amd.network import NetWork, Runner
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = "cuda:0"
    t = cfg.resnet50_tables()
    q = np.loadtxt(os.path.join(ROOT, "tests", "golden", "resnet50_Q"), dtype=np.int32)
    model = synth.synth_model(t, q, 0)
    net = NetWork(t)
    net.Init(model, synth.q_text(q), device=dev)
    B = a.batch
    x_host = synth.synth_images(t, B, 0, kind="float")
    x = torch.from_numpy(np.ascontiguousarray(x_host)).to(dev)
    refs = F.float_refs(t, model, x, device=dev)
    torch.cuda.synchronize()
    cmp_ = F.DeviceComparator(net, B)
    aud = A.DeviceAuditor(net, B)
    runner = Runner(None, net)

    graphs = {"keep_all": capture_graph(lambda: runner.run_batch(x, keep_all=True), dev).replay,
              "audit": aud.capture(x, kept_only=True),
              "fid": cmp_.capture(x, refs, kept_only=True),
              "with_fid": cmp_.capture(x, refs)}
    s = torch.cuda.current_stream()

    def timed(replay, n):
        out = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            replay()
            e1.record(s)
            out.append((e0, e1))
        torch.cuda.synchronize()
        return [p.elapsed_time(r) for p, r in out]

    graphs["with_fid"]()                                    # the maps the kept-only graphs read (both workspaces hold the same step)
    aud.observe(x)
    for g in graphs.values():
        timed(g, a.warmup)
    cmp_.reset()
    ms = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, g in graphs.items():
            ms[k] += timed(g, a.replays)
    torch.cuda.synchronize()
    rows = cmp_.rows()
    store = cmp_.store()
    seen = 2 * a.rounds * a.replays                         # the timed replays of both comparison graphs, nothing else
    for r in rows:
        first = r["offset"] // (F.SLOTS * 8)
        assert (store[first:first + r["C"], F.N] + store[first:first + r["C"], F.NONFINITE] == seen * B * r["H"] * r["W"]).all(), r
    logits_plain = runner.run_batch(x, keep_all=True).cpu().numpy()
    torch.cuda.synchronize()

    host_s = None
    if not a.no_host:                                       # the path the tree had: every row to the host, then numpy
        t0 = time.perf_counter()
        maps = [runner.read_layer(l, B) for l in range(net.num_layer)]
        t1 = time.perf_counter()
        host_refs = [r.cpu().numpy() for r in refs]
        qr = F.q_rows_of_net(net)
        one = F.reference_compare(maps, host_refs, qr, images=x_host, q0=int(qr[-1][0]))
        t2 = time.perf_counter()
        host_s = dict(read_layer_s=t1 - t0, reference_compare_s=t2 - t1, total_s=t2 - t0)
        want = one * seen
        want[:, F.MAX_ABS_D] = one[:, F.MAX_ABS_D]
        assert np.array_equal(store, want), "the store of the timed replays is not the statement times the replays"
    assert np.array_equal(cmp_.observe(x, refs).cpu().numpy(), logits_plain)

    values = sum(B * r["H"] * r["W"] * r["C"] for r in rows[1:])
    image_values = B * rows[0]["C"] * rows[0]["H"] * rows[0]["W"]
    fid_bytes = 5 * values + 4 * image_values
    audit_bytes = values + 4 * image_values
    med = {k: float(np.median(v)) for k, v in ms.items()}
    mn = {k: float(np.min(v)) for k, v in ms.items()}
    res = dict(network="resnet50", batch=B, images="float32", replays_each=a.rounds * a.replays,
               keep_all_step_ms=med["keep_all"], audit_kept_ms=med["audit"], fid_kept_ms=med["fid"], fid_run_ms=med["with_fid"],
               keep_all_step_ms_min=mn["keep_all"], audit_kept_ms_min=mn["audit"], fid_kept_ms_min=mn["fid"], fid_run_ms_min=mn["with_fid"],
               step_delta_ms=med["with_fid"] - med["keep_all"], fid_share_of_step_pct=100.0 * med["fid"] / med["keep_all"],
               rows=len(rows), records=int(store.shape[0]), int8_bytes=int(values), float_bytes=int(4 * values + 4 * image_values),
               fid_bytes=int(fid_bytes), audit_bytes=int(audit_bytes),
               fid_gb_per_s=fid_bytes / (med["fid"] * 1e-3) / 1e9, audit_gb_per_s=audit_bytes / (med["audit"] * 1e-3) / 1e9,
               fid_values_per_ns=(values + image_values) / (med["fid"] * 1e6), audit_values_per_ns=(values + image_values) / (med["audit"] * 1e6),
               hbm_peak_gb_per_s=HBM_TBS * 1e3, host_path=host_s, store_checked=not a.no_host,
               slab=F.SLAB, chans=F.CHANS, tile=F.TILE, rows_per_launch=F.ROWS_PER_LAUNCH)
    res["fid_not_below_audit_rate"] = bool(res["fid_gb_per_s"] >= res["audit_gb_per_s"])
    res["fid_pct_of_hbm_peak"] = 100.0 * res["fid_gb_per_s"] / res["hbm_peak_gb_per_s"]
    line = json.dumps(res)
    print(line)
    out = a.out or os.path.join(ROOT, "profiles", f"fidelity_time_b{B}.json")
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
