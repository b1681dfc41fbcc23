#!/usr/bin/env python3
"""Cost of the activation audit (tf2_audit_run, csrc/act_audit.hip) behind a ResNet-50 keep_all step (synthetic weights, shipped
resnet50_Q), batch 32 by default: three HIP graphs captured in one process over the same static image buffer, each replay between its
own pair of HIP events, in interleaved rounds so that clock and thermal drift fall on all three equally,
  keep_all      the keep_all step alone (Runner.run_batch(keep_all=True)): what the tree could do before the audit, the yardstick
  with_audit    tf2_audit_run: the same step, then the audit kernels (DeviceAuditor.capture)
  audit         tf2_audit_kept: the audit kernels alone on the maps the step left (DeviceAuditor.capture(kept_only=True))
Medians over --rounds x --replays replays after --warmup replays of each graph.  The bytes audited are the values tf2_audit_describe
lists (batch x H x W x C an int8 row; four bytes a value for float images), the rate is bytes / audit time beside the chip's 8 TB/s.
The store is checked at the end: every record's n is the number of replays times the row's values a channel.  Prints one JSON line
and writes it to --out (default profiles/act_audit_time_b<batch>.json)."""
import argparse
import json
import os
import sys

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
    ap.add_argument("--int8", action="store_true", help="int8 images instead of float32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tf2_amd import audit as A, config as cfg, synth
    from tf2_amd._observe import capture_graph
    from tf2_amd.network import NetWork, Runner
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = "cuda:0"
    t = cfg.resnet50_tables()
    q = np.loadtxt(os.path.join(ROOT, "tests", "golden", "resnet50_Q"), dtype=np.int32)
    net = NetWork(t)
    net.Init(synth.synth_model(t, q, 0), synth.q_text(q), device=dev)
    B = a.batch
    x = torch.from_numpy(np.ascontiguousarray(synth.synth_images(t, B, 0, kind="int8" if a.int8 else "float"))).to(dev)
    aud = A.DeviceAuditor(net, B)
    runner = Runner(None, net)

    graphs = {"keep_all": capture_graph(lambda: runner.run_batch(x, keep_all=True), dev).replay,
              "with_audit": aud.capture(x),
              "audit": aud.capture(x, kept_only=True)}
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

    graphs["with_audit"]()                                  # the maps the audit-alone graph reads
    for g in graphs.values():
        timed(g, a.warmup)
    aud.reset()
    ms = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, g in graphs.items():
            ms[k] += timed(g, a.replays)
    torch.cuda.synchronize()
    # the store saw the timed replays of both audit graphs, nothing else
    rows = aud.rows()
    store = aud.store()
    seen = 2 * a.rounds * a.replays
    for r in rows:
        first = r["offset"] // 128
        assert (store[first:first + r["C"], 0] == seen * B * r["H"] * r["W"]).all(), r
    logits_plain = runner.run_batch(x, keep_all=True).cpu().numpy()
    assert np.array_equal(aud.observe(x).cpu().numpy(), logits_plain)

    values = sum(B * r["H"] * r["W"] * r["C"] for r in rows[1:])
    image_bytes = B * rows[0]["C"] * rows[0]["H"] * rows[0]["W"] * (1 if a.int8 else 4)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = dict(network="resnet50", batch=B, images="int8" if a.int8 else "float32", replays_each=a.rounds * a.replays,
               keep_all_step_ms=med["keep_all"], with_audit_step_ms=med["with_audit"], audit_alone_ms=med["audit"],
               keep_all_step_ms_min=float(np.min(ms["keep_all"])), with_audit_step_ms_min=float(np.min(ms["with_audit"])),
               audit_alone_ms_min=float(np.min(ms["audit"])),
               step_delta_ms=med["with_audit"] - med["keep_all"], audit_share_of_step_pct=100.0 * med["audit"] / med["keep_all"],
               rows=len(rows), records=int(store.shape[0]), doubled_channels=int(sum(r["n_doubled"] for r in rows)),
               audited_bytes=int(values + image_bytes), workspace_bytes=int(aud._ws.numel()),
               audit_gb_per_s=(values + image_bytes) / (med["audit"] * 1e-3) / 1e9, hbm_peak_gb_per_s=HBM_TBS * 1e3,
               slab=A.SLAB, chans=A.CHANS, rows_per_launch=A.ROWS_PER_LAUNCH)
    res["audit_pct_of_hbm_peak"] = 100.0 * res["audit_gb_per_s"] / res["hbm_peak_gb_per_s"]
    line = json.dumps(res)
    print(line)
    out = a.out or os.path.join(ROOT, "profiles", f"act_audit_time_b{B}.json")
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
