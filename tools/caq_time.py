#!/usr/bin/env python3
"""Cost of the two calibration passes (tf2_caq_range / tf2_caq_error, csrc/act_caq.hip) on the float maps of a ResNet-50 float forward
(synthetic weights, float32 images), batch 32 by default.  One job, the same device tensors for every figure, the float forward
excluded from all of them:
  range       pass 1 as a HIP graph (tf2_caq_range over the images and every row)
  error       pass 2 as a HIP graph (tf2_caq_error against Qb = q_max of pass 1)
  calibrator  calibrate.Calibrator's own update of its element-wise maximum over the same maps (abs / amax / maximum per row, eager, as
              Calibrator.observe issues them), and the host time of its q_rows()
  fid         tf2_fid_kept, the comparison of tools/fidelity_time.py, on the same references: the yardstick for a float-map reader on
              this machine (it reads an int8 map beside every float map: its bytes are 5 a value)
Each graph replay (and each eager update) runs between its own pair of HIP events, in interleaved rounds so that clock and thermal drift
fall on all of them equally; medians and minima over --rounds x --replays after --warmup.  The check that the timed stores mean
something: n + nonfinite of every channel is the replays times its values, and q_rows(q_max(RANGE store)) equals the Calibrator's
q_rows() on the same maps.  Prints one JSON line and writes it to --out (default profiles/caq_time_b<batch>.json)."""
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tf2_amd import calibrate, caq as Q, config as cfg, fidelity as F, synth
    from tf2_amd.network import NetWork
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = "cuda:0"
    t = cfg.resnet50_tables()
    q = np.loadtxt(os.path.join(ROOT, "tests", "golden", "resnet50_Q"), dtype=np.int32)
    model = synth.synth_model(t, q, 0)
    B = a.batch
    x = torch.from_numpy(np.ascontiguousarray(synth.synth_images(t, B, 0, kind="float"))).to(dev)
    outs = calibrate.float_forward(t, model, x, dev)
    refs = F.float_refs(t, model, x, device=dev)
    torch.cuda.synchronize()

    cal = Q.DeviceCalibrator(t, tuple(x.shape[1:]), dev)
    cal.observe(x, refs)
    cal.set_base(Q.q_max(cal.range_store()))
    net = NetWork(t)
    net.Init(model, synth.q_text(q), device=dev)
    cmp_ = F.DeviceComparator(net, B)
    cmp_.observe(x, refs)                                   # the kept maps tf2_fid_kept reads
    host_cal = calibrate.Calibrator(t, model, device=dev)

    def update():                                           # Calibrator.observe behind its float forward
        for k, v in outs.items():
            m = v.abs().amax(dim=0, keepdim=True)
            host_cal.maxabs[k] = m if k not in host_cal.maxabs else torch.maximum(host_cal.maxabs[k], m)

    steps = {"range": cal.capture(x, refs), "error": cal.capture(x, refs, error=True), "calibrator": update,
             "fid": cmp_.capture(x, refs, kept_only=True)}
    s = torch.cuda.current_stream()

    def timed(step, n):
        out = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            step()
            e1.record(s)
            out.append((e0, e1))
        torch.cuda.synchronize()
        return [p.elapsed_time(r) for p, r in out]

    for g in steps.values():
        timed(g, a.warmup)
    cal.reset()
    ms = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, g in steps.items():
            ms[k] += timed(g, a.replays)
    torch.cuda.synchronize()

    seen = a.rounds * a.replays
    rng, err = cal.range_store(), cal.error_store()
    values = np.concatenate([np.full(r["C"], B * r["HW"]) for r in cal.rows])
    assert (rng[:, Q.N] + rng[:, Q.NONFINITE] == seen * values).all() and (err[:, Q.E_N] + err[:, Q.E_NONFINITE] == seen * values).all()
    t0 = time.perf_counter()
    want = host_cal.q_rows()
    q_rows_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = Q.q_rows(cal.plan, Q.q_max(rng))
    rule_s = time.perf_counter() - t0
    assert sorted(got) == sorted(want) and all(np.array_equal(got[k], want[k]) for k in want), "q_max of the store is not the Calibrator's Q"
    mse = Q.q_mse(err, cal.qb)

    n_values = int(values.sum())
    med = {k: float(np.median(v)) for k, v in ms.items()}
    mn = {k: float(np.min(v)) for k, v in ms.items()}
    tbs = lambda nbytes, k: nbytes / (med[k] * 1e-3) / 1e12
    fid_values = sum(B * r["H"] * r["W"] * r["C"] for r in cmp_.rows()[1:])
    fid_bytes = 5 * fid_values + 4 * B * int(np.prod(x.shape[1:]))
    res = dict(network="resnet50", batch=B, images="float32", replays_each=seen, records=int(rng.shape[0]), rows=len(cal.rows),
               float_values=n_values, float_bytes=4 * n_values,
               range_ms=med["range"], error_ms=med["error"], calibrator_update_ms=med["calibrator"], fid_kept_ms=med["fid"],
               range_ms_min=mn["range"], error_ms_min=mn["error"], calibrator_update_ms_min=mn["calibrator"], fid_kept_ms_min=mn["fid"],
               range_bytes=4 * n_values, error_bytes=4 * n_values, fid_bytes=int(fid_bytes),
               range_tb_per_s=tbs(4 * n_values, "range"), error_tb_per_s=tbs(4 * n_values, "error"), fid_tb_per_s=tbs(fid_bytes, "fid"),
               fid_float_tb_per_s=tbs(4 * n_values, "fid"), calibrator_map_tb_per_s=tbs(4 * n_values, "calibrator"),
               calibrator_q_rows_host_s=q_rows_s, caq_rule_host_s=rule_s, calibrator_maxabs_bytes=4 * n_values // B,
               q_max_equals_calibrator=True, mse_channels_above_base=int((mse > cal.qb).sum()),
               hbm_peak_tb_per_s=HBM_TBS, slab=Q.SLAB, rows_per_launch=Q.ROWS_PER_LAUNCH)
    res["range_not_below_fid_float_rate"] = bool(res["range_tb_per_s"] >= res["fid_float_tb_per_s"])
    line = json.dumps(res)
    print(line)
    out = a.out or os.path.join(ROOT, "profiles", f"caq_time_b{B}.json")
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
