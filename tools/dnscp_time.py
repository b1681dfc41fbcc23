#!/usr/bin/env python3
"""Cost of DNS channel pruning on the device (tf2_dnscp_step, csrc/weight_dnscp.hip) on ResNet-50's LoadModel stream
(synth.bench_network("resnet50"), every filter replaced by seeded Gaussians with three input channels in ten scaled down; the 32
prunable convs of dnscp.prunable_rows are the descriptors, thresholds from tf2_dnscp_stats):
  step      one step with every conv updated, out_dev beside dense_dev: a HIP graph (DevicePruner.capture) replayed between its own
            pair of HIP events after the keep bytes were set back, median over --replays
  numpy     tf2_amd.dnscp.reference_model_step (the numpy statement) on this host, the same step, once
  torch     the reference's expression of the step in torch on this host's CPU -- per conv abs().sum(3).sum(2).sum(0) of the weights and of a
            dense mask, a Python loop over the channels with mask[:, c] = 0 / 1 writes, the two fix-up loops, weight * mask -- once
each case in a child process of its own under a time limit.  Bytes moved, as the kernels are written: four bytes an element of the
prunable convs read by the max pass, by the sum pass and by the apply pass, four written by the apply pass; the rate is those bytes
over the time beside the chip's 8 TB/s.  Writes one JSON object to --out (default profiles/dnscp_time.json); a case run alone merges
into it."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS = 8.0


def float_stream():
    from tf2_amd import dnscp, synth
    t, q, seed, _, _ = synth.bench_network("resnet50")
    model = synth.synth_model(t, q, seed).copy()
    rng = np.random.default_rng(7)
    lay = dnscp._filter_layout(t)
    for l, (o, N, C, kk) in lay.items():
        scale = np.where(rng.random(C) < 0.3, 0.1, 1.0)
        model[o:o + N * C * kk] = (rng.standard_normal((N, C, kk)) * 0.05 * scale[None, :, None]).astype(np.float32).ravel()
    return t, model, lay


def host_thresholds(t, model, lay):
    from tf2_amd import dnscp
    return {l: dnscp.thresholds(dnscp.reference_stats(model[lay[l][0]:lay[l][0] + lay[l][1] * lay[l][2] * lay[l][3]].reshape(lay[l][1:]))[1])
            for l in dnscp.prunable_rows(t)}


def device_case(replays, warmup):
    import torch
    from tf2_amd import dnscp
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    t, model, _ = float_stream()
    dp = dnscp.DevicePruner(t)
    n_conv = sum(N * C * kk for _, N, C, kk in dp.convs)
    dense = torch.from_numpy(model).to("cuda:0")
    out = dense.clone()
    dp.stats(dense)
    dp.thresholds()
    replay = dp.capture(dense, out)
    s = torch.cuda.current_stream()
    ms = []
    for i in range(warmup + replays):
        dp.keep_dev.fill_(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s); replay(); e1.record(s)
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    st = dp.state()
    assert not st["status"].any() and (st["kept_after"] % 16 == 0).all()
    moved = 16 * n_conv
    med = float(np.median(ms))
    return {"step_ms": med, "step_ms_min": float(np.min(ms)), "step_bytes_moved": int(moved), "step_gb_per_s": moved / (med * 1e-3) / 1e9,
            "step_pct_of_hbm_peak": 100.0 * moved / (med * 1e-3) / 1e9 / (HBM_TBS * 1e3), "step_channels_kept": int(st["kept_after"].sum()),
            "channels": int(dp.n_channels), "convs": len(dp.convs), "conv_elements": int(n_conv), "stream_elements": int(model.size),
            "replays_each": replays, "hbm_peak_gb_per_s": HBM_TBS * 1e3}


def numpy_case():
    from tf2_amd import dnscp
    t, model, lay = float_stream()
    th = host_thresholds(t, model, lay)
    t0 = time.perf_counter()
    _, keeps, _, recs = dnscp.reference_model_step(t, model, None, th)
    dt = time.perf_counter() - t0
    return {"numpy_step_s": dt, "numpy_channels_kept": int(recs["kept_after"].sum())}


def torch_case():
    import torch
    from tf2_amd import dnscp
    t, model, lay = float_stream()
    th = host_thresholds(t, model, lay)
    rows = dnscp.prunable_rows(t)
    params = [torch.from_numpy(model[lay[l][0]:lay[l][0] + lay[l][1] * lay[l][2] * lay[l][3]].reshape(lay[l][1], lay[l][2], 1, lay[l][3]).copy()) for l in rows]
    masks = [torch.ones_like(p) for p in params]
    kept = 0
    t0 = time.perf_counter()
    for l, p, mask in zip(rows, params, masks):
        t_lo, t_hi = th[l]
        C = p.shape[1]
        per = p.numel() / C
        mean_w = torch.abs(p).sum(3).sum(2).sum(0) / per
        mean_m = torch.abs(mask).sum(3).sum(2).sum(0) / per
        for c in range(C):
            if mean_m[c] == 1 and mean_w[c] <= t_lo:
                mask[:, c, :, :] = 0
            elif mean_m[c] == 0 and mean_w[c] > t_hi:
                mask[:, c, :, :] = 1
        mean_m = torch.abs(mask).sum(3).sum(2).sum(0) / per
        nz = int(torch.nonzero(mean_m).size()[0])
        target = round(nz / 16) * 16 or 16
        for want, put, n in ((0, 1, target - nz), (1, 0, nz - target)):
            for c in range(C):
                if n > 0 and mean_m[c] == want:
                    mask[:, c, :, :] = put
                    n -= 1
        p.mul_(mask)
        kept += int(torch.nonzero(torch.abs(mask).sum(3).sum(2).sum(0)).size()[0])
    dt = time.perf_counter() - t0
    return {"torch_loop_step_s": dt, "torch_loop_channels_kept": kept, "torch_loop_threads": int(torch.get_num_threads()),
            "torch_loop_note": "float32 sums on the CPU of the host that ran this case; a mean within float32 rounding of a threshold may fall the other way"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=["all", "step", "numpy", "torch"])
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dnscp_time.json"))
    a = ap.parse_args()
    if a.case == "all":
        for case in ("step", "numpy", "torch"):
            cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--replays", str(a.replays), "--warmup", str(a.warmup), "--out", a.out]
            subprocess.run(cmd, check=True, timeout=a.limit)
        print(open(a.out).read().strip())
        return
    res = json.load(open(a.out)) if os.path.exists(a.out) else {"network": "resnet50"}
    res.update({"step": lambda: device_case(a.replays, a.warmup), "numpy": numpy_case, "torch": torch_case}[a.case]())
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k.startswith(a.case)}))


if __name__ == "__main__":
    main()
