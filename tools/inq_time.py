#!/usr/bin/env python3
"""Cost of INQ weight quantisation on the device (tf2_inq_step, csrc/weight_inq.hip) on ResNet-50's LoadModel stream
(synth.bench_network("resnet50"), every filter replaced by seeded Gaussians; filters and biases are the segments):
  full      one step at cur = 1 from an all-float mask
  incr      one step 0.5 -> 0.75 from the masks a 0 -> 0.5 step left
each a HIP graph (DeviceQuantizer.capture) replayed between its own pair of HIP events after the buffers were refilled, median over
--replays, each case in a child process of its own under a time limit;
  numpy     tf2_amd.inq.reference_model_step (the numpy statement) on this host, the same two steps, once each
  reference (--reference PATH, where the reference lies) its own ComputeQuantumRange + ShapeIntoTwoPower -- three Python loops an
            element -- timed on ONE tensor of --ref-elems elements and extrapolated linearly to the stream's segment elements
Bytes moved, as the kernels are written: five bytes (weight + mask) an element read by the range pass, by each of the four select
passes and by the shape pass, five written for every group of four that holds a selected weight; the rate is those bytes over the
time beside the chip's 8 TB/s.  Writes one JSON object to --out (default profiles/inq_time.json); a case run alone merges into it."""
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
    from tf2_amd import inq, synth
    t, q, seed, _, _ = synth.bench_network("resnet50")
    model = synth.synth_model(t, q, seed).copy()
    rng = np.random.default_rng(7)
    for _, o, n in inq.segments_of(t, ("filter",)):
        model[o:o + n] = (rng.standard_normal(n) * 0.05).astype(np.float32)
    return t, model


def device_case(case, replays, warmup):
    import torch
    from tf2_amd import inq
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    t, model = float_stream()
    dq = inq.DeviceQuantizer(t)
    n_seg = sum(c for _, c in dq.segs)
    mk = np.zeros(model.size, np.uint8)
    for o, c in dq.segs:
        mk[o:o + c] = 1
    w0, m0 = torch.from_numpy(model).to("cuda:0"), torch.from_numpy(mk).to("cuda:0")
    prev, cur = (0.0, 1.0) if case == "full" else (0.5, 0.75)
    if case == "incr":
        dq.step(w0, m0, 0.0, 0.5)
        torch.cuda.synchronize()
    w, m = w0.clone(), m0.clone()
    replay = dq.capture(w, m, prev, cur)
    s = torch.cuda.current_stream()
    ms = []
    for i in range(warmup + replays):
        w.copy_(w0); m.copy_(m0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s); replay(); e1.record(s)
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    st = dq.state()
    assert not st["status"].any()
    changed = (m.cpu().numpy() != m0.cpu().numpy())
    pad = (-changed.size) % 4
    groups = int(np.concatenate([changed, np.zeros(pad, bool)]).reshape(-1, 4).any(1).sum())
    moved = 6 * 5 * n_seg + 5 * 4 * groups
    med = float(np.median(ms))
    return {f"{case}_step_ms": med, f"{case}_step_ms_min": float(np.min(ms)), f"{case}_bytes_moved": int(moved),
            f"{case}_gb_per_s": moved / (med * 1e-3) / 1e9, f"{case}_pct_of_hbm_peak": 100.0 * moved / (med * 1e-3) / 1e9 / (HBM_TBS * 1e3),
            f"{case}_weights_quantised": int(changed.sum()), "segments": len(dq.segs), "segment_elements": int(n_seg),
            "stream_elements": int(model.size), "replays_each": replays, "hbm_peak_gb_per_s": HBM_TBS * 1e3}


def numpy_case():
    from tf2_amd import inq
    t, model = float_stream()
    t0 = time.perf_counter()
    full = inq.reference_model_step(t, model, None, 0.0, 1.0)
    t1 = time.perf_counter()
    a, m, _, _ = inq.reference_model_step(t, model, None, 0.0, 0.5)
    t2 = time.perf_counter()
    inq.reference_model_step(t, a, m, 0.5, 0.75)
    t3 = time.perf_counter()
    assert not full[1].any()
    return {"numpy_full_step_s": t1 - t0, "numpy_incr_step_s": t3 - t2}


def reference_case(root, elems):
    import contextlib
    import io
    from tf2_amd import inq
    sys.path.insert(0, os.path.join(root, "TransForm_Kit", "Compression", "compress_net", "core"))
    import compress_core
    t, model = float_stream()
    n_seg = sum(c for _, _, c in inq.segments_of(t))
    w = (np.random.default_rng(8).standard_normal(elems) * 0.05).astype(np.float32)
    mask = np.ones(elems)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        mx, mn = compress_core.ComputeQuantumRange(w, mask, 7)
        compress_core.ShapeIntoTwoPower(w, mask, 0.0, 1.0, mx, mn)
    dt = time.perf_counter() - t0
    return {"reference_loops_elems_timed": int(elems), "reference_loops_s_timed": dt,
            "reference_loops_full_step_s_extrapolated": dt / elems * n_seg,
            "reference_loops_note": "one tensor timed on the host that ran this case, extrapolated linearly to segment_elements"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=["all", "full", "incr", "numpy", "reference"])
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--reference", default=None, help="root of the reference tree (case reference)")
    ap.add_argument("--ref-elems", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inq_time.json"))
    a = ap.parse_args()
    if a.case == "all":
        for case in ("full", "incr", "numpy") + (("reference",) if a.reference else ()):
            cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--replays", str(a.replays), "--warmup", str(a.warmup), "--out", a.out,
                   "--ref-elems", str(a.ref_elems)] + (["--reference", a.reference] if a.reference else [])
            subprocess.run(cmd, check=True, timeout=a.limit)
        print(open(a.out).read().strip())
        return
    res = json.load(open(a.out)) if os.path.exists(a.out) else {"network": "resnet50"}
    if a.case in ("full", "incr"):
        res.update(device_case(a.case, a.replays, a.warmup))
    elif a.case == "numpy":
        res.update(numpy_case())
    else:
        assert a.reference, "--reference PATH"
        res.update(reference_case(a.reference, a.ref_elems))
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k.startswith(a.case)}))


if __name__ == "__main__":
    main()
