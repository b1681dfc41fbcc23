#!/usr/bin/env python3
"""Cost of the all-pairs histogram kernel (tf2_emb_roc_hist, embed_roc.hip) next to the tree's other distance kernel, stage 1 of
tf2_emb_match (match_slab_kernel), in ONE process on one build; D = 128, random unit rows, ten rows an identity.
  roc           one DeviceRoc.add(rows, ids) in self mode at every N of --rows (13 233: LFW's images; 100 000), HIP events on one
                stream: the median of --launches event pairs after warm-up, and --launches back-to-back calls between one pair
                divided by their number.  Nanoseconds per distance = back-to-back time / (N (N - 1) / 2).  The histogram is read
                back once at the end and its sum compared with the pairs of all the launches.
  match         one tf2_emb_match call as tools/embed_time.py times it (SqueezeNet 1.1 outputs of --batch images, top 5, ids, ground
                truth and tally, --match-rows gallery rows), timed the same way.  The call is embed + stage 1 + stage 2, so its time
                per distance (batch x rows distances) is an UPPER bound of stage 1's.
Prints one JSON line (and writes it to --out).  Stage 1's own time, and the all-pairs kernel's, come from the kernel trace of a second
run of this tool under the profiler (tracing slows the host: the event timings above are taken with it off):
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/embed_roc_time.py --launches 5 --match-launches 100
  python tools/embed_roc_time.py --merge-trace DIR/.../*_kernel_trace.csv --out profiles/embed_roc_time.json
The second command runs no device code: it adds `kernel` (the median of each kernel's dispatches, the all-pairs kernel's grouped by
grid size, in microseconds and in nanoseconds per distance) and `roc_over_stage1` (the ratio of the two per-distance times at
--match-rows rows, kernel against kernel) to the JSON of the first run."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def merge_trace(a):
    res = json.load(open(a.out))
    hist, slab = {}, []
    with open(a.merge_trace, newline="") as f:
        for r in csv.DictReader(f):
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            if "roc_hist_kernel" in r["Kernel_Name"]:
                hist.setdefault(int(r.get("Grid_Size_X") or r["Grid_Size"]), []).append(us)
            elif "match_slab_kernel" in r["Kernel_Name"]:
                slab.append(us)
    rows = sorted(int(n) for n in res["roc_us"])
    if len(hist) != len(rows) or not slab:
        raise SystemExit(f"the trace has {len(hist)} grid sizes of roc_hist_kernel for {len(rows)} row counts, {len(slab)} stage-1 dispatches")
    k = dict(roc_hist_kernel={}, match_slab_kernel={})
    for n, grid in zip(rows, sorted(hist)):                            # more rows, a larger grid
        us = float(np.median(hist[grid]))
        k["roc_hist_kernel"][str(n)] = dict(dispatches=len(hist[grid]), median_us=round(us, 2), min_us=round(min(hist[grid]), 2),
                                            ns_per_distance=round(us * 1e3 / (n * (n - 1) / 2), 6))
    us = float(np.median(slab))
    k["match_slab_kernel"] = dict(dispatches=len(slab), median_us=round(us, 2), min_us=round(min(slab), 2), batch=res["batch"], rows=res["match_rows"],
                                  ns_per_distance=round(us * 1e3 / (res["batch"] * res["match_rows"]), 6))
    res["kernel"] = k
    res["roc_over_stage1"] = {n: round(v["ns_per_distance"] / k["match_slab_kernel"]["ns_per_distance"], 3) for n, v in k["roc_hist_kernel"].items()}
    emit(res, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="13233,100000")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--match-rows", type=int, default=100000)
    ap.add_argument("--n-thr", type=int, default=400)
    ap.add_argument("--step", type=float, default=0.01)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--match-launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--merge-trace", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace(a)
    import torch
    from tf2_amd import embed as E, synth
    from tf2_amd.network import NetWork, Runner
    dev = "cuda:0"
    t, q, seed = synth.bench_network("squeezenet")[:3]
    net = NetWork(t)
    net.Init(synth.synth_model(t, q, seed), synth.q_text(q), device=dev)
    D, k = int(net.plan[-1].N), 5
    rows = [int(v) for v in a.rows.split(",")]
    cap = max(rows + [a.match_rows])
    rng = np.random.default_rng(3)
    # unit rows (the statement's embeddings of random int8 outputs), ten rows an identity: as tools/embed_time.py
    gal = E.Gallery(cap, D, dev)
    gal.load(E.reference_embed(rng.integers(-128, 128, (cap, D)).astype(np.int8), net.q[net.num_layer]), np.arange(cap, dtype=np.int32) // 10)
    res = dict(D=D, batch=a.batch, top_k=k, match_rows=a.match_rows, n_thr=a.n_thr, step=a.step, tile=E.ROC_TILE)

    def timed(fn, launches, warmup):
        """(median, p10, p90 of event pairs; back-to-back mean), microseconds"""
        s = torch.cuda.current_stream()
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        evs = []
        for _ in range(launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            evs.append((e0, e1))
        torch.cuda.synchronize()
        pairs = np.array([e0.elapsed_time(e1) for e0, e1 in evs]) * 1e3
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(launches):
            fn()
        e1.record(s)
        torch.cuda.synchronize()
        return dict(median=round(float(np.median(pairs)), 2), p10=round(float(np.percentile(pairs, 10)), 2),
                    p90=round(float(np.percentile(pairs, 90)), 2), back_to_back=round(e0.elapsed_time(e1) * 1e3 / launches, 2), launches=launches)

    res["roc_us"], res["roc_ns_per_distance"] = {}, {}
    for n in rows:
        roc = E.DeviceRoc(a.n_thr, a.step, device=dev)
        tm = timed(lambda: roc.add(gal, n=n), a.launches, a.warmup)
        pairs = n * (n - 1) // 2
        counted = int(roc.hist.sum().cpu())
        if counted != (a.warmup + 2 * a.launches) * pairs:
            raise SystemExit(f"N = {n}: the histogram holds {counted} pairs, not {(a.warmup + 2 * a.launches) * pairs}")
        res["roc_us"][str(n)] = tm
        res["roc_ns_per_distance"][str(n)] = round(tm["back_to_back"] * 1e3 / pairs, 6)

    x = torch.from_numpy(np.ascontiguousarray(synth.synth_images(t, a.batch, 100))).to(dev)
    outputs = Runner(None, net).run_batch(x).clone()
    truth = torch.from_numpy(rng.integers(0, cap // 10, a.batch).astype(np.int32)).to(dev)
    m = E.DeviceMatcher(net, k)
    tm = timed(lambda: m.match(outputs, gal, n=a.match_rows, threshold=0.5, truth=truth), a.match_launches, max(a.warmup, 30))
    res["match_call_us"] = tm
    res["match_call_ns_per_distance"] = round(tm["back_to_back"] * 1e3 / (a.batch * a.match_rows), 6)
    res["roc_over_match_call"] = {n: round(v / res["match_call_ns_per_distance"], 3) for n, v in res["roc_ns_per_distance"].items()}
    emit(res, a.out)


def emit(res, out):
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
