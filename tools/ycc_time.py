#!/usr/bin/env python3
"""Cost of the YCbCr conversion on the device (tf2_ycc_to_rgb, ycc_convert.hip): --batch frames of --src-h x --src-w, 4:2:0, as three
planes and as NV12, FANCY + JFIF, 3-byte RGB out, beside the yardstick tf2_preprocess (TORCHVISION geometry, int8 output) on the RGB
bytes the conversion wrote -- in one process, HIP events on one stream around each call, the three calls alternating inside every
step, --repeats repeats of --steps steps each after a warm-up; reported are the median over the repeats' medians and their lowest
and highest (the spread).  Each time comes with the bytes the algorithm moves, computed here from the shapes (planes read, pixels
written; for the yardstick pixels read -- every source pixel once, its gather reads at most that -- and int8 written), and the
resulting bytes/s.
Then throughput in images/s of ResNet-50 (synthetic weights) with --inflight batches in flight, one captured graph per (stream,
buffer) replayed round robin as bench.py does, each graph holding
  rgb           tf2_preprocess_aa (TORCHVISION_PIL, int8) + network + classifier, from RGB pixels already on the device
  ycc           tf2_ycc_to_rgb in front of the same three, from NV12 planes already on the device
Prints one JSON line and writes it to --out (default profiles/ycc_time_b<batch>.json).  `--kernel-only` stops after the kernels."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--src-h", type=int, default=375)
    ap.add_argument("--src-w", type=int, default=500)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tf2_amd import classify as K, config as cfg, preprocess as P, synth, ycc as Y
    from tf2_amd.network import NetWork, Runner
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = "cuda:0"
    rng = np.random.default_rng(7)
    h, w, B, sub = a.src_h, a.src_w, a.batch, (2, 2)

    t50 = cfg.resnet50_tables()
    q50 = np.loadtxt(os.path.join(ROOT, "tests", "golden", "resnet50_Q"), dtype=np.int32)
    net = NetWork(t50)
    net.Init(synth.synth_model(t50, q50, 0), synth.q_text(q50), device=dev)
    n_buf = 2 * a.inflight
    layouts = {"planar": Y.PLANAR, "nv12": Y.SEMI_CBCR}
    bufs = {name: [] for name in layouts}
    for _ in range(n_buf):
        frames = [Y.subsample_box(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), sub) for _ in range(B)]
        for name, layout in layouts.items():                    # (TORCHVISION and TORCHVISION_PIL have one geometry: one set of records)
            bufs[name].append(Y.pack_ycc(frames, layout, sub, dev, 3, preset=P.TORCHVISION_PIL))
    convs = {name: Y.DeviceConverter(Y.Desc(layout=layout, sub=sub)) for name, layout in layouts.items()}
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    pp, pp_aa = P.Preprocessor(net, P.TORCHVISION, "RGB"), P.Preprocessor(net, P.TORCHVISION_PIL, "RGB")
    ch, cw = Y.chroma_size(h, w, sub)
    oh, ow = pp.out_hw
    moved = {"ycc": B * (h * w + 2 * ch * cw) + B * h * w * 3, "preprocess": B * h * w * 3 + B * 3 * oh * ow}
    res = dict(batch=B, src_hw=[h, w], sub=list(sub), steps=a.steps, repeats=a.repeats, inflight=a.inflight,
               blocks_per_image=Y.default_blocks_per_image(B), ycc_bytes_read=B * (h * w + 2 * ch * cw), ycc_bytes_written=B * h * w * 3,
               preprocess_bytes_read=B * h * w * 3, preprocess_bytes_written=B * 3 * oh * ow)
    s = torch.cuda.current_stream()

    def ycc_call(name):
        def f(k):
            src, yc, sc, px = bufs[name][k]
            convs[name].run(src, yc, px, sc, status=status)
        return f
    calls = {"ycc_planar": ycc_call("planar"), "ycc_nv12": ycc_call("nv12"),
             "preprocess": lambda k: pp(bufs["planar"][k][3], bufs["planar"][k][2], out="q")}
    for k in range(max(a.warmup, n_buf)):
        for fn in calls.values():
            fn(k % n_buf)
    torch.cuda.synchronize()
    assert (status.cpu() == 0).all()
    meds = {name: [] for name in calls}
    for _ in range(a.repeats):
        evs = {name: [] for name in calls}
        for k in range(a.steps):
            for name, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                fn(k % n_buf)
                e1.record(s)
                evs[name].append((e0, e1))
        torch.cuda.synchronize()
        for name in calls:
            meds[name].append(float(np.median([e0.elapsed_time(e1) for e0, e1 in evs[name]])) * 1e3)
    for name in calls:
        us = float(np.median(meds[name]))
        nbytes = moved["preprocess" if name == "preprocess" else "ycc"]
        res[f"{name}_us"] = round(us, 2)
        res[f"{name}_us_spread"] = [round(min(meds[name]), 2), round(max(meds[name]), 2)]
        res[f"{name}_gb_per_s"] = round(nbytes / us * 1e-3, 1)
    for name in ("ycc_planar", "ycc_nv12"):
        res[f"{name}_over_preprocess"] = round(res[f"{name}_us"] / res["preprocess_us"], 3)
    res["ycc_bytes_over_preprocess_bytes"] = round(moved["ycc"] / moved["preprocess"], 3)

    if not a.kernel_only:
        streams = [torch.cuda.Stream() for _ in range(a.inflight)]
        runners = [Runner(None, net) for _ in range(a.inflight)]
        clss = [K.DeviceClassifier(net, 5) for _ in range(a.inflight)]
        stats = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(n_buf)]

        def step(kind, i, k):
            src, yc, sc, px = bufs["nv12"][k]
            if kind == "ycc":
                convs["nv12"].run(src, yc, px, sc, status=stats[k])
            return clss[i].run(runners[i].run_batch(pp_aa(px, sc, out="q")[0], concurrency=1))
        for kind in ("rgb", "ycc"):
            graphs = {}
            for k in range(n_buf):
                i = k % a.inflight
                step(kind, i, k)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                streams[i].wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(streams[i]):
                    with torch.cuda.graph(g, stream=streams[i]):
                        step(kind, i, k)
                torch.cuda.current_stream().wait_stream(streams[i])
                graphs[k] = g
            torch.cuda.synchronize()

            def run(n):
                for k in range(n):
                    with torch.cuda.stream(streams[k % a.inflight]):
                        graphs[k % n_buf].replay()
            rates = []
            for _ in range(a.repeats):
                run(a.warmup)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(a.steps)
                torch.cuda.synchronize()
                rates.append(B * a.steps / (time.perf_counter() - t0))
            res[f"inflight_{kind}"] = round(float(np.median(rates)), 1)
            res[f"inflight_{kind}_spread"] = [round(min(rates), 1), round(max(rates), 1)]
            del graphs
        res["inflight_ycc_over_rgb"] = round(res["inflight_ycc"] / res["inflight_rgb"], 4)
    line = json.dumps(res)
    print(line)
    out = a.out or os.path.join(ROOT, "profiles", f"ycc_time_b{B}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
