#!/usr/bin/env python3
"""Cost of the antialiased resize on the device (tf2_preprocess_aa, preprocess_aa.hip) beside the plain one (tf2_preprocess) on the
same inputs in the same process: --batch images of --src-h x --src-w uint8 RGB sources, ResNet-50 (synthetic weights), the TORCHVISION
geometry (Resize(256), CenterCrop(224)) -- TORCHVISION for the plain kernel, TORCHVISION_PIL for the antialiased one.  HIP events on
one stream around
  kernel        one call (int8 output), median over --steps calls, for each of the two; also for float32 output
then throughput in images/s of ResNet-50 steps, one batch at a time (eager, concurrency 0) and with --inflight batches in flight (one
captured graph per stream, replayed round robin, concurrency 1, as bench.py does), each
  float         Runner.run_batch on float32 images already on the device (what bench.py times)
  plain         tf2_preprocess from uint8 pixels (int8 output) + Runner.run_batch on its output, in the same step
  aa            tf2_preprocess_aa in its place
Prints one JSON line and writes it to --out (default profiles/preprocess_aa_time_b<batch>.json).  `--kernel-only` times the kernels
alone: under `rocprofv3 --kernel-trace --stats -- python tools/preprocess_aa_time.py --kernel-only` the statistics give their own time."""
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
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tf2_amd import config as cfg, preprocess as P, synth
    from tf2_amd.network import NetWork, Runner
    dev = "cuda:0"
    rng = np.random.default_rng(7)

    t50 = cfg.resnet50_tables()
    q50 = np.loadtxt(os.path.join(ROOT, "tests", "golden", "resnet50_Q"), dtype=np.int32)
    net = NetWork(t50)
    net.Init(synth.synth_model(t50, q50, 0), synth.q_text(q50), device=dev)
    pps = {"plain": P.Preprocessor(net, P.TORCHVISION, "RGB"), "aa": P.Preprocessor(net, P.TORCHVISION_PIL, "RGB")}
    n_buf = 2 * a.inflight
    srcs = []                                              # the records of the two presets are the same: one set of inputs
    for _ in range(n_buf):
        imgs = [rng.integers(0, 256, (a.src_h, a.src_w, 3), dtype=np.uint8) for _ in range(a.batch)]
        srcs.append(P.pack(imgs, P.TORCHVISION, dev))
    rh, rw, cy, cx = P.TORCHVISION.geometry(a.src_h, a.src_w)
    res = dict(batch=a.batch, src_hw=[a.src_h, a.src_w], resize_hw=[rh, rw], crop=[cy, cx], steps=a.steps, inflight=a.inflight)
    s = torch.cuda.current_stream()

    # -- the kernels alone
    for name, pp in pps.items():
        for out in ("q", "f32"):
            for _ in range(a.warmup):
                pp(*srcs[0], out=out)
            evs = []
            for k in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                pp(*srcs[k % n_buf], out=out)
                e1.record(s)
                evs.append((e0, e1))
            torch.cuda.synchronize()
            res[f"kernel_{name}_{out}_us"] = round(float(np.median([e0.elapsed_time(e1) for e0, e1 in evs])) * 1e3, 2)
    for out in ("q", "f32"):
        res[f"kernel_{out}_aa_over_plain"] = round(res[f"kernel_aa_{out}_us"] / res[f"kernel_plain_{out}_us"], 3)
    if not a.kernel_only:
        xf = [pps["plain"](px, sr, out="f32")[0].clone() for px, sr in srcs]
        torch.cuda.synchronize()
        kinds = {
            "float": lambda rn, k, conc: rn.run_batch(xf[k], concurrency=conc),
            "plain": lambda rn, k, conc: rn.run_batch(pps["plain"](*srcs[k], out="q")[0], concurrency=conc),
            "aa": lambda rn, k, conc: rn.run_batch(pps["aa"](*srcs[k], out="q")[0], concurrency=conc),
        }
        # one batch at a time, eager on the default stream
        rn = Runner(None, net)
        for name, fn in kinds.items():
            for k in range(max(a.warmup, 8)):
                fn(rn, k % n_buf, 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(a.steps):
                fn(rn, k % n_buf, 0)
            torch.cuda.synchronize()
            res[f"serial_{name}"] = round(a.batch * a.steps / (time.perf_counter() - t0), 1)
        # in flight: one graph per (stream, buffer), replayed round robin
        streams = [torch.cuda.Stream() for _ in range(a.inflight)]
        runners = [Runner(None, net) for _ in range(a.inflight)]
        for name, fn in kinds.items():
            graphs = {}
            for k in range(n_buf):
                i = k % a.inflight
                fn(runners[i], k, 1)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                streams[i].wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(streams[i]):
                    with torch.cuda.graph(g, stream=streams[i]):
                        fn(runners[i], k, 1)
                torch.cuda.current_stream().wait_stream(streams[i])
                graphs[k] = g
            torch.cuda.synchronize()

            def run(n):
                for k in range(n):
                    with torch.cuda.stream(streams[k % a.inflight]):
                        graphs[k % n_buf].replay()
            run(a.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(a.steps)
            torch.cuda.synchronize()
            res[f"inflight_{name}"] = round(a.batch * a.steps / (time.perf_counter() - t0), 1)
            del graphs
        for mode in ("serial", "inflight"):
            for name in ("plain", "aa"):
                res[f"{mode}_{name}_over_float"] = round(res[f"{mode}_{name}"] / res[f"{mode}_float"], 4)
            res[f"{mode}_aa_over_plain"] = round(res[f"{mode}_aa"] / res[f"{mode}_plain"], 4)
    line = json.dumps(res)
    print(line)
    out = a.out or os.path.join(ROOT, "profiles", f"preprocess_aa_time_b{a.batch}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
