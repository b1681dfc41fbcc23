#!/usr/bin/env python3
"""Cost of image preprocessing on the device (tf2_preprocess, preprocess.hip) at --batch images of --src-h x --src-w uint8 RGB sources
(synthetic weights).  HIP events on one stream around
  kernel        one tf2_preprocess call (ResNet-50 preset, int8 output), median over --steps calls; also for float32 output
and the bytes it moves (source bytes read + output bytes written) over that time as a fraction of the MI355X's 8 TB/s HBM peak.
Then throughput in images/s of ResNet-50 and SSD300 steps, one batch at a time (eager, concurrency 0) and with --inflight batches
in flight (one captured graph per stream, replayed round robin, concurrency 1, as bench.py does), each
  float         Runner.run_batch on float32 images already on the device (what bench.py times)
  int8          Runner.run_batch on int8 images already on the device
  preprocess    tf2_preprocess from uint8 pixels (int8 output) + Runner.run_batch on its output, in the same step
Prints one JSON line.  `--kernel-only` times the kernels alone: under
`rocprofv3 --kernel-trace --stats -- python tools/preprocess_time.py --kernel-only` the statistics give the kernel's own time."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--src-h", type=int, default=375)
    ap.add_argument("--src-w", type=int, default=500)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    import torch
    from tf2_amd import config as cfg, preprocess as P, synth
    from tf2_amd.network import NetWork, Runner
    dev = "cuda:0"
    rng = np.random.default_rng(7)

    def make_net(t, q):
        net = NetWork(t)
        net.Init(synth.synth_model(t, q, 0), synth.q_text(q), device=dev)
        return net

    def sources(preset, n_sets):
        out = []
        for _ in range(n_sets):
            imgs = [rng.integers(0, 256, (a.src_h, a.src_w, 3), dtype=np.uint8) for _ in range(a.batch)]
            out.append(P.pack(imgs, preset, dev))
        return out

    res = dict(batch=a.batch, src_hw=[a.src_h, a.src_w], steps=a.steps, inflight=a.inflight)
    t50 = cfg.resnet50_tables()
    q50 = np.loadtxt(os.path.join(ROOT, "tests", "golden", "resnet50_Q"), dtype=np.int32)
    net50 = make_net(t50, q50)
    pp50 = P.Preprocessor(net50, P.RESNET50, "RGB")
    src50 = sources(P.RESNET50, 2 * a.inflight)
    s = torch.cuda.current_stream()

    # -- the kernel alone
    for out in ("q", "f32"):
        px, sr = src50[0]
        for _ in range(a.warmup):
            pp50(px, sr, out=out)
        evs = []
        for k in range(a.steps):
            px, sr = src50[k % len(src50)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            pp50(px, sr, out=out)
            e1.record(s)
            evs.append((e0, e1))
        torch.cuda.synchronize()
        ms = float(np.median([e0.elapsed_time(e1) for e0, e1 in evs]))
        nbytes = a.batch * a.src_h * a.src_w * 3 + a.batch * 3 * 224 * 224 * (1 if out == "q" else 4)
        res[f"kernel_{out}_us"] = round(ms * 1e3, 2)
        res[f"kernel_{out}_bytes"] = nbytes
        res[f"kernel_{out}_hbm_fraction"] = round(nbytes / (ms * 1e-3) / HBM_PEAK, 4)
    if a.kernel_only:
        print(json.dumps(res))
        return

    def throughput(net, preset, srcs, tag):
        """images/s of the three step kinds, one batch at a time and in flight"""
        pp = P.Preprocessor(net, preset, "RGB")
        n_buf = len(srcs)
        xf = [pp(px, sr, out="f32")[0].clone() for px, sr in srcs]
        xq = [pp(px, sr, out="q")[0].clone() for px, sr in srcs]
        torch.cuda.synchronize()
        out = {}
        kinds = {
            "float": lambda rn, k, conc: rn.run_batch(xf[k], concurrency=conc),
            "int8": lambda rn, k, conc: rn.run_batch(xq[k], concurrency=conc),
            "preprocess": lambda rn, k, conc: rn.run_batch(pp(*srcs[k], out="q")[0], concurrency=conc),
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
            out[f"{tag}_serial_{name}"] = round(a.batch * a.steps / (time.perf_counter() - t0), 1)
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
                    i = k % a.inflight
                    with torch.cuda.stream(streams[i]):
                        graphs[k % n_buf].replay()
            run(a.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(a.steps)
            torch.cuda.synchronize()
            out[f"{tag}_inflight_{name}"] = round(a.batch * a.steps / (time.perf_counter() - t0), 1)
            del graphs
        for mode in ("serial", "inflight"):
            out[f"{tag}_{mode}_preprocess_over_float"] = round(out[f"{tag}_{mode}_preprocess"] / out[f"{tag}_{mode}_float"], 4)
            out[f"{tag}_{mode}_preprocess_over_int8"] = round(out[f"{tag}_{mode}_preprocess"] / out[f"{tag}_{mode}_int8"], 4)
        return out

    res.update(throughput(net50, P.RESNET50, src50, "resnet50"))
    del net50, pp50
    t300 = cfg.ssd300_tables()
    q300 = np.array(synth.synth_q_values(t300, 5, spread=1))
    net300 = make_net(t300, q300)
    res.update(throughput(net300, P.SSD300, sources(P.SSD300, 2 * a.inflight), "ssd300"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
