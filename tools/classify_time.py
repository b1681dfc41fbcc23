#!/usr/bin/env python3
"""Cost of classification on the device (tf2_cls_run, classify.hip) for ResNet-50 (synthetic weights): --batch images, n = 1000, top 5.
  kernel        one tf2_cls_run call (labels, features, probabilities, ranks and tallies) on a logits buffer, HIP events on one
                stream: the median of --launches event pairs after warm-up, and the whole run of --launches back-to-back calls
                between one pair divided by their number
Then images/s with --inflight batches in flight (one captured graph per stream and input buffer, replayed round robin,
concurrency 1, as bench.py's default leg), --repeats times each, alternating:
  network       Runner.run_batch alone (what bench.py times)
  device        run_batch + DeviceClassifier.run inside the replayed graphs; the tally stays on the device
  host          the graphs of `network`, then the host path per batch: wait for its stream, logits.cpu(), network.Evaluation per image
                (--host-steps steps a repeat: it runs at a small fraction of the others' rate)
Prints one JSON line.  `--kernel-only` stops after the kernel timing: under
`rocprofv3 --kernel-trace --stats -- python tools/classify_time.py --kernel-only` the statistics give the kernel's own time."""
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
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--host-steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    import torch
    from tf2_amd import classify as K, config as cfg, network, synth
    from tf2_amd.network import NetWork, Runner
    dev = "cuda:0"
    t = cfg.resnet50_tables()
    q = np.loadtxt(os.path.join(ROOT, "tests", "golden", "resnet50_Q"), dtype=np.int32)
    net = NetWork(t)
    net.Init(synth.synth_model(t, q, 0), synth.q_text(q), device=dev)
    n_buf = 2 * a.inflight
    xs = [torch.from_numpy(np.ascontiguousarray(synth.synth_images(t, a.batch, 100 + k))).to(dev) for k in range(n_buf)]
    rng = np.random.default_rng(3)
    truths = [torch.from_numpy(rng.integers(0, 1000, a.batch).astype(np.int32)).to(dev) for _ in range(n_buf)]
    res = dict(batch=a.batch, n=int(net.plan[-1].N), top_k=5, launches=a.launches, steps=a.steps, host_steps=a.host_steps,
               inflight=a.inflight, repeats=a.repeats)

    # -- the kernel alone, on the logits of a real step
    cls = K.DeviceClassifier(net, 5)
    logits = Runner(None, net).run_batch(xs[0]).clone()
    s = torch.cuda.current_stream()
    for _ in range(max(a.warmup, 50)):
        cls.run(logits, truths[0])
    torch.cuda.synchronize()
    evs = []
    for _ in range(a.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        cls.run(logits, truths[0])
        e1.record(s)
        evs.append((e0, e1))
    torch.cuda.synchronize()
    pairs = np.array([e0.elapsed_time(e1) for e0, e1 in evs]) * 1e3
    res["kernel_event_pair_us"] = dict(median=round(float(np.median(pairs)), 2), p10=round(float(np.percentile(pairs, 10)), 2),
                                       p90=round(float(np.percentile(pairs, 90)), 2))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(a.launches):
        cls.run(logits, truths[0])
    e1.record(s)
    torch.cuda.synchronize()
    res["kernel_back_to_back_us"] = round(e0.elapsed_time(e1) * 1e3 / a.launches, 2)
    if a.kernel_only:
        print(json.dumps(res))
        return

    # -- batches in flight: one graph per (stream, buffer)
    streams = [torch.cuda.Stream() for _ in range(a.inflight)]

    def capture(with_cls):
        runners = [Runner(None, net) for _ in range(a.inflight)]
        classifiers = [K.DeviceClassifier(net, 5) for _ in range(a.inflight)] if with_cls else None
        graphs, outs = {}, {}

        def step(k):
            i = k % a.inflight
            lg = runners[i].run_batch(xs[k], concurrency=1)
            return classifiers[i].run(lg, truths[k]) if with_cls else lg
        for k in range(n_buf):
            i = k % a.inflight
            step(k)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            streams[i].wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(streams[i]):
                with torch.cuda.graph(g, stream=streams[i]):
                    outs[k] = step(k)
            torch.cuda.current_stream().wait_stream(streams[i])
            graphs[k] = g
        torch.cuda.synchronize()
        return graphs, runners, classifiers

    g_net, r_net, _ = capture(False)
    g_dev, _, c_dev = capture(True)

    def replay(graphs, n):
        for k in range(n):
            with torch.cuda.stream(streams[k % a.inflight]):
                graphs[k % n_buf].replay()

    def leg_graphs(graphs):
        replay(graphs, a.warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        replay(graphs, a.steps)
        torch.cuda.synchronize()
        return a.batch * a.steps / (time.perf_counter() - t0)

    def leg_host():
        """the parent's path: a batch's labels exist once its stream has drained, its logits are on the host and Evaluation has run"""
        pending = [None] * a.inflight

        def finish(i):
            streams[i].synchronize()
            out = r_net[i]._logits.cpu().numpy()
            for b in range(a.batch):
                network.Evaluation(b, net.q, out, num_layer=net.num_layer)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(a.host_steps):
            i = k % a.inflight
            if pending[i] is not None:
                finish(i)
            with torch.cuda.stream(streams[i]):
                g_net[k % n_buf].replay()
            pending[i] = k
        for i in range(a.inflight):
            if pending[i] is not None:
                finish(i)
        return a.batch * a.host_steps / (time.perf_counter() - t0)

    legs = dict(network=[], device=[], host=[])
    for _ in range(a.repeats):
        legs["network"].append(leg_graphs(g_net))
        legs["device"].append(leg_graphs(g_dev))
        legs["host"].append(leg_host())
    for name, v in legs.items():
        res[f"inflight_{name}_images_per_s"] = dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))
    res["device_over_network"] = round(float(np.median(legs["device"]) / np.median(legs["network"])), 4)
    res["device_over_network_per_repeat"] = [round(d / n, 4) for d, n in zip(legs["device"], legs["network"])]
    res["host_over_network"] = round(float(np.median(legs["host"]) / np.median(legs["network"])), 4)
    acc = [c.accuracy() for c in c_dev]
    res["device_tally_labelled"] = sum(x["labelled"] for x in acc)                # every replayed image counted, on the device
    print(json.dumps(res))


if __name__ == "__main__":
    main()
