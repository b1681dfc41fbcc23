#!/usr/bin/env python3
"""Cost of face matching on the device (tf2_emb_match, embed_match.hip) for SqueezeNet 1.1 (synthetic weights): --batch images, D = 128,
top 5.
  match         one tf2_emb_match call (embed + stage 1 + stage 2, with truth and tallies) against galleries of --rows rows, HIP events
                on one stream: the median of --launches event pairs after warm-up, and a run of --launches back-to-back calls
                between one pair divided by their number
  copy          a plain device-to-device copy of the same gallery buffer, timed the same way in the same call: the gallery bytes a
                second of the match next to the copy's (the match reads the gallery once and writes next to nothing, the copy reads
                and writes it), and the match's float32 operations a second (3 B D N) next to the vector peak
Then images/s with --inflight batches in flight (one captured graph per stream and input buffer, replayed round robin,
concurrency 1, as bench.py's default leg), --repeats times each, alternating:
  network       Runner.run_batch alone (what bench.py times)
  device        run_batch + DeviceMatcher.match against --graph-rows rows inside the replayed graphs; the tally stays on the device
  host          the graphs of `network`, then the host path per batch: wait for its stream, outputs.cpu(), reference_embed and
                reference_match (--host-steps steps a repeat: it runs at a small fraction of the others' rate)
Prints one JSON line (and writes it to --out).  `--kernel-only` stops after the match timing: under
`rocprofv3 --kernel-trace --stats -- python tools/embed_time.py --kernel-only` the statistics give each kernel's own time."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VALU_PEAK = 256 * 4 * 32 * 2.4e9          # unfused float32 operations a second: 256 CUs x 4 SIMDs x 32 a clock (packed pairs) at 2.4 GHz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rows", default="1000,10000,100000")
    ap.add_argument("--graph-rows", type=int, default=10000)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--host-steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tf2_amd import embed as E, synth
    from tf2_amd.network import NetWork, Runner
    dev = "cuda:0"
    t, q, seed = synth.bench_network("squeezenet")[:3]
    net = NetWork(t)
    net.Init(synth.synth_model(t, q, seed), synth.q_text(q), device=dev)
    n_buf = 2 * a.inflight
    xs = [torch.from_numpy(np.ascontiguousarray(synth.synth_images(t, a.batch, 100 + k))).to(dev) for k in range(n_buf)]
    rng = np.random.default_rng(3)
    rows = [int(v) for v in a.rows.split(",")]
    cap = max(rows + [a.graph_rows])
    D, k = int(net.plan[-1].N), 5
    # a gallery of unit rows (the statement's embeddings of random int8 outputs) with ten rows an identity
    gal_host = E.reference_embed(rng.integers(-128, 128, (cap, D)).astype(np.int8), net.q[net.num_layer])
    gal = E.Gallery(cap, D, dev)
    gal.load(gal_host, np.arange(cap, dtype=np.int32) // 10)
    truths = [torch.from_numpy(rng.integers(0, cap // 10, a.batch).astype(np.int32)).to(dev) for _ in range(n_buf)]
    res = dict(batch=a.batch, D=D, top_k=k, launches=a.launches, steps=a.steps, host_steps=a.host_steps, inflight=a.inflight,
               repeats=a.repeats, graph_rows=a.graph_rows, slab=E.SLAB)

    def timed(fn):
        """(median, p10, p90 of event pairs; back-to-back mean), microseconds"""
        s = torch.cuda.current_stream()
        for _ in range(max(a.warmup, 30)):
            fn()
        torch.cuda.synchronize()
        evs = []
        for _ in range(a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            evs.append((e0, e1))
        torch.cuda.synchronize()
        pairs = np.array([e0.elapsed_time(e1) for e0, e1 in evs]) * 1e3
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(a.launches):
            fn()
        e1.record(s)
        torch.cuda.synchronize()
        return dict(median=round(float(np.median(pairs)), 2), p10=round(float(np.percentile(pairs, 10)), 2),
                    p90=round(float(np.percentile(pairs, 90)), 2), back_to_back=round(e0.elapsed_time(e1) * 1e3 / a.launches, 2))

    # -- the match alone, on the outputs of a real step
    m = E.DeviceMatcher(net, k)
    outputs = Runner(None, net).run_batch(xs[0]).clone()
    res["match_us"], res["copy_us"], res["balance"] = {}, {}, {}
    for n in rows:
        tm = timed(lambda: m.match(outputs, gal, n=n, threshold=0.5, truth=truths[0]))
        src = gal.rows[:n]
        dst = torch.empty_like(src)
        tc = timed(lambda: dst.copy_(src))
        nbytes = n * D * 4
        res["match_us"][str(n)], res["copy_us"][str(n)] = tm, tc
        res["balance"][str(n)] = dict(gallery_bytes=nbytes,
                                      match_gallery_GBps=round(nbytes / tm["back_to_back"] / 1e3, 1),
                                      copy_gallery_GBps=round(nbytes / tc["back_to_back"] / 1e3, 1),
                                      match_over_copy_time=round(tm["back_to_back"] / tc["back_to_back"], 2),
                                      match_valu_share_of_peak=round(3.0 * a.batch * D * n / (tm["back_to_back"] * 1e-6) / VALU_PEAK, 3))
    if a.kernel_only:
        emit(res, a.out)
        return

    # -- batches in flight: one graph per (stream, buffer)
    streams = [torch.cuda.Stream() for _ in range(a.inflight)]

    def capture(with_match):
        runners = [Runner(None, net) for _ in range(a.inflight)]
        matchers = [E.DeviceMatcher(net, k) for _ in range(a.inflight)] if with_match else None
        graphs, outs = {}, {}

        def step(j):
            i = j % a.inflight
            o = runners[i].run_batch(xs[j], concurrency=1)
            return matchers[i].match(o, gal, n=a.graph_rows, threshold=0.5, truth=truths[j]) if with_match else o
        for j in range(n_buf):
            i = j % a.inflight
            step(j)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            streams[i].wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(streams[i]):
                with torch.cuda.graph(g, stream=streams[i]):
                    outs[j] = step(j)
            torch.cuda.current_stream().wait_stream(streams[i])
            graphs[j] = g
        torch.cuda.synchronize()
        return graphs, runners, matchers

    g_net, r_net, _ = capture(False)
    g_dev, _, m_dev = capture(True)
    for x in m_dev:
        x.reset()

    def replay(graphs, n):
        for j in range(n):
            with torch.cuda.stream(streams[j % a.inflight]):
                graphs[j % n_buf].replay()

    def leg_graphs(graphs):
        replay(graphs, a.warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        replay(graphs, a.steps)
        torch.cuda.synchronize()
        return a.batch * a.steps / (time.perf_counter() - t0)

    gal_n = gal_host[:a.graph_rows]

    def leg_host():
        """the parent's path: a batch's matches exist once its stream has drained, its outputs are on the host and the statement has run"""
        pending = [None] * a.inflight

        def finish(i):
            streams[i].synchronize()
            out = r_net[i]._logits.cpu().numpy()
            E.reference_match(E.reference_embed(out, net.q[net.num_layer]), gal_n, None, k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(a.host_steps):
            i = j % a.inflight
            if pending[i] is not None:
                finish(i)
            with torch.cuda.stream(streams[i]):
                g_net[j % n_buf].replay()
            pending[i] = j
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
    res["device_tally_labelled"] = sum(x.accuracy()["labelled"] for x in m_dev)           # every replayed image counted, on the device
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
