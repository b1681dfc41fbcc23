#!/usr/bin/env python3
"""Cost of JPEG entropy decoding on the device (tf2_jpeg_huff, jpeg_huff.hip) against the host step it replaces: --batch files of
--src-h x --src-w, 4:2:0 -- tools/jpeg_time.py's files (its synthetic frames, its encoder) and its method (HIP events on one stream,
the calls alternating inside every step, the median over --repeats repeats' medians, one process).  In one job:
  1. tf2_jpeg_huff at the default subseq_bytes and at every --subseq value, with the rounds it used (an image's sum over its chunks:
     mean and highest of the batch);
  2. tf2_jpeg_idct on the coefficients it wrote, as the yardstick;
  3. the host -> device copy (pinned memory) of the files' entropy-coded bytes and of the dense coefficient buffer;
  4. the host step, tf2_jpeg_parse + tf2_jpeg_entropy, in files/s on 1 and on --threads threads;
  5. with --inflight batches in flight, one stream each: files/s of tf2_jpeg_huff alone (the device decode rate), and images/s of
     ResNet-50 (synthetic weights) with one captured graph per (stream, buffer) replayed round robin as bench.py does, each holding
       coef     tf2_jpeg_idct + tf2_ycc_to_rgb + tf2_preprocess_aa + network + classifier, from coefficients on the device
       bytes    tf2_jpeg_huff in front of the same five, from file bytes on the device
Prints one JSON line and writes it to --out (default profiles/jpeg_huff_time_b<batch>.json).  `--kernel-only` leaves the graphs out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import jpeg_time as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--src-h", type=int, default=375)
    ap.add_argument("--src-w", type=int, default=500)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--subseq", type=int, nargs="*", default=[64, 128, 256])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tf2_amd import classify as K, config as cfg, jpeg as J, preprocess as P, synth, ycc as Y
    from tf2_amd.network import NetWork, Runner
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = "cuda:0"
    rng = np.random.default_rng(7)
    h, w, B, sub, layout = a.src_h, a.src_w, a.batch, (2, 2), Y.PLANAR

    distinct = [T.encode(T.synth_frame(rng, h, w), sub, J.ZIGZAG) for _ in range(a.distinct)]
    files = [distinct[i % a.distinct] for i in range(B)]
    infos = [J.parse(f) for f in files]
    host = J.decode_host(files, threads=a.threads)
    assert all(st == 0 for _, _, st in host), "the tool's own files must decode"
    res = dict(batch=B, src_hw=[h, w], sub=list(sub), steps=a.steps, repeats=a.repeats, inflight=a.inflight, distinct_files=a.distinct,
               file_bytes=[len(f) for f in distinct], scan_bytes=[len(f) - i.scan_offset for f, i in zip(distinct, infos)],
               default_subseq=J.HUFF_DEFAULT_SUBSEQ, lanes=J.HUFF_LANES)

    # -- 4. the host step
    def host_step(data):
        info = J.parse(data)
        return J.entropy(data, info)[1]
    res["host_decode_files_per_s_1_thread"] = round(T.rate(host_step, files, 1), 1)
    res[f"host_decode_files_per_s_{a.threads}_threads"] = round(T.rate(host_step, files, a.threads), 1)

    # -- 1, 2. the kernels
    n_buf = 2 * a.inflight
    order = lambda k: [(files[(i + k) % B], infos[(i + k) % B]) for i in range(B)]
    bufs = [J.pack_bytes(order(k), layout, sub, dev, 3, preset=P.TORCHVISION_PIL, subseq_bytes=16) for k in range(n_buf)]
    want = np.concatenate([c for _, c, _ in host])
    dec = J.DeviceDecoder(J.Desc(layout, sub))
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    names = {0: "huff"}
    names.update({s: f"huff_s{s}" for s in a.subseq})
    ents = {s: J.DeviceEntropy(J.HuffDesc(layout, sub, s)) for s in names}
    huff = lambda s: (lambda k: ents[s].run(bufs[k][0], bufs[k][1], bufs[k][3], bufs[k][2], bufs[k][9], status=status))
    calls = {names[s]: huff(s) for s in names}
    calls["idct"] = lambda k: dec.run(bufs[k][2], bufs[k][3], bufs[k][4], bufs[k][5], bufs[k][6], bufs[k][7], status=status)
    scan_total, coef_bytes = int(bufs[0][0].numel()), int(bufs[0][2].numel()) * 2
    res.update(scan_buffer_bytes=scan_total, coef_buffer_bytes=coef_bytes, coef_bytes_over_scan_bytes=round(coef_bytes / scan_total, 2))
    for s, name in names.items():                                  # exact, and the rounds used
        bufs[0][2].fill_(0x5A5A)
        calls[name](0)
        torch.cuda.synchronize()
        assert (status.cpu() == 0).all() and np.array_equal(bufs[0][2].cpu().numpy(), want), name
        slice_ = (bufs[0][9].numel() // B) & ~7
        rounds = bufs[0][9].cpu().numpy()[:B * slice_].reshape(B, slice_)[:, :8].copy().view(np.int32)
        res[f"{name}_rounds_mean"], res[f"{name}_rounds_max"] = round(float(rounds[:, 0].mean()), 1), int(rounds[:, 0].max())
        res[f"{name}_subsequences_max"] = int(rounds[:, 1].max())
    pinned = {"scan": torch.empty(scan_total, dtype=torch.uint8).pin_memory(), "coef": torch.empty(coef_bytes, dtype=torch.uint8).pin_memory()}
    landing = {k: torch.empty(v.numel(), dtype=torch.uint8, device=dev) for k, v in pinned.items()}
    for name in pinned:
        calls["copy_" + name] = (lambda n: lambda k: landing[n].copy_(pinned[n], non_blocking=True))(name)
    s0 = torch.cuda.current_stream()
    for k in range(max(a.warmup, n_buf)):
        for fn in calls.values():
            fn(k % n_buf)
    torch.cuda.synchronize()
    meds = {name: [] for name in calls}
    for _ in range(a.repeats):
        evs = {name: [] for name in calls}
        for k in range(a.steps):
            for name, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s0)
                fn(k % n_buf)
                e1.record(s0)
                evs[name].append((e0, e1))
        torch.cuda.synchronize()
        for name in calls:
            meds[name].append(float(np.median([e0.elapsed_time(e1) for e0, e1 in evs[name]])) * 1e3)
    for name in calls:
        res[f"{name}_us"] = round(float(np.median(meds[name])), 2)
        res[f"{name}_us_spread"] = [round(min(meds[name]), 2), round(max(meds[name]), 2)]
    res["huff_over_idct"] = round(res["huff_us"] / res["idct_us"], 2)
    res["huff_files_per_s_one_stream"] = round(B / res["huff_us"] * 1e6, 1)

    # -- 5. batches in flight
    streams = [torch.cuda.Stream() for _ in range(a.inflight)]
    stats = [[torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3)] for _ in range(n_buf)]

    def measure(run):
        rates = []
        for _ in range(a.repeats):
            run(a.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(a.steps)
            torch.cuda.synchronize()
            rates.append(B * a.steps / (time.perf_counter() - t0))
        return round(float(np.median(rates)), 1), [round(min(rates), 1), round(max(rates), 1)]

    def huff_only(n):
        for k in range(n):
            b = bufs[k % n_buf]
            ents[0].run(b[0], b[1], b[3], b[2], b[9], stream=streams[k % a.inflight], status=stats[k % n_buf][0])
    res["inflight_huff_files_per_s"], res["inflight_huff_files_per_s_spread"] = measure(huff_only)
    key = f"host_decode_files_per_s_{a.threads}_threads"
    res["device_over_host_decode"] = round(res["inflight_huff_files_per_s"] / res[key], 3)

    if not a.kernel_only:
        t50 = cfg.resnet50_tables()
        q50 = np.loadtxt(os.path.join(ROOT, "tests", "golden", "resnet50_Q"), dtype=np.int32)
        net = NetWork(t50)
        net.Init(synth.synth_model(t50, q50, 0), synth.q_text(q50), device=dev)
        pp_aa = P.Preprocessor(net, P.TORCHVISION_PIL, "RGB")
        conv = Y.DeviceConverter(Y.Desc(layout=layout, sub=sub))
        runners = [Runner(None, net) for _ in range(a.inflight)]
        clss = [K.DeviceClassifier(net, 5) for _ in range(a.inflight)]

        def step(kind, i, k):
            data, scan, coef, jp, qt, planes, yc, sc, px, work = bufs[k]
            if kind == "bytes":
                ents[0].run(data, scan, jp, coef, work, status=stats[k][0])
            dec.run(coef, jp, qt, planes, yc, sc, status=stats[k][1])
            conv.run(planes, yc, px, sc, status=stats[k][2])
            return clss[i].run(runners[i].run_batch(pp_aa(px, sc, out="q")[0], concurrency=1))
        for kind in ("coef", "bytes"):
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
            res[f"inflight_{kind}"], res[f"inflight_{kind}_spread"] = measure(run)
            del graphs
        res["inflight_bytes_over_coef"] = round(res["inflight_bytes"] / res["inflight_coef"], 4)
    line = json.dumps(res)
    print(line)
    out = a.out or os.path.join(ROOT, "profiles", f"jpeg_huff_time_b{B}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
