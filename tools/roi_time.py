#!/usr/bin/env python3
"""Cost of second-stage crops on the device (tf2_roi_select / tf2_roi_crop, roi_crop.hip) at --batch source images of --src-h x
--src-w uint8 RGB, --max-rois slots an image and SqueezeNet 1.1's 227 x 227 input (batch 32, 4 slots: 128 crops).  HIP events on one
stream around --inner calls captured back to back in one graph (no host launch path inside the interval), after --warmup replays,
over --steps replays, divided by --inner: median, 10th and 90th percentile in microseconds a call of
  select        one tf2_roi_select call on a synthetic det [B, 21, 200, 5] whose every image has more candidates than slots
  crop          one tf2_roi_crop call on that table (every slot filled; boxes of a quarter to the whole of the image), int8 and float32
  select_worst  the same at the largest desc: det [B, 256, 256, 5] with every class taken, 64 slots an image (64 rounds over 65,536 rows)
  select_refill the same desc with one row a class and equal scores: all 64 winners are rows of ONE thread, which scans its rows 16 times
  preprocess    one tf2_preprocess call producing the same number of 227 x 227 outputs from whole images (each source --max-rois
                times): the yardstick, unchanged code doing the same taps per output pixel
and crop_over_preprocess, the ratio of the medians.  Then images/s (source images) of two steps with --inflight batches in flight (one
captured graph per stream, replayed round robin), SSD300 and SqueezeNet 1.1 with synthetic weights:
  detector      tf2_preprocess + tf2_ssd_run
  cascade       the same + select + crop + SqueezeNet 1.1 on the crops + tf2_emb_match against --gallery rows
(min_score is the detector's conf_thresh and every class is taken, so the synthetic detector fills the slots; cascade_filled_slots
says how many it filled).  Prints one JSON line; --out writes it to a file as well.  `--kernel-only` stops after the event times.

`--antialias` measures the antialiased crop instead (tf2_roi_crop_aa, roi_crop_aa.hip) and writes profiles/roi_aa_time_b32.json unless
--out names another file: on the same table and sources, the same way,
  crop_aa        one tf2_roi_crop_aa call, int8 and float32
  crop           one tf2_roi_crop call on the same table
  preprocess_aa  one tf2_preprocess_aa call producing the same number of 227 x 227 outputs from whole images: the yardstick, the same
                 tile kernel at the whole image's scale
crop_aa_over_preprocess_aa and crop_aa_over_crop, the ratios of the medians, the mean scale of the table's boxes, and the images/s of
the cascade with --inflight batches in flight with the plain and with the antialiased crop (their timed repeats alternate)."""
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
    ap.add_argument("--max-rois", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--gallery", type=int, default=1000)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--antialias", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tf2_amd import config as cfg, embed as E, preprocess as P, roi as R, ssd, synth
    from tf2_amd.network import NetWork, Runner
    dev = "cuda:0"
    rng = np.random.default_rng(7)
    B, M = a.batch, a.max_rois

    def make_net(t, q, seed):
        net = NetWork(t)
        net.Init(synth.synth_model(t, q, seed), synth.q_text(q), device=dev)
        return net

    res = dict(batch=B, src_hw=[a.src_h, a.src_w], max_rois=M, crops=B * M, out_hw=[227, 227], steps=a.steps, inner=a.inner,
               inflight=a.inflight)
    tsq = cfg.squeezenet11_tables()
    face = make_net(tsq, synth.synth_q_values(tsq, 21, spread=2), 21)
    n_sets = 2 * a.inflight
    images = [[rng.integers(0, 256, (a.src_h, a.src_w, 3), dtype=np.uint8) for _ in range(B)] for _ in range(n_sets)]
    srcs = [P.pack(s, P.SSD300, dev) for s in images]
    s = torch.cuda.current_stream()

    def timed(fn, tag):
        """per-call device time of fn: --inner calls captured back to back in one graph (no host launch path between them), an event
        pair around each of --steps replays, the interval divided by --inner"""
        side = torch.cuda.Stream()
        side.wait_stream(s)
        with torch.cuda.stream(side):
            fn(0)
            side.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=side):
                for k in range(a.inner):
                    fn(k)
        s.wait_stream(side)
        for _ in range(a.warmup):
            gr.replay()
        evs = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            gr.replay()
            e1.record(s)
            evs.append((e0, e1))
        torch.cuda.synchronize()
        us = np.array([e0.elapsed_time(e1) for e0, e1 in evs]) * 1e3 / a.inner
        res[f"{tag}_us"] = round(float(np.median(us)), 2)
        res[f"{tag}_us_p10_p90"] = [round(float(np.percentile(us, 10)), 2), round(float(np.percentile(us, 90)), 2)]

    # -- the kernels alone: a synthetic det with more candidates than slots in every image
    det = np.zeros((B, 21, 200, 5), np.float32)
    det[..., 0] = rng.uniform(0.0, 1.0, det.shape[:3])
    x1, y1 = rng.uniform(0.0, 0.5, det.shape[:3]), rng.uniform(0.0, 0.5, det.shape[:3])
    det[..., 1], det[..., 2] = x1, y1
    det[..., 3], det[..., 4] = x1 + rng.uniform(0.25, 0.5, det.shape[:3]), y1 + rng.uniform(0.25, 0.5, det.shape[:3])
    det_d = torch.from_numpy(det).to(dev)
    counts_d = torch.full((B, 21), 200, dtype=torch.int32, device=dev)
    crop = R.DeviceCropper(face, P.SQUEEZENET, "RGB", classes=(15,), min_score=0.5, max_rois=M)
    rois = torch.empty(B * M, R.ROI_WORDS, dtype=torch.int32, device=dev)
    roi_n = torch.empty(B, dtype=torch.int32, device=dev)
    timed(lambda k: crop.select(det_d, counts_d, srcs[k % n_sets][1], rois=rois, roi_counts=roi_n), "select")
    torch.cuda.synchronize()
    assert int(roi_n.sum()) == B * M, "the synthetic det must fill every slot"
    if a.antialias:
        return antialias(a, res, timed, face, make_net, srcs, rois, crop, rng)
    big = np.zeros((B, 256, 256, 5), np.float32)
    big[..., 0] = rng.uniform(0.0, 1.0, big.shape[:3])
    big[..., 1:3], big[..., 3:5] = 0.25, 0.75
    big[..., 3][rng.uniform(0, 1, big.shape[:3]) < 0.5] = 0.25                      # half the rows have no width: skipped every round
    big_d, big_c = torch.from_numpy(big).to(dev), torch.full((B, 256), 256, dtype=torch.int32, device=dev)
    worst = R.DeviceCropper(face, P.SQUEEZENET, "RGB", num_classes=256, top_k=256, classes=tuple(range(1, 256)), min_score=0.0, max_rois=64)
    w_rois = torch.empty(B * 64, R.ROI_WORDS, dtype=torch.int32, device=dev)
    timed(lambda k: worst.select(big_d, big_c, srcs[k % n_sets][1], rois=w_rois, roi_counts=roi_n), "select_worst")
    # the same desc with one row a class and equal scores: every winner is a row (c, 0) of thread 0, which refills its cache 15 times
    big_d[..., 0] = 0.5
    big_d[..., 3] = 0.75
    big_c.fill_(1)
    timed(lambda k: worst.select(big_d, big_c, srcs[k % n_sets][1], rois=w_rois, roi_counts=roi_n), "select_refill")
    torch.cuda.synchronize()
    assert int(roi_n.sum()) == B * 64
    del big_d, big_c
    for out, dtype in (("q", torch.int8), ("f32", torch.float32)):
        buf = torch.empty(B * M, 3, 227, 227, dtype=dtype, device=dev)
        st = torch.empty(B * M, dtype=torch.int32, device=dev)
        timed(lambda k: crop.crop(*srcs[k % n_sets], rois, out=out, images=buf, status=st), f"crop_{out}")
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0
    # the yardstick: tf2_preprocess making B * M outputs of 227 x 227 from whole images (every source M times)
    pp = P.Preprocessor(face, P.SQUEEZENET, "RGB")
    whole = []
    for px, sr in srcs:
        rec = sr.cpu().numpy().view(P.SRC_DTYPE).reshape(-1).copy()
        rec["resize_h"], rec["resize_w"], rec["crop_y"], rec["crop_x"] = 227, 227, 0, 0
        rec = np.repeat(rec, M)
        whole.append((px, torch.from_numpy(rec.view(np.int32).reshape(len(rec), P.SRC_WORDS).copy()).to(dev)))
    for out in ("q", "f32"):
        timed(lambda k: pp(*whole[k % n_sets], out=out), f"preprocess_{out}")
        res[f"crop_over_preprocess_{out}"] = round(res[f"crop_{out}_us"] / res[f"preprocess_{out}_us"], 4)
    if a.kernel_only:
        return finish(res, a)

    # -- throughput with batches in flight: the detector alone, and the whole cascade
    t300 = cfg.ssd300_tables()
    net300 = make_net(t300, np.array(synth.synth_q_values(t300, 5, spread=1)), 0)
    pp300 = P.Preprocessor(net300, P.SSD300, "RGB")
    g = rng.normal(0, 1, (a.gallery, 128)).astype(np.float32)
    gallery = torch.from_numpy(g / np.linalg.norm(g, axis=1, keepdims=True).astype(np.float32)).to(dev)
    cas_crop = R.DeviceCropper(face, P.SQUEEZENET, "RGB", classes=tuple(range(1, 21)), min_score=0.01, max_rois=M)
    dets = [ssd.DeviceDetector(net300, net300.plan, ssd.VOC) for _ in range(a.inflight)]
    runners = [Runner(None, face) for _ in range(a.inflight)]
    matchers = [E.DeviceMatcher(face, 5) for _ in range(a.inflight)]
    keep = {}

    def detector(i, k):
        px, sr = srcs[k]
        return dets[i].run(pp300(px, sr, out="q")[0]) + (px, sr)

    def cascade(i, k):
        d, c, px, sr = detector(i, k)
        crops, st, _, n = cas_crop(d, c, px, sr, out="q")
        keep[k] = n
        return matchers[i].match(runners[i].run_batch(crops, concurrency=1), gallery)

    streams = [torch.cuda.Stream() for _ in range(a.inflight)]
    for name, fn in (("detector", detector), ("cascade", cascade)):
        graphs = {}
        for k in range(n_sets):
            i = k % a.inflight
            streams[i].wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(streams[i]):
                fn(i, k)                                           # warm the launch plans of this stream's workspaces
                torch.cuda.current_stream().synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=streams[i]):
                    fn(i, k)
            torch.cuda.current_stream().wait_stream(streams[i])
            graphs[k] = gr
        torch.cuda.synchronize()

        def run(n):
            for k in range(n):
                with torch.cuda.stream(streams[k % a.inflight]):
                    graphs[k % n_sets].replay()
        run(a.warmup)
        torch.cuda.synchronize()
        rates = []
        for _ in range(3):
            t0 = time.perf_counter()
            run(a.steps)
            torch.cuda.synchronize()
            rates.append(B * a.steps / (time.perf_counter() - t0))
        res[f"{name}_inflight_images_per_s"] = round(float(np.median(rates)), 1)
        res[f"{name}_inflight_images_per_s_min_max"] = [round(min(rates), 1), round(max(rates), 1)]
        if name == "cascade":
            res["cascade_filled_slots"] = int(sum(int(v.sum()) for v in keep.values())) // len(keep)
        del graphs
    res["cascade_over_detector"] = round(res["cascade_inflight_images_per_s"] / res["detector_inflight_images_per_s"], 4)
    finish(res, a)


def antialias(a, res, timed, face, make_net, srcs, rois, crop, rng):
    """the --antialias measurement (the module docstring); rois: the table `crop.select` left on the device"""
    import torch
    from tf2_amd import config as cfg, embed as E, preprocess as P, roi as R, ssd, synth
    from tf2_amd.network import Runner
    from dataclasses import replace
    dev, B, M, n_sets = "cuda:0", a.batch, a.max_rois, len(srcs)
    crop_aa = R.DeviceCropper(face, P.SQUEEZENET, "RGB", classes=(15,), min_score=0.5, max_rois=M, antialias=True)
    table = R.rois_to_host(rois)
    res["mean_box_scale_xy"] = [round(float(np.mean((table["x1"] - table["x0"]) / 227.0)), 3),
                                round(float(np.mean((table["y1"] - table["y0"]) / 227.0)), 3)]
    res["whole_image_scale_xy"] = [round(a.src_w / 227.0, 3), round(a.src_h / 227.0, 3)]
    pre_aa = replace(P.SQUEEZENET, antialias=True)
    pp = P.Preprocessor(face, pre_aa, "RGB")
    whole = []
    for px, sr in srcs:
        rec = sr.cpu().numpy().view(P.SRC_DTYPE).reshape(-1).copy()
        rec["resize_h"], rec["resize_w"], rec["crop_y"], rec["crop_x"] = 227, 227, 0, 0
        rec = np.repeat(rec, M)
        whole.append((px, torch.from_numpy(rec.view(np.int32).reshape(len(rec), P.SRC_WORDS).copy()).to(dev)))
    for out, dtype in (("q", torch.int8), ("f32", torch.float32)):
        buf = torch.empty(B * M, 3, 227, 227, dtype=dtype, device=dev)
        st = torch.empty(B * M, dtype=torch.int32, device=dev)
        for tag, c in ((f"crop_aa_{out}", crop_aa), (f"crop_{out}", crop)):
            timed(lambda k: c.crop(*srcs[k % n_sets], rois, out=out, images=buf, status=st), tag)
            torch.cuda.synchronize()
            assert int(st.abs().sum()) == 0
        timed(lambda k: pp(*whole[k % n_sets], out=out), f"preprocess_aa_{out}")
        res[f"crop_aa_over_preprocess_aa_{out}"] = round(res[f"crop_aa_{out}_us"] / res[f"preprocess_aa_{out}_us"], 4)
        res[f"crop_aa_over_crop_{out}"] = round(res[f"crop_aa_{out}_us"] / res[f"crop_{out}_us"], 4)
    if a.kernel_only:
        return finish(res, a)

    # -- the cascade with batches in flight, plain and antialiased crops; the timed repeats of the two alternate
    t300 = cfg.ssd300_tables()
    net300 = make_net(t300, np.array(synth.synth_q_values(t300, 5, spread=1)), 0)
    pp300 = P.Preprocessor(net300, P.SSD300, "RGB")
    g = rng.normal(0, 1, (a.gallery, 128)).astype(np.float32)
    gallery = torch.from_numpy(g / np.linalg.norm(g, axis=1, keepdims=True).astype(np.float32)).to(dev)
    croppers = {name: R.DeviceCropper(face, P.SQUEEZENET, "RGB", classes=tuple(range(1, 21)), min_score=0.01, max_rois=M, antialias=aa)
                for name, aa in (("cascade", False), ("cascade_aa", True))}
    dets = [ssd.DeviceDetector(net300, net300.plan, ssd.VOC) for _ in range(a.inflight)]
    runners = [Runner(None, face) for _ in range(a.inflight)]
    matchers = [E.DeviceMatcher(face, 5) for _ in range(a.inflight)]
    streams = [torch.cuda.Stream() for _ in range(a.inflight)]
    graphs, keep = {}, {}

    def cascade(name, i, k):
        px, sr = srcs[k]
        d, c = dets[i].run(pp300(px, sr, out="q")[0])
        crops, st, _, n = croppers[name](d, c, px, sr, out="q")
        keep[name, k] = (n, st)
        return matchers[i].match(runners[i].run_batch(crops, concurrency=1), gallery)

    for name in croppers:
        for k in range(n_sets):
            i = k % a.inflight
            streams[i].wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(streams[i]):
                cascade(name, i, k)                                # warm the launch plans of this stream's workspaces
                torch.cuda.current_stream().synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=streams[i]):
                    cascade(name, i, k)
            torch.cuda.current_stream().wait_stream(streams[i])
            graphs[name, k] = gr
    torch.cuda.synchronize()

    def run(name, n):
        for k in range(n):
            with torch.cuda.stream(streams[k % a.inflight]):
                graphs[name, k % n_sets].replay()

    rates = {name: [] for name in croppers}
    for name in croppers:
        run(name, a.warmup)
    torch.cuda.synchronize()
    for _ in range(3):
        for name in croppers:
            t0 = time.perf_counter()
            run(name, a.steps)
            torch.cuda.synchronize()
            rates[name].append(B * a.steps / (time.perf_counter() - t0))
    for name in croppers:
        res[f"{name}_inflight_images_per_s"] = round(float(np.median(rates[name])), 1)
        res[f"{name}_inflight_images_per_s_min_max"] = [round(min(rates[name]), 1), round(max(rates[name]), 1)]
        res[f"{name}_filled_slots"] = int(sum(int(keep[name, k][0].sum()) for k in range(n_sets))) // n_sets
        bits = torch.cat([keep[name, k][1] for k in range(n_sets)]).cpu().numpy()
        assert set(np.unique(bits).tolist()) <= {0, R.EMPTY}, np.unique(bits)         # clipped boxes: nothing refused
    res["cascade_aa_over_cascade"] = round(res["cascade_aa_inflight_images_per_s"] / res["cascade_inflight_images_per_s"], 4)
    finish(res, a)


def finish(res, a):
    if a.antialias and not a.out:
        a.out = os.path.join(ROOT, "profiles", "roi_aa_time_b32.json")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
