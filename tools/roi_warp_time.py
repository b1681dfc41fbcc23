#!/usr/bin/env python3
"""Cost of aligned crops on the device (tf2_roi_fit / tf2_roi_warp, roi_warp.hip) at --batch source images of --src-h x --src-w uint8
RGB, --max-rois slots an image and SqueezeNet 1.1's 227 x 227 input (batch 32, 4 slots: 128 crops).  The slots are the table
tf2_roi_select makes of a synthetic det (tools/roi_time.py's: every slot filled, boxes of a quarter to the whole of the image); each
slot has five box-relative landmarks, the face template rolled by up to +-30 degrees at 0.5 .. 0.9 of the box.  HIP events on one
stream around --inner calls captured back to back in one graph (no host launch path inside the interval), after --warmup replays,
over --steps replays, divided by --inner: median, 10th and 90th percentile in microseconds a call of
  fit           one tf2_roi_fit call on the table and the landmarks
  warp          one tf2_roi_warp call on the transforms it made, int8 and float32
  warp_upright  the same with each slot's transform replaced by its box as a matrix (no roll): the window tf2_roi_crop resamples
  crop          one tf2_roi_crop call on the same slots, as boxes
  crop_aa       one tf2_roi_crop_aa call on the same slots, as boxes
and warp_over_crop, warp_over_crop_aa, the ratios of the medians.  Then images/s (source images) of the cascade -- tf2_preprocess +
tf2_ssd_run + select + (crop | fit + warp) + SqueezeNet 1.1 + tf2_emb_match against --gallery rows, SSD300 and SqueezeNet 1.1 with
synthetic weights -- with --inflight batches in flight (one captured graph per stream, replayed round robin), with the plain crop and
with fit + warp; their timed repeats alternate.  Prints one JSON line and writes profiles/roi_warp_time_b32.json unless --out names
another file.  `--kernel-only` stops after the event times."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FACE_112 = [(38.2946, 51.6963), (73.5318, 51.5014), (56.0252, 71.7366), (41.5493, 92.3655), (70.7299, 92.2041)]


def landmarks(rng, n, tpl, hw):
    """box-relative landmarks float32 [n, K, 2]: the template about the box's centre, rolled and scaled"""
    out = np.zeros((n, len(tpl), 2), np.float32)
    rel = np.asarray(tpl, np.float64) / [hw[1], hw[0]] - 0.5
    for s in range(n):
        th = np.radians(rng.uniform(-30.0, 30.0))
        rot = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        out[s] = ((rel * rng.uniform(0.5, 0.9)) @ rot.T + 0.5).astype(np.float32)
    return out


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_warp_time_b32.json"))
    a = ap.parse_args()
    import torch
    from tf2_amd import align as A, config as cfg, embed as E, preprocess as P, roi as R, ssd, synth
    from tf2_amd.network import NetWork, Runner
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = "cuda:0"
    rng = np.random.default_rng(7)
    B, M = a.batch, a.max_rois
    S = B * M

    def make_net(t, q, seed):
        net = NetWork(t)
        net.Init(synth.synth_model(t, q, seed), synth.q_text(q), device=dev)
        return net

    res = dict(batch=B, src_hw=[a.src_h, a.src_w], max_rois=M, crops=S, out_hw=[227, 227], steps=a.steps, inner=a.inner,
               inflight=a.inflight, n_points=len(FACE_112))
    tsq = cfg.squeezenet11_tables()
    face = make_net(tsq, synth.synth_q_values(tsq, 21, spread=2), 21)
    n_sets = 2 * a.inflight
    images = [[rng.integers(0, 256, (a.src_h, a.src_w, 3), dtype=np.uint8) for _ in range(B)] for _ in range(n_sets)]
    srcs = [P.pack(s, P.SSD300, dev) for s in images]
    s = torch.cuda.current_stream()

    def timed(fn, tag):
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

    # -- the kernels alone: the table of a synthetic det with more candidates than slots in every image
    det = np.zeros((B, 21, 200, 5), np.float32)
    det[..., 0] = rng.uniform(0.0, 1.0, det.shape[:3])
    x1, y1 = rng.uniform(0.0, 0.5, det.shape[:3]), rng.uniform(0.0, 0.5, det.shape[:3])
    det[..., 1], det[..., 2] = x1, y1
    det[..., 3], det[..., 4] = x1 + rng.uniform(0.25, 0.5, det.shape[:3]), y1 + rng.uniform(0.25, 0.5, det.shape[:3])
    det_d = torch.from_numpy(det).to(dev)
    counts_d = torch.full((B, 21), 200, dtype=torch.int32, device=dev)
    crop = R.DeviceCropper(face, P.SQUEEZENET, "RGB", classes=(15,), min_score=0.5, max_rois=M)
    crop_aa = R.DeviceCropper(face, P.SQUEEZENET, "RGB", classes=(15,), min_score=0.5, max_rois=M, antialias=True)
    tpl = A.scaled_template(FACE_112, (112, 112), (227, 227))
    al = A.DeviceAligner(face, P.SQUEEZENET, tpl, "RGB", space=1)
    rois, roi_n = crop.select(det_d, counts_d, srcs[0][1])
    torch.cuda.synchronize()
    assert int(roi_n.sum()) == S, "the synthetic det must fill every slot"
    table = R.rois_to_host(rois)
    res["mean_box_scale_xy"] = [round(float(np.mean((table["x1"] - table["x0"]) / 227.0)), 3),
                                round(float(np.mean((table["y1"] - table["y0"]) / 227.0)), 3)]
    lmk = torch.from_numpy(landmarks(rng, S, tpl, (227, 227))).to(dev)
    xf = torch.empty(S, A.XFORM_WORDS, dtype=torch.int32, device=dev)
    fst = torch.empty(S, dtype=torch.int32, device=dev)
    timed(lambda k: al.fit(rois, lmk, xforms=xf, status=fst), "fit")
    torch.cuda.synchronize()
    assert int(fst.abs().sum()) == 0
    fitted = A.xforms_to_host(xf)
    res["mean_fit_scale"] = round(float(np.mean(np.hypot(fitted["m"][:, 0], fitted["m"][:, 3]))), 3)
    upright = A.empty_xforms(S)                                     # the box as a matrix: x0 + (x + .5) * (x1 - x0) / 227
    upright["image"] = table["image"]
    upright["m"][:, 0], upright["m"][:, 2] = (table["x1"].astype(np.float64) - table["x0"]) / 227.0, table["x0"]
    upright["m"][:, 4], upright["m"][:, 5] = (table["y1"].astype(np.float64) - table["y0"]) / 227.0, table["y0"]
    xf_up = A.xforms_to_device(upright, dev)
    for out, dtype in (("q", torch.int8), ("f32", torch.float32)):
        buf = torch.empty(S, 3, 227, 227, dtype=dtype, device=dev)
        st = torch.empty(S, dtype=torch.int32, device=dev)
        for tag, fn in ((f"warp_{out}", lambda k: al.warp(*srcs[k % n_sets], xf, out=out, images=buf, status=st)),
                        (f"warp_upright_{out}", lambda k: al.warp(*srcs[k % n_sets], xf_up, out=out, images=buf, status=st)),
                        (f"crop_{out}", lambda k: crop.crop(*srcs[k % n_sets], rois, out=out, images=buf, status=st)),
                        (f"crop_aa_{out}", lambda k: crop_aa.crop(*srcs[k % n_sets], rois, out=out, images=buf, status=st))):
            timed(fn, tag)
            torch.cuda.synchronize()
            assert int(st.abs().sum()) == 0, tag
        res[f"warp_over_crop_{out}"] = round(res[f"warp_{out}_us"] / res[f"crop_{out}_us"], 4)
        res[f"warp_over_crop_aa_{out}"] = round(res[f"warp_{out}_us"] / res[f"crop_aa_{out}_us"], 4)
    if a.kernel_only:
        return finish(res, a)

    # -- the cascade with batches in flight, plain crops and aligned ones; the timed repeats of the two alternate
    t300 = cfg.ssd300_tables()
    net300 = make_net(t300, np.array(synth.synth_q_values(t300, 5, spread=1)), 0)
    pp300 = P.Preprocessor(net300, P.SSD300, "RGB")
    g = rng.normal(0, 1, (a.gallery, 128)).astype(np.float32)
    gallery = torch.from_numpy(g / np.linalg.norm(g, axis=1, keepdims=True).astype(np.float32)).to(dev)
    cas_crop = R.DeviceCropper(face, P.SQUEEZENET, "RGB", classes=tuple(range(1, 21)), min_score=0.01, max_rois=M)
    dets = [ssd.DeviceDetector(net300, net300.plan, ssd.VOC) for _ in range(a.inflight)]
    runners = [Runner(None, face) for _ in range(a.inflight)]
    matchers = [E.DeviceMatcher(face, 5) for _ in range(a.inflight)]
    streams = [torch.cuda.Stream() for _ in range(a.inflight)]
    names = ("cascade", "cascade_warp")
    graphs, keep = {}, {}

    def cascade(name, i, k):
        px, sr = srcs[k]
        d, c = dets[i].run(pp300(px, sr, out="q")[0])
        if name == "cascade":
            crops, st, _, n = cas_crop(d, c, px, sr, out="q")
        else:
            table_k, n = cas_crop.select(d, c, sr)
            crops, st, _, _ = al(table_k, lmk, px, sr, out="q")
        keep[name, k] = (n, st)
        return matchers[i].match(runners[i].run_batch(crops, concurrency=1), gallery)

    for name in names:
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

    rates = {name: [] for name in names}
    for name in names:
        run(name, a.warmup)
    torch.cuda.synchronize()
    for _ in range(3):
        for name in names:
            t0 = time.perf_counter()
            run(name, a.steps)
            torch.cuda.synchronize()
            rates[name].append(B * a.steps / (time.perf_counter() - t0))
    for name in names:
        res[f"{name}_inflight_images_per_s"] = round(float(np.median(rates[name])), 1)
        res[f"{name}_inflight_images_per_s_min_max"] = [round(min(rates[name]), 1), round(max(rates[name]), 1)]
        res[f"{name}_filled_slots"] = int(sum(int(keep[name, k][0].sum()) for k in range(n_sets))) // n_sets
        bits = torch.cat([keep[name, k][1] for k in range(n_sets)]).cpu().numpy()
        assert set(np.unique(bits).tolist()) <= {0, R.EMPTY}, np.unique(bits)
    res["cascade_warp_over_cascade"] = round(res["cascade_warp_inflight_images_per_s"] / res["cascade_inflight_images_per_s"], 4)
    finish(res, a)


def finish(res, a):
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
