#!/usr/bin/env python3
"""Cost of on-device detection accuracy (tf2_det_eval_run) behind an SSD300 step (synthetic weights): HIP events on one stream
around, in interleaved rounds of the same process,
  plain         tf2_ssd_run alone (DeviceDetector.run)
  with_eval     tf2_ssd_run, then tf2_det_eval_run on its det / counts (DeviceEvaluator.update), the evaluator's part between its
                own pair of events
Ground truth: per image 1..--max-gt boxes (default 42) drawn from the image's own detections of a first run, jittered, one in five
difficult, so that the matching path runs (true positives, duplicates and ignored rows exist) in the classes that have ground
truth; batch 32, top_k 200, 21 classes by default.  Medians over --steps steps after --warmup.  Prints one JSON line: the
evaluator's time in microseconds and as a share of the plain step.  Under `rocprofv3 --kernel-trace --stats -- python
tools/ssd_eval_time.py` the kernel statistics show det_eval_kernel beside ssd_heads_kernel / ssd_select_kernel."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--width-div", type=int, default=1)
    ap.add_argument("--loc-q", type=int, default=6)
    ap.add_argument("--conf-q", type=int, default=6)
    ap.add_argument("--max-gt", type=int, default=42)
    a = ap.parse_args()
    import torch
    from tf2_amd import config as cfg, ssd, synth
    from tf2_amd.network import NetWork
    t = cfg.ssd300_tables(width_div=a.width_div)
    plan = cfg.build_plan(t)
    q = np.array(synth.synth_q_values(t, 5, spread=1))
    pos = 3
    at = {}
    for L in plan:                                    # file-order Q positions (tests/test_ssd.py qrows)
        if not L.ipool:
            at[L.index] = pos; pos += L.N
        elif L.ipool == 2:
            pos += L.N
    for lr, cr in ssd.head_rows(plan):
        q[at[lr]:at[lr] + plan[lr].N] = a.loc_q
        q[at[cr]:at[cr] + plan[cr].N] = a.conf_q
    net = NetWork(t)
    net.Init(synth.synth_model(t, q, 5), synth.q_text(q), device="cuda:0")
    x = torch.from_numpy(np.ascontiguousarray(synth.synth_images(t, a.batch, 11))).to("cuda:0")
    det = ssd.DeviceDetector(net, plan, ssd.VOC)
    C, K = det.num_classes, det.top_k
    ev = ssd.DeviceEvaluator(C, K, a.batch, a.max_gt, 0.5, device="cuda:0")
    s = torch.cuda.current_stream()

    # ground truth from the step's own detections
    d0, c0 = (v.cpu().numpy() for v in det.run(x))
    rng = np.random.default_rng(3)
    images = []
    for b in range(a.batch):
        rows = []
        for _ in range(int(rng.integers(1, a.max_gt + 1))):
            c = int(rng.integers(1, C))
            if c0[b, c] == 0:
                continue
            r = int(rng.integers(0, c0[b, c]))
            box = d0[b, c, r, 1:].astype(np.float64) + rng.normal(0, 0.004, 4)
            x1, x2 = sorted((box[0], box[2]))
            y1, y2 = sorted((box[1], box[3]))
            rows.append((x1, y1, x2, y2, c, rng.random() < 0.2))
        images.append(np.asarray(rows, np.float64).reshape(-1, 6))
    gt_h, cnt_h = ssd.pack_ground_truth(images, a.max_gt)
    gt = torch.from_numpy(gt_h.view(np.int32).reshape(a.batch, a.max_gt, 6)).to("cuda:0")
    cnt = torch.from_numpy(cnt_h).to("cuda:0")
    slots = torch.arange(a.batch, dtype=torch.int32, device="cuda:0")
    status = torch.empty(a.batch, dtype=torch.int32, device="cuda:0")

    def timed(with_eval, n):
        out = []
        for _ in range(n):
            e0, em, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record(s)
            d, c = det.run(x)
            em.record(s)
            if with_eval:
                ev.update(d, c, gt, cnt, slots, status=status)
            e1.record(s)
            out.append((e0, em, e1))
        torch.cuda.synchronize()
        return out

    for w in (False, True):
        timed(w, a.warmup)
    assert status.cpu().tolist() == [0] * a.batch
    # interleaved rounds, so that clock and thermal drift fall on both equally
    t_plain, t_eval = [], []
    for _ in range(5):
        t_plain += timed(False, a.steps // 5)
        t_eval += timed(True, a.steps // 5)
    ms = lambda pairs: float(np.median([p.elapsed_time(q) for p, q in pairs]))
    res = dict(batch=a.batch, width_div=a.width_div, classes=C, top_k=K, max_gt=a.max_gt, steps=len(t_eval),
               plain_step_ms=ms([(e0, e1) for e0, _, e1 in t_plain]),
               with_eval_step_ms=ms([(e0, e1) for e0, _, e1 in t_eval]),
               eval_us=1e3 * ms([(em, e1) for _, em, e1 in t_eval]))
    res["eval_share_of_step_pct"] = 100.0 * res["eval_us"] * 1e-3 / res["plain_step_ms"]
    res["step_delta_us"] = 1e3 * (res["with_eval_step_ms"] - res["plain_step_ms"])
    m = ssd.match_reference(d0, c0, gt_h, cnt_h, 0.5)
    res["gt_per_image_mean"] = float(cnt_h.mean())
    res["rows_per_class_mean"] = float(c0[:, 1:].mean())
    res["true_positives"], res["ignored"], res["duplicates"] = int((m.flags == 1).sum()), int((m.flags == -1).sum()), int(m.duplicates.sum())
    r = ev.result()
    res["map"] = r["map"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
