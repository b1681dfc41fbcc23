#!/usr/bin/env python3
"""Cost of on-device SSD detection at SSD300 (synthetic weights): HIP events on one stream around
  ordinary      the network step on the ordinary plan (Runner.run_batch, what bench.py --net ssd300 times)
  kept          the same step on the outputs-kept plan (tf2_ssd_run up to its mark event)
  detect        heads -> boxes + probabilities, select + NMS (tf2_ssd_run from the mark event to its end)
  ssd_run       the whole tf2_ssd_run
Medians over --steps steps after --warmup.  The head Qs are set so that dequantised loc stays within +-2 and the class
logits within +-2 (--conf-q 6): the softmax is flat, nearly every prior passes conf_thresh 0.01 in every class -- the
selection's worst case.  Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats -- python tools/ssd_detect_time.py`
the kernel statistics attribute the detect time to ssd_heads_kernel / ssd_select_kernel."""
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
    a = ap.parse_args()
    import torch
    from tf2_amd import config as cfg, ssd, synth
    from tf2_amd.network import NetWork, Runner
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
    runner = Runner(None, net)
    det = ssd.DeviceDetector(net, plan, ssd.VOC)
    s = torch.cuda.current_stream()

    def timed(fn, n):
        out = []
        for _ in range(n):
            e0, em, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record(s)
            fn(em)
            e1.record(s)
            out.append((e0, em, e1))
        torch.cuda.synchronize()
        return out

    ordinary = lambda em: (runner.run_batch(x, concurrency=0), em.record(s))
    kept = lambda em: det.run(x, mark=em)
    for fn in (ordinary, kept):
        timed(fn, a.warmup)
    # interleaved rounds, so that clock and thermal drift fall on both equally
    t_ord, t_run = [], []
    for _ in range(5):
        t_ord += timed(ordinary, a.steps // 5)
        t_run += timed(kept, a.steps // 5)
    ms = lambda pairs: float(np.median([p.elapsed_time(q) for p, q in pairs]))
    res = dict(batch=a.batch, width_div=a.width_div, steps=len(t_run),
               ordinary_ms=ms([(e0, e1) for e0, _, e1 in t_ord]),
               kept_ms=ms([(e0, em) for e0, em, _ in t_run]),
               detect_ms=ms([(em, e1) for _, em, e1 in t_run]),
               ssd_run_ms=ms([(e0, e1) for e0, _, e1 in t_run]))
    res["kept_over_ordinary_pct"] = 100.0 * (res["kept_ms"] / res["ordinary_ms"] - 1.0)
    res["detect_over_ordinary_pct"] = 100.0 * res["detect_ms"] / res["ordinary_ms"]
    d, c, boxes, probs = det.run(x, decoded=True)
    torch.cuda.synchronize()
    res["candidates_per_class_mean"] = float((probs[..., 1:] > 0.01).sum(1).float().mean())
    res["kept_per_class_mean"] = float(c[:, 1:].float().mean())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
