#!/usr/bin/env python3
"""Full model in, channel-pruned model out: one DNS-CP decision on the device and the export (tf2_amd.dnscp.DevicePruner, prune_model).
  python tools/dnscp_model.py TABLES STREAM Q_FILE --out model_p.bin --out-q model_p_Q --out-tables tables_p.json
         [--keep keep.npz] [--c-rate 0.1] [--alpha-low 0.95] [--alpha-high 1.05]
TABLES: resnet50 | vgg16 | ssd300 | squeezenet | tiny, or a tables .json (tests/golden/tables_*.json); STREAM: raw little-endian float32
in LoadModel order; Q_FILE: the Q values as text.  Without --keep: tf2_dnscp_stats on the stream, thresholds from its sums, one
tf2_dnscp_step from "everything kept" -- the mask of the reference's iteration 0.  With --keep (an .npz of "row<l>" uint8 arrays, as a
training loop that called DevicePruner.step per iteration would save them): those keep bytes.  Writes the pruned stream, its Q file and
the pruned tables, and prints the per-row report.  The training that makes pruned channels dispensable stays with the caller."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.inq_model import tables_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("tables")
    ap.add_argument("stream")
    ap.add_argument("q_file")
    ap.add_argument("--out", required=True)
    ap.add_argument("--out-q", required=True)
    ap.add_argument("--out-tables", required=True)
    ap.add_argument("--keep", default=None)
    ap.add_argument("--c-rate", type=float, default=0.1)
    ap.add_argument("--alpha-low", type=float, default=0.95)
    ap.add_argument("--alpha-high", type=float, default=1.05)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    import torch
    from tf2_amd import dnscp, synth
    t = tables_of(a.tables)
    model = np.fromfile(a.stream, "<f4")
    q = np.loadtxt(a.q_file, dtype=np.int32)
    recs = None
    if a.keep:
        z = np.load(a.keep)
        keeps = {int(k[3:]): z[k] for k in z.files}
    else:
        dp = dnscp.DevicePruner(t)
        dense = torch.from_numpy(model).to(a.device)
        dp.stats(dense)
        dp.thresholds(a.c_rate, a.alpha_low, a.alpha_high)
        dp.step(dense, dense)
        keeps, recs = dp.keeps(), dp.state()
        bad = [(l, int(s)) for l, s in zip(dp.ids, recs["status"]) if s]
        if bad:
            raise SystemExit(f"status bits set (1 all zero, 2 non-finite, 4 NaN threshold): {bad}")
    t2, stream, q2 = dnscp.prune_model(t, model, q, keeps, device=a.device)
    print(dnscp.report(t, keeps, recs))
    stream.astype("<f4").tofile(a.out)
    with open(a.out_q, "wb") as f:
        f.write(synth.q_text(q2))
    with open(a.out_tables, "w") as f:
        json.dump(dict(t2), f)
    print(f"{a.out}: {stream.size} floats ({model.size} before); {a.out_q}: {q2.size} values; {a.out_tables}")


if __name__ == "__main__":
    main()
