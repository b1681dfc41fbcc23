#!/usr/bin/env python3
"""Float model in, engine-ready model out: INQ weight quantisation of a LoadModel stream on the device (tf2_amd.inq.quantize_model).
  python tools/inq_model.py TABLES FLOAT_STREAM --out model_q.bin [--out4 model_q.4bit] [--schedule 0.5,0.75,0.875,1] [--exp-floor -14]
TABLES: resnet50 | vgg16 | ssd300 | squeezenet | tiny, or a tables .json (tests/golden/tables_*.json); FLOAT_STREAM: raw little-endian
float32 in LoadModel order.  Writes the quantised stream, the 4-bit file (model4bit.write_model_4bit; every filter must come out as
4-bit codes, dtype 0) and prints the per-tensor report with what the engine's loader would misread (engine_check) before and after.
Without retraining between the steps a schedule ends where one step at 1 does; the schedule is there for callers who train in between
(quantize_model's `between`)."""
import argparse
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tables_of(name):
    from tf2_amd import config as cfg
    builtin = {"resnet50": cfg.resnet50_tables, "vgg16": cfg.vgg16_tables, "ssd300": cfg.ssd300_tables, "squeezenet": cfg.squeezenet11_tables,
               "tiny": cfg.tiny_tables}
    if name in builtin:
        return builtin[name]()
    return cfg.NetTables(json.load(open(name)))


def filter_dtypes(tables, data, stream):
    """[(name, dtype byte)] of the filters of a 4-bit file"""
    from tf2_amd import model4bit
    out, pos = [], 0
    for name, arr, is_filter in model4bit.split_model(tables, stream):
        _, dtype, _, _, _, _ = struct.unpack_from("<bbhhhh", data, pos)
        pos += len(model4bit.encode_tensor(arr, is_filter))
        if is_filter:
            out.append((name, dtype))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("tables")
    ap.add_argument("stream")
    ap.add_argument("--out", required=True)
    ap.add_argument("--out4", default=None)
    ap.add_argument("--schedule", default="1")
    ap.add_argument("--exp-floor", type=int, default=-14, help="-14: the engine's smallest weight; -127: the reference's behaviour")
    ap.add_argument("--filters-only", action="store_true", help="leave the biases float (the reference quantises them too)")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    from tf2_amd import inq, model4bit
    t = tables_of(a.tables)
    model = np.fromfile(a.stream, "<f4")
    before = inq.engine_check(t, model)
    out, rep = inq.quantize_model(t, model, schedule=[float(v) for v in a.schedule.split(",")], exp_floor=a.exp_floor,
                                  which=("filter",) if a.filters_only else ("filter", "bias"), device=a.device)
    check = inq.engine_check(t, out)
    print(inq.report(rep, check))
    print(f"engine misfits: {sum(r['misfit'] for r in before)} before, {sum(r['misfit'] for r in check)} after, of "
          f"{sum(r['count'] for r in check)} filter weights")
    out.astype("<f4").tofile(a.out)
    if a.out4:
        data = model4bit.write_model_4bit(t, out)
        floats = [n for n, d in filter_dtypes(t, data, out) if d != 0]
        if floats:
            raise SystemExit(f"filters that did not come out as 4-bit codes: {floats}")
        with open(a.out4, "wb") as f:
            f.write(data)
        print(f"{a.out4}: {len(data)} bytes ({4 * out.size} as float32)")


if __name__ == "__main__":
    main()
