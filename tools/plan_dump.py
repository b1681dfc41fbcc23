#!/usr/bin/env python3
"""The launch plans of many programs as text (no device): one line per launch -- `layer kernel grid block lds_bytes`, as
`tf2_net_describe_launches` reports them -- and the sha256 of the whole text at the end.  Two builds of the library whose outputs are
byte-identical select the same kernels with the same tile shapes, grids and LDS sizes everywhere the sweep reaches: the check of a
change to the launch planner (csrc/net_plan.hip) that is meant to change no plan.

Covered: the six `bench.py --net` networks at batches 1, 2, 3, 8, 12, 32, 33, 64, both plans (one batch at a time / batches in
flight), ResNet-50 again with pack mode 1 (conv_shift), each under the default options and under every option string of OPTS; and the
seeded generators of tests/test_fuzz_programs.py, seeds 0-7, at batches 1, 3 and 8.  A plan that fails records its error text.

  python tools/plan_dump.py [--jobs 8] [--out plan_dump.txt]           (TF2_AMD_LIB=<other build> to dump that build's plans)"""
import argparse
import hashlib
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NETS = ("resnet50", "squeezenet", "vgg16", "ssd300", "googlenet", "resnet50_pruned")
BATCHES = (1, 2, 3, 8, 12, 32, 33, 64)
FUZZ = ("random_program", "random_body_program", "random_fire_program", "random_inception_program")
FUZZ_SEEDS, FUZZ_BATCHES = range(8), (1, 3, 8)
OPTS = ("", "bfirst=1", "bfirst=0", "bfirst=0,bgroup=0", "bband=2", "bband=0", "bgroup_chain=1", "pwk=0", "pwk=2", "pwk_slabs=8,pwk_units=0",
        "pair=0", "fire=1", "fire=0,first_pool=0", "fire_pool=2", "fire_pool=4", "c3=0", "c3_pool=0", "fc=0", "stem=0", "stem_pool=0",
        "avg_fuse=0", "avg_fuse=1", "dense=0", "first=0", "sk=1", "sk=2", "pw=0", "sk_kb=0", "q128=0")

_programs = {}          # name -> (tables, Q text, model), built before the workers fork


def dump(unit):
    """One (program, pack mode, option string, batches) -> its lines."""
    name, pack_mode, opts, batches = unit
    from tf2_amd import _lib, network
    os.environ["TF2_AMD_OPTS"] = ""
    _lib.set_opts(**dict(kv.split("=") for kv in opts.split(",") if kv))
    t, q_text, model = _programs[name]
    net = network.NetWork(t)                    # (a handle takes its options when it is created)
    net.Quantization(q_text); net.LoadModel(model); net.Pack(pack_mode)
    lines = []
    for batch in batches:
        for conc in (0, 1):
            lines.append(f"# {name} pack {pack_mode} [{opts}] batch {batch} plan {conc}")
            try:
                lines += [f"{r['layer']} {r['kernel']} {r['grid']} {r['block']} {r['lds_bytes']}" for r in net.describe_launches(batch, conc)]
            except _lib.Tf2Error as e:
                lines.append(f"error: {e}")
    net.CleanUp()
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--nets", default=",".join(NETS))
    ap.add_argument("--out", default="", help="also write the text to this file")
    args = ap.parse_args()
    from tf2_amd import synth
    import test_fuzz_programs as fuzz
    units = []
    for name in [n for n in args.nets.split(",") if n]:
        t, q, seed = synth.bench_network(name)[:3]
        _programs[name] = (t, synth.q_text(q), synth.synth_model(t, q, seed))
        units += [(name, 0, o, BATCHES) for o in OPTS]
        if name == "resnet50":
            units += [(name, 1, o, BATCHES) for o in OPTS]
    for gen in FUZZ:
        for seed in FUZZ_SEEDS:
            t = getattr(fuzz, gen)(seed)
            q, model = fuzz._q_and_model(t, seed)
            _programs[f"{gen}({seed})"] = (t, synth.q_text(q), model)
            units.append((f"{gen}({seed})", 0, "", FUZZ_BATCHES))
    with multiprocessing.get_context("fork").Pool(max(1, args.jobs)) as pool:
        text = "".join(pool.map(dump, units, chunksize=1))       # (in the order of `units`, whatever the number of workers)
    text += f"# sha256 {hashlib.sha256(text.encode()).hexdigest()}\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
