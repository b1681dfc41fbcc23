#!/usr/bin/env python3
"""The launch plans of many programs as text (no device): one line per launch -- `layer kernel grid block lds_bytes`, as
`tf2_net_describe_launches` reports them -- and the sha256 of the whole text at the end.  Two builds of the library whose outputs are
byte-identical select the same kernels with the same tile shapes, grids and LDS sizes everywhere the sweep reaches: the check of a
change to the launch planner (csrc/net_plan.hip) or to the options (csrc/opt_table.h) that is meant to change no plan.

Covered: the six `bench.py --net` networks at batches 1, 2, 3, 8, 12, 32, 33, 64, both plans (one batch at a time / batches in
flight), ResNet-50 again with pack mode 1 (conv_shift), each under the default options and under every option string of OPTS; and the
seeded generators of tests/test_fuzz_programs.py, seeds 0-7, at batches 1, 3 and 8.  A plan that fails records its error text.

OPTS sets every plan-time option of csrc/opt_table.h to a value that is not its default at least once (checked against the table
before anything runs).  They need no new pack: a worker packs a program once and sweeps its share of OPTS with reload_options().
The text ends with the strings whose dumps equal the default string's on every program, or those of the string without its last
option where OPTS has that one too (an option that only rides along) -- such a string tests nothing; what may remain there are
options that cannot show in a launch record (NO_RECORD below).

  python tools/plan_dump.py [--jobs 8] [--out plan_dump.txt]           (TF2_AMD_LIB=<other build> to dump that build's plans)"""
import argparse
import hashlib
import multiprocessing
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NETS = ("resnet50", "squeezenet", "vgg16", "ssd300", "googlenet", "resnet50_pruned")
BATCHES = (1, 2, 3, 8, 12, 32, 33, 64)
FUZZ = ("random_program", "random_body_program", "random_fire_program", "random_inception_program")
FUZZ_SEEDS, FUZZ_BATCHES = range(8), (1, 3, 8)
R50_3x3_7 = hex(1 << 45 | 1 << 48 | 1 << 51)      # ResNet-50's 7 x 7 x 512 3x3 rows (conv_img.hip)
ALL_ROWS = hex((1 << 64) - 1)
OPTS = ("", "bfirst=1", "bfirst=0", "bgroup=0", "bfirst=0,bgroup=0", "bband=2", "bband=0", "bgroup_chain=1", "pwk=0", "pwk=2", "pwk_slabs=8", "pwk_units=0",
        "pwk_slabs=8,pwk_units=0", "pair=0", "fire=1", "fire=0", "fire=0,first_pool=0", "fire_pool=2", "fire_pool=4", "c3=0", "c3_pool=0", "stem=0",
        "stem_pool=0", "avg_fuse=0", "avg_fuse=1", "dense=0", "first=0", "sk=1", "sk=2", "pw=0", "sk_kb=0", "q128=0",
        # thresholds, low or high enough to move rows
        "img=0", "img=2", "img_min=1", "img_rows=" + R50_3x3_7, "noimg_rows=" + R50_3x3_7,
        "pw_slabs=4", "pw_minpix=0", "sk8=0", "sk8=100000", "sk_s3=0", "sk_s3_conc=100000",
        "sk_kb_blocks=64", "sk_kb_min=2", "sk_kb_max=2,sk_kb_min=2", "stem_pk_small=0",
        "pwk_minpix=1000000", "pwk_units=0,pwk_minpix=0,pwk_slabs=8", "pwk_sk=1,pwk_units=0,pwk_minpix=0,pwk_slabs=8",
        "pwk_rows=" + hex(1 << 27), "nopwk_rows=" + hex(1 << 5 | 1 << 8 | 1 << 11),
        "pwk=2,pwk_units=0", "pwk=2,pwk_units=0,pwk_slots=64", "pwk_slots=512", "pwk_pipe=0",
        "fc_min=1", "c3_min=100000", "c3_min=0", "c3_min=0,c3_min_hw=7", "c3_min256=0", "c3_min256=100000", "c3_w9=0", "c3_w9=2",
        "bneck_min=1", "bneck_min=100000", "bgroup_min7=1", "bgroup_min14=1", "bgroup_min28=1", "bfirst=1,bgroup_min56f=1",
        "bgroup_polls=1000", "bgroup_withhold=1", "bfirst_min=1", "bfirst_min=40", "bband_rows=4", "bband_alone_maps=4",
        "bband_alone_maps=4,bband_rows_alone=7", "bband_alone_maps=2,bband_rows_alone=7", "bband_rows_dd=4", "bband_min=1", "bband_min=40", "dense_max=1",
        "alt_min=0", "alt_min=100000", "alt_min_conc=0", "alt_min_conc=100000", "alt_narrow=0", "alt_narrow=100000",
        "alt_rows=" + ALL_ROWS, "noalt_rows=" + ALL_ROWS, "sk_rows=" + ALL_ROWS, "nosk_rows=" + ALL_ROWS)
# strings with a pack-time option: a pack each (without fc4=0 the whole-window layers are 4-bit codes, which only conv_fc can run)
PACK_OPTS = ("fc4=0", "fc4=0,fc=0", "fc4=0,fc_min=100000")
SHARES = 4              # workers per (program, pack mode): each packs once and sweeps OPTS[i::SHARES]
# plan-time options that cannot show in a launch record
NO_RECORD = {"pwk_pipe": "a kernel argument, not part of the grid", "bgroup_polls": "a control word of the step's first kernel",
             "bgroup_withhold": "a control word of the step's first kernel", "q128": "a flag inside the argument blocks of prep and stem"}

_programs = {}          # name -> (tables, Q text, model), built before the workers fork


def plan_time_options():
    """{name: default} of the plan-scope lines of csrc/opt_table.h."""
    text = open(os.path.join(ROOT, "tf2_amd", "csrc", "opt_table.h")).read()
    rows = re.findall(r"^TF2_OPT\((\w+), plan, [01], [\w ]+, \w+, ([^)]+)\)", text, re.M)
    return {name: eval(dflt) for name, dflt in rows}


def dump(unit):
    """One (program, pack mode, option strings, pack under each string?, batches) -> [(program, pack mode, option string, its lines)]."""
    name, pack_mode, opt_strings, repack, batches = unit
    from tf2_amd import _lib, network
    t, q_text, model = _programs[name]
    out, net = [], None
    for opts in opt_strings:
        os.environ["TF2_AMD_OPTS"] = ""
        _lib.set_opts(**dict(kv.split("=") for kv in opts.split(",") if kv))
        if net is None or repack:
            net = network.NetWork(t)                # (a handle takes its options when it is created)
            net.Quantization(q_text); net.LoadModel(model); net.Pack(pack_mode)
        else:
            net.reload_options()
        lines = []
        for batch in batches:
            for conc in (0, 1):
                lines.append(f"# {name} pack {pack_mode} [{opts}] batch {batch} plan {conc}")
                try:
                    lines += [f"{r['layer']} {r['kernel']} {r['grid']} {r['block']} {r['lds_bytes']}" for r in net.describe_launches(batch, conc)]
                except _lib.Tf2Error as e:
                    lines.append(f"error: {e}")
        out.append((name, pack_mode, opts, lines))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--nets", default=",".join(NETS))
    ap.add_argument("--out", default="", help="also write the text to this file")
    args = ap.parse_args()
    set_to = {}
    for kv in ",".join(OPTS + PACK_OPTS).split(","):
        if kv:
            set_to.setdefault(kv.split("=")[0], set()).add(int(kv.split("=")[1], 0))
    unswept = [k for k, dflt in plan_time_options().items() if not set_to.get(k, set()) - {dflt}]
    if unswept:
        sys.exit(f"plan_dump.py: OPTS sets no value other than the default for {unswept} (csrc/opt_table.h)")
    from tf2_amd import synth
    import test_fuzz_programs as fuzz
    units = []
    for name in [n for n in args.nets.split(",") if n]:
        t, q, seed = synth.bench_network(name)[:3]
        _programs[name] = (t, synth.q_text(q), synth.synth_model(t, q, seed))
        for pack_mode in (0, 1) if name == "resnet50" else (0,):
            units += [(name, pack_mode, OPTS[i::SHARES], False, BATCHES) for i in range(SHARES)]
            units += [(name, pack_mode, (o,), True, BATCHES) for o in PACK_OPTS]
    for gen in FUZZ:
        for seed in FUZZ_SEEDS:
            t = getattr(fuzz, gen)(seed)
            q, model = fuzz._q_and_model(t, seed)
            _programs[f"{gen}({seed})"] = (t, synth.q_text(q), model)
            units.append((f"{gen}({seed})", 0, ("",), False, FUZZ_BATCHES))
    with multiprocessing.get_context("fork").Pool(max(1, args.jobs)) as pool:
        done = [r for rs in pool.map(dump, units, chunksize=1) for r in rs]       # (in the order of `units`, whatever the number of workers)
    text = "".join(line + "\n" for _, _, _, lines in done for line in lines)
    # (a plan's first line names its option string: compared without it)
    plans = {(name, pm, o): [x for x in lines if not x.startswith("# ")] for name, pm, o, lines in done}
    for o in OPTS[1:] + PACK_OPTS:
        shorter = o.rpartition(",")[0]
        for than in {"", shorter if shorter in OPTS + PACK_OPTS else ""}:
            if all(p == plans[name, pm, than] for (name, pm, oo), p in plans.items() if oo == o):
                why = [NO_RECORD[k] for k in (kv.split("=")[0] for kv in o.split(",")) if k in NO_RECORD]
                text += f"# [{o}] gives the plans of [{than}] on every program" + (f" ({why[0]})" if why else "") + "\n"
    text += f"# sha256 {hashlib.sha256(text.encode()).hexdigest()}\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
