"""Seeded synthetic inputs in the reference's own file formats.

The trained weight files (param.bin / fpgamodel.bin) are not part of the reference
repository (Runtime_Engine/cnn/host/model/README:1-7), so parity and benchmarks use
INQ-like synthetic weights written in the exact LoadModel stream order
(model_loader.cpp:139-213; writer caffe2fpga.cpp:91-113): per layer filters
[N][C][k][k] float32, then [bias], then [mean, variance, scale_factor(1), gamma, beta].

Weights follow the INQ statistics the reference documents (TransForm_Kit/Compression/
compress_net/core/compress_train_eval.py:54, 4bit_data_format.txt): every layer has 7
magnitudes 2^e_max ... 2^(e_max-6) plus zero, random sign, ~10 % zeros.  BN statistics
are chosen so that activations stay inside the int8 range without saturating
everywhere (variance = the conv output's expected variance).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np

from . import config as cfg


def synth_q_values(tables: cfg.NetTables, seed: int = 0, lo: int = 2, hi: int = 5, spread: int = 1) -> np.ndarray:
    """Q-file ints (file order, quantization.cpp:36-53) for networks without a shipped Q
    file: per tensor a base Q in [lo,hi] with per-channel jitter of `spread`; tensors that
    are added together (residual) share one Q vector, as in the shipped resnet50_Q."""
    rng = np.random.default_rng(seed)
    plan = cfg.build_plan(tables)
    rows: Dict[int, np.ndarray] = {}
    vals: List[int] = [2, 2, 2][:3]
    for L in plan:
        if L.ipool == 1:
            continue
        if L.ipool == 2:                     # L2Norm output: weight ~ 20 times a unit vector -> Q = 2 keeps it in int8
            rows[L.index] = np.full(L.N, 2) - rng.integers(0, 2, size=L.N)
            continue
        if L.add_src >= 0 and L.add_src in rows and rows[L.add_src].size == L.N:
            r = rows[L.add_src]
        else:
            base = int(rng.integers(lo, hi + 1))
            r = np.clip(base - rng.integers(0, spread + 1, size=L.N), 0, 7)
            if L.index == len(plan) - 1:
                r = np.full(L.N, base)
        rows[L.index] = r
    # a residual source must carry the same Q as the layer that adds onto it
    for L in plan:
        if L.add_src >= 0 and not plan[L.add_src].ipool:
            rows[L.add_src] = rows[L.index]
    for L in plan:
        if L.ipool != 1:
            vals.extend(int(v) for v in rows[L.index])
    return np.asarray(vals, np.int32)


def q_text(vals) -> bytes:
    return ("\n".join(str(int(v)) for v in vals) + "\n").encode()


def synth_model(tables: cfg.NetTables, q_vals, seed: int = 0, zero_frac: float = 0.1,
                dtype=np.float32) -> np.ndarray:
    """float32 model stream in LoadModel order."""
    rng = np.random.default_rng(seed + 1000)
    plan = cfg.build_plan(tables)
    out: List[np.ndarray] = []
    for L in plan:
        fan_in = L.model_C * L.model_k * L.model_k
        if not L.ipool:
            e_max = -int(rng.integers(1, 5))                     # 2^-1 .. 2^-4
            if not L.bn_en:
                # no BN to normalise: scale the weights so the real-unit output RMS is ~1
                rin0 = 25.0 if L.src == -1 else 1.0
                e_max = int(np.clip(np.round(-0.5 * np.log2(0.19 * fan_in * rin0 * rin0)), -8, -1))
            lev = rng.integers(0, 7, size=(L.N, fan_in))
            mag = np.ldexp(1.0, e_max - lev).astype(np.float32)
            sign = np.where(rng.random((L.N, fan_in)) < 0.5, -1.0, 1.0).astype(np.float32)
            w = mag * sign
            w[rng.random((L.N, fan_in)) < zero_frac] = 0.0
            out.append(w.ravel())
            row_energy = (w.astype(np.float64) ** 2).sum(axis=1)
        else:
            row_energy = np.ones(L.N)
            if L.ipool == 2:                 # L2Norm scale weights (SSD.py:24 initialises them to 20)
                out.append(rng.uniform(12.0, 24.0, size=L.N).astype(np.float32))
        if L.bias_en:
            out.append(rng.uniform(-0.5, 0.5, size=L.N).astype(np.float32))
        if L.bn_en:
            # real-unit input RMS: ~25 for the image layer (8-bit image data), ~1 elsewhere
            rin = 25.0 if L.src == -1 else 1.0
            var = np.maximum(row_energy * rin * rin, 1e-3) * rng.uniform(0.7, 1.4, size=L.N)
            mean = rng.normal(0, 0.05, size=L.N) * np.sqrt(var)
            gamma = rng.uniform(0.5, 1.5, size=L.N)
            beta = rng.uniform(-0.5, 0.5, size=L.N)
            out.append(mean.astype(np.float32)); out.append(var.astype(np.float32))
            out.append(np.asarray([1.0], np.float32))
            out.append(gamma.astype(np.float32)); out.append(beta.astype(np.float32))
    model = np.concatenate(out).astype(dtype)
    assert model.size == cfg.model_float_count(tables)
    return model


def synth_images(tables: cfg.NetTables, batch: int, seed: int = 0, kind: str = "float") -> np.ndarray:
    """Preprocessed CHW images like the shipped resnet50_data_label_100.bin (mean-subtracted
    0..255 data, range about -126..154).  kind="int8": already quantised, uniform over the
    whole int8 range (exercises the -128 negate quirk)."""
    rng = np.random.default_rng(seed + 2000)
    C, H, W = int(tables["INPUT_IMAGE_C"]), int(tables["INPUT_IMAGE_H"]), int(tables["INPUT_IMAGE_W"])
    if kind == "int8":
        return rng.integers(-128, 128, size=(batch, C, H, W)).astype(np.int8)
    x = rng.normal(0.0, 45.0, size=(batch, C, H, W))
    return np.clip(x, -126.0, 154.0).astype(np.float32)


def squeezenet_seeded_stream(seed=5):
    """Seeded float parameters of SqueezeNet 1.1 in table order (the float32 LoadModel stream of
    cfg.squeezenet11_tables, NOT power-of-two weights: this is the float model the calibrator sees).  numpy only:
    oracle/gen_golden.py loads the same numbers into the reference's PyTorch model, tests rebuild them from the seed.
    Returns (stream, per-row dict)."""
    t = cfg.squeezenet11_tables()
    rng = np.random.default_rng(seed)
    rows, parts = [], []
    for L in cfg.build_plan(t):
        fan = L.model_C * L.model_k * L.model_k
        r = dict(w=(rng.standard_normal((L.N, L.model_C, L.model_k, L.model_k)) * np.sqrt(2.0 / fan)).astype(np.float32))
        parts.append(r["w"].ravel())
        if L.bias_en:
            r["b"] = (rng.standard_normal(L.N) * 0.1).astype(np.float32); parts.append(r["b"])
        if L.bn_en:
            r["mean"] = (rng.standard_normal(L.N) * 0.2).astype(np.float32)
            r["var"] = rng.uniform(0.5, 2.0, L.N).astype(np.float32)
            r["gamma"] = rng.uniform(0.5, 1.5, L.N).astype(np.float32)
            r["beta"] = (rng.standard_normal(L.N) * 0.3).astype(np.float32)
            parts += [r["mean"], r["var"], np.ones(1, np.float32), r["gamma"], r["beta"]]
        rows.append(r)
    return np.concatenate(parts).astype(np.float32), rows



def squeezenet_calibration_images(seed: int = 17) -> np.ndarray:
    """Three seeded 1x3x227x227 float images (BASELINE configs[0] shape), [3, 1, 3, 227, 227]."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((3, 1, 3, 227, 227)) * 50.0).astype(np.float32)


def bench_network(name: str):
    """The BASELINE.json networks as bench.py, tools/steps_only.py, tools/pmc_summary.py and tools/dma_stress.py run them:
    (tables, Q values, model seed, display name, note).  resnet50: the shipped resnet50_Q + seeded INQ weights; the others: table
    programs of tf2_amd.config with synthetic per-channel Q values (spread 1) and seeded INQ weights."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if name == "resnet50":
        t = cfg.resnet50_tables()
        qv = np.loadtxt(os.path.join(root, "tests", "golden", "resnet50_Q"), dtype=np.int32)
        return t, qv, 0, "ResNet50", "54-layer TF2 table program, shipped resnet50_Q, seeded INQ weights"
    if name in ("googlenet", "resnet50_pruned"):
        # the reference's other two shipped networks (cnn.h:29-35: compile-time selection of googlenet.h / resnet50_pruned.h): the tables
        # dumped from the shipped headers and the shipped Q files (tests/golden/, oracle/gen_golden.py), seeded INQ weights
        import json
        g = os.path.join(root, "tests", "golden")
        t = cfg.NetTables(json.load(open(os.path.join(g, f"tables_{name}.json"))))
        t.setdefault("xConv1Rewrite", 1)          # (the headers describe conv1 in its executed 3x3 form over the space-to-depth image, model_loader.cpp:244-257)
        qv = np.loadtxt(os.path.join(g, f"{name}_Q"), dtype=np.int32)
        disp = {"googlenet": "GoogLeNet", "resnet50_pruned": "pruned ResNet50"}[name]
        return t, qv, 0, disp, f"the reference's shipped {name}.h table program and {name}_Q, seeded INQ weights"
    mk, disp, seed = {"squeezenet": (cfg.squeezenet11_tables, "SqueezeNet 1.1", 6), "vgg16": (cfg.vgg16_tables, "VGG16", 1),
                      "ssd300": (cfg.ssd300_tables, "SSD300-VGG", 3)}[name]
    t = mk()
    return t, synth_q_values(t, seed, spread=1), seed, disp, "TF2 table program built by tf2_amd.config, synthetic per-channel Q values and seeded INQ weights"


# ---- extreme-regime models: parameters chosen so that the edges of the integer arithmetic are reached ----------------------------------
EXTREME_REGIMES = ("wrap", "saturate", "spread", "shift22", "shift23", "expand32", "wrap2")


def _stream_offsets(plan):
    """Per table row: offsets {w, bias, mean, var, sf, gamma, beta} (None where absent) into the LoadModel stream."""
    pos, offs = 0, []
    for L in plan:
        o = dict(w=None, bias=None, mean=None, var=None, sf=None, gamma=None, beta=None)
        if not L.ipool:
            o["w"] = pos; pos += L.N * L.model_C * L.model_k * L.model_k
        elif L.ipool == 2:
            pos += L.N
        if L.bias_en:
            o["bias"] = pos; pos += L.N
        if L.bn_en:
            o["mean"] = pos; o["var"] = pos + L.N; o["sf"] = pos + 2 * L.N; o["gamma"] = pos + 2 * L.N + 1; o["beta"] = pos + 3 * L.N + 1
            pos += 4 * L.N + 1
        offs.append(o)
    return offs


def _q_layout(tables, plan):
    """File-order Q positions: {row index: slice of its N values} (the image row's values come first)."""
    pos, out = 3, {}
    for L in plan:
        if L.ipool == 1:
            continue
        out[L.index] = slice(pos, pos + L.N)
        pos += L.N
    return out, pos


def synth_extreme(tables: cfg.NetTables, seed: int, regime: str, rows=None, q_spread: int = 1):
    """(q_values, model_stream) in the same formats as synth_q_values / synth_model, with the rows `rows` (default: every conv row
    but the image row, which takes the treatment only when named) pushed to an arithmetic edge; everything else is synth_q_values(
    spread=q_spread) and synth_model.  Regimes (the numbers are in the oracle's terms: a filter code's shift is expand - level with
    expand = 15 - Q_in[c] + Q_out[n] in file Q values, level = -log2|w|, tf2_oracle.c tf2o_encode_filters):

    wrap      Q_out 10 above the row's input Q and dense filters of magnitude 1 .. 1/8: shifts of 22 .. 25, so that
              bias + (sum << lo) wraps in Z/2^32 on a large share of the outputs.  The epilogue form is decided per LAYER (the pack-time
              proof covers all its channels): a targeted layer with an even table index gets BN scales of 2^-9 .. 2^-7 on every channel
              (|alpha| < 2^19: the SEMI form), an odd one scales of 1 .. 4 (only the generic six-instruction form may take them).  A
              targeted row that reads a boosted tensor drops its Q 8 below it instead (scales 1 .. 4), so that chains alternate.
    saturate  BN scales 32 .. 128 times the one that keeps activations in range and shifts of up to +-128 output units: most outputs clip at
              127 / -128 (-128 where the row has no ReLU); every eighth row is all-zero with beta just below 2^31 - 2^14 or above
              -2^31 (the generic form's x + 2^14 saturates); rows without ReLU in front of a residual get betas far below -128 (the
              single-clamp form of a post-ReLU residual).
    spread    per-channel output Q from 0 to 13 on the rows' producers and filters over all 15 levels: 3 to 5 exponent windows per row.
              Row 0 of a layer has one non-zero tap, row 1 none; when a layer has more than 64 rows, rows 64 .. 127 use the low levels
              only (rows with fewer windows than their layer); the layer after a targeted one keeps levels 0 .. 7 (two windows: the
              dual form).
    shift22 / shift23   Q_out = min(Q_in) + 7 / + 8 with dense filters that include magnitude 1: the layer's largest shift is exactly
              22 / 23 (conv_shift.hip's mad_i32_i24 / 32-bit multiply boundary).
    expand32  the producer of a targeted row writes its channel 0 with Q -3 and the row's Q_out is 14: expand = 32 on that channel, so
              a magnitude-1 weight encodes as 0x20, which shifts by 0 (pe.cl's & 0x1f); the other channels' shifts reach 24 .. 27.
    wrap2     wrap's Q values and BN scales (even rows SEMI, odd rows generic, chains alternate), but every weight's level is drawn
              with probability 1/2 from 0 .. 3 and else from 13 .. 14: two exponent windows 11 .. 14 apart on every row, so that a boosted
              row packs in the two-window ("dual") form, and with nodual=1 in the Horner form.  Every fourth output channel is
              all-positive and every eighth (offset 2) all-negative: the inputs are post-ReLU, so those rows' high-window sums are
              large, and both the final accumulator and hi << dshift alone leave int32 on a large share of the outputs.
    """
    assert regime in EXTREME_REGIMES, regime
    rng = np.random.default_rng(7000 + seed)
    plan = cfg.build_plan(tables)
    q = synth_q_values(tables, seed, spread=q_spread).astype(np.int32)
    model = synth_model(tables, q, seed).astype(np.float32)
    qpos, _ = _q_layout(tables, plan)
    conv_rows = [L.index for L in plan if not L.ipool and L.src != -1]
    targets = set(conv_rows if rows is None else rows)
    # residual groups share one Q vector (synth_q_values): a targeted row's Q is written to the whole group
    group = {L.index: {L.index} for L in plan}
    for L in plan:
        if L.add_src >= 0 and not plan[L.add_src].ipool and L.index in qpos and L.add_src in qpos:
            g = group[L.index] | group[L.add_src]
            for m in g:
                group[m] = g

    done = set()

    def set_q(l, vals):
        if l in done:                                          # (a residual group takes the Q of its first targeted row)
            return
        for m in group[l]:
            q[qpos[m]] = vals
        done.update(group[l])

    def q_in(L):
        """The file Q values of the row's input channels (through pool rows, which keep their input's Q; concat tensors by member)."""
        src = L.src
        while src >= 0 and src not in qpos:
            src = plan[src].src
        if src == -1:
            return q[:3].astype(np.int64)
        if src >= 0:
            return q[qpos[src]].astype(np.int64)
        qi = np.zeros(L.C, np.int64)
        for M in plan:
            if M.concat == -(src + 2) and M.index in qpos:
                qi[M.n_start:M.n_start + M.N] = q[qpos[M.index]]
        return qi

    if regime == "spread":
        # the producers of the targeted rows get per-channel Q 0 .. 13 (first, in table order: the targeted rows read them)
        for l in sorted(targets):
            L = plan[l]
            if L.src >= 0 and L.src in qpos and len(group[L.src]) == 1 and not plan[L.src].ipool:
                set_q(L.src, rng.integers(0, 14, size=plan[L.src].N))
    offs = _stream_offsets(plan)
    for l in sorted(targets):
        L = plan[l]
        if L.ipool or l not in qpos:
            continue
        o = offs[l]
        fan = L.model_C * L.model_k * L.model_k
        qi = q_in(L)
        if regime == "wrap":
            # (a row that reads a boosted tensor drops 8 below it -- expand 7, outputs in range -- so that the row behind can be boosted again)
            boosted = qi.max() < 8
            set_q(l, np.full(L.N, min(int(qi.max()) + 10, 14) if boosted else max(int(qi.max()) - 8, 0)))
            lev = rng.integers(0, 4, size=(L.N, fan))
            zero = rng.random((L.N, fan)) < 0.05
        elif regime == "wrap2":
            boosted = qi.max() < 8
            set_q(l, np.full(L.N, min(int(qi.max()) + 10, 14) if boosted else max(int(qi.max()) - 8, 0)))
            lev = np.where(rng.random((L.N, fan)) < 0.5, rng.integers(0, 4, size=(L.N, fan)), rng.integers(13, 15, size=(L.N, fan)))
            zero = rng.random((L.N, fan)) < 0.05
        elif regime == "expand32":
            if L.src >= 0 and L.src in qpos and L.src not in targets:
                for m in group[L.src]:
                    q[qpos[m].start] = -3
                qi = q_in(L)
            set_q(l, np.full(L.N, 14))
            lev = rng.integers(0, 4, size=(L.N, fan))
            zero = rng.random((L.N, fan)) < 0.05
        elif regime in ("shift22", "shift23"):
            set_q(l, np.full(L.N, int(qi.min()) + (7 if regime == "shift22" else 8)))
            lev = rng.integers(0, 7, size=(L.N, fan))
            lev[:, 0] = 0
            zero = rng.random((L.N, fan)) < 0.1
            zero[:, 0] = False
        elif regime == "spread":
            lev = rng.integers(0, 15, size=(L.N, fan))
            if L.N > 64:
                lev[64:128] = rng.integers(10, 15, size=(min(L.N, 128) - 64, fan))
            zero = rng.random((L.N, fan)) < 0.1
            zero[0] = True; zero[0, fan // 2] = False        # one non-zero tap
            zero[1] = True                                     # all-zero row
            if l + 1 < len(plan) and not plan[l + 1].ipool and l + 1 not in targets and offs[l + 1]["w"] is not None:
                M = plan[l + 1]
                fan2 = M.model_C * M.model_k * M.model_k
                lev2 = rng.integers(0, 8, size=(M.N, fan2))
                sign2 = np.where(rng.random((M.N, fan2)) < 0.5, -1.0, 1.0)
                w2 = np.ldexp(sign2, -lev2) * 2.0 ** -3
                w2[rng.random((M.N, fan2)) < 0.1] = 0.0
                model[offs[l + 1]["w"]:offs[l + 1]["w"] + M.N * fan2] = w2.astype(np.float32).ravel()
        else:                                                  # saturate: the filters stay INQ-like
            lev = None
        if lev is not None:
            sign = np.where(rng.random((L.N, fan)) < 0.5, -1.0, 1.0)
            if regime == "wrap2":
                sign[0::4] = 1.0; sign[2::8] = -1.0                # same-sign rows
            w = np.ldexp(sign, -lev)
            w[zero] = 0.0
            model[o["w"]:o["w"] + L.N * fan] = w.astype(np.float32).ravel()
        qo = q[qpos[l]].astype(np.int64)
        if o["gamma"] is None:
            if regime == "saturate" and o["bias"] is not None:
                model[o["bias"]:o["bias"] + L.N] = (rng.choice([-1.0, 1.0], L.N) * rng.uniform(2.0, 6.0, L.N)).astype(np.float32)
            continue
        n = np.arange(L.N)
        mean = np.zeros(L.N); var = np.ones(L.N)
        if regime in ("wrap", "wrap2"):
            semi = boosted and l % 2 == 0
            gamma = np.ldexp(rng.uniform(1.0, 4.0, L.N), -9) if semi else rng.uniform(1.0, 4.0, L.N)
            beta = rng.uniform(-0.5, 0.5, L.N)
        elif regime == "saturate":
            var0 = model[o["var"]:o["var"] + L.N].astype(np.float64)
            mean = model[o["mean"]:o["mean"] + L.N].astype(np.float64)
            var = var0
            gamma = rng.uniform(32.0, 128.0, L.N)
            beta = rng.choice([-1.0, 1.0], L.N) * rng.uniform(0.0, 128.0, L.N) * 2.0 ** -qo
            if not L.relu and L.add_src >= 0:
                beta = -rng.uniform(300.0, 3000.0, L.N) * 2.0 ** -qo           # y far below -128 (in output units)
            # all-zero rows whose x = beta_fix sits where x + 2^14 saturates (and its mirror at the bottom)
            edge = n[::8]
            zrow = np.zeros((L.N, fan), bool); zrow[edge] = True
            cur = model[o["w"]:o["w"] + L.N * fan].reshape(L.N, fan)
            cur[zrow] = 0.0
            mean[edge] = 0.0; var[edge] = 1.0; gamma[edge] = 1.0
            top = np.where(np.arange(edge.size) % 2 == 0, 2.0 ** 31 - 2.0 ** 13, -(2.0 ** 31) + 2.0 ** 13)
            beta[edge] = top / 2.0 ** (15 + qo[edge])
            if o["bias"] is not None:
                model[o["bias"] + edge] = 0.0
        else:
            gamma = rng.uniform(0.5, 1.5, L.N) * 2.0 ** -8
            beta = rng.uniform(-0.5, 0.5, L.N)
        model[o["mean"]:o["mean"] + L.N] = mean.astype(np.float32)
        model[o["var"]:o["var"] + L.N] = var.astype(np.float32)
        model[o["gamma"]:o["gamma"] + L.N] = gamma.astype(np.float32)
        model[o["beta"]:o["beta"] + L.N] = beta.astype(np.float32)
    assert model.size == cfg.model_float_count(tables)
    return q, model


def synth_extreme_images(tables: cfg.NetTables, batch: int, seed: int = 0) -> np.ndarray:
    """int8 images, uniform over the whole range, with -128 and 127 patches (the negate quirk and the largest magnitudes)."""
    x = synth_images(tables, batch, seed, kind="int8")
    h = x.shape[2]
    x[:, :, : max(1, h // 8), :] = -128
    x[:, :, h // 2: h // 2 + max(1, h // 8), :] = 127
    return x


# ---- post-op regimes: the maps that max pools and global averages read, set so that their edges are reached --------------------------
POSTOP_REGIMES = ("signed_pool", "avg_extreme")


def avg_of_sum(s: int, mult: int) -> int:
    """The global average of an int16 sum before the clip (full_size_pool.cl:118)."""
    return (((s * mult) >> 14) + 1) >> 1


def _wrap16(s: int) -> int:
    return (s + 32768) % 65536 - 32768


def avg_level_targets(H: int, W: int, mult: int) -> Dict[str, List[tuple]]:
    """Every pair (A, B) of int8 levels with A - B an int8 as well, by what the global average of an H x W map that holds A on the
    (H - 1) x (W - 1) pixels with row and column > 0 and B on the rest makes of it (full_size_pool.cl:101-118: int16 sum, then
    ((s * mult) >> 14) + 1 >> 1, then the clip).  Categories: half+ / half- (s * mult an odd multiple of 2^14: the rounding half, by
    the sign of s), clip+ / clip-, wrap+ / wrap- (the int16 sum wraps; by the sign of the true sum), neg (a negative average that is none
    of those)."""
    nA, nB = (H - 1) * (W - 1), H + W - 1
    out: Dict[str, List[tuple]] = {k: [] for k in ("half+", "half-", "clip+", "clip-", "wrap+", "wrap-", "neg")}
    for A in range(-128, 128):
        for B in range(max(-128, A - 127), min(127, A + 128) + 1):
            st = A * nA + B * nB
            s = _wrap16(st)
            m = avg_of_sum(s, mult)
            half = (s * mult) % 32768 == 16384
            if half:
                out["half+" if s > 0 else "half-"].append((A, B))
            if m > 127:
                out["clip+"].append((A, B))
            if m < -128:
                out["clip-"].append((A, B))
            if st != s:
                out["wrap+" if st > 0 else "wrap-"].append((A, B))
            if -128 <= m < 0 and not half and st == s and (s * mult) % 16384:
                out["neg"].append((A, B))
    return out


def _bn_const(model, o, n, v, qo, fan):
    """Channel n of a row: an output of exactly v everywhere.  With BN: mean 0, variance 1, gamma 2^-24 (alpha_fix = 0: the filters,
    left as they are, drop out) and beta v * 2^-Q (beta_fix = v << 15); without BN: all-zero filters and bias v * 2^-Q."""
    if o["gamma"] is not None:
        model[o["mean"] + n] = 0.0; model[o["var"] + n] = 1.0; model[o["gamma"] + n] = 2.0 ** -24
        model[o["beta"] + n] = np.float32(v * 2.0 ** -qo)
    else:
        model[o["w"] + n * fan:o["w"] + (n + 1) * fan] = 0.0
        model[o["bias"] + n] = np.float32(v * 2.0 ** -qo)


def synth_postop(tables: cfg.NetTables, seed: int, regime: str, rows=None):
    """(q_values, model_stream) in the formats of synth_q_values / synth_model: synth_q_values(spread=1) and synth_model, with the rows
    `rows` set so that the post-op behind them reaches its edges.

    signed_pool  rows: the pooled conv rows and the producers of pooling rows (default: all).  Channel n % 8 of a row: 0 all -128, 1 all
                 127, 2 one negative value everywhere (zero filters, the value from beta), 3 negative almost everywhere with the filters'
                 texture (gamma / 4, beta -80 output units), 4 saturated at both ends (gamma x 64); the rest as drawn.  (Constant channels keep
                 their filters where the row has BN: alpha_fix = 0 -- conv_stem's packed form needs the rewrite's unit taps in every row.)  Behind a row
                 without ReLU: every window whose inside is negative -- the whole map of channels 0, 2 -- is decided by the zero taps of
                 the padding / the ceil-mode edge, or by the zero slot of a window narrower than 3 (pool.cl:115-140, 177-186).
    avg_extreme  rows: averaged rows (default: all).  Where the averaged row R is a 1x1 row over a 3x3 / pad 1 row P over a conv row K
                 (same channels, all with BN, no residual: cfg.avg_tables), channel n of R is made a two-level map: K's channel n the
                 constant A - B, P's one tap (0, 0) of weight 1 on it plus B (so A where the tap is inside the map, B on the first row
                 and column), R the identity (P and R take K's Q); behind a P with ReLU the levels A - C, B - C with R's beta C =
                 min(A, B, 0).  The levels are drawn per channel from avg_level_targets: int16
                 wraps, rounding halves of both signs, clips at both ends and negative averages, whichever the map size admits; every
                 fourth channel keeps its texture.  Elsewhere (a residual row, ResNet-50's row 52) the averaged row's channels n % 4 = 0,
                 1, 2 get the constant outputs -128, 127 and a negative value (the residual adds on top).
    """
    assert regime in POSTOP_REGIMES, regime
    rng = np.random.default_rng(9000 + seed)
    plan = cfg.build_plan(tables)
    q = synth_q_values(tables, seed, spread=1).astype(np.int32)
    model = synth_model(tables, q, seed).astype(np.float32)
    qpos, _ = _q_layout(tables, plan)
    offs = _stream_offsets(plan)

    def fan(L):
        return L.model_C * L.model_k * L.model_k

    def zero_filters(l, n):
        L = plan[l]
        model[offs[l]["w"] + n * fan(L):offs[l]["w"] + (n + 1) * fan(L)] = 0.0

    if regime == "signed_pool":
        if rows is None:
            rows = [L.index for L in plan if L.pool_en and not L.ipool] + [L.src for L in plan if L.ipool == 1 and L.src >= 0 and not plan[L.src].ipool]
        for l in sorted(set(rows)):
            L, o = plan[l], offs[l]
            qo = q[qpos[l]].astype(np.int64)
            for n in range(L.N):
                cls = n % 8
                if cls in (0, 1, 2):
                    _bn_const(model, o, n, (-128, 127, int(rng.integers(-127, 0)))[cls], qo[n], fan(L))
                elif cls == 3:
                    if o["gamma"] is not None:
                        g = model[o["gamma"] + n] * 0.25
                        b = np.sqrt(model[o["var"] + n] + 1e-5)
                        model[o["gamma"] + n] = g
                        model[o["beta"] + n] = np.float32(-80.0 * 2.0 ** -qo[n] + g / b * model[o["mean"] + n])
                    else:
                        model[o["bias"] + n] = np.float32(-80.0 * 2.0 ** -qo[n])
                elif cls == 4 and o["gamma"] is not None:
                    model[o["gamma"] + n] *= 64.0
        assert model.size == cfg.model_float_count(tables)
        return q, model

    if rows is None:
        rows = [L.index for L in plan if L.endpool]
    for l in sorted(set(rows)):
        R = plan[l]
        P = plan[R.src] if R.src >= 0 else None
        K = plan[P.src] if P is not None and P.src >= 0 else None
        chain = (K is not None and not K.ipool and not P.ipool and R.k == 1 and R.stride == 1 and P.k == 3 and P.stride == 1 and
                 P.pad_h == 1 and P.pad_w == 1 and P.dil == 1 and R.N == P.N == K.N == R.C == P.C and R.add_src < 0 and P.add_src < 0 and
                 not (P.pool_en or P.endpool or K.pool_en or K.endpool or R.pool_en) and K.concat < 0 and P.concat < 0 and
                 all(offs[m.index]["gamma"] is not None for m in (R, P, K)) and
                 not any(M.add_src in (R.index, P.index, K.index) for M in plan))
        if not chain:
            qo = q[qpos[l]].astype(np.int64)
            for n in range(R.N):
                if n % 4 < 3:
                    _bn_const(model, offs[l], n, (-128, 127, int(rng.integers(-127, 0)))[n % 4], qo[n], fan(R))
            continue
        qk = q[qpos[K.index]].copy()
        q[qpos[P.index]] = qk
        q[qpos[R.index]] = qk
        H, W = R.H, R.W
        lv = avg_level_targets(H, W, R.endpool_mult)
        if P.relu:          # (P's levels non-negative: R's beta C = min(A, B, 0) moves them back)
            lv = {k: [(A, B) for A, B in v if max(A, B, 0) - min(A, B, 0) <= 127] for k, v in lv.items()}
        cats = [(k, v) for k, v in lv.items() if v]
        ok, op, orr = offs[K.index], offs[P.index], offs[R.index]
        for n in range(R.N):
            if n % 4 == 3:
                continue
            _, cand = cats[(n - n // 4) % len(cats)]
            A, B = cand[int(rng.integers(0, len(cand)))]
            C = min(A, B, 0) if P.relu else 0
            _bn_const(model, ok, n, A - B, qk[n], fan(K))
            for M, o, beta in ((P, op, B - C), (R, orr, C)):
                zero_filters(M.index, n)
                tap = 0 if M is P else (M.model_k * M.model_k) // 2
                model[o["w"] + n * fan(M) + n * M.model_k * M.model_k + tap] = 1.0
                model[o["mean"] + n] = 0.0; model[o["var"] + n] = 1.0; model[o["gamma"] + n] = 1.0
                model[o["beta"] + n] = np.float32(beta * 2.0 ** -qk[n])
                if o["bias"] is not None:
                    model[o["bias"] + n] = 0.0
    assert model.size == cfg.model_float_count(tables)
    return q, model
