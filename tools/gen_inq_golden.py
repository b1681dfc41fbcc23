#!/usr/bin/env python3
"""Records tests/golden/ref_inq.npz: inputs and outputs of the reference's own INQ functions, ComputeQuantumRange and ShapeIntoTwoPower
(TransForm_Kit/Compression/compress_net/core/compress_core.py), called as compress_train_eval.py:54-56 calls them.  Run once, by hand,
where the reference lies:  python tools/gen_inq_golden.py /path/to/reference [out.npz].  No test and no GPU code runs this; the tests
read the .npz and set tf2_amd.inq.reference_range / reference_step against it as bits.

Cases (key prefix cNN_): a case is one tensor walked through a schedule of portions; step k stores w_in, mask_in (what the reference
received), prev, cur, n_values and max_exp, min_exp, w_out, mask_out (what it returned).  Between steps the still-float weights are
shrunk by seeded factors in [0.7, 1) -- the retraining of the real flow, kept under the quantised maximum so that the reference does not
exit.  Kept out on purpose: zeros among the selected weights (the reference takes log(0) and raises) and magnitudes of 1.5 * 2^E exactly
with E <= -30 (tf2_amd.inq.exp_of_bits states the deviation there)."""
import contextlib
import io
import os
import sys

import numpy as np

SCHEDULES = ((0.5, 0.75, 0.875, 1.0), (0.3, 0.6, 0.8, 0.9, 1.0))


def load_reference(root):
    core = os.path.join(root, "TransForm_Kit", "Compression", "compress_net", "core")
    sys.path.insert(0, core)
    import compress_core
    return compress_core.ComputeQuantumRange, compress_core.ShapeIntoTwoPower


def walk(rng, rng_fn, shape_fn, w, schedule, n_values, out, tag):
    mask = np.ones(w.shape)                                  # float64 ones, as compress() makes them
    prev = 0.0
    steps = 0
    for k, cur in enumerate(schedule):
        if not (mask == 1).any():                            # (the reference's range function fails on most fully quantised tensors)
            break
        steps += 1
        w_in, m_in = w.copy(), mask.copy()
        with contextlib.redirect_stdout(io.StringIO()):      # (the reference prints its counts)
            mx, mn = rng_fn(w.copy(), mask.copy(), n_values)
            w_out, m_out = shape_fn(w.copy(), mask.copy(), prev, cur, mx, mn)
        p = f"{tag}_s{k}_"
        out[p + "w_in"], out[p + "mask_in"] = w_in.astype(np.float32), m_in.astype(np.uint8)
        out[p + "w_out"], out[p + "mask_out"] = np.asarray(w_out, np.float32), np.asarray(m_out).astype(np.uint8)
        out[p + "par"] = np.asarray([prev, cur], np.float64)
        out[p + "exp"] = np.asarray([int(mx), int(mn), int(n_values)], np.int64)
        w, mask = np.asarray(w_out, np.float32).copy(), np.asarray(m_out, np.float64).copy()
        still = mask == 1
        w[still] = (w[still] * rng.uniform(0.7, 1.0, int(still.sum()))).astype(np.float32)
        prev = cur
    out[tag + "_steps"] = np.asarray(steps, np.int64)


def main():
    root = sys.argv[1]
    dst = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "ref_inq.npz")
    rng_fn, shape_fn = load_reference(root)
    rng = np.random.default_rng(20190)
    out, n = {}, 0

    def case(w, schedule, n_values=7):
        nonlocal n
        walk(rng, rng_fn, shape_fn, np.asarray(w, np.float32), schedule, n_values, out, f"c{n:02d}")
        n += 1

    # random tensors of 1 .. 400 elements under both schedules (no exact zeros)
    for i, size in enumerate((1, 2, 7, 64, 129, 255, 400, 333)):
        w = (rng.standard_normal(size) * rng.choice([0.02, 0.1, 0.5, 2.0])).astype(np.float32)
        w[w == 0] = np.float32(0.01)
        case(w.reshape(-1, 1, 1, 1) if i % 2 else w, SCHEDULES[i % 2])
    # tie-heavy: five magnitudes, both signs
    mags = np.asarray([0.3, 0.11, 0.07, 0.02, 0.004], np.float32)
    w = mags[rng.integers(0, 5, 300)] * np.where(rng.random(300) < 0.5, -1, 1).astype(np.float32)
    case(w, SCHEDULES[0])
    case(w[:97], SCHEDULES[1])
    # half to even: n1 = 5, prev = 0.5, cur = 0.75 -> n_init = 10, n_keep = rint(2.5) = 2
    w5 = np.asarray([0.9, -0.4, 0.2, -0.1, 0.05, 0.6, -0.7, 0.8, 0.33, -0.45], np.float32)
    case(w5, (0.5, 0.75, 1.0))
    # 1.5 * 2^E and its two neighbours, E = -20 .. 0, one step at portion 1 with every exponent inside the window (n_values 24)
    trip = []
    for E in range(-20, 1):
        b = np.float32(1.5 * 2.0 ** E).view(np.uint32)
        trip += [np.uint32(b - 1).view(np.float32), np.uint32(b).view(np.float32), np.uint32(b + 1).view(np.float32)]
    t = np.asarray(trip, np.float32)
    case(t * np.where(np.arange(t.size) % 2, -1, 1).astype(np.float32), (1.0,), n_values=24)
    # the same with the reference's seven magnitudes: most of them flush to +0.0
    case(t, (1.0,))
    out["n_cases"] = np.asarray(n, np.int64)
    np.savez_compressed(dst, **out)
    print(f"{dst}: {n} cases, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
