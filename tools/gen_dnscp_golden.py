#!/usr/bin/env python3
"""Records tests/golden/ref_dnscp.npz: inputs and outputs of the reference's own DNS-CP functions, DnscpCore.cal_mean_std and
maskChannelCalc (TransForm_Kit/DnsChannelpruning/dnscp_core.py) and model_convert.clip_cin_channel / clip_cout_channel, called as
forward_dnscp_layer and modelblob_convert call them.  Run once, by hand, on the CPU, where the reference lies:
  python tools/gen_dnscp_golden.py /path/to/reference [out.npz]
No test and no GPU code runs this; the tests read the .npz and set tf2_amd.dnscp against it.

A case (key prefix cNN_) is one conv [N, C, k, k] walked through two iterations: cal_mean_std at iteration 0 (mu, std recorded), then
maskChannelCalc on w0 and on w1 with the mask carried over; s0_keep / s1_keep are the reference's masks per input channel.  Then the
export of the final mask: clip_cin_channel on w1, clip_cout_channel on a conv in front (pw [C, 5, k, k]) and on a vector (pv [C]).
Channel c of a conv is a seeded texture times a scale, low or high, so that both hysteresis branches, both fix-up directions, the tie at
nz / 16 = 2.5, the floor at 16 (with C too small for it as well) and a negative variance occur; the tool asserts that they do.
margin: the smallest relative distance of a channel's mean magnitude from either threshold, all in float64 -- at least 2^-10 in every
case (asserted here and by the test), so that the order of the reference's float32 sums decides no mask."""
import os
import sys

import numpy as np

MARGIN = 2.0 ** -10
C_RATE, A_LO, A_HI = 0.1, 0.95, 1.05


def load_reference(root):
    sys.path.insert(0, os.path.join(root, "TransForm_Kit", "DnsChannelpruning"))
    import dnscp_core
    import model_convert
    return dnscp_core.DnscpCore, model_convert.clip_cin_channel, model_convert.clip_cout_channel


def thresholds64(w, keep):
    """(t_lo, t_hi) of cal_mean_std's expression in float64 (NaN under a negative variance)"""
    w = w.astype(np.float64) * keep[None, :, None, None]
    nz = np.count_nonzero(w)
    mu = np.abs(w).sum() / nz
    var = ((w * w).sum() - w.size * mu * mu) / w.size
    T = mu + C_RATE * np.sqrt(var) if var >= 0 else np.nan
    return A_LO * T, A_HI * T


def margin_of(w, t_lo, t_hi):
    if t_lo != t_lo:
        return np.inf
    mean_c = np.abs(w.astype(np.float64)).sum(axis=(0, 2, 3)) / (w.shape[0] * w.shape[2] * w.shape[3])
    return float(min(np.abs(mean_c - t_lo).min() / t_lo, np.abs(mean_c - t_hi).min() / t_hi))


def main():
    import torch
    root = sys.argv[1]
    dst = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "ref_dnscp.npz")
    Core, clip_cin, clip_cout = load_reference(root)
    out, n_cases = {}, 0
    seen = set()

    def make(rng, N, C, k, low, sparse):
        tex = rng.uniform(0.5, 1.0, (N, C, k, k)) * np.where(rng.random((N, C, k, k)) < 0.5, -1, 1)
        scale = rng.uniform(0.8, 1.2, C)
        scale[low] = rng.uniform(0.02, 0.1, len(low))
        w = tex * scale[None, :, None, None]
        if sparse:
            w[rng.random(w.shape) < 0.9] = 0.0
        return w.astype(np.float32)

    def case(N, C, k, n_low, n_down=0, n_up=0, sparse=False):
        """n_low channels start low; at iteration 1 n_down high channels drop low and n_up low ones rise high"""
        nonlocal n_cases
        for seed in range(1000):
            rng = np.random.default_rng(1000 * n_cases + seed)
            low0 = rng.permutation(C)[:n_low]
            w0 = make(rng, N, C, k, low0, sparse)
            high0 = np.setdiff1d(np.arange(C), low0)
            low1 = np.concatenate([low0[n_up:], rng.permutation(high0)[:n_down]]).astype(np.int64)
            w1 = make(rng, N, C, k, low1, sparse)
            t_lo, t_hi = thresholds64(w0, np.ones(C))
            m = min(margin_of(w0, t_lo, t_hi), margin_of(w1, t_lo, t_hi))
            if m >= MARGIN:
                break
        else:
            raise SystemExit(f"case {n_cases}: no seed keeps the margin")
        core = Core()
        core._param_mask_list.append(torch.ones(N, C, k, k)); core._mu_list.append(0); core._std_list.append(0)
        p0, p1 = torch.from_numpy(w0), torch.from_numpy(w1)
        core.cal_mean_std(0, 0, p0)
        tag = f"c{n_cases:02d}_"
        out[tag + "mu"], out[tag + "std"] = np.float64(float(core._mu_list[0])), np.float64(float(core._std_list[0]))
        out[tag + "margin"] = np.float64(m)
        keep = np.ones(C, np.uint8)
        for it, (w, p) in enumerate(((w0, p0), (w1, p1))):
            core.maskChannelCalc(p, 0)
            mask = core._param_mask_list[0].numpy()
            assert ((mask == 0) | (mask == 1)).all() and (mask == mask[:1, :, :1, :1]).all()
            new = mask[0, :, 0, 0].astype(np.uint8)
            out[tag + f"s{it}_w"], out[tag + f"s{it}_keep"] = w, new
            # what happened, for the tool's own assertion below (the statement is not consulted)
            mean_c = np.abs(w.astype(np.float64)).sum(axis=(0, 2, 3)) / (N * k * k)
            if t_lo == t_lo:
                k1 = np.where(keep == 1, mean_c > t_lo, mean_c > t_hi)
                seen.update({"prune"} if (keep == 1)[~k1].any() else set())
                seen.update({"revive"} if (keep == 0)[k1].any() else set())
            else:
                k1 = keep == 1
                seen.add("negative variance")
            nz = int(k1.sum())
            target = round(nz / 16) * 16 or 16
            seen.update({"fix+"} if target > nz else {"fix-"} if target < nz else set())
            seen.update({"tie 2.5"} if nz == 40 else set())
            seen.update({"floor 16"} if round(nz / 16) == 0 else set())
            seen.update({"C too small"} if target > C else set())
            assert int(new.sum()) == min(target, C), (tag, it, nz, target, int(new.sum()))
            keep = new
        w_kept, idx = clip_cin(p1, core._param_mask_list[0])
        pw = rng.standard_normal((C, 5, k, k)).astype(np.float32)
        pv = rng.standard_normal(C).astype(np.float32)
        out[tag + "w_kept"], out[tag + "idx"] = w_kept.numpy(), idx.numpy().astype(np.int64)
        out[tag + "pw"], out[tag + "pv"] = pw, pv
        out[tag + "pw_kept"] = clip_cout(torch.from_numpy(pw), idx).numpy()
        out[tag + "pv_kept"] = clip_cout(torch.from_numpy(pv), idx).numpy()
        n_cases += 1

    case(8, 48, 1, 13, n_down=5, n_up=4)         # 35 kept -> 32: the first 3 kept go; both hysteresis branches at iteration 1
    case(6, 56, 3, 16, n_down=3)                 # 40 kept: 2.5 rounds to even, 32
    case(4, 33, 3, 4, n_up=2)                    # few low channels: the threshold sits among the high ones; 21 kept -> 16, then 27 -> 32
    case(16, 64, 1, 19, n_down=6, n_up=6)        # 45 kept -> 48
    case(5, 20, 1, 15)                           # 5 kept -> round gives 0 -> 16
    case(3, 12, 3, 9, n_up=3)                    # 3 kept -> 16 with C = 12: the loop runs out
    case(8, 24, 3, 0, sparse=True)               # nine weights in ten are zero: negative variance, NaN thresholds, 24 kept -> 32 runs out
    case(7, 80, 1, 30, n_down=10, n_up=10)       # C no multiple of 16: 50 kept -> 48
    want = {"prune", "revive", "fix+", "fix-", "tie 2.5", "floor 16", "C too small", "negative variance"}
    assert seen == want, sorted(want - seen)
    out["n_cases"] = np.asarray(n_cases, np.int64)
    np.savez_compressed(dst, **out)
    print(f"{dst}: {n_cases} cases, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
