#!/usr/bin/env python3
"""Cost of JPEG reconstruction on the device (tf2_jpeg_idct, jpeg_idct.hip) and of the host step in front of it: --batch frames of
--src-h x --src-w, 4:2:0.  The frames are synthetic (smooth shapes plus noise), encoded once here by a trivial baseline encoder --
float DCT, the standard luminance quantiser at quality 90, Huffman tables of the standard shape filled by symbol frequency;
--distinct different files, repeated to fill the batch -- so the tool needs no image library.  In one process:
  1. tf2_jpeg_idct beside the yardstick tf2_ycc_to_rgb on the planes it wrote: HIP events on one stream around each call, the calls
     alternating inside every step, --repeats repeats of --steps steps after a warm-up; the median over the repeats' medians and
     their lowest and highest, the bytes each moves (coefficients read of the blocks that hold samples, planes written; planes
     read, pixels written) and the ratio;
  2. the host -> device copy (pinned memory) of the dense coefficient buffer, of the planes and of the RGB pixels, the same way;
  3. the host step, tf2_jpeg_parse + tf2_jpeg_entropy, in images/s on 1 and on 16 threads -- and, where Pillow is importable,
     Pillow's Image.open(file).convert('RGB') on the same files and threads (else "absent");
  4. images/s of ResNet-50 (synthetic weights) with --inflight batches in flight, one captured graph per (stream, buffer) replayed
     round robin as bench.py does, each graph holding
       planes   tf2_ycc_to_rgb + tf2_preprocess_aa (TORCHVISION_PIL, int8) + network + classifier, from planes on the device
       jpeg     tf2_jpeg_idct in front of the same four, from coefficients on the device
Prints one JSON line and writes it to --out (default profiles/jpeg_time_b<batch>.json).  `--kernel-only` leaves step 4 out."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QLUM = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80,
                 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98,
                 112, 100, 103, 99])
QUANT = np.maximum(1, (QLUM * 20 + 50) // 100)                       # the standard table at libjpeg's quality 90
DC_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]            # codes per length 1..16: the shape of the standard tables
AC_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]


def synth_frame(rng, h, w):
    """uint8 [h, w, 3] taken as Y, Cb, Cr: smooth blobs and edges plus noise (stronger in Y), so that a file is about as large as
    a photograph's"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 3))
    for c in range(3):
        for _ in range(6):
            cy, cx, s, a = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(20, 120), rng.uniform(-70, 70)
            img[:, :, c] += a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
        img[:, :, c] += np.where(xx * rng.uniform(-1, 1) + yy * rng.uniform(-1, 1) > rng.uniform(-100, 200), rng.uniform(-40, 40), 0)
    img += 128 + rng.normal(0, 1.0, (h, w, 3)) * np.array([10.0, 3.0, 3.0])
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def quantised_blocks(plane, bw, bh, q):
    """int32 [bh * bw, 64] (natural order): the float DCT of the plane padded by edge repetition to bh x bw blocks, over q, rounded"""
    p = np.pad(plane.astype(np.float64) - 128, ((0, bh * 8 - plane.shape[0]), (0, bw * 8 - plane.shape[1])), mode="edge")
    k = np.arange(8)
    D = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k[:, None] == 0, np.sqrt(1 / 8), 0.5)
    b = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
    return np.rint(np.einsum("vy,abyx,ux->abvu", D, b, D).reshape(-1, 64) / q).astype(np.int32)


def symbols(coefs, order, zigzag):
    """the scan as [(table: 0 DC / 1 AC, symbol, extra bits value, extra bits count)] of blocks [n, 64] visited in `order`, which is
    a list of (component, block index); coefs: per component"""
    out, pred = [], [0] * len(coefs)
    for c, i in order:
        zz = coefs[c][i][zigzag].tolist()
        d = zz[0] - pred[c]
        pred[c] = zz[0]
        s = abs(d).bit_length()
        out.append((0, s, d if d >= 0 else d + (1 << s) - 1, s))
        run, last = 0, max((k for k in range(1, 64) if zz[k]), default=0)
        for k in range(1, last + 1):
            v = zz[k]
            if v == 0:
                run += 1
                continue
            while run > 15:
                out.append((1, 0xF0, 0, 0))
                run -= 16
            s = abs(v).bit_length()
            out.append((1, (run << 4) | s, v if v >= 0 else v + (1 << s) - 1, s))
            run = 0
        if last < 63:
            out.append((1, 0x00, 0, 0))
    return out


def table_of(freq, bits, universe):
    """(symbols in code order, {symbol: (code, length)}): the canonical code of shape `bits`, the most frequent symbol first"""
    syms = sorted(universe, key=lambda s: (-freq.get(s, 0), s))
    codes, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            codes[syms[k]] = (code, ln)
            code, k = code + 1, k + 1
        code <<= 1
    return syms, codes


def encode(frame, sub, zigzag):
    """a baseline JFIF file of a [h, w, 3] YCbCr frame (one scan, no restart markers, its own Huffman tables)"""
    import struct
    from tf2_amd import ycc as Y
    h, w = frame.shape[:2]
    planes = Y.subsample_box(frame, sub)
    mw, mh = -(-w // (8 * sub[0])), -(-h // (8 * sub[1]))
    grids = [(mw * sub[0], mh * sub[1]), (mw, mh), (mw, mh)]
    coefs = [quantised_blocks(p, bw, bh, QUANT) for p, (bw, bh) in zip(planes, grids)]
    order = []
    for r in range(mh):
        for q in range(mw):
            order += [(0, (r * sub[1] + y) * grids[0][0] + q * sub[0] + x) for y in range(sub[1]) for x in range(sub[0])]
            order += [(1, r * mw + q), (2, r * mw + q)]
    syms = symbols(coefs, order, zigzag)
    freq = [{}, {}]
    for t, s, _, _ in syms:
        freq[t][s] = freq[t].get(s, 0) + 1
    dc_syms, dc = table_of(freq[0], DC_BITS, range(12))
    ac_syms, ac = table_of(freq[1], AC_BITS, [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)])
    acc, n, out = 0, 0, bytearray()
    for t, s, v, nv in syms:
        code, ln = (ac if t else dc)[s]
        acc, n = (acc << (ln + nv)) | (code << nv) | v, n + ln + nv
        while n >= 8:
            b = (acc >> (n - 8)) & 0xFF
            out.append(b)
            if b == 0xFF:
                out.append(0)
            n -= 8
        acc &= (1 << n) - 1
    if n:
        b = ((acc << (8 - n)) | ((1 << (8 - n)) - 1)) & 0xFF
        out.append(b)
        if b == 0xFF:
            out.append(0)
    seg = lambda m, payload: bytes([0xFF, m]) + struct.pack(">H", len(payload) + 2) + payload
    head = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    head += seg(0xDB, bytes([0]) + bytes(QUANT[zigzag].tolist()))
    head += seg(0xC0, struct.pack(">BHHB", 8, h, w, 3) + bytes([1, (sub[0] << 4) | sub[1], 0, 2, 0x11, 0, 3, 0x11, 0]))
    head += seg(0xC4, bytes([0x00]) + bytes(DC_BITS) + bytes(dc_syms) + bytes([0x10]) + bytes(AC_BITS) + bytes(ac_syms))
    head += seg(0xDA, bytes([3, 1, 0x00, 2, 0x00, 3, 0x00, 0, 63, 0]))
    return head + bytes(out) + b"\xff\xd9"


def rate(fn, files, threads, seconds=1.0):
    """images/s of fn over the files on `threads` threads, for at least `seconds`"""
    done, t0 = 0, time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as pool:
        while time.perf_counter() - t0 < seconds:
            list(pool.map(fn, files))
            done += len(files)
    return done / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--src-h", type=int, default=375)
    ap.add_argument("--src-w", type=int, default=500)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tf2_amd import classify as K, config as cfg, jpeg as J, preprocess as P, synth, ycc as Y
    from tf2_amd.network import NetWork, Runner
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = "cuda:0"
    rng = np.random.default_rng(7)
    h, w, B, sub, layout = a.src_h, a.src_w, a.batch, (2, 2), Y.PLANAR

    t0 = time.perf_counter()
    distinct = [encode(synth_frame(rng, h, w), sub, J.ZIGZAG) for _ in range(a.distinct)]
    files = [distinct[i % a.distinct] for i in range(B)]
    res = dict(batch=B, src_hw=[h, w], sub=list(sub), steps=a.steps, repeats=a.repeats, inflight=a.inflight, distinct_files=a.distinct,
               file_bytes=[len(f) for f in distinct], encode_s=round(time.perf_counter() - t0, 2),
               blocks_per_image=J.default_blocks_per_image(B))
    items = [(info, coef) for info, coef, st in J.decode_host(files, threads=a.threads) if st == 0]
    assert len(items) == B, "the tool's own files must decode"
    info0 = items[0][0]
    assert (info0.h, info0.w, info0.sub, info0.upsample) == (h, w, sub, Y.FANCY)

    # -- 3. the host step
    def host_step(data):
        info = J.parse(data)
        return J.entropy(data, info)[1]
    res["host_decode_images_per_s_1_thread"] = round(rate(host_step, files, 1), 1)
    res[f"host_decode_images_per_s_{a.threads}_threads"] = round(rate(host_step, files, a.threads), 1)
    try:
        import io
        import PIL
        from PIL import Image
        pil = lambda data: Image.open(io.BytesIO(data)).convert("RGB").size
        res["pillow"] = PIL.__version__
        res["pillow_images_per_s_1_thread"] = round(rate(pil, files, 1), 1)
        res[f"pillow_images_per_s_{a.threads}_threads"] = round(rate(pil, files, a.threads), 1)
        res["rgb_equals_pillow"] = bool(np.array_equal(J.rgb_of_file(*items[0]), np.asarray(Image.open(io.BytesIO(files[0])).convert("RGB"))))
    except ImportError:
        res["pillow"] = "absent"

    # -- 1. the kernels
    n_buf = 2 * a.inflight
    bufs = [J.pack(items[k % B:] + items[:k % B], layout, sub, dev, 3, preset=P.TORCHVISION_PIL) for k in range(n_buf)]
    dec, conv = J.DeviceDecoder(J.Desc(layout, sub)), Y.DeviceConverter(Y.Desc(layout=layout, sub=sub))
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    ch, cw = Y.chroma_size(h, w, sub)
    used = -(-h // 8) * -(-w // 8) + 2 * -(-ch // 8) * -(-cw // 8)
    plane_bytes, rgb_bytes, coef_bytes = B * (h * w + 2 * ch * cw), B * h * w * 3, int(bufs[0][0].numel()) * 2
    moved = {"idct": B * used * 128 + plane_bytes, "ycc": plane_bytes + rgb_bytes}
    res.update(coef_buffer_bytes=coef_bytes, plane_bytes=plane_bytes, rgb_bytes=rgb_bytes, idct_bytes_moved=moved["idct"], ycc_bytes_moved=moved["ycc"])
    s = torch.cuda.current_stream()
    calls = {"idct": lambda k: dec.run(*bufs[k][:6], status=status),
             "ycc": lambda k: conv.run(bufs[k][3], bufs[k][4], bufs[k][6], bufs[k][5], status=status)}
    # host -> device copies, pinned
    pinned = {"coef": torch.empty(coef_bytes, dtype=torch.uint8).pin_memory(), "planes": torch.empty(plane_bytes, dtype=torch.uint8).pin_memory(),
              "rgb": torch.empty(rgb_bytes, dtype=torch.uint8).pin_memory()}
    landing = {k: torch.empty(v.numel(), dtype=torch.uint8, device=dev) for k, v in pinned.items()}
    for name in pinned:
        calls["copy_" + name] = (lambda n: lambda k: landing[n].copy_(pinned[n], non_blocking=True))(name)
    for k in range(max(a.warmup, n_buf)):                          # (also brings the clocks up)
        for fn in calls.values():
            fn(k % n_buf)
    torch.cuda.synchronize()
    assert (status.cpu() == 0).all()
    meds = {name: [] for name in calls}
    for _ in range(a.repeats):
        evs = {name: [] for name in calls}
        for k in range(a.steps):
            for name, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                fn(k % n_buf)
                e1.record(s)
                evs[name].append((e0, e1))
        torch.cuda.synchronize()
        for name in calls:
            meds[name].append(float(np.median([e0.elapsed_time(e1) for e0, e1 in evs[name]])) * 1e3)
    for name in calls:
        us = float(np.median(meds[name]))
        res[f"{name}_us"] = round(us, 2)
        res[f"{name}_us_spread"] = [round(min(meds[name]), 2), round(max(meds[name]), 2)]
        nbytes = moved.get(name) or pinned[name[5:]].numel()
        res[f"{name}_gb_per_s"] = round(nbytes / us * 1e-3, 1)
    res["idct_over_ycc"] = round(res["idct_us"] / res["ycc_us"], 3)
    res["coef_bytes_over_plane_bytes"] = round(coef_bytes / plane_bytes, 3)
    res["coef_bytes_over_rgb_bytes"] = round(coef_bytes / rgb_bytes, 3)

    # -- 4. ResNet-50 with batches in flight
    if not a.kernel_only:
        t50 = cfg.resnet50_tables()
        q50 = np.loadtxt(os.path.join(ROOT, "tests", "golden", "resnet50_Q"), dtype=np.int32)
        net = NetWork(t50)
        net.Init(synth.synth_model(t50, q50, 0), synth.q_text(q50), device=dev)
        pp_aa = P.Preprocessor(net, P.TORCHVISION_PIL, "RGB")
        streams = [torch.cuda.Stream() for _ in range(a.inflight)]
        runners = [Runner(None, net) for _ in range(a.inflight)]
        clss = [K.DeviceClassifier(net, 5) for _ in range(a.inflight)]
        stats = [(torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)) for _ in range(n_buf)]

        def step(kind, i, k):
            coef, jp, qt, planes, yc, sc, px = bufs[k]
            if kind == "jpeg":
                dec.run(coef, jp, qt, planes, yc, sc, status=stats[k][0])
            conv.run(planes, yc, px, sc, status=stats[k][1])
            return clss[i].run(runners[i].run_batch(pp_aa(px, sc, out="q")[0], concurrency=1))
        for kind in ("planes", "jpeg"):
            graphs = {}
            for k in range(n_buf):
                i = k % a.inflight
                step(kind, i, k)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                streams[i].wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(streams[i]):
                    with torch.cuda.graph(g, stream=streams[i]):
                        step(kind, i, k)
                torch.cuda.current_stream().wait_stream(streams[i])
                graphs[k] = g
            torch.cuda.synchronize()

            def run(n):
                for k in range(n):
                    with torch.cuda.stream(streams[k % a.inflight]):
                        graphs[k % n_buf].replay()
            rates = []
            for _ in range(a.repeats):
                run(a.warmup)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(a.steps)
                torch.cuda.synchronize()
                rates.append(B * a.steps / (time.perf_counter() - t0))
            res[f"inflight_{kind}"] = round(float(np.median(rates)), 1)
            res[f"inflight_{kind}_spread"] = [round(min(rates), 1), round(max(rates), 1)]
            del graphs
        res["inflight_jpeg_over_planes"] = round(res["inflight_jpeg"] / res["inflight_planes"], 4)
    line = json.dumps(res)
    print(line)
    out = a.out or os.path.join(ROOT, "profiles", f"jpeg_time_b{B}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
