#!/usr/bin/env python3
"""Time the native KL-f8 VAE encoder (sfron.vae.VAEEncoder.moments) at the two shapes the loops use: 256 px batch 32 (DiT) and 512 px
batch 8 (SD), random weights.  HIP events around each call, warm-up first, median of N; prints one JSON line.
    python tools/bench_vae.py [--iters 10] [--warmup 3] [--only 256|512]
    python tools/bench_vae.py --profile      # one warm 256 px batch-32 encode after the warm-up (under rocprofv3 --kernel-trace --stats)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

PEAK_BF16 = 2.5e15          # MI355X dense bf16 matrix peak, FLOP/s
SHAPES = {256: 32, 512: 8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", type=int, choices=sorted(SHAPES), default=None)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    from sfron import vae
    specs, _ = vae.encoder_plan()
    g = torch.Generator().manual_seed(0)
    sd = {}
    for k, shp in specs.items():
        r = torch.randn(shp, generator=g)
        sd[("encoder." + k) if not k.startswith("quant_conv.") else k] = (
            r / float(torch.tensor(shp[1:]).prod()) ** 0.5 if k.endswith(".weight") and len(shp) == 4 else
            (1 + 0.1 * r if k.endswith(".weight") else 0.1 * r))
    enc = vae.VAEEncoder.from_state_dict(sd)
    out = {"metric": "KL-f8 VAE encoder moments()", "peak_bf16_flops": PEAK_BF16}
    sizes = [256] if a.profile else ([a.only] if a.only else sorted(SHAPES))
    for size in sizes:
        B = SHAPES[size]
        imgs = torch.randint(0, 256, (B, size, size, 3), dtype=torch.uint8, generator=g).cuda()
        for _ in range(a.warmup):
            enc.moments(imgs)
        torch.cuda.synchronize()
        if a.profile:
            enc.moments(imgs)
            torch.cuda.synchronize()
            print(json.dumps({"profiled": f"{size}px batch {B}, one encode after {a.warmup} warm-up calls"}))
            return
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            enc.moments(imgs)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ms = statistics.median(ts)
        flops = vae.encoder_flops(size, size) * B
        r = {"batch": B, "ms_median": round(ms, 3), "ms_min": round(min(ts), 3), "images_per_s": round(B / ms * 1e3, 1),
             "tflops": round(flops / ms / 1e9, 1), "frac_peak": round(flops / ms / 1e-3 / PEAK_BF16, 3),
             "gflop_per_image": round(vae.encoder_flops(size, size) / 1e9, 2)}
        if size == 256:
            r["ms_added_per_dit_step"] = round(2 * ms * 32 / B, 2)       # the forget and the remain batch, 32 images each
        out[f"{size}px"] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
