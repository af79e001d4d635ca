#!/usr/bin/env python3
"""Time the native KL-f8 VAE decoder (sfron.vae.VAEDecoder.decode_u8, save_image bytes) at three shapes: 256 px batch 10 (the DiT
snapshot grid of DiT/forget.py:114-145), 256 px batch 32 and 512 px batch 8 (SD), random weights.  HIP events around each call, warm-up
first, median of N; prints one JSON line.
    python tools/bench_vae_decoder.py [--iters 10] [--warmup 3] [--only 256x10|256x32|512x8]
    python tools/bench_vae_decoder.py --profile      # one warm 256 px batch-32 decode after the warm-up (under rocprofv3 --kernel-trace --stats)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

PEAK_BF16 = 2.5e15          # MI355X dense bf16 matrix peak, FLOP/s
SHAPES = {"256x10": (256, 10), "256x32": (256, 32), "512x8": (512, 8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=list(SHAPES), default=None)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    from sfron import vae
    specs, _ = vae.decoder_plan()
    g = torch.Generator().manual_seed(0)
    sd = {}
    for k, shp in specs.items():
        r = torch.randn(shp, generator=g)
        sd[("decoder." + k) if not k.startswith("post_quant_conv.") else k] = (
            r / float(torch.tensor(shp[1:]).prod()) ** 0.5 if k.endswith(".weight") and len(shp) == 4 else
            (1 + 0.1 * r if k.endswith(".weight") else 0.1 * r))
    dec = vae.VAEDecoder.from_state_dict(sd)
    out = {"metric": "KL-f8 VAE decoder decode_u8() (save_image bytes)", "peak_bf16_flops": PEAK_BF16}
    names = ["256x32"] if a.profile else ([a.only] if a.only else list(SHAPES))
    for name in names:
        size, B = SHAPES[name]
        z = (torch.randn(B, 4, size // 8, size // 8, generator=g) * 0.8).cuda()
        for _ in range(a.warmup):
            dec.decode_u8(z)
        torch.cuda.synchronize()
        if a.profile:
            dec.decode_u8(z)
            torch.cuda.synchronize()
            print(json.dumps({"profiled": f"{size}px batch {B}, one decode_u8 after {a.warmup} warm-up calls"}))
            return
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dec.decode_u8(z)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ms = statistics.median(ts)
        flops = vae.decoder_flops(size, size) * B
        out[name] = {"px": size, "batch": B, "chunk": dec.chunk_size(size, size), "ms_median": round(ms, 3), "ms_min": round(min(ts), 3),
                     "images_per_s": round(B / ms * 1e3, 1), "tflops": round(flops / ms / 1e9, 1),
                     "frac_peak": round(flops / ms / 1e-3 / PEAK_BF16, 3), "gflop_per_image": round(vae.decoder_flops(size, size) / 1e9, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
