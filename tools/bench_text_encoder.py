#!/usr/bin/env python3
"""Time the native CLIP text encoder (sfron.text.CLIPTextEncoder.encode_ids) at SD v1's ViT-L/14 shape (49408 x 768, 12 layers, 12 heads,
MLP 3072, 77 tokens) with seeded random weights, at 2, 8, 32 and 128 prompts.  HIP events around each call (no host synchronisation inside:
check_ids=False), warm-up first, median of N; prints one line per batch and one JSON line.
    python tools/bench_text_encoder.py [--iters 20] [--warmup 3] [--batches 2,8,32,128]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

PEAK_BF16 = 2.5e15          # MI355X dense bf16 matrix peak, FLOP/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="2,8,32,128")
    a = ap.parse_args()
    from sfron import text
    specs, _ = text.param_specs()
    g = torch.Generator().manual_seed(0)
    sd = {}
    for n, shp in specs.items():
        r = torch.randn(shp, generator=g)
        if ".qkv_proj." in n:
            for i, p in enumerate(("q_proj", "k_proj", "v_proj")):
                part = r[i * 768:(i + 1) * 768]
                sd["text_model." + n.replace("qkv_proj", p)] = part * (768 ** -0.5 if n.endswith("weight") else 0.02)
            continue
        sd["text_model." + n] = (r * shp[1] ** -0.5 if len(shp) == 2 and "embedding" not in n else
                                 r * 0.02 if "embedding" in n or n.endswith("bias") else 1 + 0.1 * r)
    enc = text.CLIPTextEncoder.from_state_dict(sd)
    fl = text.encoder_flops()
    out = {"metric": "CLIP ViT-L/14 text encoder encode_ids(), 77 tokens", "gflop_per_prompt": round(fl / 1e9, 2), "peak_bf16_flops": PEAK_BF16}
    print(f"{'prompts':>8} {'ms median':>10} {'ms min':>8} {'prompts/s':>10} {'TFLOP/s':>8}")
    for B in (int(b) for b in a.batches.split(",")):
        ids = torch.randint(0, 49406, (B, 77), generator=g)
        ids[:, 0] = 49406
        ids = ids.cuda()
        for _ in range(a.warmup):
            enc.encode_ids(ids, check_ids=False)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            enc.encode_ids(ids, check_ids=False)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ms = statistics.median(ts)
        row = {"ms_median": round(ms, 3), "ms_min": round(min(ts), 3), "prompts_per_s": round(B / ms * 1e3, 1),
               "tflops": round(fl * B / ms / 1e9, 1)}
        out[f"B{B}"] = row
        print(f"{B:>8} {row['ms_median']:>10.3f} {row['ms_min']:>8.3f} {row['prompts_per_s']:>10.1f} {row['tflops']:>8.1f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
