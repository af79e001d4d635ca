#!/usr/bin/env python3
"""Time the native classifier evaluators' forward pass (sfron.resnet.ResNet.forward_u8: uint8 images -> fp32 logits) at the two shapes the
reference scripts run: ResNet-34 at 224 px batch 64 (DDPM/classifier_evaluation.py) and ResNet-50 at 224 px batch 250
(SD/eval-scripts/imageclassify.py), random weights.  HIP events around each call, warm-up first; five rounds of --iters calls, each round's
time is its median call; prints one JSON line with the minimum round, the spread of the rounds, images/s and TFLOP/s.
    python tools/bench_classifier.py [--iters 5] [--warmup 3] [--rounds 5] [--only resnet34|resnet50]
    python tools/bench_classifier.py --profile      # one warm ResNet-50 batch after the warm-up (under rocprofv3 --kernel-trace --stats)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

PEAK_BF16 = 2.5e15          # MI355X dense bf16 matrix peak, FLOP/s
SHAPES = {"resnet34": (224, 64, 10), "resnet50": (224, 250, 1000)}       # px, batch, classes


def random_state_dict(specs, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in specs.items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros((), dtype=torch.int64)
        elif len(shp) == 4:                                   # Kaiming fan-out
            sd[k] = torch.randn(shp, generator=g) * (2.0 / (shp[0] * shp[2] * shp[3])) ** 0.5
        elif len(shp) == 2:
            sd[k] = torch.randn(shp, generator=g) / shp[1] ** 0.5
        elif k.endswith(("running_var", "bn1.weight", "bn2.weight", "bn3.weight", "downsample.1.weight")):
            sd[k] = torch.rand(shp, generator=g) + 0.5
        else:
            sd[k] = torch.randn(shp, generator=g) * 0.1
    return sd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=list(SHAPES), default=None)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    from sfron import classify, resnet
    out = {"metric": "ResNet forward_u8() (uint8 images -> fp32 logits)", "peak_bf16_flops": PEAK_BF16}
    names = ["resnet50"] if a.profile else ([a.only] if a.only else list(SHAPES))
    for name in names:
        px, B, ncls = SHAPES[name]
        model = getattr(resnet, name)(ncls)
        model.load_state_dict(random_state_dict(model.specs, 0))
        mean, std = ((0.5,) * 3, (0.5,) * 3) if name == "resnet34" else (classify.IMAGENET_MEAN, classify.IMAGENET_STD)
        img = torch.randint(0, 256, (B, px, px, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
        for _ in range(a.warmup):
            model.forward_u8(img, mean, std)
        torch.cuda.synchronize()
        if a.profile:
            model.forward_u8(img, mean, std)
            torch.cuda.synchronize()
            print(json.dumps({"profiled": f"{name} {px}px batch {B}, one forward_u8 after {a.warmup} warm-up calls"}))
            return
        rounds = []
        for _ in range(a.rounds):
            ts = []
            for _ in range(a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                model.forward_u8(img, mean, std)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            rounds.append(statistics.median(ts))
        ms = min(rounds)
        per_image = resnet.resnet_flops(model.block, model.layers, ncls, px, px)
        out[name] = {"px": px, "batch": B, "chunk": model.chunk_size(px, px), "ms_min": round(ms, 3), "ms_rounds": [round(r, 3) for r in rounds],
                     "spread": round((max(rounds) - ms) / ms, 4), "images_per_s": round(B / ms * 1e3, 1),
                     "tflops": round(per_image * B / ms / 1e9, 1), "frac_peak": round(per_image * B / ms / 1e-3 / PEAK_BF16, 4),
                     "gflop_per_image": round(per_image / 1e9, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
