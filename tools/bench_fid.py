#!/usr/bin/env python3
"""Time the FID path: the Inception-v3 extractor (sfron.inception.InceptionV3.forward_u8: uint8 images -> the 2048-wide features) at batch
64 with random weights, and the fp64 feature statistics (sfron.fid.feature_statistics: mean and covariance) at N = 10 000, D = 2048.
HIP events around each call, warm-up first; --rounds rounds of --iters calls, each round's time is its median call; prints one JSON line
with the minimum round, the spread of the rounds, images/s and algorithmic TFLOP/s (inception.flops), and the statistics' time.
    python tools/bench_fid.py [--iters 5] [--warmup 3] [--rounds 5] [--px 64] [--batch 64] [--n 10000] [--d 2048]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

PEAK_BF16 = 2.5e15          # MI355X dense bf16 matrix peak, FLOP/s


def random_state_dict(specs, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in specs.items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros((), dtype=torch.int64)
        elif len(shp) == 4:                                   # Kaiming fan-in
            sd[k] = torch.randn(shp, generator=g) * (2.0 / (shp[1] * shp[2] * shp[3])) ** 0.5
        elif len(shp) == 2:
            sd[k] = torch.randn(shp, generator=g) / shp[1] ** 0.5
        elif k.endswith(("running_var", "bn.weight")):
            sd[k] = torch.rand(shp, generator=g) + 0.5
        else:
            sd[k] = torch.randn(shp, generator=g) * 0.1
    return sd


def timed(fn, iters, rounds):
    out = []
    for _ in range(rounds):
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        out.append(statistics.median(ts))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--px", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--d", type=int, default=2048)
    a = ap.parse_args()
    from sfron import fid, inception
    model = inception.InceptionV3()
    model.load_state_dict(random_state_dict(model.specs, 0))
    img = torch.randint(0, 256, (a.batch, a.px, a.px, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    for _ in range(a.warmup):
        model.forward_u8(img, taps=(2048,))
    torch.cuda.synchronize()
    rounds = timed(lambda: model.forward_u8(img, taps=(2048,)), a.iters, a.rounds)
    ms = min(rounds)
    per_image = inception.flops()
    out = {"metric": "InceptionV3.forward_u8() (uint8 images -> 2048 features) and fid.feature_statistics()", "peak_bf16_flops": PEAK_BF16,
           "extractor": {"px": a.px, "batch": a.batch, "chunk": model.chunk_size(a.px, a.px), "ms_min": round(ms, 3),
                         "ms_rounds": [round(r, 3) for r in rounds], "spread": round((max(rounds) - ms) / ms, 4),
                         "images_per_s": round(a.batch / ms * 1e3, 1), "tflops": round(per_image * a.batch / ms / 1e9, 1),
                         "frac_peak": round(per_image * a.batch / ms / 1e-3 / PEAK_BF16, 4), "gflop_per_image": round(per_image / 1e9, 2)}}
    x = torch.randn(a.n, a.d, generator=torch.Generator().manual_seed(2)).cuda()
    for _ in range(a.warmup):
        fid.feature_statistics(x)
    rounds = timed(lambda: fid.feature_statistics(x), a.iters, a.rounds)          # includes the copy of mu and sigma to the host
    ms = min(rounds)
    out["statistics"] = {"n": a.n, "d": a.d, "ms_min": round(ms, 3), "ms_rounds": [round(r, 3) for r in rounds],
                         "spread": round((max(rounds) - ms) / ms, 4), "fp64_tflops": round(2.0 * a.n * a.d * a.d / 2 / ms / 1e9, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
