#!/usr/bin/env python3
"""Time the SD image transform (Resize(512, bicubic) -> CenterCrop(512) -> RGB, sfron.resample) on the GPU against one host thread of Pillow,
per image, at three source sizes: 1536x2048 and 768x1024 (down-scaling) and 375x500 (up-scaling).
  kernel pair ....... sfron_image_resample_u8 alone, the source already resident: HIP events, median of N after warm-ups
  sd_transform_gpu .. the whole call from a decoded PIL image: pixel copy into the pinned buffer, upload, two launches; wall clock to the
                      end of the stream's work, median of N
  sd_transform ...... Pillow on one host thread (the yardstick: what the host route of the loaders costs), wall clock, median of N
The last JSON line carries the numbers and ``gpu_beats_host_at_1536x2048``, the rule ConceptImageLoader's gpu_resize default follows.
    python tools/bench_resample.py [--iters 10] [--warmup 3] [--size 512] [--interpolation bicubic]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402


def photograph(h, w, seed):
    """A synthetic photograph: smooth colour fields plus grain (the arithmetic does not depend on the content; the bytes are not constant)."""
    rng = np.random.default_rng(seed)
    low = Image.fromarray(rng.integers(0, 256, size=(h // 32 + 2, w // 32 + 2, 3), dtype=np.uint8)).resize((w, h), Image.BICUBIC)
    grain = rng.integers(-12, 13, size=(h, w, 3))
    return Image.fromarray(np.clip(np.asarray(low).astype(np.int16) + grain, 0, 255).astype(np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--interpolation", default="bicubic")
    a = ap.parse_args()
    from sfron import resample
    S, interp, dev = a.size, a.interpolation, torch.device("cuda", torch.cuda.current_device())
    out = {"metric": f"SD image transform to {S} px ({interp}), ms per image", "iters": a.iters, "warmup": a.warmup}
    print(f"{'source HxW':>12} {'kernel pair':>12} {'sd_transform_gpu':>17} {'Pillow 1 thread':>16}   (ms, medians)")
    for h, w in ((1536, 2048), (768, 1024), (375, 500)):
        img = photograph(h, w, h)
        arr = np.array(img)
        want = torch.from_numpy(resample.sd_transform(img, S, interp))
        # the kernel pair alone
        tx, ty = resample.window_tables(w, h, S, interp)
        y0, y1 = ty.rows()
        src = torch.from_numpy(arr).to(dev).reshape(-1)
        tmp = torch.empty((y1 - y0) * S * 3, dtype=torch.uint8, device=dev)
        dst = torch.empty(S, S, 3, dtype=torch.uint8, device=dev)
        ts = []
        for i in range(a.warmup + a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            status = resample.image_resample_u8(src, h, w, tx, ty, tmp, dst)
            e1.record()
            e1.synchronize()
            assert status == 0, status
            if i >= a.warmup:
                ts.append(e0.elapsed_time(e1))
        assert torch.equal(dst.cpu(), want), "the kernel does not reproduce Pillow"
        k_ms = statistics.median(ts)
        # the whole device route from a decoded image
        ts = []
        for i in range(a.warmup + a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = resample.sd_transform_gpu([img], S, interp, device=dev)
            torch.cuda.synchronize()
            if i >= a.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        assert torch.equal(got[0].cpu(), want)
        g_ms = statistics.median(ts)
        # Pillow, one thread
        ts = []
        for i in range(a.warmup + a.iters):
            t0 = time.perf_counter()
            resample.sd_transform(img, S, interp)
            if i >= a.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        p_ms = statistics.median(ts)
        out[f"{h}x{w}"] = {"kernel_pair_ms": round(k_ms, 4), "sd_transform_gpu_ms": round(g_ms, 4), "pillow_one_thread_ms": round(p_ms, 4),
                          "rows_read": y1 - y0, "ksize_x": tx.ksize, "ksize_y": ty.ksize}
        print(f"{h:>7}x{w:<4} {k_ms:>12.4f} {g_ms:>17.4f} {p_ms:>16.4f}")
    big = out["1536x2048"]
    out["gpu_beats_host_at_1536x2048"] = bool(big["sd_transform_gpu_ms"] < big["pillow_one_thread_ms"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
