#!/usr/bin/env python3
"""Time ADM's centre crop (latents.center_crop_arr: BOX halvings, BICUBIC, crop) of a batch of 32 images to 256 px on the GPU, a whole
batch per launch, against the launches it replaces and against one host thread of Pillow.  Three batches:
  375x500 .... 32 sources of 375 x 500 (no halving)
  768x1024 ... 32 sources of 768 x 1024 (one halving)
  mixed ...... 32 sources of eight sizes in both orientations, a 2048 x 1536 among them (two halvings)
and for each
  batched ......... sfron_image_resample_batch_u8, sources / tables / records resident: HIP events around the level launches
  per_image ....... the same plans image by image through sfron_image_resample_u8 (two launches per stage and image): HIP events
  center_crop_gpu . the whole call from decoded arrays: plan, gather into the pinned buffer, one upload, the level launches; wall clock
                    to the end of the stream's work
  pillow .......... center_crop_arr over the batch on one host thread, wall clock
Medians of N after warm-ups; every device result is compared with Pillow's bytes in the same run.  Each batch runs in a fresh child
process under its own time limit, and the run stops at the first one that fails.  The last JSON line carries the numbers.
    python tools/bench_center_crop.py [--iters 10] [--warmup 3] [--batch 32] [--size 256] [--limit 240] [--only NAME]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIX = [(375, 500), (768, 1024), (1536, 2048), (500, 375), (333, 500), (1024, 768), (480, 640), (2048, 1536)]          # (H, W)
BATCHES = {"375x500": [(375, 500)], "768x1024": [(768, 1024)], "mixed": MIX}


def events(fn, warmup, iters):
    import torch
    ts = []
    for i in range(warmup + iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def wall(fn, warmup, iters, sync):
    ts = []
    for i in range(warmup + iters):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def run_batch(name, a):
    import numpy as np
    import torch
    from PIL import Image
    from bench_resample import photograph
    from sfron import _lib, latents, resample
    S, B = a.size, a.batch
    dev = torch.device("cuda", torch.cuda.current_device())
    shapes = [BATCHES[name][i % len(BATCHES[name])] for i in range(B)]
    made = {hw: np.array(photograph(hw[0], hw[1], hw[0] + 7 * hw[1])) for hw in set(shapes)}
    srcs = [made[hw] for hw in shapes]
    want = torch.from_numpy(np.stack([np.asarray(latents.center_crop_arr(Image.fromarray(made[hw]), S)) for hw in shapes]))
    plans = [resample.center_crop_plan(w, h, S) for h, w in shapes]
    # batched: everything resident
    bp = resample.plan_batch([p.stages for p in plans])
    assert bp.validate()
    host = np.zeros(bp.host_bytes, dtype=np.uint8)
    bp.fill(host, srcs)
    buf = torch.from_numpy(host).to(dev)
    work = torch.empty(bp.work_bytes, dtype=torch.uint8, device=dev)
    out = torch.zeros(B, S, S, 3, dtype=torch.uint8, device=dev)
    base = buf.data_ptr()

    def batched():
        _lib.check(resample._launch_batch(bp, base + bp.pool_at, base + bp.tables_at, base, _lib.ptr(work), _lib.ptr(out), bp.pool_bytes,
                                          bp.work_bytes, out.numel()), "batch")

    b_ms = events(batched, a.warmup, a.iters)
    assert torch.equal(out.cpu(), want), "the batched kernels do not reproduce Pillow"
    # per image: the same stages through the single-image entry point (bounds rebased to the window each stage holds)
    jobs, keep, out1 = [], [], torch.zeros(B, S, S, 3, dtype=torch.uint8, device=dev)
    rebased = {}

    def rebase(t, org):
        key = (id(t), org)
        if key not in rebased:
            b = t.bounds.copy()
            b[:, 0] -= org
            rebased[key] = resample.Tables(t.coeffs, b, t.ksize)
        return rebased[key]

    for i, (p, src) in enumerate(zip(plans, srcs)):
        cur = torch.from_numpy(src).to(dev).reshape(-1)
        for s, st in enumerate(p.stages):
            tx, ty = rebase(st.tx, st.ox), rebase(st.ty, st.oy)
            y0, y1 = ty.rows()
            wo, ho = tx.bounds.shape[0], ty.bounds.shape[0]
            tmp = torch.empty((y1 - y0) * wo * 3, dtype=torch.uint8, device=dev)
            dst = out1[i].view(-1) if s == len(p.stages) - 1 else torch.empty(ho * wo * 3, dtype=torch.uint8, device=dev)
            (kx, bx), (ky, by) = tx.device(dev), ty.device(dev)
            keep.append((cur, tmp, dst))
            jobs.append((_lib.ptr(cur), st.in_h, st.in_w, _lib.ptr(kx), _lib.ptr(bx), tx.ksize, _lib.ptr(ky), _lib.ptr(by), ty.ksize, wo, ho,
                         _lib.ptr(tmp), tmp.numel(), _lib.ptr(dst)))
            cur = dst
    L = _lib.lib()

    def per_image():                                  # (the entry point itself: the wrapper's host checks are not part of what is timed)
        stream = _lib.stream_ptr()
        for job in jobs:
            _lib.check(L.sfron_image_resample_u8(*job, stream), "single")

    p_ms = events(per_image, a.warmup, a.iters)
    assert torch.equal(out1.cpu(), want), "the single-image kernels do not reproduce Pillow"
    # the whole call, and Pillow
    got = [None]

    def whole():
        got[0] = resample.center_crop_gpu(srcs, S, device=dev)

    g_ms = wall(whole, a.warmup, a.iters, torch.cuda.synchronize)
    assert torch.equal(got[0].cpu(), want)
    pil = [Image.fromarray(s) for s in srcs]
    h_ms = wall(lambda: [latents.center_crop_arr(im, S) for im in pil], 1, max(3, a.iters // 2), lambda: None)
    return {"batched_ms": round(b_ms, 4), "per_image_ms": round(p_ms, 4), "center_crop_gpu_ms": round(g_ms, 4), "pillow_one_thread_ms": round(h_ms, 4),
            "launches_batched": bp.n_levels, "launches_per_image": 2 * len(jobs), "source_MB": round(bp.pool_bytes / 1e6, 2),
            "work_MB": round(bp.work_bytes / 1e6, 2), "equal_to_pillow": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--limit", type=int, default=240, help="seconds each batch's process may take")
    ap.add_argument("--only", choices=sorted(BATCHES))
    a = ap.parse_args()
    if a.only:
        print(json.dumps({a.only: run_batch(a.only, a)}))
        return
    out = {"metric": f"center_crop_arr of {a.batch} images to {a.size} px, ms per batch", "iters": a.iters, "warmup": a.warmup}
    print(f"{'batch':>10} {'launches':>9} {'batched':>9} {'per image':>10} {'center_crop_gpu':>16} {'Pillow 1 thread':>16}   (ms per batch, medians)")
    for name in BATCHES:
        cmd = [sys.executable, os.path.abspath(__file__), "--only", name, "--iters", str(a.iters), "--warmup", str(a.warmup), "--batch", str(a.batch),
               "--size", str(a.size)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)      # a fresh process, its own time limit
        except subprocess.TimeoutExpired:
            sys.exit(f"batch {name!r} ran into its limit of {a.limit} s: nothing further is started")
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"batch {name!r} ended with status {r.returncode}: nothing further is started")
        v = json.loads(r.stdout.strip().splitlines()[-1])[name]
        out[name] = v
        print(f"{name:>10} {v['launches_batched']:>3} / {v['launches_per_image']:<4} {v['batched_ms']:>9.4f} {v['per_image_ms']:>10.4f} "
              f"{v['center_crop_gpu_ms']:>16.4f} {v['pillow_one_thread_ms']:>16.4f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
