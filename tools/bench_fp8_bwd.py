#!/usr/bin/env python3
"""Config 5 with and without the fp8 backward, one process, same box: DiT-XL/2 batch 32 SFR-on steps for three modes -- bf16, fp8 forward only,
fp8 forward + backward (DiTSFRon(fp8_backward=True)) -- run in alternating rounds; prints per-mode median / spread of the step time, then
HIP-event times of block 0's four dgrads (bf16 and fp8 forms) and of the MX casts at the same shapes.
    python tools/bench_fp8_bwd.py --rounds 3 --steps 8 --warmup 3"""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def step_times(runner, batches, steps, warmup):
    for i in range(warmup):
        runner.step(*batches[i % len(batches)])
    torch.cuda.synchronize()
    out = []
    for i in range(steps):
        t0 = time.perf_counter()
        runner.step(*batches[i % len(batches)])
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def event_ms(fn, reps=20):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3            # us


def kernel_times(batch):
    from sfron import _lib as L
    lib, s = L.lib(), L.stream_ptr()
    M, D, F = batch * 256, 1152, 4608
    dev = "cuda"
    res = {}
    ws = torch.ones(1, device=dev)
    for name, N, K, epi in (("qkv", D, 3 * D, 0), ("proj", D, D, 0), ("fc1", D, F, 0), ("fc2", F, D, 8)):
        dy = (torch.randn(M, K, device=dev) * 0.1).to(torch.bfloat16)
        w = (torch.randn(K, N, device=dev) * 0.02).to(torch.bfloat16)
        q = torch.empty(M, K, dtype=torch.uint8, device=dev)
        sc = torch.empty(M, K // 32, dtype=torch.uint8, device=dev)
        res[f"cast_mx8 {name} dY [{M}x{K}]"] = event_ms(lambda: lib.sfron_cast_mx8(L.ptr(dy), M, K, L.ptr(q), L.ptr(sc), s))
        wt8 = torch.randint(0, 120, (N, K), dtype=torch.uint8, device=dev)
        C = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        d = L.Fp8DgradDesc()
        d.A, d.a_scales, d.B, d.M, d.N, d.K, d.w_scale, d.epilogue, d.c_bf16, d.ldc_bf16 = L.ptr(q), L.ptr(sc), L.ptr(wt8), M, N, K, L.ptr(ws), epi, L.ptr(C), N
        g = L.GemmDesc()
        g.A, g.B, g.M, g.N, g.K, g.lda, g.ldb, g.b_transposed, g.epilogue, g.alpha, g.c_bf16, g.ldc_bf16 = \
            L.ptr(dy), L.ptr(w), M, N, K, K, N, 1, epi, 1.0, L.ptr(C), N
        if epi:
            codes = torch.randint(0, 252, (M, N), dtype=torch.uint8, device=dev)
            c8, cs = torch.empty(M, N, dtype=torch.uint8, device=dev), torch.empty(M, N // 32, dtype=torch.uint8, device=dev)
            part = torch.empty(M // 256, N, device=dev)
            d.aux, d.ldaux, d.c_e4m3, d.c_scales, d.col_partials = L.ptr(codes), N, L.ptr(c8), L.ptr(cs), L.ptr(part)
            g.aux, g.ldaux, g.col_partials = L.ptr(codes), N, L.ptr(part)
        assert lib.sfron_fp8_dgrad(ctypes.byref(d), s) == 0 and lib.sfron_gemm_bf16(ctypes.byref(g), s) == 0
        res[f"dgrad {name} {M}x{N}x{K} fp8"] = event_ms(lambda: lib.sfron_fp8_dgrad(ctypes.byref(d), s))
        res[f"dgrad {name} {M}x{N}x{K} bf16"] = event_ms(lambda: lib.sfron_gemm_bf16(ctypes.byref(g), s))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from sfron import data, diffusion, dit, step
    dev = "cuda"
    torch.manual_seed(0)
    model = dit.DiT_models["DiT-XL/2"](input_size=32, num_classes=1000, batch_size=a.batch)
    dit.randomize_zero_init(model, std=0.02, seed=1)
    diff = diffusion.create_diffusion("", device=dev)
    kw = dict(lr=1e-4, forget_alpha=1e-3, grad_clip=1.0, ema_decay=0.9999, mask=None, unlearn_loss="ga", forget_class=207)
    batches = [(data.synthetic_batch(0, i, "forget", a.batch, device=dev), data.synthetic_batch(0, i, "remain", a.batch, device=dev))
               for i in range(2)]
    times = {"bf16": [], "fp8 fwd": [], "fp8 fwd+bwd": []}
    for r in range(a.rounds):
        for mode in times:
            eng = model.engine
            if mode == "bf16":
                eng.disable_fp8_backward()
                eng.fp8 = None
                runner = step.DiTSFRon(model, diff, **kw)
            elif mode == "fp8 fwd":
                eng.enable_fp8()
                runner = step.DiTSFRon(model, diff, fp8=True, **kw)
            else:
                eng.enable_fp8(backward=True)
                runner = step.DiTSFRon(model, diff, fp8=True, fp8_backward=True, **kw)
            t = step_times(runner, batches, a.steps, a.warmup)
            runner.sync_sweep()
            times[mode].append(statistics.median(t))
            print(f"round {r} {mode:12s} median {statistics.median(t):7.2f} ms  (min {min(t):.2f} max {max(t):.2f})", flush=True)
    for mode, v in times.items():
        print(f"{mode:12s} per-round medians {' '.join(f'{x:.2f}' for x in v)}  -> {statistics.median(v):.2f} ms (spread {max(v) - min(v):.2f})")
    for k, v in kernel_times(a.batch).items():
        print(f"{k:40s} {v:8.1f} us")


if __name__ == "__main__":
    main()
