#!/usr/bin/env python3
"""fp8 weight gradients (DiTSFRon(fp8_wgrad=True)), one process, same box: SFR-on steps of DiT-XL/2 or DiT-B/4 for four legs -- bf16, fp8 forward,
fp8 forward + dgrads, fp8 forward + dgrads + weight gradients -- in alternating rounds; prints per-leg median / spread of the step time, then
HIP-event times of the four block weight gradients alone (bf16 k_gemm_pipe against sfron_fp8_wgrad) and of the transposing MX casts of their
two operands.
    python tools/bench_fp8_wgrad.py --model DiT-XL/2 --batch 32 --rounds 3 --steps 8 --warmup 3"""
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


def event_us(fn, reps=20):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def kernel_times(M, D, F):
    """dW[N][K] = dY[M][N]^T X[M][K] for qkv, proj, fc1, fc2: bf16 weight-gradient GEMM, the two casts, the fp8 GEMM.  Each is the mean of 20
    back-to-back repeats of one launch on the same operands: warm caches and nothing beside it (in the step the weight gradients share the
    CUs with the dgrad chain)"""
    from sfron import _lib as L
    lib, s, dev = L.lib(), L.stream_ptr(), "cuda"
    res = {}
    for name, N, K in (("qkv", 3 * D, D), ("proj", D, D), ("fc1", F, D), ("fc2", D, F)):
        dy = (torch.randn(M, N, device=dev) * 0.1).to(torch.bfloat16)
        x = torch.randn(M, K, device=dev).to(torch.bfloat16)
        C = torch.empty(N, K, dtype=torch.float32, device=dev)
        g = L.GemmDesc()
        g.A, g.B, g.M, g.N, g.K, g.lda, g.ldb, g.a_transposed, g.b_transposed = L.ptr(dy), L.ptr(x), N, K, M, N, K, 1, 1
        g.epilogue, g.alpha, g.c_f32, g.ldc_f32, g.tokens, g.split_k = L.EPI_F32, 1.0, L.ptr(C), K, 1, 1
        qa, sa = torch.empty(N, M, dtype=torch.uint8, device=dev), torch.empty(N, M // 32, dtype=torch.uint8, device=dev)
        qb, sb = torch.empty(K, M, dtype=torch.uint8, device=dev), torch.empty(K, M // 32, dtype=torch.uint8, device=dev)
        d = L.Fp8WgradDesc()
        d.A, d.a_scales, d.B, d.b_scales, d.N, d.K, d.M, d.c_f32, d.ldc = L.ptr(qa), L.ptr(sa), L.ptr(qb), L.ptr(sb), N, K, M, L.ptr(C), K
        assert lib.sfron_gemm_bf16(ctypes.byref(g), s) == 0
        assert lib.sfron_cast_mx8_t(L.ptr(dy), M, N, L.ptr(qa), L.ptr(sa), s) == 0
        assert lib.sfron_cast_mx8_t(L.ptr(x), M, K, L.ptr(qb), L.ptr(sb), s) == 0
        assert lib.sfron_fp8_wgrad(ctypes.byref(d), s) == 0
        res[f"wgrad {name} {N}x{K} over {M} bf16"] = event_us(lambda: lib.sfron_gemm_bf16(ctypes.byref(g), s))
        res[f"wgrad {name} {N}x{K} over {M} fp8"] = event_us(lambda: lib.sfron_fp8_wgrad(ctypes.byref(d), s))
        res[f"cast_mx8_t {name} dY [{M}x{N}]"] = event_us(lambda: lib.sfron_cast_mx8_t(L.ptr(dy), M, N, L.ptr(qa), L.ptr(sa), s))
        res[f"cast_mx8_t {name} X [{M}x{K}]"] = event_us(lambda: lib.sfron_cast_mx8_t(L.ptr(x), M, K, L.ptr(qb), L.ptr(sb), s))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="DiT-XL/2", choices=["DiT-XL/2", "DiT-B/4"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from sfron import data, diffusion, dit, step
    dev = "cuda"
    torch.manual_seed(0)
    model = dit.DiT_models[a.model](input_size=32, num_classes=1000, batch_size=a.batch)
    dit.randomize_zero_init(model, std=0.02, seed=1)
    diff = diffusion.create_diffusion("", device=dev)
    kw = dict(lr=1e-4, forget_alpha=1e-3, grad_clip=1.0, ema_decay=0.9999, mask=None, unlearn_loss="ga", forget_class=207)
    batches = [(data.synthetic_batch(0, i, "forget", a.batch, device=dev), data.synthetic_batch(0, i, "remain", a.batch, device=dev))
               for i in range(2)]
    legs = {"bf16": {}, "fp8 fwd": dict(fp8=True), "fp8 fwd+dgrad": dict(fp8=True, fp8_backward=True),
            "fp8 all three": dict(fp8=True, fp8_backward=True, fp8_wgrad=True)}
    times = {k: [] for k in legs}
    for r in range(a.rounds):
        for leg, flags in legs.items():
            eng = model.engine
            eng.disable_fp8_backward()
            if flags.get("fp8"):
                eng.enable_fp8(backward=flags.get("fp8_backward", False))
            else:
                eng.fp8 = None
            runner = step.DiTSFRon(model, diff, **flags, **kw)
            t = step_times(runner, batches, a.steps, a.warmup)
            runner.sync_sweep()
            times[leg].append(statistics.median(t))
            print(f"round {r} {leg:14s} median {statistics.median(t):7.2f} ms  (min {min(t):.2f} max {max(t):.2f})", flush=True)
    for leg, v in times.items():
        print(f"{leg:14s} per-round medians {' '.join(f'{x:.2f}' for x in v)}  -> {statistics.median(v):.2f} ms (spread {max(v) - min(v):.2f})")
    c = model.engine.cfg
    for k, v in kernel_times(a.batch * model.engine.tokens, c.hidden, c.mlp_hidden).items():
        print(f"{k:44s} {v:8.1f} us")


if __name__ == "__main__":
    main()
