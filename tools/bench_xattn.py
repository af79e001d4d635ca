#!/usr/bin/env python3
"""The fused differentiable cross-attention (sfron_xattn_fwd_lse + sfron_xattn_bwd) against the UNetModel._mha forward + backward launch
sequence it replaces (two batched GEMMs + softmax forward; five batched GEMMs + softmax backward), at SD v1's four attention levels:
N = 4096 / 1024 / 256 / 64 with head widths 40 / 80 / 160 / 160, 8 heads, 77 context tokens padded to 80, batch 2 and 8.
HIP events, median of 20 after 3 warm-ups.
    python tools/bench_xattn.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from sfron import _lib, sd_unet
from sfron._lib import check, stream_ptr

DEV = "cuda"
assert torch.cuda.is_available(), "bench_xattn needs a GPU"


def timed(fn, warm=3, reps=20):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[-1] - ts[0]


class Host:                                            # what UNetModel._mha / _fused_cross_attention_train read of the model
    def __init__(self, heads):
        self.heads, self.device_ = heads, torch.device(DEV)
    _mha = sd_unet.UNetModel._mha
    _fused_cross_attention_train = sd_unet.UNetModel._fused_cross_attention_train


H, Lv, Lp = 8, 77, 80
print("level  B     N   hd | _mha fwd+bwd us (spread) | fused fwd+bwd us (spread) | difference us")
for B in (2, 8):
    for N, hd in ((4096, 40), (1024, 80), (256, 160), (64, 160)):
        C = H * hd
        g = torch.Generator(device=DEV).manual_seed(N + B)
        q2 = (torch.randn(B * N, C, device=DEV, generator=g) * 1.5).to(torch.bfloat16)
        kv = (torch.randn(B * Lp, 2 * C, device=DEV, generator=g) * 1.2).to(torch.bfloat16)
        dO = torch.randn(B * N, C, device=DEV, generator=g).to(torch.bfloat16)
        dq, dkv = torch.empty_like(q2), torch.empty_like(kv)
        m = Host(H)

        def unfused():
            O, bwd = m._mha(q2.data_ptr(), C, kv.data_ptr(), 2 * C, kv.data_ptr() + 2 * C, 2 * C, B, N, Lp, Lv, C, keep=(q2, kv))
            bwd(dO, dq.data_ptr(), dkv.data_ptr(), dkv.data_ptr() + 2 * C)

        def fused():
            O, bwd = m._fused_cross_attention_train(q2, kv, B, N, Lp, Lv, C)
            bwd(dO, dq.data_ptr(), dkv.data_ptr(), dkv.data_ptr() + 2 * C)
        (tu, su), (tf, sf) = timed(unfused), timed(fused)
        print(f"       {B}  {N:4d}  {hd:3d} | {tu:10.1f} ({su:6.1f})      | {tf:10.1f} ({sf:6.1f})       | {tf - tu:+9.1f}")
