#!/usr/bin/env python3
"""The fused wide-head self-attention (sfron_wattn_fwd, sfron_wattn_bwd; csrc/wattn.hip) against the launch sequence it replaces -- two
batched GEMMs + softmax forward, five batched GEMMs + softmax backward, scores and probabilities through HBM (UNetModel._mha; with one head
the launches of Conditional_Model._attn) -- forward alone and forward + backward, at
    the DDPM AttnBlock of BASELINE config 1:  B 64, H 1, T 256, hd 256
    SD v1's 16x16 level:                      B 8 and 20, H 8, T 256, hd 160
    SD v1's 8x8 level and middle block:       B 8 and 20, H 8, T 64, hd 160
HIP events, median of 20 after 3 warm-ups, spread = max - min.  Random operands (qkv 1.0 randn), both sides on the same tensors.
    python tools/bench_wattn.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from sfron import sd_unet

DEV = "cuda"
assert torch.cuda.is_available(), "bench_wattn needs a GPU"


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


class Host:                                            # what UNetModel._mha / _wide_self_attention read of the model
    def __init__(self, heads):
        self.heads, self.device_ = heads, torch.device(DEV)
    _mha = sd_unet.UNetModel._mha
    _wide_self_attention = sd_unet.UNetModel._wide_self_attention


print("    B  H     T   hd | old fwd us (spread) | fused fwd us (spread) | old fwd+bwd us (spread) | fused fwd+bwd us (spread) | difference fwd / fwd+bwd us")
for B, H, T, hd in ((64, 1, 256, 256), (8, 8, 256, 160), (20, 8, 256, 160), (8, 8, 64, 160), (20, 8, 64, 160)):
    C = H * hd
    g = torch.Generator(device=DEV).manual_seed(T + B)
    qkv = torch.randn(B * T, 3 * C, device=DEV, generator=g).to(torch.bfloat16)
    dO = (torch.randn(B * T, C, device=DEV, generator=g) * 0.2).to(torch.bfloat16)
    dqkv = torch.empty_like(qkv)
    m = Host(H)
    p, d = qkv.data_ptr(), dqkv.data_ptr()

    def old(back):
        O, bwd = m._mha(p, 3 * C, p + 2 * C, 3 * C, p + 4 * C, 3 * C, B, T, T, T, C, keep=(qkv,))
        if back:
            bwd(dO, d, d + 2 * C, d + 4 * C)

    def fused(back):
        O, bwd = m._wide_self_attention(qkv, B, T, C, back)
        assert O is not None
        if back:
            bwd(dO, d, d + 2 * C, d + 4 * C)
    (of, osf), (ff, fsf) = timed(lambda: old(False)), timed(lambda: fused(False))
    (ob, osb), (fb, fsb) = timed(lambda: old(True)), timed(lambda: fused(True))
    print(f"   {B:2d}  {H}  {T:4d}  {hd:3d} | {of:8.1f} ({osf:6.1f})   | {ff:8.1f} ({fsf:6.1f})     | {ob:10.1f} ({osb:6.1f})     | {fb:10.1f} ({fsb:6.1f})       "
          f"| {ff - of:+8.1f} / {fb - ob:+8.1f}")
