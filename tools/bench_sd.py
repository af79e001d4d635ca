#!/usr/bin/env python3
"""BASELINE config 4 on the HIP path: SD v1 UNet nsfw_removal SFR-on iterations/s (batch 2, 64x64 latents, 77-token context).
    python tools/bench_sd.py [--steps 5] [--batch 2] [--method full|xattn]
    python tools/bench_sd.py --fused-xattn [--batch 8] [--steps 5]     both train methods, SDSFRon(fused_xattn=False) and (fused_xattn=True) taking turns
                                                                      in one process, five rounds: minimum and spread of each
    python tools/bench_sd.py --fused-wide-attn [--batch 8]             the same A-B of SDSFRon(fused_wide_attn=...) (csrc/wattn.hip)"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
ap = argparse.ArgumentParser(); ap.add_argument("--steps", type=int, default=5); ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--method", default="full")
ap.add_argument("--eager", action="store_true", help="no HIP-graph replay of the stages")
ap.add_argument("--fused-xattn", action="store_true", help="A-B of the fused differentiable cross-attention (flag off = the default path)")
ap.add_argument("--fused-wide-attn", action="store_true", help="A-B of the fused wide-head self-attention (flag off = the default path)")
a = ap.parse_args()
AB = ("fused_xattn", "fused_cross_attention_train") if a.fused_xattn else ("fused_wide_attn", "fused_wide_self_attention") if a.fused_wide_attn else None
from sfron import sd, sd_unet
if os.environ.get("SFRON_FUSE_SPLIT_FINISH"):       # A-B knob: 0 = every split convolution finishes its own output (before round 6, late)
    from sfron import unet as _u2; _u2._TapeNet.FUSE_SPLIT_FINISH = os.environ["SFRON_FUSE_SPLIT_FINISH"] != "0"
if os.environ.get("SFRON_BATCH_REDUCTIONS"):        # A-B knob: 0 = every parameter-gradient finish as its own launch (before round 6)
    from sfron import unet as _u; _u._TapeNet.BATCH_REDUCTIONS = os.environ["SFRON_BATCH_REDUCTIONS"] != "0"
if os.environ.get("SFRON_LOADER_WAVES"):            # A-B knob: 10 = convolution tiles in the shared-wave form
    from sfron import _lib as _L; _L.lib().sfron_gemm_loader_waves(int(os.environ["SFRON_LOADER_WAVES"]))
DEV = "cuda"
torch.manual_seed(0)
model = sd_unet.UNetModel()
g = torch.Generator().manual_seed(1)
with torch.no_grad():
    for p in model.parameters():
        if not bool(p.any()):
            p.copy_((torch.randn(p.shape, generator=g) * 0.02).to(p.device))
model.sync_bf16()
B = a.batch if not (AB and a.batch == 2) else 8
gd = torch.Generator(device=DEV).manual_seed(2)
rn = lambda *s: torch.randn(*s, device=DEV, generator=gd)
c_f, c_p = rn(1, 77, 768).expand(B, -1, -1).contiguous(), rn(1, 77, 768).expand(B, -1, -1).contiguous()
def batch():
    xf = rn(B, 4, 64, 64)
    return (dict(x_f=xf, x_p=xf, c_f=c_f, c_p=c_p, t=torch.randint(0, 1000, (B,), device=DEV, generator=gd), noise=rn(B, 4, 64, 64)),
            dict(x=rn(B, 4, 64, 64), c=c_p, t=torch.randint(0, 1000, (B,), device=DEV, generator=gd), noise=rn(B, 4, 64, 64)))
bts = [batch() for _ in range(2)]
if AB:
    # one model, one runner per mode (each with its own graphs); the switch is read when a stage is run eagerly or captured
    for method in ("full", "xattn"):
        runs = {}
        for on in (False, True):
            setattr(model, AB[1], False)
            runs[on] = sd.SDSFRon(model, lr=1e-5, train_method=method, use_graphs=not a.eager, **{AB[0]: on})
        times = {False: [], True: []}
        for rnd in range(6):                           # round 0 warms up (and captures)
            for on in (False, True):
                setattr(model, AB[1], on)
                torch.cuda.synchronize(); t0 = time.time()
                for i in range(a.steps): runs[on].step(*bts[i % 2])
                torch.cuda.synchronize()
                if rnd:
                    times[on].append((time.time() - t0) / a.steps * 1e3)
        off, on = times[False], times[True]
        print(f"SD v1 SFR-on iteration, batch {B}, train_method {method}: flag off min {min(off):.1f} ms (spread {max(off) - min(off):.1f}), "
              f"{AB[0]} min {min(on):.1f} ms (spread {max(on) - min(on):.1f}), difference {min(on) - min(off):+.1f} ms")
        del runs
    sys.exit(0)
run = sd.SDSFRon(model, lr=1e-5, train_method=a.method, use_graphs=not a.eager)
for i in range(2): run.step(*bts[i % 2])
torch.cuda.synchronize(); t0 = time.time()
for i in range(a.steps): run.step(*bts[i % 2])
torch.cuda.synchronize(); dt = (time.time() - t0) / a.steps
t1 = time.time()
for i in range(2): run.step(*bts[i % 2])
host = (time.time() - t1) / 2
print(f"SD v1 UNet SFR-on iteration, batch {B}, train_method {a.method}, {'eager' if a.eager else 'graph replay'}: {dt * 1e3:.0f} ms = {1 / dt:.2f} it/s (host enqueue {host * 1e3:.0f} ms)")
