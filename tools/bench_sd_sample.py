#!/usr/bin/env python3
"""ms per guided DDIM step of the SD v1 UNet (random weights, 512 px = 64x64 latents, 77-token context) at batch 2 x B, in four modes:
  parent    plain no-grad forward + guidance mix on the host + sfron_ddim_step (the means the project had before sfron.ddim)
  prepared  PreparedContext only (the attn2 key / value GEMMs leave the loop), update in sfron_ddim_cfg_step
  fused     fused cross-attention only (sfron_xattn_fwd)
  both      PreparedContext + fused cross-attention: what DDIMSampler.sample runs
Every mode is measured --repeat times, the modes taking turns; the line carries each mode's minimum and its spread (max - min), and the
spread of `parent` is the run-to-run margin the other modes are read against.
    python tools/bench_sd_sample.py [--batches 1,4,10] [--steps 20] [--repeat 5] [--mode all|parent|prepared|fused|both]
One process per GPU step is the caller's business: run it under `timeout`, and for the kernel table of the last mode
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/bench_sd_sample.py --batches 10 --mode both --steps 3 --repeat 1"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,4,10")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--mode", default="all")
a = ap.parse_args()
import sfron  # noqa: E402,F401
from sfron import _lib, sd_unet  # noqa: E402
from sfron._lib import check, ptr, stream_ptr  # noqa: E402

DEV = "cuda"
torch.manual_seed(0)
model = sd_unet.UNetModel()
g = torch.Generator().manual_seed(1)
with torch.no_grad():
    for p in model.parameters():
        if not bool(p.any()):
            p.copy_((torch.randn(p.shape, generator=g) * 0.02).to(p.device))
model.sync_bf16()
model.eval()
L = _lib.lib()
S1, S2, S3, DIR = 0.6 ** 0.5, 0.4 ** 0.5, 0.55 ** 0.5, 0.45 ** 0.5
SCALE = 7.5


def step_ms(B, prepared, fused, parent_update):
    gd = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(B, 4, 64, 64, device=DEV, generator=gd)
    ctx = torch.randn(2 * B, 77, 768, device=DEV, generator=gd)
    t = torch.full((2 * B,), 500, device=DEV, dtype=torch.long)
    model.fused_cross_attention = fused
    with torch.no_grad():
        c_in = model.prepare_context(ctx) if prepared else ctx

        def one(x):
            out = model(torch.cat([x] * 2), timesteps=t, context=c_in)
            nxt = torch.empty_like(x)
            if parent_update:
                eu, ec = out.chunk(2)
                e = (eu + SCALE * (ec - eu)).contiguous()
                check(L.sfron_ddim_step(ptr(x), ptr(e), None, x.numel(), S1, S2, S3, 0.0, DIR, ptr(nxt), None, stream_ptr()), "ddim_step")
            else:
                half = out.element_size() * (out.numel() // 2)
                check(L.sfron_ddim_cfg_step(ptr(x), out.data_ptr(), out.data_ptr() + half, None, x.numel(), SCALE, S1, S2, S3, DIR, 0.0, ptr(nxt),
                                            None, stream_ptr()), "ddim_cfg_step")
            return nxt
        for _ in range(a.warmup):
            one(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            one(x)                       # the same input every step: the time does not depend on the values
        torch.cuda.synchronize()
    model.fused_cross_attention = False
    return (time.perf_counter() - t0) / a.steps * 1e3


MODES = {"parent": (False, False, True), "prepared": (True, False, False), "fused": (False, True, False), "both": (True, True, False)}
for B in (int(v) for v in a.batches.split(",")):
    res = {"batch": B, "latent": 64, "steps": a.steps, "repeat": a.repeat}
    names = [n for n in MODES if a.mode in ("all", n)]
    ms = {n: [] for n in names}
    for _ in range(a.repeat):                # the modes take turns, so a drift of the machine falls on all of them alike
        for n in names:
            ms[n].append(step_ms(B, *MODES[n]))
    for n in names:
        res[n + "_ms"] = round(min(ms[n]), 2)
        res[n + "_spread_ms"] = round(max(ms[n]) - min(ms[n]), 2)
    print("SD-SAMPLE-STEP " + json.dumps(res), flush=True)
