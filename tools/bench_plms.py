#!/usr/bin/env python3
"""ms per guided, steady-state (fourth-order) PLMS step of the SD v1 UNet (random weights, 512 px = 64x64 latents, 77-token context) at
batch 2 x B, in three modes that share the UNet call (PreparedContext + fused cross-attention, what the samplers run):
  plms    PLMSSampler.p_sample_plms: the UNet call + ONE launch of sfron_plms_cfg_step over the three-slot history ring
  torch   the same UNet call + the reference's update written as torch ops on the device (chunk, guidance mix, the 55/-59/37/-9
          combination, the per-step scalar tensors, pred_x0, x_prev): what a user without the kernel would run
  ddim    DDIMSampler.p_sample_ddim (UNet call + sfron_ddim_cfg_step): the per-step price PLMS is paired against
Every mode is measured --repeat times, the modes taking turns; the line carries each mode's minimum and its spread (max - min).  From the
minima it also prices one image at the usual pairing: PLMS 50 steps (51 UNet calls) against DDIM 100 steps.
    python tools/bench_plms.py [--batches 1,4,10] [--steps 20] [--repeat 5] [--mode all|plms|torch|ddim]
One process per GPU step is the caller's business: run it under `timeout`."""
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
from sfron import ddim, plms, sd, sd_unet  # noqa: E402

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
ldm = sd.LatentDiffusion(model)
SCALE, INDEX = 7.5, 25


def step_ms(B, mode):
    gd = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(B, 4, 64, 64, device=DEV, generator=gd)
    cond, uc = torch.randn(B, 77, 768, device=DEV, generator=gd), torch.randn(B, 77, 768, device=DEV, generator=gd)
    ring = torch.randn(3, B, 4, 64, 64, device=DEV, generator=gd)
    s = ddim.DDIMSampler(ldm) if mode == "ddim" else plms.PLMSSampler(ldm)
    s.make_schedule(50, verbose=False)
    ts = torch.full((B,), int(s.ddim_timesteps[INDEX]), device=DEV, dtype=torch.long)
    kw = dict(index=INDEX, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc)
    old = [ring[0], ring[1], ring[2]]
    with torch.no_grad(), s._conditioning(cond, uc, SCALE) as c_in:
        def one(x):
            if mode == "ddim":
                return s.p_sample_ddim(x, cond, ts, _c_in=c_in, **kw)[0]
            if mode == "plms":
                x_prev, _, e_t = s.p_sample_plms(x, cond, ts, old_eps=old, t_next=ts, _c_in=c_in, _ring=ring, **kw)
            else:
                e_u, e_t = ldm.apply_model(torch.cat([x] * 2), torch.cat([ts] * 2), c_in).chunk(2)
                e_t = e_u + SCALE * (e_t - e_u)
                e_p = (55 * e_t - 59 * old[-1] + 37 * old[-2] - 9 * old[-3]) / 24
                a_t = torch.full((B, 1, 1, 1), float(s.ddim_alphas[INDEX]), device=DEV)
                a_prev = torch.full((B, 1, 1, 1), float(s.ddim_alphas_prev[INDEX]), device=DEV)
                sigma_t = torch.full((B, 1, 1, 1), float(s.ddim_sigmas[INDEX]), device=DEV)
                sqrt_1m = torch.full((B, 1, 1, 1), float(s.ddim_sqrt_one_minus_alphas[INDEX]), device=DEV)
                pred_x0 = (x - sqrt_1m * e_p) / a_t.sqrt()
                x_prev = a_prev.sqrt() * pred_x0 + (1.0 - a_prev - sigma_t ** 2).sqrt() * e_p
            old.append(e_t)
            old.pop(0)
            return x_prev
        for _ in range(a.warmup):
            one(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            one(x)                       # the same input every step: the time does not depend on the values
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return dt / a.steps * 1e3


MODES = ("plms", "torch", "ddim")
for B in (int(v) for v in a.batches.split(",")):
    res = {"batch": B, "latent": 64, "steps": a.steps, "repeat": a.repeat}
    names = [n for n in MODES if a.mode in ("all", n)]
    ms = {n: [] for n in names}
    for _ in range(a.repeat):                # the modes take turns, so a drift of the machine falls on all of them alike
        for n in names:
            ms[n].append(step_ms(B, n))
    for n in names:
        res[n + "_ms"] = round(min(ms[n]), 3)
        res[n + "_spread_ms"] = round(max(ms[n]) - min(ms[n]), 3)
    if "plms" in ms and "ddim" in ms:
        res["plms50_s_per_image"] = round(min(ms["plms"]) * 51 / B / 1e3, 3)
        res["ddim100_s_per_image"] = round(min(ms["ddim"]) * 100 / B / 1e3, 3)
    print("SD-PLMS-STEP " + json.dumps(res), flush=True)
