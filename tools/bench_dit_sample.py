#!/usr/bin/env python3
"""ms per guided sampling step of a DiT (random weights, clip_denoised=False), three arms per shape:
  parent  diffusion.p_sample_loop(model.forward_with_cfg, ...): per step a torch.cat of the state, a host-built timestep tensor, two
          .float() copies, sfron_cfg_combine, sfron_p_sample over all 2n rows
  ddpm    dit_sample.DiTSampler(mode="ddpm"): one forward pass from persistent buffers, sfron_dit_sample_step, sfron_dit_sampler_advance
  ddim    dit_sample.DiTSampler(mode="ddim", eta=0): the same loop with the DDIM update (no noise draw)
Shapes: DiT-XL/2 at 256 px with n = 32 at cfg 1.5 (engine batch 64) and n = 8 at cfg 4.0, DiT-B/4 at 256 px with n = 32 at cfg 1.5.
Each round is one whole run of --steps respaced steps between two events recorded on the sampler's stream (the current stream), so a
round holds its host gaps.  Every arm is measured --repeat times after one untimed run (lazily sized scratch, the allocator's first
requests, the engine a DiTSampler builds once and keeps), the arms taking turns so that a drift of the
machine falls on all of them alike; the line carries each arm's minimum and its spread (max - min).  The spread of `parent` is the
run-to-run margin the native arms are read against.
    python tools/bench_dit_sample.py [--shapes xl2_n32,xl2_n8,b4_n32] [--steps 10] [--repeat 5]
One process per GPU step is the caller's business: run it under `timeout`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

SHAPES = {"xl2_n32": ("DiT-XL/2", 32, 1.5), "xl2_n8": ("DiT-XL/2", 8, 4.0), "b4_n32": ("DiT-B/4", 32, 1.5)}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=",".join(SHAPES))
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--repeat", type=int, default=5)
a = ap.parse_args()
import sfron  # noqa: E402,F401
from sfron import diffusion, dit, dit_sample  # noqa: E402

DEV = "cuda"
LATENT = 32                                          # 256 px


def run_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.steps


diff = diffusion.create_diffusion(str(a.steps), device=DEV)
models = {}
for shape in a.shapes.split(","):
    name, n, cfg = SHAPES[shape]
    if name not in models:
        models.clear()                               # one model resident at a time
        torch.manual_seed(0)
        m = dit.DiT_models[name](input_size=LATENT, num_classes=1000, batch_size=2 * n)
        dit.randomize_zero_init(m, std=0.02, seed=1)
        m.eval()
        models[name] = m
    model = models[name]
    g = torch.Generator(device=DEV).manual_seed(2)
    z = torch.randn(n, 4, LATENT, LATENT, device=DEV, generator=g)
    y = torch.randint(0, 1000, (n,), device=DEV, generator=g)
    zc, yc = torch.cat([z, z], 0), torch.cat([y, torch.full((n,), 1000, device=DEV)], 0)
    samplers = {k: dit_sample.DiTSampler(model, diff, cfg, mode=k, eta=0.0, clip_denoised=False) for k in ("ddpm", "ddim")}
    arms = {"parent": lambda: diff.p_sample_loop(model.forward_with_cfg, zc.shape, zc, clip_denoised=False,
                                                 model_kwargs=dict(y=yc, cfg_scale=cfg), device=DEV),
            "ddpm": lambda: samplers["ddpm"].sample(z, y),
            "ddim": lambda: samplers["ddim"].sample(z, y)}
    with torch.no_grad():
        for k in arms:
            arms[k]()                                # untimed warm-up run
        ms = {k: [] for k in arms}
        for _ in range(a.repeat):
            for k in arms:
                ms[k].append(run_ms(arms[k]))
    res = {"shape": shape, "model": name, "n": n, "engine_batch": 2 * n, "cfg_scale": cfg, "steps": a.steps, "repeat": a.repeat}
    for k in arms:
        res[k + "_ms"] = round(min(ms[k]), 3)
        res[k + "_spread_ms"] = round(max(ms[k]) - min(ms[k]), 3)
    print("DIT-SAMPLE-STEP " + json.dumps(res), flush=True)
    del samplers, arms
