#!/usr/bin/env python3
"""ms per guided sampling step of the DDPM U-Net of cifar10_sfron.yml (random weights, 32 px), cond_scale 2, eta 0, in four modes:
  parent  ddpm.generalized_steps_conditional over model(mode="test"): two forward passes at batch B, sfron_axpby, sfron_ddim_step
  parent_prepped  the same loop with the convolution operands laid ONCE per run (model.auto_prep off), as DDPMSampler does: what is
          left between this column and `eager` is the pair forward and the fused update, not the hoisted re-layout
  eager   ddpm.DDPMSampler: one forward pass at batch 2B (forward_pair), sfron_ddpm_guided_step, sfron_ddpm_sampler_advance
  graph   ddpm.DDPMSampler(graph=True): the same step captured once and replayed
Each round is one whole run of --steps sampling steps, timed from the call to the synchronised end (so a round of `parent` and `eager`
holds its host work, and a round of `graph` the eager copy-in and the replays).  Every mode is measured --repeat times after one
untimed run (which also captures the graph), the modes taking turns; the line carries each mode's minimum and its spread (max - min),
and the spread of `parent` is the run-to-run margin the other modes are read against.
    python tools/bench_ddpm_sample.py [--batches 128,16] [--steps 50] [--repeat 5] [--mode all|parent|parent_prepped|eager|graph]
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
ap.add_argument("--batches", default="128,16")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--mode", default="all")
a = ap.parse_args()
import sfron  # noqa: E402,F401
from sfron import ddpm, unet  # noqa: E402

DEV = "cuda"
SCALE = 2.0
torch.manual_seed(0)
model = unet.Conditional_Model()                 # the keyword defaults are cifar10_sfron.yml's model
model.eval()
betas = ddpm.get_beta_schedule(device=DEV)
if 1000 % a.steps:
    raise SystemExit("--steps must divide 1000 (the uniform sequence then has exactly that many entries)")
seq = ddpm.sampling_sequence("uniform", 1000, a.steps)


def run_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / a.steps * 1e3


def parent_prepped(x, c):
    model._prep_conv_weights()
    model.auto_prep = False
    try:
        return ddpm.generalized_steps_conditional(x, c, seq, model, betas, cond_scale=SCALE, eta=0.0)
    finally:
        model.auto_prep = True


for B in (int(v) for v in a.batches.split(",")):
    gd = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(B, 3, 32, 32, device=DEV, generator=gd)
    c = torch.randint(0, 10, (B,), device=DEV, generator=gd)
    samplers = {g: ddpm.DDPMSampler(model, betas, timesteps=a.steps, eta=0.0, graph=g) for g in (False, True)}
    modes = {"parent": lambda: ddpm.generalized_steps_conditional(x, c, seq, model, betas, cond_scale=SCALE, eta=0.0),
             "parent_prepped": lambda: parent_prepped(x, c),
             "eager": lambda: samplers[False].sample_image(x, c, SCALE),
             "graph": lambda: samplers[True].sample_image(x, c, SCALE)}
    names = [n for n in modes if a.mode in ("all", n)]
    with torch.no_grad():
        for n in names:
            modes[n]()                               # untimed: lazily sized scratch, and the capture
        ms = {n: [] for n in names}
        for _ in range(a.repeat):                    # the modes take turns, so a drift of the machine falls on all of them alike
            for n in names:
                ms[n].append(run_ms(modes[n]))
    res = {"batch": B, "image": 32, "steps": a.steps, "repeat": a.repeat, "cond_scale": SCALE}
    for n in names:
        res[n + "_ms"] = round(min(ms[n]), 3)
        res[n + "_spread_ms"] = round(max(ms[n]) - min(ms[n]), 3)
    print("DDPM-SAMPLE-STEP " + json.dumps(res), flush=True)
    del samplers, modes
