#!/usr/bin/env python3
"""The DDPM data path, per batch: three routes from a CIFAR-shaped resident dataset to the inputs of a stage (x0, c, t), taking turns in
one process, timed with HIP events and with the host's wall clock; then a whole SFR-on iteration fed by the loader against the hand-fed
step of tools/bench_ddpm.py.
    python tools/bench_ddpm_data.py [--batches 128 64] [--iters 50] [--rounds 5] [--dequant] [--no-step] [--steps 20]

  host      the reference's shape: per image a flip draw, ToTensor on one thread, torch.stack (DataLoader's collate), the upload,
            data_transform and the antithetic t as torch ops (DDPM/runners/diffusion.py:124-135)
  torch     the same as torch ops on the resident uint8 tensor (ddpm_data.batch_torch) behind the device draws
  launch    the device draws and ONE launch (ddpm_data.ddpm_batch_u8)
The draw of e is common to all three and left out.  --dequant turns uniform dequantization on (cifar10.yml has it off)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sfron import ddpm, ddpm_data, unet  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, nargs="+", default=[128, 64])
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--dequant", action="store_true")
ap.add_argument("--no-step", action="store_true", help="skip the whole-iteration comparison")
a = ap.parse_args()
DEV, T, N = "cuda:0", 1000, 5120
torch.set_num_threads(1)                                   # the host route is one DataLoader worker's work
cfg = ddpm_data.config_with_data(unet.config_namespace(), channels=3, random_flip=True, uniform_dequantization=a.dequant,
                                 gaussian_dequantization=False, rescaled=True, logit_transform=False)
g0 = torch.Generator().manual_seed(0)
images = torch.randint(0, 256, (N, 3, 32, 32), generator=g0, dtype=torch.uint8)
labels = torch.randint(0, 10, (N,), generator=g0)
ds = ddpm_data.ResidentDataset(images, labels, device=DEV)
host_items = [(images[i], int(labels[i])) for i in range(N)]
gen = torch.Generator(device=DEV).manual_seed(1)
cpu_gen = torch.Generator().manual_seed(1)


def route_host(B):
    pick = torch.randint(0, N, (B,), generator=cpu_gen).tolist()
    xs = []
    for i in pick:
        x = host_items[i][0]
        if torch.rand(1, generator=cpu_gen) < 0.5:
            x = x.flip(-1)
        xs.append(x.float().div(255))
    x = torch.stack(xs).to(DEV)
    c = torch.tensor([host_items[i][1] for i in pick]).to(DEV)
    x = ddpm_data.data_transform(cfg, x)
    t = torch.randint(low=0, high=T, size=(B // 2 + 1,), generator=cpu_gen).to(DEV)
    return x, c, torch.cat([t, T - t - 1], dim=0)[:B]


def device_draws(B):
    idx = torch.randint(0, N, (B,), generator=gen, device=DEV)
    flip = (torch.rand(B, generator=gen, device=DEV) < 0.5).to(torch.uint8)
    u = torch.rand(B, 3, 32, 32, generator=gen, device=DEV) if a.dequant else None
    return idx, flip, u, torch.randint(0, T, (B // 2 + 1,), generator=gen, device=DEV)


def route_torch(B):
    idx, flip, u, t_half = device_draws(B)
    return ddpm_data.batch_torch(ds, idx, flip, cfg, T, u=u, t_half=t_half)


def route_launch(B):
    idx, flip, u, t_half = device_draws(B)
    return ddpm_data.ddpm_batch_u8(ds, idx, flip, cfg, T, u=u, t_half=t_half)


def timed(fn, B, iters):
    """-> (device ms per batch between two events, host wall ms per batch including the final wait)"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(iters):
        fn(B)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters, (time.perf_counter() - t0) * 1e3 / iters


def summary(v):
    return f"min {min(v):8.3f}  median {sorted(v)[len(v) // 2]:8.3f}  max {max(v):8.3f}"


routes = {"host": route_host, "torch": route_torch, "launch": route_launch}
for B in a.batches:
    res = {k: ([], []) for k in routes}
    for rnd in range(a.rounds + 1):                        # round 0 warms up
        for name, fn in routes.items():
            dev_ms, wall_ms = timed(fn, B, a.iters)
            if rnd:
                res[name][0].append(dev_ms)
                res[name][1].append(wall_ms)
    for name in routes:
        print(f"batch {B:4d} {name:7s} events ms/batch: {summary(res[name][0])} | wall ms/batch: {summary(res[name][1])}")

if not a.no_step:
    for B in a.batches:
        torch.manual_seed(1234)
        model = unet.Conditional_Model(unet.config_namespace())
        run = ddpm.DDPMSFRon(model, lr=1e-4, forget_alpha=10.0, grad_clip=1.0, ema_rate=1e-4, mask=None, unlearn_loss="adaga", lambd=0.5,
                             n_iters=50, use_graphs=True)
        forget_idx, remain_idx = torch.arange(0, N // 4), torch.arange(N // 4, N)          # multiples of both batch sizes: no short batch
        fl = ddpm_data.cycle(ddpm_data.DDPMBatchLoader(ds, forget_idx, B, cfg, T, torch.Generator(device=DEV).manual_seed(2), flip="frozen"))
        rl = ddpm_data.cycle(ddpm_data.DDPMBatchLoader(ds, remain_idx, B, cfg, T, torch.Generator(device=DEV).manual_seed(3), flip="frozen"))
        fixed = [(next(fl), next(rl)) for _ in range(2)]

        def hand(i):
            run.step(i, *fixed[i % 2])

        def fed(i):
            run.step(i, next(fl), next(rl))

        times = {"hand-fed": [], "loader-fed": []}
        for rnd in range(a.rounds + 1):
            for name, fn in (("hand-fed", hand), ("loader-fed", fed)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(a.steps):
                    fn(i)
                torch.cuda.synchronize()
                if rnd:
                    times[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
        for name, v in times.items():
            print(f"batch {B:4d} SFR-on iteration {name:10s} ms/step: {summary(v)}")
