#!/usr/bin/env python3
"""ms per step of the DiT likelihood evaluation (random weights, clip_denoised=True, unguided batch n), three arms and a floor per shape:
  torch      calc_bpd_loop as the reference writes it, torch ops around model.forward: per step a th.tensor([t] * B) upload, randn_like,
             q_sample, the posterior and model means, normal_kl AND the discretized likelihood over every element, th.where, the x_0 and
             re-derived epsilon mses (tables gathered per call, as _extract_into_tensor does)
  loop       diffusion.calc_bpd_loop(model.forward, ...): the generic path -- the same upload and draw, sfron_q_sample, model.forward,
             one sfron_dit_bpd_step
  native     dit_bpd.DiTBpdEvaluator: the draw, one engine forward pass from persistent buffers, one sfron_dit_bpd_step (terms + the next
             step's x_t), one sfron_dit_sampler_advance
  forward    the bare model.forward on fixed inputs, back to back: the floor
Shapes: DiT-XL/2 and DiT-B/4 at 256 px, n = 32.  Each round is one whole run of --steps respaced steps between two events on the current
stream, so a round holds its host gaps.  Every arm is measured --repeat times after one untimed run, the arms taking turns so that a
drift of the machine falls on all of them alike; the line carries each arm's minimum and its spread (max - min).
    python tools/bench_dit_bpd.py [--shapes xl2_n32,b4_n32] [--steps 10] [--repeat 5]
One process per GPU step is the caller's business: run it under `timeout`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch as th  # noqa: E402

SHAPES = {"xl2_n32": ("DiT-XL/2", 32), "b4_n32": ("DiT-B/4", 32)}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=",".join(SHAPES))
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--repeat", type=int, default=5)
a = ap.parse_args()
import sfron  # noqa: E402,F401
from sfron import diffusion, dit, dit_bpd  # noqa: E402

DEV = "cuda"
LATENT = 32                                          # 256 px


def run_ms(fn):
    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    th.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    th.cuda.synchronize()
    return e0.elapsed_time(e1) / a.steps


def torch_loop(d, model, x_start, y, clip_denoised=True):
    """The host loop restated in torch ops, step for step in the shape of the reference's calc_bpd_loop: what a user without the
    kernels would run."""
    tb = {k: np.asarray(v) for k, v in d.tables.items() if k != "timestep_map"}
    tb["log_betas"] = np.log(tb["betas"])

    def ext(name, t, shape):
        res = th.from_numpy(tb[name]).to(device=t.device)[t].float()
        while len(res.shape) < len(shape):
            res = res[..., None]
        return res + th.zeros(shape, device=t.device)

    def cdf(x):
        return 0.5 * (1.0 + th.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * th.pow(x, 3))))

    def mean_flat(v):
        return v.mean(dim=list(range(1, len(v.shape))))
    B, C = x_start.shape[:2]
    tmap = d.map_tensor
    vb, xstart_mse, mse = [], [], []
    for t in list(range(d.num_timesteps))[::-1]:
        t_batch = th.tensor([t] * B, device=x_start.device)
        noise = th.randn_like(x_start)
        sh = x_start.shape
        x_t = ext("sqrt_alphas_cumprod", t_batch, sh) * x_start + ext("sqrt_one_minus_alphas_cumprod", t_batch, sh) * noise
        true_mean = ext("posterior_mean_coef1", t_batch, sh) * x_start + ext("posterior_mean_coef2", t_batch, sh) * x_t
        true_lv = ext("posterior_log_variance_clipped", t_batch, sh)
        out = model(x_t, tmap[t_batch], y)
        eps_hat, var_values = th.split(out, C, dim=1)
        min_log, max_log = ext("posterior_log_variance_clipped", t_batch, sh), ext("log_betas", t_batch, sh)
        frac = (var_values + 1) / 2
        log_var = frac * max_log + (1 - frac) * min_log
        pred = ext("sqrt_recip_alphas_cumprod", t_batch, sh) * x_t - ext("sqrt_recipm1_alphas_cumprod", t_batch, sh) * eps_hat
        if clip_denoised:
            pred = pred.clamp(-1, 1)
        mean = ext("posterior_mean_coef1", t_batch, sh) * pred + ext("posterior_mean_coef2", t_batch, sh) * x_t
        kl = 0.5 * (-1.0 + log_var - true_lv + th.exp(true_lv - log_var) + ((true_mean - mean) ** 2) * th.exp(-log_var))
        kl = mean_flat(kl) / np.log(2.0)
        centered = x_start - mean
        inv_stdv = th.exp(-(0.5 * log_var))
        cdf_plus, cdf_min = cdf(inv_stdv * (centered + 1.0 / 255.0)), cdf(inv_stdv * (centered - 1.0 / 255.0))
        log_probs = th.where(x_start < -0.999, th.log(cdf_plus.clamp(min=1e-12)),
                             th.where(x_start > 0.999, th.log((1.0 - cdf_min).clamp(min=1e-12)), th.log((cdf_plus - cdf_min).clamp(min=1e-12))))
        nll = mean_flat(-log_probs) / np.log(2.0)
        vb.append(th.where((t_batch == 0), nll, kl))
        xstart_mse.append(mean_flat((pred - x_start) ** 2))
        eps = (ext("sqrt_recip_alphas_cumprod", t_batch, sh) * x_t - pred) / ext("sqrt_recipm1_alphas_cumprod", t_batch, sh)
        mse.append(mean_flat((eps - noise) ** 2))
    vb, xstart_mse, mse = th.stack(vb, dim=1), th.stack(xstart_mse, dim=1), th.stack(mse, dim=1)
    t_last = th.tensor([d.num_timesteps - 1] * B, device=x_start.device)
    tb["log_one_minus_alphas_cumprod"] = np.log(1.0 - tb["alphas_cumprod"])
    qt_mean, qt_lv = ext("sqrt_alphas_cumprod", t_last, sh) * x_start, ext("log_one_minus_alphas_cumprod", t_last, sh)
    prior = mean_flat(0.5 * (-1.0 - qt_lv + th.exp(qt_lv) + qt_mean ** 2)) / np.log(2.0)
    return {"total_bpd": vb.sum(dim=1) + prior, "prior_bpd": prior, "vb": vb, "xstart_mse": xstart_mse, "mse": mse}


diff = diffusion.create_diffusion(str(a.steps), device=DEV)
for shape in a.shapes.split(","):
    name, n = SHAPES[shape]
    th.manual_seed(0)
    model = dit.DiT_models[name](input_size=LATENT, num_classes=1000, batch_size=n)
    dit.randomize_zero_init(model, std=0.02, seed=1)
    model.eval()
    g = th.Generator(device=DEV).manual_seed(2)
    x0 = 0.5 * th.randn(n, 4, LATENT, LATENT, device=DEV, generator=g)
    y = th.randint(0, 1000, (n,), device=DEV, generator=g)
    t_fix = th.full((n,), 500, dtype=th.int64, device=DEV)
    ev = dit_bpd.DiTBpdEvaluator(model, diff, clip_denoised=True)

    def forward_only():
        for _ in range(a.steps):
            model.forward(x0, t_fix, y)
    arms = {"torch": lambda: torch_loop(diff, model.forward, x0, y),
            "loop": lambda: diff.calc_bpd_loop(model.forward, x0, clip_denoised=True, model_kwargs=dict(y=y)),
            "native": lambda: ev.evaluate(x0, y),
            "forward": forward_only}
    with th.no_grad():
        th.manual_seed(3)
        ref = arms["torch"]()                        # untimed warm-up runs; the three arms agree on the same global noise stream
        th.manual_seed(3)
        lp = arms["loop"]()
        th.manual_seed(3)
        nat = arms["native"]()
        arms["forward"]()
        agree = float(((lp["total_bpd"] - ref["total_bpd"]).abs() / ref["total_bpd"].abs()).max())
        same = all(bool(th.equal(lp[k], nat[k])) for k in lp)
        ms = {k: [] for k in arms}
        for _ in range(a.repeat):
            for k in arms:
                ms[k].append(run_ms(arms[k]))
    res = {"shape": shape, "model": name, "n": n, "steps": a.steps, "repeat": a.repeat, "loop_vs_torch_total_bpd_rel": float(f"{agree:.3e}"),
           "native_equals_loop_bits": same}
    for k in arms:
        res[k + "_ms"] = round(min(ms[k]), 3)
        res[k + "_spread_ms"] = round(max(ms[k]) - min(ms[k]), 3)
    print("DIT-BPD-STEP " + json.dumps(res), flush=True)
    ev.close()
    del ev, arms, model
