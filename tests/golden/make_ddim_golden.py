"""Generates tests/golden/ddim.npz from the reference DDIMSampler (SD/ldm/models/diffusion/ddim.py), on the CPU.

The reference class is imported, not copied; it is subclassed only to override ``register_buffer`` (the reference forces every buffer to
"cuda", ddim.py:37-41).  It is driven with a small stand-in for LatentDiffusion (num_timesteps, betas, alphas_cumprod,
alphas_cumprod_prev, device, apply_model) whose fp32 tables are built as register_schedule builds them.

Contents
  (a) sched/<S>_<eta>_<discr>/{timesteps, alphas, alphas_prev, sigmas, sqrt_one_minus_alphas}
  (b) stub/<case>/...: full ``sample`` outputs and intermediates with the analytic model eps = 0.3 x cos(t / 1000) + 0.1 mean(c) (stub_eps)
      (with / without guidance, eta 0 / 0.5 with stored step noise, t_start / till_T partial runs), ``decode``, ``stochastic_encode``
  (c) unet/...: the reference UNetModel(**SD_TINY) with sd_tiny_weights() (from the seed), S = 8, guidance 3.0, B = 2, 8x8 latents,
      context [2, 5, 24]: x, pred_x0 and the guided eps at every step

Run:  python tests/golden/make_ddim_golden.py
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402

SCHEDULES = ((50, 0.0, "uniform"), (10, 0.5, "uniform"), (7, 1.0, "uniform"), (12, 0.0, "quad"))


def stub_eps(x, t, c):
    """eps = 0.3 x cos(t / 1000) + 0.1 mean(c) in fp32 torch.  The two per-sample scalars are evaluated in fp64 and rounded once to fp32, so
    that they do not depend on a machine's fp32 cosine or on the order of its fp32 reduction; the elementwise part is single IEEE fp32
    operations, the same bits on any device."""
    cs = torch.cos(t.double() / 1000).float().view(-1, 1, 1, 1)
    m = c.double().mean(dim=(1, 2)).float().view(-1, 1, 1, 1)
    return 0.3 * x * cs + 0.1 * m


class StandIn:
    """what DDIMSampler reads of LatentDiffusion"""

    def __init__(self, ut, apply_model):
        betas = ut.make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.012)
        ac = np.cumprod(1.0 - betas, axis=0)
        f32 = lambda a: torch.tensor(a, dtype=torch.float32)
        self.num_timesteps = 1000
        self.betas, self.alphas_cumprod, self.alphas_cumprod_prev = f32(betas), f32(ac), f32(np.append(1.0, ac[:-1]))
        self.device = torch.device("cpu")
        self.calls = []
        self._fn = apply_model

    def apply_model(self, x, t, c):
        out = self._fn(x, t, c)
        self.calls.append(out)
        return out


def main():
    om, ut = mg.import_ref_sd()
    ref_ddim = importlib.import_module("ldm.models.diffusion.ddim")

    class CpuSampler(ref_ddim.DDIMSampler):
        def register_buffer(self, name, attr):
            setattr(self, name, attr)

    noise_queue = []
    ref_ddim.noise_like = lambda shape, device, repeat=False: noise_queue.pop(0)        # the k-th draw = the stored step noise

    out = {}
    arr = lambda v: np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)

    # ---- (a) schedule tables
    model = StandIn(ut, stub_eps)
    for S, eta, discr in SCHEDULES:
        s = CpuSampler(model)
        s.make_schedule(S, ddim_discretize=discr, ddim_eta=eta, verbose=False)
        key = f"sched/{S}_{eta}_{discr}/"
        out[key + "timesteps"] = arr(s.ddim_timesteps)
        out[key + "alphas"] = arr(s.ddim_alphas)
        out[key + "alphas_prev"] = arr(s.ddim_alphas_prev)
        out[key + "sigmas"] = arr(s.ddim_sigmas)
        out[key + "sqrt_one_minus_alphas"] = arr(s.ddim_sqrt_one_minus_alphas)

    # ---- (b) the analytic model
    g = torch.Generator().manual_seed(101)
    B, shape = 2, (4, 8, 8)
    x_T = torch.randn(B, *shape, generator=g)
    cond, uc = torch.randn(B, 5, 24, generator=g), torch.randn(B, 5, 24, generator=g)
    noises = torch.randn(10, B, *shape, generator=g)
    out.update({"stub/x_T": arr(x_T), "stub/cond": arr(cond), "stub/uc": arr(uc), "stub/step_noise": arr(noises)})
    cases = {"plain": dict(S=10, eta=0.0, unconditional_guidance_scale=1.0, log_every_t=1),
             "guided": dict(S=10, eta=0.0, unconditional_guidance_scale=7.5, log_every_t=3),
             "eta": dict(S=10, eta=0.5, unconditional_guidance_scale=3.0, log_every_t=1),
             "partial": dict(S=10, eta=0.0, unconditional_guidance_scale=3.0, log_every_t=1, t_start=6, till_T=2)}
    for name, kw in cases.items():
        s = CpuSampler(model)
        noise_queue[:] = list(noises) if kw["eta"] else [torch.zeros(B, *shape)] * 10
        with torch.no_grad():
            smp, inter = s.sample(batch_size=B, shape=shape, conditioning=cond, unconditional_conditioning=uc, x_T=x_T, verbose=False, **kw)
        out[f"stub/{name}/samples"] = arr(smp)
        out[f"stub/{name}/x_inter"] = np.stack([arr(v) for v in inter["x_inter"]])
        out[f"stub/{name}/pred_x0"] = np.stack([arr(v) for v in inter["pred_x0"]])
    s = CpuSampler(model)
    s.make_schedule(10, ddim_eta=0.0, verbose=False)
    noise_queue[:] = [torch.zeros(B, *shape)] * 10
    out["stub/decode"] = arr(s.decode(x_T, cond, 5, unconditional_guidance_scale=3.0, unconditional_conditioning=uc))
    t_enc = torch.tensor([3, 7])
    out["stub/encode_t"] = arr(t_enc)
    out["stub/stochastic_encode"] = arr(s.stochastic_encode(x_T, t_enc, noise=noises[0]))

    # ---- (c) the reference tiny UNet
    ref = om.UNetModel(**mg.SD_TINY)
    ref.load_state_dict(mg.sd_tiny_weights())
    ref.eval()
    umodel = StandIn(ut, lambda x, t, c: ref(x, timesteps=t, context=c))
    g = torch.Generator().manual_seed(202)
    x_T = torch.randn(2, 4, 8, 8, generator=g)
    cond, uc = torch.randn(2, 5, 24, generator=g), torch.randn(2, 5, 24, generator=g)
    s = CpuSampler(umodel)
    noise_queue[:] = [torch.zeros(2, 4, 8, 8)] * 8
    with torch.no_grad():
        smp, inter = s.sample(S=8, batch_size=2, shape=(4, 8, 8), conditioning=cond, unconditional_conditioning=uc, x_T=x_T, eta=0.0,
                              unconditional_guidance_scale=3.0, log_every_t=1, t_start=8, verbose=False)
    assert len(umodel.calls) == 8 and len(inter["x_inter"]) == 9
    eps = [o[:2] + 3.0 * (o[2:] - o[:2]) for o in umodel.calls]
    out.update({"unet/x_T": arr(x_T), "unet/cond": arr(cond), "unet/uc": arr(uc), "unet/samples": arr(smp),
                "unet/x_inter": np.stack([arr(v) for v in inter["x_inter"]]), "unet/pred_x0": np.stack([arr(v) for v in inter["pred_x0"]]),
                "unet/eps": np.stack([arr(v) for v in eps])})
    path = os.path.join(HERE, "ddim.npz")
    np.savez_compressed(path, **out)
    print("ddim.npz written:", os.path.getsize(path), "bytes;", len(out), "arrays")
    for k in sorted(out):
        if k.startswith("sched/"):
            print(k, out[k].dtype, out[k].shape)


if __name__ == "__main__":
    main()
