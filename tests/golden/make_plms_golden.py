"""Generates tests/golden/plms.npz from the reference PLMSSampler (SD/ldm/models/diffusion/plms.py), on the CPU.

The reference class is imported, not copied; it is subclassed only to override ``register_buffer`` (the reference forces every buffer to
"cuda", plms.py:23-27), and ``plms.noise_like`` is replaced by zeros (sigma is 0 for PLMS: the draw is multiplied away).  It is driven with
the stand-in for LatentDiffusion of make_ddim_golden.py, here with a ``q_sample`` that uses the register_schedule tables (fp64 square roots
rounded once to fp32) and pops a stored noise.  The per-step records are taken by wrapping the instance's ``p_sample_plms``.

Contents
  (a) sched/<S>_<discr>/{timesteps, alphas, alphas_prev, sigmas, sqrt_one_minus_alphas} and step_coef [S][4]: the four fp32 scalars of every
      step, (sqrt(1 - a_t), sqrt(a_t), sqrt(a_prev), sqrt(1 - a_prev - sigma^2)), formed by the tensor expressions of plms.py:341-355 on
      the reference sampler's tables -- on the machine that wrote the fixture: torch's CPU fp32 sqrt is not correctly rounded (an ulp off
      for some arguments, differently from host to host), so these are the scalars the recorded steps were made with
  (b) stub/<case>/{samples, x_inter, pred_x0}: whole ``sample`` runs with the analytic model of make_ddim_golden.stub_eps --
        plain (S 10, no guidance, log_every_t 1), guided (S 10, scale 7.5, log_every_t 3), s1 (one step: t_next == t), s3 (three steps, so the orders
        stop at the third; "uniform" has no three-step table -- S = 3 gives the timestep 1000, which the reference cannot index -- so this case
        is make_schedule(3, "quad") followed by plms_sampling), inpaint (S 10, scale 3.0, a 0/1 mask [2,1,8,8], an x0 and ten stored q_sample draws)
      stub/{guided,inpaint}/step_*: for every step its input x (after the blend where there is one), both halves of each model output
        (step_out: S + 1 calls, the first step makes two), x_mid (the second call's input), the history it read (step_hist: newest
        first, zero padded, step_hist_len entries), the e_t it returned, its x_prev and pred_x0
  (c) unet/...: the reference UNetModel(**SD_TINY) with sd_tiny_weights(), S = 8, guidance 3.0, B = 2, 8x8 latents, context [2, 5, 24]:
      x_inter, pred_x0 and the guided eps of all 9 model calls

Run:  python tests/golden/make_plms_golden.py
"""
import importlib
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_ddim_golden as mdg  # noqa: E402
import make_golden as mg  # noqa: E402

SCHEDULES = ((50, "uniform"), (10, "uniform"), (8, "uniform"), (1, "uniform"), (12, "quad"), (3, "quad"))
B, SHAPE = 2, (4, 8, 8)


class StandIn(mdg.StandIn):
    """what PLMSSampler reads of LatentDiffusion: the DDIM stand-in plus q_sample (ddpm.py:424-445) over the register_schedule tables"""

    def __init__(self, ut, apply_model):
        super().__init__(ut, apply_model)
        betas = ut.make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.012)
        ac = np.cumprod(1.0 - betas, axis=0)
        self.sqrt_alphas_cumprod = torch.tensor(np.sqrt(ac), dtype=torch.float32)
        self.sqrt_one_minus_alphas_cumprod = torch.tensor(np.sqrt(1.0 - ac), dtype=torch.float32)
        self.noise_queue, self.inputs = [], []

    def apply_model(self, x, t, c):
        self.inputs.append(x.clone())
        return super().apply_model(x, t, c)

    def q_sample(self, x_start, t, noise=None):
        noise = self.noise_queue.pop(0) if noise is None else noise
        view = (x_start.shape[0], 1, 1, 1)
        return self.sqrt_alphas_cumprod[t].view(view) * x_start + self.sqrt_one_minus_alphas_cumprod[t].view(view) * noise


def record_steps(sampler):
    """wrap the instance's p_sample_plms: every call's input, history and results"""
    steps, inner = [], sampler.p_sample_plms

    def wrapped(x, c, t, **kw):
        hist = [h.clone() for h in kw["old_eps"]]
        x_prev, pred_x0, e_t = inner(x, c, t, **kw)
        steps.append(dict(x=x.clone(), hist=hist, x_prev=x_prev.clone(), pred_x0=pred_x0.clone(), e_t=e_t.clone()))
        return x_prev, pred_x0, e_t
    sampler.p_sample_plms = wrapped
    return steps


def main():
    om, ut = mg.import_ref_sd()
    ref_plms = importlib.import_module("ldm.models.diffusion.plms")

    class CpuSampler(ref_plms.PLMSSampler):
        def register_buffer(self, name, attr):
            setattr(self, name, attr)

    ref_plms.noise_like = lambda shape, device, repeat=False: torch.zeros(shape)

    out = {}
    arr = lambda v: np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)
    stack = lambda vs: np.stack([arr(v) for v in vs])

    # ---- (a) schedule tables
    model = StandIn(ut, mdg.stub_eps)
    for S, discr in SCHEDULES:
        s = CpuSampler(model)
        s.make_schedule(S, ddim_discretize=discr, ddim_eta=0.0, verbose=False)
        key = f"sched/{S}_{discr}/"
        out[key + "timesteps"] = arr(s.ddim_timesteps)
        out[key + "alphas"] = arr(s.ddim_alphas)
        out[key + "alphas_prev"] = arr(s.ddim_alphas_prev)
        out[key + "sigmas"] = arr(s.ddim_sigmas)
        out[key + "sqrt_one_minus_alphas"] = arr(s.ddim_sqrt_one_minus_alphas)
        coef = []
        for index in range(len(s.ddim_timesteps)):
            full = lambda v: torch.full((B, 1, 1, 1), v)
            a_t, a_prev, sigma_t = full(s.ddim_alphas[index]), full(s.ddim_alphas_prev[index]), full(s.ddim_sigmas[index])
            coef.append([float(v[0, 0, 0, 0]) for v in (full(s.ddim_sqrt_one_minus_alphas[index]), a_t.sqrt(), a_prev.sqrt(),
                                                        (1.0 - a_prev - sigma_t ** 2).sqrt())])
        out[key + "step_coef"] = np.asarray(coef, dtype=np.float32)

    # ---- (b) the analytic model
    g = torch.Generator().manual_seed(303)
    x_T = torch.randn(B, *SHAPE, generator=g)
    cond, uc = torch.randn(B, 5, 24, generator=g), torch.randn(B, 5, 24, generator=g)
    noises = torch.randn(10, B, *SHAPE, generator=g)
    x0 = torch.randn(B, *SHAPE, generator=g)
    mask = (torch.rand(B, 1, *SHAPE[1:], generator=g) < 0.5).float()
    out.update({"stub/x_T": arr(x_T), "stub/cond": arr(cond), "stub/uc": arr(uc), "stub/inpaint_noise": arr(noises), "stub/x0": arr(x0),
                "stub/mask": arr(mask)})
    cases = {"plain": dict(S=10, unconditional_guidance_scale=1.0, log_every_t=1),
             "guided": dict(S=10, unconditional_guidance_scale=7.5, log_every_t=3),
             "s1": dict(S=1, unconditional_guidance_scale=3.0, log_every_t=1),
             "s3": dict(S=3, unconditional_guidance_scale=3.0, log_every_t=1, quad=True),
             "inpaint": dict(S=10, unconditional_guidance_scale=3.0, log_every_t=1, mask=mask, x0=x0)}
    for name, kw in cases.items():
        s = CpuSampler(model)
        steps = record_steps(s)
        model.calls.clear()
        model.inputs.clear()
        model.noise_queue[:] = list(noises) if "mask" in kw else []
        with torch.no_grad():
            if kw.pop("quad", False):
                s.make_schedule(kw["S"], ddim_discretize="quad", verbose=False)
                smp, inter = s.plms_sampling(cond, (B,) + SHAPE, x_T=x_T, unconditional_conditioning=uc, log_every_t=kw["log_every_t"],
                                             unconditional_guidance_scale=kw["unconditional_guidance_scale"])
            else:
                smp, inter = s.sample(batch_size=B, shape=SHAPE, conditioning=cond, unconditional_conditioning=uc, x_T=x_T, verbose=False, **kw)
        assert len(model.calls) == kw["S"] + 1 and len(steps) == kw["S"] and not model.noise_queue
        pre = f"stub/{name}/"
        out[pre + "samples"] = arr(smp)
        out[pre + "x_inter"] = stack(inter["x_inter"])
        out[pre + "pred_x0"] = stack(inter["pred_x0"])
        if name in ("guided", "inpaint"):
            assert all(c.shape[0] == 2 * B for c in model.calls)
            hist = np.zeros((len(steps), 3, B) + SHAPE, dtype=np.float32)
            for k, st in enumerate(steps):
                for j, h in enumerate(reversed(st["hist"])):          # newest first: old1, old2, old3
                    hist[k, j] = arr(h)
            out.update({pre + "step_x": stack(st["x"] for st in steps), pre + "step_out": stack(model.calls), pre + "step_hist": hist,
                        pre + "step_hist_len": np.asarray([len(st["hist"]) for st in steps]), pre + "step_e_t": stack(st["e_t"] for st in steps),
                        pre + "step_x_prev": stack(st["x_prev"] for st in steps), pre + "step_pred_x0": stack(st["pred_x0"] for st in steps),
                        pre + "x_mid": arr(model.inputs[1][:B])})

    # ---- (c) the reference tiny UNet
    ref = om.UNetModel(**mg.SD_TINY)
    ref.load_state_dict(mg.sd_tiny_weights())
    ref.eval()
    umodel = StandIn(ut, lambda x, t, c: ref(x, timesteps=t, context=c))
    g = torch.Generator().manual_seed(404)
    x_T = torch.randn(2, 4, 8, 8, generator=g)
    cond, uc = torch.randn(2, 5, 24, generator=g), torch.randn(2, 5, 24, generator=g)
    s = CpuSampler(umodel)
    with torch.no_grad():
        smp, inter = s.sample(S=8, batch_size=2, shape=(4, 8, 8), conditioning=cond, unconditional_conditioning=uc, x_T=x_T, eta=0.0,
                              unconditional_guidance_scale=3.0, log_every_t=1, verbose=False)
    assert len(umodel.calls) == 9 and len(inter["x_inter"]) == 9
    eps = [o[:2] + 3.0 * (o[2:] - o[:2]) for o in umodel.calls]
    out.update({"unet/x_T": arr(x_T), "unet/cond": arr(cond), "unet/uc": arr(uc), "unet/samples": arr(smp),
                "unet/x_inter": stack(inter["x_inter"]), "unet/pred_x0": stack(inter["pred_x0"]), "unet/eps": stack(eps)})
    path = os.path.join(HERE, "plms.npz")
    # fixed member order and no timestamps: the same bytes on every run
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)
    print("plms.npz written:", os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
