"""The ldm DDIM sampler (SD/ldm/models/diffusion/ddim.py ``DDIMSampler``) over the native LatentDiffusion: same constructor, the same
``make_schedule`` / ``sample`` / ``ddim_sampling`` / ``p_sample_ddim`` / ``decode`` / ``stochastic_encode`` signatures and semantics, so the
reference's ``sample_model`` (SD/train-scripts/train-esd.py:43-84) and its ESD partial trajectories (``t_start`` / ``till_T``) run on it.

What runs where: the schedule tables are host-side numpy / torch exactly as util.py:56-96 leaves them (fp32 alphas gathered from the
model's fp32 ``alphas_cumprod``; ``alphas_prev`` and the sigmas through numpy).  A step is ONE UNet call at batch 2B (unconditional rows
first) and ONE launch of sfron_ddim_cfg_step, which reads the two halves of the UNet's output in place (no ``chunk`` copy, no guidance
mix on the host).  With the native UNet the context is prepared once per call (UNetModel.prepare_context: the 16 key / value GEMMs of
attn2 leave the loop) and cross-attention runs on sfron_xattn_fwd (``fused_cross_attention``, set for the duration of the call).  The
tables, that context, the model call and the batch chunking are sfron.ldm_sampler's, shared with the PLMS sampler.

Not built (each raises NotImplementedError naming the argument): ``mask`` / ``x0`` inpainting, ``score_corrector``, ``quantize_x0``,
``dynamic_threshold``, ``noise_dropout > 0``, ``ddim_use_original_steps`` / ``use_original_steps``, ``encode``.

``step_noise``: an extra argument of ``sample`` / ``ddim_sampling`` -- ``step_noise[k]`` fixes the k-th noise draw (the convention of
ddpm.generalized_steps_conditional); for eta > 0 noise is otherwise drawn on the device.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .ldm_sampler import LDMSampler, make_ddim_sampling_parameters, make_ddim_timesteps  # noqa: F401 (the two functions: re-exported)


def _f32(v):
    """a table entry (0-dim tensor, numpy scalar or float) as the fp32 0-dim tensor ``torch.full(..., v)`` would hold"""
    return torch.tensor(float(v), dtype=torch.float32)


class DDIMSampler(LDMSampler):
    REFUSED = dict(mask=None, x0=None, score_corrector=None, quantize_x0=False, quantize_denoised=False, dynamic_threshold=None,
                   noise_dropout=0.0, ddim_use_original_steps=False, use_original_steps=False)

    @staticmethod
    def _sqrt_one_minus(alphas):
        return (1.0 - alphas).sqrt()

    # ------------------------------------------------------------------------------------------------ sampling
    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None, quantize_x0=False,
               eta=0.0, mask=None, x0=None, temperature=1.0, noise_dropout=0.0, score_corrector=None, corrector_kwargs=None, verbose=True,
               x_T=None, t_start=-1, log_every_t=100, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               dynamic_threshold=None, till_T=None, verbose_iter=False, step_noise=None, ddim_discretize="uniform", **kwargs):
        self._refuse(dict(locals(), ddim_use_original_steps=kwargs.get("ddim_use_original_steps", False)))
        self._warn_batch(conditioning, batch_size)
        self.make_schedule(ddim_num_steps=S, ddim_discretize=ddim_discretize, ddim_eta=eta, verbose=verbose)
        return self._chunked(self.ddim_sampling, conditioning, batch_size, shape,
                             dict(x_T=x_T, unconditional_conditioning=unconditional_conditioning), dict(step_noise=step_noise),
                             callback=callback, img_callback=img_callback, temperature=temperature, log_every_t=log_every_t,
                             unconditional_guidance_scale=unconditional_guidance_scale, till_T=till_T, t_start=t_start)

    @torch.no_grad()
    def ddim_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None, quantize_denoised=False,
                      mask=None, x0=None, img_callback=None, log_every_t=100, temperature=1.0, noise_dropout=0.0, score_corrector=None,
                      corrector_kwargs=None, unconditional_guidance_scale=1.0, unconditional_conditioning=None, dynamic_threshold=None,
                      t_start=-1, till_T=None, verbose_iter=False, step_noise=None):
        self._refuse(locals())
        device, img, timesteps, intermediates = self._begin(shape, x_T, timesteps)
        b = shape[0]
        timesteps = timesteps[:t_start]               # the reference's slice: t_start = -1 leaves the last table entry out
        time_range = np.flip(timesteps)
        total_steps = timesteps.shape[0]
        till = till_T if till_T is not None else 0
        with self._conditioning(cond, unconditional_conditioning, unconditional_guidance_scale) as c_in:
            for i, step in enumerate(time_range):
                index = total_steps - i - 1
                ts = torch.full((b,), int(step), device=device, dtype=torch.long)
                img, pred_x0 = self.p_sample_ddim(img, cond, ts, index=index, temperature=temperature,
                                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                                  unconditional_conditioning=unconditional_conditioning,
                                                  step_noise=None if step_noise is None else step_noise[i], _c_in=c_in)
                if callback:
                    img = callback(i, img, pred_x0)
                if img_callback:
                    img_callback(pred_x0, i)
                self._keep(intermediates, index, total_steps, log_every_t, img, pred_x0)
                if index + 1 == till:
                    break
        return img, intermediates

    def step_coefficients(self, index):
        """The five fp32 scalars of step ``index`` as p_sample_ddim forms them (ddim.py:352-372, fp32 tensor arithmetic):
        (sqrt(1 - a_t), sqrt(a_t), sqrt(a_prev), sqrt(1 - a_prev - sigma^2), sigma)."""
        a_t, a_prev, sigma = _f32(self.ddim_alphas[index]), _f32(self.ddim_alphas_prev[index]), _f32(self.ddim_sigmas[index])
        s1 = _f32(self.ddim_sqrt_one_minus_alphas[index])
        return float(s1), float(a_t.sqrt()), float(a_prev.sqrt()), float((1.0 - a_prev - sigma ** 2).sqrt()), float(sigma)

    def _update(self, x, eps_uncond, eps_cond, noise, guidance, coef):
        """One launch of sfron_ddim_cfg_step -> (x_prev, pred_x0).  eps_uncond / eps_cond: device addresses (eps_cond None or 0: no guidance)."""
        s1, s2, s3, dr, sigma = coef
        x_prev, pred_x0 = torch.empty_like(x), torch.empty_like(x)
        check(_lib.lib().sfron_ddim_cfg_step(ptr(x), eps_uncond, eps_cond or None, ptr(noise), x.numel(), float(guidance), s1, s2, s3, dr, sigma,
                                             ptr(x_prev), ptr(pred_x0), stream_ptr()), "ddim_cfg_step")
        return x_prev, pred_x0

    @torch.no_grad()
    def p_sample_ddim(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False, temperature=1.0,
                      noise_dropout=0.0, score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.0,
                      unconditional_conditioning=None, dynamic_threshold=None, step_noise=None, _c_in=None):
        self._refuse(locals())
        b = x.shape[0]
        x = x.contiguous().float()
        guided, _c_in = self._guidance(c, unconditional_conditioning, unconditional_guidance_scale, _c_in)
        out = self._model_output(x, t, _c_in, guided)          # held until the return: eu / ec are addresses into it, read by the launch
        eu, ec = self._halves(out, guided)
        coef = self.step_coefficients(index)
        noise = None
        if coef[4] != 0.0:
            if step_noise is not None:
                noise = step_noise.to(x.device, torch.float32)
            elif repeat_noise:
                noise = torch.randn((1, *x.shape[1:]), device=x.device).repeat(b, *((1,) * (x.dim() - 1)))
            else:
                noise = torch.randn(x.shape, device=x.device)
            if temperature != 1.0:
                noise = noise * temperature
            noise = noise.contiguous()
        return self._update(x, eu, ec, noise, unconditional_guidance_scale, coef)

    def encode(self, *a, **k):
        raise NotImplementedError("DDIMSampler: `encode` is not built (DESIGN.md section 7)")

    @torch.no_grad()
    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None):
        """x0 noised to the DDIM table's level t (an index tensor): sqrt(a_t) x0 + sqrt(1 - a_t) noise."""
        self._refuse(dict(use_original_steps=use_original_steps))
        if noise is None:
            noise = torch.randn_like(x0)
        view = (x0.shape[0],) + (1,) * (x0.dim() - 1)
        ti = t.to("cpu", torch.long)
        a = torch.sqrt(self.ddim_alphas)[ti].reshape(view).to(x0.device)
        s = self.ddim_sqrt_one_minus_alphas[ti].reshape(view).to(x0.device)
        return a * x0 + s * noise

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None, use_original_steps=False,
               step_noise=None):
        self._refuse(dict(use_original_steps=use_original_steps))
        timesteps = self.ddim_timesteps[:t_start]
        time_range = np.flip(timesteps)
        total_steps = timesteps.shape[0]
        x_dec = x_latent
        with self._conditioning(cond, unconditional_conditioning, unconditional_guidance_scale) as c_in:
            for i, step in enumerate(time_range):
                index = total_steps - i - 1
                ts = torch.full((x_latent.shape[0],), int(step), device=x_latent.device, dtype=torch.long)
                x_dec, _ = self.p_sample_ddim(x_dec, cond, ts, index=index, unconditional_guidance_scale=unconditional_guidance_scale,
                                              unconditional_conditioning=unconditional_conditioning,
                                              step_noise=None if step_noise is None else step_noise[i], _c_in=c_in)
        return x_dec

