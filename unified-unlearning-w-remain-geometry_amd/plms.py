"""The ldm PLMS sampler (SD/ldm/models/diffusion/plms.py ``PLMSSampler``) over the native LatentDiffusion: same constructor, the same
``make_schedule`` / ``sample`` / ``plms_sampling`` / ``p_sample_plms`` signatures and semantics, the ``mask`` / ``x0`` inpainting loop
included.  It is what CompVis ``txt2img`` samples with by default (50 steps at fourth order), and it drops into ``sd.sample_model`` and
``sd.generate_images(..., sampler=PLMSSampler(model))``.

What runs where: the schedule tables, the batch chunking and the once-per-call context preparation are sfron.ldm_sampler's, shared with
the DDIM sampler, and the step scalars follow the fp32 rule of DDIMSampler's ``step_coefficients`` with every square root correctly
rounded (see ``_sqrt32``).  A step is ONE UNet call at batch 2B (unconditional rows first) and ONE launch of sfron_plms_cfg_step, which
reads the two halves of the UNet's output in place, mixes them, forms the multistep combination with the (up to) three earlier
predictions and applies the eta = 0 update.  The first step has no history: two UNet calls and two launches (ORDER1 keeping e_t, then
MEAN), so S steps cost S + 1 UNet calls.  The history lives in three device buffers allocated once per call; from the fourth step on the new prediction
overwrites the oldest one in the launch that read it.  With ``mask`` / ``x0`` one launch of sfron_inpaint_blend in front of each step's
model call forms ``q_sample(x0, ts) * mask + (1 - mask) * img``.

Not built (each raises NotImplementedError naming the argument): ``score_corrector``, ``quantize_x0``, ``dynamic_threshold``,
``noise_dropout > 0``, ``ddim_use_original_steps`` / ``use_original_steps``, and any ``t_start`` / ``till_T`` but the defaults (partial
trajectories are an extension of the reference's DDIM sampler only).

``inpaint_noise``: an extra argument of ``sample`` / ``plms_sampling`` -- ``inpaint_noise[k]`` fixes the k-th ``q_sample`` draw (the
convention of ``step_noise`` in sfron.ddim); otherwise the noise is drawn on the device.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .ldm_sampler import LDMSampler

_ORDERS = (_lib.PLMS_ORDER1, _lib.PLMS_ORDER2, _lib.PLMS_ORDER3, _lib.PLMS_ORDER4)


def _sqrt32(v):
    """The correctly rounded fp32 square root of an fp32 value, as a Python float: the square root in double, rounded once more to fp32
    (for a square root the second rounding never changes the result: 53 >= 2 * 24 + 2 bits).  torch's CPU fp32 sqrt is not correctly
    rounded, and not the same from host to host -- measured with torch 2.10: sqrt(1 - alphas_cumprod[901]) comes out one ulp high on an AMD
    EPYC 9575F and rounded on an Intel Xeon, sqrt(alphas_cumprod[121]) one ulp low on that Xeon; numpy and libm give the rounded value on
    both -- and a step scalar that differs by an ulp moves every element of the step.  With this the sampler computes the same thing on
    every host, and the reference's own scalars wherever the reference's host rounds correctly."""
    return float(np.float32(math.sqrt(float(v))))


class PLMSSampler(LDMSampler):
    REFUSED = dict(score_corrector=None, quantize_x0=False, quantize_denoised=False, dynamic_threshold=None, noise_dropout=0.0,
                   ddim_use_original_steps=False, use_original_steps=False, t_start=-1, till_T=None)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, verbose=True):
        if ddim_eta != 0:
            raise ValueError("ddim_eta must be 0 for PLMS")
        super().make_schedule(ddim_num_steps, ddim_discretize, ddim_eta, verbose)

    @staticmethod
    def _sqrt_one_minus(alphas):
        return torch.tensor([_sqrt32(v) for v in 1.0 - alphas], dtype=torch.float32)

    def step_coefficients(self, index):
        """The rule of DDIMSampler.step_coefficients -- the five fp32 scalars of step ``index`` as the reference forms them by fp32 tensor
        arithmetic (plms.py:341-355): (sqrt(1 - a_t), sqrt(a_t), sqrt(a_prev), sqrt(1 - a_prev - sigma^2), sigma) -- in numpy fp32 scalars
        with the square roots of ``_sqrt32``, so that the scalars do not depend on the host."""
        f32 = lambda v: np.float32(float(v))            # what torch.full(..., v) holds
        a_t, a_prev, sigma = f32(self.ddim_alphas[index]), f32(self.ddim_alphas_prev[index]), f32(self.ddim_sigmas[index])
        rest = (np.float32(1.0) - a_prev) - sigma * sigma
        assert rest.dtype == np.float32
        return float(self.ddim_sqrt_one_minus_alphas[index]), _sqrt32(a_t), _sqrt32(a_prev), _sqrt32(rest), float(sigma)

    # ------------------------------------------------------------------------------------------------ sampling
    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None, quantize_x0=False,
               eta=0.0, mask=None, x0=None, temperature=1.0, noise_dropout=0.0, score_corrector=None, corrector_kwargs=None, verbose=True,
               x_T=None, log_every_t=100, unconditional_guidance_scale=1.0, unconditional_conditioning=None, dynamic_threshold=None,
               t_start=-1, till_T=None, verbose_iter=False, inpaint_noise=None, **kwargs):
        self._refuse(dict(locals(), ddim_use_original_steps=kwargs.get("ddim_use_original_steps", False)))
        self._warn_batch(conditioning, batch_size)
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        sliced = dict(x_T=x_T, unconditional_conditioning=unconditional_conditioning, x0=x0)
        kw = dict(callback=callback, img_callback=img_callback, temperature=temperature, log_every_t=log_every_t,
                  unconditional_guidance_scale=unconditional_guidance_scale)
        if mask is None or mask.shape[0] == 1:          # a mask of batch extent 1 serves every chunk whole
            kw["mask"] = mask
        else:
            sliced["mask"] = mask
        return self._chunked(self.plms_sampling, conditioning, batch_size, shape, sliced, dict(inpaint_noise=inpaint_noise), **kw)

    @torch.no_grad()
    def plms_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None, quantize_denoised=False,
                      mask=None, x0=None, img_callback=None, log_every_t=100, temperature=1.0, noise_dropout=0.0, score_corrector=None,
                      corrector_kwargs=None, unconditional_guidance_scale=1.0, unconditional_conditioning=None, dynamic_threshold=None,
                      inpaint_noise=None):
        self._refuse(locals())
        device, img, timesteps, intermediates = self._begin(shape, x_T, timesteps)
        b = shape[0]
        time_range = np.flip(timesteps)
        total_steps = timesteps.shape[0]
        if mask is not None:
            assert x0 is not None
            # the model's own fp32 q_sample tables (register_schedule: fp64 square roots rounded once), one host copy per call
            sqrt_ac = self.model.sqrt_alphas_cumprod.detach().to("cpu", torch.float32)
            sqrt_1m_ac = self.model.sqrt_one_minus_alphas_cumprod.detach().to("cpu", torch.float32)
        ring = torch.empty((3,) + tuple(shape), dtype=torch.float32, device=device)       # the history: allocated once, reused
        old_eps = []
        with self._conditioning(cond, unconditional_conditioning, unconditional_guidance_scale) as c_in:
            for i, step in enumerate(time_range):
                index = total_steps - i - 1
                ts = torch.full((b,), int(step), device=device, dtype=torch.long)
                ts_next = torch.full((b,), int(time_range[min(i + 1, len(time_range) - 1)]), device=device, dtype=torch.long)
                if mask is not None:
                    noise = torch.randn(shape, device=device) if inpaint_noise is None else inpaint_noise[i]
                    img = self._blend(img, x0, noise, mask, float(sqrt_ac[int(step)]), float(sqrt_1m_ac[int(step)]))
                img, pred_x0, e_t = self.p_sample_plms(img, cond, ts, index=index, temperature=temperature,
                                                       unconditional_guidance_scale=unconditional_guidance_scale,
                                                       unconditional_conditioning=unconditional_conditioning, old_eps=old_eps,
                                                       t_next=ts_next, _c_in=c_in, _ring=ring)
                old_eps.append(e_t)
                if len(old_eps) >= 4:
                    old_eps.pop(0)
                if callback:
                    callback(i)
                if img_callback:
                    img_callback(pred_x0, i)
                self._keep(intermediates, index, total_steps, log_every_t, img, pred_x0)
        return img, intermediates

    def _blend(self, img, x0, noise, mask, sqrt_ac, sqrt_one_minus_ac):
        """One launch of sfron_inpaint_blend -> (sqrt_ac x0 + sqrt_one_minus_ac noise) * mask + (1 - mask) * img, a new tensor."""
        if not img.is_cuda:
            raise _lib.SfronError("sfron ops need GPU tensors (no CPU fallback)")
        f = lambda v: v.to(img.device, torch.float32).contiguous()
        img, x0, noise, mask = f(img), f(x0), f(noise), f(mask)
        B, C = img.shape[0], img.shape[1]
        hw = img.numel() // (B * C)
        if x0.shape != img.shape or noise.shape != img.shape or mask.dim() != img.dim() or mask.shape[2:] != img.shape[2:]:
            raise ValueError(f"inpainting: x0 / noise must be {tuple(img.shape)} and mask [1 or B, 1 or C, H, W]; got x0 {tuple(x0.shape)}, "
                             f"noise {tuple(noise.shape)}, mask {tuple(mask.shape)}")
        out = torch.empty_like(img)
        check(_lib.lib().sfron_inpaint_blend(ptr(img), ptr(x0), ptr(noise), ptr(mask), B, C, hw, mask.shape[0], mask.shape[1], sqrt_ac,
                                             sqrt_one_minus_ac, ptr(out), stream_ptr()), "inpaint_blend")
        return out

    def _update(self, x, out, guided, old, order, guidance, coef, e_out, want_pred=True):
        """One launch of sfron_plms_cfg_step -> (x_prev, pred_x0).  out: the model's output, [2B] rows (unconditional first) when guided;
        old: the history tensors the order reads, newest first; e_out: where the guided prediction is kept (None: not kept)."""
        eu, ec = self._halves(out, guided)
        o = [ptr(t) for t in old] + [None] * (3 - len(old))
        s1, s2, s3, dr, _ = coef
        x_prev = torch.empty_like(x)
        pred_x0 = torch.empty_like(x) if want_pred else None
        check(_lib.lib().sfron_plms_cfg_step(ptr(x), eu, ec, o[0], o[1], o[2], order, x.numel(), float(guidance), s1, s2, s3, dr, ptr(e_out),
                                             ptr(x_prev), ptr(pred_x0), stream_ptr()), "plms_cfg_step")
        return x_prev, pred_x0

    @torch.no_grad()
    def p_sample_plms(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False, temperature=1.0,
                      noise_dropout=0.0, score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.0,
                      unconditional_conditioning=None, old_eps=None, t_next=None, dynamic_threshold=None, _c_in=None, _ring=None):
        """-> (x_prev, pred_x0, e_t).  old_eps: the earlier guided predictions, oldest first (the last three are read).  _ring: the
        sampling loop's three history buffers; with them e_t is written into the free slot, or over the oldest entry once three are held
        (the loop drops that entry next).  Without, e_t is a new tensor and old_eps is only read."""
        self._refuse(locals())
        x = x.contiguous().float()
        old_eps = [] if old_eps is None else old_eps
        guidance = unconditional_guidance_scale
        guided, _c_in = self._guidance(c, unconditional_conditioning, guidance, _c_in)
        coef = self.step_coefficients(index)
        k = min(len(old_eps), 3)
        old = [v.contiguous().float() for v in reversed(old_eps[len(old_eps) - k:])]          # newest first: old1, old2, old3
        if _ring is None:
            e_t = torch.empty_like(x)
        else:
            e_t = old_eps[-3] if k == 3 else _ring[k]
        out = self._model_output(x, t, _c_in, guided)
        if k > 0:
            x_prev, pred_x0 = self._update(x, out, guided, old, _ORDERS[k], guidance, coef, e_t)
            return x_prev, pred_x0, e_t
        # no history: the pseudo improved Euler step -- a plain update to t_next, a second model call there, the mean of the two predictions
        x_mid, _ = self._update(x, out, guided, [], _lib.PLMS_ORDER1, guidance, coef, e_t, want_pred=False)
        out = self._model_output(x_mid, t_next, _c_in, guided)
        x_prev, pred_x0 = self._update(x, out, guided, [e_t], _lib.PLMS_MEAN, guidance, coef, None)
        return x_prev, pred_x0, e_t
