"""The ldm DDIM sampler (SD/ldm/models/diffusion/ddim.py ``DDIMSampler``) over the native LatentDiffusion: same constructor, the same
``make_schedule`` / ``sample`` / ``ddim_sampling`` / ``p_sample_ddim`` / ``decode`` / ``stochastic_encode`` signatures and semantics, so the
reference's ``sample_model`` (SD/train-scripts/train-esd.py:43-84) and its ESD partial trajectories (``t_start`` / ``till_T``) run on it.

What runs where: the schedule tables are host-side numpy / torch exactly as util.py:56-96 leaves them (fp32 alphas gathered from the
model's fp32 ``alphas_cumprod``; ``alphas_prev`` and the sigmas through numpy).  A step is ONE UNet call at batch 2B (unconditional rows
first) and ONE launch of sfron_ddim_cfg_step, which reads the two halves of the UNet's output in place (no ``chunk`` copy, no guidance
mix on the host).  With the native UNet the context is prepared once per call (UNetModel.prepare_context: the 16 key / value GEMMs of
attn2 leave the loop) and cross-attention runs on sfron_xattn_fwd (``fused_cross_attention``, set for the duration of the call).

Not built (each raises NotImplementedError naming the argument): ``mask`` / ``x0`` inpainting, ``score_corrector``, ``quantize_x0``,
``dynamic_threshold``, ``noise_dropout > 0``, ``ddim_use_original_steps`` / ``use_original_steps``, ``encode``.

``step_noise``: an extra argument of ``sample`` / ``ddim_sampling`` -- ``step_noise[k]`` fixes the k-th noise draw (the convention of
ddpm.generalized_steps_conditional); for eta > 0 noise is otherwise drawn on the device.
"""
import contextlib

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

_LIMIT = 1 << 31          # bytes: the products refuse an operand that reaches this (csrc/common.h)


def make_ddim_timesteps(ddim_discr_method, num_ddim_timesteps, num_ddpm_timesteps):
    """util.py:56-76: every c-th step ("uniform") or a quadratic spacing over 80 % of the range ("quad"), shifted by one so that the
    last step lands on the data's alpha."""
    if ddim_discr_method == "uniform":
        steps = np.asarray(list(range(0, num_ddpm_timesteps, num_ddpm_timesteps // num_ddim_timesteps)))
    elif ddim_discr_method == "quad":
        steps = (np.linspace(0, np.sqrt(num_ddpm_timesteps * 0.8), num_ddim_timesteps) ** 2).astype(int)
    else:
        raise NotImplementedError(f'There is no ddim discretization method called "{ddim_discr_method}"')
    return steps + 1


def make_ddim_sampling_parameters(alphacums, ddim_timesteps, eta):
    """util.py:79-96 with the operand types it meets there: ``alphacums`` an fp32 CPU tensor, so ``alphas`` is an fp32 tensor, while
    ``alphas_prev`` is rebuilt from Python floats (a float64 numpy array, alphas_prev[0] = alphacums[0]) and the sigmas are formed by
    numpy / torch mixed arithmetic in this operand order.  Returns (sigmas, alphas, alphas_prev)."""
    alphas = alphacums[ddim_timesteps]
    alphas_prev = np.asarray([alphacums[0]] + alphacums[ddim_timesteps[:-1]].tolist())
    sigmas = eta * np.sqrt((1 - alphas_prev) / (1 - alphas) * (1 - alphas / alphas_prev))
    return sigmas, alphas, alphas_prev


def _f32(v):
    """a table entry (0-dim tensor, numpy scalar or float) as the fp32 0-dim tensor ``torch.full(..., v)`` would hold"""
    return torch.tensor(float(v), dtype=torch.float32)


class DDIMSampler(object):
    def __init__(self, model, schedule="linear", fused_wide_attn=False, **kwargs):
        """fused_wide_attn: for the duration of a sampling call the native UNet runs its wide-head self-attention (head width 160: the
        16x16, 8x8 and middle attn1 of SD v1) on the fused kernels of csrc/wattn.hip (UNetModel.fused_wide_self_attention); off by default."""
        super().__init__()
        self.model = model
        self.fused_wide_attn = bool(fused_wide_attn)
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule

    def register_buffer(self, name, attr):
        if isinstance(attr, torch.Tensor):
            attr = attr.to(self.model.device)
        setattr(self, name, attr)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, verbose=True):
        self.ddim_timesteps = make_ddim_timesteps(ddim_discretize, ddim_num_steps, self.ddpm_num_timesteps)
        alphas_cumprod = self.model.alphas_cumprod
        assert alphas_cumprod.shape[0] == self.ddpm_num_timesteps, "alphas have to be defined for each timestep"
        to_torch = lambda x: torch.as_tensor(x).clone().detach().to(torch.float32).to(self.model.device)
        ac = alphas_cumprod.cpu()
        self.register_buffer("betas", to_torch(self.model.betas))
        self.register_buffer("alphas_cumprod", to_torch(alphas_cumprod))
        self.register_buffer("alphas_cumprod_prev", to_torch(self.model.alphas_cumprod_prev))
        self.register_buffer("sqrt_alphas_cumprod", to_torch(ac.sqrt()))
        self.register_buffer("sqrt_one_minus_alphas_cumprod", to_torch((1.0 - ac).sqrt()))
        sigmas, alphas, alphas_prev = make_ddim_sampling_parameters(ac, self.ddim_timesteps, ddim_eta)
        # host-side tables (fp32 tensor / float64 array as the reference leaves them): p_sample_ddim reads one entry per step
        self.ddim_sigmas, self.ddim_alphas, self.ddim_alphas_prev = sigmas, alphas, alphas_prev
        self.ddim_sqrt_one_minus_alphas = (1.0 - alphas).sqrt()

    # ------------------------------------------------------------------------------------------------ guards and plumbing
    @staticmethod
    def _refuse(**kw):
        for name, (value, unset) in kw.items():
            bad = value is not None if unset is None else value != unset
            if bad:
                raise NotImplementedError(f"DDIMSampler: `{name}` is not built (DESIGN.md section 7)")

    def _unet(self):
        u = getattr(getattr(self.model, "model", None), "diffusion_model", None)
        return u if hasattr(u, "prepare_context") else None

    @staticmethod
    def _cond_tensor(c):
        if isinstance(c, dict):
            c = c[list(c.keys())[0]]
            c = torch.cat(c, 1) if isinstance(c, (list, tuple)) else c
        return c

    @contextlib.contextmanager
    def _conditioning(self, cond, uc, scale):
        """The context one loop hands to every step: unconditional rows first when guided; prepared once on the native UNet."""
        guided = not (uc is None or scale == 1.0)
        c_in = torch.cat([self._cond_tensor(uc), self._cond_tensor(cond)]) if guided else self._cond_tensor(cond)
        unet = self._unet()
        if unet is None or not isinstance(c_in, torch.Tensor):
            yield c_in
            return
        keep, unet.fused_cross_attention = unet.fused_cross_attention, True
        keep_w = unet.fused_wide_self_attention
        unet.fused_wide_self_attention = keep_w or self.fused_wide_attn
        try:
            yield unet.prepare_context(c_in)
        finally:
            unet.fused_cross_attention = keep
            unet.fused_wide_self_attention = keep_w

    def chunk_size(self, batch_size, shape):
        """Samples per run such that no operand of the UNet at batch 2B reaches 2 GiB (the library refuses those); the native UNet
        reports its widest per-sample operand, any other model is run whole."""
        unet = self._unet()
        if unet is None or not hasattr(unet, "per_sample_bytes"):
            return batch_size
        ps = 2 * unet.per_sample_bytes(shape[1], shape[2])
        if ps >= _LIMIT:
            raise ValueError(f"one {shape[1]}x{shape[2]} latent needs a {ps}-byte operand at batch 2: above 2 GiB")
        return max(1, min(batch_size, (_LIMIT - 1) // ps))

    # ------------------------------------------------------------------------------------------------ sampling
    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None, quantize_x0=False,
               eta=0.0, mask=None, x0=None, temperature=1.0, noise_dropout=0.0, score_corrector=None, corrector_kwargs=None, verbose=True,
               x_T=None, t_start=-1, log_every_t=100, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               dynamic_threshold=None, till_T=None, verbose_iter=False, step_noise=None, ddim_discretize="uniform", **kwargs):
        self._refuse(mask=(mask, None), x0=(x0, None), score_corrector=(score_corrector, None), quantize_x0=(bool(quantize_x0), False),
                     dynamic_threshold=(dynamic_threshold, None), noise_dropout=(float(noise_dropout), 0.0),
                     ddim_use_original_steps=(bool(kwargs.get("ddim_use_original_steps", False)), False))
        if conditioning is not None:
            cbs = self._cond_tensor(conditioning).shape[0]
            if cbs != batch_size:
                print(f"Warning: Got {cbs} conditionings but batch-size is {batch_size}")
        self.make_schedule(ddim_num_steps=S, ddim_discretize=ddim_discretize, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        kw = dict(callback=callback, img_callback=img_callback, temperature=temperature, log_every_t=log_every_t,
                  unconditional_guidance_scale=unconditional_guidance_scale, till_T=till_T, t_start=t_start)
        n = self.chunk_size(batch_size, shape)
        if n >= batch_size:
            return self.ddim_sampling(conditioning, (batch_size, C, H, W), x_T=x_T, unconditional_conditioning=unconditional_conditioning,
                                      step_noise=step_noise, **kw)
        # chunks of the batch, as VAEDecoder.decode runs its batch: every operand at batch 2 n stays under 2 GiB
        cut = lambda v, lo, hi: None if v is None else self._cond_tensor(v)[lo:hi]
        outs = []
        for lo in range(0, batch_size, n):
            hi = min(batch_size, lo + n)
            sn = None if step_noise is None else _SliceNoise(step_noise, lo, hi)
            outs.append(self.ddim_sampling(cut(conditioning, lo, hi), (hi - lo, C, H, W), x_T=cut(x_T, lo, hi),
                                           unconditional_conditioning=cut(unconditional_conditioning, lo, hi), step_noise=sn, **kw))
        inter = {k: [torch.cat(parts) for parts in zip(*(o[1][k] for o in outs))] for k in outs[0][1]}
        return torch.cat([o[0] for o in outs]), inter

    @torch.no_grad()
    def ddim_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None, quantize_denoised=False,
                      mask=None, x0=None, img_callback=None, log_every_t=100, temperature=1.0, noise_dropout=0.0, score_corrector=None,
                      corrector_kwargs=None, unconditional_guidance_scale=1.0, unconditional_conditioning=None, dynamic_threshold=None,
                      t_start=-1, till_T=None, verbose_iter=False, step_noise=None):
        self._refuse(mask=(mask, None), x0=(x0, None), score_corrector=(score_corrector, None),
                     quantize_x0=(bool(quantize_denoised), False), dynamic_threshold=(dynamic_threshold, None),
                     noise_dropout=(float(noise_dropout), 0.0), ddim_use_original_steps=(bool(ddim_use_original_steps), False))
        device = self.model.betas.device
        b = shape[0]
        img = torch.randn(shape, device=device) if x_T is None else x_T
        if timesteps is None:
            timesteps = self.ddim_timesteps
        else:
            subset_end = int(min(timesteps / self.ddim_timesteps.shape[0], 1) * self.ddim_timesteps.shape[0]) - 1
            timesteps = self.ddim_timesteps[:subset_end]
        timesteps = timesteps[:t_start]               # the reference's slice: t_start = -1 leaves the last table entry out
        intermediates = {"x_inter": [img], "pred_x0": [img]}
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
                if index % log_every_t == 0 or index == total_steps - 1:
                    intermediates["x_inter"].append(img)
                    intermediates["pred_x0"].append(pred_x0)
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
        """One launch of sfron_ddim_cfg_step -> (x_prev, pred_x0).  eps_uncond / eps_cond: device addresses (eps_cond 0: no guidance)."""
        s1, s2, s3, dr, sigma = coef
        x_prev, pred_x0 = torch.empty_like(x), torch.empty_like(x)
        check(_lib.lib().sfron_ddim_cfg_step(ptr(x), eps_uncond, eps_cond or None, ptr(noise), x.numel(), float(guidance), s1, s2, s3, dr, sigma,
                                             ptr(x_prev), ptr(pred_x0), stream_ptr()), "ddim_cfg_step")
        return x_prev, pred_x0

    @torch.no_grad()
    def p_sample_ddim(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False, temperature=1.0,
                      noise_dropout=0.0, score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.0,
                      unconditional_conditioning=None, dynamic_threshold=None, step_noise=None, _c_in=None):
        self._refuse(use_original_steps=(bool(use_original_steps), False), quantize_x0=(bool(quantize_denoised), False),
                     noise_dropout=(float(noise_dropout), 0.0), score_corrector=(score_corrector, None),
                     dynamic_threshold=(dynamic_threshold, None))
        b = x.shape[0]
        x = x.contiguous().float()
        guided = not (unconditional_conditioning is None or unconditional_guidance_scale == 1.0)
        if _c_in is None:
            _c_in = torch.cat([self._cond_tensor(unconditional_conditioning), self._cond_tensor(c)]) if guided else self._cond_tensor(c)
        if guided:            # one call at batch 2 B, unconditional rows first; the update reads the two halves where they are
            out = self.model.apply_model(torch.cat([x] * 2), torch.cat([t] * 2), _c_in).contiguous().float()
            eu, ec = out.data_ptr(), out.data_ptr() + out.element_size() * (out.numel() // 2)
        else:
            out = self.model.apply_model(x, t, _c_in).contiguous().float()
            eu, ec = out.data_ptr(), 0
        if not out.is_cuda:
            raise _lib.SfronError("sfron ops need GPU tensors (no CPU fallback)")
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
        self._refuse(use_original_steps=(bool(use_original_steps), False))
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
        self._refuse(use_original_steps=(bool(use_original_steps), False))
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


class _SliceNoise:
    """step_noise[k][lo:hi] of a chunked run"""

    def __init__(self, src, lo, hi):
        self.src, self.lo, self.hi = src, lo, hi

    def __getitem__(self, k):
        return self.src[k][self.lo:self.hi]
