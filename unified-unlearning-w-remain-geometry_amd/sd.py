"""The SFR-on concept-erasure iteration for Stable Diffusion (BASELINE config 4) on the native UNet.

One call of ``SDSFRon.step`` = one iteration of /root/reference/SD/train-scripts/nsfw_removal.py:108-173:
  forget: x_f / x_p noised with the SAME t and noise (:134-141) -> eps(x_f, c_forget) and stop-gradient eps(x_p, c_pseudo)
          -> forget_alpha * MSE (:143-147) -> backward -> [mask] -> Adam.step
  remain: LDM eps loss of shared_step (:164-166; ldm/models/diffusion/ddpm.py:1286-1319 with logvar = 0) -> backward -> Adam.step
Same Adam state for both steps (:81), no gradient clipping, no EMA.  ``train_method`` "full" / "xattn" (:66-77: parameters whose
name contains "attn2").  The reference's mask application (:157-160) tests a parameter NAME against a list of Parameters and is
therefore never true: ``mask_mode="as_written"`` reproduces that (no masking), ``"intended"`` multiplies
the forget-stage gradients by the saliency mask as the sibling scripts do.
``SDSFRon.step`` takes latents and prompt embeddings resident on the device; ``nsfw_removal`` is the script's loop around it, from image
folders (``ConceptImageLoader``) and prompts through ``LatentDiffusion``'s attached VAE encoder and text encoder.
"""
import numpy as np
import torch

from . import _lib, graphs, sweep
from ._lib import check, ptr, stream_ptr


class LDMSchedule:
    """register_schedule (ldm/models/diffusion/ddpm.py:153-240) for v1-inference.yaml: make_beta_schedule "linear" (a linspace of
    sqrt(beta), squared; util.py:21-30), fp64 numpy tables rounded to fp32 buffers.  Packed as the [T][8] table of sfron_q_sample."""

    def __init__(self, timesteps=1000, linear_start=0.00085, linear_end=0.012, device="cuda"):
        betas = (torch.linspace(linear_start ** 0.5, linear_end ** 0.5, timesteps, dtype=torch.float64) ** 2).numpy()
        ac = np.cumprod(1.0 - betas, axis=0)
        self.num_timesteps = timesteps
        tab = np.zeros((timesteps, _lib.TAB_COLS if hasattr(_lib, "TAB_COLS") else 8), dtype=np.float32)
        tab[:, 0] = np.sqrt(ac).astype(np.float32)
        tab[:, 1] = np.sqrt(1.0 - ac).astype(np.float32)
        self.tab = torch.from_numpy(tab).to(device).contiguous()
        # the fp32 buffers register_schedule keeps (ddpm.py:184-188: torch.tensor(fp64 table, dtype=float32)); the DDIM sampler reads them
        f32 = lambda a: torch.tensor(a, dtype=torch.float32).to(device)
        self.betas, self.alphas_cumprod, self.alphas_cumprod_prev = f32(betas), f32(ac), f32(np.append(1.0, ac[:-1]))

    def q_sample(self, x_start, t, noise):
        x_start, noise = x_start.contiguous(), noise.contiguous()
        out = torch.empty_like(x_start)
        n = x_start.shape[0]
        check(_lib.lib().sfron_q_sample(ptr(x_start), ptr(noise), ptr(t.contiguous()), ptr(self.tab), n, x_start.numel() // n, ptr(out),
                                        stream_ptr()), "q_sample")
        return out


class DiagonalGaussianPosterior:
    """ldm's DiagonalGaussianDistribution over VAE moments [B, 2z, h, w] (mean || logvar) on the device: ``mean``, ``logvar`` (clamped to
    [-30, 20] as the reference keeps it), ``parameters``, ``mode()`` and ``sample()`` = mean + exp(0.5 logvar) * eps, one launch of
    sfron_latent_sample (which clamps the same way); ``scale`` multiplies the sample in that launch."""

    def __init__(self, parameters):
        self.parameters = parameters

    mean = property(lambda self: self.parameters[:, :self.parameters.shape[1] // 2])
    logvar = property(lambda self: self.parameters[:, self.parameters.shape[1] // 2:].clamp(-30.0, 20.0))

    def mode(self):
        return self.mean

    def sample(self, eps=None, generator=None, scale=1.0):
        mom = self.parameters.contiguous()
        n, c2, h, w = mom.shape
        if eps is None:
            eps = torch.randn(n, c2 // 2, h, w, generator=generator, device=generator.device if generator is not None else mom.device)
        eps = eps.to(mom.device, torch.float32).contiguous()
        if tuple(eps.shape) != (n, c2 // 2, h, w):
            raise ValueError(f"eps must be {(n, c2 // 2, h, w)}, got {tuple(eps.shape)}")
        out = torch.empty(n, c2 // 2, h, w, dtype=torch.float32, device=mom.device)
        check(_lib.lib().sfron_latent_sample(ptr(mom), ptr(eps), n, c2 // 2, h * w, float(scale), ptr(out), stream_ptr()), "latent_sample")
        return out


class LatentDiffusion:
    """The part of ldm.models.diffusion.ddpm.LatentDiffusion the unlearning scripts call on the denoiser side, over the native UNet:
    ``model.diffusion_model`` (nsfw_removal.py:66, generate_fisher.py:30), ``num_timesteps``, ``q_sample`` (ddpm.py:424-445),
    ``apply_model(x_noisy, t, cond)`` (:1121-1131, crossattn conditioning: cond = the prompt embedding [B, 77, 768] or
    {"c_crossattn": [embedding]}), ``p_losses(x_start, cond, t, noise)`` -> (loss, loss_dict) (:1286-1319 with the v1-inference.yaml
    settings: eps-parameterisation, l2, logvar = 0 and not learned, l_simple_weight 1, original_elbo_weight 0).  The outputs take part
    in torch autograd (gradients land in the UNet's flat arena).  The first stage (VAE) and the text encoder are attached objects:
    get_input, encode_first_stage and shared_step run through a vae.VAEEncoder, get_learned_conditioning through a text.CLIPTextEncoder,
    decode_first_stage through a vae.VAEDecoder; each raises NotImplementedError without its object (latents and embeddings can always
    be handed in resident instead)."""

    parameterization, first_stage_key, cond_stage_key = "eps", "jpg", "txt"

    scale_factor = 0.18215
    first_stage_encoder = None           # (the class default: an object made without __init__ refuses the front end as one without an encoder)

    def __init__(self, unet, schedule=None, first_stage_decoder=None, cond_stage_model=None, first_stage_encoder=None):
        """first_stage_decoder: a vae.VAEDecoder; with it ``decode_first_stage(z)`` decodes latents (ldm's 1 / scale_factor * z).
        cond_stage_model: a text.CLIPTextEncoder (anything with ``encode(prompts)``); with it ``get_learned_conditioning(prompts)`` gives
        the [B, 77, D] contexts.  first_stage_encoder: a vae.VAEEncoder; with it ``encode_first_stage``, ``get_input`` and ``shared_step``
        run (images and prompts in, as the reference's scripts call them)."""
        import types
        self.model = types.SimpleNamespace(diffusion_model=unet, conditioning_key="crossattn")
        self.first_stage_decoder = first_stage_decoder
        self.first_stage_encoder = first_stage_encoder
        self.cond_stage_model = cond_stage_model
        self.schedule = schedule or LDMSchedule(device=unet.device_)
        self.num_timesteps = self.schedule.num_timesteps
        self.device = unet.device_
        self.training = True

    # the fp32 schedule buffers of ldm's LatentDiffusion (read by sfron.ddim.DDIMSampler), taken from the schedule when asked for
    betas = property(lambda self: self.schedule.betas)
    alphas_cumprod = property(lambda self: self.schedule.alphas_cumprod)
    alphas_cumprod_prev = property(lambda self: self.schedule.alphas_cumprod_prev)
    # q_sample's two fp32 tables (ddpm.py:190-191: fp64 square roots rounded once; columns 0 and 1 of the packed table), read by the
    # inpainting loop of sfron.plms.PLMSSampler
    sqrt_alphas_cumprod = property(lambda self: self.schedule.tab[:, 0])
    sqrt_one_minus_alphas_cumprod = property(lambda self: self.schedule.tab[:, 1])

    def train(self, mode=True):
        self.training = bool(mode)
        self.model.diffusion_model.train(mode)
        return self

    def eval(self):
        return self.train(False)

    def q_sample(self, x_start, t, noise=None):
        return self.schedule.q_sample(x_start, t, torch.randn_like(x_start) if noise is None else noise)

    def apply_model(self, x_noisy, t, cond):
        if isinstance(cond, dict):
            cond = torch.cat(cond["c_crossattn"], 1)
        return self.model.diffusion_model(x_noisy, t, context=cond)

    def p_losses(self, x_start, cond, t, noise=None):
        noise = torch.randn_like(x_start) if noise is None else noise
        out = self.apply_model(self.q_sample(x_start, t, noise), t, cond)
        loss_simple = ((out - noise) ** 2).mean([1, 2, 3])
        prefix = "train" if self.training else "val"
        loss = loss_simple.mean()                       # / exp(logvar) + logvar with logvar = 0; elbo weight 0
        return loss, {f"{prefix}/loss_simple": loss_simple.mean().detach(), f"{prefix}/loss": loss.detach()}

    def _outside(self, *a, **k):
        raise NotImplementedError("the VAE / CLIP front-end of LatentDiffusion is outside the unlearning hot path: hand latents and prompt "
                                  "embeddings in (sfron.latents for cached VAE moments)")

    # ---- the image / prompt front end (ddpm.py:912-972), through an attached vae.VAEEncoder; without one every entry raises, whatever
    # it is given
    def encode_first_stage(self, *args, **kwargs):
        """ddpm.py encode_first_stage: the posterior of first_stage_model.encode(x), over ``first_stage_encoder.moments(x)``.
        x: uint8 [B, H, W, 3] or fp32 [B, 3, H, W] in [-1, 1]."""
        if self.first_stage_encoder is None:
            return self._outside()
        return self._encode_first_stage(*args, **kwargs)

    def _encode_first_stage(self, x):
        return DiagonalGaussianPosterior(self.first_stage_encoder.moments(x))

    def get_first_stage_encoding(self, encoder_posterior, eps=None, generator=None):
        """ddpm.py get_first_stage_encoding: scale_factor * posterior.sample(), as ONE sfron_latent_sample launch with scale 0.18215."""
        return encoder_posterior.sample(eps=eps, generator=generator, scale=self.scale_factor)

    def get_input(self, *args, **kwargs):
        """ddpm.py:912-972 for the v1 configuration (conditioning_key "crossattn", cond_stage_key "txt", frozen cond stage):
        ``[z, c]`` = [scaled posterior sample of batch[k], prompt contexts of batch["txt"]], then ``x, xrec`` with
        return_first_stage_outputs (xrec needs the attached decoder), ``x`` with return_x, the prompts with return_original_cond -- the
        reference's order.  batch[k]: fp32 [B, H, W, 3] as the scripts pass it (a ``permute(0, 2, 3, 1)`` view of NCHW storage goes to the
        encoder without a copy), or uint8 [B, H, W, 3] (then ``x`` in the extras is the fp32 NCHW image ToTensor + Normalize(0.5, 0.5) give,
        (x / 255 - 0.5) / 0.5, which the encoder's input kernel forms).  ``eps`` / ``generator``: the posterior draw.  Anything outside that configuration raises NotImplementedError."""
        if self.first_stage_encoder is None:
            return self._outside()
        return self._get_input(*args, **kwargs)

    def _get_input(self, batch, k, return_first_stage_outputs=False, force_c_encode=False, cond_key=None, return_original_cond=False, bs=None,
                   return_x=False, generator=None, eps=None):
        x = batch[k]
        if bs is not None:
            x = x[:bs]
        x = x.to(self.device)
        if x.dim() != 4 or x.shape[3] != 3:
            raise ValueError(f"batch[{k!r}] must be [B, H, W, 3], got {tuple(x.shape)}")
        if x.dtype == torch.uint8:
            enc_in = x
        else:
            nchw = x.permute(0, 3, 1, 2)                    # 'b h w c -> b c h w' (DDPM.get_input)
            enc_in = x = (nchw if nchw.is_contiguous() else nchw.contiguous()).float()
        z = self.get_first_stage_encoding(self.encode_first_stage(enc_in), eps=eps, generator=generator).detach()
        if self.model.conditioning_key != "crossattn":
            raise NotImplementedError(f"conditioning_key {self.model.conditioning_key!r}: only 'crossattn' (v1-inference.yaml) is built")
        cond_key = self.cond_stage_key if cond_key is None else cond_key
        if cond_key != self.cond_stage_key:
            raise NotImplementedError(f"cond_key {cond_key!r}: only the prompts under {self.cond_stage_key!r} (v1-inference.yaml) are built")
        xc = batch[cond_key]
        c = self.get_learned_conditioning(xc)               # the cond stage is frozen: always encoded (force_c_encode changes nothing)
        if bs is not None:
            c = c[:bs]
        out = [z, c]
        if return_first_stage_outputs or return_x:
            if x.dtype == torch.uint8:
                x = ((x.permute(0, 3, 1, 2).float() / 255.0 - 0.5) / 0.5).contiguous()          # ToTensor + Normalize(0.5, 0.5)
        if return_first_stage_outputs:
            out.extend([x, self.decode_first_stage(z)])
        if return_x:
            out.extend([x])
        if return_original_cond:
            out.append(xc)
        return out

    def forward(self, x, c, generator=None):
        """ddpm.py LatentDiffusion.forward: t ~ U{0 .. num_timesteps - 1} per sample, drawn on the device, then p_losses (whose noise comes
        from the same generator, after t)."""
        t = torch.randint(0, self.num_timesteps, (x.shape[0],), device=self.device, generator=generator).long()
        noise = torch.randn(x.shape, device=self.device, generator=generator)
        return self.p_losses(x, c, t, noise)

    __call__ = forward

    def shared_step(self, *args, **kwargs):
        """ddpm.py shared_step: get_input(batch, first_stage_key) then forward -> (loss, loss_dict), with autograd as p_losses.  One
        ``generator`` serves the three draws in the order posterior eps, t, noise."""
        if self.first_stage_encoder is None:
            return self._outside()
        return self._shared_step(*args, **kwargs)

    def _shared_step(self, batch, generator=None):
        x, c = self.get_input(batch, self.first_stage_key, generator=generator)
        return self.forward(x, c, generator=generator)

    def get_learned_conditioning(self, c):
        """ddpm.py get_learned_conditioning with cond_stage_forward None: cond_stage_model.encode(c) (FrozenCLIPEmbedder: prompts ->
        last_hidden_state) through the attached encoder; without one it raises as the rest of the front end does."""
        if getattr(self, "cond_stage_model", None) is None:
            return self._outside(c)
        return self.cond_stage_model.encode(c)

    def decode_first_stage(self, z, *a, **k):
        """ddpm.py decode_first_stage: first_stage_model.decode(1 / scale_factor * z) -> fp32 [B, 3, H, W] in about [-1, 1], through the
        attached VAEDecoder (z / scale_factor in its head kernel); without one it raises as the rest of the front end does."""
        if self.first_stage_decoder is None:
            return self._outside(z, *a, **k)
        return self.first_stage_decoder.decode(z, scale=self.scale_factor)


class SDSFRon:
    def __init__(self, unet, schedule=None, lr=1e-5, forget_alpha=1.0, remain_alpha=1.0, train_method="full", mask=None,
                 mask_mode="as_written", process_group=None, use_graphs=False, fused_xattn=False, fused_wide_attn=False):
        """fused_wide_attn: run the UNet's self-attention of head width 160 (attn1 at the 16x16, 8x8 and middle levels) on the fused kernels of
        csrc/wattn.hip (UNetModel.fused_wide_self_attention) instead of batched products + softmax; opt-in, off by default.
        fused_xattn: run the UNet's cross-attention on the fused differentiable kernels (UNetModel.fused_cross_attention_train): scores and
        probabilities stay on the chip in the forward and the backward passes; opt-in, the default launches are unchanged."""
        from . import dp
        self.use_graphs, self._graphs, self._pool = bool(use_graphs), {}, (graphs.shared_pool() if use_graphs else None)
        if train_method not in ("full", "xattn"):
            raise ValueError("train_method must be 'full' or 'xattn' (nsfw_removal.py:66-77)")
        if mask_mode not in ("as_written", "intended"):
            raise ValueError("mask_mode must be 'as_written' or 'intended'")
        self.unet, self.s = unet, schedule or LDMSchedule(device=unet.device_)
        self.fa, self.ra, self.train_method = forget_alpha, remain_alpha, train_method
        self.pg, self._dp, self.world = process_group, dp, dp.world_size(process_group)
        p, g, w16, index = unet.flat_arena()
        # which coordinates the optimizer owns: Adam leaves a coordinate whose gradient is always zero where it is
        train = torch.zeros(p.numel(), dtype=torch.uint8, device=p.device)
        for name, (off, shape) in index.items():
            if train_method == "full" or "attn2" in name:
                n = 1
                for d in shape:
                    n *= d
                train[off:off + n] = 1
        self.train_mask = train
        self.forget_mask = train
        if mask is not None and mask_mode == "intended":
            fm = train.clone()
            for name, (off, shape) in index.items():
                m = mask.get(name, mask.get("model.diffusion_model." + name))
                if m is None:
                    raise KeyError(f"saliency mask has no entry for {name}")
                n = 1
                for d in shape:
                    n *= d
                fm[off:off + n] &= m.reshape(-1).to(device=p.device, dtype=torch.uint8)
            self.forget_mask = fm
        # contiguous arena ranges that hold the trainable tensors (offsets are multiples of 8): with "xattn" the sweep streams 5 % of the arena
        ranges = None
        if train_method != "full":
            spans = sorted((off, off + (int(np.prod(shape)) + 7) // 8 * 8) for name, (off, shape) in index.items() if "attn2" in name)
            ranges = []
            for lo, hi in spans:
                if ranges and lo <= ranges[-1][1]:
                    ranges[-1][1] = max(ranges[-1][1], hi)
                else:
                    ranges.append([lo, hi])
            ranges = [(lo, min(hi, p.numel())) for lo, hi in ranges]
        self.opt = sweep.FlatAdam(p, g, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, adamw=True, mask=self.train_mask, w_bf16=w16,
                                  ranges=ranges)
        unet.auto_prep = False                      # this loop tells the model when its weights changed
        if fused_xattn:
            unet.fused_cross_attention_train = True
        if fused_wide_attn:
            unet.fused_wide_self_attention = True
        unet.wgrad_filter = (lambda n: "attn2" in n) if train_method == "xattn" else None

    def _d_loss(self, out, target, scale):
        """d(scale * mean((out - target)^2)) / d out through the HIP loss kernel (this rank's share of the global batch mean)."""
        n, chw = out.shape[0], out[0].numel()
        coef = torch.full((n,), 2.0 * scale / (n * chw * self.world), dtype=torch.float32, device=out.device)
        d = torch.empty_like(out)
        tg, oc = target.contiguous(), out.contiguous()
        check(_lib.lib().sfron_ddpm_loss_bwd(ptr(tg), ptr(oc), ptr(coef), n, chw, ptr(d), stream_ptr()), "loss_bwd")
        return d

    def _mse(self, a, b):
        n, chw = a.shape[0], a[0].numel()
        per = torch.empty(n, dtype=torch.float32, device=a.device)
        bc, ac = b.contiguous(), a.detach().contiguous()
        check(_lib.lib().sfron_ddpm_sample_loss(ptr(bc), ptr(ac), n, chw, ptr(per), stream_ptr()), "sample_loss")
        return per.sum() / (n * chw)

    # the two stages: forward pass(es), loss, backward pass -- stream-ordered device work only, so each replays as one HIP graph
    def _forget_pass(self, x_f, x_p, c_f, c_p, t, noise):
        u, s = self.unet, self.s
        f_noisy, p_noisy = s.q_sample(x_f, t, noise), s.q_sample(x_p, t, noise)          # the SAME t and noise (:134-141)
        p_out, _ = u._run(p_noisy, t, c_p, need_grad=False)                               # stop-gradient branch (:145)
        f_out, bwd = u._run(f_noisy, t, c_f, need_grad=True)
        loss = self._mse(f_out, p_out)
        bwd(self._d_loss(f_out, p_out, self.fa))
        return loss

    def _remain_pass(self, x, c, t, noise):
        r_out, bwd = self.unet._run(self.s.q_sample(x, t, noise), t, c, need_grad=True)
        loss = self._mse(r_out, noise)
        bwd(self._d_loss(r_out, noise, self.ra))
        return loss

    def _stage(self, name, fn, **inputs):
        if not self.use_graphs:
            return fn(**inputs)
        if name not in self._graphs:
            self._graphs[name] = graphs.StageGraph(fn, warmup=1, pool=self._pool)
        return self._graphs[name](**inputs)

    def _exchange(self):
        """SUM all-reduce of this stage's gradients: the whole arena ("full"), or only the ranges the optimizer owns ("xattn" --
        the frozen layers' weight gradients are not even formed, their arena entries are stale)."""
        if self.opt.ranges is not None:
            self._dp.allreduce_ranges_(self.opt.g, self.opt.ranges, 64 << 20, self.pg)
        else:
            self._dp.allreduce_flat_(self.opt.g, 64 << 20, self.pg)

    def step(self, forget, remain):
        """forget: dict(x_f, x_p, c_f, c_p, t, noise); remain: dict(x, c, t, noise) -- device tensors, this rank's shard."""
        u = self.unet
        u.train()
        ori_forget = self._stage("forget", self._forget_pass, **{k: forget[k] for k in ("x_f", "x_p", "c_f", "c_p", "t", "noise")})
        if self.world > 1:
            self._exchange()
        self.opt.mask = self.forget_mask
        self.opt.step(max_norm=None, use_mask=True)                       # nsfw_removal.py:162 (no clipping)
        u.weights_updated(convs=self.train_method == "full")
        ori_remain = self._stage("remain", self._remain_pass, **{k: remain[k] for k in ("x", "c", "t", "noise")})
        if self.world > 1:
            self._exchange()
        self.opt.mask = self.train_mask
        self.opt.step(max_norm=None, use_mask=True)                       # :170
        u.weights_updated(convs=self.train_method == "full")
        return {"forget_loss": ori_forget, "remain_loss": ori_remain}


@torch.no_grad()
def sample_model(model, sampler, c, h, w, ddim_steps, scale, ddim_eta, start_code=None, n_samples=1, t_start=-1, log_every_t=None,
                 till_T=None, verbose=True):
    """SD/train-scripts/train-esd.py:43-84: DDIM-sample ``n_samples`` latents of an h x w image under the conditioning ``c`` with
    guidance ``scale`` (the empty prompt is encoded through ``model.get_learned_conditioning`` when scale != 1).  Returns the latents,
    or (latents, intermediates) when ``log_every_t`` is given.  ``sampler``: a sfron.ddim.DDIMSampler or a sfron.plms.PLMSSampler (whole
    trajectories only, eta 0) over ``model``."""
    uc = None
    if scale != 1.0:
        uc = model.get_learned_conditioning(n_samples * [""])
    log_t = 100 if log_every_t is None else log_every_t
    shape = [4, h // 8, w // 8]
    samples_ddim, inters = sampler.sample(S=ddim_steps, conditioning=c, batch_size=n_samples, shape=shape, verbose=False, x_T=start_code,
                                          unconditional_guidance_scale=scale, unconditional_conditioning=uc, eta=ddim_eta,
                                          verbose_iter=verbose, t_start=t_start, log_every_t=log_t, till_T=till_T)
    if log_every_t is not None:
        return samples_ddim, inters
    return samples_ddim


def decode_images_u8(model, z):
    """uint8 [B, H, W, 3] on the device: ``model.decode_first_stage(z)`` as the bytes SD/eval-scripts/generate-images.py writes,
    ``(image / 2 + 0.5).clamp(0, 1) * 255`` rounded (sfron_rows_to_image_u8, SFRON_IMAGE_ROUND)."""
    from .images import image_mode
    img = model.decode_first_stage(z).contiguous()              # fp32 [B, 3, H, W] in about [-1, 1]
    B, _, H, W = img.shape
    px = torch.empty(B * H * W, 4, dtype=torch.float32, device=img.device)
    u8 = torch.empty(B, H, W, 3, dtype=torch.uint8, device=img.device)
    L = _lib.lib()
    check(L.sfron_nchw_to_rows_f32(ptr(img), B, 3, H * W, 4, ptr(px), stream_ptr()), "nchw_to_rows_f32")
    check(L.sfron_rows_to_image_u8(ptr(px), 4, B, H, W, image_mode("round"), -1.0, 1.0, 0, 0, 0, B, ptr(u8), stream_ptr()), "rows_to_image_u8")
    return u8


@torch.no_grad()
def generate_images(model, prompts_path, save_path, guidance_scale=7.5, image_size=512, ddim_steps=100, num_samples=10, from_case=0,
                    rounds=10, sampler=None):
    """The driver loop of SD/eval-scripts/generate-images.py over the native models: for every row of the CSV at ``prompts_path``
    (columns ``case_number``, ``prompt``, ``evaluation_seed``; rows with case_number < from_case are skipped) ``torch.manual_seed(seed)``
    once, then ``rounds`` batches (the script's fixed 10) of ``num_samples`` start latents drawn on the CPU from that generator, each
    sampled with guidance and decoded through ``model.decode_first_stage`` to ``<save_path>/<case>_<k>.png``, k = round * 10 + sample
    as in the script.  Bytes are the script's ``(image / 2 + 0.5).clamp(0, 1) * 255`` rounded, through sfron_rows_to_image_u8.

    The reference script steps its latents with diffusers' LMSDiscreteScheduler.  diffusers is not part of this project's environment,
    so that scheduler cannot be pinned by a fixture and is out of scope: this driver samples with the ldm DDIM sampler (sfron.ddim,
    eta 0), the one the reference's training scripts use.  ``model``: a LatentDiffusion with a text encoder and a VAE decoder attached.
    Returns the list of paths written."""
    import csv
    import os
    from . import ddim, images
    sampler = sampler or ddim.DDIMSampler(model)
    os.makedirs(save_path, exist_ok=True)
    written = []
    with open(prompts_path, newline="") as f:
        rows = list(csv.DictReader(f))
    for row in rows:
        case_number, seed = int(row["case_number"]), int(row["evaluation_seed"])
        if case_number < from_case:
            continue
        prompt = [str(row["prompt"])] * num_samples
        generator = torch.manual_seed(seed)                 # the global CPU generator, seeded once per prompt
        for i in range(rounds):
            c = model.get_learned_conditioning(prompt)
            latents = torch.randn((num_samples, 4, image_size // 8, image_size // 8), generator=generator).to(model.device)
            z = sample_model(model, sampler, c, image_size, image_size, ddim_steps, guidance_scale, 0.0, start_code=latents,
                             n_samples=num_samples, verbose=False)
            u8 = decode_images_u8(model, z)
            B = u8.shape[0]
            for num in range(B):
                written.append(images.write_png(u8[num], os.path.join(save_path, f"{case_number}_{i * 10 + num}.png")))
    return written


# ------------------------------------------------------------------------------------------------ images and prompts in: loader, drivers
class ConceptImageLoader:
    """``cycle(DataLoader(dataset, batch_size))`` of SD/train-scripts/nsfw_removal.py:104-112 over the image files of ``folder``
    (latents.class_files order, no shuffling, the last batch of a pass short, then the pass starts over), with the transform of
    dataset.py:23-33 (sfron.resample).  ``next()`` gives this rank's strided share of the batch as device uint8 [n, S, S, 3], what
    VAEEncoder takes; ``len(loader)`` is the number of batches of one pass.  Files are decoded on the bounded host pool one batch ahead.
    gpu_resize: resample on the device (resample.sd_transform_gpu, bit-identical to the host route) instead of with Pillow on the pool's
    threads; the default is the route that measured faster."""

    def __init__(self, folder, batch_size, image_size=512, interpolation="bicubic", gpu_resize=True, workers=8, rank=0, world=1, device="cuda"):
        from concurrent.futures import ThreadPoolExecutor
        from . import latents
        self.files = latents.class_files(folder)
        if not self.files:
            raise FileNotFoundError(f"no image files under {folder}")
        if batch_size < 1 or not 0 <= rank < world:
            raise ValueError("batch_size >= 1 and 0 <= rank < world")
        self.bs, self.size, self.interp, self.gpu_resize = int(batch_size), int(image_size), interpolation, bool(gpu_resize)
        self.rank, self.world, self.dev = rank, world, torch.device(device)
        self._pool = latents._pool(workers)
        self._bg = ThreadPoolExecutor(max_workers=1)          # assembles the next batch (its own thread: it waits on _pool's tasks)
        self._i, self._ahead, self._pinned = 0, {}, None

    def __len__(self):
        return (len(self.files) + self.bs - 1) // self.bs

    def reset(self):
        """Back to the first batch of a pass."""
        self._i, self._ahead = 0, {}

    def batch_files(self, i):
        """This rank's files of batch ``i`` (counted from the start, across passes)."""
        p = i % len(self)
        return self.files[p * self.bs:(p + 1) * self.bs][self.rank::self.world]

    def _decode(self, path, on_device):
        from PIL import Image
        from . import resample
        with open(path, "rb") as fh:
            img = Image.open(fh)
            img.load()
        a = resample._rgb_array(img) if on_device else None
        # a mode the device does not take arrives transformed: size x size RGB, which the device route then passes through unchanged
        return a if a is not None else resample.sd_transform(img, self.size, self.interp)

    def host_batch(self, i):
        """The host route of batch ``i``: uint8 [n, S, S, 3] (torch, CPU) -- Pillow's bytes, for tests and tools."""
        arrs = list(self._pool.map(lambda f: self._decode(f, False), self.batch_files(i)))
        return torch.from_numpy(np.stack(arrs)) if arrs else torch.empty(0, self.size, self.size, 3, dtype=torch.uint8)

    def _host(self, i):
        if self.gpu_resize:
            return list(self._pool.map(lambda f: self._decode(f, True), self.batch_files(i)))
        return self.host_batch(i)

    def next(self):
        from . import resample
        i = self._i
        fut = self._ahead.pop(i, None)
        hb = fut.result() if fut is not None else self._host(i)
        self._ahead[i + 1] = self._bg.submit(self._host, i + 1)             # decode one batch ahead
        self._i = i + 1
        if self.gpu_resize:
            if not hb:
                return torch.empty(0, self.size, self.size, 3, dtype=torch.uint8, device=self.dev)
            return resample.sd_transform_gpu(hb, self.size, self.interp, device=self.dev)
        self._pinned = hb.pin_memory() if hb.numel() else hb                 # (the pinned batch lives until the next call)
        return self._pinned.to(self.dev, non_blocking=True)


def _expand(c, n):
    return c.expand(n, -1, -1).contiguous()


def nsfw_removal(model, forget_loader, remain_loader, n_iters, train_method, lr=1e-5, forget_alpha=1.0, remain_alpha=1.0, mask=None,
                 mask_mode="as_written", forget_prompt="a photo of a nude person", pseudo_prompt="a photo of a person wearing clothes",
                 remain_prompt=None, seed=0, log_every=10, save_every=None, on_save=None, **runner_kwargs):
    """The loop of SD/train-scripts/nsfw_removal.py:108-173 over an ``SDSFRon``: ``model`` a LatentDiffusion with the VAE encoder and the
    text encoder attached, the loaders ``ConceptImageLoader``s (anything whose ``next()`` gives what VAEEncoder.moments takes).  Returns
    (runner, forget losses, remain losses), the losses as python floats per iteration.

    Per iteration the reference calls get_input twice on the forget images and shared_step on the remain images.  Here
      * the three prompts are encoded once, before the loop, as [1, 77, D] and expanded to the batch's n rows (the cond stage is frozen);
      * the forget images are encoded once (``moments``), then drawn from twice with independent eps, as the two get_input calls draw;
      * every draw comes from one device ``torch.Generator`` seeded with ``seed``, in the order eps_f, eps_p, t, noise (forget stage),
        then eps_r, t_r, noise_r (remain stage);
      * contexts have the image batch's n rows.  (The reference sizes its prompt lists to batch_size, nsfw_removal.py:114-118, so its
        apply_model fails on the short last batch of a pass)
    ``save_every``: ``on_save(runner, step)`` after every that many iterations (sfron.export writes the checkpoint).  ``runner_kwargs`` go
    to SDSFRon (fused_xattn, fused_wide_attn, process_group; graphs need a fixed batch, so folders that leave a short batch do not suit
    them)."""
    import time
    enc, unet = model.first_stage_encoder, model.model.diffusion_model
    if enc is None or model.cond_stage_model is None:
        raise NotImplementedError("nsfw_removal needs a LatentDiffusion with first_stage_encoder and cond_stage_model attached")
    runner = SDSFRon(unet, schedule=model.schedule, lr=lr, forget_alpha=forget_alpha, remain_alpha=remain_alpha, train_method=train_method,
                     mask=mask, mask_mode=mask_mode, **runner_kwargs)
    remain_prompt = pseudo_prompt if remain_prompt is None else remain_prompt
    c_f, c_p, c_r = (model.get_learned_conditioning([p]) for p in (forget_prompt, pseudo_prompt, remain_prompt))
    gen = torch.Generator(device=model.device).manual_seed(int(seed))
    sf, T, dev = model.scale_factor, model.num_timesteps, model.device
    f_hist, r_hist, t0, logged = [], [], time.time(), 0
    for step in range(n_iters):
        model.train()
        post = model.encode_first_stage(forget_loader.next())
        n, z2, h, w = post.parameters.shape
        shape = (n, z2 // 2, h, w)
        x_f = post.sample(eps=torch.randn(shape, generator=gen, device=dev), scale=sf)
        x_p = post.sample(eps=torch.randn(shape, generator=gen, device=dev), scale=sf)
        t = torch.randint(0, T, (n,), generator=gen, device=dev).long()
        noise = torch.randn(shape, generator=gen, device=dev)
        post_r = model.encode_first_stage(remain_loader.next())
        n_r = post_r.parameters.shape[0]
        shape_r = (n_r, post_r.parameters.shape[1] // 2) + tuple(post_r.parameters.shape[2:])
        x_r = post_r.sample(eps=torch.randn(shape_r, generator=gen, device=dev), scale=sf)
        t_r = torch.randint(0, T, (n_r,), generator=gen, device=dev).long()
        noise_r = torch.randn(shape_r, generator=gen, device=dev)
        out = runner.step(dict(x_f=x_f, x_p=x_p, c_f=_expand(c_f, n), c_p=_expand(c_p, n), t=t, noise=noise),
                          dict(x=x_r, c=_expand(c_r, n_r), t=t_r, noise=noise_r))
        f_hist.append(out["forget_loss"])
        r_hist.append(out["remain_loss"])
        if log_every and (step + 1) % log_every == 0:
            fl, rl = torch.stack(f_hist[logged:]).mean().item(), torch.stack(r_hist[logged:]).mean().item()
            print(f"(step={step + 1:07d}) Forget Loss: {fl:.6f}, Remain Loss: {rl:.6f}, Train Steps/Sec: {(step + 1 - logged) / (time.time() - t0):.2f}")
            logged, t0 = step + 1, time.time()
        if save_every and on_save is not None and (step + 1) % save_every == 0:
            on_save(runner, step + 1)
    to_list = lambda h: torch.stack(h).tolist() if h else []
    return runner, to_list(f_hist), to_list(r_hist)


def setup_model(ckpt, tokenizer, device="cuda", vae_kwargs=None, text_kwargs=None, **unet_kwargs):
    """setup_model of SD/train-scripts/dataset.py:102-117 without the yaml: a CompVis checkpoint (a path, or a dict, optionally under
    "state_dict") -> LatentDiffusion with the UNet (``model.diffusion_model.*``), the VAE encoder and decoder (``first_stage_model.*``) and
    the CLIP text encoder (``cond_stage_model.*``) attached, each through its own loader.  ``tokenizer``: a text.CLIPTokenizer (its
    vocabulary is not in the checkpoint).  ``unet_kwargs`` go to sd_unet.UNetModel (defaults: v1-inference.yaml), ``vae_kwargs`` to both VAE
    halves (defaults: KL-f8), ``text_kwargs`` to text.CLIPTextEncoder (its sizes are read from the weights)."""
    from . import sd_unet, text, vae
    sd = ckpt
    if not isinstance(ckpt, dict):
        sd = torch.load(ckpt, map_location="cpu", weights_only=False)
    if "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    part = lambda pre: {k: v for k, v in sd.items() if k.startswith(pre)}
    for pre in ("model.diffusion_model.", "first_stage_model.", "cond_stage_model."):
        if not part(pre):
            raise KeyError(f"not a CompVis LatentDiffusion checkpoint: no {pre}* keys")
    unet = sd_unet.UNetModel(device=device, **unet_kwargs)
    unet.load_state_dict(part("model.diffusion_model."))
    enc, dec = vae.load_autoencoder(part("first_stage_model."), device=device, **(vae_kwargs or {}))
    cond = text.CLIPTextEncoder.from_state_dict(part("cond_stage_model."), tokenizer=tokenizer, device=device, **(text_kwargs or {}))
    return LatentDiffusion(unet, first_stage_decoder=dec, cond_stage_model=cond, first_stage_encoder=enc)
