"""Host side of the DiT diffusion loss (csrc/loss.hip).

API mirror of /root/reference/DiT/diffusion: ``create_diffusion("")`` returns an object with
``num_timesteps``, ``q_sample(x_start, t, noise)`` and
``training_losses(model, x_start, t, model_kwargs=None, noise=None) -> {"loss","mse","vb"}``
(gaussian_diffusion.py:215-230,715-787; __init__.py:10-46).  Tables are built host-side in fp64
with the same operation order as the reference and rounded once to fp32 for the kernels.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr


def space_timesteps(num_timesteps, section_counts):
    """respace.py:12-62: which original timesteps a respaced process keeps (returned as a set, like the reference)."""
    if isinstance(section_counts, str):
        if section_counts.startswith("ddim"):
            want = int(section_counts[len("ddim"):])
            for stride in range(1, num_timesteps):
                if len(range(0, num_timesteps, stride)) == want:
                    return set(range(0, num_timesteps, stride))
            raise ValueError(f"cannot create exactly {num_timesteps} steps with an integer stride")
        section_counts = [int(x) for x in section_counts.split(",")]
    size_per, extra = divmod(num_timesteps, len(section_counts))
    start, steps = 0, []
    for i, count in enumerate(section_counts):
        size = size_per + (1 if i < extra else 0)
        if size < count:
            raise ValueError(f"cannot divide section of {size} steps into {count}")
        stride = 1 if count <= 1 else (size - 1) / (count - 1)
        cur = 0.0
        for _ in range(count):
            steps.append(start + round(cur))
            cur += stride
        start += size
    return set(steps)


def _tables_fp64(num_timesteps=1000, use_timesteps=None):
    # gaussian_diffusion.py:98-115 (linear), respace.py:65-87 (betas re-derived from the cumprod of the retained
    # steps; also when every step is kept), gaussian_diffusion.py:163-201
    scale = 1000 / num_timesteps
    base = np.linspace(scale * 0.0001, scale * 0.02, num_timesteps, dtype=np.float64)
    base_ac = np.cumprod(1.0 - base, axis=0)
    last, nb, tmap = 1.0, [], []
    for i, ac in enumerate(base_ac):
        if use_timesteps is None or i in use_timesteps:
            nb.append(1 - ac / last)
            last = ac
            tmap.append(i)
    betas = np.array(nb, dtype=np.float64)
    alphas = 1.0 - betas
    ac = np.cumprod(alphas, axis=0)
    ac_prev = np.append(1.0, ac[:-1])
    post_var = betas * (1.0 - ac_prev) / (1.0 - ac)
    return dict(
        timestep_map=tmap, betas=betas, alphas_cumprod=ac,
        alphas_cumprod_prev=ac_prev, alphas_cumprod_next=np.append(ac[1:], 0.0),          # gaussian_diffusion.py:169-170
        sqrt_alphas_cumprod=np.sqrt(ac), sqrt_one_minus_alphas_cumprod=np.sqrt(1.0 - ac),
        sqrt_recip_alphas_cumprod=np.sqrt(1.0 / ac), sqrt_recipm1_alphas_cumprod=np.sqrt(1.0 / ac - 1),
        posterior_mean_coef1=betas * np.sqrt(ac_prev) / (1.0 - ac),
        posterior_mean_coef2=(1.0 - ac_prev) * np.sqrt(alphas) / (1.0 - ac),
        posterior_log_variance_clipped=np.log(np.append(post_var[1], post_var[1:])),
        log_betas=np.log(betas))


_TAB_ORDER = ["sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod",
              "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
              "posterior_log_variance_clipped", "log_betas"]


# the sampler table of sfron_dit_sample_step: the eight columns above in their order, then these three (include/sfron.h)
_SAMPLER_TAB_ORDER = _TAB_ORDER + ["alphas_cumprod", "alphas_cumprod_prev", "alphas_cumprod_next"]
_STEP_MODES = {"ddpm": _lib.DIT_SAMPLE_DDPM, "ddim": _lib.DIT_SAMPLE_DDIM, "ddim_reverse": _lib.DIT_SAMPLE_DDIM_REVERSE}


class _WrappedModel:
    """respace.py:117-129: the model sees the ORIGINAL timestep of each respaced index."""

    def __init__(self, model, map_tensor):
        self.model, self.map_tensor = model, map_tensor

    def __call__(self, x, ts, **kwargs):
        return self.model(x, self.map_tensor.to(ts.dtype)[ts], **kwargs)


class GaussianDiffusion:
    """epsilon-prediction, LEARNED_RANGE variance, MSE loss: what create_diffusion(timestep_respacing) builds
    (a SpacedDiffusion; "" keeps all steps)."""

    def __init__(self, num_timesteps=1000, device="cuda", use_timesteps=None):
        self.tables = _tables_fp64(num_timesteps, use_timesteps)
        self.original_num_steps = num_timesteps
        self.timestep_map = self.tables["timestep_map"]
        self.num_timesteps = len(self.timestep_map)
        self._identity_map = self.timestep_map == list(range(num_timesteps))
        self.map_tensor = torch.tensor(self.timestep_map, dtype=torch.int64, device=device)
        packed = np.stack([self.tables[k] for k in _TAB_ORDER], axis=1).astype(np.float32)
        self.tab = torch.from_numpy(packed).to(device).contiguous()
        # a table of its own, [T][11]: the loss / p_sample kernels index ``tab`` by 8
        spacked = np.stack([self.tables[k] for k in _SAMPLER_TAB_ORDER], axis=1).astype(np.float32)
        self.sampler_tab = torch.from_numpy(spacked).to(device).contiguous()

    def _wrap_model(self, model):
        if self._identity_map or isinstance(model, _WrappedModel):
            return model
        return _WrappedModel(model, self.map_tensor)

    def q_sample(self, x_start, t, noise=None):
        if noise is None:
            noise = torch.randn_like(x_start)
        x_start, noise = x_start.contiguous(), noise.contiguous()
        out = torch.empty_like(x_start)
        n = x_start.shape[0]
        check(_lib.lib().sfron_q_sample(ptr(x_start), ptr(noise), ptr(t.contiguous()), ptr(self.tab), n,
                                        x_start.numel() // n, ptr(out), stream_ptr()), "q_sample")
        return out

    def loss_fwd_bwd(self, model_output, x_start, t, noise, grad_scale):
        """Fused loss forward + d(grad_scale * sum_i loss_i)/d model_output.  Returns (mse[N], vb[N], d_out)."""
        n, c2 = model_output.shape[0], model_output.shape[1]
        c = c2 // 2
        hw = model_output.numel() // (n * c2)
        mse = torch.empty(n, dtype=torch.float32, device=model_output.device)
        vb = torch.empty_like(mse)
        d_out = torch.empty_like(model_output)
        check(_lib.lib().sfron_dit_loss_fwd_bwd(ptr(x_start), ptr(noise), ptr(model_output), ptr(t), ptr(self.tab),
                                                n, c, hw, float(grad_scale), ptr(mse), ptr(vb), ptr(d_out),
                                                stream_ptr()), "dit_loss_fwd_bwd")
        return mse, vb, d_out

    def training_losses(self, model, x_start, t, model_kwargs=None, noise=None):
        """Reference signature (gaussian_diffusion.py:715).  ``terms["loss"]`` carries an autograd edge into
        ``model``'s output, so ``terms["loss"].mean().backward()`` works as in DiT/forget.py:271-288."""
        if model_kwargs is None:
            model_kwargs = {}
        if noise is None:
            noise = torch.randn_like(x_start)
        x_t = self.q_sample(x_start, t, noise)
        model_output = self._wrap_model(model)(x_t, t, **model_kwargs)
        mse, vb, loss = _DitLoss.apply(model_output, self, x_start.contiguous(), t.contiguous(), noise.contiguous())
        return {"loss": loss, "mse": mse, "vb": vb}


    # ------------------------------------------------------------------ sampling (gaussian_diffusion.py:376-511)
    def p_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, noise=None):
        """One ancestral step; ``noise`` (optional) replaces the reference's ``th.randn_like(x)`` draw."""
        if denoised_fn is not None or cond_fn is not None:
            raise NotImplementedError("denoised_fn / cond_fn are not used by the unlearning scripts")
        x = x.contiguous().float()
        t = t.contiguous()
        model_output = self._wrap_model(model)(x, t, **(model_kwargs or {}))
        if isinstance(model_output, tuple):
            model_output = model_output[0]
        n, c = x.shape[0], x.shape[1]
        assert model_output.shape == (n, 2 * c, *x.shape[2:])
        if noise is None:
            noise = torch.randn_like(x)
        sample, pred = torch.empty_like(x), torch.empty_like(x)
        mo, nz = model_output.contiguous().float(), noise.contiguous()       # named: temporaries must outlive the launch
        check(_lib.lib().sfron_p_sample(ptr(x), ptr(mo), ptr(t), ptr(self.tab), ptr(nz),
                                        n, c, x[0, 0].numel(), int(bool(clip_denoised)), ptr(sample), ptr(pred), stream_ptr()),
              "p_sample")
        return {"sample": sample, "pred_xstart": pred}

    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                  model_kwargs=None, device=None, progress=False, step_noise=None):
        device = device if device is not None else self.tab.device
        img = noise if noise is not None else torch.randn(*shape, device=device)
        indices = list(range(self.num_timesteps))[::-1]
        if progress:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        for k, i in enumerate(indices):
            t = torch.tensor([i] * shape[0], device=device)
            with torch.no_grad():
                out = self.p_sample(model, img, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
                                    model_kwargs=model_kwargs, noise=None if step_noise is None else step_noise[k])
            yield out
            img = out["sample"]

    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                      device=None, progress=False, step_noise=None):
        """Reference signature (gaussian_diffusion.py:423); ``step_noise[k]`` optionally fixes the k-th per-step draw."""
        final = None
        for final in self.p_sample_loop_progressive(model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device,
                                                    progress, step_noise):
            pass
        return final["sample"]


    # ------------------------------------------------------------------ DDIM (gaussian_diffusion.py:513-680)
    def sample_step(self, x, model_output, t, mode, noise=None, eta=0.0, clip_denoised=True, cfg_scale=None, n_guided=3, sample=None,
                    sample_dup=None, pred_xstart=None):
        """One sfron_dit_sample_step launch.  x [n, C, ...], t int64 [n] (table indices, per row), model_output [n, 2C, ...], or
        [2n, 2C, ...] with ``cfg_scale`` given (row i conditional, row i + n null: the guidance of forward_with_cfg on the first
        ``n_guided`` epsilon channels).  mode "ddpm" | "ddim" | "ddim_reverse".  sample (may be x) / sample_dup / pred_xstart: output
        tensors, sample allocated when None.  Returns sample."""
        n, c = x.shape[0], x.shape[1]
        guided = cfg_scale is not None
        assert model_output.shape[0] == (2 * n if guided else n) and model_output.shape[1] == 2 * c
        if sample is None:
            sample = torch.empty_like(x)
        check(_lib.lib().sfron_dit_sample_step(ptr(x), ptr(model_output), ptr(t), ptr(self.sampler_tab), ptr(noise), n, c, x[0, 0].numel(),
                                               int(guided), int(n_guided), float(cfg_scale) if guided else 1.0, _STEP_MODES[mode],
                                               float(eta), int(bool(clip_denoised)), ptr(sample), ptr(sample_dup), ptr(pred_xstart),
                                               stream_ptr()), f"dit_sample_step({mode})")
        return sample

    def _ddim_step(self, mode, model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, eta, noise):
        if denoised_fn is not None or cond_fn is not None:
            raise NotImplementedError("denoised_fn / cond_fn are not used by the unlearning scripts")
        x = x.contiguous().float()
        t = t.contiguous()
        model_output = self._wrap_model(model)(x, t, **(model_kwargs or {}))
        if isinstance(model_output, tuple):
            model_output = model_output[0]
        n, c = x.shape[0], x.shape[1]
        assert model_output.shape == (n, 2 * c, *x.shape[2:])
        if mode == "ddim" and noise is None and eta != 0.0:
            noise = torch.randn_like(x)
        pred = torch.empty_like(x)
        mo = model_output.contiguous().float()                              # named: temporaries must outlive the launch
        nz = None if noise is None or mode == "ddim_reverse" else noise.contiguous().float()
        sample = self.sample_step(x, mo, t, mode, noise=nz, eta=eta, clip_denoised=clip_denoised, pred_xstart=pred)
        return {"sample": sample, "pred_xstart": pred}

    def ddim_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, eta=0.0, noise=None):
        """Reference signature (gaussian_diffusion.py:513); ``noise`` (optional) replaces the reference's ``th.randn_like(x)`` draw.  With
        eta == 0 and no ``noise`` nothing is drawn (the reference draws and multiplies by sigma = 0)."""
        return self._ddim_step("ddim", model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, eta, noise)

    def ddim_reverse_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, eta=0.0):
        """Reference signature (gaussian_diffusion.py:562): x_{t+1} from x_t by the reverse ODE."""
        assert eta == 0.0, "Reverse ODE only for deterministic path"
        return self._ddim_step("ddim_reverse", model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, eta, None)

    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                                     device=None, progress=False, eta=0.0, step_noise=None):
        device = device if device is not None else self.tab.device
        assert isinstance(shape, (tuple, list))
        img = noise if noise is not None else torch.randn(*shape, device=device)
        indices = list(range(self.num_timesteps))[::-1]
        if progress:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        for k, i in enumerate(indices):
            t = torch.tensor([i] * shape[0], device=device)
            with torch.no_grad():
                out = self.ddim_sample(model, img, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
                                       model_kwargs=model_kwargs, eta=eta, noise=None if step_noise is None else step_noise[k])
            yield out
            img = out["sample"]

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                         device=None, progress=False, eta=0.0, step_noise=None):
        """Reference signature (gaussian_diffusion.py:600); ``step_noise[k]`` optionally fixes the k-th per-step draw."""
        final = None
        for final in self.ddim_sample_loop_progressive(model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device,
                                                       progress, eta, step_noise):
            pass
        return final["sample"]


    # ------------------------------------------------------------------ likelihood evaluation (gaussian_diffusion.py:682-713,789-858)
    def bpd_step(self, x_start, model_output, t, clip_denoised=True, x_t=None, noise=None, vb=None, xstart_mse=None, mse=None, col=0,
                 step=None, pred_xstart=None, next_noise=None, order=None, next_xt=None):
        """One sfron_dit_bpd_step launch.  x_start [n, C, ...], model_output [n, 2C, ...], t int64 [n] (table indices, per row); x_t given,
        or recomputed from ``noise`` (sfron_q_sample's bits).  vb / xstart_mse / mse: [n, ld] fp32 matrices whose column ``col`` (or the
        device counter ``step``) receives the terms; vb is allocated as [n, 1] when None.  next_xt (with next_noise, order, step): the
        launch also writes q_sample of step order[step + 1] there.  Returns vb."""
        n, c = x_start.shape[0], x_start.shape[1]
        assert model_output.shape[0] == n and model_output.shape[1] == 2 * c and model_output.is_contiguous() and x_start.is_contiguous()
        if vb is None:
            vb = torch.empty(n, 1, dtype=torch.float32, device=x_start.device)
        ld = vb.shape[1]
        assert all(m is None or (m.shape == vb.shape and m.is_contiguous()) for m in (vb, xstart_mse, mse))
        check(_lib.lib().sfron_dit_bpd_step(ptr(x_start), ptr(x_t), ptr(noise), ptr(model_output), ptr(t), ptr(self.tab), self.num_timesteps,
                                            n, c, x_start[0, 0].numel(), int(bool(clip_denoised)), ptr(vb), ptr(xstart_mse), ptr(mse), ld,
                                            ptr(step), int(col), ptr(pred_xstart), ptr(next_noise), ptr(order),
                                            0 if order is None else order.numel(), ptr(next_xt), stream_ptr()), "dit_bpd_step")
        return vb

    def _vb_terms_bpd(self, model, x_start, x_t, t, clip_denoised=True, model_kwargs=None):
        """Reference signature (gaussian_diffusion.py:682): {"output": [N] bits per dimension (the KL term, or the decoder NLL where
        t == 0), "pred_xstart"}.  ``t`` is per row; the model sees the original timesteps of a respaced process."""
        x_start, x_t = x_start.contiguous().float(), x_t.contiguous().float()
        t = t.contiguous()
        model_output = self._wrap_model(model)(x_t, t, **(model_kwargs or {}))
        if isinstance(model_output, tuple):
            model_output = model_output[0]
        n, c = x_t.shape[0], x_t.shape[1]
        assert t.shape == (n,) and model_output.shape == (n, 2 * c, *x_t.shape[2:])
        mo = model_output.contiguous().float()                              # named: temporaries must outlive the launch
        pred = torch.empty_like(x_t)
        vb = self.bpd_step(x_start, mo, t, clip_denoised, x_t=x_t, pred_xstart=pred)
        return {"output": vb.view(n), "pred_xstart": pred}

    def _prior_bpd(self, x_start):
        """Reference signature (gaussian_diffusion.py:789): the prior KL term in bits per dimension, [N]."""
        x_start = x_start.contiguous().float()
        n = x_start.shape[0]
        ac = self.tables["alphas_cumprod"][-1]
        out = torch.empty(n, dtype=torch.float32, device=x_start.device)
        check(_lib.lib().sfron_dit_prior_bpd(ptr(x_start), n, x_start.shape[1], x_start[0, 0].numel(), float(np.float32(np.sqrt(ac))),
                                             float(np.float32(np.log(1.0 - ac))), ptr(out), stream_ptr()), "dit_prior_bpd")
        return out

    def _bpd_result(self, x_start, vb, xstart_mse, mse):
        prior_bpd = self._prior_bpd(x_start)
        return {"total_bpd": vb.sum(dim=1) + prior_bpd, "prior_bpd": prior_bpd, "vb": vb, "xstart_mse": xstart_mse, "mse": mse}

    @torch.no_grad()
    def calc_bpd_loop(self, model, x_start, clip_denoised=True, model_kwargs=None, generator=None, step_noise=None):
        """Reference signature (gaussian_diffusion.py:805) for any callable model: total_bpd [N], prior_bpd [N], vb / xstart_mse / mse
        [N, T] with column 0 the term of t = T - 1.  Step k's noise is ``step_noise[k]`` if given, else drawn from ``generator`` (None:
        ``randn_like(x_start)``, as the reference draws).  One sfron_q_sample, one model call and one sfron_dit_bpd_step per step."""
        x_start = x_start.contiguous().float()
        n, T, dev = x_start.shape[0], self.num_timesteps, x_start.device
        vb, xstart_mse, mse = (torch.empty(n, T, dtype=torch.float32, device=dev) for _ in range(3))
        wrapped = self._wrap_model(model)
        for k, i in enumerate(list(range(T))[::-1]):
            t = torch.tensor([i] * n, device=dev)
            if step_noise is not None:
                noise = step_noise[k].to(dev, torch.float32).contiguous()
            elif generator is not None:
                noise = torch.randn(x_start.shape, generator=generator, device=generator.device).to(dev)
            else:
                noise = torch.randn_like(x_start)
            x_t = self.q_sample(x_start, t, noise)
            model_output = wrapped(x_t, t, **(model_kwargs or {}))
            if isinstance(model_output, tuple):
                model_output = model_output[0]
            assert model_output.shape == (n, 2 * x_start.shape[1], *x_start.shape[2:])
            mo = model_output.contiguous().float()
            self.bpd_step(x_start, mo, t, clip_denoised, noise=noise, vb=vb, xstart_mse=xstart_mse, mse=mse, col=k)
        return self._bpd_result(x_start, vb, xstart_mse, mse)


class _DitLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model_output, diff, x_start, t, noise):
        mse, vb, d_out = diff.loss_fwd_bwd(model_output.contiguous(), x_start, t, noise, 1.0)
        ctx.save_for_backward(d_out)
        ctx.c = model_output.shape[1] // 2
        loss = mse + vb
        ctx.mark_non_differentiable(mse, vb)
        return mse, vb, loss

    @staticmethod
    def backward(ctx, g_mse, g_vb, g_loss):
        (d_out,) = ctx.saved_tensors
        # per-sample upstream weights; d_out already holds d loss_i / d out for unit weights
        g = g_loss.view(-1, *([1] * (d_out.dim() - 1)))
        return d_out * g, None, None, None, None


def create_diffusion(timestep_respacing="", diffusion_steps=1000, device="cuda", **unused):
    """DiT/diffusion/__init__.py:10-46 for the defaults the unlearning scripts use (linear schedule, learn_sigma, MSE)."""
    use = None if timestep_respacing in ("", None) else space_timesteps(diffusion_steps, timestep_respacing)
    return GaussianDiffusion(diffusion_steps, device=device, use_timesteps=use)
