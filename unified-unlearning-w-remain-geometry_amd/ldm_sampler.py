"""The host layer the ldm samplers (ddim.DDIMSampler, plms.PLMSSampler) share: the schedule tables exactly as the reference's util.py
leaves them, the refusal of arguments that are not built, the once-per-call context on the native UNet, the model call at batch 2B, the
2 GiB batch chunking and the bookkeeping of a sampling loop.  A sampler adds its loop body, its step scalars and its update launch.
"""
import contextlib

import numpy as np
import torch

from . import _lib
from .forward_net import LIMIT


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


class _SliceNoise:
    """noise[k][lo:hi] of a chunked run"""

    def __init__(self, src, lo, hi):
        self.src, self.lo, self.hi = src, lo, hi

    def __getitem__(self, k):
        return self.src[k][self.lo:self.hi]


class LDMSampler(object):
    # Per sampler: {argument as an entry point spells it: the only value that passes}.  _refuse looks every one of these names up in the
    # entry point's locals(), so an entry point whose parameter merely shares a name with a refused argument (DDIMSampler.stochastic_encode
    # takes an ``x0``) must hand _refuse a dict of its own instead of locals().
    REFUSED = {}
    _REPORTED = {"quantize_denoised": "quantize_x0"}

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
        # host-side tables (fp32 tensor / float64 array as the reference leaves them): step_coefficients reads one entry per step
        self.ddim_sigmas, self.ddim_alphas, self.ddim_alphas_prev = sigmas, alphas, alphas_prev
        self.ddim_sqrt_one_minus_alphas = self._sqrt_one_minus(alphas)

    # ------------------------------------------------------------------------------------------------ guards and plumbing
    def _refuse(self, args):
        """args: an entry point's arguments by name (its ``locals()``); every one that REFUSED lists must hold the value that passes.
        ``sample`` adds the one name it reads from its **kwargs, ``ddim_use_original_steps``; whatever else they hold is ignored."""
        for name, unset in self.REFUSED.items():
            if name in args and (args[name] is not None if unset is None else type(unset)(args[name]) != unset):
                raise NotImplementedError(f"{type(self).__name__}: `{self._REPORTED.get(name, name)}` is not built (DESIGN.md section 7)")

    def _unet(self):
        u = getattr(getattr(self.model, "model", None), "diffusion_model", None)
        return u if hasattr(u, "prepare_context") else None

    @staticmethod
    def _cond_tensor(c):
        if isinstance(c, dict):
            c = c[list(c.keys())[0]]
            c = torch.cat(c, 1) if isinstance(c, (list, tuple)) else c
        return c

    def _guidance(self, cond, uc, scale, c_in=None):
        """(guided, the context of a model call: ``c_in`` where the loop prepared one, else unconditional rows first when guided)"""
        guided = not (uc is None or scale == 1.0)
        if c_in is None:
            c_in = torch.cat([self._cond_tensor(uc), self._cond_tensor(cond)]) if guided else self._cond_tensor(cond)
        return guided, c_in

    @contextlib.contextmanager
    def _conditioning(self, cond, uc, scale):
        """The context one loop hands to every step: unconditional rows first when guided; prepared once on the native UNet."""
        c_in = self._guidance(cond, uc, scale)[1]
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

    def _model_output(self, x, t, c_in, guided):
        """The model's contiguous fp32 output; guided: ONE call at batch 2B, unconditional rows first."""
        if guided:
            x, t = torch.cat([x] * 2), torch.cat([t] * 2)
        return self.model.apply_model(x, t, c_in).contiguous().float()

    @staticmethod
    def _halves(out, guided):
        """Device addresses (eps_uncond, eps_cond or None) of the model's output: the update reads the two halves where they are.  An
        output that is not on the GPU is an error, not an eager step.  The addresses own nothing: the caller keeps ``out`` referenced
        until the update is launched, or the allocator hands its memory to the next tensor made before the launch."""
        if not out.is_cuda:
            raise _lib.SfronError("sfron ops need GPU tensors (no CPU fallback)")
        eu = out.data_ptr()
        return eu, (eu + out.element_size() * (out.numel() // 2) if guided else None)

    def chunk_size(self, batch_size, shape):
        """Samples per run such that no operand of the UNet at batch 2B reaches 2 GiB (the library refuses those); the native UNet
        reports its widest per-sample operand, any other model is run whole."""
        unet = self._unet()
        if unet is None or not hasattr(unet, "per_sample_bytes"):
            return batch_size
        ps = 2 * unet.per_sample_bytes(shape[1], shape[2])
        if ps >= LIMIT:
            raise ValueError(f"one {shape[1]}x{shape[2]} latent needs a {ps}-byte operand at batch 2: above 2 GiB")
        return max(1, min(batch_size, (LIMIT - 1) // ps))

    # ------------------------------------------------------------------------------------------------ what every run and loop does
    def _warn_batch(self, conditioning, batch_size):
        if conditioning is not None:
            cbs = self._cond_tensor(conditioning).shape[0]
            if cbs != batch_size:
                print(f"Warning: Got {cbs} conditionings but batch-size is {batch_size}")

    def _chunked(self, run, cond, batch_size, shape, sliced, noise, **kw):
        """run(cond, (b, C, H, W), **sliced, **noise, **kw) -> (samples, intermediates) over the whole batch, or over chunks of it (as
        VAEDecoder.decode runs its batch) such that every operand at batch 2 b stays under 2 GiB.  A chunk sees rows [lo:hi] of ``cond``
        and of every tensor in ``sliced``, and noise[k][lo:hi] of every per-step source in ``noise``; ``kw`` goes to each unchanged."""
        C, H, W = shape
        n = self.chunk_size(batch_size, shape)
        if n >= batch_size:
            return run(cond, (batch_size, C, H, W), **sliced, **noise, **kw)
        cut = lambda v, lo, hi: None if v is None else self._cond_tensor(v)[lo:hi]
        outs = []
        for lo in range(0, batch_size, n):
            hi = min(batch_size, lo + n)
            outs.append(run(cut(cond, lo, hi), (hi - lo, C, H, W), **{k: cut(v, lo, hi) for k, v in sliced.items()},
                            **{k: None if v is None else _SliceNoise(v, lo, hi) for k, v in noise.items()}, **kw))
        inter = {k: [torch.cat(parts) for parts in zip(*(o[1][k] for o in outs))] for k in outs[0][1]}
        return torch.cat([o[0] for o in outs]), inter

    def _begin(self, shape, x_T, timesteps):
        """-> (device, the start image, the table's steps to walk, the intermediates holding the start)"""
        device = self.model.betas.device
        img = torch.randn(shape, device=device) if x_T is None else x_T
        if timesteps is None:
            timesteps = self.ddim_timesteps
        else:
            subset_end = int(min(timesteps / self.ddim_timesteps.shape[0], 1) * self.ddim_timesteps.shape[0]) - 1
            timesteps = self.ddim_timesteps[:subset_end]
        return device, img, timesteps, {"x_inter": [img], "pred_x0": [img]}

    @staticmethod
    def _keep(intermediates, index, total_steps, log_every_t, img, pred_x0):
        if index % log_every_t == 0 or index == total_steps - 1:
            intermediates["x_inter"].append(img)
            intermediates["pred_x0"].append(pred_x0)
