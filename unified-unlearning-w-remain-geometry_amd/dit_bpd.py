"""Native DiT likelihood evaluation: the variational bound in bits per dimension of given latents under given labels.

``DiTBpdEvaluator`` is ``diffusion.calc_bpd_loop(model.forward, x_start, model_kwargs=dict(y=y))`` of the reference
(DiT/diffusion/gaussian_diffusion.py:805-858) with nothing on the host per step but the noise draw: one engine forward pass that reads x_t
and t from persistent device buffers, one sfron_dit_bpd_step (this step's three terms into column k of the [n, T] matrices, and q_sample of
the NEXT step into the engine's input buffer) and one sfron_dit_sampler_advance (the step counter and both timestep vectors from device
tables).  ``evaluate_bpd`` runs it over a ``latents.LatentCache`` class by class: after an unlearning run the bound on the forget class's
latents should rise and the bound on the remain classes' stay put -- a check that needs no outside network.

Unpinned boundary: the reference draws every step's noise from the global RNG of its device; draws here come from a caller's generator (or
the global one) and are not pinned against the reference's CUDA draws.  Out of scope: guidance inside the evaluation, cond_fn /
denoised_fn, the timestep samplers (LossAwareSampler), HIP-graph capture, and data-parallel evaluation (``evaluate_bpd`` runs on one rank).
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .diffusion import create_diffusion
from .dit_sample import _OwnEngine


class DiTBpdEvaluator(_OwnEngine):
    """``evaluate(x_start, y)`` -> the dict of ``calc_bpd_loop``: total_bpd [n], prior_bpd [n], vb / xstart_mse / mse [n, T] (column 0 is
    t = T - 1), bit-equal to ``diffusion.calc_bpd_loop(model.forward, ...)`` on the same noise with the model in eval mode.

    The batch is the n rows with the caller's labels (the null label ``model.num_classes`` is allowed), unguided, no label dropout.  The
    model runs on an engine of the evaluator's own over the model's parameter arenas (the e4m3 shadow too, when the runner armed it), as
    in ``DiTSampler``: a sweep the runner left in flight is drained first, and ``model.engine``, its batch size and the model's train /
    eval mode are never touched.  The engine is kept between calls of the same batch size; ``close()`` releases it."""

    def __init__(self, model, diffusion, clip_denoised=True):
        if not model.learn_sigma:
            raise NotImplementedError("the evaluation needs a learn_sigma model (2C output channels)")
        self.model, self.diffusion, self.clip_denoised = model, diffusion, bool(clip_denoised)

    @torch.no_grad()
    def evaluate(self, x_start, y, generator=None, step_noise=None):
        """x_start [n, C, H, W] fp32 latents, y [n] labels.  Step k's noise ([n, C, H, W]) is ``step_noise[k]`` if given, else drawn from
        ``generator`` (None: the global RNG of the device), in step order -- the stream ``calc_bpd_loop`` consumes."""
        model, diff = self.model, self.diffusion
        eng = model.engine
        dev = eng.device
        n, T = x_start.shape[0], diff.num_timesteps
        eng.drain_sweep()
        own = self._engine(n)
        try:
            x0 = x_start.to(dev, torch.float32).contiguous()
            y = y.to(dev, torch.int64).view(-1).contiguous()
            if y.numel() != n or x0.dim() != 4 or x0.shape[1] != model.in_channels:
                raise ValueError(f"x_start must be [n, {model.in_channels}, H, W] with n labels, got {tuple(x0.shape)} and {y.numel()} labels")
            if int(y.min()) < 0 or int(y.max()) > model.num_classes:
                raise ValueError(f"labels must be in [0, {model.num_classes}] ({model.num_classes} is the null label)")

            def draw(k):
                if step_noise is not None:
                    return step_noise[k].to(dev, torch.float32).contiguous()
                if generator is not None:
                    return torch.randn(x0.shape, generator=generator, device=generator.device).to(dev)
                return torch.randn(x0.shape, device=dev)
            xbuf = torch.empty_like(x0)
            out = torch.empty(own.out_shape, dtype=torch.float32, device=dev)
            vb, xstart_mse, mse = (torch.empty(n, T, dtype=torch.float32, device=dev) for _ in range(3))
            order = torch.arange(T - 1, -1, -1, dtype=torch.int64, device=dev)
            tmap = diff.map_tensor.to(dev).contiguous()
            t_idx = torch.full((n,), T - 1, dtype=torch.int64, device=dev)
            t_model = torch.full((n,), int(diff.timestep_map[T - 1]), dtype=torch.int64, device=dev)
            step = torch.zeros(1, dtype=torch.int32, device=dev)
            L = _lib.lib()
            noise = draw(0)
            check(L.sfron_q_sample(ptr(x0), ptr(noise), ptr(t_idx), ptr(diff.tab), n, x0.numel() // n, ptr(xbuf), stream_ptr()), "q_sample")
            for k in range(T):
                nxt = draw(k + 1) if k + 1 < T else noise           # the last step writes no x_t: any valid tensor
                own.forward(xbuf, t_model, y, None, out=out)
                diff.bpd_step(x0, out, t_idx, self.clip_denoised, noise=noise, vb=vb, xstart_mse=xstart_mse, mse=mse, step=step,
                              next_noise=nxt, order=order, next_xt=xbuf)
                check(L.sfron_dit_sampler_advance(ptr(order), ptr(tmap), T, tmap.numel(), ptr(step), ptr(t_idx), n, ptr(t_model), n,
                                                  stream_ptr()), "dit_sampler_advance")
                noise = nxt
            return diff._bpd_result(x0, vb, xstart_mse, mse)
        except BaseException:
            self.close()
            raise


@torch.no_grad()
def evaluate_bpd(model, cache, forget_class, *, timestep_respacing="", batch=32, max_per_class=None, generator=None, scale=0.18215):
    """The bound per class over a ``latents.LatentCache``: every class's first ``max_per_class`` (None: all) cached posteriors, in shard
    order, sampled as the latent loader samples them (sfron_latent_sample: mean + exp(0.5 logvar) * eps, times ``scale``, eps from
    ``generator``), evaluated in batches of at most ``batch`` under the class's own label with ``clip_denoised=True``.  Per batch the
    generator gives the posterior eps first, then the T step noises.  Returns ``dict(per_class={index: mean total_bpd}, count={index: n},
    forget=mean over the forget class's latents, remain=mean over every other latent)``.  One rank; no collective is issued."""
    fc = int(forget_class)
    forget, remain = cache.split(fc)
    if not forget or not remain:
        raise ValueError(f"forget_class {forget_class} is not a class of the cache, or the cache has no other class")
    dev = model.engine.device
    diffusion = create_diffusion(timestep_respacing, device=dev)
    ev = DiTBpdEvaluator(model, diffusion, clip_denoised=True)
    g = generator
    sums, counts = {}, {}
    try:
        for name in cache.classes:
            ci = cache.index[name]["index"]
            total = cache.index[name]["count"] if max_per_class is None else min(int(max_per_class), cache.index[name]["count"])
            shard = cache.shard(name)
            acc = 0.0
            for lo in range(0, total, int(batch)):
                rows = np.array(shard[lo:min(lo + int(batch), total)], dtype=np.float32)          # a copy: the map is read-only
                mom = torch.from_numpy(rows).to(dev).contiguous()
                n, c2, h, w = mom.shape
                shape = (n, c2 // 2, h, w)
                eps = (torch.randn(shape, generator=g, device=g.device).to(dev) if g is not None else torch.randn(shape, device=dev))
                x0 = torch.empty(shape, dtype=torch.float32, device=dev)
                check(_lib.lib().sfron_latent_sample(ptr(mom), ptr(eps), n, c2 // 2, h * w, float(scale), ptr(x0), stream_ptr()),
                      "latent_sample")
                y = torch.full((n,), ci, dtype=torch.int64, device=dev)
                acc += float(ev.evaluate(x0, y, generator=g)["total_bpd"].double().sum())
            sums[ci], counts[ci] = acc, total
    finally:
        ev.close()
    rem = [c for c in sums if c != fc]
    n_rem = sum(counts[c] for c in rem)
    return dict(per_class={c: sums[c] / counts[c] for c in sorted(sums) if counts[c]}, count={c: counts[c] for c in sorted(sums)},
                forget=sums[fc] / counts[fc] if counts[fc] else float("nan"),
                remain=sum(sums[c] for c in rem) / n_rem if n_rem else float("nan"))
