"""Native DiT sampling: the guided DDPM / DDIM loop on the GPU and the two sample drivers of the reference.

``DiTSampler`` is the loop of DiT/sample.py / sample_ddp.py / forget.py:114-145 (``diffusion.p_sample_loop(model.forward_with_cfg, ...)``,
or ``ddim_sample_loop``) with nothing on the host per step: one engine forward pass that reads x_t and t from persistent device buffers, one
sfron_dit_sample_step (guidance + update, the new state written into both halves of the x_t buffer) and one sfron_dit_sampler_advance (the
step counter and both timestep vectors from device tables).  ``sample`` is DiT/sample.py:50-76, ``sample_fid`` DiT/sample_ddp.py:45-146 with
its helpers ``fid_plan``, ``sample_folder_name`` and ``create_npz_from_sample_folder``.

Unpinned boundaries: the reference draws z, y and every step's noise from the CUDA global RNG, which no ROCm run reproduces -- draws
here come from a caller's generator (or the global one) and are NOT pinned against the reference; torchvision's save_image is restated
by ``images.make_grid_u8`` (torchvision is not part of this project's environment), as elsewhere.
"""
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .diffusion import create_diffusion

DEFAULT_CLASS_LABELS = (207, 360, 387, 974, 88, 979, 417, 279)       # DiT/sample.py:47


class _OwnEngine:
    """A forward-only engine of the holder's own over the arenas of ``self.model``'s engine: what DiTSampler and
    dit_bpd.DiTBpdEvaluator run the model on."""
    _eng = _eng_key = None

    def _engine(self, rows):
        """The holder's own engine at batch ``rows`` over the arenas of the model's CURRENT engine (rebuilt when the batch size, the
        arenas or the armed fp8 state changed since the last call)."""
        from .engine import DitEngine
        eng = self.model.engine
        key = (rows, eng.params.data_ptr(), eng.grads.data_ptr(), id(eng.fp8), eng.fp8_wgrad is not None)
        if self._eng is None or self._eng_key != key:
            self.close()
            samp = DitEngine(rows, share=eng, grads=eng.grads, **eng._ctor)       # forward only: the gradient arena is never written
            try:
                samp._share_fp8(eng)
            except Exception:
                samp.close()
                raise
            self._eng, self._eng_key = samp, key
        return self._eng

    def close(self):
        """Release the holder's engine (idempotent)."""
        if self._eng is not None:
            self._eng.close()
        self._eng = self._eng_key = None

    def __del__(self):
        try:
            self.close()
        except Exception:          # interpreter shutdown
            pass


class DiTSampler(_OwnEngine):
    """Guided sampling of a ``dit.DiT`` at batch 2n (row i conditional, row i + n the null label), or unguided at batch n for
    ``cfg_scale <= 1.0`` (the choice of sample_ddp.py:114-122: ``model.forward`` instead of ``forward_with_cfg``).

    mode "ddpm": ancestral steps, bit-equal on the first n rows to ``p_sample_loop(model.forward_with_cfg, ...)``; "ddim":
    ``ddim_sample`` steps with ``eta``.  Guidance covers the first ``n_guided`` epsilon channels (the reference guides three).

    The model runs on an engine of its own over the model's parameter arenas (the e4m3 shadow too, when the runner armed it); a sweep the
    runner left in flight is drained first.  ``model.engine``, its batch size and the model's train / eval mode are never touched: the
    sampler calls its own engine with no label dropout, which is what ``model.eval()`` selects.  That engine (its workspace, side stream
    and events) is kept between ``sample`` calls of the same batch size -- building it costs about a millisecond of host time with the
    GPU idle, a tenth of a millisecond per step of a 10-step run -- and is released by ``close()`` or with the sampler.

    No HIP-graph capture: the DiT forward pass is one C call that issues its launches back to back, and DESIGN section 7 measured that
    replaying it from a graph gains nothing; what the sampler removes is the host work between the passes."""

    def __init__(self, model, diffusion, cfg_scale, n_guided=3, mode="ddpm", eta=0.0, clip_denoised=False):
        if mode not in ("ddpm", "ddim"):
            raise ValueError(f"mode must be 'ddpm' or 'ddim', got {mode!r}")
        if not 0 <= int(n_guided) <= model.in_channels:
            raise ValueError(f"n_guided must be in [0, {model.in_channels}], got {n_guided}")
        if not model.learn_sigma:
            raise NotImplementedError("the sampler needs a learn_sigma model (2C output channels)")
        self.model, self.diffusion = model, diffusion
        self.cfg_scale, self.n_guided, self.mode, self.eta = float(cfg_scale), int(n_guided), mode, float(eta)
        self.clip_denoised = bool(clip_denoised)
        self.guided = self.cfg_scale > 1.0

    def needs_noise(self):
        return self.mode == "ddpm" or self.eta != 0.0

    @torch.no_grad()
    def sample(self, z, y, generator=None, step_noise=None):
        """z [n, C, H, W] fp32, y [n] class labels -> the first-half latents [n, C, H, W] after every step of the (respaced) process.
        Per-step noise: ``step_noise[k]`` if given, else drawn from ``generator`` (None: the global RNG of the device) with the shape
        of the engine batch ([2n, ...] when guided) -- its first n rows are used, so for a given generator the stream equals what
        ``p_sample_loop(..., step_noise=images._StepNoise(...))`` consumes."""
        model, diff = self.model, self.diffusion
        eng = model.engine
        dev = eng.device
        n = z.shape[0]
        rows = 2 * n if self.guided else n
        T = diff.num_timesteps
        eng.drain_sweep()
        samp = self._engine(rows)
        try:
            z = z.to(dev, torch.float32)
            y = y.to(dev, torch.int64).view(-1)
            if y.numel() != n or z.dim() != 4 or z.shape[1] != model.in_channels:
                raise ValueError(f"z must be [n, {model.in_channels}, H, W] with n labels, got {tuple(z.shape)} and {y.numel()} labels")
            xbuf = torch.empty(rows, *z.shape[1:], dtype=torch.float32, device=dev)
            ybuf = torch.full((rows,), model.num_classes, dtype=torch.int64, device=dev)
            xbuf[:n].copy_(z)
            ybuf[:n].copy_(y)
            if self.guided:
                xbuf[n:].copy_(z)
            out = torch.empty(samp.out_shape, dtype=torch.float32, device=dev)
            order = torch.arange(T - 1, -1, -1, dtype=torch.int64, device=dev)
            tmap = diff.map_tensor.to(dev).contiguous()
            t_idx = torch.full((n,), T - 1, dtype=torch.int64, device=dev)
            t_model = torch.full((rows,), int(diff.timestep_map[T - 1]), dtype=torch.int64, device=dev)
            step = torch.zeros(1, dtype=torch.int32, device=dev)
            x, dup = xbuf[:n], (xbuf[n:] if self.guided else None)
            L = _lib.lib()
            for k in range(T):
                noise = None
                if self.needs_noise():
                    if step_noise is not None:
                        noise = step_noise[k].to(dev, torch.float32)
                    elif generator is not None:
                        noise = torch.randn(xbuf.shape, generator=generator, device=generator.device).to(dev)
                    else:
                        noise = torch.randn(xbuf.shape, device=dev)
                    noise = noise[:n].contiguous()
                samp.forward(xbuf, t_model, ybuf, None, out=out)
                diff.sample_step(x, out, t_idx, self.mode, noise=noise, eta=self.eta, clip_denoised=self.clip_denoised,
                                 cfg_scale=self.cfg_scale if self.guided else None, n_guided=self.n_guided, sample=x, sample_dup=dup)
                check(L.sfron_dit_sampler_advance(ptr(order), ptr(tmap), T, tmap.numel(), ptr(step), ptr(t_idx), n, ptr(t_model), rows,
                                                  stream_ptr()), "dit_sampler_advance")
            return x.clone()
        except BaseException:
            self.close()
            raise


@torch.no_grad()
def sample(model, diffusion_steps=250, class_labels=DEFAULT_CLASS_LABELS, cfg_scale=4.0, decoder=None, path="sample.png", generator=None,
           mode="ddpm"):
    """DiT/sample.py:50-76: one guided sample per class label (null label ``model.num_classes``, clip_denoised=False) through
    ``create_diffusion(str(diffusion_steps))``, decoded (``samples / 0.18215``) and written as one grid:
    save_image(nrow=4, normalize=True, value_range=(-1, 1)).  Returns the uint8 grid [Hc, Wc, 3] on the device.  Every draw comes from
    ``generator`` (None: the device's global RNG); unpinned against the reference's CUDA draws."""
    from .images import write_png
    if decoder is None:
        raise ValueError("sample needs a vae.VAEDecoder (decoder=...)")
    dev = model.engine.device
    n = len(class_labels)
    size = model.engine._ctor["input_size"]
    diffusion = create_diffusion(str(diffusion_steps), device=dev)
    shape = (n, model.in_channels, size, size)
    if generator is not None:
        z = torch.randn(shape, generator=generator, device=generator.device).to(dev)
    else:
        z = torch.randn(*shape, device=dev)
    y = torch.tensor(list(class_labels), device=dev)
    latents = DiTSampler(model, diffusion, cfg_scale, mode=mode, clip_denoised=False).sample(z, y, generator=generator)
    grid = decoder.decode_u8(latents, 0.18215, "save_image", nrow=4, padding=2, value_range=(-1.0, 1.0))
    write_png(grid, path)
    return grid


def fid_plan(num_fid_samples, per_proc_batch_size, world_size, rank):
    """sample_ddp.py:94-138 as a pure function: dict(total_samples, samples_per_rank, iterations, global_batch, index) where
    ``index(i, j)`` is the file index of sample i of iteration j on this rank (i * world_size + rank + j * global_batch)."""
    n = int(per_proc_batch_size)
    if n < 1 or world_size < 1 or not 0 <= rank < world_size or num_fid_samples < 1:
        raise ValueError("fid_plan needs positive sizes and 0 <= rank < world_size")
    global_batch = n * world_size
    total_samples = int(math.ceil(num_fid_samples / global_batch) * global_batch)
    assert total_samples % world_size == 0, "total_samples must be divisible by world_size"
    per_rank = int(total_samples // world_size)
    assert per_rank % n == 0, "samples_needed_this_gpu must be divisible by the per-GPU batch size"
    iterations = int(per_rank // n)

    def index(i, j):
        return i * world_size + rank + j * global_batch
    return dict(total_samples=total_samples, samples_per_rank=per_rank, iterations=iterations, global_batch=global_batch, index=index)


def sample_folder_name(model_name, ckpt, image_size, vae, cfg_scale, global_seed):
    """sample_ddp.py:84-88."""
    model_string_name = model_name.replace("/", "-")
    ckpt_string_name = os.path.basename(ckpt).replace(".pt", "") if ckpt else "pretrained"
    return f"{model_string_name}-{ckpt_string_name}-size-{image_size}-vae-{vae}-cfg-{cfg_scale}-seed-{global_seed}"


def create_npz_from_sample_folder(sample_dir, num=50_000):
    """sample_ddp.py:28-42: ``{sample_dir}.npz`` with ``arr_0`` uint8 [num, H, W, 3] from ``{i:06d}.png``, i < num (Pillow reads)."""
    from PIL import Image
    samples = []
    for i in range(num):
        with Image.open(f"{sample_dir}/{i:06d}.png") as im:
            samples.append(np.asarray(im).astype(np.uint8))
    samples = np.stack(samples)
    assert samples.shape == (num, samples.shape[1], samples.shape[2], 3)
    npz_path = f"{sample_dir}.npz"
    np.savez(npz_path, arr_0=samples)
    return npz_path


def _barrier():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        dist.barrier()


@torch.no_grad()
def sample_fid(model, decoder, *, num_fid_samples, per_proc_batch_size, num_classes, cfg_scale=1.5, num_sampling_steps=250, image_size,
               sample_dir, global_seed=0, rank=0, world_size=1, mode="ddpm"):
    """DiT/sample_ddp.py:45-146 for one process per GPU: ``fid_plan`` iterations of ``per_proc_batch_size`` samples (random labels,
    guided when cfg_scale > 1.0, clip_denoised=False), decoded with ``decode_u8(mode="trunc")`` (the bytes of :132), one
    ``{index:06d}.png`` per sample under ``sample_dir``; rank 0 then builds ``{sample_dir}.npz`` from the first ``num_fid_samples`` files.
    When torch.distributed is initialised it barriers where the reference does (after the folder exists, before and after the .npz);
    no other collective is issued.  Returns the .npz path on rank 0, None elsewhere.

    The per-rank generator is seeded ``global_seed * world_size + rank``; z, y and every step's noise come from it.  The reference
    draws from the CUDA global RNG, which no ROCm run reproduces: draws are per-generator here and unpinned against the reference."""
    from .images import write_png
    assert cfg_scale >= 1.0, "In almost all cases, cfg_scale be >= 1.0"
    dev = model.engine.device
    plan = fid_plan(num_fid_samples, per_proc_batch_size, world_size, rank)
    g = torch.Generator(device=dev).manual_seed(int(global_seed) * int(world_size) + int(rank))
    diffusion = create_diffusion(str(num_sampling_steps), device=dev)
    sampler = DiTSampler(model, diffusion, cfg_scale, mode=mode, clip_denoised=False)
    if rank == 0:
        os.makedirs(sample_dir, exist_ok=True)
    _barrier()
    n, latent = int(per_proc_batch_size), image_size // 8
    for j in range(plan["iterations"]):
        z = torch.randn(n, model.in_channels, latent, latent, generator=g, device=dev)
        y = torch.randint(0, num_classes, (n,), generator=g, device=dev)
        u8 = decoder.decode_u8(sampler.sample(z, y, generator=g), 0.18215, "trunc").cpu()
        for i in range(n):
            write_png(u8[i], os.path.join(sample_dir, f"{plan['index'](i, j):06d}.png"))
    _barrier()
    path = create_npz_from_sample_folder(sample_dir, num_fid_samples) if rank == 0 else None
    _barrier()
    return path
