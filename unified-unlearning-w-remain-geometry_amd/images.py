"""Image-space front end: latents -> decoded uint8 images / grids -> PNG, and the unlearning loop's periodic snapshot.

``make_grid_u8`` / ``save_image`` restate torchvision.utils make_grid(nrow, padding, normalize, value_range) + save_image for fp32 NCHW
images on the GPU (one launch of sfron_rows_to_image_u8 after the layout kernel); ``sample_visualization`` is DiT/forget.py:114-145
(called every ``snapshot_every`` steps, :343-345) over the native sampler and ``vae.VAEDecoder``.  PIL writes the PNG and is imported
only there.
"""
import math
import os

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

_MODES = {"save_image": 0, "round": 1}          # include/sfron.h SFRON_IMAGE_SAVE_IMAGE / SFRON_IMAGE_ROUND

# DiT/forget.py:119-122: the classes of the snapshot grid
FORGET_CLASS_LABELS = (207, 360, 387, 972, 89, 979, 417, 279, 270, 980)


IMAGE_TRUNC = 2                                  # SFRON_IMAGE_TRUNC: the bytes of DiT/sample_ddp.py:132 ("trunc")


def image_mode(mode):
    if mode == "trunc":
        return IMAGE_TRUNC
    if mode not in _MODES:
        raise ValueError(f"mode must be one of {sorted(_MODES) + ['trunc']}, got {mode!r}")
    return _MODES[mode]


def grid_geometry(n, H, W, nrow=8, padding=2):
    """(canvas height, canvas width, xmaps, ymaps) of torchvision make_grid for n images of H x W: xmaps = min(nrow, n) columns,
    ceil(n / xmaps) rows, cells of (H + padding) x (W + padding) behind a padding-pixel outer border; n == 1 is the bare image."""
    if n < 1 or nrow < 1:
        raise ValueError("grid_geometry needs n >= 1 and nrow >= 1")
    if n == 1:
        return H, W, 1, 1
    xmaps = min(nrow, n)
    ymaps = int(math.ceil(n / xmaps))
    return ymaps * (H + padding) + padding, xmaps * (W + padding) + padding, xmaps, ymaps


def make_grid_u8(samples, nrow=8, padding=2, normalize=False, value_range=None):
    """uint8 [Hc, Wc, 3] on the device: the bytes save_image writes for make_grid(samples, nrow, padding, normalize=normalize,
    value_range=value_range).  samples: fp32 [B, 3, H, W] (any device).  normalize=False is value_range (0, 1) (save_image clamps to
    [0, 255] after * 255 + 0.5, which is the same bytes); normalize=True without a value_range takes the batch's min / max, as
    make_grid does with scale_each=False."""
    x = torch.as_tensor(samples)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"samples must be [B, 3, H, W], got {tuple(x.shape)}")
    x = x.to("cuda" if not x.is_cuda else x.device, torch.float32).contiguous()
    B, _, H, W = x.shape
    if not normalize:
        lo, hi = 0.0, 1.0
    elif value_range is None:
        lo, hi = float(x.min()), float(x.max())
    else:
        lo, hi = float(value_range[0]), float(value_range[1])
    hi = max(hi, lo + 1e-5)                  # make_grid's norm_ip divides by max(high - low, 1e-5)
    Hc, Wc = grid_geometry(B, H, W, nrow, padding)[:2]
    rows = torch.empty(B * H * W, 4, dtype=torch.float32, device=x.device)
    out = torch.empty(Hc, Wc, 3, dtype=torch.uint8, device=x.device)
    L = _lib.lib()
    check(L.sfron_nchw_to_rows_f32(ptr(x), B, 3, H * W, 4, ptr(rows), stream_ptr()), "nchw_to_rows_f32")
    check(L.sfron_rows_to_image_u8(ptr(rows), 4, B, H, W, _MODES["save_image"], lo, hi, int(nrow), int(padding), 0, B, ptr(out),
                                   stream_ptr()), "rows_to_image_u8")
    return out


def write_png(u8, path):
    """uint8 [H, W, 3] (any device) -> PNG through PIL."""
    try:
        from PIL import Image
    except ImportError as e:            # pragma: no cover - PIL is part of the documented environment
        raise ImportError("writing PNG files needs Pillow (PIL); decode_u8 / make_grid_u8 give the bytes without it") from e
    arr = u8.detach().to("cpu").contiguous().numpy()
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    Image.fromarray(arr).save(path)
    return path


def save_image(samples, path, nrow=8, padding=2, normalize=False, value_range=None):
    """torchvision.utils.save_image(samples, path, nrow=nrow, padding=padding, normalize=normalize, value_range=value_range) for fp32
    [B, 3, H, W] images; returns the uint8 grid it wrote."""
    grid = make_grid_u8(samples, nrow=nrow, padding=padding, normalize=normalize, value_range=value_range)
    write_png(grid, path)
    return grid


class _StepNoise:
    """p_sample_loop(step_noise=...) that draws step k's noise from ``generator`` when the loop asks for it (lazily, in step order)."""

    def __init__(self, shape, generator, device):
        self.shape, self.g, self.dev = shape, generator, device

    def __getitem__(self, k):
        return torch.randn(self.shape, generator=self.g, device=self.g.device).to(self.dev)


@torch.no_grad()
def sample_visualization(model, diffusion, decoder, latent_size, train_steps, checkpoint_dir, class_labels=FORGET_CLASS_LABELS,
                         cfg_scale=4.0, generator=None, nrow=5, native=False):
    """DiT/forget.py:114-145 on the GPU: guided ancestral sampling of ``class_labels`` (z doubled, null labels, clip_denoised=False),
    the first half decoded (``samples / 0.18215``), written as ``{train_steps:07d}_sample.png`` under ``checkpoint_dir`` (make_grid
    nrow=5, normalize=True, value_range=(-1, 1)).  Returns the uint8 grid [Hc, Wc, 3] on the device.

    ``generator``: every draw (z, then each step's noise) comes from it and the global RNG is left alone; None draws as the reference
    does.  The model runs on an engine of its own over the same parameter arenas, so a DiTSFRon runner's engine, workspaces, streams and
    batch size are as they were; a sweep the runner left in flight is drained first (the sampler reads the parameters).

    ``native=True`` runs the loop through ``dit_sample.DiTSampler`` (one forward pass, one sfron_dit_sample_step and one
    sfron_dit_sampler_advance per step, no host tensor per step): the same draws from ``generator`` and the same grid bytes for
    ``cfg_scale > 1`` (at or below 1 the sampler runs unguided at batch n, where the default path still mixes at batch 2n)."""
    dev = model.engine.device
    n = len(class_labels)
    if native:
        from .dit_sample import DiTSampler
        shape = (n, model.in_channels, latent_size, latent_size)
        if generator is not None:
            z = torch.randn(shape, generator=generator, device=generator.device).to(dev)
        else:
            z = torch.randn(*shape, device=dev)
        y = torch.tensor(list(class_labels), device=dev)
        try:
            samples = DiTSampler(model, diffusion, cfg_scale, clip_denoised=False).sample(z, y, generator=generator)
            grid = decoder.decode_u8(samples, 0.18215, "save_image", nrow=nrow)
        finally:
            model.train()                # what the default path leaves behind (forget.py:145)
        write_png(grid, os.path.join(checkpoint_dir, f"{train_steps:07d}_sample.png"))
        return grid
    eng = model.engine
    eng.drain_sweep()
    model.eval()                         # important! This disables randomized embedding dropout
    from .engine import DitEngine
    samp = DitEngine(2 * n, share=eng, grads=eng.grads, **eng._ctor)       # forward only: the gradient arena is never written
    samp._share_fp8(eng)
    model.engine = samp
    try:
        shape = (n, model.in_channels, latent_size, latent_size)
        if generator is not None:
            z = torch.randn(shape, generator=generator, device=generator.device).to(dev)
        else:
            z = torch.randn(*shape, device=dev)
        y = torch.tensor(list(class_labels), device=dev)
        z = torch.cat([z, z], 0)
        y_null = torch.tensor([model.num_classes] * n, device=dev)
        y = torch.cat([y, y_null], 0)
        step_noise = None if generator is None else _StepNoise(z.shape, generator, dev)
        samples = diffusion.p_sample_loop(model.forward_with_cfg, z.shape, z, clip_denoised=False,
                                          model_kwargs=dict(y=y, cfg_scale=cfg_scale), device=dev, step_noise=step_noise)
        samples = samples[:n]
        grid = decoder.decode_u8(samples, 0.18215, "save_image", nrow=nrow)
    finally:
        model.engine = eng
        samp.close()
        model.train()
    write_png(grid, os.path.join(checkpoint_dir, f"{train_steps:07d}_sample.png"))
    return grid
