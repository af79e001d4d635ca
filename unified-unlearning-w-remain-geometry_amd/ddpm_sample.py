"""The DDPM runner's sample modes over ``ddpm.DDPMSampler``: from trained weights to the PNG files a user judges forgetting by.

Mirror of DDPM/runners/diffusion.py ``sample_fid`` (:770-823), ``sample_classes`` (:670-722), ``sample_one_class`` (:724-768) and
``sample_visualization`` (:874-928), of ``create_class_labels`` (DDPM/functions/__init__.py:127-134, pinned by
tests/golden/ddpm_sample.npz) and of ``inverse_data_transform`` (DDPM/dataset/__init__.py:258-267).  The runner module and the
dataset module import torchvision, so the drivers and ``inverse_data_transform`` are restated from their text and not pinned by a
reference run.

The drivers keep the reference's bookkeeping -- ``n_rounds`` / ``n_left``, ONE running ``img_id`` across classes, the directory names --
and take what the reference reads from ``self.args`` / ``self.config`` as arguments: ``config`` needs ``data.channels``,
``data.image_size``, ``data.n_classes``, ``sampling.batch_size`` (and ``training.visualization_samples`` for the grid).  ``sampler`` is
anything with ``sample_image(x, c, cond_scale)``.  Per-image files hold the bytes of ``tvu.save_image(x[k], path, normalize=True)``:
one launch of sfron_images_normalize_u8 and one device-to-host copy per round, then PIL (``images.write_png``).
"""
import os

import torch

from . import _lib, images
from ._lib import check, ptr, stream_ptr


def create_class_labels(string, n_classes=10):
    """"1,3,5" -> ([1, 3, 5], []); "x2,x7" -> (every class but 2 and 7, [2, 7]): any "x" entry makes the list an exclusion list (entries
    without the "x" are then ignored, as in the reference)."""
    parts = string.split(",")
    if any(p.startswith("x") for p in parts):
        excluded = [int(p[1:]) for p in parts if p.startswith("x")]
        return [k for k in range(n_classes) if k not in excluded], excluded
    return [int(p) for p in parts], []


def inverse_data_transform(config, x):
    """DDPM/dataset/__init__.py:258-267: + image_mean (if the config has one), sigmoid (logit_transform) or (x + 1) / 2 (rescaled),
    clamped to [0, 1]."""
    if hasattr(config, "image_mean"):
        x = x + config.image_mean.to(x.device)[None, ...]
    if config.data.logit_transform:
        x = torch.sigmoid(x)
    elif config.data.rescaled:
        x = (x + 1.0) / 2.0
    return torch.clamp(x, 0.0, 1.0)


def images_normalize_u8(x):
    """fp32 [B, 3, H, W] -> uint8 [B, H, W, 3] on the device: image k holds the bytes of save_image(x[k], normalize=True), scaled by its
    own minimum and maximum (sfron_images_normalize_u8, one launch)."""
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"images must be [B, 3, H, W], got {tuple(x.shape)}")
    x = x.float().contiguous()
    B, _, H, W = x.shape
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=x.device)
    check(_lib.lib().sfron_images_normalize_u8(ptr(x), B, H, W, ptr(out), stream_ptr()), "images_normalize_u8")
    return out


def save_images_normalized(x, paths):
    """One PNG per image of the batch: one kernel launch, ONE device-to-host copy, then PIL per file."""
    u8 = images_normalize_u8(x).cpu()
    for k, path in enumerate(paths):
        images.write_png(u8[k], path)


def _rounds(total, batch):
    """The reference's round count and per-round sizes (n_rounds, n_left)."""
    n_rounds = total // batch if total % batch == 0 else total // batch + 1
    n_left, sizes = total, []
    for _ in range(n_rounds):
        n = batch if n_left >= batch else n_left
        sizes.append(n)
        n_left -= n
    return sizes


def _randn(shape, device, generator):
    if generator is None:
        return torch.randn(*shape, device=device)
    return torch.randn(*shape, generator=generator, device=generator.device).to(device)


def _sample_round(sampler, config, n, label, cond_scale, device, generator):
    x = _randn((n, config.data.channels, config.data.image_size, config.data.image_size), device, generator)
    c = torch.ones(n, device=device, dtype=torch.int64) * int(label)
    x = sampler.sample_image(x, c, cond_scale)
    return inverse_data_transform(config, x), c


@torch.no_grad()
def sample_fid(sampler, config, ckpt_folder, cond_scale, classes_to_generate, n_samples_per_class, device="cuda", generator=None,
               save=save_images_normalized):
    """``n_samples_per_class`` images of every class of ``classes_to_generate`` into ONE directory
    ``fid_samples_guidance_{cond_scale}[_excluded_class_a_b]`` as ``{img_id}.png``, img_id running across the classes.  Returns the
    directory."""
    classes, excluded = create_class_labels(classes_to_generate, n_classes=config.data.n_classes)
    sample_dir = f"fid_samples_guidance_{cond_scale}"
    if excluded:
        sample_dir = f"{sample_dir}_excluded_class_{'_'.join(str(i) for i in excluded)}"
    sample_dir = os.path.join(ckpt_folder, sample_dir)
    os.makedirs(sample_dir, exist_ok=True)
    img_id = 0
    for i in classes:
        for n in _rounds(n_samples_per_class, config.sampling.batch_size):
            x, _ = _sample_round(sampler, config, n, i, cond_scale, device, generator)
            save(x, [os.path.join(sample_dir, f"{img_id + k}.png") for k in range(n)])
            img_id += n
    return sample_dir


@torch.no_grad()
def sample_classes(sampler, config, ckpt_folder, cond_scale, classes_to_generate, n_samples_per_class, device="cuda", generator=None,
                   save=save_images_normalized):
    """As sample_fid into ``class_samples/<label>/{img_id}.png`` -- img_id still runs across the classes, so class 4 after 3 images of
    class 1 starts at 3.png, as the reference has it."""
    sample_dir = os.path.join(ckpt_folder, "class_samples")
    os.makedirs(sample_dir, exist_ok=True)
    classes, _ = create_class_labels(classes_to_generate, n_classes=config.data.n_classes)
    img_id = 0
    for i in classes:
        os.makedirs(os.path.join(sample_dir, str(i)), exist_ok=True)
        for n in _rounds(n_samples_per_class, config.sampling.batch_size):
            x, c = _sample_round(sampler, config, n, i, cond_scale, device, generator)
            labels = c.tolist()
            save(x, [os.path.join(sample_dir, str(labels[k]), f"{img_id + k}.png") for k in range(n)])
            img_id += n
    return sample_dir


@torch.no_grad()
def sample_one_class(sampler, config, ckpt_folder, cond_scale, class_label, device="cuda", generator=None, save=save_images_normalized,
                     total_n_samples=500):
    """500 images of one class into ``class_<label>/{img_id}.png`` (the classifier evaluation's input)."""
    sample_dir = os.path.join(ckpt_folder, "class_" + str(class_label))
    os.makedirs(sample_dir, exist_ok=True)
    img_id = 0
    for n in _rounds(total_n_samples, config.sampling.batch_size):
        x, _ = _sample_round(sampler, config, n, class_label, cond_scale, device, generator)
        save(x, [os.path.join(sample_dir, f"{img_id + k}.png") for k in range(n)])
        img_id += n
    return sample_dir


@torch.no_grad()
def sample_visualization(sampler, config, name, cond_scale, out_dir, device="cuda", generator=None, save_grid=images.save_image):
    """``training.visualization_samples`` images, the same number of every class in class order (repeat_interleave), sampled in
    ``torch.chunk`` rounds, as ONE sheet ``sample-{name}.png``: make_grid(nrow = samples per class, padding 0, normalize=True over the
    WHOLE batch).  Returns the path."""
    total = config.training.visualization_samples
    n_classes = config.data.n_classes
    assert total % n_classes == 0
    batch = config.sampling.batch_size
    n_rounds = total // batch if batch < total else 1
    c_all = torch.repeat_interleave(torch.arange(n_classes), total // n_classes).to(device)
    c_chunks = torch.chunk(c_all, n_rounds, dim=0)
    all_imgs = []
    for i in range(n_rounds):            # (the reference indexes c_chunks by range(n_rounds): torch.chunk may return fewer, and it then raises)
        c = c_chunks[i]
        x = _randn((c.size(0), config.data.channels, config.data.image_size, config.data.image_size), device, generator)
        all_imgs.append(inverse_data_transform(config, sampler.sample_image(x, c, cond_scale)))
    path = os.path.join(out_dir, f"sample-{name}.png")
    save_grid(torch.cat(all_imgs), path, nrow=total // n_classes, padding=0, normalize=True)
    return path


def load_sampling_model(states, config, weights="ema", device="cuda"):
    """A ``unet.Conditional_Model`` in eval mode from a reference-format checkpoint list ``[model, optimizer, step, ema]``
    (runners/diffusion.py:160-171; ``DDPMSFRon.checkpoint`` writes the same).  weights="ema": ``states[0]`` with the trainable parameters
    replaced by the EMA shadow ``states[-1]``, as ``EMAHelper.ema_copy`` does; weights="model": ``states[0]`` alone.

    The reference's quirk: ``Diffusion.sample()`` (:639-668) hands the EMA copy to sample_fid and sample_classes but the RAW model to
    sample_visualization -- pick ``weights`` accordingly when a run is to be compared with the reference's files."""
    from . import unet
    if weights not in ("ema", "model"):
        raise ValueError(f"weights must be 'ema' or 'model', got {weights!r}")
    if weights == "ema" and not isinstance(states[-1], dict):
        raise ValueError("weights='ema': the checkpoint has no EMA entry (its last element is not a state dict: written with model.ema off / "
                         "ema_rate=None); load it with weights='model'")
    model = unet.Conditional_Model(config, device=device)
    model.load_state_dict(states[0], strict=True)
    if weights == "ema":
        sd = model.state_dict()
        shadow = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in states[-1].items()}
        unknown = sorted(set(shadow) - set(sd))
        if unknown:
            raise KeyError(f"EMA entries the model does not have: {unknown[:4]}")
        sd.update(shadow)
        model.load_state_dict(sd, strict=True)
    model.eval()
    return model
