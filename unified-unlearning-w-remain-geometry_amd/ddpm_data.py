"""The way into the DDPM workload from a dataset (DDPM/dataset/__init__.py and the batch preamble of every loop of
DDPM/runners/diffusion.py): the whole uint8 training set lives on the GPU and a batch -- gather, flip, ToTensor, data_transform, labels,
antithetic timesteps -- is ONE launch of csrc/ddpm_data.hip (sfron_ddpm_batch_u8) behind the torch draws.

``load_cifar10`` / ``load_image_folder``   the two sources of the reference (CIFAR10, ImageFolder) as uint8 [N][3][H][W] + labels
``ResidentDataset``                        the device copy
``split_forget``                           get_forget_dataset's remain / forget split
``data_transform``                         the reference's function as torch ops (for callers who hold float tensors)
``DDPMBatchLoader`` / ``cycle``            DataLoader(shuffle=True) + the loop's preamble -> {"x0", "c", "t", "e"}

Parity unpinned (torchvision is not a dependency of this project, so these are restated from its published behaviour): the layout of
the ``cifar-10-batches-py`` pickles, ImageFolder's class order, ``Resize(int)``'s size rule (``resample.resized_size``).  What cannot be
reproduced at all: DataLoader's own shuffle (its sampler seeds a private generator from the global one) and the worker RNG behind
RandomHorizontalFlip.  The loader below draws everything from ONE generator in a documented order instead.
"""
import os
import pickle
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

CIFAR10_DIR = "cifar-10-batches-py"
CIFAR10_TRAIN = ("data_batch_1", "data_batch_2", "data_batch_3", "data_batch_4", "data_batch_5")
CIFAR10_TEST = ("test_batch",)
IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")       # torchvision IMG_EXTENSIONS


# ------------------------------------------------------------------------------------------------ sources
def load_cifar10(path, train=True):
    """torchvision.datasets.CIFAR10(path, train=train) without torchvision and without a download: reads
    ``path/cifar-10-batches-py/data_batch_1..5`` (or ``test_batch``), pickles (encoding latin1) with ``data`` uint8 [10000][3072] planar
    RGB and ``labels``.  -> (uint8 [N][3][32][32], int64 [N]) numpy arrays.  Parity unpinned (module docstring)."""
    root = os.path.join(path, CIFAR10_DIR)
    if not os.path.isdir(root):
        raise FileNotFoundError(f"no CIFAR-10 at {root}: unpack cifar-10-python.tar.gz under {path} (nothing is downloaded here)")
    data, labels = [], []
    for name in CIFAR10_TRAIN if train else CIFAR10_TEST:
        file = os.path.join(root, name)
        if not os.path.isfile(file):
            raise FileNotFoundError(f"CIFAR-10 batch file {file} is missing")
        with open(file, "rb") as f:
            entry = pickle.load(f, encoding="latin1")
        data.append(np.asarray(entry["data"], dtype=np.uint8))
        labels.extend(entry["labels"] if "labels" in entry else entry["fine_labels"])
    images = np.ascontiguousarray(np.vstack(data).reshape(-1, 3, 32, 32))
    return images, np.asarray(labels, dtype=np.int64)


def load_image_folder(path, image_size, device=None):
    """ImageFolder(path, Compose([Resize(image_size), ToTensor()])) up to the bytes: class sub-folders in sorted order are labels
    0, 1, ..; inside a class the files of every sub-directory in sorted walk order; ``.convert("RGB")``; Resize(image_size) -- the short
    side becomes image_size, bilinear, Pillow's bytes; an image whose short side already matches is untouched -- once, here, because it
    is deterministic.  The resize runs on ``device`` through ``classify.load_images_u8`` when that is a GPU, else with Pillow itself (the
    same bytes).  Every image must come out at one size.  -> (uint8 [N][3][H][W], int64 [N]) numpy arrays.  Parity unpinned."""
    from PIL import Image

    from . import classify, resample
    if not os.path.isdir(path):
        raise FileNotFoundError(f"no image folder at {path}")
    classes = sorted(e.name for e in os.scandir(path) if e.is_dir())
    if not classes:
        raise FileNotFoundError(f"{path} has no class sub-folders")
    images, labels = [], []
    on_gpu = device is not None and torch.device(device).type == "cuda"
    for label, cls in enumerate(classes):
        for root, _, files in sorted(os.walk(os.path.join(path, cls), followlinks=True)):
            for name in sorted(files):
                if not name.lower().endswith(IMAGE_EXTENSIONS):
                    continue
                file = os.path.join(root, name)
                with Image.open(file) as im:
                    w, h = im.size
                    nw, nh = resample.resized_size(w, h, int(image_size))
                    if (nw, nh) == (w, h):
                        a = np.array(im.convert("RGB"), dtype=np.uint8)
                    elif on_gpu:
                        a = classify.load_images_u8([file], (nh, nw), device=device)[0].cpu().numpy()
                    else:
                        a = classify.transform_host(im, (nh, nw))
                if images and a.shape != images[0].shape:
                    raise ValueError(f"{file} is {a.shape[1]} x {a.shape[0]} after Resize({image_size}), the first image "
                                     f"{images[0].shape[1]} x {images[0].shape[0]}: a resident dataset holds one size")
                images.append(a)
                labels.append(label)
    if not images:
        raise FileNotFoundError(f"{path} holds no image files")
    return np.ascontiguousarray(np.stack(images).transpose(0, 3, 1, 2)), np.asarray(labels, dtype=np.int64)


def load_dataset(config, device=None, train=True):
    """config.data.dataset -> (images, labels): CIFAR10 from config.data.path.  STL10 is not built."""
    name = getattr(config.data, "dataset", "CIFAR10")
    if name == "CIFAR10":
        return load_cifar10(config.data.path, train=train)
    if name == "STL10":
        raise NotImplementedError("STL10 is not built: the loader reads CIFAR10 (load_cifar10) and image folders (load_image_folder)")
    raise NotImplementedError(f"unknown dataset {name!r}")


class ResidentDataset:
    """The dataset on the device: ``images`` uint8 [N][C][H][W], ``labels`` int64 [N].  CIFAR-10's training set is 150 MB."""

    def __init__(self, images_u8, labels, device="cuda"):
        images = torch.as_tensor(images_u8)
        labels = torch.as_tensor(labels)
        if images.dtype != torch.uint8 or images.dim() != 4:
            raise ValueError(f"images must be uint8 [N][C][H][W], got {images.dtype} {tuple(images.shape)}")
        if labels.dim() != 1 or labels.shape[0] != images.shape[0]:
            raise ValueError(f"{images.shape[0]} images but labels of shape {tuple(labels.shape)}")
        self.labels_host = labels.to(torch.int64).cpu()
        self.device = torch.device(device)
        self.images = images.to(self.device).contiguous()
        self.labels = self.labels_host.to(self.device)

    def __len__(self):
        return self.images.shape[0]

    @property
    def shape(self):
        return tuple(self.images.shape[1:])


def split_forget(labels, label_to_drop):
    """(remain, forget) int64 index vectors in dataset order: get_forget_dataset's ``[data for data in dataset if data[1] != label]``
    and ``== label`` (DDPM/dataset/__init__.py:161-162)."""
    labels = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels).cpu()
    keep = labels != label_to_drop
    return torch.nonzero(keep).flatten(), torch.nonzero(~keep).flatten()


# ------------------------------------------------------------------------------------------------ data_transform
LOGIT_LAM = 1e-6


def logit_transform(image, lam=LOGIT_LAM):
    image = lam + (1 - 2 * lam) * image
    return torch.log(image) - torch.log1p(-image)


def data_transform(config, X, u=None, n=None, generator=None):
    """DDPM/dataset/__init__.py:241-255 op by op on X's device.  ``u`` / ``n``: the rand_like / randn_like draws when the caller holds
    them (the kernel's inputs); otherwise they are drawn here, from ``generator`` if given."""
    if getattr(config.data, "uniform_dequantization", False):
        if u is None:
            u = torch.rand(X.shape, dtype=X.dtype, device=X.device, generator=generator)
        X = X / 256.0 * 255.0 + u / 256.0
    if getattr(config.data, "gaussian_dequantization", False):
        if n is None:
            n = torch.randn(X.shape, dtype=X.dtype, device=X.device, generator=generator)
        X = X + n * 0.01
    if getattr(config.data, "rescaled", False):
        X = 2 * X - 1.0
    elif getattr(config.data, "logit_transform", False):
        X = logit_transform(X)
    if hasattr(config, "image_mean"):
        return X - config.image_mean.to(X.device)[None, ...]
    return X


def transform_mode(config):
    if getattr(config.data, "rescaled", False):
        return _lib.DDPM_DATA_RESCALED
    return _lib.DDPM_DATA_LOGIT if getattr(config.data, "logit_transform", False) else _lib.DDPM_DATA_PLAIN


def antithetic_t(t_half, num_timesteps, n):
    """``torch.cat([t, T - t - 1], dim=0)[:n]`` of the runner's loops; t_half holds n // 2 + 1 draws."""
    return torch.cat([t_half, num_timesteps - t_half - 1], dim=0)[:n]


def batch_torch(dataset, idx, flip, config, num_timesteps, u=None, n=None, t_half=None):
    """What ``ddpm_batch_u8`` computes, as torch ops on the dataset's device: the yardstick of the kernel and the middle route of
    tools/bench_ddpm_data.py.  -> (x0, c, t or None)"""
    x = dataset.images[idx]
    if flip is not None:
        x = torch.where(flip.bool()[:, None, None, None], x.flip(3), x)
    # ToTensor: byte / 255 as a TRUE division.  On the device torch turns a division by a Python number into a multiplication by its
    # reciprocal (126 of the 256 byte values then differ); a 0-dim device tensor keeps the division.
    x0 = data_transform(config, x.float() / torch.full((), 255.0, device=x.device), u=u, n=n)
    t = antithetic_t(t_half, num_timesteps, idx.shape[0]) if t_half is not None else None
    return x0, dataset.labels[idx], t


def ddpm_batch_u8(dataset, idx, flip, config, num_timesteps, u=None, n=None, t_half=None, image_mean=None, out=None):
    """One launch of sfron_ddpm_batch_u8 (include/sfron.h) on the current stream -> (x0 fp32 [B][C][H][W], c int64 [B], t int64 [B] or
    None).  ``idx`` int64 [B] and ``flip`` uint8 [B] (or None) are device tensors; ``u`` / ``n`` the dequantization draws the config asks
    for; ``image_mean`` defaults to ``config.image_mean``.  ``out``: (x0, c, t) to write into."""
    C, H, W = dataset.shape
    B = idx.shape[0]
    dev = dataset.device
    if image_mean is None and hasattr(config, "image_mean"):
        image_mean = config.image_mean.to(device=dev, dtype=torch.float32).contiguous()
    uni, gau = bool(getattr(config.data, "uniform_dequantization", False)), bool(getattr(config.data, "gaussian_dequantization", False))
    if out is None:
        out = (torch.empty(B, C, H, W, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int64, device=dev),
               torch.empty(B, dtype=torch.int64, device=dev) if t_half is not None else None)
    x0, c, t = out
    for name, v, shape, dtype in (("idx", idx, (B,), torch.int64), ("flip", flip, (B,), torch.uint8), ("u", u if uni else None, x0.shape, torch.float32),
                                  ("n", n if gau else None, x0.shape, torch.float32), ("image_mean", image_mean, (C, H, W), torch.float32),
                                  ("t_half", t_half, (B // 2 + 1,), torch.int64)):
        if v is not None and (tuple(v.shape) != tuple(shape) or v.dtype != dtype):
            raise ValueError(f"{name} must be {dtype} {tuple(shape)}, got {v.dtype} {tuple(v.shape)}")
    check(_lib.lib().sfron_ddpm_batch_u8(ptr(dataset.images), ptr(dataset.labels), len(dataset), C, H, W, ptr(idx), ptr(flip), B, int(uni),
                                         ptr(u) if uni else None, int(gau), ptr(n) if gau else None, transform_mode(config), ptr(image_mean),
                                         ptr(t_half), int(num_timesteps), ptr(x0), ptr(c), ptr(t), stream_ptr()), "sfron_ddpm_batch_u8")
    return x0, c, t


# ------------------------------------------------------------------------------------------------ the loader
def cycle(dl):
    """functions.cycle of the reference: epochs without end."""
    while True:
        for data in dl:
            yield data


class DDPMBatchLoader:
    """DataLoader(subset, batch_size, shuffle=True, drop_last=False) over ``indices`` of a ResidentDataset, fused with the preamble of
    the runner's loops: every item is ``{"x0", "c", "t", "e"}``, ready for ``DDPMSFRon.step`` / ``train_step`` and
    ``DDPMFisherAccumulator.accumulate``.  ``len()`` is ceil(n / batch_size); iterating is one epoch and the short last batch is kept.

    Every random number comes from ``generator`` (a generator on the dataset's device), in this order:

    * at construction, ``flip="frozen"`` only: ``torch.rand(n, generator) < 0.5``, flag j for ``indices[j]``;
    * at the start of every epoch: ``perm = torch.randperm(n, generator)``; batch i holds ``indices[perm[i * bs:(i + 1) * bs]]``;
    * per batch of B images, in this order: ``flip="per_access"`` only ``torch.rand(B) < 0.5``; ``u = torch.rand(B, C, H, W)`` if
      config.data.uniform_dequantization; ``n = torch.randn(B, C, H, W)`` if gaussian_dequantization; ``e = torch.randn(B, C, H, W)``;
      ``t_half = torch.randint(0, num_timesteps, (B // 2 + 1,))`` (all fp32 / int64 on the device) -- the order of
      data_transform, ``e = torch.randn_like(x)`` and the antithetic draw in the reference's loops.

    Flip modes -- a quirk of the reference worth knowing.  get_forget_dataset materialises ``[data for data in dataset ...]``: the
    RandomHorizontalFlip of its transform runs ONCE per image when the split is built and is frozen for the whole run, so sfron_forget,
    retrain and generate_fisher see every image in one orientation only (``flip="frozen"``).  get_dataset (mode train) hands the
    Dataset to the DataLoader and redraws the flip on every access (``flip="per_access"``).  ``flip=None`` is config.data.random_flip
    false.  The default follows config.data.random_flip with "frozen".

    ``rank`` / ``world``: every rank draws the GLOBAL batch from an identically seeded generator and yields its rows ``[rank::world]``;
    the antithetic t is formed on the global batch and then sliced, so the union over the ranks is the world = 1 batch.

    Unpinned: DataLoader's own shuffle and the worker RNG behind the flips cannot be reproduced (module docstring)."""

    def __init__(self, dataset, indices, batch_size, config, num_timesteps, generator, flip="default", rank=0, world=1):
        if flip == "default":
            flip = "frozen" if getattr(config.data, "random_flip", False) else None
        if flip not in (None, "frozen", "per_access"):
            raise ValueError(f"flip must be None, 'frozen' or 'per_access', got {flip!r}")
        if batch_size < 1 or not 0 <= rank < world:
            raise ValueError(f"bad batch_size {batch_size} or rank {rank} of {world}")
        self.dataset, self.config, self.batch_size, self.T = dataset, config, int(batch_size), int(num_timesteps)
        self.gen, self.flip, self.rank, self.world = generator, flip, rank, world
        self.dev = dataset.device
        if generator.device.type != self.dev.type:
            raise ValueError(f"the generator lives on {generator.device}, the dataset on {self.dev}")
        self.indices = torch.as_tensor(indices, dtype=torch.int64).to(self.dev)
        self.n = self.indices.shape[0]
        if self.n < 1:
            raise ValueError("an empty index set")
        self.frozen = (torch.rand(self.n, generator=generator, device=self.dev) < 0.5).to(torch.uint8) if flip == "frozen" else None
        self.uni = bool(getattr(config.data, "uniform_dequantization", False))
        self.gau = bool(getattr(config.data, "gaussian_dequantization", False))
        self.image_mean = (config.image_mean.to(device=self.dev, dtype=torch.float32).contiguous() if hasattr(config, "image_mean") else None)

    def __len__(self):
        return (self.n + self.batch_size - 1) // self.batch_size

    def index_batches(self):
        """One epoch of GLOBAL batches as (idx int64 [B], flip uint8 [B] or None): the part of an epoch that needs no kernel."""
        perm = torch.randperm(self.n, generator=self.gen, device=self.dev)
        for i in range(len(self)):
            pos = perm[i * self.batch_size:(i + 1) * self.batch_size]
            flip = None
            if self.flip == "frozen":
                flip = self.frozen[pos]
            elif self.flip == "per_access":
                flip = (torch.rand(pos.shape[0], generator=self.gen, device=self.dev) < 0.5).to(torch.uint8)
            yield self.indices[pos], flip

    def draws(self, B):
        """(u, n, e, t_half) of one global batch, in the documented order."""
        shape = (B,) + self.dataset.shape
        u = torch.rand(shape, generator=self.gen, device=self.dev) if self.uni else None
        n = torch.randn(shape, generator=self.gen, device=self.dev) if self.gau else None
        e = torch.randn(shape, generator=self.gen, device=self.dev)
        t_half = torch.randint(0, self.T, (B // 2 + 1,), generator=self.gen, device=self.dev)
        return u, n, e, t_half

    def rank_rows(self, v):
        """this rank's rows of a global batch"""
        return v[self.rank::self.world].contiguous()

    def __iter__(self):
        for idx, flip in self.index_batches():
            u, n, e, t_half = self.draws(idx.shape[0])
            x0, c, t = ddpm_batch_u8(self.dataset, idx, flip, self.config, self.T, u=u, n=n, t_half=t_half, image_mean=self.image_mean)
            if self.world > 1:
                x0, c, t, e = (self.rank_rows(v) for v in (x0, c, t, e))
            yield {"x0": x0, "c": c, "t": t, "e": e}


def config_with_data(config, **data):
    """A copy of a config namespace whose ``data`` section carries the given fields beside its own (dataset, path, random_flip,
    uniform_dequantization, gaussian_dequantization, rescaled, logit_transform ...): ``unet.config_namespace`` knows the model's."""
    merged = dict(vars(config.data))
    merged.update(data)
    out = SimpleNamespace(**vars(config))
    out.data = SimpleNamespace(**merged)
    return out
