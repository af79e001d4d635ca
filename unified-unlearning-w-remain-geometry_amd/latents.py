"""Latent front-end of the DiT class-forgetting loop.

The reference feeds the step from an ImageFolder split by class (DiT/unlearn_dataset.py:277-292 ``get_unlearn_dataset``: the
forget set is the class whose index -- position in the alphabetically sorted class-directory list -- equals ``forget_class``,
the remain set is every other class) and encodes each image batch with the frozen VAE inside the loop
(DiT/forget.py:265-267,305-307: ``vae.encode(x).latent_dist.sample().mul_(0.18215)``).  The encoder never changes, so here
its OUTPUT is cached once, offline, as the posterior moments (mean || logvar, [8, 32, 32] fp16/fp32 per image) in per-class
shards, and the step's inputs come from that cache: the class split is the reference's, the posterior sample + 0.18215
scaling is sfron_latent_sample on the device, and batches reach the GPU through pinned buffers on a copy stream one batch
ahead of the step (data-parallel ranks take strided shares of each global batch).  ``write_shard`` takes whatever moments the
caller's encoder produced; ``encode_image_folder`` fills the cache from an ImageFolder with the native encoder (sfron.vae).

The online route, ``UnlearnImageLoader``, is the reference's loop with the encode included: decode + centre crop on host threads,
RandomHorizontalFlip drawn per sample, and the KL-f8 encoder + posterior sample on the device in each ``next()``.  It enumerates and
draws like the cache route, so one seed gives both routes the same batches (flips aside).
"""
from concurrent.futures import ThreadPoolExecutor
import json
import os

import numpy as np
import torch
from PIL import Image

from . import _lib
from ._lib import check, ptr, stream_ptr

IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")


def find_classes(directory):
    """torchvision.datasets.folder.find_classes as the reference uses it: sorted sub-directory names -> index."""
    classes = sorted(e.name for e in os.scandir(directory) if e.is_dir())
    if not classes:
        raise FileNotFoundError(f"Couldn't find any class folder in {directory}.")
    return classes, {c: i for i, c in enumerate(classes)}


def class_split(data_path, forget_class):
    """DiT/unlearn_dataset.py:277-292: (forget class names, remain class names, class_to_idx) of ``data_path/train``."""
    classes, class_to_idx = find_classes(os.path.join(data_path, "train"))
    forget = [c for c in classes if class_to_idx[c] == forget_class]
    remain = [c for c in classes if class_to_idx[c] != forget_class]
    return forget, remain, class_to_idx


def write_shard(cache_dir, class_name, class_index, moments):
    """One class's cached VAE posterior moments [N, 2C, H, W] (mean || logvar) -> <cache_dir>/<class_name>.npy + index entry."""
    os.makedirs(cache_dir, exist_ok=True)
    m = np.asarray(moments)
    assert m.ndim == 4 and m.shape[1] % 2 == 0
    np.save(os.path.join(cache_dir, class_name + ".npy"), m)
    idx_path = os.path.join(cache_dir, "index.json")
    idx = json.load(open(idx_path)) if os.path.isfile(idx_path) else {}
    idx[class_name] = {"index": int(class_index), "count": int(m.shape[0]), "shape": list(m.shape[1:]), "dtype": str(m.dtype)}
    json.dump(idx, open(idx_path, "w"), indent=1, sort_keys=True)


class LatentCache:
    """Memory-mapped per-class shards written by write_shard; ``split(forget_class)`` gives the reference's two datasets."""

    def __init__(self, cache_dir):
        self.dir = cache_dir
        self.index = json.load(open(os.path.join(cache_dir, "index.json")))
        self.classes = sorted(self.index)                                  # alphabetical, as find_classes
        for i, c in enumerate(self.classes):
            if self.index[c]["index"] != i:
                raise ValueError(f"class {c!r} was cached with index {self.index[c]['index']}, the sorted position is {i}")
        self._maps = {}

    def shard(self, name):
        if name not in self._maps:
            self._maps[name] = np.load(os.path.join(self.dir, name + ".npy"), mmap_mode="r")
        return self._maps[name]

    def split(self, forget_class):
        forget = [c for c in self.classes if self.index[c]["index"] == forget_class]
        remain = [c for c in self.classes if self.index[c]["index"] != forget_class]
        return forget, remain

    def samples(self, names):
        """[(class name, class index, position in shard)] in ImageFolder order (classes sorted, files in shard order)."""
        return [(c, self.index[c]["index"], i) for c in names for i in range(self.index[c]["count"])]


def _batch_draws(seed, stream, step, n_samples, gb, num_timesteps, drop_prob, C, h, w):
    """The host draws of one global batch: (sample ids, t, noise, eps, drop, g2), keyed by (seed, epoch / step, stream).  Shuffling is
    per epoch (drop_last), the per-step generator g2 draws t, noise, posterior eps and the label-dropout mask in that order; a caller
    that needs more draws (the image loader's flips) takes them from g2 after these."""
    per_epoch = max(1, n_samples // gb)                                          # drop_last, as the reference's loaders
    epoch, pos = divmod(step, per_epoch)
    g = torch.Generator().manual_seed(((seed * 1_000_003 + epoch) * 2 + (stream == "remain")) & 0x7FFFFFFF)
    perm = torch.randperm(n_samples, generator=g)
    ids = perm[pos * gb:(pos + 1) * gb] if n_samples >= gb else perm[torch.arange(gb) % n_samples]
    g2 = torch.Generator().manual_seed(((seed * 7_000_003 + step) * 2 + (stream == "remain")) & 0x7FFFFFFF)
    t = torch.randint(0, num_timesteps, (gb,), generator=g2)
    noise = torch.randn(gb, C, h, w, generator=g2)
    eps = torch.randn(gb, C, h, w, generator=g2)
    drop = (torch.rand(gb, generator=g2) < drop_prob).to(torch.uint8)
    return ids, t, noise, eps, drop, g2


class UnlearnLatentLoader:
    """Infinite forget / remain batch streams for DiTSFRon.step (the reference cycles two shuffled DataLoaders,
    DiT/forget.py:219-228,241-246): each ``next()`` returns ``dict(x0, y, t, noise, drop)`` on the device for this rank's share
    of a global batch.  Shuffling, timesteps, noise, posterior noise and label-dropout draws are keyed by (seed, epoch / step,
    stream) on the host generator, so every world size sees the same global batch."""

    def __init__(self, cache, forget_class, global_batch, rank=0, world=1, seed=0, num_timesteps=1000, drop_prob=0.1, scale=0.18215,
                 device="cuda"):
        assert global_batch % world == 0
        self.cache, self.gb, self.rank, self.world, self.seed = cache, global_batch, rank, world, seed
        self.T, self.p, self.scale, self.dev = num_timesteps, drop_prob, scale, torch.device(device)
        f, r = cache.split(forget_class)
        self.sets = {"forget": cache.samples(f), "remain": cache.samples(r)}
        if not self.sets["forget"] or not self.sets["remain"]:
            raise ValueError("empty forget or remain set")
        self.step = {"forget": 0, "remain": 0}
        self._copy = torch.cuda.Stream(device=self.dev) if self.dev.type == "cuda" else None
        self._ahead = {}

    def _host_batch(self, stream, step):
        s = self.sets[stream]
        shp = self.cache.index[s[0][0]]["shape"]
        ids, t, noise, eps, drop, _ = _batch_draws(self.seed, stream, step, len(s), self.gb, self.T, self.p, shp[0] // 2, shp[1], shp[2])
        mine = list(range(self.rank, self.gb, self.world))                     # strided share of the global batch
        mom = np.stack([np.asarray(self.cache.shard(s[int(ids[j])][0])[s[int(ids[j])][2]], dtype=np.float32) for j in mine])
        y = torch.tensor([s[int(ids[j])][1] for j in mine], dtype=torch.int64)
        return dict(moments=torch.from_numpy(mom), eps=eps[mine].contiguous(), y=y, t=t[mine].contiguous(), noise=noise[mine].contiguous(),
                    drop=drop[mine].contiguous())

    def _stage(self, stream, step):
        hb = self._host_batch(stream, step)
        if self._copy is None:
            return hb, None
        pinned = {k: v.pin_memory() for k, v in hb.items()}
        with torch.cuda.stream(self._copy):
            dv = {k: v.to(self.dev, non_blocking=True) for k, v in pinned.items()}
            ev = torch.cuda.Event()
            ev.record(self._copy)
        return dv, (ev, pinned)

    def next(self, stream):
        step = self.step[stream]
        staged = self._ahead.pop((stream, step), None) or self._stage(stream, step)
        self._ahead[(stream, step + 1)] = self._stage(stream, step + 1)        # one batch ahead, on the copy stream
        self.step[stream] = step + 1
        dv, sync = staged
        if sync is not None:
            cur = torch.cuda.current_stream()
            cur.wait_event(sync[0])
            # the staged tensors were allocated on the copy stream: tell the caching allocator that the consumer stream
            # reads them, so a dropped batch is not handed to a later staging copy while queued step kernels still use it
            # (the fast path never syncs the host and may run several steps ahead of the GPU)
            for v in dv.values():
                v.record_stream(cur)
        mom = dv["moments"].contiguous()
        n, c2, h, w = mom.shape
        x0 = torch.empty(n, c2 // 2, h, w, dtype=torch.float32, device=mom.device)
        check(_lib.lib().sfron_latent_sample(ptr(mom), ptr(dv["eps"]), n, c2 // 2, h * w, float(self.scale), ptr(x0), stream_ptr()),
              "latent_sample")
        return dict(x0=x0, y=dv["y"], t=dv["t"], noise=dv["noise"], drop=dv["drop"])


# ------------------------------------------------------------------------------------------------ image front-end
MAX_HOST_THREADS = 16      # a GPU host gives one command 16 CPUs


def center_crop_arr(pil_image, image_size):
    """ADM's centre crop as DiT/forget.py:89-107 uses it: halve with a BOX filter while the short side is >= 2 x image_size, resize
    with BICUBIC so the short side is image_size (sizes rounded), then crop the centre image_size x image_size."""
    img = pil_image
    while min(img.size) >= 2 * image_size:
        img = img.resize(tuple(d // 2 for d in img.size), resample=Image.BOX)
    s = image_size / min(img.size)
    img = img.resize(tuple(round(d * s) for d in img.size), resample=Image.BICUBIC)
    a = np.array(img)
    top, left = (a.shape[0] - image_size) // 2, (a.shape[1] - image_size) // 2
    return Image.fromarray(a[top:top + image_size, left:left + image_size])


def class_files(directory):
    """torchvision's make_dataset order for one class directory: os.walk (followlinks) in sorted order, file names sorted, image extensions."""
    out = []
    for root, _, fnames in sorted(os.walk(directory, followlinks=True)):
        for f in sorted(fnames):
            if f.lower().endswith(IMG_EXTENSIONS):
                out.append(os.path.join(root, f))
    return out


def load_image(path, image_size):
    """pil_loader (RGB) + center_crop_arr -> uint8 [image_size, image_size, 3]."""
    with open(path, "rb") as fh:
        img = Image.open(fh).convert("RGB")
    return np.asarray(center_crop_arr(img, image_size), dtype=np.uint8)


def decode_image(path):
    """pil_loader alone: the decoded RGB pixels, uint8 [H, W, 3] (every mode arrives as RGB), for the device crop (resample.center_crop_gpu)."""
    with open(path, "rb") as fh:
        return np.asarray(Image.open(fh).convert("RGB"), dtype=np.uint8)


def _pool(workers):
    return ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_HOST_THREADS)))


def encode_image_folder(data_path, encoder, cache_dir, image_size=256, batch=32, dtype=np.float32, workers=8, gpu_resize=False):
    """``data_path/train/<class>/*`` -> one write_shard per class of the encoder's posterior moments (what LatentCache and
    UnlearnLatentLoader read), files in ImageFolder order.  Images are decoded and cropped on a host thread pool while the
    previous batch encodes on the device; with ``gpu_resize`` the pool only decodes and the centre crop runs on the device
    (resample.center_crop_gpu: the same bytes, so the same shards).  Returns {class name: image count}."""
    if gpu_resize:
        from . import resample
        load = decode_image
        crop = lambda imgs: resample.center_crop_gpu(imgs, image_size, device=encoder.dev)
    else:
        load = lambda f: load_image(f, image_size)
        crop = lambda imgs: torch.from_numpy(np.stack(imgs))
    classes, class_to_idx = find_classes(os.path.join(data_path, "train"))
    mdt = {np.dtype(np.float32): torch.float32, np.dtype(np.float16): torch.float16}[np.dtype(dtype)]
    counts = {}
    with _pool(workers) as pool:
        for c in classes:
            files = class_files(os.path.join(data_path, "train", c))
            parts = []
            nxt = pool.map(load, files[:batch]) if files else None
            for lo in range(0, len(files), batch):
                imgs = list(nxt)
                nxt = pool.map(load, files[lo + batch:lo + 2 * batch]) if lo + batch < len(files) else None
                parts.append(encoder.moments(crop(imgs), dtype=mdt).cpu().numpy())
            if not parts:
                raise FileNotFoundError(f"class {c!r} has no image files")
            write_shard(cache_dir, c, class_to_idx[c], np.concatenate(parts))
            counts[c] = len(files)
    return counts


class UnlearnImageLoader:
    """UnlearnLatentLoader's contract -- ``next(stream)`` gives ``dict(x0, y, t, noise, drop)`` on the device for this rank's strided share
    of a global batch -- with the images read from ``data_path/train`` and encoded on the GPU in the call (DiT/forget.py:200-246,
    265-267,305-307: centre crop, RandomHorizontalFlip, ToTensor + Normalize, vae.encode(x).latent_dist.sample().mul_(0.18215)).
    Sample ids, shuffling and the t / noise / eps / drop draws equal the cache route's; the flips are drawn after them, so with
    ``flip_prob=0`` every field but x0 equals UnlearnLatentLoader's bit for bit.  The next batch is decoded on host threads and copied
    on a side stream while the current one is consumed.

    ``gpu_resize=True`` moves the centre crop to the device, with the same bytes (resample.center_crop_gpu's parts): the pool threads
    only decode, the batch-ahead thread plans the batch and gathers its pixels, tables and pass records into a pinned buffer
    (resample.CropStaging: a batch being assembled never waits for the one being consumed), ``next`` uploads it on the copy stream and
    runs the level launches, then the encoder, on the caller's stream."""

    def __init__(self, data_path, forget_class, encoder, global_batch, rank=0, world=1, seed=0, image_size=256, flip_prob=0.5,
                 num_timesteps=1000, drop_prob=0.1, scale=0.18215, device="cuda", workers=8, gpu_resize=False):
        assert global_batch % world == 0
        self.enc, self.gb, self.rank, self.world, self.seed = encoder, global_batch, rank, world, seed
        self.size, self.flip_prob, self.T, self.p, self.scale = image_size, float(flip_prob), num_timesteps, drop_prob, scale
        self.dev = torch.device(device)
        f = 1 << (len(encoder.ch_mult) - 1)
        self.lat_shape = (encoder.z, image_size // f, image_size // f)
        forget, remain, class_to_idx = class_split(data_path, forget_class)
        root = os.path.join(data_path, "train")
        samples = lambda names: [(p, class_to_idx[c]) for c in names for p in class_files(os.path.join(root, c))]
        self.sets = {"forget": samples(forget), "remain": samples(remain)}
        if not self.sets["forget"] or not self.sets["remain"]:
            raise ValueError("empty forget or remain set")
        self.step = {"forget": 0, "remain": 0}
        self._copy = torch.cuda.Stream(device=self.dev)
        self._pool = _pool(workers)                # decodes the images of a batch
        self._bg = ThreadPoolExecutor(max_workers=1)   # assembles the next batch (its own thread: it waits on _pool's tasks)
        self._ahead, self._pinned = {}, None
        self.gpu_resize = bool(gpu_resize)
        if self.gpu_resize:
            from . import resample
            self._crop = resample.crop_staging(self.dev)

    def _host_batch(self, stream, step, gather=False):
        s = self.sets[stream]
        C, h, w = self.lat_shape
        ids, t, noise, eps, drop, g2 = _batch_draws(self.seed, stream, step, len(s), self.gb, self.T, self.p, C, h, w)
        flip = (torch.rand(self.gb, generator=g2) < self.flip_prob).to(torch.uint8)
        mine = list(range(self.rank, self.gb, self.world))
        y = torch.tensor([s[int(ids[j])][1] for j in mine], dtype=torch.int64)
        hb = dict(flip=flip[mine].contiguous(), eps=eps[mine].contiguous(), y=y, t=t[mine].contiguous(), noise=noise[mine].contiguous(),
                  drop=drop[mine].contiguous())
        if self.gpu_resize:
            hb["sources"] = list(self._pool.map(lambda j: decode_image(s[int(ids[j])][0]), mine))
            if gather:                              # (the batch-ahead thread: plan and fill the pinned buffer)
                hb["gathered"] = self._crop.gather(hb.pop("sources"), self.size)
        else:
            imgs = np.stack(list(self._pool.map(lambda j: load_image(s[int(ids[j])][0], self.size), mine)))
            hb = dict(images=torch.from_numpy(imgs), **hb)
        return hb

    def _stage(self, hb):
        gathered = hb.pop("gathered", None)
        pinned = {k: v.pin_memory() for k, v in hb.items()}
        with torch.cuda.stream(self._copy):
            dv = {k: v.to(self.dev, non_blocking=True) for k, v in pinned.items()}
            if gathered is not None:
                dv["crop_bytes"] = gathered.upload()
            ev = torch.cuda.Event()
            ev.record(self._copy)
        return dv, (ev, pinned), gathered

    def host_batch(self, stream, step):
        """The host side of batch `step` of `stream` (uint8 images [n, S, S, 3], flips and the draws), for tests and tools; with
        ``gpu_resize`` the decoded sources (a list of uint8 [H, W, 3]) stand in place of ``images``."""
        return self._host_batch(stream, step)

    def next(self, stream):
        step = self.step[stream]
        fut = self._ahead.pop((stream, step), None)
        hb = fut.result() if fut is not None else self._host_batch(stream, step, True)
        self._ahead[(stream, step + 1)] = self._bg.submit(self._host_batch, stream, step + 1, True)     # decode one batch ahead
        self.step[stream] = step + 1
        dv, (ev, self._pinned), gathered = self._stage(hb)     # (the pinned batch lives until the next call)
        cur = torch.cuda.current_stream()
        cur.wait_event(ev)
        for v in dv.values():
            v.record_stream(cur)
        images = dv["images"] if gathered is None else gathered.run(dv["crop_bytes"])      # (the level launches, on the caller's stream)
        x0 = self.enc.encode(images, eps=dv["eps"], flip=dv["flip"], scale=self.scale)
        return dict(x0=x0, y=dv["y"], t=dv["t"], noise=dv["noise"], drop=dv["drop"])
