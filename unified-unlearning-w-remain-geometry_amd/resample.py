"""The image transform of the SD scripts (SD/train-scripts/dataset.py:23-33: Resize(size, bicubic) -> CenterCrop(size) -> RGB; ToTensor and
Normalize(0.5, 0.5) are the encoder's uint8 input kernel) on the host with Pillow and on the GPU with csrc/resample.hip.

``torchvision.transforms.Resize`` on a PIL image is ``Image.resize``: Pillow's separable fixed-point convolution (src/libImaging/Resample.c,
8-bit path, PRECISION_BITS = 22).  It is integer arithmetic over coefficients that are made once per axis in float64, so the GPU version is
specified bit for bit: ``resample_tables`` restates the coefficient computation on the host, sfron_image_resample_u8 does the two integer
passes.  The centre crop is folded in: the tables are sliced to the crop window, so only the window is computed.

torchvision is not part of this project's environment: ``resized_size`` and ``center_crop_offsets`` restate its published rules and are not
pinned by a fixture.
"""
import functools
import math

import numpy as np
import torch
from PIL import Image

from . import _lib
from ._lib import stream_ptr

PRECISION_BITS = 22
FILTERS = {"box": 0.5, "bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}          # name -> support
_PIL_FILTER = {"box": Image.BOX, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _filter_values(name, x):
    """Pillow's filter functions over a float64 array (elementwise; + - * only, so numpy gives the C doubles; lanczos through math.sin)."""
    if name == "box":
        return np.where((x > -0.5) & (x <= 0.5), 1.0, 0.0)
    if name == "bilinear":
        a = np.abs(x)
        return np.where(a < 1.0, 1.0 - a, 0.0)
    if name == "bicubic":
        a, x = -0.5, np.abs(x)
        return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))
    if name == "lanczos":
        flat = [(_sinc(v) * _sinc(v / 3) if -3.0 <= v < 3.0 else 0.0) for v in x.ravel().tolist()]
        return np.asarray(flat, dtype=np.float64).reshape(x.shape)
    raise ValueError(f"filter must be one of {sorted(FILTERS)}, got {name!r}")


class Tables:
    """One axis of a resize: ``coeffs`` int32 [n][ksize], ``bounds`` int32 [n][2] = (first source index, tap count), ``ksize``; for the
    ``n`` outputs first .. first + n - 1 of the n_out the axis has.  ``device(dev)`` gives (and keeps) the copies the kernel reads."""

    def __init__(self, coeffs, bounds, ksize):
        self.coeffs, self.bounds, self.ksize = coeffs, bounds, int(ksize)
        self._dev = {}

    def __iter__(self):                                    # (coeffs, bounds, ksize) = resample_tables(...)
        return iter((self.coeffs, self.bounds, self.ksize))

    def device(self, dev):
        dev = torch.device(dev)
        if dev not in self._dev:
            self._dev[dev] = (torch.from_numpy(self.coeffs.copy()).to(dev).contiguous(), torch.from_numpy(self.bounds.copy()).to(dev).contiguous())
        return self._dev[dev]

    def rows(self):
        """[lo, hi): the union of the source indices the outputs read (bounds ascend)."""
        return int(self.bounds[0, 0]), int(self.bounds[-1, 0] + self.bounds[-1, 1])


@functools.lru_cache(maxsize=512)
def resample_tables(n_in, n_out, filter="bicubic", first=0, count=None):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for one axis (Resample.c), in float64 on the host:
        scale = n_in / n_out, fs = max(scale, 1), sup = support * fs, ksize = ceil(sup) * 2 + 1
        per output xx: center = (xx + 0.5) * scale, xmin = max(int(center - sup + 0.5), 0), xmax = min(int(center + sup + 0.5), n_in) - xmin,
        w[x] = f((x + xmin - center + 0.5) * (1 / fs)) for x < xmax, summed in ascending order and divided by the sum when it is not zero,
        coefficient = int(0.5 + w * 2^22) for w >= 0, int(-0.5 + w * 2^22) for w < 0 (truncation toward zero).
    Returns the Tables of outputs first .. first + count - 1 (all of them by default); cached with their device copies."""
    n_in, n_out, first = int(n_in), int(n_out), int(first)
    count = n_out - first if count is None else int(count)
    if n_in < 1 or n_out < 1 or first < 0 or count < 1 or first + count > n_out:
        raise ValueError(f"resample_tables: n_in {n_in}, n_out {n_out}, first {first}, count {count}")
    support = FILTERS.get(filter)
    if support is None:
        raise ValueError(f"filter must be one of {sorted(FILTERS)}, got {filter!r}")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    sup = support * fs
    ksize = int(math.ceil(sup)) * 2 + 1
    ss = 1.0 / fs
    xx = np.arange(first, first + count, dtype=np.float64)
    center = (xx + 0.5) * scale
    xmin = np.maximum(np.trunc(center - sup + 0.5), 0).astype(np.int64)
    xmax = np.minimum(np.trunc(center + sup + 0.5), n_in).astype(np.int64) - xmin
    x = np.arange(ksize, dtype=np.int64)
    live = x[None, :] < xmax[:, None]
    w = _filter_values(filter, ((x[None, :] + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    w = np.where(live, w, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                       # a running sum: ascending order, as the C loop (the padding adds exact zeros)
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    q = w * float(1 << PRECISION_BITS)
    coeffs = np.trunc(np.where(w < 0, -0.5 + q, 0.5 + q)).astype(np.int32)
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    coeffs.setflags(write=False)
    bounds.setflags(write=False)
    return Tables(np.ascontiguousarray(coeffs), np.ascontiguousarray(bounds), ksize)


# ------------------------------------------------------------------------------------------------ torchvision's size rules (unpinned)
def resized_size(w, h, size):
    """(new_w, new_h) of torchvision.transforms.Resize(size) with an int ``size``: the short side becomes ``size``, the long side
    ``int(size * long / short)``; unchanged when the short side already equals ``size``."""
    short, long = (w, h) if w <= h else (h, w)
    if short == size:
        return w, h
    new_short, new_long = size, int(size * long / short)
    return (new_short, new_long) if w <= h else (new_long, new_short)


def center_crop_offsets(h, w, size, crop=None):
    """(top, left) of torchvision.transforms.CenterCrop(crop) on an h x w image that is at least crop x crop; ``crop`` defaults to
    ``size``, the Resize(size) -> CenterCrop(size) of the SD scripts (Resize(232) -> CenterCrop(224) passes crop=224)."""
    crop = size if crop is None else int(crop)
    return int(round((h - crop) / 2.0)), int(round((w - crop) / 2.0))


def _filter_name(interpolation):
    name = str(interpolation).lower()
    if name not in FILTERS:
        raise ValueError(f"interpolation must be one of {sorted(FILTERS)}, got {interpolation!r}")
    return name


# ------------------------------------------------------------------------------------------------ the transform on the host
def sd_transform(pil_image, size, interpolation="bicubic", crop=None):
    """get_transform of SD/train-scripts/dataset.py up to the bytes: Resize(size, interpolation) -> CenterCrop(size) -> convert("RGB"),
    as uint8 [size, size, 3] on the host with Pillow.  The yardstick of ``sd_transform_gpu`` and its route for the modes the device does
    not take."""
    img = pil_image if isinstance(pil_image, Image.Image) else Image.fromarray(np.asarray(pil_image, dtype=np.uint8))
    w, h = img.size
    nw, nh = resized_size(w, h, size)
    if (nw, nh) != (w, h):
        img = img.resize((nw, nh), _PIL_FILTER[_filter_name(interpolation)])
    crop = size if crop is None else int(crop)
    top, left = center_crop_offsets(nh, nw, size, crop)
    img = img.crop((left, top, left + crop, top + crop)).convert("RGB")
    return np.array(img, dtype=np.uint8)                   # (a copy the caller owns: np.asarray of a PIL image is read-only)


# ------------------------------------------------------------------------------------------------ the transform on the device
def image_resample_u8(src, Hs, Ws, tx, ty, tmp, dst, tmp_bytes=None):
    """sfron_image_resample_u8 behind the checks that need the tables' contents (include/sfron.h: "who checks what"): returns the status,
    _lib.ERR_ARG before any upload or launch when a bound reaches outside the Hs x Ws source, the row bounds do not ascend, or
    ``tmp_bytes`` (default: all of ``tmp``) is below (y1 - y0) * Wo * 3.  src / tmp / dst: device uint8 tensors (None is passed on as a
    null pointer, which the entry point refuses); tx / ty: Tables of the window's columns / rows."""
    Wo, Ho = int(tx.bounds.shape[0]), int(ty.bounds.shape[0])
    for t, n_in in ((tx, Ws), (ty, Hs)):
        b = t.bounds.astype(np.int64)
        if (b[:, 0] < 0).any() or (b[:, 1] < 0).any() or (b[:, 0] + b[:, 1] > n_in).any() or (b[:, 1] > t.ksize).any():
            return _lib.ERR_ARG
    by = ty.bounds.astype(np.int64)
    if (np.diff(by[:, 0]) < 0).any() or (np.diff(by[:, 0] + by[:, 1]) < 0).any():
        return _lib.ERR_ARG
    y0, y1 = ty.rows()
    if tmp_bytes is None:
        tmp_bytes = 0 if tmp is None else tmp.numel()
    if tmp_bytes < (y1 - y0) * Wo * 3 or (tmp is not None and tmp.numel() < tmp_bytes):
        return _lib.ERR_ARG
    if dst is not None and dst.numel() < Ho * Wo * 3 or src is not None and src.numel() < Hs * Ws * 3:
        return _lib.ERR_ARG
    dev = next((t.device for t in (src, tmp, dst) if t is not None), None)
    if dev is None:
        return _lib.ERR_ARG
    kx, bx = tx.device(dev)
    ky, by_d = ty.device(dev)
    p = lambda t: None if t is None else _lib.ptr(t)
    return _lib.lib().sfron_image_resample_u8(p(src), Hs, Ws, p(kx), p(bx), tx.ksize, p(ky), p(by_d), ty.ksize, Wo, Ho, p(tmp), int(tmp_bytes),
                                              p(dst), stream_ptr())


def window_tables(w, h, size, interpolation="bicubic", crop=None):
    """(tx, ty) of the crop x crop (default size x size) centre-crop window of the resize of a w x h image (``resized_size`` +
    ``center_crop_offsets``)."""
    name = _filter_name(interpolation)
    crop = size if crop is None else int(crop)
    nw, nh = resized_size(w, h, size)
    top, left = center_crop_offsets(nh, nw, size, crop)
    return resample_tables(w, nw, name, left, crop), resample_tables(h, nh, name, top, crop)


class _Staging:
    """The buffers ``sd_transform_gpu`` reuses across calls on one device, grown on demand: a pinned host buffer the decoded pixels are
    gathered into, its device copy, and the horizontal pass's tmp.  One upload per call, on the current stream; the pinned buffer is
    written again only after the previous call's copy has finished (an event, waited on by the host)."""

    def __init__(self, dev):
        self.dev, self.host, self.src, self.tmp, self.done = dev, None, None, None, None

    def host_bytes(self, n):
        if self.done is not None:
            self.done.synchronize()
            self.done = None
        if self.host is None or self.host.numel() < n:
            self.host = torch.empty(max(n, 1 << 20), dtype=torch.uint8).pin_memory()
        return self.host

    def upload(self, n):
        if self.src is None or self.src.numel() < n:
            self.src = torch.empty(self.host.numel(), dtype=torch.uint8, device=self.dev)
        self.src[:n].copy_(self.host[:n], non_blocking=True)
        self.done = torch.cuda.Event()
        self.done.record(torch.cuda.current_stream(self.dev))
        return self.src

    def tmp_bytes(self, n):
        if self.tmp is None or self.tmp.numel() < n:
            self.tmp = torch.empty(max(n, 1 << 20), dtype=torch.uint8, device=self.dev)
        return self.tmp


_staging = {}


def _rgb_array(img):
    """uint8 [H, W, 3] of an image the device takes (RGB; L replicated to RGB, which commutes with the per-channel resize), else None."""
    if isinstance(img, Image.Image):
        if img.mode == "L":
            img = img.convert("RGB")
        if img.mode != "RGB":
            return None
        return np.asarray(img, dtype=np.uint8)
    a = img.numpy() if isinstance(img, torch.Tensor) else np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"sd_transform_gpu takes PIL images or uint8 [H, W, 3] arrays, got {a.dtype} {a.shape}")
    return a


def sd_transform_gpu(images, size, interpolation="bicubic", out=None, device="cuda"):
    """``sd_transform`` of a list of images on the GPU: device uint8 [B, size, size, 3], bit-identical to the host route.  images: PIL
    images or host uint8 [H, W, 3] arrays.  RGB (and L, replicated) pixels are gathered into one pinned buffer, uploaded with one copy on
    the current stream and resampled by sfron_image_resample_u8, two launches per image; any other mode (P, 1, RGBA, LA, CMYK, 16-bit:
    Pillow resizes those with other rules, and the reference resizes before it converts) is transformed on the host by ``sd_transform``
    and travels in the same upload."""
    size = int(size)
    dev = torch.device(out.device if out is not None else device)
    if dev.type != "cuda":
        raise _lib.SfronError("sd_transform_gpu needs a GPU (sd_transform is the host route)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    B = len(images)
    if out is None:
        out = torch.empty(B, size, size, 3, dtype=torch.uint8, device=dev)
    if tuple(out.shape) != (B, size, size, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError(f"out must be contiguous uint8 {(B, size, size, 3)}")
    items, total = [], 0
    for img in images:
        a = _rgb_array(img)
        ready = a is None
        if ready:
            a = sd_transform(img, size, interpolation)
        items.append((a, total, ready))
        total += (a.size + 15) // 16 * 16
    st = _staging.setdefault(dev, _Staging(dev))
    host = st.host_bytes(total).numpy()
    for a, off, _ in items:
        host[off:off + a.size] = a.reshape(-1)
    src = st.upload(total)
    for i, (a, off, ready) in enumerate(items):
        if ready:
            out[i].copy_(src[off:off + a.size].view(size, size, 3))
            continue
        h, w = a.shape[:2]
        tx, ty = window_tables(w, h, size, interpolation)
        y0, y1 = ty.rows()
        tmp = st.tmp_bytes((y1 - y0) * size * 3)
        _lib.check(image_resample_u8(src[off:off + a.size], h, w, tx, ty, tmp, out[i], tmp_bytes=(y1 - y0) * size * 3), "image_resample_u8")
    return out
