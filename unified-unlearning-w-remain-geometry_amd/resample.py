"""The image transform of the SD scripts (SD/train-scripts/dataset.py:23-33: Resize(size, bicubic) -> CenterCrop(size) -> RGB; ToTensor and
Normalize(0.5, 0.5) are the encoder's uint8 input kernel) on the host with Pillow and on the GPU with csrc/resample.hip.

``torchvision.transforms.Resize`` on a PIL image is ``Image.resize``: Pillow's separable fixed-point convolution (src/libImaging/Resample.c,
8-bit path, PRECISION_BITS = 22).  It is integer arithmetic over coefficients that are made once per axis in float64, so the GPU version is
specified bit for bit: ``resample_tables`` restates the coefficient computation on the host, sfron_image_resample_u8 does the two integer
passes.  The centre crop is folded in: the tables are sliced to the crop window, so only the window is computed.

ADM's centre crop of the DiT scripts (DiT/forget.py:89-107, latents.center_crop_arr: BOX halvings, BICUBIC, crop) is a chain of such
resizes: ``center_crop_plan`` makes its table pairs with the crop folded back through every stage, ``plan_batch`` lays a batch of chains
out as the pool / tables / pass records that sfron_image_resample_batch_u8 runs in one launch per level, and ``center_crop_gpu`` is the
whole route from decoded images.

torchvision is not part of this project's environment: ``resized_size`` and ``center_crop_offsets`` restate its published rules and are not
pinned by a fixture.
"""
import functools
import math
import threading

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


# ------------------------------------------------------------------------------------------------ ADM's center_crop_arr, planned
class Stage:
    """One resize of a chain.  ``tx`` / ``ty``: the Tables of the columns / rows it forms, their bounds indexing the FULL image of the
    previous stage; ``ox`` / ``oy`` / ``in_w`` / ``in_h``: origin and extents of the window of that image which is actually held (the
    whole source for a first stage), so an executor reads index ``bound - origin``."""
    __slots__ = ("tx", "ty", "ox", "oy", "in_w", "in_h")

    def __init__(self, tx, ty, ox, oy, in_w, in_h):
        self.tx, self.ty, self.ox, self.oy, self.in_w, self.in_h = tx, ty, int(ox), int(oy), int(in_w), int(in_h)


class CropPlan:
    """``center_crop_plan``'s result: ``stages`` (BOX halvings, then BICUBIC), ``sizes`` = the (w, h) of the source and of every stage's
    full image, ``halvings`` and the crop's ``(left, top)`` in the last of them."""

    def __init__(self, stages, sizes, crop):
        self.stages, self.sizes, self.crop, self.halvings = tuple(stages), tuple(sizes), crop, len(sizes) - 2


@functools.lru_cache(maxsize=512)
def center_crop_plan(w, h, image_size):
    """The stages of ``latents.center_crop_arr`` (ADM's centre crop, DiT/forget.py:89-107) for one w x h RGB image, sizes as the reference
    text forms them: halve (``d // 2``, BOX) while ``min(size) >= 2 * image_size``; then ``s = image_size / min(size)`` and BICUBIC to
    ``round(d * s)``; then crop ``image_size`` from ``(n - image_size) // 2``.  The crop is folded back through the chain: the BICUBIC
    tables are sliced to the crop window, every BOX stage to the union of the indices the next stage reads (``Tables.rows()``), so no
    stage forms a pixel that nothing reads.  Cached, with the tables."""
    w, h, S = int(w), int(h), int(image_size)
    if w < 1 or h < 1 or S < 1:
        raise ValueError(f"center_crop_plan: w {w}, h {h}, image_size {S}")
    sizes = [(w, h)]
    while min(sizes[-1]) >= 2 * S:
        sizes.append(tuple(d // 2 for d in sizes[-1]))
    s = S / min(sizes[-1])
    sizes.append(tuple(round(d * s) for d in sizes[-1]))
    left, top = (sizes[-1][0] - S) // 2, (sizes[-1][1] - S) // 2
    pairs = [(resample_tables(sizes[-2][0], sizes[-1][0], "bicubic", left, S), resample_tables(sizes[-2][1], sizes[-1][1], "bicubic", top, S))]
    windows = [(left, top)]                                  # first column / row each stage forms, in its own full image
    for k in range(len(sizes) - 2, 0, -1):                   # the BOX stage sizes[k - 1] -> sizes[k], cut to what the stage after it reads
        (x0, x1), (y0, y1) = pairs[0][0].rows(), pairs[0][1].rows()
        pairs.insert(0, (resample_tables(sizes[k - 1][0], sizes[k][0], "box", x0, x1 - x0), resample_tables(sizes[k - 1][1], sizes[k][1], "box", y0, y1 - y0)))
        windows.insert(0, (x0, y0))
    stages = []
    for i, (tx, ty) in enumerate(pairs):
        if i == 0:
            stages.append(Stage(tx, ty, 0, 0, w, h))
        else:
            stages.append(Stage(tx, ty, windows[i - 1][0], windows[i - 1][1], pairs[i - 1][0].bounds.shape[0], pairs[i - 1][1].bounds.shape[0]))
    return CropPlan(stages, sizes, (left, top))


# ------------------------------------------------------------------------------------------------ a batch of chains on the device
PASS_WORDS = 16                     # sfron_resample_pass: 16 x int64 (include/sfron.h)
(P_IN_BUF, P_IN_OFF, P_IN_W, P_IN_H, P_OUT_BUF, P_OUT_OFF, P_N_OUT, P_ORG, P_ROW0, P_NROWS, P_K_OFF, P_B_OFF, P_KSIZE) = range(13)
_ALIGN = 16


def _up(n, a=_ALIGN):
    return (n + a - 1) // a * a


class BatchPlan:
    """What sfron_image_resample_batch_u8 takes, on the host: ``tables`` (int32 blob), ``passes`` (int64 [n][PASS_WORDS], grouped by
    level), ``level_first`` / ``level_rows`` / ``level_cols`` (int32), the byte sizes the records assume of the pool, the work buffer and
    ``out``, and ``src_off`` (where each source lies in the pool).  ``n_levels`` is the number of launches."""

    def __init__(self, tables, passes, level_first, level_rows, level_cols, src_off, src_shape, pool_bytes, work_bytes, out_bytes):
        self.tables, self.passes = tables, passes
        self.level_first, self.level_rows, self.level_cols = level_first, level_rows, level_cols
        self.src_off, self.src_shape = src_off, src_shape
        self.pool_bytes, self.work_bytes, self.out_bytes = int(pool_bytes), int(work_bytes), int(out_bytes)

    @property
    def n_levels(self):
        return int(self.level_rows.shape[0])

    # one host buffer for one upload: records | tables | pool
    @property
    def tables_at(self):
        return _up(self.passes.size * 8)

    @property
    def pool_at(self):
        return _up(self.tables_at + self.tables.size * 4)

    @property
    def host_bytes(self):
        return self.pool_at + self.pool_bytes

    def fill(self, host, sources):
        """Gather records, tables and the pixels of ``sources`` (uint8 [h, w, 3] arrays, in the plan's order) into ``host`` (uint8 numpy)."""
        host[:self.passes.size * 8] = self.passes.reshape(-1).view(np.uint8)
        host[self.tables_at:self.tables_at + self.tables.size * 4] = self.tables.view(np.uint8)
        pool = host[self.pool_at:self.pool_at + self.pool_bytes]
        for a, off, (h, w) in zip(sources, self.src_off, self.src_shape):
            if a.shape != (h, w, 3) or a.dtype != np.uint8:
                raise ValueError(f"source {a.dtype} {a.shape} does not match the plan's {(h, w, 3)}")
            pool[off:off + a.size] = a.reshape(-1)

    def validate(self, pool_bytes=None, work_bytes=None, out_bytes=None):
        """The checks that need the records' and tables' contents (include/sfron.h: "who checks what"), on the host: True when every
        pass reads inside its input, its row bounds ascend, its offsets and extents lie inside pool / work / out / tables of the given
        sizes (default: the plan's own), and no pass reads or writes what another pass of its level writes."""
        cap = {_lib.RESAMPLE_POOL: self.pool_bytes if pool_bytes is None else int(pool_bytes),
               _lib.RESAMPLE_WORK: self.work_bytes if work_bytes is None else int(work_bytes),
               _lib.RESAMPLE_OUT: self.out_bytes if out_bytes is None else int(out_bytes)}
        P, T, lf = self.passes, self.tables, self.level_first
        L = self.n_levels
        if P.ndim != 2 or P.shape[1] != PASS_WORDS or P.dtype != np.int64 or T.dtype != np.int32 or T.ndim != 1:
            return False
        if L < 2 or L % 2 or lf.shape[0] != L + 1 or lf[0] != 0 or lf[-1] != P.shape[0] or (np.diff(lf) < 1).any():
            return False
        for l in range(L):
            horizontal = l % 2 == 0
            reads, writes = [], []
            for p in P[lf[l]:lf[l + 1]].tolist():
                in_buf, in_off, in_w, in_h, out_buf, out_off, n_out = p[P_IN_BUF], p[P_IN_OFF], p[P_IN_W], p[P_IN_H], p[P_OUT_BUF], p[P_OUT_OFF], p[P_N_OUT]
                org, row0, nrows, k_off, b_off, ks = p[P_ORG], p[P_ROW0], p[P_NROWS], p[P_K_OFF], p[P_B_OFF], p[P_KSIZE]
                if in_buf not in ((_lib.RESAMPLE_POOL, _lib.RESAMPLE_WORK) if horizontal else (_lib.RESAMPLE_WORK,)):
                    return False
                if out_buf not in ((_lib.RESAMPLE_WORK,) if horizontal else (_lib.RESAMPLE_WORK, _lib.RESAMPLE_OUT)):
                    return False
                if min(in_w, in_h, n_out, ks) < 1 or in_w * 3 >= 1 << 31 or n_out * 3 >= 1 << 31:
                    return False
                if in_off < 0 or in_off + in_h * in_w * 3 > cap[in_buf]:
                    return False
                if horizontal and (row0 < 0 or nrows < 1 or row0 + nrows > in_h):
                    return False
                out_n = nrows * n_out * 3 if horizontal else n_out * in_w * 3
                if out_off < 0 or out_off + out_n > cap[out_buf]:
                    return False
                if k_off < 0 or b_off < 0 or k_off + n_out * ks > T.shape[0] or b_off + 2 * n_out > T.shape[0]:
                    return False
                b = T[b_off:b_off + 2 * n_out].reshape(n_out, 2).astype(np.int64)
                first, count = b[:, 0] - org, b[:, 1]
                if (first < 0).any() or (count < 0).any() or (count > ks).any() or (first + count > (in_w if horizontal else in_h)).any():
                    return False
                if not horizontal and ((np.diff(first) < 0).any() or (np.diff(first + count) < 0).any()):
                    return False
                if horizontal:
                    reads.append((in_buf, in_off + row0 * in_w * 3, in_off + (row0 + nrows) * in_w * 3))
                else:
                    reads.append((in_buf, in_off, in_off + in_h * in_w * 3))
                writes.append((out_buf, out_off, out_off + out_n))
            for i, (wb, w0, w1) in enumerate(writes):
                for j, (ob, o0, o1) in enumerate(reads + writes):
                    if j != len(reads) + i and ob == wb and o0 < w1 and w0 < o1:
                        return False
        return True


def plan_batch(chains, src_off=None, out_off=None):
    """The BatchPlan of a batch of chains (one list of ``Stage`` per image; ``CropPlan.stages``, or a single ``Stage`` for a plain
    resize window).  ``src_off``: byte offset of each source in the pool (default: packed at multiples of 16; any alignment runs);
    ``out_off``: byte offset of each result in ``out`` (default: packed in order).  Level 2s holds the horizontal passes of stage s,
    2s + 1 the vertical ones; an image's last vertical pass writes ``out``.  In the work buffer an image owns one region for its
    horizontal results and one for its stage images: a level only ever reads what the level before it wrote."""
    n = len(chains)
    if n < 1 or any(len(c) < 1 for c in chains):
        raise ValueError("plan_batch needs at least one image and one stage per image")
    blob, where, n_words = [], {}, 0

    def put(arr):
        nonlocal n_words
        key = id(arr)
        if key not in where:
            where[key] = n_words
            blob.append(arr.reshape(-1))
            n_words += arr.size
        return where[key]

    if src_off is None:
        src_off, at = [], 0
        for c in chains:
            src_off.append(at)
            at = _up(at + c[0].in_w * c[0].in_h * 3)
    if out_off is None:
        out_off, at = [], 0
        for c in chains:
            out_off.append(at)
            at += c[-1].tx.bounds.shape[0] * c[-1].ty.bounds.shape[0] * 3
    pool_bytes = max(o + c[0].in_w * c[0].in_h * 3 for o, c in zip(src_off, chains))
    out_bytes = max(o + c[-1].tx.bounds.shape[0] * c[-1].ty.bounds.shape[0] * 3 for o, c in zip(out_off, chains))
    L = 2 * max(len(c) for c in chains)
    levels = [[] for _ in range(L)]
    work_at = 0
    for i, c in enumerate(chains):
        rows = [st.ty.rows() for st in c]
        a_bytes = max((y1 - y0) * st.tx.bounds.shape[0] * 3 for st, (y0, y1) in zip(c, rows))
        b_bytes = max([st.tx.bounds.shape[0] * st.ty.bounds.shape[0] * 3 for st in c[:-1]] + [0])
        a_off, b_off = work_at, _up(work_at + a_bytes)
        work_at = _up(b_off + b_bytes)
        for s, (st, (y0, y1)) in enumerate(zip(c, rows)):
            wo, ho = st.tx.bounds.shape[0], st.ty.bounds.shape[0]
            last = s == len(c) - 1
            hp, vp = [0] * PASS_WORDS, [0] * PASS_WORDS
            hp[P_IN_BUF], hp[P_IN_OFF] = (_lib.RESAMPLE_POOL, src_off[i]) if s == 0 else (_lib.RESAMPLE_WORK, b_off)
            hp[P_IN_W], hp[P_IN_H], hp[P_OUT_BUF], hp[P_OUT_OFF], hp[P_N_OUT] = st.in_w, st.in_h, _lib.RESAMPLE_WORK, a_off, wo
            hp[P_ORG], hp[P_ROW0], hp[P_NROWS] = st.ox, y0 - st.oy, y1 - y0
            hp[P_K_OFF], hp[P_B_OFF], hp[P_KSIZE] = put(st.tx.coeffs), put(st.tx.bounds), st.tx.ksize
            vp[P_IN_BUF], vp[P_IN_OFF], vp[P_IN_W], vp[P_IN_H] = _lib.RESAMPLE_WORK, a_off, wo, y1 - y0
            vp[P_OUT_BUF], vp[P_OUT_OFF] = (_lib.RESAMPLE_OUT, out_off[i]) if last else (_lib.RESAMPLE_WORK, b_off)
            vp[P_N_OUT], vp[P_ORG], vp[P_ROW0], vp[P_NROWS] = ho, y0, 0, y1 - y0
            vp[P_K_OFF], vp[P_B_OFF], vp[P_KSIZE] = put(st.ty.coeffs), put(st.ty.bounds), st.ty.ksize
            levels[2 * s].append(hp)
            levels[2 * s + 1].append(vp)
    passes = np.array([p for lv in levels for p in lv], dtype=np.int64)
    level_first = np.cumsum([0] + [len(lv) for lv in levels]).astype(np.int32)
    level_rows = np.array([max(p[P_NROWS] if l % 2 == 0 else p[P_N_OUT] for p in lv) for l, lv in enumerate(levels)], dtype=np.int32)
    level_cols = np.array([max(p[P_N_OUT] if l % 2 == 0 else p[P_IN_W] * 3 for p in lv) for l, lv in enumerate(levels)], dtype=np.int32)
    return BatchPlan(np.concatenate(blob).astype(np.int32, copy=False), passes, level_first, level_rows, level_cols, list(src_off),
                     [(c[0].in_h, c[0].in_w) for c in chains], pool_bytes, max(work_at, 1), out_bytes)


def _launch_batch(bp, pool, tables, passes, work, out, pool_bytes, work_bytes, out_bytes):
    a = lambda v: v.ctypes.data
    return _lib.lib().sfron_image_resample_batch_u8(pool, int(pool_bytes), tables, int(bp.tables.size), passes, int(bp.passes.shape[0]),
                                                    a(bp.level_first), a(bp.level_rows), a(bp.level_cols), bp.n_levels, work, int(work_bytes),
                                                    out, int(out_bytes), stream_ptr())


def image_resample_batch_u8(bp, pool, work, out, pool_bytes=None, work_bytes=None, out_bytes=None):
    """sfron_image_resample_batch_u8 behind ``BatchPlan.validate``: returns the status, _lib.ERR_ARG before any upload or launch when the
    records or tables do not fit the buffers.  pool / work / out: device uint8 tensors (None is passed on as a null pointer, which the
    entry point refuses), their sizes the tensors' unless given; the tables and records are uploaded here.  ``bp.n_levels`` launches."""
    size = lambda t, n: (0 if t is None else t.numel()) if n is None else int(n)
    pool_bytes, work_bytes, out_bytes = size(pool, pool_bytes), size(work, work_bytes), size(out, out_bytes)
    if not bp.validate(pool_bytes, work_bytes, out_bytes):
        return _lib.ERR_ARG
    if any(t is not None and t.numel() < n for t, n in ((pool, pool_bytes), (work, work_bytes), (out, out_bytes))):
        return _lib.ERR_ARG
    dev = next((t.device for t in (pool, work, out) if t is not None), None)
    if dev is None:
        return _lib.ERR_ARG
    tables, passes = torch.from_numpy(bp.tables).to(dev), torch.from_numpy(bp.passes).to(dev)
    p = lambda t: None if t is None else _lib.ptr(t)
    return _launch_batch(bp, p(pool), p(tables), p(passes), p(work), p(out), pool_bytes, work_bytes, out_bytes)


class _Gathered:
    """One batch between ``CropStaging.gather`` and its launches: ``upload()`` copies the pinned bytes to a fresh device buffer on the
    current stream (and hands the pinned buffer back), ``run(buf)`` does the level launches on the current stream."""

    def __init__(self, staging, bp, host, n_images, size):
        self.staging, self.bp, self.host, self.n_images, self.size = staging, bp, host, n_images, size

    def upload(self):
        n = self.bp.host_bytes
        buf = torch.empty(n, dtype=torch.uint8, device=self.staging.dev)
        buf.copy_(self.host[:n], non_blocking=True)
        self.staging.release(self.host)
        self.host = None
        return buf

    def run(self, buf, out=None):
        bp, dev, S = self.bp, self.staging.dev, self.size
        if out is None:
            out = torch.empty(self.n_images, S, S, 3, dtype=torch.uint8, device=dev)
        work = torch.empty(bp.work_bytes, dtype=torch.uint8, device=dev)
        base = buf.data_ptr()
        _lib.check(_launch_batch(bp, base + bp.pool_at, base + bp.tables_at, base, _lib.ptr(work), _lib.ptr(out), bp.pool_bytes, bp.work_bytes,
                                 out.numel()), "image_resample_batch_u8")
        return out


class CropStaging:
    """The pinned host buffers ``center_crop_gpu`` and the DiT image loader gather into, reused across calls.  ``gather`` plans a batch
    and fills a free buffer with its records, tables and pixels; a buffer is free again once the upload that reads it has been queued,
    and is written again only after that copy has finished (an event of the copying stream, waited on by the host -- never the
    consumer's stream).  Several batches may be between gather and upload at once: a further buffer is made when none is free.  The
    device side (the uploaded bytes, the work buffer, the result) comes from the caching allocator on the stream that uses it."""

    def __init__(self, dev):
        self.dev, self._free, self._lock = torch.device(dev), [], threading.Lock()

    def _take(self, n):
        with self._lock:
            fit = [i for i, (h, _) in enumerate(self._free) if h.numel() >= n]
            host, done = self._free.pop(fit[0] if fit else 0) if self._free else (None, None)
        if done is not None:
            done.synchronize()
        if host is None or host.numel() < n:
            host = torch.empty(max(n, 1 << 20), dtype=torch.uint8).pin_memory()
        return host

    def release(self, host):
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(self.dev))
        with self._lock:
            self._free.append((host, done))

    def gather(self, images, image_size):
        S = int(image_size)
        arrays = [_crop_source(img) for img in images]
        bp = plan_batch([center_crop_plan(a.shape[1], a.shape[0], S).stages for a in arrays])
        if not bp.validate():
            raise _lib.SfronError("center_crop_gpu: the planned records do not validate")
        host = self._take(bp.host_bytes)
        bp.fill(host.numpy(), arrays)
        return _Gathered(self, bp, host, len(arrays), S)


def _crop_source(img):
    if isinstance(img, Image.Image):
        if img.mode != "RGB":
            raise ValueError(f"center_crop_gpu takes RGB images (convert first), got mode {img.mode!r}")
        return np.asarray(img, dtype=np.uint8)
    a = img.numpy() if isinstance(img, torch.Tensor) else np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"center_crop_gpu takes PIL RGB images or uint8 [H, W, 3] arrays, got {a.dtype} {a.shape}")
    return a


_crop_staging = {}


def crop_staging(dev):
    dev = torch.device(dev)
    if dev.type != "cuda":
        raise _lib.SfronError("center_crop_gpu needs a GPU (latents.center_crop_arr is the host route)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return _crop_staging.setdefault(dev, CropStaging(dev))


def center_crop_gpu(images, image_size, out=None, device="cuda"):
    """``latents.center_crop_arr`` of a list of images on the GPU: device uint8 [B, image_size, image_size, 3], bit-identical to the host
    route per image.  images: PIL RGB images or host uint8 [H, W, 3] arrays, of any sizes.  The pixels, the tables and the pass records
    of ``center_crop_plan`` are gathered into one pinned buffer and uploaded with one copy on the current stream; then
    sfron_image_resample_batch_u8 runs every chain in 2 * (1 + most halvings in the batch) launches, whatever the batch size."""
    S = int(image_size)
    st = crop_staging(out.device if out is not None else device)
    if out is not None and (tuple(out.shape) != (len(images), S, S, 3) or out.dtype != torch.uint8 or not out.is_contiguous()):
        raise ValueError(f"out must be contiguous uint8 {(len(images), S, S, 3)}")
    with torch.cuda.device(st.dev):
        g = st.gather(images, S)
        return g.run(g.upload(), out)
