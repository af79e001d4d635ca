"""Frechet Inception Distance of image folders and ``.npz`` sample files over ``inception.InceptionV3`` and csrc/inception.hip.

``InceptionFeatures``  the extractor: uint8 batches, a folder of image files (listing and decoding as classify.py) or an ``.npz`` whose
                       ``arr_0`` holds NHWC bytes (what dit_sample.create_npz_from_sample_folder and the ADM suite write) -> fp32 [n][D]
                       appended to a buffer that stays on the device.
``feature_statistics`` mean and covariance of that buffer in fp64 on the device (sfron_feature_stats: np.mean / np.cov's arithmetic).
``FIDStatistics``      DDPM/evaluator.py:108-156: ``frechet_distance`` with its singular-product retry and imaginary-part check, plus
                       ``save`` / ``load`` (an ``.npz`` with ``mu`` and ``sigma``) so that a real set's statistics are computed once.
``fid_folders``        the shape of SD/eval-scripts/compute-fid.py: two folders, one feature width, optionally resized first.
``fid_npz``            the FID line of DDPM/evaluator.py:main: a reference and a sample ``.npz``.

The matrix square root of the Frechet distance is ``scipy.linalg.sqrtm`` in fp64 ON THE HOST, as in the reference: that step is not a
kernel.  Everything before it -- resize, network, statistics -- runs on the device.  No pretrained weights ship with the project: the
drivers take the path of a checkpoint holding the published ``pt_inception-2015-12-05`` state dict and refuse to run
without one.  Inception Score, precision and recall over the same feature buffer are evaluator.py.  Not built: sFID, data-parallel
extraction, fp8.
"""
import warnings

import numpy as np
import torch
from PIL import Image
from scipy import linalg

from . import _lib, classify, inception
from ._lib import check, ptr, stream_ptr
from .forward_net import guard


# ------------------------------------------------------------------------------------------------ statistics
class FIDStatistics:
    """``mu`` [D] and ``sigma`` [D][D] as fp64 numpy arrays (DDPM/evaluator.py:108-156)."""

    def __init__(self, mu, sigma):
        self.mu = mu
        self.sigma = sigma

    def frechet_distance(self, other, eps=1e-6):
        """|mu1 - mu2|^2 + tr(sigma1) + tr(sigma2) - 2 tr(sqrtm(sigma1 sigma2)); host fp64 (scipy), not a kernel."""
        mu1, sigma1 = np.atleast_1d(self.mu), np.atleast_2d(self.sigma)
        mu2, sigma2 = np.atleast_1d(other.mu), np.atleast_2d(other.sigma)
        assert mu1.shape == mu2.shape, f"Training and test mean vectors have different lengths: {mu1.shape}, {mu2.shape}"
        assert sigma1.shape == sigma2.shape, f"Training and test covariances have different dimensions: {sigma1.shape}, {sigma2.shape}"
        diff = mu1 - mu2
        covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)        # product might be almost singular
        if not np.isfinite(covmean).all():
            warnings.warn("fid calculation produces singular product; adding %s to diagonal of cov estimates" % eps)
            offset = np.eye(sigma1.shape[0]) * eps
            covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
        if np.iscomplexobj(covmean):                          # numerical error might give slight imaginary component
            if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
                raise ValueError("Imaginary component {}".format(np.max(np.abs(covmean.imag))))
            covmean = covmean.real
        return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, mu=np.asarray(self.mu, dtype=np.float64), sigma=np.asarray(self.sigma, dtype=np.float64))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            if "mu" not in z.files or "sigma" not in z.files:
                raise KeyError(f"{path}: no mu / sigma (keys {z.files})")
            return cls(np.asarray(z["mu"], dtype=np.float64), np.asarray(z["sigma"], dtype=np.float64))


def feature_statistics(features):
    """FIDStatistics of fp32 activations [N][D] resident on the device: np.mean(axis=0) and np.cov(rowvar=False) in fp64, one launch
    pair; only mu and sigma leave the device."""
    x = features
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        raise _lib.SfronError("feature_statistics takes fp32 [N][D] activations on the GPU (no CPU fallback)")
    N, D = x.shape
    if N < 2:
        raise ValueError(f"feature_statistics needs at least 2 samples, got {N}")
    x = x.contiguous()
    mu = torch.empty(D, dtype=torch.float64, device=x.device)
    sigma = torch.empty(D, D, dtype=torch.float64, device=x.device)
    guard(x, sigma)
    check(_lib.lib().sfron_feature_stats(ptr(x), N, D, D, ptr(mu), ptr(sigma), stream_ptr()), "feature_stats")
    return FIDStatistics(mu.cpu().numpy(), sigma.cpu().numpy())


# ------------------------------------------------------------------------------------------------ extraction
def load_model(checkpoint, device="cuda", **kw):
    """``inception.InceptionV3`` with the state dict stored at ``checkpoint`` (a torch file; FID ignores its ``fc.*``, the Inception Score of
    evaluator.py reads ``fc.weight``)."""
    if not checkpoint:
        raise ValueError("FID needs the Inception checkpoint: pass checkpoint=<path of the pt_inception-2015-12-05 state dict> "
                         "(no pretrained weights ship with this project, see INTEGRATION.md)")
    sd = torch.load(checkpoint, map_location="cpu", weights_only=True)
    return inception.InceptionV3(device=device, **kw).load_state_dict(sd)


class InceptionFeatures:
    """Collects the ``feature``-wide pooled activations of everything it is fed in one device buffer fp32 [capacity][D] (grown by
    doubling); ``features()`` is the view of the rows filled so far."""

    def __init__(self, model, feature=2048, batch_size=64):
        if feature not in inception.TAPS:
            raise ValueError(f"feature must be one of {inception.TAPS}, got {feature}")
        self.model, self.feature, self.batch_size = model, int(feature), int(batch_size)
        self.n = 0
        self._buf = torch.empty(0, self.feature, dtype=torch.float32, device=model.dev)

    def _reserve(self, more):
        need = self.n + more
        if need > self._buf.shape[0]:
            new = torch.empty(max(need, 2 * self._buf.shape[0]), self.feature, dtype=torch.float32, device=self.model.dev)
            new[:self.n] = self._buf[:self.n]
            self._buf = new

    def add_images(self, images_u8_nhwc):
        """uint8 [B, H, W, 3] (host or device, numpy or torch)."""
        x = torch.as_tensor(images_u8_nhwc)
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
            raise ValueError(f"add_images takes uint8 [B, H, W, 3], got {x.dtype} {tuple(x.shape)}")
        self._reserve(x.shape[0])
        for lo in range(0, x.shape[0], self.batch_size):
            part = x[lo:lo + self.batch_size]
            self._buf[self.n:self.n + part.shape[0]] = self.model.forward_u8(part, taps=(self.feature,))[self.feature]
            self.n += part.shape[0]
        return self

    def add_folder(self, folder, image_size=None, interpolation="bicubic"):
        """Every image file of ``folder`` (classify.image_paths).  With ``image_size`` each is first resized to image_size x image_size by
        the Pillow-exact GPU resize (setup_fid_data's transform); without, files are decoded on the host and batched by equal size."""
        files = classify.image_paths(folder)
        if not files:
            raise FileNotFoundError(f"{folder}: no image files")
        if image_size is not None:
            for lo in range(0, len(files), self.batch_size):
                self.add_images(classify.load_images_u8(files[lo:lo + self.batch_size], (image_size, image_size), interpolation=interpolation,
                                                        device=self.model.dev))
            return self
        run = []
        for p in files:
            with Image.open(p) as im:
                a = np.asarray(im.convert("RGB"), dtype=np.uint8)
            if run and (a.shape != run[0].shape or len(run) == self.batch_size):
                self.add_images(np.stack(run))
                run = []
            run.append(a)
        self.add_images(np.stack(run))
        return self

    def add_npz(self, path):
        with np.load(path) as z:
            if "arr_0" not in z.files:
                raise KeyError(f"{path}: no arr_0 (keys {z.files})")
            arr = z["arr_0"]
        if arr.shape[0] == 0:
            raise ValueError(f"{path}: arr_0 is empty")
        return self.add_images(arr)

    def features(self):
        return self._buf[:self.n]

    def statistics(self):
        return feature_statistics(self.features())


# ------------------------------------------------------------------------------------------------ drivers
def _model(model, checkpoint):
    return model if model is not None else load_model(checkpoint)


def fid_folders(real, fake, feature=2048, image_size=None, checkpoint=None, model=None, batch_size=64):
    """SD/eval-scripts/compute-fid.py: FID between the images of two folders at one feature width (the reference asks torchmetrics for 64).
    The resized BYTES go to the network; the reference's cast of Normalize()d floats to uint8 is not reproduced."""
    if feature not in inception.TAPS:
        raise ValueError(f"feature must be one of {inception.TAPS}, got {feature}")
    model = _model(model, checkpoint)
    stats = [InceptionFeatures(model, feature, batch_size).add_folder(f, image_size).statistics() for f in (real, fake)]
    return stats[1].frechet_distance(stats[0])


def fid_npz(ref, sample, feature=2048, checkpoint=None, model=None, batch_size=64):
    """The FID line of DDPM/evaluator.py:main: ``sample_stats.frechet_distance(ref_stats)``.  A ``ref`` file that carries ``mu`` and
    ``sigma`` (FIDStatistics.save, or the ADM suite's reference batches) is not run through the network again."""
    if feature not in inception.TAPS:
        raise ValueError(f"feature must be one of {inception.TAPS}, got {feature}")
    model = _model(model, checkpoint)
    with np.load(ref) as z:
        has_stats = "mu" in z.files and "sigma" in z.files
    ref_stats = FIDStatistics.load(ref) if has_stats else InceptionFeatures(model, feature, batch_size).add_npz(ref).statistics()
    if ref_stats.mu.shape[0] != feature:
        raise ValueError(f"{ref}: statistics of width {ref_stats.mu.shape[0]}, feature is {feature}")
    return InceptionFeatures(model, feature, batch_size).add_npz(sample).statistics().frechet_distance(ref_stats)
