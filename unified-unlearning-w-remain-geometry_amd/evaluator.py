"""Inception Score, FID, precision and recall of a sample set: the table row of DDPM/evaluator.py:main over csrc/manifold.hip.

``ManifoldEstimator``        the reference's class without the TensorFlow session: ``manifold_radii`` (k-th nearest-neighbour distances,
                             the self-distance counted, as ``np.partition`` over the full distance row counts it) and ``evaluate_pr``
                             (``DistanceBlock.less_thans`` fused into the product's tile).  Features are fp32 device tensors; radii stay on
                             the device between the two calls; the N x N distance matrix is never stored.
``compute_inception_score``  the 1008-way head WITHOUT its bias (``inception.InceptionV3.logits``), softmax, per-split exp(mean KL).
``compute_prec_recall``      the reference's ``Evaluator.compute_prec_recall``: (precision, recall) at nhood 3.
``evaluate_npz`` / ``evaluate_folders``  the drivers: each set goes through ``fid.InceptionFeatures`` ONCE at width 2048, and the four
                             numbers {"Inception Score", "FID", "Precision", "Recall"} come from that one buffer; with ``csv_path`` the
                             row is written through ``classify.update_result_csv``.

Every distance is the reference's fp32 branch, ``max(norm_u - 2 u.v + norm_v, 0)``, on the exact fp32-input matrix core instruction.
A probability that underflowed to 0 adds 0 to the Inception Score's KL sum (its limit; the reference's numpy gives NaN there).

Not built: sFID (its tap ``mixed_6/conv:0[..., :7]`` is a raw convolution output in front of a BatchNorm that is
folded at load here, and its identity under the published state dict's names cannot be confirmed offline); the fp16 first attempt of
``DistanceBlock`` (a TensorFlow throughput shortcut whose bits no other runtime reproduces); ``cv2.imread``'s BGR order of the reference's
``read_images_folder``; data-parallel evaluation; ``ManifoldEstimator.evaluate`` (realism scores, which the reference's main never calls).
"""
import ctypes

import numpy as np
import torch

from . import _lib, classify, fid
from ._lib import check, ptr, stream_ptr

MAX_NHOOD, MAX_NHOODS = 7, 4          # csrc/manifold.hip: a query keeps its 8 smallest distances; up to 4 radii per point


def _features(x, what):
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        raise _lib.SfronError(f"{what} takes fp32 [N][D] features on the GPU (no CPU fallback)")
    if x.shape[1] % 4 != 0:
        raise ValueError(f"{what}: the feature width must be a multiple of 4, got {x.shape[1]}")
    if x.stride(1) != 1 or x.stride(0) % 4 != 0 or x.stride(0) < x.shape[1] or x.data_ptr() % 16 != 0:
        x = x.contiguous()
    return x


class ManifoldEstimator:
    """DDPM/evaluator.py:258-422 without the session.  The batch sizes chunk the launches as they chunk the reference's loops; the
    result does not depend on them.  The 2 GiB operand rule holds per launch, i.e. per batch of rows: a batch that reaches it is refused by
    the entry point (``SfronError``); a whole set may be larger."""

    def __init__(self, row_batch_size=10000, col_batch_size=10000, nhood_sizes=(3,), clamp_to_percentile=None, eps=1e-5):
        self.row_batch_size = int(row_batch_size)
        self.col_batch_size = int(col_batch_size)
        self.nhood_sizes = tuple(int(k) for k in nhood_sizes)
        self.num_nhoods = len(self.nhood_sizes)
        self.clamp_to_percentile = clamp_to_percentile
        self.eps = eps
        if self.row_batch_size < 1 or self.col_batch_size < 1:
            raise ValueError("batch sizes must be positive")
        if not 1 <= self.num_nhoods <= MAX_NHOODS or any(not 1 <= k <= MAX_NHOOD for k in self.nhood_sizes):
            raise ValueError(f"nhood_sizes: 1 .. {MAX_NHOODS} sizes, each in 1 .. {MAX_NHOOD}, got {self.nhood_sizes}")

    def manifold_radii(self, features):
        """fp32 [N][K] on the device: radii[i][a] = the nhood_sizes[a]-th smallest squared distance from row i to every row, i included."""
        x = _features(features, "manifold_radii")
        N, D = x.shape
        if N <= max(self.nhood_sizes):
            raise ValueError(f"manifold_radii: {N} rows, kth(={max(self.nhood_sizes)}) out of bounds (np.partition raises there)")
        L = _lib.lib()
        nbytes = L.sfron_manifold_radii_workspace(N, self.row_batch_size, self.col_batch_size)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        radii = torch.empty(N, self.num_nhoods, dtype=torch.float32, device=x.device)
        nh = (ctypes.c_int * self.num_nhoods)(*self.nhood_sizes)
        check(L.sfron_manifold_radii_batched(x.data_ptr(), N, D, x.stride(0), self.row_batch_size, self.col_batch_size, nh, self.num_nhoods,
                                             ptr(radii), ptr(ws), nbytes, stream_ptr()), "manifold_radii")
        if self.clamp_to_percentile is not None:            # np.percentile on the host over the small radii array, as the reference
            r = radii.cpu().numpy()
            max_distances = np.percentile(r, self.clamp_to_percentile, axis=0)
            r[r > max_distances] = 0
            radii = torch.from_numpy(r).to(x.device)
        return radii

    def evaluate(self, features, radii, eval_features):
        raise NotImplementedError("ManifoldEstimator.evaluate (realism scores and nearest indices) is not built: the reference's main never "
                                  "calls it (DESIGN.md section 7)")

    def status(self, features_1, radii_1, features_2, radii_2):
        """(features_1_status uint8 [N1][K2], features_2_status uint8 [N2][K1]) on the device: the two flag arrays of evaluate_pr."""
        x1, x2 = _features(features_1, "evaluate_pr"), _features(features_2, "evaluate_pr")
        if x1.shape[1] != x2.shape[1]:
            raise ValueError(f"evaluate_pr: feature widths {x1.shape[1]} and {x2.shape[1]}")
        r = []
        for x, rad in ((x1, radii_1), (x2, radii_2)):
            rad = torch.as_tensor(rad, dtype=torch.float32).to(x.device).contiguous()
            if rad.dim() != 2 or rad.shape[0] != x.shape[0] or not 1 <= rad.shape[1] <= MAX_NHOODS:
                raise ValueError(f"evaluate_pr: radii of shape {tuple(rad.shape)} for {x.shape[0]} rows (1 .. {MAX_NHOODS} columns)")
            r.append(rad)
        N1, N2, K1, K2 = x1.shape[0], x2.shape[0], r[0].shape[1], r[1].shape[1]
        in1 = torch.zeros(N1, K2, dtype=torch.uint8, device=x1.device)
        in2 = torch.zeros(N2, K1, dtype=torch.uint8, device=x1.device)
        L = _lib.lib()
        for b1 in range(0, N1, self.row_batch_size):
            n1 = min(self.row_batch_size, N1 - b1)
            for b2 in range(0, N2, self.col_batch_size):
                n2 = min(self.col_batch_size, N2 - b2)
                check(L.sfron_manifold_pr(x1.data_ptr() + 4 * b1 * x1.stride(0), n1, r[0].data_ptr() + 4 * b1 * K1, K1,
                                          x2.data_ptr() + 4 * b2 * x2.stride(0), n2, r[1].data_ptr() + 4 * b2 * K2, K2, x1.shape[1],
                                          x1.stride(0), x2.stride(0), in1.data_ptr() + b1 * K2, in2.data_ptr() + b2 * K1, stream_ptr()),
                      "manifold_pr")
        return in1, in2

    def evaluate_pr(self, features_1, radii_1, features_2, radii_2):
        """(precision fp64 [K1], recall fp64 [K2]): the share of set 2 inside set 1's manifold, and of set 1 inside set 2's."""
        in1, in2 = self.status(features_1, radii_1, features_2, radii_2)
        return (np.mean(in2.cpu().numpy().astype(bool).astype(np.float64), axis=0),
                np.mean(in1.cpu().numpy().astype(bool).astype(np.float64), axis=0))


def inception_scores(logits, split_size=5000):
    """Per-split scores fp64 [ceil(N / split_size)] on the device from logits fp32 [N][C] (a copy is taken: the kernel works in place)."""
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype != torch.float32 or logits.dim() != 2:
        raise _lib.SfronError("inception_scores takes fp32 [N][C] logits on the GPU (no CPU fallback)")
    split_size = int(split_size)
    if split_size < 1 or logits.shape[0] < 1:
        raise ValueError("inception_scores needs at least one row and a positive split_size")
    p = logits.contiguous().clone()
    N, C = p.shape
    L = _lib.lib()
    nbytes = L.sfron_inception_score_workspace(N, C, split_size)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    scores = torch.empty((N + split_size - 1) // split_size, dtype=torch.float64, device=p.device)
    check(L.sfron_inception_score(ptr(p), N, C, C, split_size, ptr(scores), ptr(ws), nbytes, stream_ptr()), "inception_score")
    return scores


def compute_inception_score(model, features, split_size=5000):
    """DDPM/evaluator.py:228-245 over pooled features fp32 [N][2048] on the device: the mean of the per-split scores, a float."""
    return float(np.mean(inception_scores(model.logits(features), split_size).cpu().numpy()))


def compute_prec_recall(features_ref, features_sample):
    """DDPM/evaluator.py:247-255: (precision, recall) with the reference's default estimator (nhood 3)."""
    est = ManifoldEstimator()
    radii_1 = est.manifold_radii(features_ref)
    radii_2 = est.manifold_radii(features_sample)
    pr = est.evaluate_pr(features_ref, radii_1, features_sample, radii_2)
    return float(pr[0][0]), float(pr[1][0])


def default_name(ref):
    """The row name of the reference's main: ``ref.split("/")[-3] + "/" + ref.split("/")[-2]``."""
    parts = str(ref).split("/")
    if len(parts) < 3:
        raise ValueError(f"{ref}: the default row name takes the path's last two folders; pass name=")
    return parts[-3] + "/" + parts[-2]


def _evaluate(model, ref_feats, sample_feats, ref, csv_path, name):
    if getattr(model, "fc_weight", None) is None:
        raise _lib.SfronError("the Inception Score needs the 1008-way head: the checkpoint's state dict has no fc.weight")
    xr, xs = ref_feats.features(), sample_feats.features()
    precision, recall = compute_prec_recall(xr, xs)
    result = {"Inception Score": compute_inception_score(model, xs),
              "FID": sample_feats.statistics().frechet_distance(ref_feats.statistics()),
              "Precision": precision, "Recall": recall}
    if csv_path is not None:
        classify.update_result_csv(csv_path, name if name is not None else default_name(ref), result)
    return result


def _checked_model(model, checkpoint):
    model = model if model is not None else fid.load_model(checkpoint)
    if getattr(model, "fc_weight", None) is None:
        raise _lib.SfronError("the Inception Score needs the 1008-way head: the checkpoint's state dict has no fc.weight")
    return model


def evaluate_npz(ref, sample, checkpoint=None, model=None, batch_size=64, csv_path=None, name=None):
    """DDPM/evaluator.py:main over two ``.npz`` files whose ``arr_0`` holds NHWC bytes (sFID is not built)."""
    model = _checked_model(model, checkpoint)
    if csv_path is not None and name is None:
        default_name(ref)                                   # refuse before the network runs
    with np.load(ref) as z:
        if "arr_0" not in z.files:
            if "mu" in z.files and "sigma" in z.files:
                raise ValueError(f"{ref}: holds only mu / sigma; precision and recall need the reference set's features (an arr_0 of images)")
            raise KeyError(f"{ref}: no arr_0 (keys {z.files})")
    feats = [fid.InceptionFeatures(model, 2048, batch_size).add_npz(p) for p in (ref, sample)]
    return _evaluate(model, feats[0], feats[1], ref, csv_path, name)


def evaluate_folders(ref, sample, checkpoint=None, model=None, batch_size=64, csv_path=None, name=None, image_size=None):
    """The same over two image folders (files decoded to RGB; the reference's cv2 BGR order is not reproduced)."""
    model = _checked_model(model, checkpoint)
    if csv_path is not None and name is None:
        default_name(ref)
    feats = [fid.InceptionFeatures(model, 2048, batch_size).add_folder(p, image_size) for p in (ref, sample)]
    return _evaluate(model, feats[0], feats[1], ref, csv_path, name)
