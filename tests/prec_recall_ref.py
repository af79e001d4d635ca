"""Reference for sfron.evaluator and csrc/manifold.hip: numpy restatements of DDPM/evaluator.py's ManifoldEstimator / DistanceBlock (its
fp32 branch) and compute_inception_score, and the acceptance functions the CPU and GPU tests share.  Every function takes ``dtype``:
float64 is the reference, float32 -- the same code -- is the yardstick.  Nothing here calls a kernel.

The fixture tests/golden/evaluator.npz (tests/golden/make_evaluator_golden.py) holds what the reference's OWN classes return on integer
lattices: every dot product and norm is an integer below 2^24 there, so every distance is exact in fp32 in any summation order and the
acceptance is bit equality (``accept_pr``).  ``accept_is`` holds a score under ``bound32`` of tests/dit_rows_ref.py with the fixture's
fp64 value as the reference and the reference implementation's own float as the yardstick.

Variants (``strict``, ``skip_self``, ``bias``, ``whole_mean``) restate the mistakes the acceptance must reject: ``<`` for ``<=``, the
self-distance left out of the neighbour count, fc.bias added to the logits, the split's column mean taken over the whole set."""
import os

import numpy as np
import torch

from dit_rows_ref import bound32

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evaluator.npz")
PR_ENTRIES = ("a", "a_k235", "a_clamp50", "b", "c_chunk", "d", "e")
IS_ENTRIES = ("is37", "is1203")
# float-feature cases: (name, N1, N2, D, seed)
FLOAT_CASES = (("f64", 300, 260, 64, 1), ("f2048", 257, 129, 2048, 2))
FLAG_CAP = 0.01


# ------------------------------------------------------------------------------------------------ the expressions
def pairwise(U, V, dtype):
    """_batch_pairwise_distances: max(norm_u - 2 U V^T + norm_v, 0), every step in ``dtype``."""
    U, V = np.asarray(U, dtype=dtype), np.asarray(V, dtype=dtype)
    norm_u = np.sum(np.square(U), 1).reshape(-1, 1)
    norm_v = np.sum(np.square(V), 1).reshape(1, -1)
    return np.maximum(norm_u - dtype(2) * (U @ V.T) + norm_v, dtype(0))


def manifold_radii(X, nhood, dtype, clamp=None, skip_self=False):
    d = pairwise(X, X, dtype)
    kmax = max(nhood)
    if skip_self:
        d = d + np.diag(np.full(len(d), np.inf, dtype=dtype))
        part = np.sort(d, axis=1)
        radii = part[:, list(nhood)]                     # index k of a row WITHOUT the self-distance: the (k + 1)-th neighbour
    else:
        part = np.partition(d, np.arange(kmax + 1), axis=1)
        radii = part[:, list(nhood)]
    radii = np.ascontiguousarray(radii)
    if clamp is not None:
        radii[radii > np.percentile(radii, clamp, axis=0)] = 0
    return radii


def status(X1, r1, X2, r2, dtype, strict=False):
    """(features_1_status [N1][K2], features_2_status [N2][K1]) of evaluate_pr."""
    d = pairwise(X1, X2, dtype)[..., None]
    r1, r2 = np.asarray(r1, dtype=dtype), np.asarray(r2, dtype=dtype)
    if strict:
        return np.any(d < r2[None], axis=1), np.any(d < r1[:, None], axis=0)
    return np.any(d <= r2[None], axis=1), np.any(d <= r1[:, None], axis=0)


def prec_recall(in1, in2):
    return np.mean(in2.astype(np.float64), axis=0), np.mean(in1.astype(np.float64), axis=0)


def evaluate(X1, X2, nhood, dtype, clamp=None, strict=False, skip_self=False):
    """-> dict(radii1, radii2, in1, in2, precision, recall)"""
    r1 = manifold_radii(X1, nhood, dtype, clamp, skip_self)
    r2 = manifold_radii(X2, nhood, dtype, clamp, skip_self)
    in1, in2 = status(X1, r1, X2, r2, dtype, strict)
    p, r = prec_recall(in1, in2)
    return dict(radii1=r1, radii2=r2, in1=in1, in2=in2, precision=p, recall=r)


def softmax_rows(z):
    e = np.exp(z - np.max(z, axis=1, keepdims=True))
    return e / np.sum(e, axis=1, keepdims=True)


def split_scores(preds, split_size, whole_mean=False):
    """compute_inception_score's loop over softmax outputs, in the dtype of ``preds``."""
    scores = []
    for i in range(0, len(preds), split_size):
        part = preds[i:i + split_size]
        mean = np.mean(preds if whole_mean else part, 0)
        kl = part * (np.log(part) - np.log(np.expand_dims(mean, 0)))
        scores.append(np.exp(np.mean(np.sum(kl, 1))))
    return np.asarray(scores)


def inception_score(acts, w, split_size, dtype, bias=None, whole_mean=False):
    """acts [N][2048], w [2048][1008] (the head's matrix as the reference multiplies it: no bias) -> the mean of the split scores."""
    z = np.asarray(acts, dtype=dtype) @ np.asarray(w, dtype=dtype)
    if bias is not None:
        z = z + np.asarray(bias, dtype=dtype)
    return float(np.mean(split_scores(softmax_rows(z), split_size, whole_mean)))


# ------------------------------------------------------------------------------------------------ inputs
_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def pr_entry(name):
    """-> dict(x1, x2 fp32; nhood tuple; clamp float or None; batches (row, col); radii1, radii2, in1, in2, precision, recall)."""
    g = golden()
    src = str(g[name + "/inputs"])
    clamp = float(g[name + "/clamp"])
    return dict(x1=g[src + "/x1"].astype(np.float32), x2=g[src + "/x2"].astype(np.float32), nhood=tuple(int(k) for k in g[name + "/nhood"]),
                clamp=None if clamp < 0 else clamp, batches=tuple(int(b) for b in g[name + "/batches"]),
                **{k: g[f"{name}/{k}"] for k in ("radii1", "radii2", "in1", "in2", "precision", "recall")})


def is_entry(name):
    """-> dict(acts fp32 [N][2048], w fp32 [2048][1008], split_size, ref32, ref64)."""
    g = golden()
    n = int(g[name + "/n"])
    w = (np.tile(g["is/w_block"].astype(np.float32), (2048 // g["is/w_block"].shape[0], 1)) * np.float32(g["is/scale"])).astype(np.float32)
    return dict(acts=g["is/acts"][:n].astype(np.float32), w=w, split_size=int(g[name + "/split_size"]), ref32=float(g[name + "/ref32"]),
                ref64=float(g[name + "/ref64"]))


def lattice(n, D, lo, hi, p, rng, centres=None):
    """The fixture's recipe: rows are copies of six random integer centres with each coordinate redrawn with probability p."""
    if centres is None:
        centres = rng.integers(lo, hi + 1, (6, D))
    x = centres[rng.integers(0, 6, n)].copy()
    redraw = rng.random((n, D)) < p
    x[redraw] = rng.integers(lo, hi + 1, (n, D))[redraw]
    return x.astype(np.float32), centres


def float_features(N1, N2, D, seed):
    """A 4-dimensional Gaussian pushed through a random 4 x D map plus 0.02 noise, offset 0.5; the sample set 1.15 x wider."""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((4, D)) / 2.0
    x1 = rng.standard_normal((N1, 4)) @ m + 0.02 * rng.standard_normal((N1, D)) + 0.5
    x2 = 1.15 * (rng.standard_normal((N2, 4)) @ m) + 0.02 * rng.standard_normal((N2, D)) + 0.5
    return x1.astype(np.float32), x2.astype(np.float32)


def float_case(N1, N2, D, seed, nhood=(3,)):
    """-> x1, x2, the fp64 restatement, the fp32 restatement (the same numpy code), the fp32 restatement's largest
    distance error ``eps`` (over the cross distances and both sets' own) and the mask of DECIDED flags: a flag is decided when its
    decisive margin -- the closest any of its pairs comes to its radius, min |d - r| in fp64 -- exceeds eps."""
    x1, x2 = float_features(N1, N2, D, seed)
    r64, r32 = evaluate(x1, x2, nhood, np.float64), evaluate(x1, x2, nhood, np.float32)
    d64, d32 = pairwise(x1, x2, np.float64), pairwise(x1, x2, np.float32)
    eps = float(np.max(np.abs(d32.astype(np.float64) - d64)))
    for X in (x1, x2):
        eps = max(eps, float(np.max(np.abs(pairwise(X, X, np.float32).astype(np.float64) - pairwise(X, X, np.float64)))))
    m1 = np.min(np.abs(d64[..., None] - r64["radii2"][None]), axis=1)          # [N1][K2]: the closest any pair comes to its radius
    m2 = np.min(np.abs(d64[..., None] - r64["radii1"][:, None]), axis=0)       # [N2][K1]
    return dict(x1=x1, x2=x2, ref64=r64, ref32=r32, eps=eps, decided1=m1 > eps, decided2=m2 > eps)


# ------------------------------------------------------------------------------------------------ acceptance
def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def accept_pr(entry, got):
    """``got`` dict(radii1, radii2, in1, in2, precision, recall) must equal the fixture entry bit for bit."""
    for k in ("radii1", "radii2"):
        a, b = _np(got[k]).astype(np.float32), entry[k].astype(np.float32)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), f"{k}: {int((a != b).sum())} of {a.size} radii differ"
    for k in ("in1", "in2"):
        a, b = _np(got[k]).astype(bool), entry[k].astype(bool)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert np.array_equal(a, b), f"{k}: {int((a != b).sum())} of {a.size} flags differ"
    for k in ("precision", "recall"):
        a, b = np.asarray(got[k], dtype=np.float64), np.asarray(entry[k], dtype=np.float64)
        assert a.shape == b.shape and np.array_equal(a, b), f"{k}: {a} != {b}"


def accept_is(entry, got, name=None):
    """the mean split score under bound32: reference = the fixture's fp64 value, yardstick = the reference implementation's float."""
    t = lambda v: torch.tensor([float(v)], dtype=torch.float64)
    return bound32(t(got), t(entry["ref64"]), t(entry["ref32"]), name=name)


def accept_flags(case, in1, in2):
    """decided flags equal the fp64 decision; -> the share of flags left out (asserted under FLAG_CAP)."""
    in1, in2 = _np(in1).astype(bool), _np(in2).astype(bool)
    left = 0
    for got, want, dec in ((in1, case["ref64"]["in1"], case["decided1"]), (in2, case["ref64"]["in2"], case["decided2"])):
        assert got.shape == want.shape, (got.shape, want.shape)
        bad = (got != want) & dec
        assert not bad.any(), f"{int(bad.sum())} decided flags differ from the fp64 decision"
        left += int((~dec).sum())
    share = left / (in1.size + in2.size)
    assert share <= FLAG_CAP, f"{share:.4f} of the flags are under the margin (cap {FLAG_CAP})"
    return share
