"""Writes tests/golden/fid.npz from the reference's own DDPM/evaluator.py:

    python tests/golden/make_fid_golden.py --reference <checkout of the reference project>

The reference module imports tensorflow, cv2, pandas and requests, which this project's environment does not have; stub modules stand in
for them (and for tqdm) while it is imported.  Only ``FIDStatistics`` is used, with the statistics the reference's ``compute_statistics``
forms: ``np.mean(activations, axis=0)`` and ``np.cov(activations, rowvar=False)``.  Recorded per case <name> at D = 64 and 192:

  a<D>, b<D>                  the two seeded activation sets, fp32 [D + 8][D], shared by the cases
  <name><D>/mu_a, mu_b        the means (fp64);  <name><D>/sigma_a, sigma_b the covariances (fp64) -- in full at D = 64, at D = 192 only
                              shifted192/sigma_b (a committed file stays under 1 MiB)
  <name><D>/fid               ``FIDStatistics(a).frechet_distance(FIDStatistics(b))``
  <name><D>/eps_branch        whether the reference warned "singular product" and took its eps retry

Cases: ``equal`` (b is a), ``shifted`` (b = 1.3 a' + 0.5 of another draw) and ``deficient`` (the first D / 2 rows of each: n < D, both
covariances singular).  With scipy 1.15 the Schur method behind sqrtm returns a finite (complex) root for the deficient pair, so the
reference does NOT retry there (eps_branch is recorded False).  ``nilpotent64`` is therefore added: statistics given directly, sigma_a =
the single entry [0][1] = 1, sigma_b = I, whose product has no square root -- sqrtm returns NaN and the reference retries with eps on the
diagonals (eps_branch True).
"""
import argparse
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

SEED = 20251204


def load_evaluator(reference):
    path = os.path.join(reference, "DDPM", "evaluator.py")
    saved = {}
    names = ["cv2", "pandas", "requests", "tensorflow", "tensorflow.compat", "tensorflow.compat.v1", "tqdm", "tqdm.auto"]
    for n in names:
        saved[n] = sys.modules.get(n)
        sys.modules[n] = types.ModuleType(n)
    sys.modules["tensorflow"].compat = sys.modules["tensorflow.compat"]
    sys.modules["tensorflow.compat"].v1 = sys.modules["tensorflow.compat.v1"]
    sys.modules["tqdm.auto"].tqdm = lambda x, **k: x
    env = {k: os.environ.get(k) for k in ("PATH", "LD_LIBRARY_PATH")}
    try:
        spec = importlib.util.spec_from_file_location("reference_evaluator", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in env.items():                     # the module edits PATH / LD_LIBRARY_PATH at import
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        for n in names:
            if saved[n] is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = saved[n]
    return mod


def cases(D, rng):
    a = rng.standard_normal((D + 8, D)).astype(np.float32) * rng.uniform(0.5, 2.0, D).astype(np.float32)
    yield "equal", a, a.copy()
    b = (1.3 * rng.standard_normal((D + 8, D)) * rng.uniform(0.5, 2.0, D) + 0.5).astype(np.float32)
    yield "shifted", a, b
    yield "deficient", a[:D // 2].copy(), b[:D // 2].copy()


def record(ev, out, key, sa, sb, sigmas):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        fid = sa.frechet_distance(sb)
    out[key + "/mu_a"], out[key + "/mu_b"] = sa.mu, sb.mu
    for which, st in (("a", sa), ("b", sb)):
        if which in sigmas:
            out[f"{key}/sigma_{which}"] = st.sigma
    out[key + "/fid"] = np.float64(fid)
    out[key + "/eps_branch"] = np.bool_(any("singular product" in str(x.message) for x in w))
    print(key, "fid", fid, "eps branch", bool(out[key + "/eps_branch"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "fid.npz"))
    args = ap.parse_args()
    ev = load_evaluator(args.reference)
    out = {}
    for D in (64, 192):
        rng = np.random.default_rng(SEED + D)
        for name, a, b in cases(D, rng):
            sa = ev.FIDStatistics(np.mean(a, axis=0), np.cov(a, rowvar=False))
            sb = ev.FIDStatistics(np.mean(b, axis=0), np.cov(b, rowvar=False))
            key = f"{name}{D}"
            if name == "shifted":
                out[f"a{D}"], out[f"b{D}"] = a, b
            record(ev, out, key, sa, sb, sigmas=("a", "b") if D == 64 else (("b",) if name == "shifted" else ()))
    rng = np.random.default_rng(SEED)
    s1 = np.zeros((64, 64))
    s1[0, 1] = 1.0
    record(ev, out, "nilpotent64", ev.FIDStatistics(rng.standard_normal(64), s1), ev.FIDStatistics(rng.standard_normal(64), np.eye(64)),
           sigmas=("a", "b"))
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
