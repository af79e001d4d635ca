"""sfron.fid.FIDStatistics against the reference's own (DDPM/evaluator.py:108-156), recorded in tests/golden/fid.npz by
tests/golden/make_fid_golden.py: equal, shifted and rank-deficient (n < D) seeded activation pairs at D = 64 and 192, and a crafted pair
whose covariance product has no square root, which takes the eps retry.

Tolerance.  The distance is invariant under one permutation applied to the feature axis of both sets (sigma -> P^T sigma P), but
scipy.linalg.sqrtm's Schur form is not: over permuted inputs it returns traces that differ by its own rounding error.  ``spread`` measures
that on this CPU: the largest |FID(permuted) - FID(unpermuted)| over 8 seeded permutations.  The recorded value (another machine's BLAS
and LAPACK) and the one computed here are two such draws, so they may differ by twice the spread; to that the bound adds the four roundings
of the final expression |dmu|^2 + tr s1 + tr s2 - 2 tr covmean, at the size of its largest partial sum: 4 ulp(|dmu|^2 + tr s1 + tr s2).
Nothing else enters: mean, covariance and the traces are the same numpy calls on the same bytes."""
import os
import warnings

import numpy as np
import pytest

from sfron import fid

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [f"{n}{D}" for D in (64, 192) for n in ("equal", "shifted", "deficient")]


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(HERE, "golden", "fid.npz")) as z:
        return {k: z[k] for k in z.files}


def sets(golden, case):
    D = int(case[-3:]) if case.endswith("192") else 64
    a, b = golden[f"a{D}"], golden[f"b{D}"]
    if case.startswith("equal"):
        return a, a
    if case.startswith("deficient"):
        return a[:D // 2], b[:D // 2]
    return a, b


def stats(x):
    return fid.FIDStatistics(np.mean(x, axis=0), np.cov(x, rowvar=False))


def distance(sa, sb, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return sa.frechet_distance(sb, **kw)


def bound(sa, sb, base):
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(8):
        p = rng.permutation(sa.mu.shape[0])
        pa, pb = (fid.FIDStatistics(s.mu[p], s.sigma[p][:, p]) for s in (sa, sb))
        worst = max(worst, abs(distance(pa, pb) - base))
    d = sa.mu - sb.mu
    return 2 * worst + 4 * np.spacing(d.dot(d) + np.trace(sa.sigma) + np.trace(sb.sigma))


@pytest.mark.parametrize("case", CASES)
def test_frechet_distance_matches_reference(golden, case):
    a, b = sets(golden, case)
    sa, sb = stats(a), stats(b)
    np.testing.assert_array_equal(sa.mu, golden[case + "/mu_a"])          # np.mean over axis 0: pairwise sums, no BLAS
    np.testing.assert_array_equal(sb.mu, golden[case + "/mu_b"])
    for which, st in (("a", sa), ("b", sb)):
        key = f"{case}/sigma_{which}"
        if key in golden:                    # np.cov goes through BLAS: one rounding per term of an n-term dot product of O(sigma) terms
            scale = np.sqrt(np.outer(np.diag(golden[key]), np.diag(golden[key])))
            assert np.all(np.abs(st.sigma - golden[key]) <= a.shape[0] * 2.0 ** -52 * scale)
    assert not bool(golden[case + "/eps_branch"])
    got = distance(sa, sb)
    tol = bound(sa, sb, got)
    want = float(golden[case + "/fid"])
    print(f"{case}: reference {want!r}, here {got!r}, |diff| {abs(got - want):.3e}, bound {tol:.3e}")
    assert abs(got - want) <= tol


def test_rank_deficient_sets_are_rank_deficient(golden):
    for D in (64, 192):
        a, _ = sets(golden, f"deficient{D}")
        assert a.shape[0] < D and np.linalg.matrix_rank(np.cov(a, rowvar=False)) < a.shape[0]


def test_eps_branch(golden):
    """sigma_a sigma_b is nilpotent: sqrtm fails with NaN, the reference warns and retries with eps on both diagonals (eps_branch recorded
    True).  The same bound as above, measured on the retry."""
    key = "nilpotent64"
    assert bool(golden[key + "/eps_branch"])
    sa = fid.FIDStatistics(golden[key + "/mu_a"], golden[key + "/sigma_a"])
    sb = fid.FIDStatistics(golden[key + "/mu_b"], golden[key + "/sigma_b"])
    with pytest.warns(UserWarning, match="singular product"):
        got = sa.frechet_distance(sb)
    want = float(golden[key + "/fid"])
    assert abs(got - want) <= bound(sa, sb, got)
    with pytest.warns(UserWarning, match="singular product"):
        other = sa.frechet_distance(sb, eps=1e-3)
    assert other != got                       # eps is used


def test_imaginary_component_is_refused():
    s = np.array([[-4.0, 0.0], [0.0, 1.0]])
    with pytest.raises(ValueError, match="Imaginary component"):
        fid.FIDStatistics(np.zeros(2), s).frechet_distance(fid.FIDStatistics(np.zeros(2), np.eye(2)))


def test_save_load_roundtrip(golden, tmp_path):
    st = stats(golden["b64"])
    p = str(tmp_path / "stats.npz")
    st.save(p)
    back = fid.FIDStatistics.load(p)
    np.testing.assert_array_equal(back.mu, st.mu)
    np.testing.assert_array_equal(back.sigma, st.sigma)
    with np.load(p) as z:
        assert sorted(z.files) == ["mu", "sigma"]
    np.savez(str(tmp_path / "bad.npz"), arr_0=np.zeros((1, 2, 2, 3), np.uint8))
    with pytest.raises(KeyError):
        fid.FIDStatistics.load(str(tmp_path / "bad.npz"))


def test_drivers_refuse_without_checkpoint_or_with_a_bad_feature(tmp_path):
    with pytest.raises(ValueError, match="checkpoint"):
        fid.fid_folders(str(tmp_path), str(tmp_path), feature=64)
    with pytest.raises(ValueError, match="checkpoint"):
        fid.fid_npz("a.npz", "b.npz", feature=64)
    with pytest.raises(ValueError, match="feature"):
        fid.fid_folders(str(tmp_path), str(tmp_path), feature=100, checkpoint="x.pt")
    with pytest.raises(ValueError, match="feature"):
        fid.fid_npz("a.npz", "b.npz", feature=2047, checkpoint="x.pt")
