"""tests/prec_recall_ref.py against tests/golden/evaluator.npz (the reference's own ManifoldEstimator and compute_inception_score), the
acceptance functions against the mistakes they must reject, and what sfron.evaluator can be asked without a GPU.

The lattice entries are exact: the fp32 restatement must equal the fixture bit for bit.  The Inception Score entries hold the reference's
float and the fp64 value of the same formula; the restatement reproduces both."""
import os
import re

import numpy as np
import pytest

import prec_recall_ref as ref
from sfron import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sfron_gemm_nt_f32", "sfron_manifold_radii", "sfron_manifold_radii_batched", "sfron_manifold_pr", "sfron_inception_score"]
SIZE_SYMBOLS = ["sfron_manifold_radii_workspace", "sfron_inception_score_workspace"]


def restated(e, **kw):
    return ref.evaluate(e["x1"], e["x2"], e["nhood"], np.float32, e["clamp"], **kw)


@pytest.mark.parametrize("name", ref.PR_ENTRIES)
def test_restatement_equals_the_fixture(name):
    e = ref.pr_entry(name)
    ref.accept_pr(e, restated(e))
    assert all(0 < v < 1 for v in list(e["precision"]) + list(e["recall"]))
    assert e["radii1"].shape == (len(e["x1"]), len(e["nhood"])) and e["in1"].shape == (len(e["x1"]), len(e["nhood"]))


def test_fixture_covers_the_parameters_the_issue_names():
    assert ref.pr_entry("a_k235")["nhood"] == (2, 3, 5)
    assert ref.pr_entry("a_clamp50")["clamp"] == 50 and (ref.pr_entry("a_clamp50")["radii1"] == 0).any()
    assert ref.pr_entry("c_chunk")["batches"] == (128, 96)
    for key in "ABCDE":
        assert int(ref.golden()[key + "/ties"]) >= 1
    assert os.path.getsize(ref.GOLDEN) < (1 << 20)


@pytest.mark.parametrize("name", ["a", "b", "c_chunk", "d", "e"])
def test_acceptance_rejects_the_named_mistakes(name):
    e = ref.pr_entry(name)
    with pytest.raises(AssertionError):
        ref.accept_pr(e, restated(e, strict=True))                    # < for <=
    with pytest.raises(AssertionError):
        ref.accept_pr(e, restated(e, skip_self=True))                 # the self-distance left out: k off by one
    good = restated(e)
    with pytest.raises(AssertionError):
        ref.accept_pr(e, dict(good, precision=good["recall"], recall=good["precision"]))
    with pytest.raises(AssertionError):                               # the two sets in the other order
        sw = ref.evaluate(e["x2"], e["x1"], e["nhood"], np.float32, e["clamp"])
        ref.accept_pr(e, dict(good, precision=sw["precision"], recall=sw["recall"]))


@pytest.mark.parametrize("name", ref.IS_ENTRIES)
def test_inception_score_restatement_and_rejections(name):
    e = ref.is_entry(name)
    assert np.abs(e["acts"] @ e["w"]).max() <= 20
    assert ref.inception_score(e["acts"], e["w"], e["split_size"], np.float32) == e["ref32"]
    assert ref.inception_score(e["acts"], e["w"], e["split_size"], np.float64) == e["ref64"]
    ref.accept_is(e, e["ref32"])
    ref.accept_is(e, e["ref64"])
    bias = np.random.default_rng(3).standard_normal(1008) * 0.05
    with pytest.raises(AssertionError):
        ref.accept_is(e, ref.inception_score(e["acts"], e["w"], e["split_size"], np.float64, bias=bias))
    if len(e["acts"]) > e["split_size"]:
        with pytest.raises(AssertionError):
            ref.accept_is(e, ref.inception_score(e["acts"], e["w"], e["split_size"], np.float64, whole_mean=True))
    else:
        assert name == "is37"


@pytest.mark.parametrize("case", ref.FLOAT_CASES)
def test_float_cases_fp32_restatement_stays_within_the_flag_cap(case):
    name, N1, N2, D, seed = case
    c = ref.float_case(N1, N2, D, seed)
    share = ref.accept_flags(c, c["ref32"]["in1"], c["ref32"]["in2"])
    p, r = c["ref64"]["precision"][0], c["ref64"]["recall"][0]
    print(f"{name}: P / R {p:.3f} / {r:.3f}, eps {c['eps']:.3e}, share of flags left out {share:.5f}")
    assert 0 < p < 1 and 0 < r < 1


def test_symbols_in_header_prototypes_and_library():
    assert _lib.ABI_VERSION == 17
    with open(os.path.join(ROOT, "unified-unlearning-w-remain-geometry_amd", "csrc", "api.hip")) as f:
        assert "sfron_abi_version(void) { return 17; }" in f.read()
    with open(os.path.join(ROOT, "include", "sfron.h")) as f:
        header = f.read()
    lib = _lib.lib()
    assert lib.sfron_abi_version() == 17
    for name, ret in [(n, "int") for n in NEW_SYMBOLS] + [(n, "int64_t") for n in SIZE_SYMBOLS]:
        m = re.search(r"\b" + ret + " " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/sfron.h"
        assert name in _lib._PROTOS, name
        assert len(_lib._PROTOS[name][1]) == m.group(1).count(",") + 1, name
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    # the size functions run on the host
    assert lib.sfron_manifold_radii_workspace(300, 0, 0) > 0
    assert lib.sfron_manifold_radii_workspace(300, 128, 96) >= lib.sfron_manifold_radii_workspace(128, 128, 128)
    assert lib.sfron_inception_score_workspace(1203, 1008, 500) >= 1008 * 8


def test_module_refusals_without_a_gpu(tmp_path):
    import torch
    from sfron import evaluator
    with pytest.raises(ValueError, match="checkpoint"):
        evaluator.evaluate_npz("a.npz", "b.npz")
    with pytest.raises(ValueError, match="checkpoint"):
        evaluator.evaluate_folders(str(tmp_path), str(tmp_path))

    class Headless:
        fc_weight = None

    class Headed:
        fc_weight = object()

    with pytest.raises(_lib.SfronError, match="fc.weight"):
        evaluator.evaluate_npz("a.npz", "b.npz", model=Headless())
    with pytest.raises(_lib.SfronError, match="fc.weight"):
        evaluator.evaluate_folders(str(tmp_path), str(tmp_path), model=Headless())
    stats = str(tmp_path / "stats.npz")
    np.savez(stats, mu=np.zeros(2048), sigma=np.eye(2048, dtype=np.float32))
    with pytest.raises(ValueError, match="mu / sigma"):
        evaluator.evaluate_npz(stats, "b.npz", model=Headed())
    est = evaluator.ManifoldEstimator()
    assert (est.row_batch_size, est.col_batch_size, est.nhood_sizes, est.clamp_to_percentile, est.eps) == (10000, 10000, (3,), None, 1e-5)
    with pytest.raises(NotImplementedError, match="ManifoldEstimator.evaluate"):
        est.evaluate(None, None, None)
    with pytest.raises(_lib.SfronError, match="no CPU fallback"):
        est.manifold_radii(torch.zeros(8, 8))
    with pytest.raises(_lib.SfronError, match="no CPU fallback"):
        est.evaluate_pr(torch.zeros(8, 8), torch.zeros(8, 1), torch.zeros(8, 8), torch.zeros(8, 1))
    for bad in ((), (0,), (8,), (1, 2, 3, 4, 5)):
        with pytest.raises(ValueError, match="nhood_sizes"):
            evaluator.ManifoldEstimator(nhood_sizes=bad)
    assert evaluator.default_name("results/cifar10/forget/ref/images.npz") == "forget/ref"
