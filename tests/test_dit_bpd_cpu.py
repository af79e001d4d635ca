"""CPU: the host side of the DiT likelihood evaluation (csrc/dit_bpd.hip, sfron.diffusion.GaussianDiffusion._vb_terms_bpd / _prior_bpd /
calc_bpd_loop, sfron.dit_bpd).

The tests' float64 restatement (tests/dit_bpd_ref.py) against the reference's own fp32 outputs (tests/golden/dit_bpd.npz, made by
tests/golden/make_dit_bpd_golden.py) at the observed fp32-vs-fp64 distance; the ABI surface of the two new entry points and their refusals
(SFRON_ERR_ARG before any launch: no GPU is touched); the shape of calc_bpd_loop's result on the restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dit_bpd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sfron_dit_bpd_step", "sfron_dit_prior_bpd")
KEYS = ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")
LOOP_SEED = 77
# The fixture is fp32 arithmetic, the restatement float64 on the same fp32 inputs.  Observed over every entry (printed with -s): the
# terms lie within 0.21 of |d| <= 2e-7 + 1e-5 |want| (the worst is a T = 1000 vb column; terms near zero, a KL of 1e-6 bits at t = 999
# under the clamp, differ by percents of themselves and need the absolute part), so that bound is asserted: a margin of five over what
# fp32 in the reference's order gives.  pred_xstart has a derived bound instead (pred_err): observed 0.94 of it.
TERM_RTOL, TERM_ATOL = 1e-5, 2e-7


@pytest.fixture(scope="module")
def G(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "dit_bpd.npz")))


@pytest.fixture(scope="module")
def S(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "dit_sampling.npz")))


def _dist(name, got, want, rtol, atol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())
    print(f"DIT-BPD-METRIC cpu {name} max_rel={float((np.abs(got - want) / np.maximum(np.abs(want), 1e-30)).max()):.3e} err/bound={err:.3f}")
    return err


def pred_err(name, got, r):
    """pred_xstart = a - b is two fp32 products and one difference, each rounded to nearest: |error| <= 2^-24 (|a| + |b| + |a - b|) <=
    2^-23 (|a| + |b|) against the exact value (the clamp only shrinks an error).  In units of that bound."""
    err = float((np.abs(np.asarray(got, dtype=np.float64) - r["pred_xstart"]) / (2.0 ** -23 * r["pred_mag"])).max())
    print(f"DIT-BPD-METRIC cpu {name} err/bound={err:.3f}")
    return err


def loop_noise(x0, T):
    """The stream the reference's calc_bpd_loop consumed: one randn_like(x_start) per step from the seeded global CPU generator."""
    g = torch.Generator().manual_seed(LOOP_SEED)
    x0 = torch.as_tensor(x0)
    return [torch.randn(x0.shape, generator=g) for _ in range(T)]


# ------------------------------------------------------------------------------------------------ restatement against the fixture
def test_seeded_generator_draws_are_the_global_stream():
    torch.manual_seed(LOOP_SEED)
    x = torch.zeros(2, 4, 4, 4)
    want = [torch.randn_like(x) for _ in range(3)]
    assert all(torch.equal(a, b) for a, b in zip(loop_noise(x, 3), want))


@pytest.mark.parametrize("name", ["stub", "stub2"])
@pytest.mark.parametrize("clip", [0, 1])
def test_restated_single_terms_are_within_fp32_distance_of_the_reference(G, name, clip):
    from sfron import diffusion
    d = diffusion.create_diffusion("", device="cpu")
    r = R.vb_terms(d.tab.numpy(), G["one_x0"], G["one_t"], G[f"one/{name}/model_out"], clip, x_t=G["one_xt"], detail=True)
    errs = [_dist(f"one/{name}/clip{clip}/output", r["output"], G[f"one/{name}/clip{clip}/output"], TERM_RTOL, TERM_ATOL),
            pred_err(f"one/{name}/clip{clip}/pred_xstart", G[f"one/{name}/clip{clip}/pred_xstart"], r)]
    assert max(errs) <= 1.0, errs
    # the fixture's inputs: all three likelihood branches in the extreme row, nothing fragile at t == 0
    x4 = G["one_x0"][4]
    assert (x4 < -0.999).any() and (x4 > 0.999).any() and (np.abs(x4) <= 0.999).any()
    assert R.fragile_count(r, G["one_x0"]) == (0, 0)
    if clip:
        assert np.abs(r["pred_xstart"]).max() <= 1.0 and (np.abs(r["pred_xstart"]) == 1.0).any()


def test_restated_prior_is_within_fp32_distance_of_the_reference(G):
    from sfron import diffusion
    errs = [_dist("prior_full", R.prior_bpd(diffusion.create_diffusion("", device="cpu").tables, G["one_x0"]), G["prior_full"], TERM_RTOL, TERM_ATOL),
            _dist("prior_10", R.prior_bpd(diffusion.create_diffusion("10", device="cpu").tables, G["x0_10"]), G["prior_10"], TERM_RTOL, TERM_ATOL)]
    assert max(errs) <= 1.0, errs


@pytest.fixture(scope="module")
def restated_loops(G, S):
    """The float64 restatement of every fixture loop, computed once: {(tag, stub, clip): dict}."""
    from sfron import diffusion
    named = dict(zip(("stub", "stub2"), R.stubs(S["A"], S["abar1000"], S["z"].shape[1], torch.float64)))
    res = {}
    for tag, spec, names in (("loop10", "10", ("stub", "stub2")), ("loopfull", "", ("stub2",))):
        d = diffusion.create_diffusion(spec, device="cpu")
        x0 = G["x0_" + tag[4:]]
        noise = [z.numpy() for z in loop_noise(x0, d.num_timesteps)]
        for name in names:
            for clip in (0, 1):
                res[tag, name, clip] = R.calc_bpd_loop(d, named[name], x0, noise, clip)
    return res


def test_restated_loops_are_within_fp32_distance_of_the_reference(G, restated_loops):
    errs = [_dist(f"{tag}/{name}/clip{clip}/{k}", r[k], G[f"{tag}/{name}/clip{clip}/{k}"], TERM_RTOL, TERM_ATOL)
            for (tag, name, clip), r in restated_loops.items() for k in KEYS]
    assert len(errs) == 6 * len(KEYS) and max(errs) <= 1.0, max(errs)


def test_loop_result_columns_stacking_order_and_total(G, S, restated_loops):
    from sfron import diffusion
    for (tag, name, clip), r in restated_loops.items():
        spec = "10" if tag == "loop10" else ""
        d = diffusion.create_diffusion(spec, device="cpu")
        x0 = G["x0_" + tag[4:]]
        n, T = x0.shape[0], d.num_timesteps
        assert r["vb"].shape == r["xstart_mse"].shape == r["mse"].shape == (n, T) and r["total_bpd"].shape == r["prior_bpd"].shape == (n,)
        assert np.array_equal(r["total_bpd"], r["vb"].sum(1) + r["prior_bpd"])
        for k in KEYS:
            assert G[f"{tag}/{name}/clip{clip}/{k}"].shape == r[k].shape
        if tag != "loop10":
            continue
        # column k is t = T - 1 - k: recompute two columns on their own
        noise = [z.numpy() for z in loop_noise(x0, T)]
        fn = dict(zip(("stub", "stub2"), R.stubs(S["A"], S["abar1000"], S["z"].shape[1], torch.float64)))[name]
        tab = d.tab.numpy().astype(np.float64)
        for k in (0, T - 1):
            i = T - 1 - k
            x_t = tab[i, 0] * x0.astype(np.float64) + tab[i, 1] * noise[k]
            out = fn(torch.from_numpy(x_t), torch.full((n,), d.timestep_map[i])).numpy()
            one = R.vb_terms(d.tab.numpy(), x0, np.full(n, i), out, clip, x_t=x_t, noise=noise[k])
            assert np.array_equal(one["output"], r["vb"][:, k]) and np.array_equal(one["mse"], r["mse"][:, k])
        # the last column is the decoder NLL (t == 0), not a KL: with the same inputs read as t = 1 it differs
        assert not np.allclose(r["vb"][:, T - 1], r["vb"][:, T - 2])


# ------------------------------------------------------------------------------------------------ ABI
def test_new_prototypes_in_header_and_binding_and_abi_stays_16():
    from sfron import _lib
    L = _lib.lib()
    assert L.sfron_abi_version() == 17 and _lib.ABI_VERSION == 17          # additive: the ABI version stays
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfron.h")).read(), flags=re.S)
    kinds = {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double, "int": ctypes.c_int}
    for name in NEW:
        assert getattr(L, name) is not None and name in _lib.declared_symbols()
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, f"{name} is not declared in include/sfron.h"
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib._PROTOS[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for at, p in zip(args, params):
            assert at is (ctypes.c_void_p if "*" in p else kinds[p.split()[0]]), (name, p, at)
    src = open(os.path.join(ROOT, "unified-unlearning-w-remain-geometry_amd", "csrc", "dit_bpd.hip")).read()
    assert "atomicAdd" not in src                                           # fixed-order reductions only


def test_the_three_methods_and_the_evaluator_exist_with_the_reference_signatures():
    import inspect
    from sfron import diffusion, dit_bpd
    D = diffusion.GaussianDiffusion
    assert list(inspect.signature(D._vb_terms_bpd).parameters) == ["self", "model", "x_start", "x_t", "t", "clip_denoised", "model_kwargs"]
    assert list(inspect.signature(D._prior_bpd).parameters) == ["self", "x_start"]
    assert list(inspect.signature(D.calc_bpd_loop).parameters) == ["self", "model", "x_start", "clip_denoised", "model_kwargs", "generator",
                                                                   "step_noise"]
    assert inspect.signature(D.calc_bpd_loop).parameters["clip_denoised"].default is True
    assert inspect.signature(D._vb_terms_bpd).parameters["clip_denoised"].default is True
    assert list(inspect.signature(dit_bpd.DiTBpdEvaluator.__init__).parameters) == ["self", "model", "diffusion", "clip_denoised"]
    assert list(inspect.signature(dit_bpd.DiTBpdEvaluator.evaluate).parameters) == ["self", "x_start", "y", "generator", "step_noise"]
    p = inspect.signature(dit_bpd.evaluate_bpd).parameters
    assert list(p) == ["model", "cache", "forget_class", "timestep_respacing", "batch", "max_per_class", "generator", "scale"]
    assert (p["timestep_respacing"].default, p["batch"].default, p["max_per_class"].default, p["scale"].default) == ("", 32, None, 0.18215)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[3:])


# never dereferenced: every call below is refused before a launch.  Distinct 256-byte "buffers" inside one host allocation.
_HOST = (ctypes.c_char * 4096)()
_P = [ctypes.addressof(_HOST) + 256 * k for k in range(14)]
_STEP_KEYS = ("x0", "x_t", "noise", "model_out", "t", "tab", "T", "n", "c", "hw", "clip", "vb", "xs", "mse", "ld", "step", "col", "pred",
              "next_noise", "order", "steps", "next_xt")


def _step_args(**kw):
    a = dict(x0=_P[0], x_t=None, noise=_P[1], model_out=_P[2], t=_P[3], tab=_P[4], T=10, n=2, c=4, hw=8, clip=1, vb=_P[5], xs=_P[6], mse=_P[7],
             ld=10, step=_P[8], col=0, pred=None, next_noise=_P[9], order=_P[10], steps=10, next_xt=_P[11])
    a.update(kw)
    return [a[k] for k in _STEP_KEYS] + [None]


@pytest.mark.parametrize("bad", [
    dict(x0=None), dict(model_out=None), dict(t=None), dict(tab=None), dict(vb=None),                      # a null required pointer
    dict(noise=None, mse=None, next_xt=None), dict(noise=None, x_t=_P[12], next_xt=None),                  # neither x_t nor noise / mse without noise
    dict(T=0), dict(n=0), dict(c=0), dict(hw=-1), dict(ld=0),                                              # a non-positive extent
    dict(step=None, next_xt=None, col=-1), dict(step=None, next_xt=None, col=10),                          # a column outside the matrices
    dict(next_noise=None), dict(order=None), dict(step=None), dict(steps=0), dict(steps=11),               # the next step's operands
    dict(next_xt=_P[0]), dict(next_xt=_P[1]), dict(next_xt=_P[9]), dict(next_xt=_P[12], x_t=_P[12]), dict(next_xt=_P[13], pred=_P[13]),
    dict(pred=_P[0]), dict(pred=_P[1]), dict(pred=_P[12], x_t=_P[12]),                                     # pred_xstart aliases an input
    dict(n=1 << 12, c=1 << 10, hw=1 << 9), dict(n=1 << 20, c=1, hw=1, ld=1 << 11, steps=1),               # an int product
], ids=lambda b: ",".join(f"{k}={'P%d' % _P.index(v) if v in _P else v}" for k, v in b.items()))
def test_step_refusals_come_before_any_launch(bad):
    from sfron import _lib
    assert _lib.lib().sfron_dit_bpd_step(*_step_args(**bad)) == _lib.ERR_ARG


def test_prior_refusals_come_before_any_launch():
    from sfron import _lib
    L = _lib.lib()
    good = dict(x0=_P[0], n=2, c=4, hw=8, sa=0.006, lv=-4e-5, out=_P[1])
    for bad in (dict(x0=None), dict(out=None), dict(n=0), dict(c=-1), dict(hw=0), dict(n=1 << 12, c=1 << 10, hw=1 << 9),
                dict(sa=float("nan")), dict(lv=float("inf"))):
        a = dict(good, **bad)
        assert L.sfron_dit_prior_bpd(*[a[k] for k in good], None) == _lib.ERR_ARG, bad


def test_evaluator_refuses_a_model_without_learned_sigma():
    from sfron import dit_bpd

    class M:
        learn_sigma = False
    with pytest.raises(NotImplementedError):
        dit_bpd.DiTBpdEvaluator(M(), None)
