"""CPU: the host side of the ldm PLMS sampler (sfron.plms).

The fixture (tests/golden/plms.npz, made by tests/golden/make_plms_golden.py from SD/ldm/models/diffusion/plms.py) loads without the
reference; ABI surface of sfron_plms_cfg_step / sfron_inpaint_blend (header <-> ctypes); the schedule tables against the reference's; the
ValueError and every NotImplementedError guard; the history bookkeeping with the model and the update mocked (S + 1 model calls, the order
of every launch, a ring of three buffers, the first step keeping e_t and not e_t_next); the slices a chunked run hands on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_ddim_cpu import host_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("plain", "guided", "s1", "s3", "inpaint")


@pytest.fixture(scope="module")
def P(golden_dir):
    return np.load(os.path.join(golden_dir, "plms.npz"))


def test_fixture_loads_without_the_reference(P):
    for case, S in zip(CASES, (10, 10, 1, 3, 10)):
        pre = f"stub/{case}/"
        assert P[pre + "samples"].shape == (2, 4, 8, 8) and P[pre + "samples"].dtype == np.float32
        assert np.array_equal(P[pre + "samples"], P[pre + "x_inter"][-1])
        assert np.array_equal(P[pre + "x_inter"][0], P["stub/x_T"]) and len(P[pre + "x_inter"]) == len(P[pre + "pred_x0"])
    assert len(P["stub/guided/x_inter"]) == 1 + 4          # the start, then the indices with index % 3 == 0: 9 (also the first step), 6, 3, 0
    for case in ("guided", "inpaint"):
        pre = f"stub/{case}/"
        assert P[pre + "step_out"].shape == (11, 4, 4, 8, 8) and P[pre + "step_hist"].shape == (10, 3, 2, 4, 8, 8)
        assert P[pre + "step_hist_len"].tolist() == [0, 1, 2] + [3] * 7
        for name in ("step_x", "step_e_t", "step_x_prev", "step_pred_x0"):
            assert P[pre + name].shape == (10, 2, 4, 8, 8)
        # the history a step read is what the steps before it returned, newest first
        for k in range(1, 10):
            for j in range(min(k, 3)):
                assert np.array_equal(P[pre + "step_hist"][k, j], P[pre + "step_e_t"][k - 1 - j])
    m = P["stub/mask"]
    assert m.shape == (2, 1, 8, 8) and set(np.unique(m)) == {0.0, 1.0}
    assert P["unet/eps"].shape == (9, 2, 4, 8, 8) and P["unet/x_inter"].shape == (9, 2, 4, 8, 8)


def test_new_symbols_header_and_ctypes_agree():
    from sfron import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfron.h")).read(), flags=re.S)
    for name in ("sfron_plms_cfg_step", "sfron_inpaint_blend"):
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, f"{name} is not declared in include/sfron.h"
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib._PROTOS[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for at, p in zip(args, params):
            if "*" in p:
                assert at is ctypes.c_void_p, (name, p, at)
            else:
                assert at is {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}[p.split()[0]], (name, p, at)
    enum = dict(re.findall(r"SFRON_PLMS_(\w+)\s*=\s*(\d+)", hdr))
    assert {k: int(v) for k, v in enum.items()} == {"ORDER1": _lib.PLMS_ORDER1, "ORDER2": _lib.PLMS_ORDER2, "ORDER3": _lib.PLMS_ORDER3,
                                                    "ORDER4": _lib.PLMS_ORDER4, "MEAN": _lib.PLMS_MEAN}
    assert _lib.ABI_VERSION == 17          # additive: the ABI version stays


def test_schedule_tables_equal_the_reference(P):
    from sfron import plms
    names = sorted({k.split("/")[1] for k in P.files if k.startswith("sched/")})
    assert names == ["10_uniform", "12_quad", "1_uniform", "3_quad", "50_uniform", "8_uniform"]
    for name in names:
        S, discr = name.split("_")
        s = plms.PLMSSampler(host_model())
        s.make_schedule(int(S), ddim_discretize=discr, verbose=False)
        pre = f"sched/{name}/"
        assert s.ddim_timesteps.dtype == P[pre + "timesteps"].dtype and np.array_equal(s.ddim_timesteps, P[pre + "timesteps"])
        for key, got in (("alphas", s.ddim_alphas), ("alphas_prev", s.ddim_alphas_prev), ("sigmas", s.ddim_sigmas),
                         ("sqrt_one_minus_alphas", s.ddim_sqrt_one_minus_alphas)):
            got = got.numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
            want = P[pre + key]
            assert got.dtype == want.dtype, (name, key, got.dtype, want.dtype)
            assert np.array_equal(got.astype(np.float32), want.astype(np.float32)), (name, key)
        assert not np.any(np.asarray(s.ddim_sigmas, dtype=np.float64))
        # the step scalars: the reference's are torch CPU square roots, which are within an ulp of the rounded root but not always it
        # (plms._sqrt32); the sampler's are the rounded ones, so the two agree to one fp32 ulp, and exactly where torch rounded correctly
        want = P[pre + "step_coef"]
        got = np.asarray([s.step_coefficients(i)[:4] for i in range(len(s.ddim_timesteps))], dtype=np.float32)
        assert got.shape == want.shape and np.all(np.abs(got.view(np.int32) - want.view(np.int32)) <= 1), name
        assert all(s.step_coefficients(i)[4] == 0.0 for i in range(len(s.ddim_timesteps)))
    assert len(P["sched/3_quad/timesteps"]) == 3 and len(P["sched/1_uniform/timesteps"]) == 1


def test_square_roots_are_correctly_rounded():
    """_sqrt32(v) is the fp32 number nearest to the exact root: v lies between the squares of the two midpoints around it (exact rationals)"""
    from fractions import Fraction
    from sfron import plms
    g = torch.Generator().manual_seed(3)
    vals = torch.cat([torch.rand(2000, generator=g), host_model().alphas_cumprod, 1.0 - host_model().alphas_cumprod]).numpy()
    for v in vals:
        r = np.float32(plms._sqrt32(v))
        lo, hi = np.nextafter(r, np.float32(0)), np.nextafter(r, np.float32(2))
        mid_lo, mid_hi = (Fraction(float(lo)) + Fraction(float(r))) / 2, (Fraction(float(hi)) + Fraction(float(r))) / 2
        assert mid_lo * mid_lo <= Fraction(float(v)) <= mid_hi * mid_hi, float(v)


def test_guards_raise_naming_the_argument():
    from sfron import plms
    s = plms.PLMSSampler(host_model())
    with pytest.raises(ValueError, match="ddim_eta must be 0 for PLMS"):
        s.make_schedule(10, ddim_eta=0.5)
    base = dict(S=4, batch_size=1, shape=(4, 8, 8), conditioning=torch.zeros(1, 5, 24))
    with pytest.raises(ValueError, match="ddim_eta must be 0 for PLMS"):
        s.sample(**base, eta=1.0)
    one = torch.ones(1, 4, 8, 8)
    for kw, word in ((dict(score_corrector=object()), "score_corrector"), (dict(quantize_x0=True), "quantize_x0"),
                     (dict(dynamic_threshold=0.5), "dynamic_threshold"), (dict(noise_dropout=0.1), "noise_dropout"),
                     (dict(ddim_use_original_steps=True), "ddim_use_original_steps"), (dict(t_start=2), "t_start"), (dict(till_T=1), "till_T")):
        with pytest.raises(NotImplementedError, match="PLMSSampler: `" + word):
            s.sample(**base, **kw)
    s.make_schedule(4)
    for kw, word in ((dict(score_corrector=object()), "score_corrector"), (dict(quantize_denoised=True), "quantize_x0"),
                     (dict(dynamic_threshold=0.5), "dynamic_threshold"), (dict(noise_dropout=0.1), "noise_dropout"),
                     (dict(ddim_use_original_steps=True), "ddim_use_original_steps")):
        with pytest.raises(NotImplementedError, match=word):
            s.plms_sampling(torch.zeros(1, 5, 24), (1, 4, 8, 8), **kw)
    for kw, word in ((dict(use_original_steps=True), "use_original_steps"), (dict(score_corrector=object()), "score_corrector"),
                     (dict(quantize_denoised=True), "quantize_x0"), (dict(dynamic_threshold=0.5), "dynamic_threshold"),
                     (dict(noise_dropout=0.1), "noise_dropout")):
        with pytest.raises(NotImplementedError, match=word):
            s.p_sample_plms(one, torch.zeros(1, 5, 24), torch.zeros(1, dtype=torch.long), 0, old_eps=[], **kw)
    with pytest.raises(AssertionError):                 # mask without x0, as in the reference
        s.sample(**base, mask=one, x_T=one)


def test_sampler_refuses_cpu_model_outputs():
    """no CPU fall-back of the update or of the blend: a model that answers on the CPU is an error, not an eager step"""
    from sfron import _lib, plms
    m = host_model()
    m.apply_model = lambda x, t, c: x
    m.sqrt_alphas_cumprod, m.sqrt_one_minus_alphas_cumprod = m.alphas_cumprod.sqrt(), (1 - m.alphas_cumprod).sqrt()
    base = dict(S=4, batch_size=1, shape=(4, 8, 8), conditioning=torch.zeros(1, 5, 24), x_T=torch.zeros(1, 4, 8, 8))
    with pytest.raises(_lib.SfronError):
        plms.PLMSSampler(m).sample(**base)
    with pytest.raises(_lib.SfronError):
        plms.PLMSSampler(m).sample(**base, unconditional_guidance_scale=2.0, unconditional_conditioning=torch.zeros(1, 5, 24))
    with pytest.raises(_lib.SfronError):
        plms.PLMSSampler(m).sample(**base, mask=torch.ones(1, 1, 8, 8), x0=torch.zeros(1, 4, 8, 8))


@pytest.mark.parametrize("S,guided", [(1, True), (2, False), (3, True), (8, True)])
def test_history_bookkeeping(S, guided):
    """The model answers with its call number in every element; the mocked update writes that number where the sampler asked for the
    prediction to be kept.  So every launch's history can be read as call numbers: step k > 0 is model call k + 1, step 0 is calls 0 and 1
    and keeps call 0 (e_t), not call 1 (e_t_next)."""
    from sfron import _lib, plms
    m = host_model()
    B = 2
    calls, launches = [], []

    def apply_model(x, t, c):
        calls.append((x.shape[0], t.tolist(), c.shape[0]))
        return torch.full(x.shape, float(len(calls) - 1))
    m.apply_model = apply_model
    s = plms.PLMSSampler(m)

    def update(x, out, is_guided, old, order, guidance, coef, e_out, want_pred=True):
        assert is_guided == guided and out.shape[0] == (2 * B if guided else B) and len(old) <= 3
        launches.append(dict(order=order, old=[float(o.flatten()[0]) for o in old], call=float(out.flatten()[0]), kept=e_out is not None,
                             slot=None if e_out is None else e_out.data_ptr(), coef=coef, want_pred=want_pred))
        if e_out is not None:
            e_out.fill_(float(out.flatten()[0]))
        return torch.zeros_like(x), (torch.zeros_like(x) if want_pred else None)
    s._update = update
    kw = dict(unconditional_guidance_scale=2.0, unconditional_conditioning=torch.zeros(B, 5, 24)) if guided else {}
    seen = []
    s.make_schedule(S, ddim_discretize="quad" if S == 3 else "uniform", verbose=False)
    total = len(s.ddim_timesteps)
    smp, inter = s.plms_sampling(torch.zeros(B, 5, 24), (B, 4, 8, 8), x_T=torch.zeros(B, 4, 8, 8), log_every_t=1, callback=seen.append,
                                 img_callback=lambda pred, i: seen.append(("img", i, tuple(pred.shape))), **kw)
    assert total == S and len(calls) == S + 1 and len(launches) == S + 1
    assert all(c[0] == (2 * B if guided else B) and c[2] == c[0] for c in calls)
    # the timesteps of the calls: t, then t_next for the second half of the first step (t itself when S == 1), then every later step's t
    ts = [int(t) for t in np.flip(s.ddim_timesteps)]
    assert [c[1][0] for c in calls] == [ts[0], ts[min(1, S - 1)]] + ts[1:]
    want_orders = [_lib.PLMS_ORDER1, _lib.PLMS_MEAN] + [(_lib.PLMS_ORDER2, _lib.PLMS_ORDER3, _lib.PLMS_ORDER4)[min(k, 3) - 1] for k in range(1, S)]
    assert [l["order"] for l in launches] == want_orders
    # the first step: ORDER1 keeps call 0 and wants no pred_x0; MEAN reads it back as old1 and keeps nothing
    assert launches[0]["kept"] and launches[0]["old"] == [] and not launches[0]["want_pred"]
    assert not launches[1]["kept"] and launches[1]["old"] == [0.0] and launches[1]["call"] == 1.0 and launches[1]["want_pred"]
    assert launches[0]["coef"] == launches[1]["coef"] == s.step_coefficients(S - 1)
    kept = [0.0]                                        # the predictions held, oldest first, as call numbers
    for k in range(1, S):
        l = launches[k + 1]
        assert l["call"] == float(k + 1) and l["kept"] and l["coef"] == s.step_coefficients(S - 1 - k)
        assert l["old"] == list(reversed(kept[-3:])), (k, l["old"], kept)
        kept.append(l["call"])
        kept = kept[-3:]                                 # never more than three
    assert len({l["slot"] for l in launches if l["slot"] is not None}) == min(S, 3)       # three buffers, allocated once and reused
    assert seen == [v for i in range(S) for v in (i, ("img", i, (B, 4, 8, 8)))]
    assert len(inter["x_inter"]) == S + 1 and smp is inter["x_inter"][-1]


def test_chunked_runs_slice_their_operands():
    from sfron import plms
    s = plms.PLMSSampler(host_model())
    s.chunk_size = lambda batch_size, shape: 2
    B = 5
    g = torch.Generator().manual_seed(1)
    x_T, x0, cond, uc = (torch.randn(B, 4, 8, 8, generator=g), torch.randn(B, 4, 8, 8, generator=g), torch.randn(B, 5, 24, generator=g),
                         torch.randn(B, 5, 24, generator=g))
    noise = torch.randn(4, B, 4, 8, 8, generator=g)
    seen = []

    def plms_sampling(cond, shape, **kw):
        seen.append(dict(cond=cond, shape=shape, **kw))
        return kw["x_T"] + 1, {"x_inter": [kw["x_T"], kw["x_T"] + 1], "pred_x0": [kw["x_T"], kw["x_T"] - 1]}
    s.plms_sampling = plms_sampling
    for mask in (torch.ones(B, 1, 8, 8) * torch.arange(B).view(B, 1, 1, 1), torch.ones(1, 1, 8, 8)):
        seen.clear()
        smp, inter = s.sample(S=4, batch_size=B, shape=(4, 8, 8), conditioning=cond, unconditional_conditioning=uc, x_T=x_T, mask=mask, x0=x0,
                              inpaint_noise=noise, unconditional_guidance_scale=2.0, log_every_t=1, verbose=False)
        assert [c["shape"] for c in seen] == [(2, 4, 8, 8), (2, 4, 8, 8), (1, 4, 8, 8)]
        for c, (lo, hi) in zip(seen, ((0, 2), (2, 4), (4, 5))):
            assert torch.equal(c["cond"], cond[lo:hi]) and torch.equal(c["unconditional_conditioning"], uc[lo:hi])
            assert torch.equal(c["x_T"], x_T[lo:hi]) and torch.equal(c["x0"], x0[lo:hi])
            assert torch.equal(c["mask"], mask if mask.shape[0] == 1 else mask[lo:hi])
            for k in range(4):
                assert torch.equal(c["inpaint_noise"][k], noise[k][lo:hi])
            assert c["unconditional_guidance_scale"] == 2.0 and c["log_every_t"] == 1
        assert torch.equal(smp, x_T + 1) and torch.equal(inter["x_inter"][1], x_T + 1) and torch.equal(inter["pred_x0"][1], x_T - 1)
    # without inpainting nothing is sliced that is not there
    seen.clear()
    s.sample(S=4, batch_size=B, shape=(4, 8, 8), conditioning=cond, x_T=x_T, verbose=False)
    assert all(c["mask"] is None and c["x0"] is None and c["inpaint_noise"] is None and c["unconditional_conditioning"] is None for c in seen)


def test_sample_model_drives_the_sampler_unchanged():
    """sd.sample_model hands t_start = -1, till_T = None and verbose_iter on: the defaults pass, nothing else does"""
    import types
    from sfron import plms, sd
    s = plms.PLMSSampler(host_model())
    seen = {}

    def plms_sampling(cond, shape, **kw):
        seen.update(kw, shape=shape)
        return "z", "inter"
    s.plms_sampling = plms_sampling
    model = types.SimpleNamespace(get_learned_conditioning=lambda p: torch.zeros(len(p), 5, 24))
    assert sd.sample_model(model, s, torch.zeros(2, 5, 24), 64, 64, 8, 3.0, 0.0, n_samples=2, verbose=False) == "z"
    assert seen["shape"] == (2, 4, 8, 8) and len(s.ddim_timesteps) == 8 and seen["unconditional_guidance_scale"] == 3.0
    with pytest.raises(NotImplementedError, match="t_start"):
        sd.sample_model(model, s, torch.zeros(2, 5, 24), 64, 64, 7, 3.0, 0.0, n_samples=2, t_start=5)
    with pytest.raises(ValueError):
        sd.sample_model(model, s, torch.zeros(2, 5, 24), 64, 64, 7, 3.0, 0.5, n_samples=2)
