"""GPU: the native DiT sampler (csrc/dit_sample.hip, sfron.dit_sample, the DDIM API of sfron.diffusion.GaussianDiffusion).

Step kernel: mode DDPM bit for bit against sfron_cfg_combine + sfron_p_sample (the library builds with -ffp-contract=off), modes DDIM and
DDIM_REVERSE against an fp32 torch restatement of the reference's expressions at the project's bound for a single p_sample step (2e-6).
Public API against the reference's own outputs (tests/golden/dit_sampler.npz, made by tests/golden/make_dit_sampler_golden.py) at the
bounds the ancestral loops have on the same stubs.  The advance kernel against the host tables.  The whole sampler on a small DiT, bit for
bit against the existing host loop from the same generator.  SFRON_IMAGE_TRUNC against the float64 byte rule, and the drivers' files.

Every kernel output sits between guard regions pre-filled with a bit pattern (as in test_gpu_attention_grid.py): a store outside the body
changes a guard.  Measured distances are printed before they are asserted (DIT-SAMPLER-METRIC lines)."""
import os

import numpy as np
import pytest
import torch

from test_dit_sampler_cpu import trunc_u8_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEAD, TAIL = 8, 256                                  # guard elements in front of / behind every output
PATTERN = {torch.float32: 0x5AA55AA5, torch.int64: 0x5AA55AA55AA55AA5, torch.int32: 0x5AA55AA5, torch.uint8: 0xAB}
BITS = {torch.float32: torch.int32, torch.int64: torch.int64, torch.int32: torch.int32, torch.uint8: torch.uint8}


@pytest.fixture(scope="module")
def G(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "dit_sampler.npz")))


@pytest.fixture(scope="module")
def S(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "dit_sampling.npz")))


class _Out:
    """An output of ``shape`` at offset LEAD of an allocation of LEAD + n + TAIL elements, all pre-filled with the bit pattern."""

    def __init__(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.n, self.pat = n, PATTERN[dtype]
        self.big = torch.empty(LEAD + n + TAIL, dtype=dtype, device=DEV)
        self.bits = self.big.view(BITS[dtype])
        self.bits.fill_(self.pat)
        self.t = self.big[LEAD:LEAD + n].view(shape)

    def guards_intact(self):
        return bool((self.bits[:LEAD] == self.pat).all()) and bool((self.bits[LEAD + self.n:] == self.pat).all())

    def untouched(self):
        return bool((self.bits == self.pat).all())


def _call(name, *args):
    from sfron import _lib
    from sfron._lib import stream_ptr
    return getattr(_lib.lib(), name)(*args, stream_ptr())


def _step(d, x, out, t, noise, n, C, hw, guided, n_guided, s, mode, eta, clip, sample, dup, pred):
    from sfron._lib import ptr
    p = lambda v: v if isinstance(v, int) or v is None else ptr(v)
    return _call("sfron_dit_sample_step", ptr(x), ptr(out), ptr(t), ptr(d.sampler_tab), p(noise), n, C, hw, int(guided), n_guided, s, mode, eta,
                 int(clip), p(sample), p(dup), p(pred))


def _inputs(n, C, hw, rows, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, hw, generator=g).to(DEV)
    out = torch.randn(rows, 2 * C, hw, generator=g).to(DEV)
    noise = torch.randn(n, C, hw, generator=g).to(DEV)
    t = torch.tensor([0, 9, 3, 1, 5][:n] if n <= 5 else [k % 10 for k in range(n)], dtype=torch.int64, device=DEV)
    return x, out, noise, t


@pytest.fixture(scope="module")
def d10():
    from sfron import diffusion
    return diffusion.create_diffusion("10", device=DEV)


# ------------------------------------------------------------------------------------------------ step kernel, mode DDPM: bit for bit
# hw = 5 and 4099 are odd; C * 4099 = 16396 elements per sample is more than the 64 x 256 threads of a grid row (the stride loop runs twice)
@pytest.mark.parametrize("n,C,hw,n_guided", [(3, 4, 64, 0), (3, 4, 64, 3), (3, 4, 64, 4), (1, 4, 5, 3), (2, 4, 4099, 3), (3, 3, 63, 2)])
@pytest.mark.parametrize("clip", [0, 1])
def test_guided_ancestral_step_is_cfg_combine_then_p_sample_bit_for_bit(d10, n, C, hw, n_guided, clip):
    from sfron._lib import ptr
    s = 1.7
    x, out, noise, t = _inputs(n, C, hw, 2 * n, seed=n + hw + n_guided)
    ref_out = out.clone()
    if n_guided > 0:                                   # sfron_cfg_combine refuses n_guided == 0: nothing to mix
        assert _call("sfron_cfg_combine", ptr(ref_out), 2 * n, 2 * C, hw, n_guided, s) == 0
    want, want_pred = torch.empty_like(x), torch.empty_like(x)
    assert _call("sfron_p_sample", ptr(x), ptr(ref_out), ptr(t), ptr(d10.tab), ptr(noise), n, C, hw, clip, ptr(want), ptr(want_pred)) == 0
    sample, dup, pred = _Out(x.shape), _Out(x.shape), _Out(x.shape)
    out_before = out.clone()
    assert _step(d10, x, out, t, noise, n, C, hw, 1, n_guided, s, 0, 0.0, clip, sample.t, dup.t, pred.t) == 0
    assert sample.guards_intact() and dup.guards_intact() and pred.guards_intact()
    assert torch.equal(sample.t, want) and torch.equal(pred.t, want_pred) and torch.equal(dup.t, sample.t)
    assert torch.equal(out, out_before)                # the model output is read only
    # in place on x, without the optional outputs
    xi = _Out(x.shape)
    xi.t.copy_(x)
    assert _step(d10, xi.t, out, t, noise, n, C, hw, 1, n_guided, s, 0, 0.0, clip, xi.t, None, None) == 0
    assert xi.guards_intact() and torch.equal(xi.t, want)


@pytest.mark.parametrize("n,C,hw", [(3, 4, 64), (1, 4, 5), (2, 4, 4099)])
def test_unguided_ancestral_step_is_p_sample_bit_for_bit(d10, n, C, hw):
    from sfron._lib import ptr
    x, out, noise, t = _inputs(n, C, hw, n, seed=hw)
    want, want_pred = torch.empty_like(x), torch.empty_like(x)
    assert _call("sfron_p_sample", ptr(x), ptr(out), ptr(t), ptr(d10.tab), ptr(noise), n, C, hw, 0, ptr(want), ptr(want_pred)) == 0
    sample, pred = _Out(x.shape), _Out(x.shape)
    assert _step(d10, x, out, t, noise, n, C, hw, 0, 3, 4.0, 0, 0.0, 0, sample.t, None, pred.t) == 0
    assert sample.guards_intact() and pred.guards_intact() and torch.equal(sample.t, want) and torch.equal(pred.t, want_pred)
    # a t == 0 row ignores the noise (row 0), every other row does not
    again = _Out(x.shape)
    assert _step(d10, x, out, t, (noise * 3).contiguous(), n, C, hw, 0, 3, 4.0, 0, 0.0, 0, again.t, None, None) == 0
    assert torch.equal(again.t[0], sample.t[0])
    assert all(not torch.equal(again.t[k], sample.t[k]) for k in range(1, n))


def test_a_refused_step_leaves_the_outputs_untouched(d10):
    from sfron import _lib
    n, C, hw = 2, 4, 16
    x, out, noise, t = _inputs(n, C, hw, 2 * n, seed=1)
    sample, dup, pred = _Out(x.shape), _Out(x.shape), _Out(x.shape)
    for kw in (dict(mode=3), dict(n_guided=5), dict(s=float("nan")), dict(mode=2, eta=0.5), dict(mode=1, eta=0.5, noise=None),
               dict(mode=0, noise=None)):
        a = dict(mode=0, n_guided=3, s=4.0, eta=0.0, noise=noise)
        a.update(kw)
        rc = _step(d10, x, out, t, a["noise"], n, C, hw, 1, a["n_guided"], a["s"], a["mode"], a["eta"], 0, sample.t, dup.t, pred.t)
        assert rc == _lib.ERR_ARG, kw
    assert _step(d10, x, out, t, noise, n, C, hw, 1, 3, 4.0, 0, 0.0, 0, sample.t, dup.t, sample.t) == _lib.ERR_ARG          # pred aliases sample
    torch.cuda.synchronize()
    assert sample.untouched() and dup.untouched() and pred.untouched()


# ------------------------------------------------------------------------------------------------ step kernel, modes DDIM / DDIM_REVERSE
def _restate(d, x, out, t, noise, mode, eta, clip, guided, n_guided, s):
    """gaussian_diffusion.py:513-598 over p_mean_variance (:254-332) and forward_with_cfg's mix, expression for expression, in fp32 torch
    on the device; the gathered table entries are the fp32 values _extract_into_tensor yields."""
    n, C = x.shape[0], x.shape[1]
    r = d.sampler_tab[t]
    col = lambda k: r[:, k].view(-1, 1, 1)
    eps = out[:n, :C].clone()
    if guided and n_guided:
        c, u = out[:n, :n_guided], out[n:, :n_guided]
        eps[:, :n_guided] = u + s * (c - u)
    pred = col(2) * x - col(3) * eps
    if clip:
        pred = pred.clamp(-1, 1)
    eps = (col(2) * x - pred) / col(3)
    if mode == 2:
        abn = col(10)
        return pred * torch.sqrt(abn) + torch.sqrt(1 - abn) * eps, pred
    ab, abp = col(8), col(9)
    sigma = eta * torch.sqrt((1 - abp) / (1 - ab)) * torch.sqrt(1 - ab / abp)
    mean = pred * torch.sqrt(abp) + torch.sqrt(1 - abp - sigma ** 2) * eps
    nz = (t != 0).float().view(-1, 1, 1)
    return mean + nz * sigma * noise, pred


@pytest.mark.parametrize("guided", [0, 1])
@pytest.mark.parametrize("mode,eta", [(1, 0.0), (1, 0.5), (1, 1.0), (2, 0.0)])
def test_ddim_steps_match_the_fp32_restatement(d10, mode, eta, guided):
    worst = 0.0
    for n, C, hw, clip in ((5, 4, 64, 0), (5, 4, 64, 1), (1, 4, 5, 0), (2, 4, 4099, 0)):
        x, out, noise, t = _inputs(n, C, hw, (2 if guided else 1) * n, seed=7 * n + hw + mode)
        want, want_pred = _restate(d10, x, out, t, noise, mode, eta, clip, guided, 3, 1.7)
        assert torch.isfinite(want).all()
        sample, dup, pred = _Out(x.shape), _Out(x.shape), _Out(x.shape)
        assert _step(d10, x, out, t, noise, n, C, hw, guided, 3, 1.7, mode, eta, clip, sample.t, dup.t, pred.t) == 0
        assert sample.guards_intact() and dup.guards_intact() and pred.guards_intact()
        err = float(((sample.t - want).abs() / (2e-6 + 2e-6 * want.abs())).max())          # in units of the bound
        worst = max(worst, err)
        print(f"DIT-SAMPLER-METRIC step mode={mode} eta={eta} guided={guided} n={n} hw={hw} clip={clip} err/bound={err:.3f} "
              f"max_abs={float((sample.t - want).abs().max()):.3e}")
        torch.testing.assert_close(sample.t, want, rtol=2e-6, atol=2e-6)
        torch.testing.assert_close(pred.t, want_pred, rtol=2e-6, atol=2e-6)
        assert torch.equal(dup.t, sample.t)
        if mode == 2 or eta == 0.0:                    # a NULL noise counts as zeros
            nn = _Out(x.shape)
            assert _step(d10, x, out, t, None, n, C, hw, guided, 3, 1.7, mode, eta, clip, nn.t, None, None) == 0
            assert nn.guards_intact() and torch.equal(nn.t, sample.t)
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ the public DDIM API against the reference
def _stubs(S):
    A = torch.from_numpy(S["A"]).to(DEV)
    s1m = torch.tensor(np.sqrt(1.0 - S["abar1000"]), dtype=torch.float32, device=DEV)
    C = S["z"].shape[1]
    seen = []

    def stub(x, ts, **kw):
        seen.append(ts.clone())
        return torch.einsum("oc,nchw->nohw", A, x) * torch.cos(ts.float() / 300.0).view(-1, 1, 1, 1) + 0.05

    def stub2(x, ts, **kw):
        seen.append(ts.clone())
        lin = torch.einsum("oc,nchw->nohw", A, x)
        eps = 0.9 * x / s1m[ts].view(-1, 1, 1, 1) + 0.02 * lin[:, :C]
        return torch.cat([eps, lin[:, C:] * torch.cos(ts.float() / 300.0).view(-1, 1, 1, 1) + 0.05], dim=1)
    return stub, stub2, seen


def _report(name, got, want, rtol, atol):
    got, want = got.detach().cpu().double(), torch.as_tensor(want).double()
    err = float(((got - want).abs() / (atol + rtol * want.abs())).max())
    print(f"DIT-SAMPLER-METRIC {name} max_abs={float((got - want).abs().max()):.3e} err/bound={err:.3f}")
    return err


def test_ddim_single_steps_match_the_reference(d10, G, S):
    stub, _, seen = _stubs(S)
    z = torch.from_numpy(S["z"])
    t = torch.tensor([0, 9, 3, 0], device=DEV)
    torch.manual_seed(5)                                    # the reference drew randn_like(x) from this CPU stream
    noise = torch.randn_like(z)
    one = d10.ddim_sample(stub, z.to(DEV), t, clip_denoised=False, model_kwargs={}, eta=0.5, noise=noise.to(DEV))
    rev = d10.ddim_reverse_sample(stub, z.to(DEV), t, clip_denoised=False, model_kwargs={}, eta=0.0)
    errs = [_report("one_ddim_sample", one["sample"], G["one_ddim_sample"], 2e-6, 2e-6),
            _report("one_ddim_pred_xstart", one["pred_xstart"], G["one_ddim_pred_xstart"], 2e-6, 2e-6),
            _report("one_rev_sample", rev["sample"], G["one_rev_sample"], 2e-6, 2e-6),
            _report("one_rev_pred_xstart", rev["pred_xstart"], G["one_rev_pred_xstart"], 2e-6, 2e-6)]
    assert [s.tolist() for s in seen] == [[int(G["map_10"][k]) for k in (0, 9, 3, 0)]] * 2          # ORIGINAL timesteps, per row
    assert max(errs) <= 1.0, errs
    # t == 0 rows carry no noise
    one3 = d10.ddim_sample(stub, z.to(DEV), t, clip_denoised=False, model_kwargs={}, eta=0.5, noise=(noise * 3).to(DEV))
    assert torch.equal(one3["sample"][0], one["sample"][0]) and torch.equal(one3["sample"][3], one["sample"][3])
    assert not torch.equal(one3["sample"][1], one["sample"][1])


@pytest.mark.parametrize("spec", ["10", "ddim25"])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_ddim_sample_loop_matches_the_reference(G, S, spec, eta):
    """Clipped loops (linear stub) at rtol = atol = 2e-5, the unclamped ones (contractive stub2) at rtol 2e-4, atol 2e-5: the bounds of
    the ancestral loops on the same stubs (tests/test_gpu_sampling.py)."""
    from sfron import diffusion
    d = diffusion.create_diffusion(spec, device=DEV)
    stub, stub2, seen = _stubs(S)
    z = torch.from_numpy(S["z"])
    errs = []
    for name, fn, clip, rtol, atol in (("stub_clip1", stub, True, 2e-5, 2e-5), ("stub2_clip0", stub2, False, 2e-4, 2e-5)):
        torch.manual_seed(77)                               # one randn_like(x) per step from this CPU stream, for eta == 0 too
        step_noise = [torch.randn_like(z).to(DEV) for _ in range(d.num_timesteps)]
        del seen[:]
        got = d.ddim_sample_loop(fn, z.shape, z.to(DEV), clip_denoised=clip, model_kwargs={}, device=DEV, eta=eta, step_noise=step_noise)
        assert torch.isfinite(got).all()
        assert [int(s[0]) for s in seen] == list(G[f"map_{spec}"])[::-1]           # the model sees ORIGINAL timesteps, last first
        errs.append(_report(f"loop/{spec}/{name}/{eta}", got, G[f"loop/{spec}/{name}/{eta}"], rtol, atol))
    assert max(errs) <= 1.0, errs


def test_ddim_reverse_trajectory_matches_the_reference(d10, G, S):
    _, stub2, seen = _stubs(S)
    x = (0.1 * torch.from_numpy(S["z"])).to(DEV)
    errs = []
    for i in range(10):
        x = d10.ddim_reverse_sample(stub2, x, torch.full((4,), i, dtype=torch.int64, device=DEV), clip_denoised=False, model_kwargs={})["sample"]
        errs.append(_report(f"rev_traj[{i}]", x, G["rev_traj"][i], 2e-4, 2e-5))
    assert [int(s[0]) for s in seen] == list(G["map_10"])                          # first to last
    assert max(errs) <= 1.0, errs


# ------------------------------------------------------------------------------------------------ advance kernel
@pytest.mark.parametrize("n,rows", [(3, 6), (300, 600)])
def test_advance_kernel_walks_the_host_tables_and_clamps(n, rows):
    from sfron import diffusion
    from sfron._lib import ptr
    d = diffusion.create_diffusion("5", device=DEV)
    T = d.num_timesteps
    order = torch.arange(T - 1, -1, -1, dtype=torch.int64, device=DEV)
    step, t_idx, t_model = _Out((1,), torch.int32), _Out((n,), torch.int64), _Out((rows,), torch.int64)
    step.t.zero_()
    for k in range(T + 1):
        assert _call("sfron_dit_sampler_advance", ptr(order), ptr(d.map_tensor), T, T, ptr(step.t), ptr(t_idx.t), n, ptr(t_model.t), rows) == 0
        i = T - 1 - min(k + 1, T - 1)                       # order[min(k + 1, T - 1)] on the host
        assert step.guards_intact() and t_idx.guards_intact() and t_model.guards_intact()
        assert int(step.t) == min(k + 1, T), k              # a launch past the end leaves the counter at T
        assert t_idx.t.tolist() == [i] * n and t_model.t.tolist() == [d.timestep_map[i]] * rows, k
    step.t.fill_(-7)                                        # a counter below the range counts as 0
    assert _call("sfron_dit_sampler_advance", ptr(order), ptr(d.map_tensor), T, T, ptr(step.t), ptr(t_idx.t), n, ptr(t_model.t), rows) == 0
    assert int(step.t) == 1 and t_idx.t.tolist() == [T - 2] * n


# ------------------------------------------------------------------------------------------------ the whole sampler on a small DiT
def _small_dit(seed=0):
    from sfron import dit
    from test_gpu_dit import CASES
    torch.manual_seed(seed)
    model = dit.DiT(batch_size=4, **CASES["hd64"])
    dit.randomize_zero_init(model, std=0.05, seed=seed + 1)
    model.train()
    return model


LABELS = [1, 9, 4]


def _draw_z(seed, n=3):
    g = torch.Generator().manual_seed(seed)
    return g, torch.randn(n, 4, 32, 32, generator=g)


def test_sampler_ddpm_is_the_host_loop_bit_for_bit_and_leaves_the_runner_alone():
    from sfron import diffusion, dit_sample, images
    model = _small_dit()
    eng = model.engine
    d5 = diffusion.create_diffusion("5", device=DEV)
    n = len(LABELS)
    g, z = _draw_z(11)
    rng_cpu, rng_gpu = torch.get_rng_state(), torch.cuda.get_rng_state()
    got = dit_sample.DiTSampler(model, d5, 4.0, mode="ddpm").sample(z.to(DEV), torch.tensor(LABELS, device=DEV), generator=g)
    assert torch.equal(torch.get_rng_state(), rng_cpu) and torch.equal(torch.cuda.get_rng_state(), rng_gpu)
    assert model.engine is eng and model.engine.cfg.batch == 4 and model.training          # engine, batch size and mode as they were
    assert got.shape == (n, 4, 32, 32) and torch.isfinite(got).all()
    # the existing loop, same seed: z, then one [2n, ...] draw per step
    g2, z2 = _draw_z(11)
    zc = torch.cat([z2, z2], 0).to(DEV)
    yc = torch.tensor(LABELS + [10] * n, device=DEV)
    model.eval()
    want = d5.p_sample_loop(model.forward_with_cfg, zc.shape, zc, clip_denoised=False, model_kwargs=dict(y=yc, cfg_scale=4.0), device=DEV,
                            step_noise=images._StepNoise(zc.shape, g2, DEV))
    assert torch.equal(got, want[:n])
    assert not torch.equal(got, z.to(DEV))
    # explicit per-step noise gives the same
    g3, z3 = _draw_z(11)
    noises = [torch.randn(2 * n, 4, 32, 32, generator=g3).to(DEV) for _ in range(5)]
    again = dit_sample.DiTSampler(model, d5, 4.0).sample(z3.to(DEV), torch.tensor(LABELS, device=DEV), step_noise=noises)
    assert torch.equal(again, got) and not model.training          # eval stays eval


def test_sampler_ddim_is_the_host_loop_bit_for_bit():
    from sfron import diffusion, dit_sample
    model = _small_dit(seed=2)
    model.eval()
    d5 = diffusion.create_diffusion("5", device=DEV)
    n = len(LABELS)
    _, z = _draw_z(5)
    y = torch.tensor(LABELS, device=DEV)
    got = dit_sample.DiTSampler(model, d5, 4.0, mode="ddim", eta=0.0).sample(z.to(DEV), y)
    x = torch.cat([z, z], 0).to(DEV)
    yc = torch.tensor(LABELS + [10] * n, device=DEV)
    for i in range(4, -1, -1):
        t = torch.full((2 * n,), i, dtype=torch.int64, device=DEV)
        x = d5.ddim_sample(model.forward_with_cfg, x, t, clip_denoised=False, model_kwargs=dict(y=yc, cfg_scale=4.0), eta=0.0)["sample"]
    assert torch.isfinite(got).all() and torch.equal(got, x[:n])
    # unguided (cfg_scale <= 1): the engine runs at batch n through the plain forward pass
    plain = dit_sample.DiTSampler(model, d5, 1.0, mode="ddim").sample(z.to(DEV), y)
    want = d5.ddim_sample_loop(model.forward, z.shape, z.to(DEV), clip_denoised=False, model_kwargs=dict(y=y), device=DEV)
    assert torch.equal(plain, want) and not torch.equal(plain, got)
    # eta != 0 draws per step from the generator, [2n, ...] each, first n rows used
    g = torch.Generator().manual_seed(3)
    noisy = dit_sample.DiTSampler(model, d5, 4.0, mode="ddim", eta=0.5).sample(z.to(DEV), y, generator=g)
    g = torch.Generator().manual_seed(3)
    x = torch.cat([z, z], 0).to(DEV)
    for i in range(4, -1, -1):
        t = torch.full((2 * n,), i, dtype=torch.int64, device=DEV)
        nz = torch.randn(2 * n, 4, 32, 32, generator=g).to(DEV)
        x = d5.ddim_sample(model.forward_with_cfg, x, t, clip_denoised=False, model_kwargs=dict(y=yc, cfg_scale=4.0), eta=0.5, noise=nz)["sample"]
    assert torch.equal(noisy, x[:n])


# ------------------------------------------------------------------------------------------------ SFRON_IMAGE_TRUNC
def test_trunc_image_mode_is_the_float64_rule_and_leaves_the_other_modes_alone():
    from sfron import images
    from sfron._lib import ptr
    from test_vae_decoder_cpu import round_u8, save_image_u8
    g = torch.Generator().manual_seed(8)
    B, H, W, ld = 3, 9, 11, 4
    # multiples of 2^-12: 127.5 x and the sum are exact in fp32, so the fp32 kernel and the float64 rule see the same number
    rows = torch.round(torch.randn(B * H * W, ld, generator=g) * 0.8 * 4096) / 4096
    edges = torch.tensor([-1.004, -1.0, -0.5 / 127.5, 0.0, 1.0 - 1.0 / 255.0, 1.0, 1.01, -0.0, 1e9, -1e9, 0.5, -0.5, 1.0 - 1.5 / 255.0])
    rows.view(-1)[: edges.numel()] = edges
    img = rows[:, :3].reshape(B, H, W, 3)
    assert float((img.abs() > 1).double().mean()) > 0.05
    dr = rows.to(DEV)
    out = _Out((B, H, W, 3), torch.uint8)
    assert _call("sfron_rows_to_image_u8", ptr(dr), ld, B, H, W, images.image_mode("trunc"), 0.0, 0.0, 0, 0, 0, B, ptr(out.t)) == 0
    assert out.guards_intact()
    assert np.array_equal(out.t.cpu().numpy(), trunc_u8_f64(img.numpy()))
    # arbitrary fp32 values: the reference's own fp32 line (sample_ddp.py:132), evaluated by torch on the device
    wild = (torch.randn(B * H * W, ld, generator=g) * 0.8).to(DEV)
    out2 = _Out((B, H, W, 3), torch.uint8)
    assert _call("sfron_rows_to_image_u8", ptr(wild), ld, B, H, W, 2, 0.0, 0.0, 0, 0, 0, B, ptr(out2.t)) == 0
    want2 = torch.clamp(127.5 * wild[:, :3].reshape(B, H, W, 3) + 128.0, 0, 255).to(torch.uint8)
    assert out2.guards_intact() and torch.equal(out2.t, want2)
    # the make_grid canvas carries the same bytes
    grid = torch.full(images.grid_geometry(B, H, W, 2, 1)[:2] + (3,), 0xAB, dtype=torch.uint8, device=DEV)
    assert _call("sfron_rows_to_image_u8", ptr(dr), ld, B, H, W, 2, 0.0, 0.0, 2, 1, 0, B, ptr(grid)) == 0
    assert torch.equal(grid[1:1 + H, 1:1 + W], out.t[0]) and torch.equal(grid[2 + H:2 + 2 * H, 1:1 + W], out.t[2])
    # modes 0 and 1 on the same input: the existing expectations
    for mode, want in (("save_image", save_image_u8(img)), ("round", round_u8(img))):
        o = _Out((B, H, W, 3), torch.uint8)
        assert _call("sfron_rows_to_image_u8", ptr(dr), ld, B, H, W, images.image_mode(mode), -1.0, 1.0, 0, 0, 0, B, ptr(o.t)) == 0
        assert o.guards_intact() and torch.equal(o.t.cpu(), want), mode
    x = rows[:, :3].reshape(B, H, W, 3).permute(0, 3, 1, 2).contiguous()
    from test_vae_decoder_cpu import make_grid_u8_ref
    assert torch.equal(images.make_grid_u8(x.to(DEV), nrow=2, normalize=True, value_range=(-1, 1)).cpu(),
                       make_grid_u8_ref(save_image_u8(img), 2, 2))


# ------------------------------------------------------------------------------------------------ drivers
@pytest.fixture(scope="module")
def small_dec(golden_dir):
    from test_gpu_vae_decoder import small_decoder
    return small_decoder(dict(np.load(os.path.join(golden_dir, "vae_decoder.npz"))))


def test_sample_fid_writes_the_files_and_the_npz_of_a_seeded_sampler(small_dec, tmp_path):
    from sfron import diffusion, dit_sample
    model = _small_dit(seed=1)
    d = str(tmp_path / dit_sample.sample_folder_name("DiT-S/4", None, 256, "ema", 1.5, 3))
    path = dit_sample.sample_fid(model, small_dec, num_fid_samples=5, per_proc_batch_size=2, num_classes=10, cfg_scale=1.5,
                                 num_sampling_steps=3, image_size=256, sample_dir=d, global_seed=3)
    assert path == d + ".npz" and sorted(os.listdir(d)) == [f"{k:06d}.png" for k in range(6)]
    arr = np.load(path)["arr_0"]
    assert model.training and model.engine.cfg.batch == 4
    # a second, identically seeded sampler
    g = torch.Generator(device=DEV).manual_seed(3 * 1 + 0)
    sampler = dit_sample.DiTSampler(model, diffusion.create_diffusion("3", device=DEV), 1.5)
    want = []
    for _ in range(3):
        z = torch.randn(2, 4, 32, 32, generator=g, device=DEV)
        y = torch.randint(0, 10, (2,), generator=g, device=DEV)
        want.append(small_dec.decode_u8(sampler.sample(z, y, generator=g), 0.18215, "trunc"))
    want = torch.cat(want).cpu().numpy()
    assert arr.dtype == np.uint8 and arr.shape == (5,) + want.shape[1:] and want.shape[3] == 3
    assert np.array_equal(arr, want[:5])
    assert len(np.unique(arr)) > 8                          # pictures, not a constant


def test_sample_writes_the_reference_grid(small_dec, tmp_path):
    from PIL import Image
    from sfron import diffusion, dit_sample, images
    model = _small_dit(seed=1)
    labels = (1, 9, 4, 7, 2)
    p = str(tmp_path / "sample.png")
    grid = dit_sample.sample(model, diffusion_steps=3, class_labels=labels, cfg_scale=4.0, decoder=small_dec, path=p,
                             generator=torch.Generator().manual_seed(4))
    H = W = small_dec.factor * 32
    assert tuple(grid.shape) == images.grid_geometry(5, H, W, nrow=4, padding=2)[:2] + (3,)          # save_image(nrow=4): 2 rows of 4 cells
    assert np.array_equal(np.asarray(Image.open(p).convert("RGB")), grid.cpu().numpy())
    g, z = torch.Generator().manual_seed(4), None
    z = torch.randn(5, 4, 32, 32, generator=g)
    lat = dit_sample.DiTSampler(model, diffusion.create_diffusion("3", device=DEV), 4.0).sample(z.to(DEV), torch.tensor(labels, device=DEV),
                                                                                                  generator=g)
    assert torch.equal(grid, small_dec.decode_u8(lat, 0.18215, "save_image", nrow=4, value_range=(-1.0, 1.0)))


def test_sample_visualization_native_gives_the_default_path_bytes(small_dec, tmp_path):
    from sfron import diffusion, images
    model = _small_dit()
    eng = model.engine
    d5 = diffusion.create_diffusion("5", device=DEV)
    labels = [1, 9, 4, 7]
    a = images.sample_visualization(model, d5, small_dec, 32, 7, str(tmp_path / "a"), class_labels=labels,
                                    generator=torch.Generator().manual_seed(11))
    b = images.sample_visualization(model, d5, small_dec, 32, 7, str(tmp_path / "b"), class_labels=labels,
                                    generator=torch.Generator().manual_seed(11), native=True)
    assert torch.equal(a, b) and len(torch.unique(a)) > 8
    assert model.engine is eng and model.engine.cfg.batch == 4 and model.training
    assert open(tmp_path / "a" / "0000007_sample.png", "rb").read() == open(tmp_path / "b" / "0000007_sample.png", "rb").read()
