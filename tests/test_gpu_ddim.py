"""GPU: the ldm DDIM sampler and prompt-to-image path of SD v1 -- the two kernels it adds (sfron_ddim_cfg_step, sfron_xattn_fwd), the
UNet's inference path (PreparedContext, fused_cross_attention), sfron.ddim.DDIMSampler against the reference's trajectories
(tests/golden/ddim.npz, made by tests/golden/make_ddim_golden.py from SD/ldm/models/diffusion/ddim.py) and generate_images end to end.

Bounds (none is tuned to what the kernels give):
  sfron_ddim_cfg_step  per element 8 * 2^-24 * (|x| s3 / s2 + (1 + 2 g) max|eps| (s1 s3 / s2 + dir) + sigma |noise|): eight fp32 roundings
                       of a sum whose terms have these magnitudes (pred_x0: the same with s3 = 1 and dir = 0).
  sfron_xattn_fwd      per element 2^-8 |O_ref| + (2^-8 + 1e-3) max|V|: the output's bf16 rounding, bf16 probabilities (each within 2^-9
                       relative; a convex combination of V moves by at most 2^-8 max|V|), and the 1e-3 softmax row-sum allowance of
                       tests/test_gpu_large_shapes.py for __expf / the normalisation.  A restatement with bf16-rounded P is checked against
                       the same bound on the CPU first.
  stub-model sampler   x and pred_x0 within 4 fp32 ulp (4 * 2^-23) of the step's largest term: for x_prev the largest of |sqrt(a_prev) pred_x0|,
                       |dir e| and |sigma noise|, for pred_x0 the larger of |x| / sqrt(a_t) and sqrt(1 - a_t) |e| / sqrt(a_t), rebuilt in fp64
                       from the fixture's x_prev and pred_x0 of the step; decode / stochastic_encode: half of max|result| (a sum's larger
                       term is at least that).
  tiny UNet            per step ||x_prev - ref|| <= (|1 - g| + g) 1.5e-2 |c_k| ||eps_ref,k|| + 1e-6 ||ref||, c_k = dir_k - sqrt(a_prev,k)
                       sqrt(1 - a_k) / sqrt(a_k): the project's single-forward tolerance (rel-L2 1.5e-2 per UNet output, both halves of the
                       guided mix) pushed through the update; free-running: the sum of the per-step bounds.
"""
import csv
import os
import types

import numpy as np
import pytest
import torch

from test_ddim_cpu import G  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_UNSUPPORTED = 1002


def _L():
    from sfron import _lib
    return _lib.lib()


def _rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ------------------------------------------------------------------------------------------------ sfron_ddim_cfg_step
def _step_ref(x, eu, ec, nz, g, s1, s2, s3, dr, sg):
    x, eu = x.double(), eu.double()
    e = eu if ec is None else eu + g * (ec.double() - eu)
    pred = (x - s1 * e) / s2
    xp = s3 * pred + dr * e
    if nz is not None:
        xp = xp + sg * nz.double()
    return xp, pred


@pytest.mark.parametrize("guidance", [1.0, 7.5])
@pytest.mark.parametrize("n", [1, 255, 4 * 8 * 8 * 2, 1000003])
def test_ddim_cfg_step_vs_fp64(n, guidance):
    from sfron._lib import ptr, stream_ptr
    g = torch.Generator().manual_seed(n)
    x, eu, ec, nz = (torch.randn(n, generator=g).to(DEV) for _ in range(4))
    f = lambda v: float(np.float32(v))
    s1, s2, s3, dr, sg = f(0.6 ** 0.5), f(0.4 ** 0.5), f(0.55 ** 0.5), f((1 - 0.55 - 0.04) ** 0.5), f(0.2)
    emax = torch.maximum(eu.abs(), ec.abs()).double()
    variants = [("all", ec, nz, True, False), ("no_cond", None, nz, True, False), ("no_noise", ec, None, True, False),
                ("no_pred", ec, nz, False, False), ("in_place", ec, nz, True, True)]
    for name, c, z, want_pred, in_place in variants:
        sigma = sg if z is not None else 0.0
        xin = x.clone()
        xp = xin if in_place else torch.full_like(x, float("nan"))
        pred = torch.full_like(x, float("nan")) if want_pred else None
        st = _L().sfron_ddim_cfg_step(ptr(xin), ptr(eu), ptr(c), ptr(z), n, guidance, s1, s2, s3, dr, sigma, ptr(xp), ptr(pred), stream_ptr())
        assert st == 0, (name, st)
        rx, rp = _step_ref(x, eu, c, z, guidance, s1, s2, s3, dr, sigma)
        em = emax if c is not None else eu.abs().double()
        gg = guidance if c is not None else 0.0
        noise_term = sigma * z.abs().double() if z is not None else 0.0
        bx = 8 * 2.0 ** -24 * (x.abs().double() / s2 * s3 + (1 + 2 * gg) * em * (s1 * s3 / s2 + dr) + noise_term)
        bp = 8 * 2.0 ** -24 * (x.abs().double() / s2 + (1 + 2 * gg) * em * (s1 / s2))
        ex = (xp.double() - rx).abs()
        print(f"ddim_cfg_step n={n} g={guidance} {name}: worst err / bound {float((ex / bx).max()):.3f}")
        assert bool((ex <= bx).all()), (name, float((ex / bx).max()))
        if want_pred:
            assert bool(((pred.double() - rp).abs() <= bp).all()), name
        if not in_place:
            assert torch.equal(xin, x)
    # sigma != 0 without noise, and a zero sqrt(a_t), are argument errors
    assert _L().sfron_ddim_cfg_step(ptr(x), ptr(eu), None, None, n, 1.0, s1, s2, s3, dr, 0.5, ptr(x.clone()), None, stream_ptr()) == 1001
    assert _L().sfron_ddim_cfg_step(ptr(x), ptr(eu), None, None, n, 1.0, s1, 0.0, s3, dr, 0.0, ptr(x.clone()), None, stream_ptr()) == 1001


# ------------------------------------------------------------------------------------------------ sfron_xattn_fwd
XATTN_CASES = [(2, 2, 64, 40, 77, 80), (1, 2, 128, 80, 77, 80), (1, 1, 64, 160, 77, 80), (1, 2, 16, 40, 5, 8), (1, 1, 80, 80, 128, 128),
               (1, 1, 1, 40, 1, 8), (2, 8, 200, 40, 77, 80)]
POISON = 3.0e4          # large and finite: what the padded key / value rows hold


def _xattn_inputs(B, H, N, hd, Lv, Lk, seed):
    g = torch.Generator().manual_seed(seed)
    C = H * hd
    q = (torch.randn(B * N, C, generator=g) * 1.5).to(torch.bfloat16)
    kv = (torch.randn(B, Lk, 2 * C, generator=g) * 1.2).to(torch.bfloat16)           # k = columns 0 .. C-1, v = C .. 2C-1: ldk = ldv = 2C
    kv[:, Lv:] = POISON
    return q, kv.reshape(B * Lk, 2 * C)


def _xattn_ref(q, kv, B, H, N, hd, Lv, Lk, p_bf16=False):
    C = H * hd
    qd = q.double().view(B, N, H, hd).permute(0, 2, 1, 3)
    k = kv.double().view(B, Lk, 2, H, hd)[:, :Lv, 0].permute(0, 2, 1, 3)
    v = kv.double().view(B, Lk, 2, H, hd)[:, :Lv, 1].permute(0, 2, 1, 3)
    p = torch.softmax(qd @ k.transpose(-1, -2) * hd ** -0.5, -1)
    if p_bf16:
        p = p.to(torch.bfloat16).double()
    o = (p @ v).permute(0, 2, 1, 3).reshape(B * N, C)
    vmax = v.abs().amax(dim=(2, 3))                                                     # [B][H]: max |V| of the head
    return o, vmax[:, None, :, None].expand(B, N, H, hd).reshape(B * N, C)


def _xattn_bound(o_ref, vmax):
    return 2.0 ** -8 * o_ref.abs() + (2.0 ** -8 + 1e-3) * vmax


@pytest.mark.parametrize("B,H,N,hd,Lv,Lk", XATTN_CASES)
def test_xattn_fwd_vs_fp64(B, H, N, hd, Lv, Lk):
    q, kv = _xattn_inputs(B, H, N, hd, Lv, Lk, seed=N + hd + Lv)
    C = H * hd
    o_ref, vmax = _xattn_ref(q, kv, B, H, N, hd, Lv, Lk)
    bound = _xattn_bound(o_ref, vmax)
    o_p, _ = _xattn_ref(q, kv, B, H, N, hd, Lv, Lk, p_bf16=True)                       # the CPU check of the bound itself
    assert bool(((o_p.to(torch.bfloat16).double() - o_ref).abs() <= bound).all())
    qd, kvd = q.to(DEV), kv.to(DEV)
    TAIL = 7                                                                           # rows past N: never stored
    o = torch.full((B * N + TAIL, C), 77.0, dtype=torch.bfloat16, device=DEV)
    st = _L().sfron_xattn_fwd(qd.data_ptr(), C, kvd.data_ptr(), 2 * C, kvd.data_ptr() + 2 * C, 2 * C, o.data_ptr(), C, B, N, Lk, Lv, H, hd,
                              float(hd ** -0.5), torch.cuda.current_stream().cuda_stream)
    assert st == 0, st
    torch.cuda.synchronize()
    got = o[:B * N].double().cpu()
    assert bool(torch.isfinite(got).all())
    err = (got - o_ref).abs()
    print(f"xattn B={B} H={H} N={N} hd={hd} Lv={Lv} Lk={Lk}: worst err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    assert bool((o[B * N:] == 77.0).all())
    # a wider output row (ldo > C) leaves the columns beside it alone
    o2 = torch.full((B * N, C + 8), 77.0, dtype=torch.bfloat16, device=DEV)
    assert _L().sfron_xattn_fwd(qd.data_ptr(), C, kvd.data_ptr(), 2 * C, kvd.data_ptr() + 2 * C, 2 * C, o2.data_ptr(), C + 8, B, N, Lk, Lv, H, hd,
                                float(hd ** -0.5), torch.cuda.current_stream().cuda_stream) == 0
    assert torch.equal(o2[:, :C], o[:B * N]) and bool((o2[:, C:] == 77.0).all())


def test_xattn_fwd_refuses_what_it_does_not_take():
    t = torch.zeros(256, 2 * 1280, dtype=torch.bfloat16, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    call = lambda hd, Lk, Lv=5, H=2: _L().sfron_xattn_fwd(t.data_ptr(), H * hd, t.data_ptr(), H * hd, t.data_ptr(), H * hd, t.data_ptr(), H * hd,
                                                           1, 16, Lk, Lv, H, hd, 0.1, s)
    assert call(64, 80) == ERR_UNSUPPORTED
    assert call(40, 136) == ERR_UNSUPPORTED
    assert call(40, 77) == ERR_UNSUPPORTED
    assert call(40, 80, Lv=81) == 1001 and call(40, 80, Lv=0) == 1001
    assert call(40, 80) == 0


# ------------------------------------------------------------------------------------------------ UNet inference path
INFER = dict(in_channels=4, out_channels=4, model_channels=320, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=(1, 2), num_heads=8,
             context_dim=64)


@pytest.fixture(scope="module")
def infer():
    from test_gpu_sd import _pair
    ref, model = _pair(INFER, seed=77)
    g = torch.Generator().manual_seed(78)
    x, t, ctx = torch.randn(2, 4, 8, 8, generator=g), torch.tensor([37, 801]), torch.randn(2, 77, 64, generator=g)
    with torch.no_grad():
        want = ref(x, timesteps=t, context=ctx)
    xd, td, cd = x.to(DEV), t.to(DEV), ctx.to(DEV)
    model.eval()
    with torch.no_grad():
        plain = model(xd, timesteps=td, context=cd).clone()
    return types.SimpleNamespace(model=model, x=xd, t=td, ctx=cd, want=want, plain=plain)


def test_prepared_context_is_bit_identical_to_the_plain_forward(infer):
    m = infer.model
    assert m.fused_cross_attention is False
    with torch.no_grad():
        pc = m.prepare_context(infer.ctx)
        assert sorted(pc.kv) == sorted(n for n, _ in m.st_blocks) and pc.Lp == 80 and pc.Lv == 77
        out = m(infer.x, timesteps=infer.t, context=pc)
        again = m(infer.x, timesteps=infer.t, context=pc)
    assert torch.equal(out, infer.plain) and torch.equal(again, infer.plain)
    assert _rel(out, infer.want) < 1.5e-2


def test_fused_cross_attention_matches_the_oracle(infer):
    m = infer.model
    m.fused_cross_attention = True
    try:
        with torch.no_grad():
            out = m(infer.x, timesteps=infer.t, context=infer.ctx)
            out_pc = m(infer.x, timesteps=infer.t, context=m.prepare_context(infer.ctx))
    finally:
        m.fused_cross_attention = False
    e = _rel(out, infer.want)
    print(f"fused cross-attention forward vs oracle: rel-L2 {e:.3e} (plain forward {_rel(infer.plain, infer.want):.3e})")
    assert e < 1.5e-2, e
    assert torch.equal(out, out_pc)
    assert not torch.equal(out, infer.plain)            # the fused kernel really ran (hd 40 and 80 are both supported)


def test_prepared_context_guards(infer):
    m = infer.model
    with pytest.raises(AssertionError):
        m.prepare_context(infer.ctx)                    # grad mode
    with torch.no_grad():
        pc = m.prepare_context(infer.ctx)
        with pytest.raises(AssertionError):
            m(infer.x[:1], timesteps=infer.t[:1], context=pc)           # another batch size
    with pytest.raises(AssertionError):
        m(infer.x, timesteps=infer.t, context=pc)       # grad mode


def test_nothing_is_cached_across_calls(infer):
    m = infer.model
    m.fused_cross_attention = True                      # the flag does nothing where grad is enabled
    try:
        m.train()
        out = m(infer.x, timesteps=infer.t, context=infer.ctx)
        out.sum().backward()
        m.eval()
    finally:
        m.fused_cross_attention = False
    assert _rel(out, infer.want) < 1.5e-2
    with torch.no_grad():
        assert torch.equal(m(infer.x, timesteps=infer.t, context=infer.ctx), infer.plain)
        assert torch.equal(m(infer.x, timesteps=infer.t, context=m.prepare_context(infer.ctx)), infer.plain)


# ------------------------------------------------------------------------------------------------ sampler, analytic model
class StubLDM:
    """what DDIMSampler reads of LatentDiffusion, with the fixture's analytic denoiser (make_ddim_golden.stub_eps): the two per-sample
    scalars cos(t / 1000) and mean(c) in fp64 on the host, rounded once to fp32 (no dependence on a machine's fp32 cosine or reduction
    order); the products and sums are single IEEE fp32 operations on either device."""

    def __init__(self):
        from sfron import sd
        s = sd.LDMSchedule(device=DEV)
        self.num_timesteps, self.betas, self.alphas_cumprod, self.alphas_cumprod_prev = s.num_timesteps, s.betas, s.alphas_cumprod, s.alphas_cumprod_prev
        self.device = torch.device(DEV)

    def apply_model(self, x, t, c):
        cs = torch.cos(t.cpu().double() / 1000).float().view(-1, 1, 1, 1).to(DEV)
        m = c.cpu().double().mean(dim=(1, 2)).float().view(-1, 1, 1, 1).to(DEV)
        return 0.3 * x * cs + 0.1 * m


STUB_CASES = {"plain": dict(S=10, eta=0.0, unconditional_guidance_scale=1.0, log_every_t=1),
              "guided": dict(S=10, eta=0.0, unconditional_guidance_scale=7.5, log_every_t=3),
              "eta": dict(S=10, eta=0.5, unconditional_guidance_scale=3.0, log_every_t=1),
              "partial": dict(S=10, eta=0.0, unconditional_guidance_scale=3.0, log_every_t=1, t_start=6, till_T=2)}
ULP4 = 4 * 2.0 ** -23


def _logged_indices(kw):
    total = len(range(10)[:kw.get("t_start", -1)])
    out = []
    for i in range(total):
        index = total - i - 1
        if index % kw["log_every_t"] == 0 or index == total - 1:
            out.append(index)
        if index + 1 == (kw.get("till_T") or 0):
            break
    return out


@pytest.mark.parametrize("case", sorted(STUB_CASES))
def test_sampler_with_the_analytic_model(G, case):  # noqa: F811
    from sfron import ddim
    kw = STUB_CASES[case]
    x_T, cond, uc, sn = (torch.from_numpy(G["stub/" + n]).to(DEV) for n in ("x_T", "cond", "uc", "step_noise"))
    s = ddim.DDIMSampler(StubLDM())
    smp, inter = s.sample(batch_size=2, shape=(4, 8, 8), conditioning=cond, unconditional_conditioning=uc, x_T=x_T, step_noise=sn, verbose=False, **kw)
    pre = f"sched/10_{kw['eta']}_uniform/" if kw["eta"] else None
    if pre:
        assert np.array_equal(s.ddim_timesteps, G[pre + "timesteps"])
        assert np.array_equal(np.asarray(s.ddim_sigmas, dtype=np.float32), G[pre + "sigmas"].astype(np.float32))
        assert np.array_equal(s.ddim_alphas.numpy(), G[pre + "alphas"])
    want_x, want_p = G[f"stub/{case}/x_inter"], G[f"stub/{case}/pred_x0"]
    idx = _logged_indices(kw)
    assert len(inter["x_inter"]) == len(want_x) == len(idx) + 1 and len(inter["pred_x0"]) == len(want_p)
    assert torch.equal(inter["x_inter"][0], x_T) and torch.equal(inter["pred_x0"][0], x_T)
    worst, total = 0.0, len(range(10)[:kw.get("t_start", -1)])
    for j, index in enumerate(idx, start=1):
        # the step's terms, rebuilt in fp64 from the fixture's own x_prev and pred_x0 of that step:
        #   x_prev = s3 pred + dir e + sigma noise  ->  e;   pred = x / s2 - s1 e / s2  ->  x
        s1, s2, s3, dr, sg = s.step_coefficients(index)
        pred, xprev = want_p[j].astype(np.float64), want_x[j].astype(np.float64)
        nz = sg * G["stub/step_noise"][total - 1 - index].astype(np.float64)
        e = (xprev - s3 * pred - nz) / dr
        x_in = s2 * pred + s1 * e
        tol_x = ULP4 * float(max(np.abs(s3 * pred).max(), np.abs(dr * e).max(), np.abs(nz).max()))
        tol_p = ULP4 * float(max(np.abs(x_in / s2).max(), np.abs(s1 * e / s2).max()))
        ex = float(np.abs(inter["x_inter"][j].double().cpu().numpy() - want_x[j]).max())
        ep = float(np.abs(inter["pred_x0"][j].double().cpu().numpy() - want_p[j]).max())
        worst = max(worst, ex / tol_x, ep / tol_p)
        assert ex <= tol_x and ep <= tol_p, (case, index, ex, tol_x, ep, tol_p)
    print(f"stub sampler {case}: worst error / tolerance {worst:.3f} over {len(idx)} logged steps")
    assert torch.equal(smp, inter["x_inter"][-1])


def test_decode_and_stochastic_encode_with_the_analytic_model(G):  # noqa: F811
    from sfron import ddim
    x_T, cond, uc, sn = (torch.from_numpy(G["stub/" + n]).to(DEV) for n in ("x_T", "cond", "uc", "step_noise"))
    s = ddim.DDIMSampler(StubLDM())
    s.make_schedule(10, ddim_eta=0.0, verbose=False)
    got = s.decode(x_T, cond, 5, unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
    want = G["stub/decode"]
    assert float(np.abs(got.double().cpu().numpy() - want).max()) <= ULP4 * 0.5 * float(np.abs(want).max())     # a sum's larger term >= half of it
    enc = s.stochastic_encode(x_T, torch.from_numpy(G["stub/encode_t"]).to(DEV), noise=sn[0])
    want = G["stub/stochastic_encode"]
    assert float(np.abs(enc.double().cpu().numpy() - want).max()) <= ULP4 * 0.5 * float(np.abs(want).max())


# ------------------------------------------------------------------------------------------------ sampler, tiny UNet
@pytest.fixture(scope="module")
def tiny_ldm():
    from test_gpu_reference_fixtures import _sd_from_fixture
    from sfron import sd
    model, _ = _sd_from_fixture()
    model.eval()
    return sd.LatentDiffusion(model)


def _unet_bounds(G, s, g=3.0):  # noqa: F811
    out = []
    for k in range(8):
        index = 7 - k
        s1, s2, s3, dr, _ = s.step_coefficients(index)
        ck = abs(dr - s3 * s1 / s2)
        out.append((abs(1 - g) + g) * 1.5e-2 * ck * float(np.linalg.norm(G["unet/eps"][k].astype(np.float64))))
    return out


def test_sampler_teacher_forced_on_the_tiny_unet(G, tiny_ldm):  # noqa: F811
    from sfron import ddim
    s = ddim.DDIMSampler(tiny_ldm)
    s.make_schedule(8, ddim_eta=0.0, verbose=False)
    cond, uc = torch.from_numpy(G["unet/cond"]).to(DEV), torch.from_numpy(G["unet/uc"]).to(DEV)
    bounds = _unet_bounds(G, s)
    for k in range(8):
        index = 7 - k
        x = torch.from_numpy(G["unet/x_inter"][k]).to(DEV)
        ts = torch.full((2,), int(s.ddim_timesteps[index]), device=DEV, dtype=torch.long)
        x_prev, pred = s.p_sample_ddim(x, cond, ts, index=index, unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
        ref = G["unet/x_inter"][k + 1].astype(np.float64)
        err = float(np.linalg.norm(x_prev.double().cpu().numpy() - ref))
        tol = bounds[k] + 1e-6 * float(np.linalg.norm(ref))
        print(f"teacher-forced step {k} (index {index}): ||x_prev - ref|| {err:.3e}, bound {tol:.3e}, pred_x0 rel-L2 {_rel(pred, G['unet/pred_x0'][k + 1]):.3e}")
        assert err <= tol, (k, err, tol)


def test_sampler_free_running_on_the_tiny_unet(G, tiny_ldm):  # noqa: F811
    """Measured on MI355X: final latent rel-L2 5.42e-3, ||diff|| 0.974 against 2.579 for the sum of the eight step bounds."""
    from sfron import ddim
    s = ddim.DDIMSampler(tiny_ldm)
    cond, uc, x_T = (torch.from_numpy(G["unet/" + n]).to(DEV) for n in ("cond", "uc", "x_T"))
    unet = tiny_ldm.model.diffusion_model
    smp, inter = s.sample(S=8, batch_size=2, shape=(4, 8, 8), conditioning=cond, unconditional_conditioning=uc, x_T=x_T, eta=0.0,
                          unconditional_guidance_scale=3.0, log_every_t=1, t_start=8, verbose=False)
    assert unet.fused_cross_attention is False          # set for the call only
    assert len(inter["x_inter"]) == 9
    ref = G["unet/samples"].astype(np.float64)
    err = float(np.linalg.norm(smp.double().cpu().numpy() - ref))
    total = sum(_unet_bounds(G, s))
    print(f"free-running 8 steps: final latent rel-L2 {err / np.linalg.norm(ref):.3e}; ||diff|| {err:.3e}, sum of the step bounds {total:.3e}")
    assert err <= total, (err, total)
    # a chunked run (one sample per chunk) is the same computation per sample
    s.chunk_size = lambda batch_size, shape: 1
    smp1, inter1 = s.sample(S=8, batch_size=2, shape=(4, 8, 8), conditioning=cond, unconditional_conditioning=uc, x_T=x_T, eta=0.0,
                            unconditional_guidance_scale=3.0, log_every_t=1, t_start=8, verbose=False)
    assert len(inter1["x_inter"]) == 9 and inter1["x_inter"][3].shape == (2, 4, 8, 8)
    assert float(np.linalg.norm(smp1.double().cpu().numpy() - ref)) <= total


# ------------------------------------------------------------------------------------------------ prompt to image
def test_generate_images_end_to_end(golden_dir, tmp_path):
    from test_gpu_sd import SMALL, _pair
    from test_gpu_text_encoder import fixture_encoder
    from test_gpu_vae_decoder import small_decoder
    from sfron import sd
    tfx = dict(np.load(os.path.join(golden_dir, "text_encoder.npz")))
    dfx = dict(np.load(os.path.join(golden_dir, "vae_decoder.npz")))
    enc = fixture_encoder(tfx, str(tmp_path))
    _, unet = _pair(dict(SMALL, context_dim=enc.D), seed=5)
    unet.eval()
    ldm = sd.LatentDiffusion(unet, first_stage_decoder=small_decoder(dfx), cond_stage_model=enc)
    p = tmp_path / "prompts.csv"
    with open(p, "w", newline="") as f:
        w = csv.writer(f)
        w.writerows([["case_number", "prompt", "evaluation_seed"], [0, "a photo of a nude person", 3], [4, "a photo of a person wearing clothes", 9]])
    runs = []
    for d in ("a", "b"):
        out = sd.generate_images(ldm, str(p), str(tmp_path / d), guidance_scale=7.5, image_size=64, ddim_steps=4, num_samples=2, rounds=1)
        assert [os.path.basename(x) for x in out] == ["0_0.png", "0_1.png", "4_0.png", "4_1.png"]
        runs.append([open(x, "rb").read() for x in out])
    from PIL import Image
    im = Image.open(out[0])
    f = ldm.first_stage_decoder.factor
    assert im.size == (8 * f, 8 * f) and im.mode == "RGB"
    assert runs[0] == runs[1]                           # deterministic for a fixed seed: byte-identical files
    assert runs[0][0] != runs[0][1] and runs[0][0] != runs[0][2]
