"""GPU: the ldm PLMS sampler of SD v1 -- the two kernels it adds (sfron_plms_cfg_step, sfron_inpaint_blend), sfron.plms.PLMSSampler against
the reference's trajectories (tests/golden/plms.npz, made by tests/golden/make_plms_golden.py from SD/ldm/models/diffusion/plms.py) and
generate_images with the sampler swapped in.

Yardsticks (none is what the kernels give):
  kernels              equal as fp32 values (torch.equal) to the reference's recorded step (teacher-forced on the fixture, with the step
                       scalars the fixture records), and to the same formula evaluated by torch on the CPU in the reference's left-to-right
                       order (all forms).  Every operation of the two kernels is one IEEE fp32 operation (the library is built with
                       -ffp-contract=off), as it is in torch on the CPU.
  stub-model sampler   x and pred_x0 within 4 fp32 ulp (4 * 2^-23) of the step's largest term, the rule of tests/test_gpu_ddim.py with
                       sigma = 0: for x_prev the larger of |sqrt(a_prev) pred_x0| and |dir e'|, for pred_x0 the larger of |x| / sqrt(a_t) and
                       sqrt(1 - a_t) |e'| / sqrt(a_t), rebuilt in fp64 from the fixture's x_prev and pred_x0 of the step.
  tiny UNet            per step ||x_prev - ref|| <= (|1 - g| + g) 1.5e-2 |c_k| sum_j |w_j| ||eps_ref,j|| + 1e-6 ||ref||: the bound of
                       test_gpu_ddim._unet_bounds (its 1.5e-2 is the project's single-forward tolerance) with ||eps|| replaced by the
                       weighted norms of the step's combination (w = 1/2, 1/2 | 3/2, 1/2 | 23/12, 16/12, 5/12 | 55/24, 59/24, 37/24, 9/24);
                       free-running: the sum of the per-step bounds.
"""
import csv
import os

import numpy as np
import pytest
import torch

from test_ddim_cpu import host_model
from test_plms_cpu import P  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = 1001
O1, O2, O3, O4, MEAN = range(5)
MAX_THREADS = 4096 * 256                # the capped grid of csrc/plms.hip: one more element than this takes a second trip of the loop
WEIGHTS = {O1: (1.0,), MEAN: (0.5, 0.5), O2: (1.5, 0.5), O3: (23 / 12, 16 / 12, 5 / 12), O4: (55 / 24, 59 / 24, 37 / 24, 9 / 24)}


def _L():
    from sfron import _lib
    return _lib.lib()


def _launch(x, eu, ec, old, order, g, coef, e_out, x_prev, pred, n=None):
    from sfron._lib import ptr, stream_ptr
    o = list(old) + [None] * (3 - len(old))
    s1, s2, s3, dr = coef[:4]
    return _L().sfron_plms_cfg_step(ptr(x), ptr(eu), ptr(ec), ptr(o[0]), ptr(o[1]), ptr(o[2]), order, x.numel() if n is None else n, g, s1, s2, s3,
                                    dr, ptr(e_out), ptr(x_prev), ptr(pred), stream_ptr())


def _blend(img, x0, nz, mask, B, C, hw, mb, mc, sa, sb, out):
    from sfron._lib import ptr, stream_ptr
    return _L().sfron_inpaint_blend(ptr(img), ptr(x0), ptr(nz), ptr(mask), B, C, hw, mb, mc, sa, sb, ptr(out), stream_ptr())


def _step_ref(x, eu, ec, old, order, g, coef):
    """plms.py:311-312, 349-380 by torch on the CPU, fp32, the reference's expressions -> (e, x_prev, pred_x0)"""
    s1, s2, s3, dr = (torch.tensor(v, dtype=torch.float32) for v in coef[:4])
    e = eu if ec is None else eu + g * (ec - eu)
    if order == O1:
        ep = e
    elif order == O2:
        ep = (3 * e - old[0]) / 2
    elif order == O3:
        ep = (23 * e - 16 * old[0] + 5 * old[1]) / 12
    elif order == O4:
        ep = (55 * e - 59 * old[0] + 37 * old[1] - 9 * old[2]) / 24
    else:
        ep = (old[0] + e) / 2
    pred = (x - s1 * ep) / s2
    return e, s3 * pred + dr * ep, pred


def _blend_ref(img, x0, nz, mask, sa, sb):
    sa, sb = torch.tensor(sa, dtype=torch.float32), torch.tensor(sb, dtype=torch.float32)
    orig = sa * x0 + sb * nz
    return orig * mask + (1.0 - mask) * img


def _sampler(S, discr="uniform"):
    """a host-side sampler: the step scalars of a schedule"""
    from sfron import plms
    s = plms.PLMSSampler(host_model())
    s.make_schedule(S, ddim_discretize=discr, verbose=False)
    return s


def _tables():
    from sfron import sd
    tab = sd.LDMSchedule(device="cpu").tab
    return tab[:, 0].clone(), tab[:, 1].clone()


# ------------------------------------------------------------------------------------------------ kernels, teacher-forced on the fixture
@pytest.mark.parametrize("case,g", [("guided", 7.5), ("inpaint", 3.0)])
def test_kernels_teacher_forced_on_the_reference(P, case, g):  # noqa: F811
    pre = f"stub/{case}/"
    s = _sampler(10)
    COEF = P["sched/10_uniform/step_coef"]             # the reference's own four scalars of every step
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    X, OUT, HIST, HL = P[pre + "step_x"], P[pre + "step_out"], P[pre + "step_hist"], P[pre + "step_hist_len"]
    E, XP, PR = P[pre + "step_e_t"], P[pre + "step_x_prev"], P[pre + "step_pred_x0"]
    sa_tab, sb_tab = _tables()
    for k in range(10):
        index = 9 - k
        coef = tuple(float(v) for v in COEF[index])
        x = d(X[k])
        if case == "inpaint":              # the blend in front of the step: img is the step before's x_prev (x_T at the start)
            img = d(P["stub/x_T"] if k == 0 else XP[k - 1])
            t = int(s.ddim_timesteps[index])
            got = torch.full_like(img, float("nan"))
            assert _blend(img, d(P["stub/x0"]), d(P["stub/inpaint_noise"][k]), d(P["stub/mask"]), 2, 4, 64, 2, 1, float(sa_tab[t]), float(sb_tab[t]),
                          got) == 0
            assert torch.equal(got.cpu(), torch.from_numpy(X[k])), (case, k, "blend")
        call = 0 if k == 0 else k + 1
        out = d(OUT[call])
        e_out, x_prev, pred = (torch.full_like(x, float("nan")) for _ in range(3))
        if k == 0:
            assert HL[0] == 0
            assert _launch(x, out[:2], out[2:], [], O1, g, coef, e_out, x_prev, None) == 0
            assert torch.equal(e_out.cpu(), torch.from_numpy(E[0])), (case, "e_t of the first step")
            assert torch.equal(x_prev.cpu(), torch.from_numpy(P[pre + "x_mid"])), (case, "x_mid")
            out = d(OUT[1])
            assert _launch(x, out[:2], out[2:], [e_out], MEAN, g, coef, None, x_prev, pred) == 0
        else:
            old = [d(HIST[k, j]) for j in range(int(HL[k]))]
            assert _launch(x, out[:2], out[2:], old, (O2, O3, O4)[int(HL[k]) - 1], g, coef, e_out, x_prev, pred) == 0
            assert torch.equal(e_out.cpu(), torch.from_numpy(E[k])), (case, k, "e_t")
        assert torch.equal(x_prev.cpu(), torch.from_numpy(XP[k])), (case, k, "x_prev")
        assert torch.equal(pred.cpu(), torch.from_numpy(PR[k])), (case, k, "pred_x0")


# ------------------------------------------------------------------------------------------------ kernels, all forms
@pytest.mark.parametrize("guidance", [None, 7.5])
@pytest.mark.parametrize("n", [1, 255, 257, MAX_THREADS + 257])
@pytest.mark.parametrize("order", [O1, O2, O3, O4, MEAN])
def test_plms_cfg_step_equals_torch_on_the_cpu(order, n, guidance):
    gen = torch.Generator().manual_seed(1000 * order + n % 997)
    x, eu, ec, h1, h2, h3 = (torch.randn(n, generator=gen) for _ in range(6))
    if guidance is None:
        ec = None
    f = lambda v: float(np.float32(v))
    coef = (f(0.6 ** 0.5), f(0.4 ** 0.5), f(0.55 ** 0.5), f(0.45 ** 0.5))
    nold = {O1: 0, O2: 1, O3: 2, O4: 3, MEAN: 1}[order]
    old = [h1, h2, h3][:nold]
    g = 1.0 if guidance is None else guidance
    we, wx, wp = _step_ref(x, eu, ec, old, order, g, coef)
    d = lambda v: None if v is None else v.to(DEV)
    xd, eud, ecd, oldd = d(x), d(eu), d(ec), [d(v) for v in old]
    e_out, x_prev, pred = (torch.full((n + 3,), 77.0, device=DEV) for _ in range(3))     # three guard elements past n
    assert _launch(xd, eud, ecd, oldd, order, g, coef, e_out, x_prev, pred, n=n) == 0
    assert torch.equal(e_out[:n].cpu(), we) and torch.equal(x_prev[:n].cpu(), wx) and torch.equal(pred[:n].cpu(), wp)
    assert all(bool((t[n:] == 77.0).all()) for t in (e_out, x_prev, pred))
    assert torch.equal(xd.cpu(), x) and all(torch.equal(a.cpu(), b) for a, b in zip(oldd, old))       # inputs untouched
    # pred_x0 and e_out NULL
    x_prev2 = torch.full_like(xd, 77.0)
    assert _launch(xd, eud, ecd, oldd, order, g, coef, None, x_prev2, None) == 0
    assert torch.equal(x_prev2.cpu(), wx)
    # x_prev == x
    xin = xd.clone()
    assert _launch(xin, eud, ecd, oldd, order, g, coef, None, xin, pred) == 0
    assert torch.equal(xin.cpu(), wx) and torch.equal(pred[:n].cpu(), wp)
    # e_out == the oldest history buffer the call reads (the ring overwritten in place)
    if nold:
        ring = [v.clone() for v in oldd]
        x_prev3 = torch.full_like(xd, 77.0)
        assert _launch(xd, eud, ecd, ring, order, g, coef, ring[-1], x_prev3, None) == 0
        assert torch.equal(x_prev3.cpu(), wx) and torch.equal(ring[-1].cpu(), we)
        assert all(torch.equal(a, b) for a, b in zip(ring[:-1], oldd[:-1]))


@pytest.mark.parametrize("mb,mc", [(1, 1), (1, 3), (2, 1), (2, 3)])
def test_inpaint_blend_equals_torch_on_the_cpu(mb, mc):
    B, C, H, W = 2, 3, 5, 7                                                            # hw = 35: odd, no multiple of anything
    gen = torch.Generator().manual_seed(10 * mb + mc)
    img, x0, nz = (torch.randn(B, C, H, W, generator=gen) for _ in range(3))
    mask = torch.rand(mb, mc, H, W, generator=gen)
    mask[..., 0, :] = 0.0
    mask[..., 1, :] = 1.0                                                              # soft values and the two hard ones
    sa, sb = float(np.float32(0.8 ** 0.5)), float(np.float32(0.2 ** 0.5))
    want = _blend_ref(img, x0, nz, mask, sa, sb)
    imgd, x0d, nzd, md = (v.to(DEV) for v in (img, x0, nz, mask))
    out = torch.full((B * C * H * W + 3,), 77.0, device=DEV)
    assert _blend(imgd, x0d, nzd, md, B, C, H * W, mb, mc, sa, sb, out) == 0
    assert torch.equal(out[:-3].cpu().view(B, C, H, W), want) and bool((out[-3:] == 77.0).all())
    assert torch.equal(imgd.cpu(), img)
    assert _blend(imgd, x0d, nzd, md, B, C, H * W, mb, mc, sa, sb, imgd) == 0          # out == img
    assert torch.equal(imgd.cpu(), want)


def test_inpaint_blend_takes_a_second_trip_of_the_grid():
    B, C, hw = 2, 4, MAX_THREADS // 8 + 3                                              # 24 elements more than the capped grid has threads
    gen = torch.Generator().manual_seed(5)
    img, x0, nz = (torch.randn(B, C, hw, generator=gen) for _ in range(3))
    mask = (torch.rand(B, 1, hw, generator=gen) < 0.5).float()
    want = _blend_ref(img, x0, nz, mask, 0.75, 0.5)
    out = torch.full((B, C, hw), 77.0, device=DEV)
    assert _blend(img.to(DEV), x0.to(DEV), nz.to(DEV), mask.to(DEV), B, C, hw, B, 1, 0.75, 0.5, out) == 0
    assert torch.equal(out.cpu(), want)


def test_refusals_leave_the_outputs_alone():
    n = 64
    x, eu, ec, h1, h2, h3 = (torch.randn(n, device=DEV) for _ in range(6))
    coef = (0.5, 0.75, 0.25, 0.5)
    outs = [torch.full((n,), 77.0, device=DEV) for _ in range(3)]
    ok = dict(x=x, eu=eu, ec=ec, old=[h1, h2, h3], order=O4, g=7.5, coef=coef, n=n)

    def call(**kw):
        a = dict(ok, **kw)
        x_prev = a.pop("x_prev", outs[1])
        return _launch(a["x"], a["eu"], a["ec"], a["old"], a["order"], a["g"], a["coef"], outs[0], x_prev, outs[2], n=a["n"])
    bad = [dict(x=None), dict(eu=None), dict(x_prev=None), dict(n=0), dict(n=-5), dict(coef=(0.5, 0.0, 0.25, 0.5)), dict(order=5), dict(order=-1),
           dict(order=O2, old=[]), dict(order=MEAN, old=[]), dict(order=O3, old=[h1]), dict(order=O3, old=[None, h2]), dict(order=O4, old=[h1, h2]),
           dict(order=O4, old=[None, h2, h3]), dict(g=float("nan")), dict(g=float("inf")), dict(g=float("-inf"))]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    B, C, hw = 2, 3, 8
    img, x0, nz, out = (torch.full((B, C, hw), 77.0, device=DEV) for _ in range(4))
    mask = torch.ones(B, C, hw, device=DEV)
    okb = dict(img=img, x0=x0, nz=nz, mask=mask, B=B, C=C, hw=hw, mb=B, mc=C)
    for kw in (dict(img=None), dict(x0=None), dict(nz=None), dict(mask=None), dict(out=None), dict(B=0), dict(C=-1), dict(hw=0), dict(mb=3), dict(mb=0),
               dict(mc=2), dict(mc=0), dict(mc=4)):
        a = dict(okb, **kw)
        o = a.pop("out", out)
        assert _blend(a["img"], a["x0"], a["nz"], a["mask"], a["B"], a["C"], a["hw"], a["mb"], a["mc"], 0.5, 0.5, o) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert all(bool((t == 77.0).all()) for t in outs + [out])
    assert call() == 0 and _blend(img, x0, nz, mask, B, C, hw, B, C, 0.5, 0.5, out) == 0          # the accepted forms of the same calls
    assert not bool((outs[1] == 77.0).all())


# ------------------------------------------------------------------------------------------------ sampler, analytic model
class StubLDM:
    """what PLMSSampler reads of LatentDiffusion, with the fixture's analytic denoiser (make_ddim_golden.stub_eps): the two per-sample
    scalars cos(t / 1000) and mean(c) in fp64 on the host, rounded once to fp32; the products and sums are single IEEE fp32 operations on
    either device.  q_sample and its two tables are sd.LDMSchedule's."""

    def __init__(self):
        from sfron import sd
        s = sd.LDMSchedule(device=DEV)
        self.schedule = s
        self.num_timesteps, self.betas, self.alphas_cumprod, self.alphas_cumprod_prev = s.num_timesteps, s.betas, s.alphas_cumprod, s.alphas_cumprod_prev
        self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod = s.tab[:, 0], s.tab[:, 1]
        self.device = torch.device(DEV)
        self.calls = 0

    def q_sample(self, x_start, t, noise=None):
        return self.schedule.q_sample(x_start, t, torch.randn_like(x_start) if noise is None else noise)

    def apply_model(self, x, t, c):
        self.calls += 1
        cs = torch.cos(t.cpu().double() / 1000).float().view(-1, 1, 1, 1).to(DEV)
        m = c.cpu().double().mean(dim=(1, 2)).float().view(-1, 1, 1, 1).to(DEV)
        return 0.3 * x * cs + 0.1 * m


STUB_CASES = {"plain": dict(S=10, unconditional_guidance_scale=1.0, log_every_t=1),
              "guided": dict(S=10, unconditional_guidance_scale=7.5, log_every_t=3),
              "s1": dict(S=1, unconditional_guidance_scale=3.0, log_every_t=1),
              "s3": dict(S=3, unconditional_guidance_scale=3.0, log_every_t=1),
              "inpaint": dict(S=10, unconditional_guidance_scale=3.0, log_every_t=1)}
ULP4 = 4 * 2.0 ** -23


@pytest.mark.parametrize("case", sorted(STUB_CASES))
def test_sampler_with_the_analytic_model(P, case):  # noqa: F811
    """Measured on MI355X: worst error / tolerance 0.000 in every case (each logged tensor has the reference's bits)."""
    from sfron import plms
    kw = dict(STUB_CASES[case])
    S = kw.pop("S")
    x_T, cond, uc = (torch.from_numpy(P["stub/" + n]).to(DEV) for n in ("x_T", "cond", "uc"))
    model = StubLDM()
    s = plms.PLMSSampler(model)
    if case == "inpaint":
        kw.update(mask=torch.from_numpy(P["stub/mask"]).to(DEV), x0=torch.from_numpy(P["stub/x0"]).to(DEV),
                  inpaint_noise=torch.from_numpy(P["stub/inpaint_noise"]).to(DEV))
    if case == "s3":                       # "uniform" has no three-step table: the fixture's case is make_schedule(3, "quad") + plms_sampling
        s.make_schedule(3, ddim_discretize="quad", verbose=False)
        smp, inter = s.plms_sampling(cond, (2, 4, 8, 8), x_T=x_T, unconditional_conditioning=uc, **kw)
    else:
        smp, inter = s.sample(S=S, batch_size=2, shape=(4, 8, 8), conditioning=cond, unconditional_conditioning=uc, x_T=x_T, verbose=False, **kw)
    assert model.calls == S + 1
    pre = f"sched/{S}_{'quad' if case == 's3' else 'uniform'}/"
    assert np.array_equal(s.ddim_timesteps, P[pre + "timesteps"]) and np.array_equal(s.ddim_alphas.numpy(), P[pre + "alphas"])
    want_x, want_p = P[f"stub/{case}/x_inter"], P[f"stub/{case}/pred_x0"]
    idx = [index for index in range(S - 1, -1, -1) if index % kw["log_every_t"] == 0 or index == S - 1]
    assert len(inter["x_inter"]) == len(want_x) == len(idx) + 1 and len(inter["pred_x0"]) == len(want_p)
    assert torch.equal(inter["x_inter"][0], x_T) and torch.equal(inter["pred_x0"][0], x_T)
    worst = 0.0
    for j, index in enumerate(idx, start=1):
        # the step's terms, rebuilt in fp64 from the fixture's own x_prev and pred_x0 of that step:
        #   x_prev = s3 pred + dir e'  ->  e';   pred = x / s2 - s1 e' / s2  ->  x
        s1, s2, s3, dr, _ = s.step_coefficients(index)
        pred, xprev = want_p[j].astype(np.float64), want_x[j].astype(np.float64)
        e = (xprev - s3 * pred) / dr
        x_in = s2 * pred + s1 * e
        tol_x = ULP4 * float(max(np.abs(s3 * pred).max(), np.abs(dr * e).max()))
        tol_p = ULP4 * float(max(np.abs(x_in / s2).max(), np.abs(s1 * e / s2).max()))
        ex = float(np.abs(inter["x_inter"][j].double().cpu().numpy() - want_x[j]).max())
        ep = float(np.abs(inter["pred_x0"][j].double().cpu().numpy() - want_p[j]).max())
        worst = max(worst, ex / tol_x, ep / tol_p)
        assert ex <= tol_x and ep <= tol_p, (case, index, ex, tol_x, ep, tol_p)
    print(f"stub PLMS sampler {case}: worst error / tolerance {worst:.3f} over {len(idx)} logged steps")
    assert torch.equal(smp, inter["x_inter"][-1])


def test_blend_with_a_full_mask_is_the_models_q_sample(P):  # noqa: F811
    """the blend's q_sample half against the project's own q_sample kernel (the same two tables, the same two products and one sum)"""
    from sfron import plms
    model = StubLDM()
    s = plms.PLMSSampler(model)
    x0, nz = torch.from_numpy(P["stub/x0"]).to(DEV), torch.from_numpy(P["stub/inpaint_noise"][0]).to(DEV)
    sa, sb = _tables()
    for t in (1, 501, 999):
        got = s._blend(torch.zeros_like(x0), x0, nz, torch.ones(1, 1, 8, 8, device=DEV), float(sa[t]), float(sb[t]))
        assert torch.equal(got, model.q_sample(x0, torch.full((2,), t, device=DEV, dtype=torch.long), nz)), t


# ------------------------------------------------------------------------------------------------ sampler, tiny UNet
@pytest.fixture(scope="module")
def tiny_ldm():
    from test_gpu_reference_fixtures import _sd_from_fixture
    from sfron import sd
    model, _ = _sd_from_fixture()
    model.eval()
    return sd.LatentDiffusion(model)


def _history(k):
    """the model calls (indices into unet/eps) step k combines, newest first: step 0 keeps call 0, step k > 0 is call k + 1"""
    call = lambda j: 0 if j == 0 else j + 1
    if k == 0:
        return MEAN, [1, 0]
    return (O2, O3, O4)[min(k, 3) - 1], [call(j) for j in range(k, max(k - 4, -1), -1)]


def _unet_bounds(P, s, g=3.0):  # noqa: F811
    out = []
    for k in range(8):
        s1, s2, s3, dr, _ = s.step_coefficients(7 - k)
        ck = abs(dr - s3 * s1 / s2)
        order, calls = _history(k)
        comb = sum(w * float(np.linalg.norm(P["unet/eps"][c].astype(np.float64))) for w, c in zip(WEIGHTS[order], calls))
        out.append((abs(1 - g) + g) * 1.5e-2 * ck * comb)
    return out


def test_sampler_teacher_forced_on_the_tiny_unet(P, tiny_ldm):  # noqa: F811
    from sfron import plms
    s = plms.PLMSSampler(tiny_ldm)
    s.make_schedule(8, verbose=False)
    cond, uc = torch.from_numpy(P["unet/cond"]).to(DEV), torch.from_numpy(P["unet/uc"]).to(DEV)
    bounds = _unet_bounds(P, s)
    ts_all = [int(t) for t in np.flip(s.ddim_timesteps)]
    for k in range(8):
        index = 7 - k
        x = torch.from_numpy(P["unet/x_inter"][k]).to(DEV)
        ts = torch.full((2,), ts_all[k], device=DEV, dtype=torch.long)
        ts_next = torch.full((2,), ts_all[min(k + 1, 7)], device=DEV, dtype=torch.long)
        order, calls = _history(k)
        old = [] if k == 0 else [torch.from_numpy(P["unet/eps"][c]).to(DEV) for c in reversed(calls[1:])]       # oldest first, as old_eps is
        x_prev, pred, e_t = s.p_sample_plms(x, cond, ts, index=index, unconditional_guidance_scale=3.0, unconditional_conditioning=uc,
                                            old_eps=old, t_next=ts_next)
        ref = P["unet/x_inter"][k + 1].astype(np.float64)
        err = float(np.linalg.norm(x_prev.double().cpu().numpy() - ref))
        tol = bounds[k] + 1e-6 * float(np.linalg.norm(ref))
        rel_e = float((e_t.double().cpu() - torch.from_numpy(P["unet/eps"][calls[0] if k else 0]).double()).norm() /
                      np.linalg.norm(P["unet/eps"][calls[0] if k else 0]))
        print(f"teacher-forced PLMS step {k} (index {index}, order code {order}): ||x_prev - ref|| {err:.3e}, bound {tol:.3e}, e_t rel-L2 {rel_e:.3e}")
        assert err <= tol, (k, err, tol)
        assert all(torch.equal(o, torch.from_numpy(P["unet/eps"][c]).to(DEV)) for o, c in zip(old, reversed(calls[1:])))     # only read


def test_sampler_free_running_on_the_tiny_unet(P, tiny_ldm):  # noqa: F811
    """Measured on MI355X: final latent rel-L2 4.46e-3, ||diff|| 0.786 against 10.29 for the sum of the eight step bounds."""
    from sfron import plms
    s = plms.PLMSSampler(tiny_ldm)
    cond, uc, x_T = (torch.from_numpy(P["unet/" + n]).to(DEV) for n in ("cond", "uc", "x_T"))
    unet = tiny_ldm.model.diffusion_model
    kw = dict(S=8, batch_size=2, shape=(4, 8, 8), conditioning=cond, unconditional_conditioning=uc, x_T=x_T, eta=0.0,
              unconditional_guidance_scale=3.0, log_every_t=1, verbose=False)
    smp, inter = s.sample(**kw)
    assert unet.fused_cross_attention is False and unet.fused_wide_self_attention is False          # set for the call only
    assert len(inter["x_inter"]) == 9
    ref = P["unet/samples"].astype(np.float64)
    err = float(np.linalg.norm(smp.double().cpu().numpy() - ref))
    total = sum(_unet_bounds(P, s))
    print(f"free-running 8 PLMS steps: final latent rel-L2 {err / np.linalg.norm(ref):.3e}; ||diff|| {err:.3e}, sum of the step bounds {total:.3e}")
    assert err <= total, (err, total)
    # a chunked run (one sample per chunk) is the same computation per sample
    s.chunk_size = lambda batch_size, shape: 1
    smp1, inter1 = s.sample(**kw)
    assert len(inter1["x_inter"]) == 9 and inter1["x_inter"][3].shape == (2, 4, 8, 8)
    assert float(np.linalg.norm(smp1.double().cpu().numpy() - ref)) <= total


# ------------------------------------------------------------------------------------------------ prompt to image
def test_generate_images_with_the_plms_sampler(golden_dir, tmp_path):
    from test_gpu_sd import SMALL, _pair
    from test_gpu_text_encoder import fixture_encoder
    from test_gpu_vae_decoder import small_decoder
    from sfron import plms, sd
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
    runs = {}
    for d, sampler in (("a", plms.PLMSSampler(ldm)), ("b", plms.PLMSSampler(ldm)), ("ddim", None)):
        out = sd.generate_images(ldm, str(p), str(tmp_path / d), guidance_scale=7.5, image_size=64, ddim_steps=4, num_samples=2, rounds=1,
                                 sampler=sampler)
        assert [os.path.basename(x) for x in out] == ["0_0.png", "0_1.png", "4_0.png", "4_1.png"]
        assert sorted(os.listdir(tmp_path / d)) == ["0_0.png", "0_1.png", "4_0.png", "4_1.png"]
        runs[d] = [open(x, "rb").read() for x in out]
        assert unet.fused_cross_attention is False and unet.fused_wide_self_attention is False
    assert runs["a"] == runs["b"]                       # deterministic for a fixed seed: byte-identical files
    assert all(a != b for a, b in zip(runs["a"], runs["ddim"]))
    assert runs["a"][0] != runs["a"][1] and runs["a"][0] != runs["a"][2]
