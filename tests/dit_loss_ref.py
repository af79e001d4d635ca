"""Reference for the DiT loss, sampling-step, layout and step-guard kernels (csrc/loss.hip, the non-conditioning half of csrc/embed.hip):
plain restatements of the reference's expressions (DiT/diffusion/gaussian_diffusion.py:215-230 q_sample, :254-332 p_mean_variance,
:376-421 p_sample, :682-713 _vb_terms_bpd, :746-783 training_losses; diffusion_utils.py:10-88; DiT/models.py:258-266 the guidance mix,
:224-236 unpatchify; DDPM/functions/losses.py:22-69) and of the counting rules include/sfron.h states for the guard kernels.  Every function
takes `dtype`: float64 is the reference, float32 -- the same code on the CPU -- is the yardstick the bounds are built from (bound32 of
tests/dit_rows_ref.py).  Nothing here calls a kernel; tests/test_dit_loss_ref_cpu.py holds the float64 restatement to the oracle.

Table entries are the fp32 table widened (what is compared is the arithmetic, not the table), and grad_scale is the fp32 value the C ABI
receives, widened.

loss_inputs() builds stratified inputs for the fused loss.  Its t == 0 rows reach all three branches of the discretised likelihood and
both sides of the |x| = 0.999 threshold, and every element of them is either
  regular     |z| <= 2.5, z = inv_std (x0 - model_mean): the CDF difference is a well-conditioned fp32 number, or
  saturated   30 <= |z| <= 60: every tanh is exactly +-1 in fp32 and in float64, the probability is exactly 0 (clamped to 1e-12) or 1 and
              the var-gradient is exactly 0.0 in both.
Nothing lies in between: for 2.6 < |z| < 29 the fp32 CDF difference cancels or saturates while the float64 one does not, so fp32 has no
float64 reference there (strata() counts such elements; the CPU file asserts zero at every shape the GPU file runs).

accept_loss(got, ref64, ref32) is the acceptance function of the fused loss, shared by the CPU teeth test and the GPU test:
  d_out   bound32 per sample and per channel half (eps, var), never over the whole tensor: the eps half is 1e2 .. 1e6 times the var half
  mse/vb  |got - ref64| <= (MARGIN r + 4 * 2^-24) |ref64| per sample, r = the largest relative error of the float32 restatement among the
          rows of the same class (t == 0, t > 0)
  saturated elements' var-gradient is exactly 0.0
At t = 998 and 999 the two log-variance bounds nearly coincide (max_log - min_log, formed in fp32, keeps a few bits) and the var half's
yardstick error is a tenth to a quarter of its size: there the bound only says "finite and tiny" (1e-11 beside 1e-3 for eps)."""
import math

import torch

from dit_rows_ref import MARGIN, RECORD, _rec, bound32

T_EXTRA = (1, 2, 500, 998, 999, 37)
PLANTED = (0.9985, -0.9985, 0.9995, -0.9995, 1.0, -1.0)
WRONG = ("half256", "cubic04", "thr1", "noln2", "swap", "nodetach", "varfactor", "msechw")
LOSS_SHAPES = [(4, 5), (4, 63), (3, 341), (4, 1024), (4, 4099)]           # (C, hw)
LAYOUT_SHAPES = [(2, 4, 8, 8, 1), (2, 4, 32, 32, 2), (1, 4, 32, 32, 4), (2, 4, 64, 64, 8), (3, 8, 16, 24, 2), (1, 3, 12, 20, 4),
                 (3, 4, 256, 192, 4)]                                      # (n, C, H, W, p); the last: 589824 elements, the grid strides


def table():
    """the [T][8] fp32 schedule table of the 1000-step linear schedule (oracle.diffusion_ref.DiffusionTables.packed_fp32)"""
    from oracle import diffusion_ref as dref
    return torch.from_numpy(dref.DiffusionTables(1000).packed_fp32())


def f32_scalar(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _cols(tab, t, dtype, ndim):
    r = tab.to(dtype)[t]
    return lambda k: r[:, k].view((-1,) + (1,) * (ndim - 1))


def mean_flat(x):
    return x.reshape(x.shape[0], -1).mean(1)


# ------------------------------------------------------------------------------------------------ the fused loss
def _cdf(x, k1):
    return 0.5 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + k1 * torch.pow(x, 3))))


def dit_loss(x0, noise, out, t, tab, grad_scale, dtype, wrong=None):
    """x0 / noise [n][C][...], out [n][2 C][...], t [n] int64, tab [T][8] fp32 -> mse [n], vb [n], d_out = d(grad_scale sum_i(mse_i + vb_i))
    / d out by autograd on this expression (oracle/diffusion_ref.py:111-170 restated with a dtype; eps_hat is detached inside vb).
    `wrong` names one deliberately wrong formula (WRONG), for the teeth test only."""
    assert wrong is None or wrong in WRONG
    n, C = x0.shape[0], x0.shape[1]
    half = 1.0 / 256.0 if wrong == "half256" else 1.0 / 255.0
    k1 = 0.04 if wrong == "cubic04" else 0.044715
    thr = 1.0 if wrong == "thr1" else 0.999
    x0, noise = x0.to(dtype), noise.to(dtype)
    o = out.to(dtype).clone().requires_grad_(True)
    col = _cols(tab, t, dtype, x0.dim())
    eps_hat, v = o[:, :C], o[:, C:]
    x_t = col(0) * x0 + col(1) * noise
    mse = mean_flat((noise - eps_hat) ** 2)
    eh = eps_hat if wrong == "nodetach" else eps_hat.detach()
    min_log, max_log = col(6), col(7)
    frac = (v + 1) / 2
    lv = frac * max_log + (1 - frac) * min_log
    pred_x0 = col(2) * x_t - col(3) * eh
    mu_t = col(4) * pred_x0 + col(5) * x_t
    mu_q = col(4) * x0 + col(5) * x_t
    kl = 0.5 * (-1.0 + lv - min_log + torch.exp(min_log - lv) + ((mu_q - mu_t) ** 2) * torch.exp(-lv))
    cx = x0 - mu_t
    inv_std = torch.exp(-(0.5 * lv))
    cdf_plus, cdf_min = _cdf(inv_std * (cx + half), k1), _cdf(inv_std * (cx - half), k1)
    logp = torch.where(x0 < -thr, torch.log(cdf_plus.clamp(min=1e-12)),
                       torch.where(x0 > thr, torch.log((1.0 - cdf_min).clamp(min=1e-12)), torch.log((cdf_plus - cdf_min).clamp(min=1e-12))))
    ln2 = 1.0 if wrong == "noln2" else math.log(2.0)
    kl, nll = mean_flat(kl) / ln2, mean_flat(-logp) / ln2
    vb = torch.where(t != 0, nll, kl) if wrong == "swap" else torch.where(t == 0, nll, kl)
    (f32_scalar(grad_scale) * (mse + vb).sum()).backward()
    d_out = o.grad.detach().clone()
    if wrong == "varfactor":                       # (max_log - min_log) instead of half of it
        d_out[:, C:] *= 2.0
    if wrong == "msechw":                          # the mse gradient without 1 / chw
        d_out[:, :C] *= x0[0].numel()
    return mse.detach(), vb.detach(), d_out


def z_center(x0, noise, out, t, tab):
    """float64 z = inv_std (x0 - model_mean) of every element (the argument the discretised likelihood is centred on)"""
    F = torch.float64
    C = x0.shape[1]
    x0, noise, out = x0.to(F), noise.to(F), out.to(F)
    col = _cols(tab, t, F, x0.dim())
    eh, v = out[:, :C], out[:, C:]
    x_t = col(0) * x0 + col(1) * noise
    frac = (v + 1) / 2
    lv = frac * col(7) + (1 - frac) * col(6)
    mu_t = col(4) * (col(2) * x_t - col(3) * eh) + col(5) * x_t
    return torch.exp(-0.5 * lv) * (x0 - mu_t)


def loss_inputs(n_extra, C, hw, seed=0, rows0=3, tab=None):
    """n = rows0 + n_extra samples of [C][hw] (fp32) with t = 0 on rows 0 .. rows0 - 1 and T_EXTRA[k % 6] on the others.
    t == 0 rows: row 0 x0 uniform in (-0.95, 0.95) (the middle branch), row 1 in (-1.5, -1.0), row 2 in (1.0, 1.5); the first six elements
    of each hold PLANTED (both sides of the 0.999 threshold); eps_hat is solved in float64 so that z hits a chosen target -- three quarters
    regular (|z| <= 2.5), the rest saturated (30 <= |z| <= 60, random sign; |eps_hat| reaches about 60), the planted six always regular.
    t > 0 rows: x0 uniform in (-1, 1), eps_hat = noise + 0.5 randn.  Var channels are uniform in (-1.5, 1.5) everywhere.
    -> dict(x0, noise, out, t, sat [n][C][hw] bool, C, hw)"""
    assert 1 <= rows0 <= 3 and C * hw >= len(PLANTED)
    tab = table() if tab is None else tab
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * n_extra + 104729 * C + hw + 31 * rows0)
    n = rows0 + n_extra
    F = torch.float64
    u = lambda *s: torch.rand(*s, generator=g, dtype=F)
    t = torch.tensor([0] * rows0 + [T_EXTRA[k % len(T_EXTRA)] for k in range(n_extra)], dtype=torch.int64)
    x0 = u(n, C, hw) * 2 - 1
    lo_hi = [(-0.95, 0.95), (-1.5, -1.0), (1.0, 1.5)]
    for r in range(rows0):
        lo, hi = lo_hi[r]
        x0[r] = lo + (hi - lo) * u(C, hw)
        x0[r].view(-1)[:len(PLANTED)] = torch.tensor(PLANTED, dtype=F)
    x0 = x0.float()
    noise = torch.randn(n, C, hw, generator=g, dtype=F).float()
    v = (u(n, C, hw) * 3 - 1.5).float()
    eh = (noise.double() + 0.5 * torch.randn(n, C, hw, generator=g, dtype=F))
    sat = torch.zeros(n, C, hw, dtype=torch.bool)
    # t == 0 rows: solve  z = inv_std (x0 - c1 (sra x_t - srm1 eh) - c2 x_t)  for eh (linear), all in float64 on the fp32 inputs
    tr = tab.double()[0]
    sa, s1, sra, srm1, c1, c2, min_log, max_log = (float(tr[k]) for k in range(8))
    for r in range(rows0):
        x, e, vv = x0[r].double(), noise[r].double(), v[r].double()
        x_t = sa * x + s1 * e
        frac = (vv + 1) / 2
        std = torch.exp(0.5 * (frac * max_log + (1 - frac) * min_log))
        z = u(C, hw) * 5 - 2.5
        big = (30 + 30 * u(C, hw)) * torch.where(u(C, hw) < 0.5, -1.0, 1.0)
        is_sat = u(C, hw) < 0.25
        is_sat.view(-1)[:len(PLANTED)] = False
        z = torch.where(is_sat, big, z)
        eh[r] = (sra * x_t - (x - z * std - c2 * x_t) / c1) / srm1
        sat[r] = is_sat
    out = torch.cat([eh.float(), v], dim=1)
    return dict(x0=x0, noise=noise, out=out, t=t, sat=sat, C=C, hw=hw)


def strata(inp, tab):
    """-> (elements of the t == 0 rows with 2.6 < |z| < 29, saturated elements with |z| < 30 or > 60.5, regular elements with |z| > 2.5001)"""
    rows = inp["t"] == 0
    z = z_center(inp["x0"], inp["noise"], inp["out"], inp["t"], tab)[rows].abs()
    sat = inp["sat"][rows]
    return int(((z > 2.6) & (z < 29)).sum()), int((sat & ((z < 29.999) | (z > 60.5))).sum()), int((~sat & (z > 2.5001)).sum())


def loss_case(inp, grad_scale, tab, dtype, wrong=None):
    """the fused loss on loss_inputs() as the dict accept_loss takes: mse, vb, d_out (+ t, sat, C for the reference side)"""
    mse, vb, d_out = dit_loss(inp["x0"], inp["noise"], inp["out"], inp["t"], tab, grad_scale, dtype, wrong)
    return dict(mse=mse, vb=vb, d_out=d_out, t=inp["t"], sat=inp["sat"], C=inp["C"])


def used32(got, ref64, ref32):
    """the share of bound32's allowance that `got` uses: max|got - ref64| / (MARGIN max|ref32 - ref64| + 4 * 2^-24 max|ref64|)"""
    f64 = lambda a: a.detach().cpu().double()
    got, ref64, ref32 = f64(got), f64(ref64), f64(ref32)
    allowed = MARGIN * float((ref32 - ref64).abs().max()) + 4 * 2.0 ** -24 * float(ref64.abs().max())
    err = float((got - ref64).abs().max())
    return err / allowed if allowed > 0 else (0.0 if err == 0 else math.inf)


def checked32(got, ref64, ref32, name):
    """bound32 with the figure printed first, as a DIT-LOSS-METRIC line"""
    print(f"DIT-LOSS-METRIC {name} used={used32(got, ref64, ref32):.4g}")
    return bound32(got, ref64, ref32, name)


def accept_loss(got, ref64, ref32, name="dit_loss"):
    """got: dict(mse [n], vb [n], d_out [n][2 C][hw]); ref64 / ref32: loss_case() in float64 / float32.  Raises AssertionError where `got`
    is further from ref64 than the bounds in the module docstring allow.  With a name, the largest share of each allowance that `got`
    uses is printed (DIT-LOSS-METRIC lines) before anything is asserted, and kept in RECORD."""
    f64 = lambda a: a.detach().cpu().double()
    t, C, sat = ref64["t"], ref64["C"], ref64["sat"]
    n = t.shape[0]
    g, r64, r32 = f64(got["d_out"]), f64(ref64["d_out"]), f64(ref32["d_out"])
    assert g.shape == r64.shape, (name, g.shape, r64.shape)
    cls_of = lambda i: "t0" if int(t[i]) == 0 else "t998+" if int(t[i]) >= 998 else "t"
    halves = (("d_eps", slice(0, C)), ("d_var", slice(C, 2 * C)))
    scalars = {}
    for key in ("mse", "vb"):
        a, b, c = f64(got[key]), f64(ref64[key]), f64(ref32[key])
        for cls, rows in (("t0", t == 0), ("t", t != 0)):
            if bool(rows.any()):
                r = float(((c[rows] - b[rows]).abs() / b[rows].abs()).max())
                scalars[key, cls] = ((a[rows] - b[rows]).abs(), (MARGIN * r + 4 * 2.0 ** -24) * b[rows].abs(), r, b[rows].abs())
    if name is not None:
        fig = {}
        for i in range(n):
            for h, sl in halves:
                k = f"{name}.{h}.{cls_of(i)}"
                fig[k] = max(fig.get(k, 0.0), used32(g[i, sl], r64[i, sl], r32[i, sl]))
        for (key, cls), (err, allowed, r, mag) in scalars.items():
            fig[f"{name}.{key}.{cls}"] = float((err / allowed).max())
        for k in sorted(fig):
            print(f"DIT-LOSS-METRIC {k} used={fig[k]:.4g}")
            _rec(k, "used", fig[k])
    for i in range(n):
        for h, sl in halves:
            bound32(g[i, sl], r64[i, sl], r32[i, sl], None if name is None else f"{name}.{h}.{cls_of(i)}")
    got_sat = g[:, C:][sat]
    assert bool((got_sat == 0.0).all()), f"{name}: {int((got_sat != 0).sum())} saturated elements with a var-gradient != 0.0"
    assert bool((r64[:, C:][sat] == 0.0).all()) and bool((r32[:, C:][sat] == 0.0).all()), f"{name}: the reference's saturated gradients"
    for key in ("mse", "vb"):
        assert torch.isfinite(f64(got[key])).all(), f"{name}.{key}: non-finite values"
    for (key, cls), (err, allowed, r, mag) in scalars.items():
        assert bool((err <= allowed).all()), (f"{name}.{key}.{cls}: |got - ref64| / |ref64| = {float((err / mag).max()):.4g} > "
                                              f"{MARGIN} * {r:.4g} + 4 * 2^-24")


# ------------------------------------------------------------------------------------------------ plain restatements
def q_sample(x0, noise, t, tab, dtype):
    col = _cols(tab, t, dtype, x0.dim())
    return col(0) * x0.to(dtype) + col(1) * noise.to(dtype)


def cfg_combine(out, n_guided, s, dtype):
    """out [2 half][cout][hw]: channels < n_guided of sample i and i + half both become uncond + s (cond - uncond); the rest is unchanged"""
    out = out.to(dtype).clone()
    half = out.shape[0] // 2
    c, u = out[:half, :n_guided], out[half:, :n_guided]
    h = u + torch.tensor(s, dtype=torch.float32).to(dtype) * (c - u)
    out[:half, :n_guided] = h
    out[half:, :n_guided] = h
    return out


def p_sample(x, out, t, tab, noise, clip, dtype):
    """-> sample, pred_xstart (both [n][C][hw])"""
    C = x.shape[1]
    x, out, noise = x.to(dtype), out.to(dtype), noise.to(dtype)
    col = _cols(tab, t, dtype, x.dim())
    eps, v = out[:, :C], out[:, C:]
    frac = (v + 1) / 2
    lv = frac * col(7) + (1 - frac) * col(6)
    px = col(2) * x - col(3) * eps
    if clip:
        px = px.clamp(-1, 1)
    mean = col(4) * px + col(5) * x
    nz = (t != 0).to(dtype).view((-1,) + (1,) * (x.dim() - 1))
    return mean + nz * torch.exp(0.5 * lv) * noise, px


def ddpm_q_sample(x0, e, t, abar, dtype):
    """DDPM/functions/losses.py:30: x0 sqrt(a) + e sqrt(1 - a), a = abar[t] (fp32 table; 1 - a formed in fp32 as the reference forms it)"""
    a = abar[t].view((-1,) + (1,) * (x0.dim() - 1))
    return x0.to(dtype) * a.to(dtype).sqrt() + e.to(dtype) * (1.0 - a).to(dtype).sqrt()


def ddpm_sample_loss(e, out, dtype):
    return ((e.to(dtype) - out.to(dtype)) ** 2).reshape(e.shape[0], -1).sum(1)


def ddpm_loss_coef(per, mode, lambd, scale, n_global, dtype, wsum=None):
    """mode 0: loss = sum(per) / n_global, coef_i = 2 scale / n_global.  mode 1: w_i = 1 / (per_i^lambd + 1e-8), W = sum w (or the given
    `wsum`: the sum over every part of a split batch), loss = sum(w_i per_i) / W, coef_i = 2 scale w_i / W.  -> coef [n], loss, W"""
    per = per.to(dtype)
    scale = torch.tensor(scale, dtype=torch.float32).to(dtype)
    if mode == 0:
        W = torch.tensor(float(n_global), dtype=dtype)
        w = torch.ones_like(per)
    else:
        w = 1.0 / (torch.pow(per, torch.tensor(lambd, dtype=torch.float32).to(dtype)) + 1e-8)
        W = w.sum() if wsum is None else wsum.to(dtype)
    return 2.0 * scale * (w / W), (w * per).sum() / W, W


def ddpm_loss_bwd(e, out, coef, dtype):
    return coef.to(dtype).view((-1,) + (1,) * (e.dim() - 1)) * (out.to(dtype) - e.to(dtype))


def patchify(img, p, chan_last):
    """image [n][C][H][W] -> token rows [n T][C p p] bf16; column c p p + ph p + pw, or (ph p + pw) C + c with chan_last"""
    n, C, H, W = img.shape
    x = img.reshape(n, C, H // p, p, W // p, p)
    x = x.permute(0, 2, 4, 3, 5, 1) if chan_last else x.permute(0, 2, 4, 1, 3, 5)
    return x.reshape(n * (H // p) * (W // p), C * p * p).to(torch.bfloat16)


def unpatchify(rows, n, C, H, W, p):
    """token rows [n T][p p C] (chan_last order) -> image [n][C][H][W] (DiT/models.py:224-236)"""
    x = rows.reshape(n, H // p, W // p, p, p, C)
    return torch.einsum("nhwpqc->nchpwq", x).reshape(n, C, H, W)


def guard_inputs(y, t, num_classes, T):
    """-> y clamped into [0, num_classes), t clamped into [0, T), the number of labels and of timesteps the clamp changed"""
    ys, ts = y.clamp(0, num_classes - 1), t.clamp(0, T - 1)
    return ys, ts, int((ys != y).sum()), int((ts != t).sum())


def guard_finite(terms, stats):
    """terms: the vectors that were passed (None entries are skipped); -> the increments of flags[0] and flags[1] (0 or 1 each)"""
    bad = any(not bool(torch.isfinite(v).all()) for v in terms if v is not None)
    return int(bad), int(stats is not None and not bool(torch.isfinite(stats[0])))
