"""The tests' own float64 numpy restatement of DiT/diffusion/gaussian_diffusion.py's likelihood evaluation (_vb_terms_bpd :682-713,
_prior_bpd :789-803, calc_bpd_loop :805-858 over p_mean_variance, q_posterior_mean_variance and diffusion_utils.py) for the LEARNED_RANGE /
EPSILON model, and an fp32 torch restatement of one term for error comparisons on the device.

Table entries are the fp32 values the reference's _extract_into_tensor yields (the fp64 table rounded once), widened to float64: what is
compared is the arithmetic, not the table.  ``tab`` is the [T, 8] table of sfron.diffusion.GaussianDiffusion (sqrt_ac, sqrt_1m_ac,
sqrt_recip_ac, sqrt_recipm1_ac, post_coef1, post_coef2, post_logvar_clipped, log_beta)."""
import numpy as np
import torch

LN2 = np.log(2.0)


def _cdf(x):
    return 0.5 * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


def _u(x):
    return np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)


def vb_terms(tab, x0, t, model_out, clip, x_t=None, noise=None, detail=False):
    """One term for per-row table indices ``t``: dict(output [n], pred_xstart, xstart_mse [n], mse [n] (None without noise)).  x_t is
    given or q_sample(x0, t, noise).  detail=True adds the t == 0 rows' likelihood internals (cdf_delta, the tanh arguments) and
    pred_mag = |sqrt_recip_ac x_t| + |sqrt_recipm1_ac eps_hat|, the operand magnitude behind pred_xstart."""
    tab = np.asarray(tab, dtype=np.float32).astype(np.float64)
    x0 = np.asarray(x0, dtype=np.float64)
    out = np.asarray(model_out, dtype=np.float64)
    t = np.asarray(t).astype(np.int64)
    n, C = x0.shape[0], x0.shape[1]
    col = lambda k: tab[t, k].reshape((n,) + (1,) * (x0.ndim - 1))
    if x_t is None:
        noise = np.asarray(noise, dtype=np.float64)
        x_t = col(0) * x0 + col(1) * noise
    x_t = np.asarray(x_t, dtype=np.float64)
    eps_hat, v = out[:, :C], out[:, C:]
    frac = (v + 1) / 2
    lv = frac * col(7) + (1 - frac) * col(6)
    px = col(2) * x_t - col(3) * eps_hat
    if clip:
        px = np.clip(px, -1.0, 1.0)
    mu_t = col(4) * px + col(5) * x_t
    mu_q = col(4) * x0 + col(5) * x_t
    kl = 0.5 * (-1.0 + lv - col(6) + np.exp(col(6) - lv) + (mu_q - mu_t) ** 2 * np.exp(-lv))
    cx = x0 - mu_t
    inv_std = np.exp(-0.5 * lv)
    plus_in, min_in = inv_std * (cx + 1.0 / 255.0), inv_std * (cx - 1.0 / 255.0)
    cdf_plus, cdf_min = _cdf(plus_in), _cdf(min_in)
    delta = cdf_plus - cdf_min
    logp = np.where(x0 < -0.999, np.log(np.maximum(cdf_plus, 1e-12)),
                    np.where(x0 > 0.999, np.log(np.maximum(1.0 - cdf_min, 1e-12)), np.log(np.maximum(delta, 1e-12))))
    flat = lambda a: a.reshape(n, -1).mean(axis=1)
    res = dict(output=np.where(t == 0, flat(-logp), flat(kl)) / LN2, pred_xstart=px, xstart_mse=flat((px - x0) ** 2), mse=None)
    if noise is not None:
        res["mse"] = flat(((col(2) * x_t - px) / col(3) - np.asarray(noise, dtype=np.float64)) ** 2)
    if detail:
        # the probability the chosen branch takes the log of, and the tanh arguments behind it
        res.update(prob=np.where(x0 < -0.999, cdf_plus, np.where(x0 > 0.999, 1.0 - cdf_min, delta)), u_plus=_u(plus_in), u_min=_u(min_in),
                   rows0=(t == 0), pred_mag=np.abs(col(2) * x_t) + np.abs(col(3) * eps_hat))
    return res


def fragile_count(detail, x0):
    """Elements of the t == 0 rows whose log-likelihood a ONE-ULP difference in fp32 tanh could move by more than the tests' tolerance.
    fp32 cdf values near 0 or 1 are multiples of 2^-25 (3e-8), so a probability below 1e-5 is fragile (one step is 0.3 % of it or more)
    UNLESS every tanh that the branch reads is saturated with a margin (|u| > 9.5: tanhf is exactly +-1 from 9.02 on), where fp32 gives
    exactly 0 and the 1e-12 clamp decides.  Returns (fragile, within a factor of 10 of the clamp) over the rows with t == 0."""
    x0 = np.asarray(x0, dtype=np.float64)
    rows = detail["rows0"]
    p, up, um = detail["prob"][rows], detail["u_plus"][rows], detail["u_min"][rows]
    x = x0[rows]
    lo, hi = x < -0.999, x > 0.999
    sat = np.where(lo, up < -9.5, np.where(hi, um > 9.5, (np.minimum(up, um) > 9.5) | (np.maximum(up, um) < -9.5)))
    fragile = (p < 1e-5) & ~sat
    near = (p > 1e-13) & (p < 1e-11)
    return int(fragile.sum()), int(near.sum())


def prior_bpd(tables, x0):
    """_prior_bpd from the fp64 tables dict of sfron.diffusion (fp32-rounded scalars, as the reference gathers them)."""
    ac = tables["alphas_cumprod"][-1]
    sa, lv1 = float(np.float32(np.sqrt(ac))), float(np.float32(np.log(1.0 - ac)))
    x0 = np.asarray(x0, dtype=np.float64)
    kl = 0.5 * (-1.0 + 0.0 - lv1 + np.exp(lv1 - 0.0) + (sa * x0 - 0.0) ** 2 * np.exp(-0.0))
    return kl.reshape(x0.shape[0], -1).mean(axis=1) / LN2


def calc_bpd_loop(d, model, x0, step_noise, clip):
    """calc_bpd_loop on a sfron.diffusion.GaussianDiffusion ``d`` (its tables and timestep map), ``model(x_t float64 tensor, original
    timesteps) -> tensor``: the reference's dict, float64.  Column k is t = T - 1 - k."""
    T, n = d.num_timesteps, x0.shape[0]
    tab = d.tab.cpu().numpy()
    x0 = np.asarray(x0, dtype=np.float64)
    vb, xs, mse = [], [], []
    for k, i in enumerate(range(T - 1, -1, -1)):
        t = np.full((n,), i, dtype=np.int64)
        noise = np.asarray(step_noise[k], dtype=np.float64)
        tf = tab.astype(np.float64)
        x_t = tf[i, 0] * x0 + tf[i, 1] * noise
        out = model(torch.from_numpy(x_t), torch.full((n,), int(d.timestep_map[i]), dtype=torch.int64)).double().numpy()
        r = vb_terms(tab, x0, t, out, clip, x_t=x_t, noise=noise)
        vb.append(r["output"]), xs.append(r["xstart_mse"]), mse.append(r["mse"])
    vb, xs, mse = np.stack(vb, 1), np.stack(xs, 1), np.stack(mse, 1)
    prior = prior_bpd(d.tables, x0)
    return dict(total_bpd=vb.sum(1) + prior, prior_bpd=prior, vb=vb, xstart_mse=xs, mse=mse)


def stubs(A, abar1000, C, dtype=torch.float32, device="cpu"):
    """The two stub models of tests/golden/make_dit_sampler_golden.py (the linear stub and the contractive stub2), in ``dtype``."""
    A = torch.as_tensor(A).to(device, dtype)
    s1m = torch.tensor(np.sqrt(1.0 - np.asarray(abar1000)), dtype=torch.float32).to(device, dtype)

    def stub(x, ts, **kw):
        return torch.einsum("oc,nchw->nohw", A, x) * torch.cos(ts.to(dtype) / 300.0).view(-1, 1, 1, 1) + 0.05

    def stub2(x, ts, **kw):
        lin = torch.einsum("oc,nchw->nohw", A, x)
        eps = 0.9 * x / s1m[ts].view(-1, 1, 1, 1) + 0.02 * lin[:, :C]
        return torch.cat([eps, lin[:, C:] * torch.cos(ts.to(dtype) / 300.0).view(-1, 1, 1, 1) + 0.05], dim=1)
    return stub, stub2


def vb_terms_fp32(tab, x0, t, model_out, clip, noise):
    """The same term, expression for expression, in fp32 torch on the tensors' device: (output, xstart_mse, mse), each [n] -- the
    yardstick of what fp32 arithmetic in the reference's order costs against float64."""
    n, C = x0.shape[0], x0.shape[1]
    r = tab[t]
    col = lambda k: r[:, k].view((n,) + (1,) * (x0.dim() - 1))
    x_t = col(0) * x0 + col(1) * noise
    eps_hat, v = model_out[:, :C], model_out[:, C:]
    frac = (v + 1) / 2
    lv = frac * col(7) + (1 - frac) * col(6)
    px = col(2) * x_t - col(3) * eps_hat
    if clip:
        px = px.clamp(-1, 1)
    mu_t = col(4) * px + col(5) * x_t
    mu_q = col(4) * x0 + col(5) * x_t
    kl = 0.5 * (-1.0 + lv - col(6) + torch.exp(col(6) - lv) + ((mu_q - mu_t) ** 2) * torch.exp(-lv))
    cx = x0 - mu_t
    inv = torch.exp(-(0.5 * lv))
    cdf = lambda z: 0.5 * (1.0 + torch.tanh(np.sqrt(2.0 / np.pi) * (z + 0.044715 * torch.pow(z, 3))))
    cp, cm = cdf(inv * (cx + 1.0 / 255.0)), cdf(inv * (cx - 1.0 / 255.0))
    logp = torch.where(x0 < -0.999, torch.log(cp.clamp(min=1e-12)),
                       torch.where(x0 > 0.999, torch.log((1.0 - cm).clamp(min=1e-12)), torch.log((cp - cm).clamp(min=1e-12))))
    flat = lambda a: a.reshape(n, -1).mean(dim=1)
    output = torch.where(t == 0, flat(-logp) / np.log(2.0), flat(kl) / np.log(2.0))
    eps = (col(2) * x_t - px) / col(3)
    return output, flat((px - x0) ** 2), flat((eps - noise) ** 2)
