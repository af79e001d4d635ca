"""Generates tests/golden/dit_bpd.npz from the reference's likelihood evaluation (DiT/diffusion/gaussian_diffusion.py: _vb_terms_bpd
:682-713, _prior_bpd :789-803, calc_bpd_loop :805-858), on the CPU.

The reference package is imported, not copied.  A and abar1000 are dit_sampling.npz's, the stub models those of
make_dit_sampler_golden.py: the linear stub and the contractive stub2.

Contents
  one_x0, one_xt, one_t            x0 = 0.5 randn [5, 4, 8, 8] (see below), x_t = q_sample(x0, t, randn), t = [0, 1, 500, 999, 0] per row.  Row 4
                                   is the deliberately extreme row: every other element is pushed beyond +-0.999 (alternating sides), so at
                                   t = 0 all three branches of discretized_gaussian_log_likelihood are taken
  one/<stub>/model_out             what the stub returned for (x_t, t) on create_diffusion("")
  one/<stub>/clip<0|1>/output, /pred_xstart      _vb_terms_bpd
  prior_full, prior_10             _prior_bpd of one_x0 on create_diffusion("") and of x0_10 on create_diffusion("10")
  x0_10 [3, 4, 8, 8], loop10/<stub>/clip<0|1>/<key>      calc_bpd_loop on create_diffusion("10"), both stubs, key = total_bpd, prior_bpd,
                                   vb, xstart_mse, mse; torch.manual_seed(LOOP_SEED) before each run
  x0_full [2, 4, 4, 4], loopfull/stub2/clip<0|1>/<key>   calc_bpd_loop on create_diffusion("") (T = 1000), stub2
The per-step noise is NOT stored: calc_bpd_loop draws one randn_like(x_start) per step and nothing else from the global CPU stream, so
``torch.manual_seed(LOOP_SEED); [torch.randn_like(x0) for _ in range(T)]`` regenerates it.

Inputs and the t == 0 term.  At t = 0 the model's standard deviation is about 0.01, and fp32 cdf values near 0 or 1 are multiples of
3e-8: an element whose probability is small but not far below the 1e-12 clamp (roughly 4 to 7 standard deviations out) gets a log that
a one-ulp difference in tanhf moves by whole nats, and a comparison on it means nothing.  stub2 puts x0 - mean at 0.9 x0, i.e. 90 |x0|
standard deviations, so elements with |x0| < 0.12 are shrunk to 0.15 x0 (under 2.2 standard deviations); the rest lie 10 standard
deviations out or more, where every fp32 implementation gives exactly 0 and the clamp decides.  With clip_denoised the mean
cannot follow an x0 beyond +-1, so elements with |x0| > 0.95 are stretched to 1.25 x0 and the extreme row's pushed elements lie at 1.15 or
more (15 standard deviations past the clamped mean), for the same reason.  Over the seeds tried, the first whose
every run has no fragile element (tests/dit_bpd_ref.py fragile_count, a float64 restatement) is taken, the extreme row included; the
number of elements within a factor of 10 of the clamp is reported too and must be 0.

Run:  python tests/golden/make_dit_bpd_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
from make_dit_sampler_golden import stubs  # noqa: E402
import dit_bpd_ref as R  # noqa: E402

ONE_T = [0, 1, 500, 999, 0]
ONE_NOISE_SEED, LOOP_SEED = 21, 77
KEYS = ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")


def draw_x0(seed, shape):
    x = 0.5 * torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    x = torch.where(x.abs() < 0.12, 0.15 * x, x)
    return torch.where(x.abs() > 0.95, 1.25 * x, x)


def tab8(d):
    """The [T, 8] table of sfron.diffusion from the reference's own fp64 arrays."""
    return np.stack([d.sqrt_alphas_cumprod, d.sqrt_one_minus_alphas_cumprod, d.sqrt_recip_alphas_cumprod, d.sqrt_recipm1_alphas_cumprod,
                     d.posterior_mean_coef1, d.posterior_mean_coef2, d.posterior_log_variance_clipped, np.log(d.betas)], 1).astype(np.float32)


class Recorder:
    """Wraps a stub: keeps the last (x_t, output) it saw -- in calc_bpd_loop that is the t = 0 step."""

    def __init__(self, fn):
        self.fn = fn

    def __call__(self, x, ts, **kw):
        self.x, self.out = x.clone(), self.fn(x, ts, **kw)
        return self.out


def build(seed, ref, src):
    A = torch.from_numpy(src["A"])
    C = A.shape[1]
    named = dict(zip(("stub", "stub2"), stubs(A, src["abar1000"], C)))
    dfull, d10 = ref.create_diffusion(timestep_respacing=""), ref.create_diffusion(timestep_respacing="10")
    out, fragile, near, log = {}, 0, 0, []

    def check(d, x0, x_t, mo, clip, what):
        det = R.vb_terms(tab8(d), x0.numpy(), np.zeros(x0.shape[0], dtype=np.int64), mo.numpy(), clip, x_t=x_t.numpy(), detail=True)
        f, nr = R.fragile_count(det, x0.numpy())
        log.append(f"  {what}: t = 0 elements {x0.numel()}, fragile {f}, within 10x of the clamp {nr}, min probability {det['prob'].min():.3e}")
        return f, nr

    # ---- single calls
    x0 = draw_x0(seed, (5, C, 8, 8))
    side = torch.where(torch.arange(x0[4].numel() // 2) % 2 == 0, -1.0, 1.0)
    x0[4].view(-1)[::2] = side * (1.15 + 0.3 * torch.rand(side.shape, generator=torch.Generator().manual_seed(seed + 1)))
    t = torch.tensor(ONE_T)
    x_t = dfull.q_sample(x0, t, noise=torch.randn(x0.shape, generator=torch.Generator().manual_seed(ONE_NOISE_SEED)))
    out.update(one_x0=x0.numpy(), one_xt=x_t.numpy(), one_t=np.array(ONE_T))
    for name, fn in named.items():
        mo = fn(x_t, t)
        out[f"one/{name}/model_out"] = mo.numpy()
        for clip in (0, 1):
            r = dfull._vb_terms_bpd(fn, x0, x_t, t, clip_denoised=bool(clip), model_kwargs={})
            out[f"one/{name}/clip{clip}/output"], out[f"one/{name}/clip{clip}/pred_xstart"] = r["output"].numpy(), r["pred_xstart"].numpy()
            rows = [0, 4]
            f, nr = check(dfull, x0[rows], x_t[rows], mo[rows], clip, f"one/{name}/clip{clip}")
            fragile, near = fragile + f, near + nr
    x0e = x0[4].flatten()
    assert (x0e < -0.999).any() and (x0e > 0.999).any() and (x0e.abs() <= 0.999).any()
    out["prior_full"] = dfull._prior_bpd(x0).numpy()
    # ---- loops
    x10, xfull = draw_x0(seed + 2, (3, C, 8, 8)), draw_x0(seed + 3, (2, C, 4, 4))
    out.update(x0_10=x10.numpy(), x0_full=xfull.numpy())
    out["prior_10"] = d10._prior_bpd(x10).numpy()
    for tag, d, x, names in (("loop10", d10, x10, ("stub", "stub2")), ("loopfull", dfull, xfull, ("stub2",))):
        for name in names:
            for clip in (0, 1):
                rec = Recorder(named[name])
                torch.manual_seed(LOOP_SEED)
                r = d.calc_bpd_loop(rec, x, clip_denoised=bool(clip), model_kwargs={})
                for k in KEYS:
                    out[f"{tag}/{name}/clip{clip}/{k}"] = r[k].numpy()
                f, nr = check(d, x, rec.x, rec.out, clip, f"{tag}/{name}/clip{clip}")
                fragile, near = fragile + f, near + nr
                log.append(f"    total_bpd {r['total_bpd'].numpy()}")
    return out, fragile, near, log


def main():
    ref = mg.import_ref_dit_diffusion()
    src = np.load(os.path.join(HERE, "dit_sampling.npz"))
    for seed in range(20):
        out, fragile, near, log = build(seed, ref, src)
        print(f"seed {seed}: fragile {fragile}, within 10x of the clamp {near}")
        print("\n".join(log))
        if fragile == 0 and near == 0:
            break
    else:
        raise SystemExit("no seed without a fragile t = 0 element")
    out["seed"] = np.array(seed)
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    path = os.path.join(HERE, "dit_bpd.npz")
    np.savez_compressed(path, **out)
    print("dit_bpd.npz:", len(out), "entries,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
