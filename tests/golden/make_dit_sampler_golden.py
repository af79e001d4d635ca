"""Generates tests/golden/dit_sampler.npz from the reference's DDIM sampler (DiT/diffusion/gaussian_diffusion.py:513-680), on the CPU.

The reference package is imported, not copied.  Inputs are dit_sampling.npz's: A, z [4, 4, 8, 8], abar1000 and that file's two stub
models -- the linear stub (run with clip_denoised=True: it grows without the clamp) and the contractive stub2 (clip_denoised=False).

Contents
  ac_prev10 / ac_next10            the fp64 alphas_cumprod_prev / alphas_cumprod_next of create_diffusion("10")
  loop/<spec>/<stub>/<eta>         ddim_sample_loop outputs, spec "10" and "ddim25", eta 0, 0.5, 1, torch.manual_seed(77) before each run
                                   (the reference draws one randn_like(x) per step, for eta == 0 too)
  one_ddim_* / one_rev_*           one ddim_sample (eta 0.5, torch.manual_seed(5)) and one ddim_reverse_sample step at t = [0, 9, 3, 0] on
                                   the linear stub, clip_denoised=False, with their pred_xstart
  rev_traj                         the 10 ddim_reverse_sample steps t = 0 .. 9 from 0.1 z on stub2, clip_denoised=False: every state

Run:  python tests/golden/make_dit_sampler_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

ETAS = (0.0, 0.5, 1.0)
SPECS = ("10", "ddim25")


def stubs(A, abar1000, C):
    s1m = torch.tensor(np.sqrt(1.0 - abar1000), dtype=torch.float32)

    def stub(x, ts, **kw):                       # sees ORIGINAL timesteps through the wrapped model
        return torch.einsum("oc,nchw->nohw", A, x) * torch.cos(ts.float() / 300.0).view(-1, 1, 1, 1) + 0.05

    def stub2(x, ts, **kw):
        lin = torch.einsum("oc,nchw->nohw", A, x)
        eps = 0.9 * x / s1m[ts].view(-1, 1, 1, 1) + 0.02 * lin[:, :C]
        return torch.cat([eps, lin[:, C:] * torch.cos(ts.float() / 300.0).view(-1, 1, 1, 1) + 0.05], dim=1)
    return stub, stub2


def main():
    ref = mg.import_ref_dit_diffusion()
    src = np.load(os.path.join(HERE, "dit_sampling.npz"))
    z, A = torch.from_numpy(src["z"]), torch.from_numpy(src["A"])
    stub, stub2 = stubs(A, src["abar1000"], z.shape[1])
    out = {}
    d10 = ref.create_diffusion(timestep_respacing="10")
    out["ac_prev10"], out["ac_next10"] = np.asarray(d10.alphas_cumprod_prev), np.asarray(d10.alphas_cumprod_next)
    assert out["ac_prev10"].dtype == np.float64 and out["ac_next10"].dtype == np.float64
    for spec in SPECS:
        d = ref.create_diffusion(timestep_respacing=spec)
        out[f"map_{spec}"] = np.array(d.timestep_map)
        for name, fn, clip in (("stub_clip1", stub, True), ("stub2_clip0", stub2, False)):
            for eta in ETAS:
                torch.manual_seed(77)
                r = d.ddim_sample_loop(fn, z.shape, z, clip_denoised=clip, model_kwargs={}, device="cpu", eta=eta).numpy()
                assert np.isfinite(r).all() and np.abs(r).max() < 1e3, (spec, name, eta, np.abs(r).max())
                out[f"loop/{spec}/{name}/{eta}"] = r
                print(f"loop {spec:7s} {name:11s} eta {eta}: max |x| {np.abs(r).max():.4g}")
    t = torch.tensor([0, 9, 3, 0])
    torch.manual_seed(5)
    one = d10.ddim_sample(stub, z, t, clip_denoised=False, model_kwargs={}, eta=0.5)
    out["one_ddim_sample"], out["one_ddim_pred_xstart"] = one["sample"].numpy(), one["pred_xstart"].numpy()
    rev = d10.ddim_reverse_sample(stub, z, t, clip_denoised=False, model_kwargs={}, eta=0.0)
    out["one_rev_sample"], out["one_rev_pred_xstart"] = rev["sample"].numpy(), rev["pred_xstart"].numpy()
    x, traj = 0.1 * z, []
    for i in range(d10.num_timesteps):
        x = d10.ddim_reverse_sample(stub2, x, torch.tensor([i] * z.shape[0]), clip_denoised=False, model_kwargs={}, eta=0.0)["sample"]
        traj.append(x.numpy())
    out["rev_traj"] = np.stack(traj)
    print(f"reverse trajectory: final max |x| {np.abs(traj[-1]).max():.4g}")
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    np.savez_compressed(os.path.join(HERE, "dit_sampler.npz"), **out)
    print("dit_sampler.npz:", len(out), "entries,", os.path.getsize(os.path.join(HERE, "dit_sampler.npz")), "bytes")


if __name__ == "__main__":
    main()
