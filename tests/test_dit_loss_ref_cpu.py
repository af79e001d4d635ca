"""CPU: the reference of tests/test_gpu_dit_loss.py is independent of the kernels and its bounds can fail.

  * the float64 restatement of the fused loss against oracle.diffusion_ref.training_losses_from_output (fp32, torch autograd) at fp32
    distance, and its forward vb against tests/dit_bpd_ref.vb_terms (numpy float64) at float64 distance;
  * at every shape the GPU file runs: no element of a t == 0 row has 2.6 < |z| < 29, dit_bpd_ref.fragile_count is (0, 0), the saturated
    var-gradients are exactly zero in both dtypes, and the float32 restatement passes accept_loss (ratio 1 / MARGIN);
  * teeth: each of the eight wrong formulas of dit_loss_ref.WRONG, applied to the float32 restatement, is rejected by accept_loss at every
    loss shape and both grad_scale signs;
  * the guard references on hand-written vectors; patchify / unpatchify round trips at every layout shape; the DDPM restatements against
    the oracle's."""
import numpy as np
import pytest
import torch

import dit_bpd_ref as B
import dit_loss_ref as L
import dit_rows_ref as R

F64, F32 = torch.float64, torch.float32
TAB = L.table()
N_EXTRA = 6


def _inputs(C, hw):
    return L.loss_inputs(N_EXTRA, C, hw)


@pytest.mark.parametrize("C,hw", L.LOSS_SHAPES)
def test_float64_restatement_agrees_with_the_oracle_and_the_bpd_reference(C, hw):
    from oracle import diffusion_ref as dref
    i = _inputs(C, hw)
    n = i["t"].shape[0]
    gs = -0.001 / n
    mse, vb, d_out = L.dit_loss(i["x0"], i["noise"], i["out"], i["t"], TAB, gs, F64)
    # the oracle: fp32 torch with autograd, on the same inputs
    tabs = dref.DiffusionTables(1000)
    o = i["out"].clone().requires_grad_(True)
    x_t = dref.q_sample(tabs, i["x0"], i["t"], i["noise"])
    terms = dref.training_losses_from_output(tabs, o, i["x0"], x_t, i["t"], i["noise"])
    (L.f32_scalar(gs) * terms["loss"].sum()).backward()
    m32, v32, d32 = L.dit_loss(i["x0"], i["noise"], i["out"], i["t"], TAB, gs, F32)
    # fp32 distance: the oracle is as far from float64 as the float32 restatement is, up to the order of its operations (factor MARGIN)
    for name, got, ref, yard in (("mse", terms["mse"].detach(), mse, m32), ("vb", terms["vb"].detach(), vb, v32)):
        rel = ((got.double() - ref).abs() / ref.abs()).max().item()
        ry = ((yard.double() - ref).abs() / ref.abs()).max().item()
        assert rel <= R.MARGIN * ry + 4 * 2.0 ** -24, (name, rel, ry)
    for h, sl in (("eps", slice(0, C)), ("var", slice(C, 2 * C))):
        for r in range(n):
            R.bound32(o.grad[r, sl], d_out[r, sl], d32[r, sl], None)
    # forward vb against the numpy float64 restatement of the likelihood evaluation
    want = B.vb_terms(TAB.numpy(), i["x0"].numpy(), i["t"].numpy(), i["out"].numpy(), clip=False, noise=i["noise"].numpy())
    assert np.abs(vb.numpy() - want["output"]).max() <= 1e-12 * np.abs(want["output"]).max()
    assert np.abs(mse.numpy() - want["mse"]).max() <= 1e-9 * np.abs(want["mse"]).max()      # eps recovered from pred_xstart there
    # q_sample restated
    assert torch.equal(L.q_sample(i["x0"], i["noise"], i["t"], TAB, F32), x_t)


@pytest.mark.parametrize("C,hw", L.LOSS_SHAPES)
@pytest.mark.parametrize("rows0,n_extra", [(3, N_EXTRA), (1, 0)])
def test_strata_hold_at_every_gpu_shape(C, hw, rows0, n_extra):
    i = L.loss_inputs(n_extra, C, hw, rows0=rows0)
    assert L.strata(i, TAB) == (0, 0, 0)
    d = B.vb_terms(TAB.numpy(), i["x0"].numpy(), i["t"].numpy(), i["out"].numpy(), clip=False, noise=i["noise"].numpy(), detail=True)
    assert B.fragile_count(d, i["x0"].numpy()) == (0, 0)
    rows = i["t"] == 0
    sat = i["sat"]
    assert not bool(sat[~rows].any())
    share = float(sat[rows].double().mean())
    assert C * hw < 100 or 0.15 < share < 0.35, share
    # every branch is occupied on both sides of the threshold
    x = i["x0"][0].view(-1)[:6]
    assert int((x < -0.999).sum()) == 2 and int((x > 0.999).sum()) == 2
    if rows0 == 3:
        assert bool((i["x0"][1].view(-1)[6:] < -0.999).all()) and bool((i["x0"][2].view(-1)[6:] > 0.999).all())
    n = i["t"].shape[0]
    for gs in (1.0 / n, -0.001 / n):
        c64, c32 = L.loss_case(i, gs, TAB, F64), L.loss_case(i, gs, TAB, F32)
        for c in (c64, c32):
            v = c["d_out"][:, C:]
            assert bool((v[sat] == 0.0).all())
            assert int((v[rows.view(-1, 1, 1) & ~sat] != 0).sum()) > 0.7 * int((rows.view(-1, 1, 1) & ~sat).sum())
        L.accept_loss(c32, c64, c32, name=None)                     # the yardstick itself: ratio 1 / MARGIN
        assert float(c64["mse"].min()) > 0 and float(c64["vb"].abs().min()) > 0


@pytest.mark.parametrize("C,hw", L.LOSS_SHAPES)
@pytest.mark.parametrize("wrong", L.WRONG)
def test_accept_loss_rejects_every_wrong_formula(C, hw, wrong):
    i = _inputs(C, hw)
    n = i["t"].shape[0]
    for gs in (1.0 / n, -0.001 / n):
        c64, c32 = L.loss_case(i, gs, TAB, F64), L.loss_case(i, gs, TAB, F32)
        L.accept_loss(c32, c64, c32, name=None)
        bad = L.loss_case(i, gs, TAB, F32, wrong=wrong)
        with pytest.raises(AssertionError):
            L.accept_loss(bad, c64, c32, name=None)


def test_accept_loss_rejects_a_nonzero_saturated_gradient_and_a_scaled_var_half():
    """what the whole-tensor rtol of the older test lets through: the var half wrong by a factor, on one sample"""
    i = _inputs(4, 63)
    gs = 1.0 / 9
    c64, c32 = L.loss_case(i, gs, TAB, F64), L.loss_case(i, gs, TAB, F32)
    for row in range(9):
        bad = dict(c32, d_out=c32["d_out"].clone())
        bad["d_out"][row, 4:] *= 1.01
        if int(i["t"][row]) >= 998:                 # "finite and tiny" is all the bound says there (yardstick error: 7 % and 13 % of the size)
            L.accept_loss(bad, c64, c32, name=None)
            continue
        with pytest.raises(AssertionError):
            L.accept_loss(bad, c64, c32, name=None)
        whole = (bad["d_out"] - c64["d_out"]).abs().max() / c64["d_out"].abs().max()
        assert whole < 5e-4                          # ... and a whole-tensor bound would have passed it
    bad = dict(c32, d_out=c32["d_out"].clone())
    idx = i["sat"].nonzero()[0]
    bad["d_out"][idx[0], 4 + idx[1], idx[2]] = 1e-30
    with pytest.raises(AssertionError, match="saturated"):
        L.accept_loss(bad, c64, c32, name=None)


# ------------------------------------------------------------------------------------------------ guard references
def test_guard_references_on_hand_written_vectors():
    y = torch.tensor([0, 9, -1, 10, 2 ** 40, -2 ** 40, 5], dtype=torch.int64)
    t = torch.tensor([0, 999, 1000, -1, 3, 2 ** 40, -2 ** 40], dtype=torch.int64)
    ys, ts, by, bt = L.guard_inputs(y, t, 10, 1000)
    assert ys.tolist() == [0, 9, 0, 9, 9, 0, 5] and by == 4
    assert ts.tolist() == [0, 999, 999, 0, 3, 999, 0] and bt == 4
    ys, ts, by, bt = L.guard_inputs(ys, ts, 10, 1000)
    assert (by, bt) == (0, 0)
    ok = torch.tensor([1.0, 3.4028234663852886e38, 1e-45, -0.0])
    nan, inf = torch.tensor([1.0, float("nan")]), torch.tensor([-float("inf"), 0.0])
    assert L.guard_finite([ok, None, None, None], None) == (0, 0)
    assert L.guard_finite([ok[:2], nan, None, None], None) == (1, 0)
    assert L.guard_finite([ok[:2], nan, inf, nan], torch.tensor([1.0, float("nan")])) == (1, 0)      # one per call; only stats[0] counts
    assert L.guard_finite([ok[:2], None, inf, None], torch.tensor([float("inf")])) == (1, 1)
    assert L.guard_finite([ok], torch.tensor([float("nan")])) == (0, 1)


# ------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("n,C,H,W,p", L.LAYOUT_SHAPES)
def test_patchify_unpatchify_round_trips(n, C, H, W, p):
    g = torch.Generator().manual_seed(H * W + p)
    img = torch.randn(n, C, H, W, generator=g)
    K, T = C * p * p, (H // p) * (W // p)
    rows = L.patchify(img, p, 1)
    assert rows.shape == (n * T, K) and rows.dtype == torch.bfloat16
    assert torch.equal(L.unpatchify(rows.float(), n, C, H, W, p), img.to(torch.bfloat16).float())
    assert torch.equal(L.unpatchify(L.patchify(img, p, 1).float(), n, C, H, W, p).to(torch.bfloat16), img.to(torch.bfloat16))
    tok = torch.randn(n * T, K, generator=g)
    assert torch.equal(L.patchify(L.unpatchify(tok, n, C, H, W, p), p, 1), tok.to(torch.bfloat16))
    # the channel-first order is Conv2d(kernel = stride = p)'s im2col: the same rows, columns regrouped
    a, b = L.patchify(img, p, 0), L.patchify(img, p, 1)
    assert torch.equal(a.view(-1, C, p * p).transpose(1, 2).reshape(-1, K), b)
    w = torch.randn(5, C, p, p, generator=g).to(torch.bfloat16).float()
    conv = torch.nn.functional.conv2d(img.to(torch.bfloat16).double(), w.double(), stride=p).flatten(2).transpose(1, 2).reshape(n * T, 5)
    assert float((a.double() @ w.double().view(5, -1).t() - conv).abs().max()) <= 1e-12 * float(conv.abs().max())


# ------------------------------------------------------------------------------------------------ sampling step and DDPM restatements
def test_p_sample_and_cfg_restatements_agree_with_the_oracle():
    from oracle import diffusion_ref as dref
    tabs = dref.DiffusionTables(1000)
    g = torch.Generator().manual_seed(4)
    n, C = 5, 4
    x = torch.randn(n, C, 6, 6, generator=g)
    out = torch.randn(n, 2 * C, 6, 6, generator=g)
    noise = torch.randn(n, C, 6, 6, generator=g)
    t = torch.tensor([0, 1, 500, 999, 0])
    for clip in (False, True):
        want = dref.p_sample(tabs, lambda xx, ts, **kw: out, x, t, clip_denoised=clip, noise=noise)
        got, px = L.p_sample(x, out, t, TAB, noise, clip, F64)
        s32, p32 = L.p_sample(x, out, t, TAB, noise, clip, F32)
        R.bound32(want["sample"], got, s32)
        R.bound32(want["pred_xstart"], px, p32)
    o = torch.randn(6, 8, 5, generator=g)
    half, s = 3, 1.5
    eps, rest = o[:, :3], o[:, 3:]                                   # DiT/models.py:258-266
    ce, ue = eps[:half], eps[half:]
    h = ue + s * (ce - ue)
    want = torch.cat([torch.cat([h, h], 0), rest], 1)
    assert torch.equal(L.cfg_combine(o, 3, s, F32), want)


def test_ddpm_restatements_agree_with_the_oracle():
    from oracle import sfron_ref
    g = torch.Generator().manual_seed(9)
    n = 7
    x0, e = torch.rand(n, 3, 4, 4, generator=g) * 2 - 1, torch.randn(n, 3, 4, 4, generator=g)
    t = torch.tensor([0, 999, 1, 500, 37, 998, 2])
    b = sfron_ref.ddpm_get_betas()
    abar = sfron_ref.ddpm_alphas_cumprod_fp32(b)
    model = lambda x, tf: 0.5 * x
    per = sfron_ref.ddpm_loss_per_sample(model, x0, t, e, b).double()
    x_t = L.ddpm_q_sample(x0, e, t, abar, F64)
    got = L.ddpm_sample_loss(e, 0.5 * x_t, F64)
    assert float(((got - per).abs() / per).max()) < 1e-5
    for lambd in (0.5, 2.0):
        p = per.clone().requires_grad_(True)
        loss = sfron_ref.ddpm_adaptive_loss(p, lambd)
        loss.backward()
        coef, l, W = L.ddpm_loss_coef(per, 1, lambd, 1.0, n, F64)
        assert abs(float(l) - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
        assert float((coef / 2 - p.grad).abs().max()) <= 1e-12 * float(p.grad.abs().max())          # coef_i / 2 = d loss / d per_i
        # a batch split in two with the summed weights: the whole batch's coefficients and loss
        _, _, Wa = L.ddpm_loss_coef(per[:3], 1, lambd, 1.0, n, F64)
        _, _, Wb = L.ddpm_loss_coef(per[3:], 1, lambd, 1.0, n, F64)
        ca, la, _ = L.ddpm_loss_coef(per[:3], 1, lambd, 1.0, n, F64, wsum=Wa + Wb)
        cb, lb, _ = L.ddpm_loss_coef(per[3:], 1, lambd, 1.0, n, F64, wsum=Wa + Wb)
        assert float((torch.cat([ca, cb]) - coef).abs().max()) <= 1e-14 * float(coef.abs().max())
        assert abs(float(la + lb) - float(l)) <= 1e-14 * abs(float(l))
    coef, l, W = L.ddpm_loss_coef(per, 0, 0.0, 3.0, 4 * n, F64)
    assert float(W) == 4 * n and abs(float(l) - float(per.sum()) / (4 * n)) < 1e-12 and bool((coef == 6.0 / (4 * n)).all())
    d = L.ddpm_loss_bwd(e, 0.5 * x_t, coef, F64)
    o = (0.5 * x_t).clone().requires_grad_(True)
    (3.0 * L.ddpm_sample_loss(e, o, F64).sum() / (4 * n)).backward()
    assert float((d - o.grad).abs().max()) <= 1e-14 * float(d.abs().max())
