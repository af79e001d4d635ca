"""CPU: the reference of tests/test_gpu_unet_rows.py is independent of the kernels, and its bounds are reachable.

  * every float64 restatement in tests/unet_rows_ref.py against torch's own operator or autograd in float64 (F.layer_norm, F.gelu,
    torch.softmax, permute / cat, index_select / index_add_), to 1e-12;
  * layernorm_rows_per_block against hand-worked values (and against the library's own function);
  * at every shape the GPU file runs, the float32 restatement alone passes bound_bf16 on exactly the element sets the GPU file caps;
  * the mask argument of bound_bf16: the cap is taken over the masked elements, the error bound over all of them;
  * the dropout restatement against a scalar, one-element-at-a-time evaluation of the same draw in Python integers."""
import math

import pytest
import torch
import torch.nn.functional as F

import unet_rows_ref as U

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
TIGHT = 1e-12


def near(a, b, what):
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert err <= TIGHT * max(1.0, float(b.abs().max())), (what, err)


# ------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("rows,D,eps", [(37, 260, 1e-5), (5, 63, 1e-6), (40, 8, 1e-5)])
def test_layernorm_restatement_equals_autograd(rows, D, eps):
    i = U.ln_inputs(rows, D)
    x = i["x"].double().requires_grad_(True)
    gm, bt = i["gamma"].double().requires_grad_(True), i["beta"].double().requires_grad_(True)
    y = F.layer_norm(x, (D,), gm, bt, eps)
    y.backward(i["dy"].double())
    got, mean, rstd = U.layernorm_fwd(i["x"], i["gamma"], i["beta"], eps, F64)
    near(got, y.detach(), "y")
    near(mean, i["x"].double().mean(1), "mean")
    near(rstd, 1.0 / torch.sqrt(i["x"].double().var(1, unbiased=False) + eps), "rstd")
    rpb = 16
    dx, pg, pb = U.layernorm_bwd(i["dy"], i["x"], i["gamma"], eps, None, 0, None, rpb, F64)
    near(dx, x.grad, "dx")
    assert pg.shape == (-(-rows // rpb), D)
    near(pg.sum(0), gm.grad, "d gamma")
    near(pb.sum(0), bt.grad, "d beta")
    near(pb[-1], i["dy"].double()[(pg.shape[0] - 1) * rpb:].sum(0), "the last, short block")
    near(pb[0], i["dy"].double()[:rpb].sum(0), "the first block")
    for acc, extra in ((1, None), (0, i["extra"]), (1, i["extra"])):
        want = x.grad + (i["dx0"].double() if acc else 0.0) + (extra.double() if extra is not None else 0.0)
        near(U.layernorm_bwd(i["dy"], i["x"], i["gamma"], eps, i["dx0"], acc, extra, rpb, F64)[0], want, f"dx acc={acc}")
    # float32: (dx_prev + extra) + gradient, in that order
    g32 = U.layernorm_bwd(i["dy"], i["x"], i["gamma"], eps, None, 0, None, rpb, F32)[0]
    assert torch.equal(U.layernorm_bwd(i["dy"], i["x"], i["gamma"], eps, i["dx0"], 1, i["extra"], rpb, F32)[0], (i["dx0"] + i["extra"]) + g32)


def test_layernorm_rows_per_block_hand_worked():
    for rows, want in ((1, 16), (37, 16), (8192, 16), (8193, 20), (8196, 20), (10240, 20), (10241, 24), (30720, 60), (30721, 64),
                       (30724, 64), (10 ** 7, 64)):
        assert U.layernorm_rows_per_block(rows) == want, (rows, U.layernorm_rows_per_block(rows), want)
    assert 8196 % 20 == 16 and 30724 % 64 == 4                # the short last blocks the GPU module relies on


def test_layernorm_rows_per_block_is_the_library_s():
    import __graft_entry__ as ge
    ge.build()
    from sfron import _lib
    L = _lib.lib()
    for rows in (1, 3, 37, 8192, 8193, 8196, 10240, 10241, 30720, 30721, 30724, 10 ** 7):
        assert L.sfron_layernorm_rows_per_block(rows) == U.layernorm_rows_per_block(rows), rows


@pytest.mark.parametrize("rows,F_", [(7, 5), (3, 1028)])
def test_geglu_restatement_equals_autograd(rows, F_):
    h, d_out = U.geglu_inputs(rows, F_)
    hd = h.double().requires_grad_(True)
    out = hd[:, :F_] * F.gelu(hd[:, F_:])
    out.backward(d_out.double())
    near(U.geglu_fwd(h, F64), out.detach(), "geglu")
    near(U.geglu_bwd(d_out, h, F64), hd.grad, "geglu backward")
    gate = h[:, F_:].reshape(-1)
    assert torch.equal(gate[:22], torch.tensor(U.GEGLU_TAILS * 2))


@pytest.mark.parametrize("rows,n,nv,scale", U.SOFTMAX_CASES + [U.SOFTMAX_LARGE])
def test_softmax_restatement_equals_torch(rows, n, nv, scale):
    s, dp = U.softmax_inputs(rows, n, nv, scale, large=(rows, n, nv, scale) == U.SOFTMAX_LARGE)
    sc = float(torch.tensor(scale, dtype=F32))
    z = (s.double()[:, :nv] * sc).requires_grad_(True)
    p = torch.softmax(z, 1)
    got = U.softmax_fwd(s, nv, scale, F64)
    near(got[:, :nv], p.detach(), "softmax")
    assert bool((got[:, nv:] == 0).all())
    p16 = U.to_bf16(got)
    ds = U.softmax_bwd(p16, dp, scale, F64)
    assert bool((ds[:, nv:] == 0).all())
    # d/ds of sum(dp * softmax(scale s)) at exact probabilities
    p.backward(dp.double()[:, :nv])
    near(U.softmax_bwd(got, dp, scale, F64)[:, :nv], z.grad * sc, "softmax backward")


def test_layout_restatements():
    for B, C, HW in U.LAYOUT_SHAPES:
        x = torch.arange(B * C * HW, dtype=F32).view(B, C, HW) + 1
        for c_pad in (C, C + 1, (C + 7) // 8 * 8):
            want = torch.cat([x.permute(0, 2, 1).reshape(B * HW, C), torch.zeros(B * HW, c_pad - C)], 1)
            assert torch.equal(U.nchw_to_rows(x, c_pad), want)
            assert torch.equal(U.rows_to_nchw(U.nchw_to_rows(x, c_pad) + (torch.arange(c_pad) >= C) * 99.0, B, C, HW), x)
    x = U.tie_values(7, 260, 3)
    lo = x.view(torch.int32) & 0xFFFF
    assert int((lo == 0x8000).sum()) > 400 and int((lo == 0x8001).sum()) > 100 and int((lo == 0x7FFF).sum()) > 100
    up = (U.cast_rows(x).view(torch.int16).int() & 0xFFFF) != ((x.view(torch.int32) >> 16) & 0xFFFF)
    ties = lo == 0x8000
    assert 0.3 < float(up[ties].float().mean()) < 0.7, "ties go to even: about half of them up"
    assert bool(up[lo == 0x8001].all()) and not bool(up[lo == 0x7FFF].any())
    a, b = torch.tensor([1.0, 3.0, 1e-3]), torch.tensor([2.0, 3.0 + 2 ** -21, 7.0])
    assert torch.equal(U.axpby(a, b, 8.5, -7.5), a * 8.5 + b * -7.5)
    d = torch.randn(2, 6, 4, 3)
    near(U.pool2_sum(d, F64), 4 * F.avg_pool2d(d.double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1), "pool2_sum")
    near(U.sample_colsum(d.view(2 * 24, 3), 2, 24, F64), d.double().sum((1, 2)), "sample_colsum")


def test_class_embedding_restatement():
    g = torch.Generator().manual_seed(4)
    nc, D, n = 10, 12, 9
    table, null = torch.randn(nc, D, generator=g), torch.randn(D, generator=g)
    c = torch.tensor([3, 3, -1, nc, 0, 9, 5, 3, 2])
    keep = torch.tensor([1, 0, 1, 1, 1, 1, 0, 1, 1], dtype=torch.uint8)
    for kp in (None, keep):
        use = U.class_embed_used(c, kp, nc)
        assert not use[2] and not use[3] and (kp is None or (not use[1] and not use[6]))
        both = torch.cat([table, null[None]])                        # the null row as row n_classes of one table
        idx = torch.where(use, c, torch.full_like(c, nc))
        assert torch.equal(U.class_embed_fwd(table, null, c, kp, nc), both.index_select(0, idx))
        d = torch.randn(n, D, generator=g)
        t0 = torch.randn(nc, D, generator=g)
        dt, dn = U.class_embed_bwd(d, c, kp, nc, t0, F64)
        want = torch.cat([t0.double(), torch.zeros(1, D, dtype=F64)]).index_add_(0, idx, d.double())
        near(dt, want[:nc], "d_table")
        near(dn, want[nc], "d_null")


def test_timestep_embedding_restatement():
    from oracle import ddpm_ref
    fn = ddpm_ref.timestep_embedding                    # the oracle's copy of get_timestep_embedding, fp32
    t = torch.tensor(U.TEMB_T_SMALL + U.TEMB_T_LARGE)
    for dim in U.TEMB_DIMS:
        e = U.ddpm_timestep_embed(t, dim, F64)
        half = dim // 2
        f = torch.exp(-math.log(10000) * torch.arange(half, dtype=F64) / (half - 1))
        near(e[:, :half], torch.sin(t.double()[:, None] * f), "sin half")
        near(e[:, half:2 * half], torch.cos(t.double()[:, None] * f), "cos half")
        assert e.shape == (len(t), dim) and (dim % 2 == 0 or bool((e[:, -1] == 0).all()))
        assert torch.equal(U.ddpm_timestep_embed(t, dim, F32), fn(t, dim))


def test_dropout_restatement_against_a_scalar_evaluation():
    M = (1 << 64) - 1
    assert U.dropout_thresh(0.0) == 0 and U.dropout_thresh(0.5) == 32768 and U.dropout_thresh(0.1) == 6554 and U.dropout_thresh(0.999) == 65470
    for seed, counter, salt, n, p in ((0x1234567890ABCDEF, 0, 1, 13, 0.5), (2 ** 64 - 3, 5, 77, 1001, 0.1), (7, 5, 2 ** 40 + 1, 5, 0.999)):
        base = seed ^ (counter * 0x9E3779B97F4A7C15 & M) ^ (salt * 0xD1B54A32D192ED03 & M)
        want = []
        for i in range(n):
            z = (base + (i // 4 + 1) * 0x9E3779B97F4A7C15) & M
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
            z ^= z >> 31
            want.append(int(((z >> (16 * (i % 4))) & 0xFFFF) >= U.dropout_thresh(p)))
        assert U.dropout_mask(seed, counter, salt, n, p).tolist() == want
    assert bool(U.dropout_mask(1, 0, 0, 1001, 0.0).all())
    keep = float(U.dropout_mask(1, 0, 0, 400000, 0.1).float().mean())
    assert abs(keep - 0.9) < 4 * math.sqrt(0.09 / 400000)


# ------------------------------------------------------------------------------------------------ the cap is reachable
@pytest.mark.parametrize("rows,D", U.LN_SHAPES + [(37, D) for D in U.LN_MISALIGNED_D])
def test_float32_layernorm_meets_the_cap(rows, D):
    for eps in U.LN_EPS:
        i = U.ln_inputs(rows, D)
        y64, m64, r64 = U.layernorm_fwd(i["x"], i["gamma"], i["beta"], eps, F64)
        y32, m32, r32 = U.layernorm_fwd(i["x"], i["gamma"], i["beta"], eps, F32)
        U.bound_bf16(y32.to(BF16), y64, y32)
        U.bound32(m32, m64, m32)
        U.bound32(r32, r64, r32)


def test_float32_layernorm_meets_the_cap_shifted():
    i = U.ln_inputs(37, 260, shifted=True)
    y64, m64, r64 = U.layernorm_fwd(i["x"], i["gamma"], i["beta"], 1e-5, F64)
    y32, m32, r32 = U.layernorm_fwd(i["x"], i["gamma"], i["beta"], 1e-5, F32)
    # x - mean carries the fp32 rounding of a mean of 300 (1.5e-5 of a value near 1): the float32 restatement alone differs from
    # bf16(ref64) on 1 - 2 % of y here, so this case is held to the error bound alone, here and on the GPU
    none = torch.zeros(y64.shape, dtype=torch.bool)
    with pytest.raises(AssertionError, match="differ from bf16"):
        U.bound_bf16(y32.to(BF16), y64, y32)
    U.bound_bf16(y32.to(BF16), y64, y32, cap_mask=none)
    U.bound32(m32, m64, m32)
    U.bound32(r32, r64, r32)
    # what the case is for: E[x^2] - mean^2 in fp32 is useless here (x^2 ~ 9e4 carries 2^-8 absolute, the variance is 1)
    x = i["x"]
    one_pass = 1.0 / torch.sqrt(((x * x).mean(1) - x.mean(1) ** 2).clamp_min(0) + 1e-5)
    with pytest.raises(AssertionError):
        U.bound32(one_pass, r64, r32)


@pytest.mark.parametrize("F_,rows,_mis", U.GEGLU_VECTOR + U.GEGLU_PLAIN)
def test_float32_geglu_meets_the_cap_on_the_capped_elements(F_, rows, _mis):
    h, d_out = U.geglu_inputs(rows, F_)
    mf, mb = U.geglu_cap_masks(h)
    o64, o32 = U.geglu_fwd(h, F64), U.geglu_fwd(h, F32)
    assert bool(torch.isfinite(o32).all())
    U.bound_bf16(o32.to(BF16), o64, o32, cap_mask=mf)
    b64, b32 = U.geglu_bwd(d_out, h, F64), U.geglu_bwd(d_out, h, F32)
    assert bool(torch.isfinite(b32).all())
    U.bound_bf16(b32.to(BF16), b64, b32, cap_mask=mb)


@pytest.mark.parametrize("rows,n,nv,scale", U.SOFTMAX_CASES)
def test_float32_softmax_meets_the_cap(rows, n, nv, scale):
    s, dp = U.softmax_inputs(rows, n, nv, scale)
    z = s[:, :nv].double() * scale
    assert float((z.max(1).values - z.min(1).values).max()) <= U.SOFTMAX_CAP_SPREAD        # the cases the cap is applied to
    p64, p32 = U.softmax_fwd(s, nv, scale, F64), U.softmax_fwd(s, nv, scale, F32)
    U.bound_bf16(p32.to(BF16), p64, p32)
    p16 = p32.to(BF16)
    U.bound_bf16(U.softmax_bwd(p16, dp, scale, F32).to(BF16), U.softmax_bwd(p16, dp, scale, F64), U.softmax_bwd(p16, dp, scale, F32))


def test_float32_softmax_large_logits_meet_the_error_bound():
    rows, n, nv, scale = U.SOFTMAX_LARGE
    s, _ = U.softmax_inputs(rows, n, nv, scale, large=True)
    assert float(s[:, :nv].abs().max()) > 60
    p64, p32 = U.softmax_fwd(s, nv, scale, F64), U.softmax_fwd(s, nv, scale, F32)
    U.bound_bf16(p32.to(BF16), p64, p32, cap_mask=torch.zeros(p64.shape, dtype=torch.bool))
    assert bool(((p32.to(BF16).float().sum(1) - 1).abs() <= 2 ** -6).all())


@pytest.mark.parametrize("dim", U.TEMB_DIMS)
def test_float32_timestep_embedding_meets_the_cap_on_small_t(dim):
    t = torch.tensor(U.TEMB_T_SMALL + U.TEMB_T_LARGE)
    e64, e32 = U.ddpm_timestep_embed(t, dim, F64), U.ddpm_timestep_embed(t, dim, F32)
    mask = (t <= 7)[:, None].expand(-1, dim)
    U.bound_bf16(e32.to(BF16), e64, e32, cap_mask=mask)
    small = torch.tensor(U.TEMB_T_SMALL)
    U.bound_bf16(U.ddpm_timestep_embed(small, dim, F32).to(BF16), U.ddpm_timestep_embed(small, dim, F64), U.ddpm_timestep_embed(small, dim, F32))


def test_bound_bf16_mask_caps_the_masked_elements_only():
    g = torch.Generator().manual_seed(9)
    ref64 = torch.randn(40, 50, generator=g).double() + 3.0
    ref32 = (ref64 * (1 + 1e-7)).float()
    got = U.to_bf16(ref64).clone()
    one_up = (got.view(torch.int16) + 1).view(BF16)                 # one bf16 step: inside 2^-8 |ref| of the reference or just past it
    inside = (one_up.double() - ref64).abs() <= 2.0 ** -8 * ref64.abs()
    left = torch.zeros(40, 50, dtype=torch.bool)
    left[:, :25] = True
    move = inside & ~left
    assert int(move.sum()) > 0.01 * got.numel()
    got[move] = one_up[move]
    with pytest.raises(AssertionError, match="differ from bf16"):
        U.bound_bf16(got, ref64, ref32)
    U.bound_bf16(got, ref64, ref32, cap_mask=left)                  # the moved elements are outside the cap set ...
    with pytest.raises(AssertionError, match="differ from bf16"):
        U.bound_bf16(got, ref64, ref32, cap_mask=~left)
    bad = got.clone()
    bad[0, 30] = 7.0                                                # ... but still under the error bound
    with pytest.raises(AssertionError, match="elements past"):
        U.bound_bf16(bad, ref64, ref32, cap_mask=left)
    U.bound_bf16(got, ref64, ref32, cap_mask=torch.zeros(40, 50, dtype=torch.bool))
