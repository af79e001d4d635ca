"""CPU: the reference of tests/test_gpu_dit_rows.py is independent of the kernels and its bounds can fail.

  * every float64 restatement in tests/dit_rows_ref.py against torch autograd in float64 on the reference model's own expression
    (F.layer_norm, F.silu, nn.Embedding-style indexing, index_add_), to 1e-12;
  * at every shape the GPU file runs, the float32 restatement alone passes bound_bf16 -- the 0.2 % cap is reachable;
  * the host-side form selection the shape lists rely on (sfron_rows_per_chunk, the RPW choice of the forward launcher);
  * the bounds reject an LN with eps 1e-5 and a modulate that reads the next sample's scale row (the first passes rtol = atol = 1e-2);
  * guarded() sees a write into any guard region."""
import math

import pytest
import torch
import torch.nn.functional as F

import dit_rows_ref as R

F64, F32 = torch.float64, torch.float32
TIGHT = 1e-12


def near(a, b, what):
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert err <= TIGHT * max(1.0, float(b.abs().max())), (what, err)


@pytest.mark.parametrize("B,T,D", [(2, 64, 128), (3, 5, 144), (2, 12, 4), (1, 33, 1280)])
@pytest.mark.parametrize("shifted", [False, True])
def test_row_restatements_equal_autograd(B, T, D, shifted):
    i = R.row_inputs(B, T, D, shifted)
    rows = 1 if T % 2 else 2 if T % 4 else 4
    x = i["x"].double().requires_grad_(True)
    sh, sc = i["shift"].double().requires_grad_(True), i["scale"].double().requires_grad_(True)
    out = F.layer_norm(x, (D,), eps=1e-6).view(B, T, D) * (1 + sc.unsqueeze(1)) + sh.unsqueeze(1)      # modulate(norm(x), shift, scale)
    d_out = i["d_out"].double()
    out.backward(d_out.view(B, T, D))
    got, mean, rstd = R.ln_modulate_fwd(i["x"], i["shift"], i["scale"], T, F64)
    near(got, out.detach().view(B * T, D), "out")
    near(mean, i["x"].double().mean(1), "mean")
    near(rstd, 1.0 / torch.sqrt(i["x"].double().var(1, unbiased=False) + 1e-6), "rstd")
    dx, ps, pc = R.ln_modulate_bwd(i["d_out"], i["x"], i["scale"], T, rows, F64)
    near(dx, x.grad, "dx")
    near(R.sample_sums(ps, B), sh.grad, "d shift")
    near(R.sample_sums(pc, B), sc.grad, "d scale")
    near(ps, d_out.view(-1, rows, D).sum(1), "p_shift chunks")
    # gate: y = x + gate.unsqueeze(1) * branch
    br = i["branch"].double().requires_grad_(True)
    gt = i["gate"].double().requires_grad_(True)
    dy = i["dx0"].double()
    (gt.unsqueeze(1) * br.view(B, T, D)).backward(dy.view(B, T, D))
    db, pg, pd = R.gate_bwd(i["dx0"], i["branch"], i["gate"], T, rows, F64)
    near(db, br.grad, "d_branch")
    near(R.sample_sums(pg, B), gt.grad, "d gate")
    near(R.sample_sums(pd, B), dy.view(B, T, D).sum(1), "sum dy")
    # fused: the gate backward reads dx0 + dLN
    for acc in (0, 1):
        fx, fs, fc, fb, fg, fd = R.ln_gate_bwd(i["d_out"], i["x"], i["scale"], i["dx0"], acc, i["branch"], i["gate"], T, rows, F64)
        want_dx = x.grad + (dy if acc else 0.0)
        near(fx, want_dx, "fused dx")
        near(fb, want_dx * gt.detach()[R.sample_of_row(B * T, T)], "fused d_branch")
        near(R.sample_sums(fg, B), (want_dx * br.detach()).view(B, T, D).sum(1), "fused d gate")
        near(fd, want_dx.view(-1, rows, D).sum(1), "fused p_dy")
        near(fs, ps, "fused p_shift")
        near(fc, pc, "fused p_scale")


def test_conditioning_restatements_equal_autograd():
    g = torch.Generator().manual_seed(3)
    n, D, nc = 37, 20, 10
    t_emb = torch.randn(n, D, generator=g)
    table = torch.randn(nc + 1, D, generator=g)
    y = torch.randint(0, nc, (n,), generator=g)
    y[3], y[4], y[5] = -1, nc, 2 ** 40
    drop = (torch.rand(n, generator=g) < 0.3).to(torch.uint8)
    lab = R.labels_used(y, drop, nc)
    assert lab[3] == nc and lab[4] == nc and lab[5] == nc and bool((lab[drop.bool()] == nc).all())
    assert torch.equal(R.labels_used(y[6:], None, nc), y[6:])
    tab = table.double().requires_grad_(True)
    te = t_emb.double().requires_grad_(True)
    c_ref = te + F.embedding(lab, tab)                       # LabelEmbedder + c = t + y
    d_silu = torch.randn(n, D, generator=g).double()
    F.silu(c_ref).backward(d_silu)
    c, sc = R.cond_fwd(t_emb, table, y, drop, nc, F64)
    near(c, c_ref.detach(), "c")
    near(sc, F.silu(c_ref.detach()), "silu_c")
    t0 = torch.randn(nc + 1, D, generator=g)
    d_c, d_tab = R.cond_bwd(d_silu, c, y, drop, nc, t0, F64)
    near(d_c, te.grad, "d_c")
    near(d_tab, t0.double() + tab.grad, "d_table")
    x = torch.linspace(-30, 30, 601).double().requires_grad_(True)
    F.silu(x).sum().backward()
    near(R.silu(x.detach(), F64), F.silu(x.detach()), "silu")
    near(R.silu_grad(x.detach(), F64), x.grad, "silu'")


def test_timestep_embedding_restatement():
    from oracle import dit_ref
    t = torch.tensor([0, 1, 2, 37, 500, 999])
    for dim in (64, 256):
        want = dit_ref.TimestepEmbedder.timestep_embedding(t, dim)         # the reference's fp32 expression
        assert torch.equal(R.timestep_embed(t, dim, F32), want)
        half = dim // 2
        args = (t[:, None].float() * torch.exp(-math.log(10000) * torch.arange(half, dtype=F32) / half)[None]).double()
        near(R.timestep_embed(t, dim, F64), torch.cat([torch.cos(args), torch.sin(args)], -1), "embedding")


def test_reduction_restatements():
    g = torch.Generator().manual_seed(5)
    P = torch.randn(5, 7, 12, generator=g)
    w = torch.randn(5, 12, generator=g)
    near(R.weighted_reduce(P, w, F64), torch.einsum("gc,gjc->c", w.double(), P.double()), "weighted_reduce")
    near(R.colsum(P[0], F64), P[0].double().sum(0), "colsum")
    layers, B, D = 3, 2, 8
    ldg, gstride, gwhich = layers * 6 * D, 6 * D, 3 * D
    gate = torch.randn(B, ldg, generator=g)
    S = torch.randn(layers, 2, B, D, generator=g)
    got = R.gated_bias_grads(S, gate.reshape(-1)[2 * D:], ldg, gstride, gwhich, layers, B, D, F64)
    gv = gate.double().view(B, layers, 6, D)
    want = torch.stack([torch.stack([(gv[:, l, 2 + 3 * which] * S[l, which].double()).sum(0) for which in range(2)]) for l in range(layers)])
    near(got, want, "gated_bias_grads")


# ------------------------------------------------------------------------------------------------ the cap is reachable
@pytest.mark.parametrize("B,T,D", R.FWD_SHAPES)
def test_float32_restatement_meets_the_bf16_cap_forward(B, T, D):
    for shifted in (False, True):
        i = R.row_inputs(B, T, D, shifted)
        o64, m64, r64 = R.ln_modulate_fwd(i["x"], i["shift"], i["scale"], T, F64)
        o32, m32, r32 = R.ln_modulate_fwd(i["x"], i["shift"], i["scale"], T, F32)
        R.bound_bf16(o32.to(torch.bfloat16), o64, o32)
        R.bound32(m32, m64, m32)
        R.bound32(r32, r64, r32)
        R.check_e4m3(o32.mul(8.0).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8), o64, o32, 8.0)


@pytest.mark.parametrize("T,D", R.BWD_SHAPES)
def test_float32_restatement_meets_the_bf16_cap_backward(T, D):
    B = 3
    rows = R.ROWS_PER_CHUNK[T]
    i = R.row_inputs(B, T, D)
    a64 = R.ln_gate_bwd(i["d_out"], i["x"], i["scale"], i["dx0"], 1, i["branch"], i["gate"], T, rows, F64)
    a32 = R.ln_gate_bwd(i["d_out"], i["x"], i["scale"], i["dx0"], 1, i["branch"], i["gate"], T, rows, F32)
    R.bound_bf16(a32[3].to(torch.bfloat16), a64[3], a32[3])
    g64, g32 = R.gate_bwd(i["dx0"], i["branch"], i["gate"], T, rows, F64), R.gate_bwd(i["dx0"], i["branch"], i["gate"], T, rows, F32)
    R.bound_bf16(g32[0].to(torch.bfloat16), g64[0], g32[0])


def test_float32_restatement_meets_the_bf16_cap_conditioning():
    g = torch.Generator().manual_seed(11)
    for n in (1, 5, 32, 33, 70):
        for D in (4, 128, 300, 1152):
            t_emb, table = torch.randn(n, D, generator=g), torch.randn(11, D, generator=g)
            y = torch.randint(0, 10, (n,), generator=g)
            R.bound_bf16(R.cond_fwd(t_emb, table, y, None, 10, F32)[1].to(torch.bfloat16), R.cond_fwd(t_emb, table, y, None, 10, F64)[1],
                         R.cond_fwd(t_emb, table, y, None, 10, F32)[1])
    for n in (1, 255, 257, 70000):
        x = torch.rand(n, generator=g) * 60 - 30
        dy = torch.randn(n, generator=g)
        R.bound_bf16(R.silu(x, F32).to(torch.bfloat16), R.silu(x, F64), R.silu(x, F32))
        d64, d32 = dy.double() * R.silu_grad(x, F64), dy * R.silu_grad(x, F32)
        R.bound_bf16(d32.to(torch.bfloat16), d64, d32)
    t = torch.tensor([0, 1, 2, 37, 500, 999])
    for dim in (64, 256):
        R.bound_bf16(R.timestep_embed(t, dim, F32).to(torch.bfloat16), R.timestep_embed(t, dim, F64), R.timestep_embed(t, dim, F32))


# ------------------------------------------------------------------------------------------------ host-side form selection
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from sfron import _lib
    return _lib.lib()


def test_rows_per_chunk_plans_the_shape_lists_rely_on(L):
    """pick_chunk (csrc/norm.hip): 8 / 4 / 2 / 1 rows per wave with the LDS combine (32 / 16 / 8 / 4 rows per chunk), 2 / 1 rows per wave
    without it.  If this fails after a retune of pick_chunk, update BWD_SHAPES in tests/dit_rows_ref.py so that every plan is still reached."""
    for T, want in zip((256, 64, 48, 24, 12, 6, 5, 1), (32, 16, 16, 8, 4, 2, 1, 1)):
        assert L.sfron_rows_per_chunk(T) == want, (T, L.sfron_rows_per_chunk(T), want)
    for T, _ in R.BWD_SHAPES:
        assert L.sfron_rows_per_chunk(T) == R.ROWS_PER_CHUNK[T]
    assert {R.ROWS_PER_CHUNK[T] for T, _ in R.BWD_SHAPES} == {32, 16, 8, 4, 2, 1}


def test_forward_shape_list_reaches_every_rpw_template():
    for B, T, D in R.FWD_SHAPES:
        assert R.fwd_rpw(B * T, T) == R.FWD_RPW[(B, T, D)]
        assert D % 4 == 0 and D <= 1280
    assert sorted(set(R.FWD_RPW.values())) == [1, 2, 4]
    assert (1366 * 6) % 8 == 4 and (683 * 12) % 16 == 4           # a half-idle last workgroup, a tail


# ------------------------------------------------------------------------------------------------ the bounds can fail
def test_bounds_reject_a_wrong_epsilon_and_a_wrong_sample_row():
    B, T, D = 3, 16, 144
    i = R.row_inputs(B, T, D)
    o64, m64, r64 = R.ln_modulate_fwd(i["x"], i["shift"], i["scale"], T, F64)
    o32, m32, r32 = R.ln_modulate_fwd(i["x"], i["shift"], i["scale"], T, F32)
    # eps 1e-5: rstd moves by 4.5e-6 / var relative (var = 4: 19 fp32 ulps) -- past bound32, far inside rtol = atol = 1e-2
    oe, _, re = R.ln_modulate_fwd(i["x"], i["shift"], i["scale"], T, F32, eps=1e-5)
    with pytest.raises(AssertionError):
        R.bound32(re, r64, r32)
    torch.testing.assert_close(oe, o64.float(), rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(re, r64.float(), rtol=1e-3, atol=1e-3)
    # ... and on rows of standard deviation 0.2 (var 0.04: rstd and every output move by 1.1e-4 relative, a twentieth of a bf16 step:
    # about one element in twenty rounds the other way) past bound_bf16's share cap too, still inside 1e-2
    xs = (i["x"] - 0.3) * 0.1 + 0.3
    s64, s32 = R.ln_modulate_fwd(xs, i["shift"], i["scale"], T, F64)[0], R.ln_modulate_fwd(xs, i["shift"], i["scale"], T, F32)[0]
    se = R.ln_modulate_fwd(xs, i["shift"], i["scale"], T, F32, eps=1e-5)[0]
    R.bound_bf16(s32.to(torch.bfloat16), s64, s32)
    with pytest.raises(AssertionError):
        R.bound_bf16(se.to(torch.bfloat16), s64, s32)
    torch.testing.assert_close(se, s64.float(), rtol=1e-2, atol=1e-2)
    # sample b + 1's scale row
    ow, _, _ = R.ln_modulate_fwd(i["x"], i["shift"], i["scale"].roll(-1, 0), T, F32)
    with pytest.raises(AssertionError):
        R.bound_bf16(ow.to(torch.bfloat16), o64, o32)
    rows = 16
    d64 = R.ln_modulate_bwd(i["d_out"], i["x"], i["scale"], T, rows, F64)[0]
    d32 = R.ln_modulate_bwd(i["d_out"], i["x"], i["scale"], T, rows, F32)[0]
    with pytest.raises(AssertionError):
        R.bound32(R.ln_modulate_bwd(i["d_out"], i["x"], i["scale"].roll(-1, 0), T, rows, F32)[0], d64, d32)
    with pytest.raises(AssertionError):
        R.bound32(R.ln_modulate_bwd(i["d_out"], i["x"], i["scale"], T, rows, F32, eps=1e-5)[0], d64, d32)
    # one row out of 48 with the wrong scale row is enough
    one = o32.clone()
    one[T - 1] = ow[T - 1]
    with pytest.raises(AssertionError):
        R.bound_bf16(one.to(torch.bfloat16), o64, o32)


def test_guarded_sees_writes_outside_the_view():
    for dtype in (torch.float32, torch.bfloat16, torch.uint8, torch.int32):
        v, check = R.guarded((3, 5, 8), dtype, ld=12, device="cpu")
        assert v.shape == (3, 5, 8) and v.stride() == (60, 12, 1) and v.data_ptr() % 16 == 0
        R.untouched(check)
        v.copy_(torch.ones(3, 5, 8).to(dtype))
        check()
        with pytest.raises(AssertionError):
            R.untouched(check)
        flat = check.full
        pad = R.GUARD_BYTES // v.element_size()
        for at in (pad - 1, pad + 8, pad + 3 * 5 * 12, flat.numel() - 1, 0):        # before, a row gap, just after, the far ends
            keep = flat[at].clone()
            flat[at] = 0
            with pytest.raises(AssertionError):
                check()
            flat[at] = keep
        check()
    d, check = R.guarded((7,), torch.float32, device="cpu")
    assert d.shape == (7,) and bool(torch.isnan(d).all())
