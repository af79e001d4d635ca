"""GPU: the fp8 BACKWARD of BASELINE config 5 (engine.enable_fp8(backward=True), DiTSFRon(fp8=True, fp8_backward=True)): the four dgrads of
every block on v_mfma_scale_f32_16x16x128_f8f6f4 with an MX-scaled e4m3 dY (one E8M0 byte per 32 elements of a row) and a transposed copy of
the e4m3 weight shadow.  The rule restated here is the one include/sfron.h states:
  X = ceil(log2(amax / 448)) over a 32-block, clamped to [-127, 127], all-zero block -> -127; byte = X + 127; code = e4m3fn_RNE(x * 2^-X)."""
import copy
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"

CFG = dict(input_size=16, patch_size=2, in_channels=4, hidden_size=128, depth=2, num_heads=2, num_classes=10)     # 64 tokens; batch 4 -> M = 256


def _rel(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def mx_ref(x):
    """torch restatement of the MX rule on a [M][N] tensor (N % 32 == 0): (codes uint8 [M][N], scale bytes uint8 [M][N / 32], dequantised fp32)"""
    M, N = x.shape
    xb = x.float().reshape(M, N // 32, 32)
    amax = xb.abs().amax(dim=2).double()
    X = torch.where(amax > 0, torch.ceil(torch.log2(amax / 448.0)), torch.full_like(amax, -127.0)).clamp(-127, 127)
    s = torch.pow(2.0, -X).float()
    q = (xb * s[..., None]).to(torch.float8_e4m3fn)
    deq = q.float() / s[..., None]
    return q.view(torch.uint8).reshape(M, N), (X + 127).to(torch.uint8), deq.reshape(M, N)


def _lib():
    from sfron import _lib as L
    return L


def cast_mx8(x):
    L = _lib()
    M, N = x.shape
    q = torch.empty(M, N, dtype=torch.uint8, device=DEV)
    s = torch.empty(M, N // 32, dtype=torch.uint8, device=DEV)
    L.check(L.lib().sfron_cast_mx8(L.ptr(x), M, N, L.ptr(q), L.ptr(s), L.stream_ptr()), "cast_mx8")
    return q, s


def dgrad(A8, As, Bt8, w_scale, epilogue=0, tile=0, aux=None, want_partials=False):
    """sfron_fp8_dgrad: C[M][N] = MX(A) . Bt8[N][K]^T / w_scale"""
    L = _lib()
    M, K = A8.shape
    N = Bt8.shape[0]
    d = L.Fp8DgradDesc()
    C = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    ws = torch.tensor([w_scale], dtype=torch.float32, device=DEV)
    d.A, d.a_scales, d.B, d.M, d.N, d.K, d.w_scale = L.ptr(A8), L.ptr(As), L.ptr(Bt8), M, N, K, L.ptr(ws)
    d.epilogue, d.c_bf16, d.ldc_bf16, d.tile_hint = epilogue, L.ptr(C), N, tile
    out = dict(C=C)
    if aux is not None:
        out["C8"] = torch.empty(M, N, dtype=torch.uint8, device=DEV)
        out["Cs"] = torch.empty(M, N // 32, dtype=torch.uint8, device=DEV)
        d.aux, d.ldaux, d.c_e4m3, d.c_scales = L.ptr(aux), N, L.ptr(out["C8"]), L.ptr(out["Cs"])
        if want_partials:
            out["P"] = torch.empty(M // 256, N, dtype=torch.float32, device=DEV)
            d.col_partials = L.ptr(out["P"])
    rc = L.lib().sfron_fp8_dgrad(ctypes.byref(d), L.stream_ptr())
    torch.cuda.synchronize()
    out["rc"] = rc
    return out


def _heavy_rows(M, N, gen):
    x = torch.randn(M, N, generator=gen) * torch.exp(torch.randn(M, 1, generator=gen) * 3) * torch.randn(M, N, generator=gen).abs() ** 3
    x[0, :64] = 0.0                                           # all-zero blocks
    x[1, 32:64] = 0.0
    x[1, 40] = 3.0e38                                         # one huge value in a block
    x[2, :32] = torch.tensor([0.0, -0.0] * 16)                # +-0
    x[3, :32] = torch.randn(32, generator=gen) * 1e-39        # bf16 subnormals
    x[3, 32:64] = torch.randn(32, generator=gen) * 1e-39
    x[3, 40] = 1.0                                            # ... beside a normal value
    x[4, :32] = 448.0 * 2.0 ** torch.arange(-8, 8).repeat(2)  # amax exactly 448 * 2^X
    return x.to(torch.bfloat16)


@pytest.mark.parametrize("N", [1152, 3456])
def test_cast_mx8_bit_exact(N):
    gen = torch.Generator().manual_seed(N)
    x = _heavy_rows(64, N, gen)
    q, s = cast_mx8(x.to(DEV))
    wq, ws, _ = mx_ref(x)
    assert torch.equal(s.cpu(), ws)
    assert torch.equal(q.cpu(), wq)
    assert int(ws[0, 0]) == 0 and int(ws[4, 0]) == 127 + 7       # all-zero block -> X = -127; 448 * 2^7 -> X = 7


def test_mx_rule_hand_cases():
    x = torch.zeros(1, 32 * 4)
    x[0, 0] = 448.0           # X = 0, code 448 = 0x7E
    x[0, 32] = 452.0          # X = 1, 226 -> 224 = 0x76 (round to nearest even)
    x[0, 64] = 1.0            # ceil(log2(1 / 448)) = -8, 1 * 2^8 = 256 = 0x78
    q, s = cast_mx8(x.to(torch.bfloat16).to(DEV))
    assert s.cpu().tolist() == [[127, 128, 119, 0]]
    assert [q.cpu()[0, j].item() for j in (0, 32, 64)] == [0x7E, 0x76, 0x78]


def _exact_operands(M, N, K, gen):
    """e4m3 codes of small dyadic values (every product and partial sum exact in fp32) and a DIFFERENT scale byte per (row, 32-block)"""
    vals = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, -0.5, -1.0, -1.5, -2.0, 0.25, -0.25])
    a = vals[torch.randint(0, len(vals), (M, K), generator=gen)]
    b = vals[torch.randint(0, len(vals), (N, K), generator=gen)]
    X = ((torch.arange(M)[:, None] * 5 + torch.arange(K // 32)[None, :] * 3) % 13 - 6).to(torch.int64)     # -6 .. 6
    a8 = a.to(torch.float8_e4m3fn).view(torch.uint8)
    b8 = b.to(torch.float8_e4m3fn).view(torch.uint8)
    sA = (X + 127).to(torch.uint8)
    A = a * torch.pow(2.0, X.double()).float().repeat_interleave(32, dim=1)
    return a8, sA, b8, A, b


@pytest.mark.parametrize("M,N,K,tile", [(256, 128, 128, 8), (256, 144, 256, 9), (512, 1152, 384, 8), (512, 1152, 384, 9)])
def test_scaled_mfma_lane_map_exact(M, N, K, tile):
    """exact-integer data, one scale byte per (row, 32-block) that differs from its neighbours: a wrong lane <-> scale map changes products
    by powers of two -- the comparison is bit for bit, no tolerance"""
    gen = torch.Generator().manual_seed(M + N + K)
    a8, sA, b8, A, b = _exact_operands(M, N, K, gen)
    out = dgrad(a8.to(DEV), sA.to(DEV), b8.to(DEV), 1.0, tile=tile)
    assert out["rc"] == 0
    want = (A.double() @ b.double().T).float().to(torch.bfloat16)
    assert torch.equal(out["C"].cpu(), want)


@pytest.mark.parametrize("M,N,K,tile", [(8192, 1152, 3456, 0), (8192, 1152, 3456, 8), (8192, 1152, 1152, 9), (8192, 1152, 4608, 0),
                                        (2048, 768, 2304, 0), (2048, 768, 768, 0), (2048, 768, 3072, 0),      # DiT-B/4 batch 32 (config 2)
                                        (256, 128, 384, 8), (512, 288, 256, 9)])
def test_dgrad_bf16_vs_torch(M, N, K, tile):
    gen = torch.Generator().manual_seed(M + N + K + tile)
    dy = (torch.randn(M, K, generator=gen) * torch.exp(torch.randn(M, 1, generator=gen))).to(torch.bfloat16)
    w = torch.randn(K, N, generator=gen) * 0.02                     # W[out][in]
    from oracle import fp8_ref
    ws = fp8_ref.weight_scale(w)
    wt8 = fp8_ref.e4m3_bytes(w.T.contiguous(), ws)                  # transposed shadow [in][out]
    q, s = cast_mx8(dy.to(DEV))
    out = dgrad(q, s, wt8.to(DEV), ws, tile=tile)
    assert out["rc"] == 0
    _, _, dyq = mx_ref(dy)
    want = dyq.to(DEV) @ fp8_ref.q_e4m3(w, ws).to(DEV)
    e = _rel(out["C"].float(), want)
    print(f"dgrad {M}x{N}x{K} tile {tile}: rel {e:.2e}")
    assert e < 3e-3, e


@pytest.mark.parametrize("M,N,K,q", [(8192, 4608, 1152, True), (8192, 4608, 1152, False), (2048, 3072, 768, True), (256, 512, 128, False),
                                     (512, 256, 384, True)])
def test_dgrad_dgelu_vs_torch(M, N, K, q):
    """fc2 dgrad * GELU' (codes or bf16 pre-activation): d_hpre, its MX copy (= sfron_cast_mx8(d_hpre) bit for bit) and the fc1.bias partials"""
    from oracle import fp8_ref
    gen = torch.Generator().manual_seed(M + N + K + int(q))
    dy = (torch.randn(M, K, generator=gen) * 0.1).to(torch.bfloat16)
    w = torch.randn(K, N, generator=gen) * 0.02
    ws = fp8_ref.weight_scale(w)
    wt8 = fp8_ref.e4m3_bytes(w.T.contiguous(), ws)
    pre = (torch.randn(M, N, generator=gen) * 2).clamp(-8, 8)      # (the bf16 path's GELU' form, common.h gelu_tanh_grad4, is for |x| < ~10)
    if q:
        codes = torch.randint(0, 252, (M, N), generator=gen, dtype=torch.int64).to(torch.uint8)
        gp = codes.float() / 196.0 - 0.15
        aux = codes
    else:
        pre = pre.to(torch.bfloat16)
        p = pre.double()
        k0, k1 = math.sqrt(2.0 / math.pi), 0.044715
        th = torch.tanh(k0 * (p + k1 * p ** 3))
        gp = (0.5 * (1 + th) + 0.5 * p * (1 - th ** 2) * k0 * (1 + 3 * k1 * p ** 2)).float()
        aux = pre
    qa, sa = cast_mx8(dy.to(DEV))
    out = dgrad(qa, sa, wt8.to(DEV), ws, epilogue=8 if q else 4, aux=aux.to(DEV), want_partials=True)
    assert out["rc"] == 0
    _, _, dyq = mx_ref(dy)
    r = (dyq.to(DEV) @ fp8_ref.q_e4m3(w, ws).to(DEV)) * gp.to(DEV)
    e = _rel(out["C"].float(), r)
    q8, s8 = cast_mx8(out["C"])
    assert torch.equal(out["C8"], q8) and torch.equal(out["Cs"], s8)
    ep = _rel(out["P"], r.view(M // 256, 256, N).sum(dim=1))
    print(f"dgelu {M}x{N}x{K} q={q}: rel {e:.2e}, partials {ep:.2e}")
    assert e < 3e-3, e
    assert ep < 2e-5, ep


def test_dgrad_refuses_unsupported():
    L = _lib()
    a = torch.zeros(256, 128, dtype=torch.uint8, device=DEV)
    s = torch.zeros(256, 4, dtype=torch.uint8, device=DEV)
    b = torch.zeros(144, 128, dtype=torch.uint8, device=DEV)
    assert dgrad(a, s, b, 1.0, tile=8)["rc"] != 0                      # 144 is not a multiple of 128
    aux = torch.zeros(256, 144, dtype=torch.bfloat16, device=DEV)
    assert dgrad(a, s, b, 1.0, epilogue=4, aux=aux)["rc"] != 0         # MX output: 256 x 128 tiles only
    assert dgrad(a[:200], s[:200], b[:128], 1.0)["rc"] != 0             # M % 256


# ------------------------------------------------------------------ the DiT passes
def _model(cfg, batch, seed, std=0.05, backward=True):
    from oracle import dit_ref
    from sfron import dit
    torch.manual_seed(seed)
    ref = dit_ref.DiT(**cfg)
    dit_ref.randomize_zero_init(ref, std=std, seed=seed + 1)
    model = dit.DiT(batch_size=batch, **cfg)
    model.load_state_dict(ref.state_dict())
    model.engine.enable_fp8(backward=backward)
    return ref, model


def _w8t_consistent(eng):
    lay, c = eng.layout, eng.cfg
    D, Fh = c.hidden, c.mlp_hidden
    base = lay["blocks"] & ~255
    w8, w8t = eng.fp8["w8"], eng.fp8["w8t"]["t"]
    for l in range(c.depth):
        b = lay["blocks"] + l * lay["blk_stride"]
        for key, R, C in (("qkv_w", 3 * D, D), ("proj_w", D, D), ("fc1_w", Fh, D), ("fc2_w", D, Fh)):
            o = b + lay[key]
            if not torch.equal(w8[o:o + R * C].view(R, C).T.contiguous().flatten(), w8t[o - base:o - base + R * C]):
                return False
    return True


def test_transposed_shadow_equals_transpose_after_enable():
    _, model = _model(CFG, 4, seed=2)
    torch.cuda.synchronize()
    assert _w8t_consistent(model.engine)


@pytest.mark.parametrize("across", [False, True])
def test_transposed_shadow_is_fresh_at_every_backward_pass(across):
    """every writer of the e4m3 shadow (the re-quantising sweeps, the block sweep left in flight beside the next forward pass) is followed by
    the transpose before a backward pass reads it: checked at each of the six backward passes of three SFR-on iterations"""
    from sfron import data, diffusion, step
    _, model = _model(CFG, 4, seed=11)
    model.train()
    runner = step.DiTSFRon(model, diffusion.create_diffusion(""), lr=1e-3, forget_alpha=0.5, mask=None, fp8=True, fp8_backward=True,
                           forget_class=3)
    runner.sweep_across_steps = across
    eng = model.engine
    seen = []
    real = eng.backward_factored_ada

    def checked(*a, **k):
        r = real(*a, **k)
        torch.cuda.synchronize()
        seen.append(_w8t_consistent(model.engine))
        return r
    eng.backward_factored_ada = checked
    kw = dict(global_batch=4, num_classes=10, forget_class=3, input_size=16)
    w8_0 = eng.fp8["w8"].clone()
    for it in range(3):
        f, r = data.synthetic_batch(1, it, "forget", **kw), data.synthetic_batch(1, it, "remain", **kw)
        runner.step({k: v.to(DEV) for k, v in f.items()}, {k: v.to(DEV) for k, v in r.items()})
    runner.sync_sweep()
    torch.cuda.synchronize()
    assert len(seen) == 6 and all(seen), seen
    assert not torch.equal(eng.fp8["w8"], w8_0)


class _MxLinearFn(torch.autograd.Function):
    """forward F.linear(xq, wq, b); backward: dX = MX(dY) . wq (the fp8 dgrad), dW = dY^T xq, db = sum dY (the weight gradient keeps dY)"""

    @staticmethod
    def forward(ctx, x, xq, w, wq, b):
        ctx.save_for_backward(xq, wq)
        return F.linear(xq, wq, b)

    @staticmethod
    def backward(ctx, g):
        xq, wq = ctx.saved_tensors
        g2 = g.reshape(-1, g.shape[-1])
        _, _, gq = mx_ref(g2)
        dx = (gq @ wq).reshape(*g.shape[:-1], wq.shape[1])
        dw = g2.T @ xq.reshape(-1, xq.shape[-1])
        return dx, None, dw, None, g2.sum(0)


def _apply_mx_backward(fq):
    from oracle import fp8_ref
    for blk in fq.blocks:
        for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2):
            def fwd(x, lin=lin):
                ws = lin.w_scale_override if lin.w_scale_override is not None else fp8_ref.weight_scale(lin.weight)
                return _MxLinearFn.apply(x, fp8_ref.q_e4m3(x, lin.act_scale), lin.weight, fp8_ref.q_e4m3(lin.weight, ws), lin.bias)
            lin.forward = fwd
    return fq


def _grads(model):
    return {n: p.grad.detach().float().cpu().clone() for n, p in model.named_parameters() if p.grad is not None}


def _run_backward(model, x, t, y, drop, w):
    model.zero_grad()
    out = model(x.to(DEV), t.to(DEV), y.to(DEV), force_drop_ids=drop.to(DEV))
    (out * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return _grads(model)


def _cos(ga, gb):
    a = torch.cat([ga[n].flatten().double() for n in gb])
    b = torch.cat([gb[n].flatten().double() for n in gb])
    return (torch.dot(a, b) / (a.norm() * b.norm())).item()


@pytest.mark.parametrize("size", ["fixture", "xl2"])
def test_whole_backward_vs_mx_oracle_and_bf16_backward(size):
    from oracle import dit_ref, fp8_ref
    from sfron import dit
    if size == "fixture":
        cfg, B, S = CFG, 4, 16
    else:
        cfg, B, S = dict(input_size=32, patch_size=2, in_channels=4, hidden_size=1152, depth=28, num_heads=16, num_classes=1000), 4, 32
    ref, model = _model(cfg, B, seed=3, std=0.02)
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(B, 4, S, S, generator=gen)
    t, y, drop = torch.tensor([0, 999, 17, 500]), torch.tensor([1, 9, 4, 4]), torch.tensor([0, 1, 0, 0])
    w = torch.randn(B, 8, S, S, generator=gen) * 0.1
    model.train()
    g8 = _run_backward(model, x, t, y, drop, w)
    # (b) the same weights through the fp8 forward / bf16 backward path
    eng = model.engine
    L = _lib()
    L.check(L.lib().sfron_aux_set_fp8_dgrad(eng.aux, None, None, None), "disarm")
    gb = _run_backward(model, x, t, y, drop, w)
    cos_b = _cos(g8, gb)
    worst_b = max(_rel(g8[n], gb[n]) for n in gb if gb[n].norm() > 0)
    # (a) fake-quant oracle with the MX dgrads, scales pinned to the ones in use
    res = dict(cos_b=cos_b, worst_b=worst_b)
    # (the oracle in fp32 on the CPU at the fixture size, on the GPU at DiT-XL/2 -- TF32 off, so it stays an fp32 restatement)
    odev = "cpu" if size == "fixture" else DEV
    fq = fp8_ref.apply_fake_quant(copy.deepcopy(ref))
    sc = eng.fp8["scales"].cpu().view(-1, 4)
    for l, blk in enumerate(fq.blocks):
        for i, lin in enumerate((blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2)):
            lin.w_scale_override = float(sc[l, i])
    _apply_mx_backward(fq)
    fq.to(odev).train()
    keep = torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = torch.backends.cudnn.allow_tf32 = False
    try:
        out = fq(x.to(odev), t.to(odev), y.to(odev), force_drop_ids=drop.to(odev))
        (out * w.to(odev)).sum().backward()
    finally:
        torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = keep
    ga = {n: p.grad.detach().float().cpu().clone() for n, p in fq.named_parameters() if p.grad is not None}
    del fq, out
    res["cos_a"] = _cos(g8, ga)
    # attn.qkv.bias: its k third has a gradient of zero in exact arithmetic (adding one vector to every key shifts all logits of a query by
    # the same amount, which softmax ignores), so that third is rounding noise in both paths -- compared: the q and v thirds
    D = cfg["hidden_size"]

    def part(n, g):
        return torch.cat([g[:D], g[2 * D:]]) if n.endswith("attn.qkv.bias") else g
    res["worst_a"] = max(_rel(part(n, g8[n]), part(n, ga[n])) for n in ga if ga[n].norm() > 0)
    print(f"whole backward ({size}): {res}")
    # bounds: 2 x the measured distance (MI355X, this seed).  Fixture: cos_b 1 - 1.1e-7, worst tensor 0.042; against the MX oracle cos 1 - 4.9e-6,
    # worst tensor 0.034.  DiT-XL/2 batch 4: cos_b 1 - 4.4e-5, worst tensor 0.045; against the MX oracle cos 1 - 9.9e-5, worst tensor 0.040
    if size == "fixture":
        assert cos_b > 1 - 2.2e-7 and worst_b < 0.084, res
        assert res["cos_a"] > 1 - 1e-5 and res["worst_a"] < 0.069, res
    else:
        assert cos_b > 1 - 8.8e-5 and worst_b < 0.091, res
        assert res["cos_a"] > 1 - 2e-4 and res["worst_a"] < 0.080, res


def test_trajectory_vs_fp8_forward_only():
    """three SFR-on iterations, fp8_backward=True against fp8=True on the same seeds: per-tensor update cosine and norm ratio"""
    from sfron import data, diffusion, step
    ups = []
    for fb in (True, False):
        ref, model = _model(CFG, 4, seed=7, backward=fb)
        model.train()
        gm = torch.Generator().manual_seed(5)
        mask = {"module." + n: (torch.rand(p.shape, generator=gm) < 0.5) for n, p in ref.named_parameters() if p.requires_grad}
        mask["module.pos_embed"] = 0
        runner = step.DiTSFRon(model, diffusion.create_diffusion(""), lr=2e-4, forget_alpha=0.3, grad_clip=1.0, mask=mask, fp8=True,
                               fp8_backward=fb, forget_class=3)
        eng = model.engine
        p0 = eng.params.clone()
        kw = dict(global_batch=4, num_classes=10, forget_class=3, input_size=16)
        for it in range(3):
            f, r = data.synthetic_batch(9, it, "forget", **kw), data.synthetic_batch(9, it, "remain", **kw)
            runner.step({k: v.to(DEV) for k, v in f.items()}, {k: v.to(DEV) for k, v in r.items()})
        runner.sync_sweep()
        torch.cuda.synchronize()
        ups.append({n: (eng.view(eng.params, n) - eng.view(p0, n)).flatten().double().cpu() for n in eng.index if eng.index[n][2]})
    worst_cos, worst_ratio = 1.0, 1.0
    ga = torch.cat([ups[0][n] for n in ups[1]])
    gb = torch.cat([ups[1][n] for n in ups[1]])
    glob = (torch.dot(ga, gb) / (ga.norm() * gb.norm())).item()
    for n in ups[1]:
        a, b = ups[0][n], ups[1][n]
        if b.norm() == 0:
            continue
        c = (torch.dot(a, b) / (a.norm() * b.norm())).item()
        worst_cos = min(worst_cos, c)
        worst_ratio = max(worst_ratio, abs(a.norm().item() / b.norm().item() - 1) + 1)
    print(f"trajectory fp8_backward vs fp8 forward only: global update cosine {glob:.6f}, worst per-tensor update cosine {worst_cos:.5f}, "
          f"worst norm ratio {worst_ratio:.4f}")
    # 2 x the measured distance (MI355X): global cosine 0.99690, worst per-tensor cosine 0.829 (a small tensor whose Adam steps follow
    # near-zero gradients), norm ratio 1.027
    assert glob > 1 - 2 * 0.0031 and worst_cos > 1 - 2 * 0.172 and worst_ratio < 1 + 2 * 0.027, (glob, worst_cos, worst_ratio)


def test_xl2_batch32_iteration_reproducible():
    """DiT-XL/2, batch 32, fp8 forward + backward: two fresh runs of one SFR-on iteration agree bit for bit (parameters, w8, w8t, scales)"""
    from sfron import data, dit, diffusion, step
    res = []
    for run in range(2):
        torch.manual_seed(0)
        model = dit.DiT_models["DiT-XL/2"](input_size=32, num_classes=1000, batch_size=32)
        dit.randomize_zero_init(model, std=0.02, seed=1)
        eng = model.engine
        runner = step.DiTSFRon(model, diffusion.create_diffusion("", device=DEV), lr=1e-4, forget_alpha=1e-3, grad_clip=1.0, mask=None,
                               unlearn_loss="ga", forget_class=207, fp8=True, fp8_backward=True)
        out = runner.step(data.synthetic_batch(7, 0, "forget", 32, device=DEV), data.synthetic_batch(7, 0, "remain", 32, device=DEV))
        runner.sync_sweep()
        torch.cuda.synchronize()
        runner.guard.poll(block=True)
        assert torch.isfinite(out["forget_mse"]).all() and torch.isfinite(out["remain_mse"]).all()
        res.append((eng.params[:eng.n_trainable].clone(), eng.fp8["w8"].clone(), eng.fp8["w8t"]["t"].clone(), eng.fp8["scales"].clone()))
        del runner, model, eng
        torch.cuda.empty_cache()
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b), "two fresh runs of the same fp8-backward iteration must agree bit for bit"
    assert torch.isfinite(res[0][0]).all()


def test_refusals():
    from sfron import diffusion, dit, step
    _, model = _model(CFG, 4, seed=1, backward=False)
    diff = diffusion.create_diffusion("")
    with pytest.raises(ValueError):
        step.DiTSFRon(dit.DiT(batch_size=4, **CFG), diff, fp8=False, fp8_backward=True)
    with pytest.raises(ValueError):
        step.DiTSFRon(model, diff, fp8=True, fp8_backward=True, method="joint")
    with pytest.raises(ValueError):
        step.DiTSFRon(model, diff, fp8=True, fp8_backward=True, micro_batches=2)
    with pytest.raises(ValueError):
        step.DiTSFRon(model, diff, fp8=True, fp8_backward=True, overlap_allreduce=True)
    assert model.engine.fp8.get("w8t") is None                        # nothing was armed by a refused construction
    from sfron import _lib as L
    # an unsupported shape at enable time: batch 2 -> M = 128 token rows is not a multiple of the 256-row fp8 tile
    small = dit.DiT(batch_size=2, **CFG)
    with pytest.raises(L.SfronError):
        small.engine.enable_fp8(backward=True)
    assert small.engine.fp8 is None
    with pytest.raises(L.SfronError):
        dit.DiT(batch_size=4, **CFG).engine.enable_fp8_backward()        # needs enable_fp8 first


def test_acceptance_config2_fifty_iterations_fp8_backward_vs_fp8_forward():
    """BASELINE config 2 (DiT-B/4, batch 32: the dgrad shapes 2048 x 768 x {2304, 768, 3072} and 2048 x 3072 x 768): 50 SFR-on iterations with
    fp8_backward=True against fp8=True on the same weights, seeds and mask.  The held-out eps-MSE of the two must agree within the north
    star's 1e-4 -- the increment the fp8 backward adds to the fp8 forward."""
    from sfron import data, diffusion, dit, step
    B, res = 32, []
    for fb in (True, False):
        torch.manual_seed(0)
        model = dit.DiT_models["DiT-B/4"](input_size=32, num_classes=1000, batch_size=B)
        dit.randomize_zero_init(model, std=0.02, seed=1)
        model.train()
        eng = model.engine
        mask = (torch.rand(eng.n_trainable, generator=torch.Generator().manual_seed(5)) < 0.5).to(torch.uint8).to(DEV)
        diff = diffusion.create_diffusion("", device=DEV)
        runner = step.DiTSFRon(model, diff, lr=1e-4, forget_alpha=1e-3, grad_clip=1.0, ema_decay=0.9999, mask=None, unlearn_loss="ga",
                               forget_class=207, fp8=True, fp8_backward=fb)
        runner.mask_arena = runner.opt.mask = mask
        assert (eng.fp8.get("w8t") is not None) == fb
        losses = []
        for it in range(50):
            out = runner.step(data.synthetic_batch(9, it, "forget", B, device=DEV), data.synthetic_batch(9, it, "remain", B, device=DEV))
            losses.append((out["forget_mse"].mean(), out["remain_mse"].mean()))
        runner.sync_sweep()
        runner.guard.poll(block=True)
        model.eval()
        hb = data.synthetic_batch(10, 0, "remain", B, device=DEV)
        with torch.no_grad():
            o = model(diff.q_sample(hb["x0"], hb["t"], hb["noise"]), hb["t"], hb["y"])
            mse, _, _ = diff.loss_fwd_bwd(o.contiguous(), hb["x0"], hb["t"], hb["noise"], 1.0)
        torch.cuda.synchronize()
        res.append((mse.mean().item(), torch.tensor([[a.item(), b.item()] for a, b in losses])))
        del runner, model, eng
        torch.cuda.empty_cache()
    gap = abs(res[0][0] - res[1][0])
    step_gap = (res[0][1] - res[1][1]).abs().max().item()
    print(f"config 2, 50 iterations: held-out eps-MSE fp8 fwd+bwd {res[0][0]:.6f}, fp8 fwd {res[1][0]:.6f}, gap {gap:.2e}; "
          f"max per-step training-loss gap {step_gap:.2e}")
    assert math.isfinite(res[0][0]) and math.isfinite(res[1][0])
    assert gap < 1e-4, gap                     # the north star
    # 2 x the measured gaps (MI355X): held-out 1.0e-5, per-step training loss 1.6e-3
    assert gap < 2.1e-5 and step_gap < 3.3e-3, (gap, step_gap)


def test_runner_without_the_flag_disarms_an_armed_engine():
    """DiTSFRon(fp8=True) over an engine an earlier fp8_backward runner armed runs the bf16 dgrads: same gradients as an engine never armed"""
    from sfron import diffusion, step
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(4, 4, 16, 16, generator=gen)
    t, y, drop = torch.tensor([0, 999, 17, 500]), torch.tensor([1, 9, 4, 4]), torch.tensor([0, 1, 0, 0])
    w = torch.randn(4, 8, 16, 16, generator=gen) * 0.1
    _, plain = _model(CFG, 4, seed=3, backward=False)
    plain.train()
    want = _run_backward(plain, x, t, y, drop, w)
    _, model = _model(CFG, 4, seed=3, backward=False)
    model.train()
    diff = diffusion.create_diffusion("")
    step.DiTSFRon(model, diff, fp8=True, fp8_backward=True)
    assert model.engine.fp8.get("w8t") is not None
    armed = _run_backward(model, x, t, y, drop, w)
    step.DiTSFRon(model, diff, fp8=True)
    assert model.engine.fp8.get("w8t") is None
    got = _run_backward(model, x, t, y, drop, w)
    assert any(not torch.equal(armed[n], want[n]) for n in want)          # the armed pass did take the fp8 dgrads
    assert all(torch.equal(got[n], want[n]) for n in want)
