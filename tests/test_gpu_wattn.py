"""GPU: the fused wide-head self-attention of csrc/wattn.hip (head widths 160 and 256) through the C ABI against float64 torch on the CPU
from the same bf16 inputs, and the opt-in switches through Conditional_Model / DDPMSFRon and UNetModel.

Bounds (none is tuned to what the kernels give):
  O, dQ, dK, dV  relative 2-norm 2e-2 per (sample, head), over all columns of the head and over its last eight alone; O also per element
                 (rtol 2e-2 / atol 2e-2): the bounds of tests/test_gpu_attention_grid.py.  The bf16 restatement of tests/test_wattn_cpu.py
                 sits under half of 2e-2 on these inputs.
  lse            per row within 4 hd 2^-24 scale max_j sum_i |q_i k_ji| + 1e-5 of float64: four times the worst-case fp32 accumulation
                 error of the row's dot products plus the exp / log rounding, computed from the inputs (tests/test_wattn_cpu.reference)
  DDPM model     out rel-L2 1.5e-2, worst gradient rel-L2 5e-2, cosine 0.9995: tests/test_gpu_unet.test_unet_forward_backward_vs_oracle
  SD model       tests/test_gpu_sd._compare_unet's defaults (1.5e-2 / 6e-2 / 0.9995), what test_sd_unet_forward_backward_vs_oracle holds
                 the flag-off HD160 model to
Every tensor handed to the library sits between guard elements (tests/test_gpu_attention_grid._Buf): outputs are pre-filled with a bit
pattern that must survive outside the body (guard columns behind the heads included), inputs carry NaN guards."""
import math

import pytest
import torch

import test_wattn_cpu as W
from test_gpu_attention_grid import LEAD, _Buf, _close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1001, 1002
# (B, H, T, hd, separate): the grid of the issue as column slices of one qkv matrix; separate tensors with ld > H hd; one workgroup;
# the longest accepted T
GRID = [(2, 3, T, hd, False) for hd in (160, 256) for T in (64, 128, 192, 256)]
CASES = GRID + [(2, 3, 128, 160, True), (1, 1, 64, 256, False), (1, 1, 1024, 160, False)]
PAD = 24                                              # guard columns of the separate-tensor case


def _L():
    from sfron import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Run:
    """One case on the device: inputs between NaN guards, forward (with and without lse) and backward into patterned outputs"""

    def __init__(self, B, H, T, hd, separate):
        self.B, self.H, self.T, self.hd, self.sep = B, H, T, hd, separate
        self.D = D = H * hd
        qkv, d_o = W.inputs(B, H, T, hd)
        rows = B * T
        if separate:                                   # q, k, v, d_o of their own, rows PAD elements longer than the heads (NaN there)
            self.ld = self.ldo = D + PAD
            def wide(x):
                t = torch.full((rows, D + PAD), float("nan"), dtype=torch.bfloat16)
                t[:, :D] = x
                return _Buf(t.numel(), torch.bfloat16, t)
            self.q, self.k, self.v = (wide(qkv[:, i * D:(i + 1) * D]) for i in range(3))
            self.g = wide(d_o)
            self.in_ptrs = [self.q.t.data_ptr(), self.k.t.data_ptr(), self.v.t.data_ptr()]
        else:
            self.ld, self.ldo = 3 * D, D
            self.qkv = _Buf(qkv.numel(), torch.bfloat16, qkv)
            self.g = _Buf(d_o.numel(), torch.bfloat16, d_o)
            self.in_ptrs = [self.qkv.t.data_ptr() + 2 * D * i for i in range(3)]
        self.scale = float(hd ** -0.5)

    def fwd(self, with_lse=True):
        B, H, T, hd = self.B, self.H, self.T, self.hd
        o = _Buf(B * T * self.ldo, torch.bfloat16)
        lse = _Buf(B * H * T, torch.float32)
        q, k, v = self.in_ptrs
        rc = _L().sfron_wattn_fwd(q, self.ld, k, self.ld, v, self.ld, o.t.data_ptr(), self.ldo, lse.t.data_ptr() if with_lse else None,
                                  B, T, H, hd, self.scale, _stream())
        torch.cuda.synchronize()
        return rc, o, lse

    def bwd(self, o, lse, short=0):
        B, H, T, hd, D = self.B, self.H, self.T, self.hd, self.D
        q, k, v = self.in_ptrs
        o_in = _Buf(o.n, torch.bfloat16, o.t) if not self.sep else o          # (separate: o's guard columns hold the pattern, finite)
        lse_in = _Buf(lse.n, torch.float32, lse.t)
        nb = _L().sfron_wattn_bwd_ws_bytes(B, T, H, hd)
        ws = torch.empty(nb + 16, dtype=torch.uint8, device=DEV)
        if self.sep:
            outs = [_Buf(B * T * self.ld, torch.bfloat16) for _ in range(3)]
            ptrs, ldd = [x.t.data_ptr() for x in outs], self.ld
        else:
            outs = [_Buf(B * T * 3 * D, torch.bfloat16)]
            ptrs, ldd = [outs[0].t.data_ptr() + 2 * D * i for i in range(3)], 3 * D
        rc = _L().sfron_wattn_bwd(q, self.ld, k, self.ld, v, self.ld, o_in.t.data_ptr(), self.ldo, self.g.t.data_ptr(), self.ldo if self.sep else D,
                                  lse_in.t.data_ptr(), ptrs[0], ldd, ptrs[1], ldd, ptrs[2], ldd, B, T, H, hd, self.scale, ws.data_ptr(),
                                  nb - short, _stream())
        torch.cuda.synchronize()
        return rc, outs

    def body(self, buf, ld):
        """[B*T][D] of a [B*T][ld] output on the CPU, and whether its guard columns still hold the pattern"""
        t = buf.t.view(self.B * self.T, ld)
        bits = buf.bits[LEAD:LEAD + buf.n].view(self.B * self.T, ld)
        return t[:, :self.D].cpu(), bool((bits[:, self.D:] == buf.pat).all())

    def grads(self, outs):
        """d qkv [B*T][3 D] on the CPU"""
        if not self.sep:
            return outs[0].t.view(self.B * self.T, 3 * self.D).cpu()
        parts = []
        for x in outs:
            t, ok = self.body(x, self.ld)
            assert ok, "sfron_wattn_bwd stored into the guard columns"
            parts.append(t)
        return torch.cat(parts, 1)


def _assert_heads(got, ref, B, H, T, hd, parts, what):
    names = ("dQ", "dK", "dV") if parts == 3 else ("O",)
    for err, cols in zip(W.head_errors(got, ref, B, H, T, hd, parts), ("all columns", "last 8 columns")):
        b, p, h = (int(i) for i in torch.unravel_index(err.argmax(), err.shape))
        print(f"[wattn] {what} B {B} H {H} T {T} hd {hd} {cols}: worst relative error {float(err.max()):.3e} at {names[p]} sample {b} head {h}")
        assert float(err.max()) < W.BOUND, (what, cols, names[p], f"sample {b} head {h}", float(err.max()))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d-H%d-T%d-hd%d-%s" % (c[:4] + ("separate" if c[4] else "qkv",)))
def test_forward_and_backward_vs_fp64(case):
    B, H, T, hd, sep = case
    o_ref, lse_ref, g_ref, lse_tol = W.reference(B, H, T, hd)
    r = _Run(*case)
    # ---- forward
    rc, o, lse = r.fwd()
    assert rc == OK, rc
    assert o.guards_intact() and lse.guards_intact(), "sfron_wattn_fwd stored outside o / lse"
    o_body, cols_ok = r.body(o, r.ldo)
    assert cols_ok, "sfron_wattn_fwd stored into the guard columns of o"
    _close(o_body, o_ref, 2e-2, 2e-2, f"O B {B} H {H} T {T} hd {hd}")
    _assert_heads(o_body, o_ref, B, H, T, hd, 1, "forward")
    lse_e = (lse.t.double().cpu().view(B, H, T) - lse_ref).abs()
    assert bool(torch.isfinite(lse.t).all())
    print(f"[wattn] lse B {B} H {H} T {T} hd {hd}: worst err / allowance {float((lse_e / lse_tol).max()):.3f}, max |err| {float(lse_e.max()):.2e}")
    assert bool((lse_e <= lse_tol).all()), float((lse_e / lse_tol).max())
    # the all-zero query row: uniform P, lse = log T (its allowance is the 1e-5 alone), O = the mean of V to bf16
    zr = W.stress_rows(T)[3]
    assert float((lse.t.double().cpu().view(B, H, T)[:, :, zr] - math.log(T)).abs().max()) <= 1e-5
    v = W.split(W.inputs(B, H, T, hd)[0].double(), B, H, T, hd)[2]
    mean_v = v.mean(2).reshape(B, H * hd)                                          # [B][D]
    got = o_body.double().view(B, T, H * hd)[:, zr]
    # one bf16 rounding (2^-9 relative) of a fp32 sum of T bf16 values (T 2^-24 of sum |v| / T ~ 1): 2^-8 |x| + 1e-5 covers both
    assert bool(((got - mean_v).abs() <= 2.0 ** -8 * mean_v.abs() + 1e-5).all()), float((got - mean_v).abs().max())
    # without lse: the same O, bit for bit; twice: the same bits
    rc2, o2, lse2 = r.fwd(with_lse=False)
    assert rc2 == OK and torch.equal(o.bits, o2.bits) and lse2.untouched()
    rc3, o3, lse3 = r.fwd()
    assert rc3 == OK and torch.equal(o.bits, o3.bits) and torch.equal(lse.bits, lse3.bits), "two forward calls differ"
    # ---- backward
    rc, outs = r.bwd(o, lse)
    assert rc == OK, rc
    assert all(x.guards_intact() for x in outs), "sfron_wattn_bwd stored outside its outputs"
    g = r.grads(outs)
    assert bool(torch.isfinite(g.float()).all()), "non-finite gradient"
    _assert_heads(g, g_ref, B, H, T, hd, 3, "backward")
    rc2, outs2 = r.bwd(o, lse)
    assert rc2 == OK and all(torch.equal(a.bits, b.bits) for a, b in zip(outs, outs2)), "two backward calls differ"


@pytest.mark.parametrize("hd", [160, 256])
def test_one_key_dominating_a_row(hd):
    """Query 5 scores key 77 (of the second 64-key chunk, so the running maximum moves) at least 30 above every other key: the row is finite,
    P is one-hot to rounding -- O[5] = V[77] exactly, every other weight being below exp(-30) -- and lse = that score."""
    B, H, T = 1, 1, 128
    gen = torch.Generator().manual_seed(hd)
    qkv = torch.randn(T, 3 * hd, generator=gen)
    u = qkv[5, :hd] * (hd ** 0.5 / qkv[5, :hd].norm())               # |u|^2 = hd
    qkv[5, :hd] = u
    qkv[77, hd:2 * hd] = 3.0 * u                                     # score = scale * 3 hd = 3 sqrt(hd) >= 37.9
    qkv = qkv.to(torch.bfloat16)
    s = (qkv[5, :hd].double() @ qkv[:, hd:2 * hd].double().T) * hd ** -0.5
    gap = float(s[77] - torch.cat([s[:77], s[78:]]).max())
    assert gap >= 30.0, gap
    buf = _Buf(qkv.numel(), torch.bfloat16, qkv)
    o, lse = _Buf(T * hd, torch.bfloat16), _Buf(T, torch.float32)
    p = buf.t.data_ptr()
    rc = _L().sfron_wattn_fwd(p, 3 * hd, p + 2 * hd, 3 * hd, p + 4 * hd, 3 * hd, o.t.data_ptr(), hd, lse.t.data_ptr(), B, T, H, hd,
                              float(hd ** -0.5), _stream())
    torch.cuda.synchronize()
    assert rc == OK and o.guards_intact() and lse.guards_intact()
    assert bool(torch.isfinite(o.t.float()).all()) and bool(torch.isfinite(lse.t).all())
    row = o.t.view(T, hd)[5].cpu()
    want = qkv[77, 2 * hd:]
    # the other 127 weights sum to less than 127 exp(-30) = 1.2e-11: invisible in bf16
    assert torch.equal(row, want), float((row.float() - want.float()).abs().max())
    assert abs(float(lse.t[5]) - float(s[77])) <= 4 * hd * 2.0 ** -24 * float(s[77].abs()) + 1e-5
    print(f"[wattn] dominant key hd {hd}: gap {gap:.1f}, O row equals V[77] bit for bit, lse {float(lse.t[5]):.4f} vs {float(s[77]):.4f}")


def test_refusals_leave_outputs_untouched():
    B, H = 1, 1
    n = 1088 * 3 * 256                                    # big enough for every shape tried below
    src = _Buf(n, torch.bfloat16, torch.zeros(n))
    o, dqkv = _Buf(n, torch.bfloat16), _Buf(n, torch.bfloat16)
    lse = _Buf(4096, torch.float32)
    ws = torch.full((1 << 16,), 7, dtype=torch.uint8, device=DEV)

    def fwd(T, hd, off=0):
        p = src.t.data_ptr()
        return _L().sfron_wattn_fwd(p + off, 3 * hd, p + 2 * hd, 3 * hd, p + 4 * hd, 3 * hd, o.t.data_ptr(), hd, lse.t.data_ptr(), B, T, H, hd,
                                    float(hd ** -0.5), _stream())

    def bwd(T, hd, off=0, short=0):
        p, d = src.t.data_ptr(), dqkv.t.data_ptr()
        nb = _L().sfron_wattn_bwd_ws_bytes(B, T, H, hd) - short
        return _L().sfron_wattn_bwd(p + off, 3 * hd, p + 2 * hd, 3 * hd, p + 4 * hd, 3 * hd, o.t.data_ptr(), hd, p, hd, lse.t.data_ptr(),
                                    d, 3 * hd, d + 2 * hd, 3 * hd, d + 4 * hd, 3 * hd, B, T, H, hd, float(hd ** -0.5), ws.data_ptr(), nb, _stream())
    for T, hd in W.REFUSED:
        assert fwd(T, hd) == ERR_UNSUPPORTED and bwd(T, hd) == ERR_UNSUPPORTED, (T, hd)
    for f in (fwd, bwd):
        assert f(64, 160, off=8) == ERR_ARG                # q on 8 bytes only
    assert bwd(64, 160, short=1) == ERR_ARG and bwd(256, 256, short=1) == ERR_ARG       # a workspace one byte short
    # the old entry points keep refusing the wide heads
    assert _L().sfron_attn_fwd(src.t.data_ptr(), o.t.data_ptr(), lse.t.data_ptr(), B, 64, H, 160, _stream()) != OK
    torch.cuda.synchronize()
    assert o.untouched() and dqkv.untouched() and lse.untouched() and bool((ws == 7).all())


# ------------------------------------------------------------------------------------------------ DDPM model level
# tests/test_gpu_unet.test_unet_forward_backward_vs_oracle: the bounds it holds the flag-off model to
UNET_OUT_TOL, UNET_GRAD_TOL, UNET_COS_MIN = 1.5e-2, 5e-2, 0.9995


class _Counting:
    """_lib.lib() with the calls of the named entry points counted"""

    def __init__(self, real, names):
        self._real, self.calls = real, {n: 0 for n in names}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name in self.calls:
            def counted(*a, _fn=fn, _n=name):
                self.calls[_n] += 1
                return _fn(*a)
            return counted
        return fn


NAMES = ("sfron_wattn_fwd", "sfron_wattn_bwd", "sfron_softmax_fwd", "sfron_softmax_bwd")


def test_ddpm_model_fused_attention_vs_oracle(monkeypatch):
    """A Conditional_Model whose attention levels have C = 256 and T = 64 (16 px input, ch 128, mult (1, 2), attention at 8), batch 2:
    output and every parameter gradient with fused_attention = True against the CPU oracle."""
    import test_gpu_unet as U
    from sfron import _lib, unet
    ref, model = U._pair(U.SMALL, seed=2)
    model.dropout_p = 0.0
    assert model.fused_attention is False
    model.fused_attention = True
    c = _Counting(_lib.lib(), NAMES)
    monkeypatch.setattr(unet, "_L", lambda: c)
    out, out_ref = U._fwd_bwd_both(ref, model, U.SMALL, 2, seed=11, p_drop=0.0)
    assert c.calls["sfron_wattn_fwd"] >= 2 and c.calls["sfron_wattn_bwd"] == c.calls["sfron_wattn_fwd"]      # down.1.attn.0, mid.attn_1, up.1.attn.*
    assert c.calls["sfron_softmax_fwd"] == 0 and c.calls["sfron_softmax_bwd"] == 0
    e_out = U._rel(out, out_ref)
    worst, wname, dots, na, nb = 0.0, "", 0.0, 0.0, 0.0
    gmax = max(q.grad.norm().item() for q in ref.parameters())
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        ga, gb = p.grad.detach().cpu().flatten(), q.grad.flatten()
        assert torch.isfinite(ga).all(), n
        if n.endswith(".k.bias"):                     # d k.bias = 0 exactly: rounding noise on both sides (test_gpu_unet)
            assert ga.norm().item() < 1e-3 * gmax and gb.norm().item() < 1e-3 * gmax, n
            continue
        e = ((ga - gb).norm() / (gb.norm() + 1e-30)).item()
        if e > worst:
            worst, wname = e, n
        dots += torch.dot(ga.double(), gb.double()).item(); na += ga.double().pow(2).sum().item(); nb += gb.double().pow(2).sum().item()
    cos = dots / math.sqrt(na * nb)
    print(f"[wattn] DDPM U-Net fused attention B=2: out rel-L2 {e_out:.3e}, worst grad rel-L2 {worst:.3e} ({wname}), cosine {cos:.6f}")
    assert e_out < UNET_OUT_TOL and worst < UNET_GRAD_TOL and cos > UNET_COS_MIN, (e_out, wname, worst, cos)


def test_ddpm_step_under_stage_graphs_with_the_flag_on():
    import test_gpu_unet as U
    from sfron import ddpm
    cfg = dict(U.SMALL, dropout=0.0)
    B, n_it = 2, 4                                       # eager warm-up, capture, then two replays per stage
    g = torch.Generator().manual_seed(41)
    _, model = U._pair(cfg, seed=40)
    run = ddpm.DDPMSFRon(model, lr=1e-4, forget_alpha=10.0, grad_clip=1.0, ema_rate=1e-4, unlearn_loss="adaga", n_iters=n_it, use_graphs=True,
                         fused_attn=True)
    assert model.fused_attention is True
    for it in range(n_it):
        pair = []
        for stream in ("forget", "remain"):
            b = U._synthetic(it, stream, B, g)
            b["x0"], b["e"] = b["x0"][:, :, :16, :16].contiguous(), b["e"][:, :, :16, :16].contiguous()
            b["keep_mask"] = (torch.rand(B, generator=g) >= 0.1).to(torch.uint8)
            pair.append({k: v.to(DEV) for k, v in b.items()})
        out = run.step(it, *pair)
        assert torch.isfinite(out["forget_loss"]).item() and torch.isfinite(out["remain_loss"]).item()
    torch.cuda.synchronize()
    assert run._graphs["forget"].graph is not None and run._graphs["remain"].graph is not None
    assert torch.isfinite(run.flat.p).all().item()


# ------------------------------------------------------------------------------------------------ SD model level
def _sd_batch(cfg, B=2, S=8, Lc=77):
    g = torch.Generator().manual_seed(9)
    return (torch.randn(B, 4, S, S, generator=g), torch.randint(0, 1000, (B,), generator=g), torch.randn(B, Lc, cfg["context_dim"], generator=g),
            torch.randn(B, 4, S, S, generator=g) * 0.1)


def test_sd_model_fused_wide_self_attention_vs_oracle(monkeypatch):
    """A UNetModel with one level of head width 160 (320 channels, 2 heads) at 8 x 8 latents: grad mode against the oracle at
    _compare_unet's bounds; under no_grad the forward without lse against the oracle's output at the same output bound."""
    import test_gpu_sd as S
    from sfron import _lib, sd_unet
    ref, model = S._pair(S.HD160, seed=2)
    ref.train(); model.train()
    assert model.fused_wide_self_attention is False
    model.fused_wide_self_attention = True
    c = _Counting(_lib.lib(), NAMES)
    monkeypatch.setattr(sd_unet, "_L", lambda: c)
    x, t, ctx, w = _sd_batch(S.HD160)
    S._compare_unet(ref, model, x, t, ctx, w, "[wattn] SD UNet HD160 B=2 8x8 ctx 77, fused wide self-attention")
    nblk = len(model.st_blocks)
    assert c.calls["sfron_wattn_fwd"] == nblk and c.calls["sfron_wattn_bwd"] == nblk
    with torch.no_grad():
        want = ref(x, timesteps=t, context=ctx)
        got = model(x.to(DEV), timesteps=t.to(DEV), context=ctx.to(DEV))
    assert c.calls["sfron_wattn_fwd"] == 2 * nblk and c.calls["sfron_wattn_bwd"] == nblk
    e = S._rel(got, want)
    print(f"[wattn] SD UNet HD160 no_grad, fused wide self-attention: out rel-L2 {e:.3e}")
    assert e < 1.5e-2, e                                  # _compare_unet's out_tol


def test_sd_flags_off_forward_is_bit_identical_to_a_model_without_the_attribute():
    import test_gpu_sd as S
    _, model = S._pair(S.HD160, seed=2)
    model.train()
    x, t, ctx, _ = (v.to(DEV) for v in _sd_batch(S.HD160))
    with torch.no_grad():
        a = model(x, timesteps=t, context=ctx).clone()
    _, bare = S._pair(S.HD160, seed=2)
    bare.train()
    del bare.fused_wide_self_attention                    # a model that never had the attribute (an instance from before the switch)
    assert not hasattr(bare, "fused_wide_self_attention")
    with torch.no_grad():
        b = bare(x, timesteps=t, context=ctx).clone()
    assert model.fused_wide_self_attention is False and model.fused_cross_attention_train is False
    assert torch.equal(a, b)
