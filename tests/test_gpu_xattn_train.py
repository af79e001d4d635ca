"""GPU: the differentiable fused cross-attention -- sfron_xattn_fwd_lse / sfron_xattn_bwd against float64 torch on the CPU from the same
bf16 inputs, and the opt-in switch through UNetModel (fused_cross_attention_train), the autograd surface and SDSFRon(fused_xattn=True).

Bounds (none is tuned to what the kernels give):
  O        torch.equal to sfron_xattn_fwd's
  lse      1e-3 + 2^-16 max_j |s_ij| of the float64 log-sum-exp: the project's softmax row-sum allowance (an absolute error in the logarithm)
           plus fp32 roundings of the scaled scores
  dQ/dK/dV relative 2-norm 2e-2 per (sample, head), the bound tests/test_gpu_attention_grid.py holds the self-attention backward to; the
           bf16 restatement of tests/test_xattn_train_cpu.py sits under half of it on these inputs.  One key: dQ = dK = 0, dV = sum_n dO.
  model    the bounds tests/test_gpu_sd.py applies to the flag-off path (its _compare_unet defaults and SD_ORACLE_UPDATE_* constants).
The Fisher-mask comparison of the issue is left out: no existing test gives the share by which two flag-off runs at different batch
orderings differ, which is the yardstick it asks for."""
import math

import pytest
import torch

import test_xattn_train_cpu as X
from test_gpu_ddim import INFER
from test_gpu_sd import SD_ORACLE_UPDATE_COS_MIN, SD_ORACLE_UPDATE_NORM_TOL, SMALL, _compare_unet, _pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG, ERR_UNSUPPORTED = 1001, 1002
FILL = 77.0
_REF = {}


def _L():
    from sfron import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ref(case):
    """inputs and the float64 reference of a case, computed once and shared"""
    if case not in _REF:
        B, H, N, hd, Lv, Lk = case
        q, kv, d_o = X.inputs(B, H, N, hd, Lv, Lk, seed=N + hd + Lv)
        _REF[case] = (q, kv, d_o, X.reference(q, kv, d_o, B, H, N, hd, Lv, Lk))
    return _REF[case]


def _run_case(case, pad=8, tail=5):
    """forward with lse + backward on the device; outputs have `pad` guard columns and dq `tail` guard rows, all pre-filled with FILL"""
    B, H, N, hd, Lv, Lk = case
    C = H * hd
    q, kv, d_o, _ = _ref(case)
    qd, kvd, gd = q.to(DEV), kv.to(DEV), d_o.to(DEV)
    s = float(hd ** -0.5)
    o0 = torch.full((B * N, C), FILL, dtype=torch.bfloat16, device=DEV)
    o = torch.full((B * N, C), FILL, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B * H * N,), FILL, dtype=torch.float32, device=DEV)
    k_, v_ = kvd.data_ptr(), kvd.data_ptr() + 2 * C
    assert _L().sfron_xattn_fwd(qd.data_ptr(), C, k_, 2 * C, v_, 2 * C, o0.data_ptr(), C, B, N, Lk, Lv, H, hd, s, _stream()) == 0
    assert _L().sfron_xattn_fwd_lse(qd.data_ptr(), C, k_, 2 * C, v_, 2 * C, o.data_ptr(), C, B, N, Lk, Lv, H, hd, s, lse.data_ptr(), _stream()) == 0
    nb = _L().sfron_xattn_bwd_ws_bytes(B, N, Lk, H, hd)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    dq = torch.full((B * N + tail, C + pad), FILL, dtype=torch.bfloat16, device=DEV)
    dkv = torch.full((B * Lk, 2 * (C + pad)), FILL, dtype=torch.bfloat16, device=DEV)      # dk = columns 0 .. C-1, dv = C+pad .. 2C+pad-1
    st = _L().sfron_xattn_bwd(qd.data_ptr(), C, k_, 2 * C, v_, 2 * C, o.data_ptr(), C, gd.data_ptr(), C, lse.data_ptr(), dq.data_ptr(), C + pad,
                              dkv.data_ptr(), 2 * (C + pad), dkv.data_ptr() + 2 * (C + pad), 2 * (C + pad), B, N, Lk, Lv, H, hd, s,
                              ws.data_ptr(), nb, _stream())
    assert st == 0, st
    torch.cuda.synchronize()
    return o0.cpu(), o.cpu(), lse.cpu(), dq.cpu(), dkv.cpu()


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: "B%d-H%d-N%d-hd%d-Lv%d-Lk%d" % c)
def test_xattn_fwd_lse_and_bwd_vs_fp64(case):
    B, H, N, hd, Lv, Lk = case
    C, pad, tail = H * hd, 8, 5
    q, kv, d_o, ref = _ref(case)
    o0, o, lse, dq, dkv = _run_case(case, pad, tail)
    tag = "xattn train B%d H%d N%d hd%d Lv%d/%d" % case
    # ---- forward: O bit-identical, lse within the softmax allowance
    assert torch.equal(o, o0)
    lse_b = 1e-3 + 2.0 ** -16 * ref["s"].abs().amax(-1)
    lse_e = (lse.double().view(B, H, N) - ref["lse"]).abs()
    print(f"{tag}: lse worst err / bound {float((lse_e / lse_b).max()):.3f}")
    assert bool((lse_e <= lse_b).all())
    # ---- guards and padding
    assert bool(torch.isfinite(dq.float()).all()) and bool(torch.isfinite(dkv.float()).all())
    assert bool((dq[B * N:] == FILL).all()) and bool((dq[:, C:] == FILL).all())
    dk_full, dv_full = dkv[:, :C].view(B, Lk, C), dkv[:, C + pad:2 * C + pad].view(B, Lk, C)
    assert bool((dkv[:, C:C + pad] == FILL).all()) and bool((dkv[:, 2 * C + pad:] == FILL).all())
    assert not dk_full[:, Lv:].any() and not dv_full[:, Lv:].any()               # exact zeros behind the real keys
    # ---- gradients per (sample, head)
    got = dict(dq=dq[:B * N, :C].double().view(B, N, H, hd).permute(0, 2, 1, 3),
               dk=dk_full[:, :Lv].double().view(B, Lv, H, hd).permute(0, 2, 1, 3),
               dv=dv_full[:, :Lv].double().view(B, Lv, H, hd).permute(0, 2, 1, 3))
    if Lv == 1:                                       # one key: exact
        assert not got["dq"].any() and not got["dk"].any()
        assert torch.equal(got["dv"], ref["dv"].to(torch.bfloat16).double())
        print(f"{tag}: dQ = dK = 0 and dV = bf16(sum dO) exactly")
        return
    for name in ("dq", "dk", "dv"):
        worst = float(X.head_rel(got[name], ref[name]).max())
        print(f"{tag}: {name} worst rel err / bound {worst / X.GRAD_TOL:.3f}")
        assert worst <= X.GRAD_TOL, (name, worst)


def test_xattn_bwd_is_deterministic():
    case = (1, 2, 1100, 40, 77, 80)
    a, b = _run_case(case), _run_case(case)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_xattn_train_refusals_leave_outputs_untouched():
    B, H, N, hd, Lv, Lk = 1, 2, 16, 40, 5, 8
    q, kv, d_o = (t.to(DEV) for t in X.inputs(B, H, N, 64, Lv, 136, seed=3))      # big enough for every shape tried below
    o = torch.full((B * N, 2 * 64), FILL, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B * H * N,), FILL, dtype=torch.float32, device=DEV)
    dq, dkv = torch.full_like(o, FILL), torch.full((B * 136, 4 * 64), FILL, dtype=torch.bfloat16, device=DEV)
    ws = torch.full((1 << 20,), 7, dtype=torch.uint8, device=DEV)

    def fwd(hd=hd, Lk=Lk, Lv=Lv, off=0):
        C = H * hd
        return _L().sfron_xattn_fwd_lse(q.data_ptr() + off, C, kv.data_ptr(), 2 * C, kv.data_ptr() + 2 * C, 2 * C, o.data_ptr(), C, B, N, Lk, Lv, H, hd,
                                        float(hd ** -0.5), lse.data_ptr(), _stream())

    def bwd(hd=hd, Lk=Lk, Lv=Lv, off=0, short=0):
        C = H * hd
        nb = _L().sfron_xattn_bwd_ws_bytes(B, N, Lk, H, hd) - short
        return _L().sfron_xattn_bwd(q.data_ptr() + off, C, kv.data_ptr(), 2 * C, kv.data_ptr() + 2 * C, 2 * C, o.data_ptr(), C, d_o.data_ptr(), C,
                                    lse.data_ptr(), dq.data_ptr(), C, dkv.data_ptr(), 2 * C, dkv.data_ptr() + 2 * C, 2 * C, B, N, Lk, Lv, H, hd,
                                    float(hd ** -0.5), ws.data_ptr(), nb, _stream())
    for f in (fwd, bwd):
        assert f(hd=64) == ERR_UNSUPPORTED and f(Lk=136, Lv=100) == ERR_UNSUPPORTED and f(Lk=77, Lv=70) == ERR_UNSUPPORTED
        assert f(Lv=0) == ERR_ARG and f(Lv=Lk + 1) == ERR_ARG and f(off=8) == ERR_ARG
    assert bwd(short=1) == ERR_ARG
    torch.cuda.synchronize()
    for t in (o, dq, dkv):
        assert bool((t == FILL).all())
    assert bool((lse == FILL).all()) and bool((ws == 7).all())


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


NAMES = ("sfron_xattn_fwd", "sfron_xattn_fwd_lse", "sfron_xattn_bwd", "sfron_softmax_fwd", "sfron_softmax_bwd")


def _counted(monkeypatch):
    from sfron import _lib, sd_unet
    c = _Counting(_lib.lib(), NAMES)
    monkeypatch.setattr(sd_unet, "_L", lambda: c)
    return c


def _infer_batch():
    g = torch.Generator().manual_seed(78)
    return (torch.randn(2, 4, 8, 8, generator=g), torch.tensor([37, 801]), torch.randn(2, 77, 64, generator=g),
            torch.randn(2, 4, 8, 8, generator=g) * 0.1)


def test_default_launches_are_unchanged(monkeypatch):
    _, model = _pair(INFER, seed=77)
    model.train()
    assert model.fused_cross_attention_train is False and model.fused_cross_attention is False
    x, t, ctx, w = (v.to(DEV) for v in _infer_batch())
    c = _counted(monkeypatch)
    out, bwd = model._run(x, t, ctx, need_grad=True)
    bwd(w)
    model._run(x, t, ctx, need_grad=False)
    torch.cuda.synchronize()
    nblk = len(model.st_blocks)
    assert c.calls["sfron_xattn_fwd"] == c.calls["sfron_xattn_fwd_lse"] == c.calls["sfron_xattn_bwd"] == 0
    assert c.calls["sfron_softmax_bwd"] >= nblk and c.calls["sfron_softmax_fwd"] >= 2 * nblk      # attn2 of every block through _mha
    # flag on: tape passes take the lse forward and the fused backward, passes without a tape the plain forward, grad mode on or off
    model.fused_cross_attention_train = True
    base = dict(c.calls)
    out, bwd = model._run(x, t, ctx, need_grad=True)
    bwd(w)
    model._run(x, t, ctx, need_grad=False)
    torch.cuda.synchronize()
    assert c.calls["sfron_xattn_fwd_lse"] == nblk and c.calls["sfron_xattn_bwd"] == nblk and c.calls["sfron_xattn_fwd"] == nblk
    # what is left on the softmax kernels is the 16-token self-attention level, which takes _mha: the flag-off count minus attn2's
    assert c.calls["sfron_softmax_bwd"] - base["sfron_softmax_bwd"] == base["sfron_softmax_bwd"] - nblk


def test_model_gradients_fused_vs_oracle_and_flag_off():
    x, t, ctx, w = _infer_batch()
    ref, model = _pair(INFER, seed=77)
    ref.train(); model.train()
    model.fused_cross_attention_train = True
    # the autograd surface (_SDFn -> _run(need_grad=True)) against the CPU oracle, at the flag-off path's bounds (_compare_unet's defaults)
    _compare_unet(ref, model, x, t, ctx, w, "SD UNet INFER B=2 8x8 ctx 77, fused cross-attention")
    # (the tape forms no gradient with respect to the latent -- conv_in's backward is asked for none -- so there is no input gradient to compare)
    fused = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    for flag in (True, False):
        model.fused_cross_attention_train = flag
        for p in model.parameters():
            p.grad = None
        (model(x.to(DEV), timesteps=t.to(DEV), context=ctx.to(DEV)) * w.to(DEV)).sum().backward()
        if flag:
            for n, p in model.named_parameters():
                assert torch.equal(p.grad, fused[n]), n                       # the fused path is reproducible
    gmed = float(torch.tensor([q.grad.norm().item() for q in ref.parameters()]).median())
    worst, wname, dots, na, nb = 0.0, "", 0.0, 0.0, 0.0
    for n, p in model.named_parameters():
        a, b = fused[n].double().flatten().cpu(), p.grad.double().flatten().cpu()
        dots += float(a @ b); na += float(a @ a); nb += float(b @ b)
        if b.norm().item() < 2e-3 * gmed:
            continue                                                          # cancellation noise on both sides (see _compare_unet)
        e = float((a - b).norm() / (b.norm() + 1e-30))
        if e > worst:
            worst, wname = e, n
    cos = dots / math.sqrt(na * nb)
    print(f"fused vs flag-off: worst grad rel-L2 {worst:.3e} ({wname}), cosine {cos:.6f}")
    assert worst < 6e-2 and cos > 0.9995                                      # _compare_unet's grad_tol / cos_min


def _sd_batches(B, S, Lc, n, seed):
    g = torch.Generator().manual_seed(seed)
    c_f = torch.randn(1, Lc, 64, generator=g).expand(B, -1, -1).contiguous()
    c_p = torch.randn(1, Lc, 64, generator=g).expand(B, -1, -1).contiguous()
    out = []
    for _ in range(n):
        xf = torch.randn(B, 4, S, S, generator=g)
        out.append((dict(x_f=xf, x_p=xf, c_f=c_f, c_p=c_p, t=torch.randint(0, 1000, (B,), generator=g), noise=torch.randn(B, 4, S, S, generator=g)),
                    dict(x=torch.randn(B, 4, S, S, generator=g), c=c_p, t=torch.randint(0, 1000, (B,), generator=g),
                         noise=torch.randn(B, 4, S, S, generator=g))))
    return out


def test_sd_sfron_xattn_iterations_fused_vs_oracle_and_graphs():
    from oracle import sd_ref
    from sfron import sd
    hp = dict(lr=1e-4, forget_alpha=1.0, remain_alpha=1.0, train_method="xattn")
    batches = _sd_batches(2, 8, 77, 2, seed=16)
    ref, _ = _pair(INFER, seed=14)
    p0 = {n: p.detach().clone() for n, p in ref.named_parameters()}
    orc = sd_ref.SDSfronOracle(ref, sd_ref.LDMSchedule(), **hp)
    want = [orc.step(f, r) for f, r in batches]
    res = []
    for use in (False, True):
        _, model = _pair(INFER, seed=14)
        run = sd.SDSFRon(model, use_graphs=use, fused_xattn=True, **hp)
        assert model.fused_cross_attention_train is True
        losses = [run.step({k: v.to(DEV) for k, v in f.items()}, {k: v.to(DEV) for k, v in r.items()}) for f, r in batches]
        res.append((model.params.clone(), [(l["forget_loss"].item(), l["remain_loss"].item()) for l in losses], model))
    assert res[0][1] == res[1][1] and torch.equal(res[0][0], res[1][0])       # graph replay: bit-equal losses and parameters
    model = res[0][2]
    for (fl, rl), w in zip(res[0][1], want):
        assert fl == pytest.approx(w["forget_loss"], rel=4e-2, abs=1e-5) and rl == pytest.approx(w["remain_loss"], rel=3e-2)
    worst_cos, worst_ratio = 2.0, 1.0
    for n, q in ref.named_parameters():
        mine = model.view(model.params, n).cpu()
        if "attn2" not in n:
            assert torch.equal(mine, p0[n]), n
            continue
        du_ref, du = (q.detach() - p0[n]).flatten().double(), (mine - p0[n]).flatten().double()
        assert du_ref.norm().item() > 0, n
        cos = float((du * du_ref).sum() / (du.norm() * du_ref.norm() + 1e-30))
        ratio = float(du.norm() / (du_ref.norm() + 1e-30))
        worst_cos = min(worst_cos, cos)
        worst_ratio = ratio if abs(ratio - 1) > abs(worst_ratio - 1) else worst_ratio
        assert cos >= SD_ORACLE_UPDATE_COS_MIN["xattn"], (n, cos)
        assert abs(ratio - 1.0) < SD_ORACLE_UPDATE_NORM_TOL["xattn"], (n, ratio)
    print(f"SD xattn fused: min per-tensor update cosine {worst_cos:.4f}, worst norm ratio {worst_ratio:.4f}")
