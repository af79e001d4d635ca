"""GPU: the CLIP text encoder (sfron.text over csrc/text.hip + gemm.hip) -- each new kernel against torch, the whole encoder against the
reference fixture (tests/golden/text_encoder.npz: FrozenCLIPEmbedder over a small seeded CLIPTextModel) and, at the ViT-L/14 shape of SD v1,
against the fp64 restatement of tests/test_text_encoder_cpu.py, and prompt contexts through one SDSFRon step.
Bounds: 2 x the value measured on MI355X (written next to each)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_text_encoder_cpu import clip_fp32, fixture_config, fixture_tokenizer, fixture_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def tfx(golden_dir):
    import os
    return dict(np.load(os.path.join(golden_dir, "text_encoder.npz")))


def _L():
    from sfron import _lib
    return _lib.lib()


def fixture_encoder(tfx, tmp_dir):
    from sfron import text
    cfg, heads = fixture_config(tfx)
    return text.CLIPTextEncoder.from_state_dict(fixture_weights(tfx), heads=heads, tokenizer=fixture_tokenizer(tfx, tmp_dir))


# ------------------------------------------------------------------------------------------------ kernels
def test_clip_embed_bit_exact_and_error_word():
    from sfron._lib import ptr, stream_ptr
    g = torch.Generator().manual_seed(1)
    V, P, D, B, T = 1000, 77, 768, 3, 77
    tok, pos = torch.randn(V, D, generator=g).to(DEV), torch.randn(P, D, generator=g).to(DEV)
    ids = torch.randint(0, V, (B, T), generator=g).to(DEV)
    out = torch.full((B * T, D), 7.0, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert _L().sfron_clip_embed(ptr(ids), B, T, ptr(tok), V, ptr(pos), D, ptr(out), ptr(err), stream_ptr()) == 0
    want = (tok[ids] + pos[:T][None]).reshape(B * T, D)
    assert torch.equal(out, want) and int(err.item()) == 0
    bad = ids.clone()
    bad[1, 5], bad[2, 0] = V, -3
    assert _L().sfron_clip_embed(ptr(bad), B, T, ptr(tok), V, ptr(pos), D, ptr(out), ptr(err), stream_ptr()) == 0
    assert int(err.item()) == 1
    rows = out.view(B, T, D)
    assert torch.equal(rows[1, 5], torch.zeros(D, device=DEV)) and torch.equal(rows[2, 0], torch.zeros(D, device=DEV))
    keep = torch.ones(B, T, dtype=torch.bool)
    keep[1, 5] = keep[2, 0] = False
    assert torch.equal(rows[keep.to(DEV)], want.view(B, T, D)[keep.to(DEV)])


def _qkv(B, T, H, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B * T, 3 * H * 64, generator=g) * 1.5).to(torch.bfloat16).to(DEV)


def _attn_ref(qkv, B, T, H):
    x = qkv.double().view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    s = q @ k.transpose(-1, -2) * 0.125
    s = s.masked_fill(torch.ones(T, T, dtype=torch.bool, device=qkv.device).triu(1), float("-inf"))
    return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B * T, H * 64)


def _attn(qkv, B, T, H):
    from sfron._lib import ptr, stream_ptr
    o = torch.full((B * T, H * 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    assert _L().sfron_attn_causal_fwd(ptr(qkv), ptr(o), B, T, H, 64, stream_ptr()) == 0
    return o


ATTN_TOL = 6.5e-3      # max |o - ref| / max |ref|; measured on MI355X: 3.25e-3 (T 80, B 1, H 2), 0 at T = 1


@pytest.mark.parametrize("T", [1, 16, 77, 80, 128])
@pytest.mark.parametrize("B,H", [(1, 2), (3, 12), (3, 2), (1, 12)])
def test_attn_causal_vs_fp64(T, B, H):
    qkv = _qkv(B, T, H, seed=T * 100 + B * 10 + H)
    o = _attn(qkv, B, T, H)
    ref = _attn_ref(qkv, B, T, H)
    err = ((o.double() - ref).abs().max() / ref.abs().max()).item()
    print(f"attn_causal T={T} B={B} H={H}: rel max err {err:.2e}")
    assert torch.isfinite(o.float()).all()
    assert err < ATTN_TOL, err


def test_attn_causal_is_causal():
    B, T, H, D = 2, 77, 12, 768
    qkv = _qkv(B, T, H, seed=5)
    base = _attn(qkv, B, T, H).view(B, T, D)
    g = torch.Generator().manual_seed(6)
    for i in (0, 15, 16, 40, 75):
        other = qkv.clone().view(B, T, 3 * D)
        other[:, i + 1:, D:] = (torch.randn(B, T - i - 1, 2 * D, generator=g) * 3).to(torch.bfloat16).to(DEV)
        o = _attn(other.view(B * T, 3 * D), B, T, H).view(B, T, D)
        assert torch.equal(o[:, :i + 1], base[:, :i + 1]), i
        assert not torch.equal(o[:, i + 1:], base[:, i + 1:]), i


def test_attn_causal_refuses_other_shapes():
    from sfron._lib import ptr, stream_ptr
    qkv = torch.zeros(2 * 192 * 3 * 128, dtype=torch.bfloat16, device=DEV)
    o = torch.zeros(2 * 192 * 128, dtype=torch.bfloat16, device=DEV)
    for T, H, hd in ((129, 2, 64), (192, 2, 64), (0, 2, 64), (77, 2, 72), (77, 1, 128), (16, 4, 32)):
        assert _L().sfron_attn_causal_fwd(ptr(qkv), ptr(o), 1, T, H, hd, stream_ptr()) == 1002, (T, H, hd)
    assert torch.count_nonzero(o).item() == 0


def _gemm(a, w, M, N, K, bias, epi, c_bf16=None, c_f32=None, accumulate=0):
    from sfron import _lib
    d = _lib.GemmDesc(A=a.data_ptr(), B=w.data_ptr(), M=M, N=N, K=K, lda=K, ldb=K, epilogue=epi, alpha=1.0, bias=bias.data_ptr(),
                      c_bf16=c_bf16.data_ptr() if c_bf16 is not None else None, ldc_bf16=N,
                      c_f32=c_f32.data_ptr() if c_f32 is not None else None, ldc_f32=N, tokens=1, accumulate=accumulate)
    return _L().sfron_gemm_bf16(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)


QGELU_TOL = 6.5e-3     # max |c - ref| / (1 + |ref|) (bf16 output); measured on MI355X: 3.11e-3 (M 9856, the 128 x 128 tile; 3.10e-3 generic)


@pytest.mark.parametrize("M", [2 * 77, 8 * 77, 32 * 77, 128 * 77])
def test_gemm_quick_gelu_vs_torch(M):
    from sfron import _lib
    N, K = 3072, 768
    g = torch.Generator().manual_seed(M)
    a = (torch.randn(M, K, generator=g)).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16).to(DEV)
    b = (torch.randn(N, generator=g) * 0.5).to(DEV)
    c = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    assert _gemm(a, w, M, N, K, b, _lib.EPI_QUICK_GELU, c_bf16=c) == 0
    r = a.float() @ w.float().T + b
    ref = r * torch.sigmoid(1.702 * r)
    err = ((c.float() - ref).abs() / (1 + ref.abs())).max().item()
    print(f"quick_gelu M={M}: max err {err:.2e}")
    assert err < QGELU_TOL, err
    # refused where it does not apply
    assert _gemm(a, w, M, N, K, b, _lib.EPI_QUICK_GELU, c_bf16=c, accumulate=1) == 1001


RESID_TOL = 2.5e-5     # max |x - ref| (fp32 output, unit-scale operands); measured on MI355X: 1.14e-5 (M 19712, K 3072)


@pytest.mark.parametrize("M", [2 * 77, 128 * 77, 256 * 77])
@pytest.mark.parametrize("K", [768, 3072])
def test_gemm_residual_bias_accumulate(M, K):
    """out_proj / fc2: x += o W^T + b (SFRON_EPI_F32, accumulate = 1, bias) on every tile the token counts reach."""
    from sfron import _lib
    N = 768
    g = torch.Generator().manual_seed(M + K)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    x0 = torch.randn(M, N, generator=g).to(DEV)
    x = x0.clone()
    assert _gemm(a, w, M, N, K, b, _lib.EPI_F32, c_f32=x, accumulate=1) == 0
    ref = x0 + (a.float() @ w.float().T + b)
    err = (x - ref).abs().max().item()
    print(f"residual M={M} K={K}: max err {err:.2e}")
    assert err < RESID_TOL, err


@pytest.mark.parametrize("rows,D", [(154, 768), (77, 128), (5, 1000)])
def test_layernorm_f32_vs_torch(rows, D):
    from sfron._lib import ptr, stream_ptr
    g = torch.Generator().manual_seed(rows)
    x = (torch.randn(rows, D, generator=g) * 3 + 1).to(DEV)
    x[0] *= 40                                                   # a large-magnitude row, like CLIP's BOS
    gam, bet = (torch.randn(D, generator=g) * 0.3 + 1).to(DEV), (torch.randn(D, generator=g) * 0.2).to(DEV)
    y = torch.empty(rows, D, device=DEV)
    assert _L().sfron_layernorm_fwd_f32(ptr(x), ptr(gam), ptr(bet), rows, D, 1e-5, ptr(y), stream_ptr()) == 0
    ref = F.layer_norm(x.double(), (D,), gam.double(), bet.double(), 1e-5)
    err = (y.double() - ref).abs().max().item()
    print(f"layernorm_f32 rows={rows} D={D}: max err {err:.2e}")
    assert err < 1.7e-6, err          # measured on MI355X: 8.5e-7 (154 x 768)


# ------------------------------------------------------------------------------------------------ the encoder
FIXTURE_TOL = 2.3e-2   # max |h - reference| over all tokens (hidden std 1); measured on MI355X: 1.15e-2 (mean 1.6e-3)


def test_encoder_matches_reference_fixture(tfx, tmp_path):
    enc = fixture_encoder(tfx, str(tmp_path))
    prompts = [str(p) for p in tfx["prompts"]]
    got = enc(prompts)
    assert got.dtype == torch.float32 and tuple(got.shape) == tfx["hidden"].shape
    want = torch.from_numpy(tfx["hidden"]).to(DEV)
    err = (got - want).abs().max().item()
    print(f"fixture encoder: max err {err:.2e}, mean {(got - want).abs().mean().item():.2e}")
    assert err < FIXTURE_TOL, err
    # ids straight in: the same bits; a shorter sequence is the prefix (causal)
    ids = torch.from_numpy(tfx["ids"])
    assert torch.equal(enc.encode_ids(ids), got)
    assert (enc.encode_ids(ids[:, :20]) - got[:, :20]).abs().max().item() < FIXTURE_TOL
    with pytest.raises(ValueError):
        bad = ids.clone()
        bad[0, 3] = int(tfx["config"][0])
        enc.encode_ids(bad)


def _vit_l_weights(seed=7):
    """SD v1's text encoder shape (49408 x 768, 12 layers, 12 heads, MLP 3072) with seeded random weights in HF naming; the BOS token's
    embedding carries a few large channels, so that its hidden row has the large magnitude of the real model's."""
    from sfron import text
    specs, _ = text.param_specs()
    g = torch.Generator().manual_seed(seed)
    w = {}
    D = 768
    for n, shp in specs.items():
        if ".qkv_proj." in n:
            parts = ("q_proj", "k_proj", "v_proj")
            sub = (D, D) if n.endswith("weight") else (D,)
            for p in parts:
                w["text_model." + n.replace("qkv_proj", p)] = torch.randn(sub, generator=g) * (D ** -0.5 if n.endswith("weight") else 0.02)
            continue
        if n.endswith("weight") and len(shp) == 2 and "embedding" not in n:
            t = torch.randn(shp, generator=g) * shp[1] ** -0.5
        elif "token_embedding" in n:
            t = torch.randn(shp, generator=g) * 0.02
            t[49406, :8] = 100.0
        elif "position_embedding" in n:
            t = torch.randn(shp, generator=g) * 0.01
        elif "norm" in n and n.endswith("weight"):
            t = 1 + 0.1 * torch.randn(shp, generator=g)
        else:
            t = 0.02 * torch.randn(shp, generator=g)
        w["text_model." + n] = t
    return w


VIT_TOL = 1.7e-2       # max over token rows of max |h - ref| / max |ref| of the row; measured on MI355X: 8.4e-3 (BOS rows 4.7e-4, at 2.8 x the others' magnitude)


def test_encoder_vit_l_shape_vs_fp64_and_deterministic():
    from sfron import text
    w = _vit_l_weights()
    enc = text.CLIPTextEncoder.from_state_dict(w)
    assert (enc.vocab, enc.D, enc.L, enc.H, enc.F) == (49408, 768, 12, 12, 3072)
    g = torch.Generator().manual_seed(8)
    ids = torch.full((3, 77), 49407, dtype=torch.int64)
    ids[:, 0] = 49406
    for b, n in enumerate((5, 30, 75)):
        ids[b, 1:1 + n] = torch.randint(0, 49406, (n,), generator=g)
    got = enc.encode_ids(ids)
    again = enc.encode_ids(ids)
    assert torch.equal(got, again)
    canon = {k: v.to(DEV, torch.float64) for k, v in text.canonical_state_dict(w, enc.specs).items()}
    ref = clip_fp32(canon, ids.to(DEV), 12, 12)
    row_err = ((got.double() - ref).abs().amax(-1) / ref.abs().amax(-1))
    bos_scale = ref[:, 0].abs().max().item() / ref[:, 1:].abs().amax(-1).mean().item()
    print(f"ViT-L/14 shape: worst row rel err {row_err.max().item():.2e} (BOS rows {row_err[:, 0].max().item():.2e}, "
          f"BOS magnitude {bos_scale:.1f} x the other rows)")
    assert row_err.max().item() < VIT_TOL, row_err.max().item()


# ------------------------------------------------------------------------------------------------ prompts into the SD step
def test_sd_step_with_prompt_contexts_equals_tensor_contexts(tfx, tmp_path):
    from test_gpu_sd import SMALL, _pair
    from sfron import sd
    enc = fixture_encoder(tfx, str(tmp_path))
    cfg = dict(SMALL, context_dim=enc.D)
    B, S = 2, 8
    g = torch.Generator().manual_seed(40)
    xf = torch.randn(B, 4, S, S, generator=g).to(DEV)
    forget = dict(x_f=xf, x_p=xf, t=torch.randint(0, 1000, (B,), generator=g).to(DEV), noise=torch.randn(B, 4, S, S, generator=g).to(DEV))
    remain = dict(x=torch.randn(B, 4, S, S, generator=g).to(DEV), t=torch.randint(0, 1000, (B,), generator=g).to(DEV),
                  noise=torch.randn(B, 4, S, S, generator=g).to(DEV))
    res, ctx = [], None
    for from_prompts in (True, False):
        _, model = _pair(cfg, seed=41)
        ldm = sd.LatentDiffusion(model, cond_stage_model=enc)
        if from_prompts:
            c_f = ldm.get_learned_conditioning(["a photo of a nude person"] * B)            # nsfw_removal.py:132-137
            c_p = ldm.get_learned_conditioning(["a photo of a person wearing clothes"] * B)
            ctx = (c_f.clone(), c_p.clone())
            assert tuple(c_f.shape) == (B, 77, enc.D)
        else:
            c_f, c_p = ctx
        run = sd.SDSFRon(model, lr=1e-4, train_method="full")
        out = run.step(dict(forget, c_f=c_f, c_p=c_p), dict(remain, c=c_p))
        torch.cuda.synchronize()
        res.append((model.params.clone(), out["forget_loss"].item(), out["remain_loss"].item()))
    assert res[0][1:] == res[1][1:]
    assert torch.equal(res[0][0], res[1][0])
