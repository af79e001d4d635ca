"""CPU: the host side of the fused wide-head self-attention (csrc/wattn.hip: sfron_wattn_supported, sfron_wattn_fwd,
sfron_wattn_bwd_ws_bytes, sfron_wattn_bwd), and the check of the GPU test's own bound.

ABI surface: the four symbols are exported, header and ctypes prototypes agree, the ABI version stays 16 (additive), the
sfron_wattn_supported truth table, the workspace size.  The opt-in switches exist and default to off.

The bound.  tests/test_gpu_wattn.py holds O, dQ, dK and dV to a relative 2-norm of 2e-2 per (sample, head) against float64 -- the bound of
tests/test_gpu_attention_grid.py.  `restate` below is a float64 restatement that rounds to bf16 where the kernels round: the unnormalised
P of each 64-key chunk before P V, O, P and dS before the three gradient products, delta from the rounded O, lse to fp32, the gradients
themselves (the construction of test_gpu_attention_grid.test_restatement_uses_under_half_the_bound).  With that module's inputs (qkv
1.0 randn, the stress rows times 3, d_o 0.2 randn) it stays under 1e-2, half the bound, in every per-head norm at T 64 / 256 and head widths
160 / 256 -- the wider contraction did not need the inputs scaled down (INPUT_SCALE = 1.0).  The inputs, cases and both references live
here; the GPU test imports them."""
import ctypes
import functools
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 2e-2                    # relative 2-norm per (sample, head): tests/test_gpu_attention_grid.py
INPUT_SCALE, SPIKE = 1.0, 3.0   # deviation of q / k / v, factor of the stress rows (tests/test_gpu_attention_grid.py SCALE, SPIKE)
ACCEPTED = [(64, 160), (256, 256), (1024, 160)]
REFUSED = [(16, 256), (96, 160), (1088, 160), (256, 128), (256, 80), (256, 168)]


# ------------------------------------------------------------------------------------------------ inputs, reference, restatement
def stress_rows(T):
    """(spiky key of the first chunk, spiky key of the last chunk, spiky query, all-zero query), as tests/test_gpu_attention_grid._rows"""
    return 5, T - 3, 9, 11


@functools.lru_cache(maxsize=None)
def inputs(B, H, T, hd):
    """qkv bf16 [B*T][3 D] (column = which * D + head * hd + i) and d_o bf16 [B*T][D]"""
    gen = torch.Generator().manual_seed(1000 * T + hd + 7 * B + H)
    D = H * hd
    qkv = (torch.randn(B, T, 3 * D, generator=gen) * INPUT_SCALE).to(torch.bfloat16)
    k_first, k_last, q_spiky, q_zero = stress_rows(T)
    qkv[:, k_first, D:2 * D] *= SPIKE
    qkv[:, k_last, D:2 * D] *= SPIKE            # the running maximum moves at the last 64-key chunk
    qkv[:, q_spiky, :D] *= SPIKE
    qkv[:, q_zero, :D] = 0.0                    # uniform P, lse = log T
    d_o = (torch.randn(B, T, D, generator=gen) * 0.2).to(torch.bfloat16)
    return qkv.view(B * T, 3 * D), d_o.view(B * T, D)


def split(qkv, B, H, T, hd):
    """[B*T][3 D] -> q, k, v [B][H][T][hd]"""
    return qkv.view(B, T, 3, H, hd).permute(2, 0, 3, 1, 4).unbind(0)


@functools.lru_cache(maxsize=None)
def reference(B, H, T, hd):
    """float64 from the bf16 inputs: O [B*T][D], lse [B][H][T], d qkv [B*T][3 D], and the lse allowance of the GPU test
    4 hd 2^-24 scale max_j sum_i |q_i k_ji| + 1e-5 per row [B][H][T].  Computed once per shape, never modified."""
    qkv, d_o = inputs(B, H, T, hd)
    D, scale = H * hd, hd ** -0.5
    x = qkv.double().requires_grad_(True)
    q, k, v = split(x, B, H, T, hd)
    s = (q @ k.transpose(-2, -1)) * scale
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(B * T, D)
    o.backward(d_o.double())
    qa, ka = q.detach().abs(), k.detach().abs()
    lse_tol = 4 * hd * 2.0 ** -24 * scale * (qa @ ka.transpose(-2, -1)).amax(-1) + 1e-5
    return o.detach(), torch.logsumexp(s.detach(), -1), x.grad.detach(), lse_tol


def _bf(x):
    return x.to(torch.bfloat16).double()


def restate(B, H, T, hd):
    """The kernels' rounding points in float64 (the products and sums themselves exact): O [B*T][D], d qkv [B*T][3 D]"""
    qkv, d_o = inputs(B, H, T, hd)
    D, scale = H * hd, hd ** -0.5
    q, k, v = split(qkv.double(), B, H, T, hd)
    do = d_o.double().view(B, T, H, hd).transpose(1, 2)
    s = q @ k.transpose(-2, -1) * scale
    m = torch.full((B, H, T), -math.inf, dtype=torch.float64)
    l = torch.zeros(B, H, T, dtype=torch.float64)
    acc = torch.zeros(B, H, T, hd, dtype=torch.float64)
    for c0 in range(0, T, 64):                                 # the online softmax over 64-key chunks
        sc = s[..., c0:c0 + 64]
        mn = torch.maximum(m, sc.amax(-1))
        alpha = torch.exp(m - mn)
        p = torch.exp(sc - mn[..., None])
        l = l * alpha + p.sum(-1)
        acc = acc * alpha[..., None] + _bf(p) @ v[:, :, c0:c0 + 64]
        m = mn
    o = _bf(acc / l[..., None])
    lse = (m + torch.log(l)).float().double()
    P = torch.exp(s - lse[..., None])
    delta = (do * o).sum(-1)
    dS = P * (do @ v.transpose(-2, -1) - delta[..., None]) * scale
    P, dS = _bf(P), _bf(dS)
    dq, dk, dv = _bf(dS @ k), _bf(dS.transpose(-2, -1) @ q), _bf(P.transpose(-2, -1) @ do)
    g = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(B * T, 3 * D)
    return o.transpose(1, 2).reshape(B * T, D), g


def head_errors(got, ref, B, H, T, hd, parts):
    """Relative 2-norm error per (sample, part, head) of [B*T][parts * D] against ref, over all columns of the head and over its last
    eight (tests/test_gpu_attention_grid._head_errors).  Returns two [B][parts][H] tensors."""
    got, ref = got.double().view(B, T, parts, H, hd), ref.view(B, T, parts, H, hd)
    out = []
    for lo in (0, hd - 8):
        num = (got[..., lo:] - ref[..., lo:]).pow(2).sum((1, 4)).sqrt()
        den = ref[..., lo:].pow(2).sum((1, 4)).sqrt()
        out.append(num / den.clamp_min(1e-6 * (T * (8 if lo else hd)) ** 0.5))
    return out


# ------------------------------------------------------------------------------------------------ ABI
NEW = (("sfron_wattn_supported", "int"), ("sfron_wattn_fwd", "int"), ("sfron_wattn_bwd_ws_bytes", "int64_t"), ("sfron_wattn_bwd", "int"))


def test_library_exports_the_four_symbols_and_abi_stays_16():
    from sfron import _lib
    L = _lib.lib()
    assert L.sfron_abi_version() == 17 and _lib.ABI_VERSION == 17          # additive: the ABI version stays
    for name, _ in NEW:
        assert getattr(L, name) is not None


def test_header_and_ctypes_agree():
    from sfron import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfron.h")).read(), flags=re.S)
    kinds = {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}
    for name, rtype in NEW:
        m = re.search(r"\b" + rtype + r"\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, f"{name} is not declared in include/sfron.h"
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib._PROTOS[name]
        assert res is kinds[rtype] and len(args) == len(params), (name, len(args), len(params))
        for at, p in zip(args, params):
            if "*" in p:
                assert at is ctypes.c_void_p, (name, p, at)
            else:
                assert at is kinds[p.split()[0]], (name, p, at)


def test_supported_truth_table():
    from sfron import _lib
    L = _lib.lib()
    for T, hd in ACCEPTED:
        assert L.sfron_wattn_supported(T, hd) == 1, (T, hd)
    for T, hd in REFUSED:
        assert L.sfron_wattn_supported(T, hd) == 0, (T, hd)
    # every multiple of 64 up to 1024 at both widths, nothing else
    for hd in (160, 256):
        for T in range(0, 1200, 16):
            assert L.sfron_wattn_supported(T, hd) == int(T % 64 == 0 and 64 <= T <= 1024), (T, hd)


def test_workspace_is_positive_and_grows_with_the_batch():
    from sfron import _lib
    L = _lib.lib()
    for T, hd, H in ((64, 160, 8), (256, 256, 1), (1024, 160, 1)):
        sizes = [L.sfron_wattn_bwd_ws_bytes(B, T, H, hd) for B in (1, 2, 3, 8, 64)]
        assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:])), sizes
        assert all(s % 16 == 0 and s >= B * H * T * 4 for s, B in zip(sizes, (1, 2, 3, 8, 64)))      # delta, fp32 [B*H*T]
    assert L.sfron_wattn_bwd_ws_bytes(0, 64, 1, 160) == 0


def test_flags_exist_and_default_off():
    import inspect
    from sfron import ddim, ddpm, sd, sd_unet, unet
    assert inspect.signature(ddpm.DDPMSFRon.__init__).parameters["fused_attn"].default is False
    assert inspect.signature(sd.SDSFRon.__init__).parameters["fused_wide_attn"].default is False
    assert inspect.signature(ddim.DDIMSampler.__init__).parameters["fused_wide_attn"].default is False
    assert "self.fused_attention = False" in inspect.getsource(unet.Conditional_Model.__init__)
    assert "self.fused_wide_self_attention = False" in inspect.getsource(sd_unet.UNetModel.__init__)


# ------------------------------------------------------------------------------------------------ the bound
@pytest.mark.parametrize("T", [64, 256])
@pytest.mark.parametrize("hd", [160, 256])
def test_restatement_uses_under_half_the_bound(hd, T):
    B, H = 2, 3
    o_ref, _, g_ref, _ = reference(B, H, T, hd)
    o, g = restate(B, H, T, hd)
    worst = [0.0, 0.0]
    for got, ref, parts in ((o, o_ref, 1), (g, g_ref, 3)):
        for i, err in enumerate(head_errors(got, ref, B, H, T, hd, parts)):
            worst[i] = max(worst[i], float(err.max()))
    print(f"[wattn] restatement T {T} hd {hd} (input scale {INPUT_SCALE}): worst per-head relative error {worst[0]:.2e}, "
          f"last 8 columns {worst[1]:.2e} / {BOUND / 2:.0e}")
    assert worst[0] < BOUND / 2 and worst[1] < BOUND / 2, worst
