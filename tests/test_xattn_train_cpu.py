"""CPU: the host side of the differentiable fused cross-attention (sfron_xattn_fwd_lse, sfron_xattn_bwd, sfron_xattn_bwd_ws_bytes).

ABI surface (header <-> ctypes, ABI version 16), and the check of the GPU test's own bound: a float64 restatement of the backward that
rounds O, P, dS and the outputs to bf16 where the kernel does and takes lse in fp32 differs from exact float64, on the GPU test's
inputs, by at most HALF of the bound tests/test_gpu_xattn_train.py holds the kernel to (relative 2-norm 2e-2 per (sample, head) for each
of dQ, dK, dV: the bound of tests/test_gpu_attention_grid.py).  The inputs, cases and both references live here; the GPU test imports them."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_TOL = 2e-2                 # relative 2-norm per (sample, head): tests/test_gpu_attention_grid.py's backward bound
POISON = 3.0e4                  # what the padded key / value rows hold (tests/test_gpu_ddim.py)

# B, H, N, hd, Lv, Lk.  The first eight are the issue's; then the two shapes at which the kernel takes another path: chunks of more than
# one 64-row tile (B H ntile above the 1024-workgroup target) and hd 160 with more than 80 keys (K / V staged again per tile).
CASES = [(2, 2, 64, 40, 77, 80), (1, 2, 128, 80, 77, 80), (1, 1, 64, 160, 77, 80), (1, 2, 16, 40, 5, 8), (1, 1, 80, 80, 128, 128),
         (1, 1, 1, 40, 1, 8), (2, 8, 200, 40, 77, 80), (1, 2, 1100, 40, 77, 80), (2, 8, 4167, 40, 77, 80), (1, 1, 70, 160, 128, 128)]


def inputs(B, H, N, hd, Lv, Lk, seed):
    """q, kv as _xattn_inputs of tests/test_gpu_ddim.py (q 1.5 randn, k / v 1.2 randn, padded rows 3e4) plus dO = randn, all bf16"""
    g = torch.Generator().manual_seed(seed)
    C = H * hd
    q = (torch.randn(B * N, C, generator=g) * 1.5).to(torch.bfloat16)
    kv = (torch.randn(B, Lk, 2 * C, generator=g) * 1.2).to(torch.bfloat16)           # k = columns 0 .. C-1, v = C .. 2C-1: ldk = ldv = 2C
    kv[:, Lv:] = POISON
    d_o = torch.randn(B * N, C, generator=g).to(torch.bfloat16)
    return q, kv.reshape(B * Lk, 2 * C), d_o


def _heads(q, kv, d_o, B, H, N, hd, Lv, Lk):
    qd = q.double().view(B, N, H, hd).permute(0, 2, 1, 3)
    k = kv.double().view(B, Lk, 2, H, hd)[:, :Lv, 0].permute(0, 2, 1, 3)
    v = kv.double().view(B, Lk, 2, H, hd)[:, :Lv, 1].permute(0, 2, 1, 3)
    g = d_o.double().view(B, N, H, hd).permute(0, 2, 1, 3)
    return qd, k, v, g


def _bf(x):
    return x.to(torch.bfloat16).double()


def reference(q, kv, d_o, B, H, N, hd, Lv, Lk, restate=False):
    """float64 from the bf16 inputs -> dict of [B][H][...] tensors: s (scaled scores), lse, o, dq [N][hd], dk / dv [Lv][hd].
    restate: round where the kernel rounds -- O to bf16 (delta's operand), lse to fp32, P and dS to bf16 as MFMA operands, outputs to bf16."""
    qd, k, v, g = _heads(q, kv, d_o, B, H, N, hd, Lv, Lk)
    scale = hd ** -0.5
    s = qd @ k.transpose(-1, -2) * scale
    lse = torch.logsumexp(s, -1)
    if restate:
        lse = lse.float().double()
    p = torch.exp(s - lse[..., None])
    o = (_bf(p) if restate else p) @ v
    if restate:                                       # the forward normalises after the product: O = (bf16(e) V) / l, same rounding class
        o = _bf(o)
    delta = (g * o).sum(-1, keepdim=True)
    dp = g @ v.transpose(-1, -2)
    ds = scale * p * (dp - delta)
    if Lv == 1:                                       # one key: P = 1 and dP = delta analytically; float64 would leave its own rounding noise
        ds = torch.zeros_like(ds)
    p_op, ds_op = (_bf(p), _bf(ds)) if restate else (p, ds)
    dq, dk, dv = ds_op @ k, ds_op.transpose(-1, -2) @ qd, p_op.transpose(-1, -2) @ g
    if restate:
        dq, dk, dv = _bf(dq), _bf(dk), _bf(dv)
    return dict(s=s, lse=lse, o=o, dq=dq, dk=dk, dv=dv)


def head_rel(a, b):
    """relative 2-norm per (sample, head) of [B][H][rows][hd] tensors; a head whose reference is exactly 0 must be exactly 0"""
    num, den = (a - b).flatten(2).norm(dim=2), b.flatten(2).norm(dim=2)
    inf = torch.full_like(num, float("inf"))
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, inf, torch.zeros_like(num)))


def test_new_symbols_header_and_ctypes_agree():
    from sfron import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfron.h")).read(), flags=re.S)
    kinds = {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}
    for name, rtype in (("sfron_xattn_fwd_lse", "int"), ("sfron_xattn_bwd_ws_bytes", "int64_t"), ("sfron_xattn_bwd", "int")):
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
    # sfron_xattn_fwd_lse = sfron_xattn_fwd's arguments with lse in front of the stream
    fwd, lse = _lib._PROTOS["sfron_xattn_fwd"][1], _lib._PROTOS["sfron_xattn_fwd_lse"][1]
    assert lse == fwd[:-1] + [ctypes.c_void_p] + fwd[-1:]
    assert _lib.ABI_VERSION == 17          # additive: the ABI version stays


def test_library_exports_the_entry_points():
    from sfron import _lib
    L = _lib.lib()
    assert L.sfron_abi_version() == 17
    for name in ("sfron_xattn_fwd_lse", "sfron_xattn_bwd_ws_bytes", "sfron_xattn_bwd"):
        assert getattr(L, name) is not None
    # one fp32 slab [2][Lk][hd] per (sample, head, chunk); never more chunks than 64-row tiles, and B H chunks near 1024 when there are more tiles
    assert L.sfron_xattn_bwd_ws_bytes(1, 64, 80, 1, 40) == 2 * 80 * 40 * 4
    assert L.sfron_xattn_bwd_ws_bytes(1, 1100, 80, 2, 40) == 2 * 18 * 2 * 80 * 40 * 4
    assert L.sfron_xattn_bwd_ws_bytes(8, 4096, 80, 8, 40) == 64 * 16 * 2 * 80 * 40 * 4
    assert L.sfron_xattn_bwd_ws_bytes(0, 64, 80, 1, 40) == 0


def test_flags_exist_and_default_off():
    import inspect
    from sfron import sd, sd_unet
    assert inspect.signature(sd.SDSFRon.__init__).parameters["fused_xattn"].default is False
    src = inspect.getsource(sd_unet.UNetModel.__init__)
    assert "self.fused_cross_attention_train = False" in src and "self.fused_cross_attention = False" in src


@pytest.mark.parametrize("B,H,N,hd,Lv,Lk", CASES)
def test_bf16_restatement_within_half_the_gpu_bound(B, H, N, hd, Lv, Lk):
    q, kv, d_o = inputs(B, H, N, hd, Lv, Lk, seed=N + hd + Lv)
    exact = reference(q, kv, d_o, B, H, N, hd, Lv, Lk)
    rest = reference(q, kv, d_o, B, H, N, hd, Lv, Lk, restate=True)
    for name in ("dq", "dk", "dv"):
        worst = float(head_rel(rest[name], exact[name]).max())
        print(f"xattn bwd restatement B{B} H{H} N{N} hd{hd} Lv{Lv}/{Lk} {name}: worst rel {worst:.3e} / bound {GRAD_TOL / 2:.1e}")
        assert worst <= GRAD_TOL / 2, (name, worst)
    if Lv == 1:                                       # one key: P = 1, dS = 0 exactly
        assert not exact["dq"].any() and not exact["dk"].any()
        assert torch.equal(exact["dv"], _heads(q, kv, d_o, B, H, N, hd, Lv, Lk)[3].sum(2, keepdim=True))
