"""Reference for the DiT row, reduction and conditioning kernels (csrc/norm.hip, csrc/embed.hip, the quantising LN twin in csrc/fp8.hip):
plain restatements of the reference model's expressions (DiT/models.py:19-20 modulate, :41-59 timestep_embedding, :78-94 LabelEmbedder,
:113-121 the adaLN block, :243 c = t + y) and of the reduction formulas include/sfron.h states.  Every function takes `dtype`: float64 is
the reference, float32 -- the same code on the CPU -- is the yardstick the bounds are built from.  Nothing here calls a kernel;
tests/test_dit_rows_ref_cpu.py holds each float64 restatement to torch autograd on the reference's own expression.

Helpers for the GPU tests (tests/test_gpu_dit_rows.py):
  guarded()     a device view inside a sentinel-filled allocation + a checker that every sentinel survived
  bound32()     fp32 outputs:  max|got - ref64| <= 4 max|ref32 - ref64| + 4 * 2^-24 max|ref64|
  bound_bf16()  bf16 outputs:  every |got - ref64| <= 2^-8 |ref64| + 4 max|ref32 - ref64|, and got != bf16(ref64) on at most 0.2 %
                               (of all elements, or of those a cap_mask names: tests/unet_rows_ref.py)
  check_e4m3()  e4m3 bytes:    decoded within half an e4m3 step of ref64 * scale plus the bf16 slack times scale; at most 0.2 % differ
                               from oracle.fp8_ref.e4m3_bytes(ref64, scale)
The factor 4 covers a summation order that differs from the yardstick's but is as long (a wave butterfly over D, chunk order over rows) and
1-2 ulp device expf / sqrtf; the second term of bound32 is four fp32 ulps of the largest value, for outputs whose yardstick error is exactly
zero (sums of bf16 values are exact in fp32 at these sizes).  The 0.2 % cap is a condition, not a measurement: the float32 restatement
itself disagrees with bf16(ref64) on 0 .. 4.4e-5 of the elements (tests/test_dit_rows_ref_cpu.py asserts the cap for it at every shape).
RECORD collects, per named output, the largest ratio and mismatch share seen (printed by the GPU module at teardown)."""
import math

import torch

LN_EPS = 1e-6
MARGIN = 4.0
BF16_REL = 2.0 ** -8
SHARE_CAP = 0.002
RECORD = {}


def _rec(name, key, v):
    if name is not None:
        d = RECORD.setdefault(name, {})
        d[key] = max(d.get(key, 0.0), float(v))


# ------------------------------------------------------------------------------------------------ the expressions
def sample_of_row(M, T):
    return torch.arange(M) // T


def ln_modulate_fwd(x, shift, scale, T, dtype, eps=LN_EPS):
    """x [M][D], shift / scale [B][D] (row b serves rows b T .. b T + T - 1) -> out [M][D], mean [M], rstd [M]"""
    x, shift, scale = x.to(dtype), shift.to(dtype), scale.to(dtype)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    b = sample_of_row(x.shape[0], T)
    out = (x - mean[:, None]) * rstd[:, None] * (1.0 + scale[b]) + shift[b]
    return out, mean, rstd


def chunk_sums(v, rows):
    """[M][D] -> [M / rows][D]: sums over `rows` consecutive rows"""
    M, D = v.shape
    return v.view(M // rows, rows, D).sum(1)


def ln_modulate_bwd(d_out, x, scale, T, rows, dtype, eps=LN_EPS):
    """backward of ln_modulate_fwd wrt x, and the column sums the adaLN Linear's gradient needs:
    -> dx [M][D] (the LN path's gradient alone), p_shift = chunk sums of d_out, p_scale = chunk sums of d_out * xhat ([M / rows][D])"""
    d_out, x, scale = d_out.to(dtype), x.to(dtype), scale.to(dtype)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * rstd
    g = d_out * (1.0 + scale[sample_of_row(x.shape[0], T)])
    m1 = g.mean(1, keepdim=True)
    m2 = (g * xhat).mean(1, keepdim=True)
    dx = rstd * (g - m1 - xhat * m2)
    return dx, chunk_sums(d_out, rows), chunk_sums(d_out * xhat, rows)


def gate_bwd(dy, branch, gate, T, rows, dtype):
    """backward of x + gate.unsqueeze(1) * branch wrt branch and gate: d_branch = dy * gate[b]; chunk sums of dy * branch and of dy"""
    dy, branch, gate = dy.to(dtype), branch.to(dtype), gate.to(dtype)
    return dy * gate[sample_of_row(dy.shape[0], T)], chunk_sums(dy * branch, rows), chunk_sums(dy, rows)


def ln_gate_bwd(d_out, x, scale, dx0, accumulate, branch, gate, T, rows, dtype, eps=LN_EPS):
    """the fused form: the LN backward lands on dx0 (or replaces it), the gate backward reads the freshly formed dx
    -> dx, p_shift, p_scale, d_branch, p_gate, p_dy"""
    dln, ps, pc = ln_modulate_bwd(d_out, x, scale, T, rows, dtype, eps)
    dx = dx0.to(dtype) + dln if accumulate else dln
    db, pg, pd = gate_bwd(dx, branch, gate, T, rows, dtype)
    return dx, ps, pc, db, pg, pd


def sample_sums(p, B):
    """per-chunk partial rows [B * per][D] -> per-sample sums [B][D]"""
    return p.view(B, p.shape[0] // B, p.shape[1]).sum(1)


def timestep_embed(t, dim, dtype):
    """cos(t f) || sin(t f), f_j = exp(-ln(1e4) j / half): frequencies and arguments in fp32 as the reference forms them
    (t[:, None].float() * freqs), the cosine / sine of that fp32-rounded argument in `dtype`"""
    half = dim // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half)
    args = (t[:, None].float() * freqs[None]).to(dtype)
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


def silu(x, dtype):
    x = x.to(dtype)
    return x / (1.0 + torch.exp(-x))


def silu_grad(x, dtype):
    x = x.to(dtype)
    s = 1.0 / (1.0 + torch.exp(-x))
    return s * (1.0 + x * (1.0 - s))


def labels_used(y, drop, num_classes):
    """dropped or out-of-range labels go to row num_classes (the null class)"""
    bad = (y < 0) | (y >= num_classes)
    if drop is not None:
        bad = bad | drop.bool()
    return torch.where(bad, torch.full_like(y, num_classes), y)


def cond_fwd(t_emb, table, y, drop, num_classes, dtype):
    """c = t_emb + table[label]; silu(c)"""
    c = t_emb.to(dtype) + table.to(dtype)[labels_used(y, drop, num_classes)]
    return c, silu(c, dtype)


def cond_bwd(d_silu_c, c, y, drop, num_classes, table0, dtype):
    """d_c = d_silu_c * silu'(c); d_table = table0 with d_c's rows added onto their labels' rows"""
    d_c = d_silu_c.to(dtype) * silu_grad(c, dtype)
    return d_c, table0.to(dtype).clone().index_add_(0, labels_used(y, drop, num_classes), d_c)


def gated_bias_grads(S, gate, ldg, gate_stride, gate_which, layers, B, D, dtype):
    """include/sfron.h: out[l][which][c] = sum_b gate[b ldg + l gate_stride + which gate_which + c] * S[((2 l + which) B + b) D + c]
    (S and gate flat) -> [layers][2][D]; the caller places row (l, which) at l * out_stride + out_which{0,1}"""
    S, gate = S.to(dtype).reshape(-1), gate.to(dtype).reshape(-1)
    out = torch.zeros(layers, 2, D, dtype=dtype)
    c = torch.arange(D)
    for l in range(layers):
        for which in range(2):
            for b in range(B):
                out[l, which] += gate[b * ldg + l * gate_stride + which * gate_which + c] * S[((2 * l + which) * B + b) * D + c]
    return out


def weighted_reduce(P, w, dtype):
    """include/sfron.h: out[c] = sum_g w[g][c] * sum_j P[g][j][c];  P [groups][per][D], w [groups][D]"""
    return (w.to(dtype) * P.to(dtype).sum(1)).sum(0)


def colsum(X, dtype):
    return X.to(dtype).sum(0)


# ------------------------------------------------------------------------------------------------ bounds
def _f64(t):
    return t.detach().cpu().double()


def bound32(got, ref64, ref32, name=None, margin=MARGIN):
    got, ref64, ref32 = _f64(got), _f64(ref64), _f64(ref32)
    assert got.shape == ref64.shape == ref32.shape, (name, got.shape, ref64.shape, ref32.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    err = float((got - ref64).abs().max())
    yard = float((ref32 - ref64).abs().max())
    ulp = 2.0 ** -24 * float(ref64.abs().max())
    if yard > 0:
        _rec(name, "ratio", err / yard)
    _rec(name, "ulps_of_max", err / ulp if ulp > 0 else 0.0)
    assert err <= margin * yard + 4 * ulp, f"{name}: max|got - ref64| = {err:.4g} > {margin} * {yard:.4g} + 4 * {ulp:.4g}"
    return err, yard


def to_bf16(ref64):
    return ref64.to(torch.float32).to(torch.bfloat16)


def bound_bf16(got, ref64, ref32, name=None, margin=MARGIN, cap_mask=None):
    """cap_mask (bool, got's shape; default: every element): the elements the mismatch-share cap is taken over, for outputs whose float32
    restatement itself comes close to the cap on the others (tests/unet_rows_ref.py).  The error bound applies to every element."""
    assert got.dtype == torch.bfloat16, (name, got.dtype)
    got, ref64, ref32 = _f64(got), _f64(ref64), _f64(ref32)
    assert got.shape == ref64.shape == ref32.shape, (name, got.shape, ref64.shape, ref32.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    yard = float((ref32 - ref64).abs().max())
    err = (got - ref64).abs()
    slack = BF16_REL * ref64.abs() + margin * yard
    differs = got != _f64(to_bf16(ref64))
    if cap_mask is None:
        share = float(differs.double().mean())
    else:
        cap_mask = cap_mask.detach().cpu().bool()
        assert cap_mask.shape == got.shape, (name, cap_mask.shape, got.shape)
        share = float(differs[cap_mask].double().mean()) if bool(cap_mask.any()) else 0.0
        _rec(name, "share_all", float(differs.double().mean()))
    _rec(name, "excess", float((err / slack.clamp_min(1e-300)).max()))
    _rec(name, "share", share)
    if yard > 0:
        _rec(name, "ratio", float(err.max()) / yard)
    bad = err > slack
    assert not bad.any(), (f"{name}: {int(bad.sum())} elements past 2^-8 |ref64| + {margin} * {yard:.4g}; worst |got - ref64| = "
                           f"{float(err[bad].max()):.4g}")
    assert share <= SHARE_CAP, f"{name}: {share:.4%} of the elements differ from bf16(ref64) (cap {SHARE_CAP:.1%})"
    return share


def e4m3_decode(b):
    return b.detach().cpu().contiguous().view(torch.float8_e4m3fn).double()


def check_e4m3(got_bytes, ref64, ref32, scale, name=None, margin=MARGIN):
    """half an e4m3 step (3 mantissa bits, smallest normal exponent -6) taken at |target| + slack: a value the slack carries over a power of
    two rounds on the coarser grid above it"""
    from oracle import fp8_ref
    ref64, ref32 = _f64(ref64), _f64(ref32)
    dec = e4m3_decode(got_bytes)
    assert torch.isfinite(dec).all(), f"{name}: NaN codes"
    target = (ref64 * scale).clamp(-448.0, 448.0)
    slack = scale * (BF16_REL * ref64.abs() + margin * float((ref32 - ref64).abs().max()))
    e = torch.floor(torch.log2((target.abs() + slack).clamp_min(2.0 ** -6)))
    half = 0.5 * 2.0 ** (e - 3)
    err = (dec - target).abs()
    bad = err > half + slack
    want = fp8_ref.e4m3_bytes(ref64, scale)
    share = float((got_bytes.detach().cpu() != want).double().mean())
    _rec(name, "share", share)
    assert not bad.any(), f"{name}: {int(bad.sum())} bytes further than half a step + slack; worst {float(err[bad].max()):.4g}"
    assert share <= SHARE_CAP, f"{name}: {share:.4%} of the bytes differ from e4m3(ref64 * scale) (cap {SHARE_CAP:.1%})"
    return share


# ------------------------------------------------------------------------------------------------ guarded device buffers
GUARD_BYTES = 4096
_SENT = {torch.float32: (torch.int32, 0x7FC00A5A), torch.bfloat16: (torch.int16, 0x7FC5),
         torch.uint8: (torch.uint8, 0xA5), torch.int32: (torch.int32, 0x25A5A5A5), torch.int64: (torch.int64, 0x25A5A5A5A5A5A5A5)}


def guarded(shape, dtype, ld=None, device="cuda:0"):
    """-> (view, check).  `view` has `shape`, rows `ld` elements apart (default: dense), starts 16-byte aligned and lies inside one
    allocation whose every other element -- the gaps between rows and GUARD_BYTES before and after -- holds a sentinel (NaN for fp32, a
    NaN bit pattern for bf16, 0xA5 bytes, 0x25A5.. words for int32 / int64); the view itself starts out as sentinels too.  check(what) asserts that every sentinel outside
    the view is unchanged.  check.full / check.inside give the whole allocation's bits and the view's place in it."""
    shape = tuple(shape)
    width = shape[-1]
    rows = 1
    for s in shape[:-1]:
        rows *= s
    ld = width if ld is None else ld
    assert ld >= width
    itype, sent = _SENT[dtype]
    es = torch.empty(0, dtype=dtype).element_size()
    pad = GUARD_BYTES // es
    full = torch.full((2 * pad + rows * ld,), sent, dtype=itype, device=device)
    inside = torch.zeros(full.shape, dtype=torch.bool, device=device)
    inside[pad:pad + rows * ld].view(rows, ld)[:, :width] = True
    body = full.view(dtype)[pad:pad + rows * ld]
    view = body.as_strided(shape[:-1] + (width,), _strides(shape, ld))
    assert view.data_ptr() % 16 == 0

    def check(what=""):
        hit = full[~inside] != sent
        assert not hit.any(), f"{what}: {int(hit.sum())} guard elements were overwritten"

    check.full, check.inside, check.sentinel = full, inside, sent
    return view, check


def _strides(shape, ld):
    st = [1]
    if len(shape) > 1:
        st.insert(0, ld)
        for s in reversed(shape[1:-1]):
            st.insert(0, st[0] * s)
    return tuple(st)


def untouched(check, what=""):
    """the whole allocation, the view included, still holds the sentinel (an entry point that refused its arguments launched nothing)"""
    assert bool((check.full == check.sentinel).all()), f"{what}: the buffer was written to"


# ------------------------------------------------------------------------------------------------ shapes and inputs shared by both test files
# (B, T, D): M = B T rows.  sfron_ln_modulate_fwd(_q) picks RPW 4 at M >= 8192 with T % 4 == 0, RPW 2 at M >= 4096 with T % 2 == 0, else 1
FWD_SHAPES = [(3, 16, 144), (3, 5, 1280), (3, 1, 4), (16, 256, 64), (1366, 6, 16), (32, 256, 64), (683, 12, 16), (2731, 3, 16),
              (3, 16, 256), (3, 16, 260)]
FWD_RPW = {(3, 16, 144): 1, (3, 5, 1280): 1, (3, 1, 4): 1, (16, 256, 64): 2, (1366, 6, 16): 2, (32, 256, 64): 4, (683, 12, 16): 4,
           (2731, 3, 16): 1, (3, 16, 256): 1, (3, 16, 260): 1}
# (T, D) at B = 3.  pick_chunk(T): rows per chunk 32 / 16 / 8 / 4 with the LDS combine, 2 / 1 (one wave's rows) without
BWD_SHAPES = ([(T, 144) for T in (256, 48, 24, 12, 6, 5, 1)] + [(256, 1152), (6, 1152)]
              + [(T, D) for T in (16, 6) for D in (4, 256, 260, 768, 772, 1280)])
ROWS_PER_CHUNK = {256: 32, 64: 16, 48: 16, 24: 8, 12: 4, 6: 2, 5: 1, 1: 1, 16: 16}


def fwd_rpw(M, T):
    """restatement of the launcher's template choice"""
    return 4 if M >= 8192 and T % 4 == 0 else 2 if M >= 4096 and T % 2 == 0 else 1


def row_inputs(B, T, D, shifted=False, seed=0):
    """x fp32 [M][D] (randn * 2 + 0.3, or the shifted variant randn + 8 whose |mean| * rstd is large); mod fp32 [B][6 D]: every sample
    its own rows (shift at 3 D, scale at 4 D, gate at 2 D as adaLN's chunk(6) lays them out; amplitude 0.5, 0.1 for the shifted variant so
    that -mean * rstd, the value a lane past the row end holds, exceeds every live output); d_out / branch bf16, dx0 / dy fp32"""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * B + 104729 * T + D + (1 if shifted else 0))
    M = B * T
    x = torch.randn(M, D, generator=g) + 8.0 if shifted else torch.randn(M, D, generator=g) * 2 + 0.3
    mod = torch.randn(B, 6 * D, generator=g) * (0.1 if shifted else 0.5)
    d_out = (torch.randn(M, D, generator=g) * 0.1).to(torch.bfloat16)
    branch = torch.randn(M, D, generator=g).to(torch.bfloat16)
    dx0 = torch.randn(M, D, generator=g) * 0.1
    return dict(x=x, mod=mod, shift=mod[:, 3 * D:4 * D].contiguous(), scale=mod[:, 4 * D:5 * D].contiguous(),
                gate=mod[:, 2 * D:3 * D].contiguous(), d_out=d_out, branch=branch, dx0=dx0)
