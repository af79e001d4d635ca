"""csrc/attn.hip at every head width and sequence-length class its C entry points accept: sfron_attn_fwd, sfron_attn_bwd and
sfron_attn_bwd_bias through the C ABI, against float64 torch on the CPU (softmax(q k^T hd^-0.5) v, its logsumexp, its autograd gradients for a
bf16-rounded d_o) on the same bf16-rounded inputs.  Nothing here calls the library for a reference.

What is compared.  O and LSE per element with the bounds of test_gpu_blocks.test_attention_fwd_bwd (rtol 2e-2 / atol 2e-2; rtol 1e-4 / atol
1e-3); O, dQ, dK and dV each on their own in the 2-norm, relative error below 2e-2 (test_attention_backward_fused_vs_two_kernel_and_torch),
with every norm taken per (sample, head) and once more over the LAST EIGHT COLUMNS of every head alone -- an error confined to one head or to
a head's last d-tile cannot hide under the other heads or parts.  The row of the all-zero query has lse = log T (uniform P, l = T exactly):
asserted to 1e-5, sixteen fp32 ulps at log 512.  Every output is finite.  Two calls of every entry point give the same bits.

Guard regions.  Every tensor handed to the library is carved out of a larger allocation at element offset 8 (16 bytes for bf16: the alignment
the entry points ask for and no more).  Outputs are pre-filled, body and guards, with a fixed bit pattern (a finite 2.3e16): after the call
the 8 leading and 256 trailing elements must hold the same bits -- a store past column hd of the last head of the last row lands there -- and
a body element left unwritten fails the comparison.  Inputs carry NaN guards: a read past the valid columns of the last rows turns up as a
non-finite result.  Nothing addresses memory outside these allocations.

The 2e-2 bound at the widths below 40, where it had not been measured: `_restate` below is a float64 restatement that rounds to bf16 where
the kernels do (attn.hip: the unnormalised P of each 64-key chunk before P V, O, P and dS before the three gradient products, delta from the
rounded O, the gradients themselves; T < 64 keeps P and dS in fp32 and rounds O and the gradients only).  test_restatement_uses_under_half_the_bound
(CPU) asserts, for every case of the grid and of the short path, that this restatement alone stays under 1e-2 -- half the bound -- in every
per-head norm.  At the scale of the existing tests (qkv 1.5 randn, rows times 6) it did not: 1.0e-2 .. 1.7e-2 at every width, 2.3e-2 at
(T 63, hd 1) -- nearly all of it delta = rowsum(dO * O) taken from the bf16 O, against the near-cancelling P (dP - delta) of the saturated
rows -- so, as the bound is not to be widened, the inputs are qkv 1.0 randn with the stress rows times 3 (the spiky key still takes the row
maximum in about one row of six), d_o 0.2 randn; (T 17, hd 20) alone uses 0.8 / times 4.  Worst case per head width over T = 64 .. 512 with
these inputs: relative 2-norm error of the restatement, largest over O / dQ / dK / dV and over (sample, head); in brackets the same over the
last eight columns of a head:

    width  8: 5.5e-3 (5.5e-3)     width 16: 6.0e-3 (5.1e-3)     width 24: 5.7e-3 (6.0e-3)     width 32: 4.5e-3 (4.6e-3)
    width 40: 7.2e-3 (7.7e-3)     width 48: 5.9e-3 (7.4e-3)     width 56: 4.7e-3 (4.6e-3)     width 64: 8.5e-3 (8.1e-3)
    width 72: 7.0e-3 (7.0e-3)     width 80: 6.7e-3 (6.6e-3)     short path (five shapes): 6.0e-3 (6.0e-3)

A per-head norm whose float64 value is zero (T = 1: dQ = dK = 0) is held to 1e-6 per element absolutely."""
import functools
import math

import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1001, 1002        # csrc/common.h
B, H = 2, 3                                          # an inner head, a last head and a second sample
WIDTHS = (8, 16, 24, 32, 40, 48, 56, 64, 72, 80)
LENGTHS = (64, 128, 192, 256, 384, 512)
SHORT = ((1, 8), (63, 128), (17, 20), (63, 1), (33, 72))
LEAD, TAIL = 8, 256                                  # guard elements in front of / behind every tensor
PATTERN = {torch.bfloat16: 0x5AA5, torch.float32: 0x5AA55AA5}
BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
BOUND = 2e-2
SCALE, SPIKE = 1.0, 3.0                              # deviation of q / k / v, factor of the spiky rows (see the module docstring)
SCALE_OF = {(17, 20): (0.8, 4.0)}                    # ... and of the one shape whose restatement passed half the bound with them


# ------------------------------------------------------------------------------------------------ inputs, reference, restatement (CPU)
def _rows(T):
    """(spiky key of the first chunk, spiky key of the last chunk, spiky query, all-zero query); None where T has no room."""
    if T < 16:
        return None
    return 5, T - 3, 9, 11


@functools.lru_cache(maxsize=None)
def _inputs(T, hd):
    gen = torch.Generator().manual_seed(1000 * T + hd)
    D = H * hd
    SCALE, SPIKE = SCALE_OF.get((T, hd), (globals()["SCALE"], globals()["SPIKE"]))
    qkv = (torch.randn(B, T, 3 * D, generator=gen) * SCALE).to(torch.bfloat16)
    rows = _rows(T)
    if rows:
        k_first, k_last, q_spiky, q_zero = rows
        qkv[:, k_first, D:2 * D] *= SPIKE
        qkv[:, k_last, D:2 * D] *= SPIKE          # the running maximum moves at the last 64-key chunk
        qkv[:, q_spiky, :D] *= SPIKE
        qkv[:, q_zero, :D] = 0.0                # uniform P, lse = log T
    d_o = (torch.randn(B, T, D, generator=gen) * 0.2).to(torch.bfloat16)
    return qkv.view(B * T, 3 * D), d_o.view(B * T, D)


def _split(qkv, T, hd):
    """[B*T][3 D] -> q, k, v [B][H][T][hd]."""
    return qkv.view(B, T, 3, H, hd).permute(2, 0, 3, 1, 4).unbind(0)


@functools.lru_cache(maxsize=None)
def _reference(T, hd):
    """float64: O [B*T][D], LSE [B][H][T], d qkv [B*T][3 D].  Computed once per shape, never modified."""
    qkv, d_o = _inputs(T, hd)
    D = H * hd
    x = qkv.double().requires_grad_(True)
    q, k, v = _split(x, T, hd)
    s = (q @ k.transpose(-2, -1)) * hd ** -0.5
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(B * T, D)
    o.backward(d_o.double())
    return o.detach(), torch.logsumexp(s.detach(), -1), x.grad.detach()


def _bf(x):
    return x.to(torch.bfloat16).double()


def _restate(T, hd):
    """The kernels' rounding points in float64 (the products and sums themselves exact): O [B*T][D], d qkv [B*T][3 D]."""
    qkv, d_o = _inputs(T, hd)
    D, scale, tiled = H * hd, hd ** -0.5, T >= 64
    q, k, v = _split(qkv.double(), T, hd)
    do = d_o.double().view(B, T, H, hd).transpose(1, 2)
    s = q @ k.transpose(-2, -1)
    m = torch.full((B, H, T), -math.inf, dtype=torch.float64)
    l = torch.zeros(B, H, T, dtype=torch.float64)
    acc = torch.zeros(B, H, T, hd, dtype=torch.float64)
    step = 64 if tiled else T
    for c0 in range(0, T, step):                               # the online softmax over 64-key chunks
        sc = s[..., c0:c0 + step]
        mn = torch.maximum(m, sc.amax(-1))
        alpha = torch.exp((m - mn) * scale)
        p = torch.exp((sc - mn[..., None]) * scale)
        l = l * alpha + p.sum(-1)
        acc = acc * alpha[..., None] + (_bf(p) if tiled else p) @ v[:, :, c0:c0 + step]
        m = mn
    o = _bf(acc / l[..., None])
    lse = (m * scale + torch.log(l)).float().double()
    P = torch.exp(s * scale - lse[..., None])
    delta = (do * o).sum(-1)
    dS = P * (do @ v.transpose(-2, -1) - delta[..., None]) * scale
    if tiled:
        P, dS = _bf(P), _bf(dS)
    dq, dk, dv = _bf(dS @ k), _bf(dS.transpose(-2, -1) @ q), _bf(P.transpose(-2, -1) @ do)
    g = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(B * T, 3 * D)
    return o.transpose(1, 2).reshape(B * T, D), g


def _head_errors(got, ref, T, hd, parts):
    """Relative 2-norm error per (sample, part, head) of [B*T][parts * D] against ref, over all columns of the head and over its last eight
    (all of them when the head is narrower).  Returns two [B][parts][H] tensors."""
    got, ref = got.double().view(B, T, parts, H, hd), ref.view(B, T, parts, H, hd)
    out = []
    for lo in (0, max(hd - 8, 0)):
        num = (got[..., lo:] - ref[..., lo:]).pow(2).sum((1, 4)).sqrt()
        den = ref[..., lo:].pow(2).sum((1, 4)).sqrt()
        out.append(num / den.clamp_min(1e-6 * (T * min(hd, 8 if lo else hd)) ** 0.5))
    return out


def _assert_heads(got, ref, T, hd, parts, what, bound=BOUND):
    names = ("dQ", "dK", "dV") if parts == 3 else ("O",)
    for err, cols in zip(_head_errors(got, ref, T, hd, parts), ("all columns", "last 8 columns")):
        worst = int(err.argmax())
        b, p, h = (int(i) for i in torch.unravel_index(torch.tensor(worst), err.shape))
        print(f"[grid] {what} T {T} hd {hd} {cols}: worst relative error {float(err.max()):.3e} at {names[p]} sample {b} head {h}")
        assert float(err.max()) < bound, (what, cols, names[p], f"sample {b} head {h}", float(err.max()))


@pytest.mark.parametrize("hd", WIDTHS + ("short",))
def test_restatement_uses_under_half_the_bound(hd):
    """CPU only.  The float64 restatement with the kernels' bf16 rounding points stays under half of the 2e-2 bound in every per-head norm
    of every case below, so the bound leaves the kernels' fp32 arithmetic the other half and needs no widening at the new widths."""
    worst = [0.0, 0.0]
    for T, w in (SHORT if hd == "short" else [(T, hd) for T in LENGTHS]):
        o_ref, _, g_ref = _reference(T, w)
        o, g = _restate(T, w)
        for got, ref, parts in ((o, o_ref, 1), (g, g_ref, 3)):
            for i, err in enumerate(_head_errors(got, ref, T, w, parts)):
                worst[i] = max(worst[i], float(err.max()))
    print(f"[grid] restatement, width {hd}: worst per-head relative error {worst[0]:.2e}, last 8 columns {worst[1]:.2e}")
    assert worst[0] < BOUND / 2 and worst[1] < BOUND / 2, worst


# ------------------------------------------------------------------------------------------------ guarded buffers and the three calls
class _Buf:
    """n elements at offset LEAD of an allocation of LEAD + n + TAIL.  data = None: an output, every element (guards and body) the bit
    pattern.  Otherwise an input: the data between NaN guards."""

    def __init__(self, n, dtype, data=None):
        self.n, self.pat = n, PATTERN[dtype]
        self.big = torch.empty(LEAD + n + TAIL, dtype=dtype, device=DEV)
        self.bits = self.big.view(BITS[dtype])
        if data is None:
            self.bits.fill_(self.pat)
        else:
            self.big.fill_(float("nan"))
            self.big[LEAD:LEAD + n] = data.reshape(-1).to(DEV)
        self.t = self.big[LEAD:LEAD + n]

    def guards_intact(self):
        return bool((self.bits[:LEAD] == self.pat).all()) and bool((self.bits[LEAD + self.n:] == self.pat).all())

    def untouched(self):
        return bool((self.bits == self.pat).all())


class _Case:
    """One (T, hd): the inputs on the device between NaN guards, and the three entry points into freshly patterned outputs."""

    def __init__(self, T, hd):
        from sfron import _lib
        self.L, self.T, self.hd, self.D = _lib.lib(), T, hd, H * hd
        qkv, d_o = _inputs(T, hd)
        self.qkv, self.d_o = _Buf(qkv.numel(), torch.bfloat16, qkv), _Buf(d_o.numel(), torch.bfloat16, d_o)

    def fwd(self):
        from sfron._lib import ptr, stream_ptr
        o, lse = _Buf(B * self.T * self.D, torch.bfloat16), _Buf(B * H * self.T, torch.float32)
        rc = self.L.sfron_attn_fwd(ptr(self.qkv.t), ptr(o.t), ptr(lse.t), B, self.T, H, self.hd, stream_ptr())
        torch.cuda.synchronize()
        return rc, o, lse

    def bwd_inputs(self, o, lse):
        """The forward outputs as backward INPUTS: copied between NaN guards."""
        self.o_in, self.lse_in = _Buf(o.n, torch.bfloat16, o.t), _Buf(lse.n, torch.float32, lse.t)

    def bwd(self):
        from sfron._lib import ptr, stream_ptr
        dqkv, delta = _Buf(B * self.T * 3 * self.D, torch.bfloat16), _Buf(B * H * self.T, torch.float32)
        rc = self.L.sfron_attn_bwd(ptr(self.qkv.t), ptr(self.o_in.t), ptr(self.d_o.t), ptr(self.lse_in.t), ptr(delta.t), ptr(dqkv.t),
                                   B, self.T, H, self.hd, stream_ptr())
        torch.cuda.synchronize()
        return rc, dqkv, delta

    def bwd_bias(self):
        from sfron._lib import ptr, stream_ptr
        dqkv, part = _Buf(B * self.T * 3 * self.D, torch.bfloat16), _Buf(B * 3 * self.D, torch.float32)
        rc = self.L.sfron_attn_bwd_bias(ptr(self.qkv.t), ptr(self.o_in.t), ptr(self.d_o.t), ptr(self.lse_in.t), ptr(dqkv.t), ptr(part.t),
                                        B, self.T, H, self.hd, stream_ptr())
        torch.cuda.synchronize()
        return rc, dqkv, part


def _close(got, ref, rtol, atol, what):
    got = got.double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    over = (got - ref).abs() - (atol + rtol * ref.abs())
    print(f"[grid] {what}: max |err| {float((got - ref).abs().max()):.3e}")
    assert float(over.max()) <= 0.0, f"{what}: {int((over > 0).sum())} of {got.numel()} elements out of tolerance"


def _forward_and_backward(c):
    """Forward and backward of case c by the rule, every check of the module docstring; returns (o, lse, dqkv) buffers."""
    T, hd = c.T, c.hd
    o_ref, lse_ref, g_ref = _reference(T, hd)
    rc, o, lse = c.fwd()
    assert rc == OK, f"sfron_attn_fwd returned {rc}"
    assert o.guards_intact() and lse.guards_intact(), "sfron_attn_fwd stored outside o / lse"
    _close(o.t, o_ref, 2e-2, 2e-2, f"O T {T} hd {hd}")
    _close(lse.t, lse_ref, 1e-4, 1e-3, f"LSE T {T} hd {hd}")
    _assert_heads(o.t.cpu(), o_ref, T, hd, 1, "forward")
    if _rows(T):
        zero_row = lse.t.view(B, H, T)[:, :, _rows(T)[3]].double().cpu()
        assert float((zero_row - math.log(T)).abs().max()) <= 1e-5, ("lse of the all-zero query row", zero_row, math.log(T))
    rc2, o2, lse2 = c.fwd()
    assert rc2 == OK and torch.equal(o.bits, o2.bits) and torch.equal(lse.bits, lse2.bits), "two forward calls differ"

    c.bwd_inputs(o, lse)
    rc, dqkv, delta = c.bwd()
    assert rc == OK, f"sfron_attn_bwd returned {rc}"
    assert dqkv.guards_intact() and delta.guards_intact(), "sfron_attn_bwd stored outside dqkv / delta_scratch"
    assert bool(torch.isfinite(dqkv.t.float()).all()), "non-finite gradient"
    _assert_heads(dqkv.t.cpu(), g_ref, T, hd, 3, "backward")
    rc2, dqkv2, _ = c.bwd()
    assert rc2 == OK and torch.equal(dqkv.bits, dqkv2.bits), "two backward calls differ"
    return o, lse, dqkv


# ------------------------------------------------------------------------------------------------ 1 + 2. the tiled grid
@gpu
@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("hd", WIDTHS)
def test_tiled_grid(hd, T):
    """Every head width the tiled path accepts (templates <64, 2, 3> to 48, <64, 2, 4> to 64, <96, 3, 5> to 80) times every launch class:
    T 64 single-tile forward / two-kernel backward, 128 fused backward KT = 1, 192 forward <..., 1> / two-kernel, 256 fused KT = 2, 384
    forward <..., 2> / two-kernel, 512 k_attn_fwd8 by the rule.  At T = 128 and 256 also the two-kernel form against the same reference and
    against the fused one (6e-3, per head), and sfron_attn_bwd_bias: dqkv bit-identical to the plain call, the partial rows against the
    column sums of the float64 gradient (|a - b| <= 2e-2 sum_t |g| + 1e-6, test_attention_backward_with_qkv_bias_partials)."""
    c = _Case(T, hd)
    _, _, dqkv = _forward_and_backward(c)
    if T not in (128, 256):
        return
    g_ref, D = _reference(T, hd)[2], H * hd
    old = c.L.sfron_attn_bwd_form(2)
    try:
        rc, two, delta = c.bwd()
    finally:
        c.L.sfron_attn_bwd_form(old)
    assert rc == OK and two.guards_intact() and delta.guards_intact()
    assert bool(torch.isfinite(two.t.float()).all())
    _assert_heads(two.t.cpu(), g_ref, T, hd, 3, "two-kernel backward")
    _assert_heads(dqkv.t.cpu(), two.t.double().cpu(), T, hd, 3, "fused against two-kernel", bound=6e-3)

    assert c.L.sfron_attn_bwd_bias_supported(T) == 1
    rc, dq_b, part = c.bwd_bias()
    assert rc == OK, f"sfron_attn_bwd_bias returned {rc}"
    assert dq_b.guards_intact() and part.guards_intact(), "sfron_attn_bwd_bias stored outside dqkv / the partial rows"
    assert torch.equal(dq_b.bits, dqkv.bits), "sfron_attn_bwd_bias: dqkv differs from the plain call"
    rc2, dq_b2, part2 = c.bwd_bias()
    assert rc2 == OK and torch.equal(dq_b.bits, dq_b2.bits) and torch.equal(part.bits, part2.bits), "two sfron_attn_bwd_bias calls differ"
    got = part.t.double().cpu().view(B, 3 * D)
    assert bool(torch.isfinite(got).all())
    want, scale = g_ref.view(B, T, 3 * D).sum(1), g_ref.view(B, T, 3 * D).abs().sum(1)
    over = (got - want).abs() - (2e-2 * scale + 1e-6)
    print(f"[grid] bias partials T {T} hd {hd}: worst |err| / sum|g| {float(((got - want).abs() / (scale + 1e-9)).max()):.3e}")
    assert float(over.max()) <= 0.0, f"bias partials: {int((over > 0).sum())} of {got.numel()} columns out of tolerance"


# ------------------------------------------------------------------------------------------------ 3. the short path at its edges
@gpu
@pytest.mark.parametrize("T,hd", SHORT)
def test_short_path_edges(T, hd):
    """T < 64 (k_attn_small_fwd / _bwd, any width up to 128): one token, the largest accepted LDS request (T 63, hd 128: 162 540 bytes in the
    backward kernel -- the call must return SFRON_OK, not an error of hipFuncSetAttribute), a width that is no multiple of 8, width 1, and
    an odd T at the DiT-XL width.  Same reference, norms and guards as the grid."""
    _forward_and_backward(_Case(T, hd))


# ------------------------------------------------------------------------------------------------ 4. refusals leave outputs alone
@gpu
@pytest.mark.parametrize("T,hd,only_bias,misalign,want", [
    (100, 64, False, 0, ERR_UNSUPPORTED),      # T >= 64 that is no multiple of 64
    (64, 12, False, 0, ERR_UNSUPPORTED),       # tiled path, width not a multiple of 8
    (64, 88, False, 0, ERR_UNSUPPORTED),       # would need a sixth output d-tile
    (16, 136, False, 0, ERR_UNSUPPORTED),      # short path, wider than 128
    (192, 64, True, 0, ERR_UNSUPPORTED),       # sfron_attn_bwd_bias where the backward is the two-kernel form
    (64, 64, False, 1, ERR_ARG),               # qkv one element off 16-byte alignment
])
def test_refusals_leave_outputs_alone(T, hd, only_bias, misalign, want):
    from sfron import _lib
    from sfron._lib import ptr, stream_ptr
    L, D = _lib.lib(), H * hd
    qkv = torch.zeros(B * T * 3 * D + 8, dtype=torch.bfloat16, device=DEV)
    o_in = torch.zeros(B * T * D, dtype=torch.bfloat16, device=DEV)
    d_o = torch.zeros(B * T * D, dtype=torch.bfloat16, device=DEV)
    lse_in = torch.zeros(B * H * T, dtype=torch.float32, device=DEV)
    q = ptr(qkv) + 2 * misalign
    o, lse = _Buf(B * T * D, torch.bfloat16), _Buf(B * H * T, torch.float32)
    dqkv, delta, part = _Buf(B * T * 3 * D, torch.bfloat16), _Buf(B * H * T, torch.float32), _Buf(B * 3 * D, torch.float32)
    s = stream_ptr()
    if not only_bias:
        assert L.sfron_attn_fwd(q, ptr(o.t), ptr(lse.t), B, T, H, hd, s) == want
        assert L.sfron_attn_bwd(q, ptr(o_in), ptr(d_o), ptr(lse_in), ptr(delta.t), ptr(dqkv.t), B, T, H, hd, s) == want
    assert L.sfron_attn_bwd_bias(q, ptr(o_in), ptr(d_o), ptr(lse_in), ptr(dqkv.t), ptr(part.t), B, T, H, hd, s) == want
    torch.cuda.synchronize()
    for name, buf in (("o", o), ("lse", lse), ("dqkv", dqkv), ("delta_scratch", delta), ("bias partials", part)):
        assert buf.untouched(), f"a refused call wrote to {name}"
