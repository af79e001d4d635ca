"""Reference for the row-wise and elementwise kernels of the DDPM U-Net and the SD / ldm transformer block (csrc/rows.hip): plain
restatements of the reference models' expressions (SD/ldm/modules/attention.py:37-45 GEGLU, :223-225 LayerNorm, DDPM/models/diffusion.py:17-35
get_timestep_embedding, :131 Dropout, :168-186 the AttnBlock softmax, :340-357 the guidance mix, :370-376 the class-embedding select) and of
what include/sfron.h states about each entry point.  Every arithmetic function takes `dtype`: float64 is the reference, float32 -- the same
code on the CPU -- is the yardstick the bounds are built from.  Nothing here calls a kernel; tests/test_unet_rows_ref_cpu.py holds each
float64 restatement to torch's own operator or autograd.

The bounds, the guarded buffers and RECORD are those of tests/dit_rows_ref.py (bound32, bound_bf16 with its 0.2 % mismatch-share cap,
guarded, untouched).  The cap is a condition the float32 restatement itself must meet, so it is applied only where that restatement stays
far inside it (measured on the CPU, float32 against float64; tests/test_unet_rows_ref_cpu.py asserts each line):
  LayerNorm y, D = 1 .. 2048                  <= 3.5e-5      all elements
  softmax p                                   0              the cases whose scaled logits stay within 16 of the row maximum
  GEGLU forward, gate ~ 1.5 randn             0.13 - 0.17 %  over all elements -- too close to the cap: the 1 + erf cancellation on
                                                             negative gates; <= 1.1e-5 over the elements with gate >= -2: those
  GEGLU backward                              0.10 %         over all elements; 5e-5 over the elements with gate >= -1: those
  timestep embedding                          0              rows with t <= 7; 0.29 % at t up to 999, dim 512: those rows get the
                                                             error bound alone
Elements outside a cap set still get bound_bf16's error bound.

The shape lists the GPU module runs live here so that the CPU module can assert the cap for the yardstick at exactly those shapes."""
import math

import numpy as np
import torch

from dit_rows_ref import RECORD, bound32, bound_bf16, guarded, to_bf16, untouched  # noqa: F401  (re-exported for the two test modules)

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


# ------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_fwd(x, gamma, beta, eps, dtype):
    """x [rows][D] -> y = (x - mean) rstd gamma + beta, mean [rows], rstd [rows] = 1 / sqrt(biased variance + eps)"""
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean[:, None]) * rstd[:, None] * gamma + beta, mean, rstd


def layernorm_rows_per_block(rows):
    """csrc/rows.hip: about 512 workgroups, a multiple of 4 rows each, 16 .. 64"""
    r = ((rows + 511) // 512 + 3) // 4 * 4
    return min(max(r, 16), 64)


def block_sums(v, rpb):
    """[rows][D] -> [ceil(rows / rpb)][D]: sums over rpb consecutive rows, the last block short"""
    rows, D = v.shape
    nblk = -(-rows // rpb)
    full = torch.zeros(nblk * rpb, D, dtype=v.dtype)
    full[:rows] = v
    return full.view(nblk, rpb, D).sum(1)


def layernorm_bwd(dy, x, gamma, eps, dx_prev, accumulate, extra, rpb, dtype):
    """-> dx = (dx_prev + extra) + gradient (dx_prev only with accumulate, extra only when given: the order include/sfron.h states),
    part_gamma = block sums of dy * xhat, part_beta = block sums of dy"""
    dy, x, gamma = dy.to(dtype), x.to(dtype), gamma.to(dtype)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * rstd
    g = dy * gamma
    grad = rstd * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    head = None
    if accumulate:
        head = dx_prev.to(dtype)
    if extra is not None:
        head = extra.to(dtype) if head is None else head + extra.to(dtype)
    dx = grad if head is None else head + grad
    return dx, block_sums(dy * xhat, rpb), block_sums(dy, rpb)


# (rows, D).  Forms of sfron_layernorm_fwd / _bwd: _r<2> D <= 512, _r<3> D <= 768, _r<5> D <= 1280 (D % 4 == 0, 16-byte pointers), else plain
LN_VECTOR_D = (4, 256, 260, 512, 516, 640, 768, 772, 1280)
LN_PLAIN_D = (1284, 2048, 1, 63, 322)
LN_SHAPES = [(37, D) for D in LN_VECTOR_D + LN_PLAIN_D] + [(r, D) for r in (1, 3, 5) for D in (260, 640, 63)]
LN_MISALIGNED_D = (320, 640)
LN_BWD_SHAPES = [(37, D) for D in LN_VECTOR_D + LN_PLAIN_D] + [(8196, 8), (30724, 8), (3, 260), (3, 63)]
LN_EPS = (1e-5, 1e-6)


def ln_form(D):
    return "plain" if D % 4 or D > 1280 else "r2" if D <= 512 else "r3" if D <= 768 else "r5"


def ln_inputs(rows, D, shifted=False):
    """x = 2 randn + 0.5 (shifted: randn + 300, where a one-pass variance would lose everything), gamma around 1, beta, dy, a non-zero dx
    to accumulate onto and the residual stream's term"""
    g = torch.Generator().manual_seed(7919 * rows + D + (1 if shifted else 0))
    r = lambda *s: torch.randn(*s, generator=g)
    x = r(rows, D) + 300.0 if shifted else r(rows, D) * 2 + 0.5
    return dict(x=x, gamma=1.0 + 0.3 * r(D), beta=0.2 * r(D), dy=r(rows, D), dx0=r(rows, D), extra=r(rows, D))


# ------------------------------------------------------------------------------------------------ GEGLU
def geglu_fwd(h, dtype):
    """h [rows][2F] = value || gate -> value * gelu(gate), the exact (erf) GELU of F.gelu"""
    h = h.to(dtype)
    F_ = h.shape[1] // 2
    a, g = h[:, :F_], h[:, F_:]
    return a * (0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0))))


def geglu_bwd(d_out, h, dtype):
    """-> dh [rows][2F]: d value = d_out gelu(gate) || d gate = d_out value gelu'(gate), gelu'(g) = Phi(g) + g phi(g)"""
    d_out, h = d_out.to(dtype), h.to(dtype)
    F_ = h.shape[1] // 2
    a, g = h[:, :F_], h[:, F_:]
    cdf = 0.5 * (1.0 + torch.erf(g / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)
    return torch.cat([d_out * (g * cdf), d_out * a * (cdf + g * pdf)], 1)


GEGLU_TAILS = (0.0, 1e-3, -1e-3, 3.0, -3.0, 6.0, -6.0, 10.0, -10.0, 40.0, -40.0)
# (F, rows, misaligned operand or None).  sfron_geglu_*: float4 form at F % 4 == 0 with aligned pointers (256 threads x 4 columns per column
# block, rows_per_block = ceil(rows / min(4096 / column blocks, rows))), else the grid-stride scalar form (4096 workgroups at the most)
GEGLU_VECTOR = [(4, 7, None), (1024, 3, None), (1028, 3, None), (8, 4099, None)]
GEGLU_PLAIN = [(5, 7, None), (8, 7, "h"), (8, 7, "out"), (8, 7, "d_out"), (1023, 1030, None)]
GEGLU_FWD_CAP_GATE, GEGLU_BWD_CAP_GATE = -2.0, -1.0


def geglu_inputs(rows, F_):
    """value ~ randn, gate ~ 1.5 randn with the first 22 gate elements (in row-major order) set to GEGLU_TAILS twice; d_out ~ randn"""
    g = torch.Generator().manual_seed(104729 * rows + F_)
    h = torch.randn(rows, 2 * F_, generator=g)
    h[:, F_:] *= 1.5
    gate = h[:, F_:].clone().reshape(-1)
    gate[:2 * len(GEGLU_TAILS)] = torch.tensor(GEGLU_TAILS * 2)
    h[:, F_:] = gate.view(rows, F_)
    return h, torch.randn(rows, F_, generator=g)


def geglu_cap_masks(h):
    """the element sets the mismatch-share cap applies to: forward [rows][F], backward [rows][2F] (both halves of dh)"""
    gate = h[:, h.shape[1] // 2:]
    bwd = gate >= GEGLU_BWD_CAP_GATE
    return gate >= GEGLU_FWD_CAP_GATE, torch.cat([bwd, bwd], 1)


# ------------------------------------------------------------------------------------------------ softmax
def softmax_fwd(s, n_valid, scale, dtype):
    """rows of n stored logits of which the first n_valid are keys: softmax(scale * s) there, probability 0 in the padding"""
    z = s.to(dtype)[:, :n_valid] * torch.tensor(scale, dtype=F32).to(dtype)
    e = torch.exp(z - z.max(1, keepdim=True).values)
    p = torch.zeros(s.shape, dtype=dtype)
    p[:, :n_valid] = e / e.sum(1, keepdim=True)
    return p


def softmax_bwd(p_bf16, dp, scale, dtype):
    """ds = scale * p * (dp - sum(p dp)) from the bf16 probabilities the kernel is given"""
    p, dp = p_bf16.to(dtype), dp.to(dtype)
    return torch.tensor(scale, dtype=F32).to(dtype) * p * (dp - (p * dp).sum(1, keepdim=True))


# (rows, n, n_valid, scale); the last one is the large-logit case (30 randn at scale 1), held to the error bound alone
SOFTMAX_CASES = [(5, 3, 3, 1.0), (3, 64, 64, 0.125), (37, 65, 65, 0.079), (37, 80, 77, 0.125), (6, 200, 130, 0.05)]
SOFTMAX_LARGE = (8, 77, 77, 1.0)
SOFTMAX_CAP_SPREAD = 16.0


def softmax_inputs(rows, n, n_valid, scale, large=False):
    """logits whose scaled values are 1.5 randn (large: 30 randn); the padding columns hold 1e30, which no sum or maximum may see"""
    g = torch.Generator().manual_seed(1000003 * rows + 31 * n + n_valid)
    s = torch.randn(rows, n, generator=g) * ((30.0 if large else 1.5) / scale)
    s[:, n_valid:] = 1e30
    return s, torch.randn(rows, n, generator=g)


# ------------------------------------------------------------------------------------------------ layouts, casts, copies, small pieces
def nchw_to_rows(x, c_pad):
    """[B][C][HW] -> [B HW][c_pad], channels C.. zero"""
    B, C, HW = x.shape
    rows = torch.zeros(B * HW, c_pad, dtype=x.dtype)
    rows[:, :C] = x.permute(0, 2, 1).reshape(B * HW, C)
    return rows


def rows_to_nchw(rows, B, C, HW):
    """[B HW][ld] -> [B][C][HW] from columns 0 .. C - 1"""
    return rows[:, :C].reshape(B, HW, C).permute(0, 2, 1).contiguous()


LAYOUT_SHAPES = [(2, 3, 5), (3, 4, 16), (2, 130, 7)]


def cast_rows(x):
    """fp32 -> bf16, round to nearest even"""
    return x.to(BF16)


def tie_values(rows, C, seed):
    """fp32 values for the casts: randn, with every third element moved onto a bf16 rounding tie (the low 16 bits 0x8000: even and odd
    neighbours both occur) and every seventh one bit above / below a tie"""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randn(rows * C, generator=g).view(torch.int32).clone()
    i = torch.arange(rows * C)
    bits[i % 3 == 0] = (bits[i % 3 == 0] & -65536) | 0x8000
    bits[i % 7 == 1] = (bits[i % 7 == 1] & -65536) | 0x8001
    bits[i % 7 == 2] = (bits[i % 7 == 2] & -65536) | 0x7FFF
    return bits.view(F32).view(rows, C)


def axpby(a, b, alpha, beta):
    """two rounded fp32 products and one rounded sum (the library builds with -ffp-contract=off)"""
    return torch.tensor(alpha, dtype=F32) * a + torch.tensor(beta, dtype=F32) * b


def sample_colsum(x, B, HW, dtype):
    """[B HW][C] -> [B][C]"""
    return x.to(dtype).view(B, HW, -1).sum(1)


def pool2_sum(dy, dtype):
    """backward of the nearest x2 upsampling: [B][2H][2W][C] -> [B][H][W][C], the sums of the 2 x 2 blocks"""
    B, H2, W2, C = dy.shape
    return dy.to(dtype).view(B, H2 // 2, 2, W2 // 2, 2, C).sum((2, 4))


# ------------------------------------------------------------------------------------------------ dropout masks
_M64 = (1 << 64) - 1
_GOLDEN, _SALT = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03


def dropout_thresh(p):
    """(unsigned)(p * 65536.0f + 0.5f), in fp32"""
    return int(np.float32(np.float32(p) * np.float32(65536.0)) + np.float32(0.5))


def dropout_mask(seed, counter, salt, n, p):
    """the keep mask of sfron_dropout_mask: elements 4 q .. 4 q + 3 are the four 16-bit fields (low to high) of
    splitmix64(base + (q + 1) * 0x9E37...), base = seed ^ counter * 0x9E37... ^ salt * 0xD1B5... (mod 2^64), kept when the field >= thresh"""
    base = (seed & _M64) ^ ((counter * _GOLDEN) & _M64) ^ ((salt * _SALT) & _M64)
    nq = (n + 3) // 4
    with np.errstate(over="ignore"):
        z = np.uint64(base) + np.arange(1, nq + 1, dtype=np.uint64) * np.uint64(_GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    fields = np.stack([(z >> np.uint64(s)) & np.uint64(0xFFFF) for s in (0, 16, 32, 48)], 1).reshape(-1)[:n]
    return torch.from_numpy((fields >= np.uint64(dropout_thresh(p))).astype(np.uint8))


# ------------------------------------------------------------------------------------------------ DDPM conditioning
def ddpm_timestep_embed(t, dim, dtype):
    """DDPM/models/diffusion.py:17-35 get_timestep_embedding: sin(t f) || cos(t f), f_j = exp(-ln(1e4) j / (half - 1)), half = dim // 2,
    t float; an odd dim gets a zero last column"""
    half = dim // 2
    emb = math.log(10000) / (half - 1)
    emb = torch.exp(torch.arange(half, dtype=dtype) * -emb)
    emb = t.to(dtype)[:, None] * emb[None, :]
    emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=1)
    if dim % 2 == 1:
        emb = torch.nn.functional.pad(emb, (0, 1, 0, 0))
    return emb


TEMB_DIMS = (4, 128, 129, 512)
TEMB_T_SMALL, TEMB_T_LARGE = (0.0, 0.5, 1.0, 3.0, 7.0), (37.0, 250.0, 999.0)


def class_embed_used(c, keep, n_classes):
    """a label inside [0, n_classes) of a kept sample reads its table row; every other sample reads the null row"""
    use = (c >= 0) & (c < n_classes)
    return use if keep is None else use & keep.bool()


def class_embed_fwd(table, null_emb, c, keep, n_classes):
    """DDPM/models/diffusion.py:370-376 -> [n][D] in the table's dtype"""
    use = class_embed_used(c, keep, n_classes)
    return torch.where(use[:, None], table[torch.where(use, c, torch.zeros_like(c))], null_emb[None, :].expand(c.shape[0], -1))


def class_embed_bwd(d, c, keep, n_classes, d_table0, dtype):
    """serially over the batch: d_table[c[b]] += d[b] for the samples that read the table, the others summed (from 0) into d_null, which
    is overwritten.  Adds only: in float32 this is the kernel's arithmetic, operation for operation"""
    use = class_embed_used(c, keep, n_classes)
    d, d_table = d.to(dtype), d_table0.to(dtype).clone()
    d_null = torch.zeros(d.shape[1], dtype=dtype)
    for b in range(d.shape[0]):
        if use[b]:
            d_table[c[b]] += d[b]
        else:
            d_null += d[b]
    return d_table, d_null
