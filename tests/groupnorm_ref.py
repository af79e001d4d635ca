"""Reference for the GroupNorm kernels (csrc/groupnorm.hip): plain restatements of GroupNorm(groups, eps) (+ swish) (+ dropout) on NHWC
rows -- DDPM/models/diffusion.py:38-46,126-131 -- forward and backward, of what include/sfron.h states about each entry point, and of the
launcher's dispatch rule.  Every arithmetic function takes `dtype`: float64 is the reference, float32 -- the same code on the CPU -- is the
yardstick the bounds are built from.  Nothing here calls a kernel; tests/test_groupnorm_ref_cpu.py holds each float64 restatement to
F.group_norm plus autograd, and the restated rule to the library's own host functions.

The bounds, the guarded buffers and RECORD are those of tests/dit_rows_ref.py (bound32, bound_bf16 with its 0.2 % mismatch-share cap,
guarded, untouched).

Sums over the pixels.  torch's float32 sum is pairwise, which is more accurate than any serial order a kernel can use, so a yardstick built
from it would ask more of the kernels than float32 arithmetic gives.  For the three outputs that ARE sums over the pixels of a sample --
part_gamma, part_beta and the column sums of dx -- the float32 yardstick is therefore a serial float32 sum in pixel order,
np.cumsum(..., dtype=np.float32)[-1]; the float64 reference uses torch's sum.  (The kernels add row replicas, then replicas or chunks, in
index order: shorter chains than the serial sum, so they stay inside it.)  Everything else -- the group statistics, k1 / k2, y, dx -- is the
plain expression in `dtype`.

eps and drop_scale cross the C ABI as float: the restatements round both to float32 first, in either dtype.

The case table the GPU module runs lives here (CASES) so that the CPU module can assert, through the restated rule, which kernel family and
sub-form each case reaches, and that the float32 restatement alone meets the mismatch-share cap at every one of them."""
import collections

import numpy as np
import torch

from dit_rows_ref import RECORD, bound32, bound_bf16, guarded, to_bf16, untouched  # noqa: F401  (re-exported for the two test modules)

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
EPS = 1e-6


def f32(v):
    """the value a float argument of the C ABI carries"""
    return float(torch.tensor(v, dtype=F32))


# ------------------------------------------------------------------------------------------------ the expressions
def _act(z, swish):
    return z / (1.0 + torch.exp(-z)) if swish else z


def _act_grad(z):
    s = 1.0 / (1.0 + torch.exp(-z))
    return s * (1.0 + z * (1.0 - s))


def _per_channel(v, cg):
    """[B][groups] -> [B][1][C]"""
    return v.repeat_interleave(cg, 1)[:, None, :]


def _stats(x, groups, eps, dtype):
    """x [B][HW][C] -> mean, rstd [B][groups] (biased variance, as torch.nn.GroupNorm) and xhat [B][HW][C]"""
    B, HW, C = x.shape
    cg = C // groups
    xg = x.to(dtype).view(B, HW, groups, cg)
    mean = xg.mean((1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))
    rstd = 1.0 / torch.sqrt(var + f32(eps))
    xhat = (x.to(dtype) - _per_channel(mean, cg)) * _per_channel(rstd, cg)
    return mean, rstd, xhat


def groupnorm_fwd(x, gamma, beta, groups, eps, swish, mask, drop_scale, dtype):
    """x [B][HW][C], mask uint8 [B][HW][C] or None -> y = act(xhat gamma + beta) (* mask * drop_scale), mean [B][groups], rstd [B][groups]"""
    mean, rstd, xhat = _stats(x, groups, eps, dtype)
    y = _act(xhat * gamma.to(dtype) + beta.to(dtype), swish)
    if mask is not None:
        y = torch.where(mask.bool(), y * f32(drop_scale), torch.zeros((), dtype=dtype))
    return y, mean, rstd


def pixel_sum(v, dtype):
    """[B][HW][C] -> [B][C]: float64 torch's sum; float32 a serial sum in pixel order (see the module docstring)"""
    if dtype == F64:
        return v.sum(1)
    assert v.dtype == F32
    return torch.from_numpy(np.cumsum(v.numpy(), axis=1, dtype=np.float32)[:, -1].copy())


GnBwd = collections.namedtuple("GnBwd", "dx pg pb colsum dx16")


def groupnorm_bwd(dy, x, gamma, beta, groups, eps, swish, mask, drop_scale, dx_prev, accumulate, extra, dtype):
    """dy [B][HW][C] = the gradient wrt y ->
      dx      (dx_prev + extra) + gradient: dx_prev only with accumulate, extra only when given -- the order include/sfron.h states
      pg, pb  [B][C] per-sample sums over the pixels of dz xhat and dz, dz = dy (* mask * drop_scale) (* act'(z))
      colsum  [B][C] per-sample column sums of dx
      dx16    the bf16 rounding of dx"""
    B, HW, C = x.shape
    cg = C // groups
    mean, rstd, xhat = _stats(x, groups, eps, dtype)
    ga = gamma.to(dtype)
    d = dy.to(dtype)
    if mask is not None:
        d = torch.where(mask.bool(), d * f32(drop_scale), torch.zeros((), dtype=dtype))
    if swish:
        d = d * _act_grad(xhat * ga + beta.to(dtype))
    pg, pb = pixel_sum(d * xhat, dtype), pixel_sum(d, dtype)
    dg = d * ga
    k1 = dg.view(B, HW, groups, cg).mean((1, 3))
    k2 = (dg * xhat).view(B, HW, groups, cg).mean((1, 3))
    grad = _per_channel(rstd, cg) * (dg - _per_channel(k1, cg) - xhat * _per_channel(k2, cg))
    head = None
    if accumulate:
        head = dx_prev.to(dtype)
    if extra is not None:
        head = extra.to(dtype) if head is None else head + extra.to(dtype)
    dx = grad if head is None else head + grad
    return GnBwd(dx, pg, pb, pixel_sum(dx, dtype), dx.to(F32).to(BF16))


# ------------------------------------------------------------------------------------------------ the dispatch rule (csrc/groupnorm.hip)
GNB, TPB = 1024, 256


def gn_chunks(B, HW):
    """pixel chunks per sample of the two-phase pair: about 512 workgroups, at most 32, at least 8 pixels each"""
    return max(1, min((512 + B - 1) // B, 32, HW // 8))


def gn3_gpb(B, HW, C, groups):
    """-> (groups per workgroup of the one-launch form, the slab rule that admitted it): (8 | 4 | 2 | 1, "128K"), (8, "512K") or (0, None)"""
    cg = C // groups
    for gpb in (8, 4, 2, 1):
        Cs = gpb * cg
        if groups % gpb or Cs % 16 or Cs > 1024 or HW * Cs * 4 > (128 << 10) or B * (groups // gpb) < 192:
            continue
        return gpb, "128K"
    Cs = 8 * cg
    if groups % 8 == 0 and Cs % 32 == 0 and Cs <= 1024 and HW * Cs * 4 <= (512 << 10) and B * (groups // 8) >= 192:
        return 8, "512K"
    return 0, None


def one_launch(B, HW, C, groups):
    return int(B > 0 and HW > 0 and C > 0 and groups > 0 and C % groups == 0 and C % 4 == 0 and groups <= 64 and gn3_gpb(B, HW, C, groups)[0] > 0)


def bwd_cast_ok(ldx, C, groups):
    return int(C > 0 and groups > 0 and C % groups == 0 and C % 4 == 0 and ldx % 4 == 0 and C <= 2048 and groups <= 64)


def scratch_bytes(B, HW, C, groups):
    if B <= 0 or HW <= 0 or C <= 0 or groups <= 0:
        return 0
    n = gn_chunks(B, HW)
    return max(B * n * groups * 2 * 8, B * n * C * 2 * 4)


def gn2_ok(ldx, ld2, C, groups, scratch, aligned=True):
    """the row-coalesced forms (two-phase and one-launch) take the call; otherwise the per-(sample, group) kernels do.  `aligned`: x, y / dy
    / dx 16-byte (y 8-byte) aligned, the mask 4-byte aligned, the scratch 16-byte aligned"""
    return bool(scratch and aligned and C % 4 == 0 and ldx % 4 == 0 and ld2 % 4 == 0 and C <= 4 * GNB and groups <= 64)


def gn2_stats_lds(C):
    """dynamic LDS bytes of k_gn2_stats: [rows per pass][C][2] doubles"""
    qpr = C // 4
    return (GNB // min(qpr, GNB)) * C * 2 * 8


# ------------------------------------------------------------------------------------------------ the cases
# cls: "gn3.8" "gn3.4" "gn3.2" "gn3.1" (one launch, 128 KB slab rule), "gn3.8w" (one launch, 512 KB rule), "gn2" (two-phase pair),
# "gn1" (per-(sample, group) kernels).  scratch False: NULL scratch; ldx_pad: x rows C + ldx_pad apart; x_mis: x 4 bytes past a 16-byte line
Case = collections.namedtuple("Case", "name B HW C groups cls scratch ldx_pad x_mis gpu")


def _c(B, HW, C, groups, cls, scratch=True, ldx_pad=0, x_mis=False, gpu=True):
    name = f"{cls}-{B}x{HW}x{C}g{groups}" + ("" if scratch else "-noscratch") + (f"-ldx{ldx_pad}" if ldx_pad else "") + ("-xmis" if x_mis else "")
    return Case(name, B, HW, C, groups, cls, scratch, ldx_pad, x_mis, gpu)


CASES = [
    _c(48, 9, 64, 32, "gn3.8"),          # one pass holds 256 row replicas, HW has 9 rows
    _c(48, 25, 1280, 32, "gn3.8"),       # 80 quads per row, 12 replicas, 64 idle threads
    _c(24, 25, 128, 64, "gn3.8"),        # 64 groups
    _c(64, 1024, 128, 32, "gn3.8"),      # slab exactly 128 KB
    _c(24, 529, 256, 32, "gn3.4"),
    _c(64, 9, 48, 12, "gn3.4"),          # groups not a multiple of 8
    _c(64, 1025, 128, 32, "gn3.4"),      # one pixel over the 128 KB line
    _c(12, 529, 512, 32, "gn3.2"),
    _c(6, 529, 1024, 32, "gn3.1"),
    _c(192, 9, 16, 1, "gn3.1"),
    _c(48, 729, 384, 32, "gn3.8w"),
    _c(47, 9, 64, 32, "gn2"),            # one workgroup short of 192
    _c(3, 9, 64, 32, "gn2"),             # 1 chunk
    _c(3, 100, 320, 32, "gn2"),          # 12 uneven chunks: the 8 + 4 partials loop
    _c(3, 1000, 128, 32, "gn2"),         # 32 chunks that do not divide HW
    _c(3, 72, 2048, 32, "gn2"),          # the widest bwd_cast, 9 chunks
    _c(2, 25, 4096, 32, "gn2"),          # the widest row form: k_gn2_stats asks for exactly 64 KB of LDS
    _c(3, 25, 64, 64, "gn2"),            # one channel per group
    _c(3, 9, 4, 1, "gn2"),
    _c(3, 9, 256, 1, "gn2"),             # one group of 256 channels
    _c(2, 25, 96, 32, "gn2"),            # 3 channels per group: every quad straddles two groups
    _c(64, 1024, 320, 32, "gn2", gpu=False),
    _c(48, 9, 64, 32, "gn1", scratch=False),
    _c(3, 100, 320, 32, "gn1", scratch=False),
    _c(2, 25, 30, 3, "gn1"),             # C % 4 != 0
    _c(2, 9, 128, 128, "gn1"),           # more than 64 groups
    _c(2, 9, 4128, 32, "gn1"),           # C > 4096, 129 channels per group
    _c(3, 9, 256, 1, "gn1", scratch=False),      # 256 channels per group, one slot
    _c(2, 25, 96, 32, "gn1", scratch=False),     # 3 channels per group, 85 slots and one idle thread
    _c(3, 100, 320, 32, "gn1", ldx_pad=2),
    _c(3, 9, 64, 32, "gn1", x_mis=True),
]
GPU_CASES = [c for c in CASES if c.gpu]
SRC_CASES = [c for c in CASES if c.name in ("gn3.8-48x9x64g32", "gn3.4-24x529x256g32", "gn3.2-12x529x512g32", "gn3.1-6x529x1024g32",
                                            "gn3.8w-48x729x384g32")]
CONST_CASES = [c for c in CASES if c.name in ("gn3.8-48x9x64g32", "gn3.4-64x9x48g12", "gn2-3x100x320g32", "gn1-2x25x96g32-noscratch")]


def classify(c, ldx_more=0, lddx_more=0):
    """the family and sub-form the restated rule sends a case to (ldx_more / lddx_more: further padding a run adds to the row strides)"""
    ldx = c.C + c.ldx_pad + ldx_more
    if not gn2_ok(ldx, c.C + lddx_more, c.C, c.groups, c.scratch, aligned=not c.x_mis):
        return "gn1"
    gpb, rule = gn3_gpb(c.B, c.HW, c.C, c.groups)
    if not gpb:
        return "gn2"
    return f"gn3.{gpb}" + ("w" if rule == "512K" else "")


# shapes whose first draw leaves the float32 restatement itself past a quarter of the mismatch-share cap (at 1728 elements one mismatch is
# 5.8e-4): they draw from another seed (tests/test_groupnorm_ref_cpu.py asserts the quarter at every case)
RESEED = {(3, 9, 64, 32): 1}


def gn_inputs(c, variant="randn"):
    """x = 1.5 randn + 0.3, gamma around 1, beta small, dy = 0.1 randn, a mask that keeps 90 % with scale 1 / 0.9, a non-zero dx to accumulate
    onto and the residual branch's term.
    variant "int":   dy small integers, mask keeps half with scale 2 -- with swish off every dz is an integer and part_beta an exact integer sum
    variant "const": one group of one sample holds 0.75 everywhere: variance 0, rstd = eps^-1/2, xhat = 0, y = act(beta) there"""
    B, HW, C, groups = c.B, c.HW, c.C, c.groups
    g = torch.Generator().manual_seed(7919 * B + 104729 * HW + 31 * C + groups + {"randn": 0, "int": 1, "const": 2}[variant]
                                     + 1000003 * RESEED.get((B, HW, C, groups), 0))
    x = torch.randn(B, HW, C, generator=g) * 1.5 + 0.3
    gamma, beta = torch.randn(C, generator=g) * 0.5 + 1.0, torch.randn(C, generator=g) * 0.2
    i = dict(x=x, gamma=gamma, beta=beta)
    if variant == "int":
        i["dy"] = torch.randint(-3, 4, (B, HW, C), generator=g).float()
        i["mask"], i["scale"] = (torch.rand(B, HW, C, generator=g) > 0.5).to(torch.uint8), 2.0
    else:
        i["dy"] = torch.randn(B, HW, C, generator=g) * 0.1
        i["mask"], i["scale"] = (torch.rand(B, HW, C, generator=g) > 0.1).to(torch.uint8), f32(1.0 / 0.9)
    i["dx0"], i["extra"] = torch.randn(B, HW, C, generator=g) * 0.1, torch.randn(B, HW, C, generator=g) * 0.1
    if variant == "const":
        cg = C // groups
        i["const"] = (B // 2, groups // 2)
        x[B // 2, :, (groups // 2) * cg:(groups // 2 + 1) * cg] = 0.75
    return i


def stat_close(got, ref64, rtol, atol, what):
    got, ref64 = got.detach().cpu().double().reshape(-1), ref64.double().reshape(-1)
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    bad = ~((got - ref64).abs() <= atol + rtol * ref64.abs())
    assert not bad.any(), f"{what}: {int(bad.sum())} values past rtol {rtol} atol {atol}; worst |got - ref64| = {float((got - ref64).abs()[bad].max()):.4g}"
