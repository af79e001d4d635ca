"""csrc/inception.hip through the C ABI, and sfron.inception.InceptionV3 against the torch restatement (tests/inception_torch_ref.py).

Guard regions, as tests/test_gpu_attention_grid.py: every tensor handed to the library is carved out of a larger allocation at element
offset LEAD (a multiple of 16 bytes); outputs are pre-filled, body and guards, with a fixed bit pattern, and the guards must hold the same
bits after the call; where a row is wider than its live columns (``ld`` > C) the dead columns of an input hold NaN and those of an output
must keep the pattern.  Nothing addresses memory outside these allocations.

Bounds.
  patch matrix, max pools   pure data movement / selection: bit-equal.
  convolution forms         integer inputs in -3 .. 3: every partial sum is an integer below 2^24, exact in fp32 in any order: equal.
  average pool              the kernel adds the window in fp64 (nine fp32 terms: at most 8 roundings of 2^-53 relative to sum |x|), rounds
                            to fp32 once (2^-24 |S|) and divides in fp32 (2^-24 |S / n|): |got - want| <= 2 * 2^-24 |want| (1 + 2^-23) +
                            2^-50 mean|x|; a bf16 output adds its one rounding, 2^-8 |want| (8 significant
                            bits: unit roundoff 2^-8).
  resize                    ``_resize_bound``: the fp32 evaluation of the stated expression plus the one bf16 rounding.
  statistics                ``_cov_bound``: the first-order bound of an n-term fp64 sum of the centred products in any order.
  network                   rel_l2(GPU, fp32 restatement) <= 2 * e_emul per tap, e_emul = rel_l2(bf16-operand emulation, fp32 restatement):
                            the rule and margin of tests/test_gpu_classifier.py."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_torch_ref as ref

gpu = pytest.mark.gpu
DEV = "cuda:0"
OK, ERR_ARG = 0, 1001
LEAD, TAIL = 64, 256
PATTERN = {torch.bfloat16: 0x5AA5, torch.float32: 0x5AA55AA5, torch.float64: 0x5AA55AA55AA55AA5, torch.uint8: 0x5A}
BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64, torch.uint8: torch.uint8}
PATCH_FORMS = [(1, 7, 1, 0, 3), (7, 1, 1, 3, 0), (1, 3, 1, 0, 1), (3, 1, 1, 1, 0), (5, 5, 1, 2, 2), (3, 3, 2, 0, 0), (3, 3, 1, 0, 0)]


def L():
    from sfron import _lib
    return _lib.lib()


def S():
    return torch.cuda.current_stream().cuda_stream


class Carved:
    """A tensor of ``numel`` elements inside a larger allocation pre-filled with the pattern; ``check()`` asserts the guards are intact."""

    def __init__(self, numel, dtype, data=None):
        self.whole = torch.full((LEAD + numel + TAIL,), PATTERN[dtype], dtype=torch.int64, device=DEV).to(BITS[dtype]).view(dtype)
        self.t = self.whole[LEAD:LEAD + numel]
        if data is not None:
            self.t.copy_(data.reshape(-1).to(DEV))
        self.numel, self.dtype = numel, dtype

    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        w = self.whole.view(BITS[self.dtype]).cpu()
        pat = torch.tensor(PATTERN[self.dtype], dtype=torch.int64).to(BITS[self.dtype])
        assert bool((w[:LEAD] == pat).all()) and bool((w[LEAD + self.numel:] == pat).all()), "a guard region was written"

    def untouched(self, mask):
        """the elements of the body selected by ``mask`` still hold the pattern"""
        w = self.t.view(BITS[self.dtype]).cpu()
        pat = torch.tensor(PATTERN[self.dtype], dtype=torch.int64).to(BITS[self.dtype])
        assert bool((w[mask.reshape(-1)] == pat).all()), "a dead column was written"


def rows_with_dead_columns(x, ld):
    """[..., C] -> [..., ld] whose columns C .. ld - 1 hold NaN"""
    out = torch.full(x.shape[:-1] + (ld,), float("nan"), dtype=x.dtype)
    out[..., :x.shape[-1]] = x
    return out


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


# ------------------------------------------------------------------------------------------------ patch matrix
def unfold_rows(x_nhwc, kh, kw, s, ph, pw):
    """F.unfold re-laid to [B * Ho * Wo][(i * kw + j) * C + c]"""
    B, H, W, C = x_nhwc.shape
    u = F.unfold(x_nhwc.permute(0, 3, 1, 2).float(), (kh, kw), padding=(ph, pw), stride=s)          # [B][C * kh * kw][L], c major
    return u.view(B, C, kh * kw, -1).permute(0, 3, 2, 1).reshape(-1, kh * kw * C)


@gpu
@pytest.mark.parametrize("form", PATCH_FORMS)
def test_patch_rows_bit_equal_to_unfold(form):
    kh, kw, s, ph, pw = form
    g = torch.Generator().manual_seed(sum(form))
    for H, W in ((9, 11), (8, 8)):
        for C in (8, 40):
            ld, B = C + 8, 2
            x = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16)
            want = unfold_rows(x, *form).to(torch.bfloat16)
            xin = Carved(B * H * W * ld, torch.bfloat16, rows_with_dead_columns(x, ld))
            out = Carved(want.numel(), torch.bfloat16)
            assert L().sfron_patch_rows(xin.ptr(), ld, B, H, W, C, kh, kw, s, ph, pw, out.ptr(), S()) == OK
            torch.cuda.synchronize()
            out.check()
            assert torch.equal(bits(out.t.cpu()), bits(want.reshape(-1))), (form, H, W, C)


# ------------------------------------------------------------------------------------------------ convolution forms
def int_conv_case(form, C, seed, n_out=12, H=9, W=11, B=2):
    g = torch.Generator().manual_seed(seed)
    kh, kw, s, ph, pw = form
    x = torch.randint(-3, 4, (B, H, W, C), generator=g).float()
    w = torch.randint(-3, 4, (n_out, C, kh, kw), generator=g).float()
    b = torch.randint(-3, 4, (n_out,), generator=g).float()
    want = F.conv2d(x.permute(0, 3, 1, 2), w, b, stride=s, padding=(ph, pw)).permute(0, 2, 3, 1).contiguous()      # NHWC
    assert float(want.abs().max()) < 2 ** 24 and kh * kw * C * 9 + 3 < 2 ** 24
    return x, w, b, want


def check_slice(out, ldc, col, want2d):
    """``want2d`` [rows][n] sits in columns col .. col + n - 1 of the fp32 rows [rows][ldc]; every other column keeps the pattern"""
    got = out.t.cpu().view(-1, ldc)
    n = want2d.shape[1]
    assert torch.equal(got[:, col:col + n], want2d)
    dead = torch.ones(got.shape, dtype=torch.bool)
    dead[:, col:col + n] = False
    out.untouched(dead)
    out.check()


@gpu
@pytest.mark.parametrize("form", PATCH_FORMS)
def test_conv_forms_as_patch_gemm_exact(form):
    from sfron.unet import bgemm
    kh, kw, s, ph, pw = form
    for C in (8, 40):
        x, w, b, want = int_conv_case(form, C, 100 + sum(form) + C)
        B, H, W, _ = x.shape
        n_out, K = w.shape[0], kh * kw * C
        rows = want.shape[0] * want.shape[1] * want.shape[2]
        xin = Carved(x.numel(), torch.bfloat16, x.to(torch.bfloat16))
        pat = Carved(rows * K, torch.bfloat16)
        wt = Carved(n_out * K, torch.bfloat16, w.permute(0, 2, 3, 1).to(torch.bfloat16))
        bias = Carved(n_out, torch.float32, b)
        ldc, col = n_out + 8, 4
        out = Carved(rows * ldc, torch.float32)
        assert L().sfron_patch_rows(xin.ptr(), C, B, H, W, C, kh, kw, s, ph, pw, pat.ptr(), S()) == OK
        bgemm(pat.ptr(), wt.ptr(), rows, n_out, K, lda=K, ldb=K, bias=bias.ptr(), c_f32=out.ptr() + 4 * col, ldc=ldc)
        torch.cuda.synchronize()
        pat.check()
        # the last row's slice ends 4 columns before the row does: those belong to the carved body and must keep the pattern
        check_slice(out, ldc, col, want.reshape(rows, n_out))


@gpu
@pytest.mark.parametrize("form", [(3, 3, 2, 0, 0), (3, 3, 1, 0, 0)])
def test_conv_fwd_pad0_forms_exact(form):
    from sfron import _lib
    from sfron.unet import _conv_desc
    kh, kw, s, ph, pw = form
    for C in (8, 40):
        x, w, b, want = int_conv_case(form, C, 200 + sum(form) + C)
        B, H, W, _ = x.shape
        n_out = w.shape[0]
        ho, wo = want.shape[1], want.shape[2]
        rows = B * ho * wo
        xin = Carved(x.numel(), torch.bfloat16, x.to(torch.bfloat16))
        w32 = Carved(w.numel(), torch.float32, w)
        wt = Carved(n_out * 9 * C, torch.bfloat16)
        bias = Carved(n_out, torch.float32, b)
        ldc, col = n_out + 8, 4
        out = Carved(rows * ldc, torch.float32)
        assert L().sfron_conv_wprep(w32.ptr(), n_out, C, 9, n_out, C, wt.ptr(), None, S()) == OK
        d = _conv_desc(B, H, W, C, ho, wo, n_out, 9, s, ph, 0, 0, bias=bias.ptr(), out_f32=out.ptr() + 4 * col, ld_out=ldc)
        assert L().sfron_conv_fwd(ctypes.byref(d), xin.ptr(), wt.ptr(), S()) == OK
        torch.cuda.synchronize()
        wt.check()
        check_slice(out, ldc, col, want.reshape(rows, n_out))


# ------------------------------------------------------------------------------------------------ pools
POOL_SHAPES = ((7, 9), (8, 8), (5, 5))


def pool_run(kind, x, x_dtype, y_dtype, ld_extra=4, out_extra=12, col=4):
    """x fp32 [B, H, W, C] (rounded to x_dtype) through sfron_pool3 into columns col .. col + C - 1 of rows [.][C + out_extra] -> (y fp32
    [B, Ho, Wo, C], the x values the kernel saw)"""
    B, H, W, C = x.shape
    x = x.to(x_dtype)
    ld, ldo = C + ld_extra, C + out_extra
    Ho, Wo = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if kind == 0 else (H, W)
    xin = Carved(B * H * W * ld, x_dtype, rows_with_dead_columns(x, ld))
    out = Carved(B * Ho * Wo * ldo, y_dtype)
    esz = 2 if y_dtype == torch.bfloat16 else 4
    assert L().sfron_pool3(xin.ptr(), int(x_dtype == torch.bfloat16), ld, B, H, W, C, kind, out.ptr() + esz * col, int(y_dtype == torch.bfloat16),
                           ldo, S()) == OK
    torch.cuda.synchronize()
    out.check()
    got = out.t.cpu().view(B, Ho, Wo, ldo)
    dead = torch.ones(got.shape, dtype=torch.bool)
    dead[..., col:col + C] = False
    out.untouched(dead)
    return got[..., col:col + C].contiguous(), x


@gpu
@pytest.mark.parametrize("kind", [0, 1])
def test_max_pools_bit_equal(kind):
    g = torch.Generator().manual_seed(40 + kind)
    for H, W in POOL_SHAPES:
        for C in (8, 36):
            for xd, yd in ((torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32)):
                x = torch.randn(2, H, W, C, generator=g)
                got, xs = pool_run(kind, x, xd, yd)
                nchw = xs.float().permute(0, 3, 1, 2)
                want = (F.max_pool2d(nchw, 3, 2) if kind == 0 else F.max_pool2d(nchw, 3, 1, 1)).permute(0, 2, 3, 1).to(yd)
                assert torch.equal(bits(got), bits(want)), (kind, H, W, C, xd, yd)


@gpu
def test_average_pool_divides_by_the_in_bounds_count():
    g = torch.Generator().manual_seed(42)
    u = 2.0 ** -24
    for H, W in POOL_SHAPES:
        for C in (8, 36):
            for xd, yd in ((torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32)):
                x = torch.randn(2, H, W, C, generator=g) * 3 + 1
                got, xs = pool_run(2, x, xd, yd)
                nchw = xs.double().permute(0, 3, 1, 2)
                want = F.avg_pool2d(nchw, 3, 1, 1, count_include_pad=False).permute(0, 2, 3, 1)
                mean_abs = F.avg_pool2d(nchw.abs(), 3, 1, 1, count_include_pad=False).permute(0, 2, 3, 1)
                bound = 2 * u * want.abs() * (1 + 2 * u) + 2.0 ** -50 * mean_abs
                if yd == torch.bfloat16:
                    bound = bound + 2.0 ** -8 * want.abs()
                err = (got.double() - want).abs()
                assert bool((err <= bound).all()), (H, W, C, xd, yd, float((err / bound).max()))
            # the divisors on their own: an image of ones averages to exactly 1 only where the divisor is the in-bounds count
            got, _ = pool_run(2, torch.ones(2, H, W, C), torch.float32, torch.float32)
            corners = got[:, [0, 0, -1, -1], [0, -1, 0, -1]]
            edges = torch.cat([got[:, 0, 1:-1].reshape(-1), got[:, -1, 1:-1].reshape(-1), got[:, 1:-1, 0].reshape(-1), got[:, 1:-1, -1].reshape(-1)])
            inner = got[:, 1:-1, 1:-1]
            assert bool((corners == 1.0).all()), "corner windows divide by 4"
            assert bool((edges == 1.0).all()), "edge windows divide by 6"
            assert bool((inner == 1.0).all()), "interior windows divide by 9"


@gpu
def test_global_average_fixed_order():
    g = torch.Generator().manual_seed(43)
    for HW, C, ld in ((35, 8, 12), (64, 36, 36), (1, 2048, 2048)):
        x = torch.randn(3, HW, C, generator=g)
        xin = Carved(3 * HW * ld, torch.float32, rows_with_dead_columns(x, ld))
        outs = []
        for _ in range(2):
            out = Carved(3 * C, torch.float32)
            assert L().sfron_global_avgpool(xin.ptr(), 0, ld, 3, HW, C, out.ptr(), S()) == OK
            torch.cuda.synchronize()
            out.check()
            outs.append(out.t.cpu().view(3, C))
        assert torch.equal(bits(outs[0]), bits(outs[1]))
        s = torch.zeros(3, C)
        for k in range(HW):                       # the stated order: rows ascending, fp32
            s = s + x[:, k]
        assert torch.equal(bits(outs[0]), bits(s / float(HW)))


# ------------------------------------------------------------------------------------------------ resize
def _resize_bound(want, H, W):
    """|got - want| for the kernel's fp32 evaluation of  top = tl + (tr - tl) fx;  bot alike;  v = top + (bot - top) fy;  y = (v - 128) / 128
    followed by one bf16 rounding, against the same expression in float64 (u = 2^-24, bytes <= 255):
      coordinates   src = dst * (in / out): the quotient and the product round once each, |d src| <= 2 u src <= 2 u in; lo = floor(src) and
                    frac = src - lo are then exact.  The interpolant is continuous and piecewise linear with slope <= 255 per source pixel
                    along either axis -- also across a floor that falls on the other side of an integer -- so the two coordinate errors move
                    v by at most 255 * 2 u (H + W).
      arithmetic    tr - tl is exact; the product and the sum of each lerp round once (<= 255 u each): top and bot carry 2 * 255 u; bot -
                    top inherits 4 * 255 u and rounds (255 u), times fy rounds (255 u), plus top inherits 2 * 255 u and rounds (255 u):
                    <= 12 * 255 u in all (loosely counted).  v - 128 rounds once (<= 128 u); / 128 is exact.
      bf16          round to nearest even with 8 significant bits: unit roundoff 2^-8 relative to the fp32 value.
    e32 = (255 u (12 + 2 (H + W)) + 128 u) / 128;  bound = e32 + 2^-8 (|want| + e32)."""
    u = 2.0 ** -24
    e32 = (255 * u * (12 + 2 * (H + W)) + 128 * u) / 128
    return e32 + 2.0 ** -8 * (want.abs() + e32)


@gpu
@pytest.mark.parametrize("shape", [(32, 32), (40, 56), (320, 300)])
def test_resize_tf1(shape):
    H, W = shape
    g = torch.Generator().manual_seed(H + W)
    img = torch.randint(0, 256, (2, H, W, 3), generator=g, dtype=torch.uint8)
    want = (ref.resize_tf1(img.permute(0, 3, 1, 2), dtype=torch.float64) - 128.0) / 128.0          # [B][3][299][299]
    xin = Carved(img.numel(), torch.uint8, img)
    out = Carved(2 * 299 * 299 * 8, torch.bfloat16)
    assert L().sfron_resize_tf1_u8(xin.ptr(), 2, H, W, 299, 299, 8, out.ptr(), S()) == OK
    torch.cuda.synchronize()
    out.check()
    got = out.t.cpu().view(2, 299, 299, 8)
    assert bool((bits(got[..., 3:]) == 0).all()), "the padded channels are +0"
    err = (got[..., :3].double().permute(0, 3, 1, 2) - want).abs()
    bound = _resize_bound(want, H, W)
    print(f"resize {H}x{W}: worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    # teeth: the half-pixel rule is far outside the bound
    half = (F.interpolate(img.permute(0, 3, 1, 2).double(), size=(299, 299), mode="bilinear", align_corners=False) - 128.0) / 128.0
    assert float(((half - want).abs() > bound).double().mean()) > 0.5


# ------------------------------------------------------------------------------------------------ statistics
def _cov_bound(xl, N):
    """First-order bound of the kernel's sigma against np.cov in extended precision, u = 2^-53.  With a_n = x[n][i] - mu[i], b_n alike:
      mean      N - 1 additions in any order and one division: |d mu_i| <= (N + 1) u mean_n |x[n][i]|
      centring  a_n is one subtraction of the rounded mean: |d a_n| <= u |a_n| + |d mu_i|
      products  a_n b_n summed by fma in any order, N terms: <= (N + 1) u sum |a_n b_n|, plus the centring errors carried through the sum:
                2 u sum |a_n b_n| + |d mu_i| sum |b_n| + |d mu_j| sum |a_n|
      scaling   1 / (N - 1) rounds once and the product with it once: 2 u |sigma_ij|
    |d sigma_ij| <= ((N + 3) u sum |a_n b_n| + |d mu_i| sum |b_n| + |d mu_j| sum |a_n|) / (N - 1) + 2 u |sigma_ij|.
    Returns (bound on mu, bound on sigma)."""
    u = np.longdouble(2.0) ** -53
    mu = xl.mean(axis=0)
    A = np.abs(xl - mu)
    dmu = (N + 1) * u * np.abs(xl).mean(axis=0)
    S1 = A.sum(axis=0)
    sig = (xl - mu).T @ (xl - mu) / (N - 1)
    return dmu, ((N + 3) * u * (A.T @ A) + np.outer(dmu, S1) + np.outer(S1, dmu)) / (N - 1) + 2 * u * np.abs(sig)


def run_stats(x, ld=None):
    N, D = x.shape
    ld = ld or D + 4
    xin = Carved(N * ld, torch.float32, rows_with_dead_columns(torch.as_tensor(x), ld))
    mu, sigma = Carved(D, torch.float64), Carved(D * D, torch.float64)
    assert L().sfron_feature_stats(xin.ptr(), N, D, ld, mu.ptr(), sigma.ptr(), S()) == OK
    torch.cuda.synchronize()
    mu.check()
    sigma.check()
    return mu.t.cpu().numpy().copy(), sigma.t.cpu().numpy().reshape(D, D).copy()


@gpu
@pytest.mark.parametrize("N", [5, 37, 300])
@pytest.mark.parametrize("D", [4, 64, 192])
def test_feature_stats(N, D):
    rng = np.random.default_rng(N * 1000 + D)
    for name, x in (("randn", rng.standard_normal((N, D)) * rng.uniform(0.5, 2.0, D)), ("offset", 12.0 + 0.05 * rng.standard_normal((N, D)))):
        x = x.astype(np.float32)
        mu, sigma = run_stats(x)
        xl = x.astype(np.longdouble)
        want_mu = xl.mean(axis=0)
        want = (xl - want_mu).T @ (xl - want_mu) / (N - 1)
        bmu, bsig = _cov_bound(xl, N)
        assert np.all(np.abs(mu - want_mu) <= bmu), name
        ratio = float((np.abs(sigma - want) / bsig).max())
        print(f"stats N={N} D={D} {name}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0, name
        assert np.array_equal(sigma, sigma.T)
        mu2, sigma2 = run_stats(x)
        assert np.array_equal(mu.view(np.int64), mu2.view(np.int64)) and np.array_equal(sigma.view(np.int64), sigma2.view(np.int64))
    # small integers with integer column means: every step is exact, np.cov's bits
    xi = rng.integers(-3, 4, (N, D))
    xi[-1] = -xi[:-1].sum(axis=0)                       # column sums 0 ...
    xi = (xi + rng.integers(-2, 3, D)).astype(np.float32)      # ... then an integer mean per column
    mu, sigma = run_stats(xi)
    assert np.array_equal(mu, np.mean(xi.astype(np.float64), axis=0))
    assert np.array_equal(sigma, np.cov(xi.astype(np.float64), rowvar=False).reshape(D, D))


@gpu
def test_refusals():
    """SFRON_ERR_ARG before any launch: the outputs keep their pattern"""
    lib = L()
    x = Carved(4096, torch.float32)
    y = Carved(4096, torch.float32)
    p, q, s = x.ptr(), y.ptr(), S()
    calls = [
        lib.sfron_patch_rows(None, 8, 1, 4, 4, 8, 3, 3, 1, 1, 1, q, s), lib.sfron_patch_rows(p, 8, 1, 4, 4, 8, 3, 3, 1, 1, 1, None, s),
        lib.sfron_patch_rows(p, 8, 0, 4, 4, 8, 3, 3, 1, 1, 1, q, s), lib.sfron_patch_rows(p, 8, 1, 4, 4, 12, 3, 3, 1, 1, 1, q, s),
        lib.sfron_patch_rows(p, 8, 1, 4, 4, 8, 0, 3, 1, 1, 1, q, s), lib.sfron_patch_rows(p, 8, 1, 4, 4, 8, 3, 3, 3, 1, 1, q, s),
        lib.sfron_patch_rows(p, 8, 1, 2, 2, 8, 3, 3, 1, 0, 0, q, s), lib.sfron_patch_rows(p, 8, 1, 16384, 16384, 8, 1, 1, 1, 0, 0, q, s),
        lib.sfron_resize_tf1_u8(None, 1, 4, 4, 8, 8, 8, q, s), lib.sfron_resize_tf1_u8(p, 1, 4, 4, 8, 8, 8, None, s),
        lib.sfron_resize_tf1_u8(p, 1, 0, 4, 8, 8, 8, q, s), lib.sfron_resize_tf1_u8(p, 1, 4, 4, 8, 8, 4, q, s),
        lib.sfron_resize_tf1_u8(p, 1, 4, 4, 16384, 16384, 8, q, s),
        lib.sfron_pool3(None, 0, 8, 1, 4, 4, 8, 0, q, 0, 8, s), lib.sfron_pool3(p, 0, 8, 1, 4, 4, 8, 0, None, 0, 8, s),
        lib.sfron_pool3(p, 0, 8, 1, 4, 4, 8, 3, q, 0, 8, s), lib.sfron_pool3(p, 0, 8, 1, 4, 4, 6, 1, q, 0, 8, s),
        lib.sfron_pool3(p, 0, 8, 1, 2, 4, 8, 0, q, 0, 8, s), lib.sfron_pool3(p, 0, 8, 1, 4, 4, 8, 1, q, 0, 4, s),
        lib.sfron_pool3(p, 0, 8, 1, 16384, 16384, 8, 1, q, 0, 8, s),
        lib.sfron_global_avgpool(None, 0, 8, 1, 4, 8, q, s), lib.sfron_global_avgpool(p, 0, 8, 1, 4, 8, None, s),
        lib.sfron_global_avgpool(p, 0, 8, 1, 0, 8, q, s), lib.sfron_global_avgpool(p, 0, 4, 1, 4, 8, q, s),
        lib.sfron_global_avgpool(p, 0, 2048, 1 << 10, 1 << 9, 2048, q, s),
        lib.sfron_feature_stats(None, 8, 8, 8, q, q + 1024, s), lib.sfron_feature_stats(p, 8, 8, 8, None, q + 1024, s),
        lib.sfron_feature_stats(p, 8, 8, 8, q, None, s), lib.sfron_feature_stats(p, 1, 8, 8, q, q + 1024, s),
        lib.sfron_feature_stats(p, 8, 6, 8, q, q + 1024, s), lib.sfron_feature_stats(p, 8, 2052, 2052, q, q + 1024, s),
        lib.sfron_feature_stats(p, 8, 8, 4, q, q + 1024, s), lib.sfron_feature_stats(p, 1 << 29, 4, 4, q, q + 1024, s),
    ]
    torch.cuda.synchronize()
    assert calls == [ERR_ARG] * len(calls), calls
    y.check()
    y.untouched(torch.ones(4096, dtype=torch.bool))


# ------------------------------------------------------------------------------------------------ the network
def images():
    g = torch.Generator().manual_seed(3)
    return (torch.randint(0, 256, (2, 32, 32, 3), generator=g, dtype=torch.uint8),
            torch.randint(0, 256, (3, 40, 56, 3), generator=g, dtype=torch.uint8))


@pytest.fixture(scope="module")
def nets():
    from sfron import inception
    m = ref.randomize(ref.FIDInceptionV3(), 11, probe=images()[0])
    emu = ref.Emulated(m)
    with torch.no_grad():
        f32 = [m(x) for x in images()]
        e = [emu(x) for x in images()]
    net = inception.InceptionV3(device=DEV).load_state_dict(m.state_dict())
    return m, net, {t: torch.cat([f[t] for f in f32]) for t in ref.TAPS}, {t: torch.cat([f[t] for f in e]) for t in ref.TAPS}


@gpu
def test_network_within_twice_the_emulation_error(nets):
    """Measured on an MI355X (seed 11, 2 images of 32 x 32 and 3 of 40 x 56), e_emul / GPU vs fp32 / GPU vs emulation:
    tap 64 1.236e-3 / 1.236e-3 / 1.2e-6, tap 192 1.577e-3 / 1.577e-3 / 2.6e-6, tap 768 3.881e-3 / 3.854e-3 / 6.0e-4, tap 2048 4.147e-3 /
    4.151e-3 / 1.6e-3."""
    m, net, f32, emul = nets
    got = [net.forward_u8(x.to(DEV)) for x in images()]
    got = {t: torch.cat([g[t] for g in got]).cpu() for t in ref.TAPS}
    worst = []
    for t in ref.TAPS:
        e_emul, e_gpu, e_ge = ref.rel_l2(emul[t], f32[t]), ref.rel_l2(got[t], f32[t]), ref.rel_l2(got[t], emul[t])
        print(f"tap {t}: e_emul {e_emul:.3e}  GPU vs fp32 {e_gpu:.3e}  GPU vs emulation {e_ge:.3e}")
        assert bool(torch.isfinite(got[t]).all())
        worst.append((t, e_gpu, 2 * e_emul))
    for t, e_gpu, lim in worst:
        assert e_gpu <= lim, (t, e_gpu, lim)


@gpu
def test_chunked_run_is_bit_equal(nets):
    m, net, f32, emul = nets
    x = images()[1].to(DEV)
    whole = net.forward_u8(x)
    keep = net.max_chunk_bytes
    try:
        net.max_chunk_bytes = 2 * net.per_sample_bytes(40, 56)          # 3 images: a chunk of 2 and a short last chunk of 1
        assert net.chunk_size(40, 56) == 2
        parts = net.forward_u8(x)
    finally:
        net.max_chunk_bytes = keep
    for t in ref.TAPS:
        assert torch.equal(bits(whole[t].cpu()), bits(parts[t].cpu())), t
    again = net.forward_u8(x)
    for t in ref.TAPS:
        assert torch.equal(bits(whole[t].cpu()), bits(again[t].cpu())), t


@gpu
def test_taps_on_request_and_state_dict_forms(nets):
    from sfron import inception
    m, net, f32, emul = nets
    x = images()[0].to(DEV)
    full = net.forward_u8(x)
    for t in ref.TAPS:
        only = net.forward_u8(x, taps=(t,))
        assert list(only) == [t] and torch.equal(bits(only[t].cpu()), bits(full[t].cpu()))
    with pytest.raises(ValueError):
        net.forward_u8(x, taps=(100,))
    with pytest.raises(ValueError):
        net.forward_u8(x.float())
    sd = m.state_dict()
    no_fc = {k: v for k, v in sd.items() if not k.startswith("fc.") and not k.endswith("num_batches_tracked")}
    other = inception.InceptionV3(device=DEV).load_state_dict(no_fc)
    assert torch.equal(bits(other.forward_u8(x, taps=(64,))[64].cpu()), bits(full[64].cpu()))
    with pytest.raises(KeyError):
        inception.InceptionV3(device=DEV).load_state_dict({**sd, "AuxLogits.fc.weight": torch.zeros(1)})
    with pytest.raises(KeyError):
        inception.InceptionV3(device=DEV).load_state_dict({k: v for k, v in sd.items() if k != "Mixed_7c.branch_pool.conv.weight"})
