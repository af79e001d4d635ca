"""GPU: the DiT loss, sampling-step, layout and step-guard kernels (csrc/loss.hip, the non-conditioning half of csrc/embed.hip) at every form,
through the C ABI, against the restatements of tests/dit_loss_ref.py (the yardstick is the float32 CPU evaluation of the same expression,
never the kernel).  Every output lives in a guarded() buffer whose sentinels are checked after every call; a refused call leaves the
sentinel-filled outputs untouched.  Distances are printed (DIT-LOSS-METRIC lines: the share of the allowance a result uses) before they are
asserted, and RECORD is printed at teardown (pytest -s).

  a. sfron_dit_loss_fwd_bwd   (C, hw) = (4,5) three idle waves, (4,63) one short of a workgroup, (3,341), (4,1024) the model's, (4,4099) odd;
                              nine stratified rows (dit_loss_ref.loss_inputs) and a single t == 0 row; grad_scale +1/n and -0.001/n;
                              dit_loss_ref.accept_loss: d_out per sample and per channel half, mse / vb relative per class, saturated
                              var-gradients exactly 0.0.  At t = 998 / 999 the var half's bound only says "finite and tiny" (the yardstick's own
                              error is a tenth to a quarter of the value: max_log - min_log cancels in fp32).
  b. bit for bit              sfron_q_sample, sfron_cfg_combine, sfron_ddpm_loss_bwd, sfron_ddpm_q_sample against separate fp32 torch ops in the
                              kernel's order (the library is built with -ffp-contract=off); 5, 252, 4096, 16396 elements per sample
  c. sfron_p_sample           bound32 per sample; clip 0 / 1 with the clipped share asserted; pred_xstart NULL / given; a t == 0 row ignores the noise
  d. layout                   sfron_patchify / sfron_unpatchify bit for bit at dit_loss_ref.LAYOUT_SHAPES (the last strides the 2048-workgroup
                              grid), both column orders, ld = K and K + 8
  e. DDPM loss                sfron_ddpm_sample_loss, sfron_ddpm_loss_coef (both modes, n = 1, 8, 300, a zero loss, the use_wsum = 1 form on a
                              batch of 300 split 120 + 180)
  f. step guard               sfron_guard_inputs / sfron_guard_finite at n = 1, 5, 256, 257, 1000; guard.StepGuard; one step.DiTSFRon per violation

Timesteps handed to sfron_q_sample, sfron_dit_loss_fwd_bwd, sfron_p_sample and sfron_ddpm_q_sample are always inside [0, T): they index the
schedule table unchecked, by design.  Out-of-range indices go only to sfron_guard_inputs, StepGuard.check_inputs and a runner step, which
clamps them first.

Largest share of an allowance seen on an MI355X (1.0 = the bound; the float32 restatement itself sits at 1 / MARGIN = 0.25 where the 4-ulp term
is negligible):
  dit_loss    d_eps 0.32   d_var 0.29 (t = 998 / 999: 1.4e-4)   mse 0.11   vb 0.39        p_sample   sample 0.16   pred_xstart 0.25
  ddpm        sample_loss 0.14   coef 0.22   loss 0.21   wsum 0.26
The var-gradient lands on the yardstick's own distance (ratio 0.95 .. 1.19): its error is the cancellation in x0 - model_mean, which the kernel and
the float32 restatement form from the same fp32 operations; the device tanhf / logf / expf add nothing that shows."""
import functools

import pytest
import torch

import dit_loss_ref as L
import dit_rows_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = 1001          # csrc/common.h
F64, F32, BF16, I64 = torch.float64, torch.float32, torch.bfloat16, torch.int64
T_STEPS = 1000


def _L():
    from sfron import _lib
    return _lib.lib()


def _sp():
    from sfron._lib import stream_ptr
    return stream_ptr()


_LIVE = []


def dev(t):
    """a device copy that stays allocated until the test ends: dev(x).data_ptr() in an argument list must not hand the copy's memory back to
    the caching allocator, where the next copy of the same list would take it"""
    d = t.contiguous().to(DEV)
    _LIVE.append(d)
    return d


def sync():
    torch.cuda.synchronize()


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
    """a launch that faulted leaves the device context unusable: end the session there instead of launching the remaining cases on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault in tests/test_gpu_dit_loss.py: {e}", returncode=3)
    del _LIVE[:]


@pytest.fixture(scope="module", autouse=True)
def _print_record():
    yield
    print()
    for name in sorted(R.RECORD):
        print("RECORD", name, " ".join(f"{k}={v:.4g}" for k, v in sorted(R.RECORD[name].items())))


@functools.lru_cache(maxsize=None)
def tab_cpu():
    return L.table()


@functools.lru_cache(maxsize=None)
def tab_dev():
    return dev(tab_cpu())


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ================================================================================================ a. the fused loss
@functools.lru_cache(maxsize=None)
def loss_ref(C, hw, rows0, n_extra, gs_kind):
    i = L.loss_inputs(n_extra, C, hw, rows0=rows0)
    n = rows0 + n_extra
    gs = 1.0 / n if gs_kind == "plus" else -0.001 / n
    return i, gs, L.loss_case(i, gs, tab_cpu(), F64), L.loss_case(i, gs, tab_cpu(), F32)


def launch_loss(i, gs, n=None, x0_ptr=True):
    n = i["t"].shape[0] if n is None else n
    C, hw = i["C"], i["hw"]
    x0, noise, out, t = dev(i["x0"]), dev(i["noise"]), dev(i["out"]), dev(i["t"])
    assert int(t.min()) >= 0 and int(t.max()) < T_STEPS
    mse, c_mse = R.guarded((max(n, 1),), F32)
    vb, c_vb = R.guarded((max(n, 1),), F32)
    d_out, c_d = R.guarded((max(n, 1), 2 * C * hw), F32)
    st = _L().sfron_dit_loss_fwd_bwd(x0.data_ptr() if x0_ptr else None, noise.data_ptr(), out.data_ptr(), t.data_ptr(), tab_dev().data_ptr(), n, C, hw,
                                     gs, mse.data_ptr(), vb.data_ptr(), d_out.data_ptr(), _sp())
    sync()
    return st, dict(mse=mse, vb=vb, d_out=d_out.view(max(n, 1), 2 * C, hw)), (c_mse, c_vb, c_d)


@pytest.mark.parametrize("gs_kind", ["plus", "forget"])
@pytest.mark.parametrize("C,hw", L.LOSS_SHAPES)
def test_dit_loss_fwd_bwd_on_stratified_rows(C, hw, gs_kind):
    i, gs, c64, c32 = loss_ref(C, hw, 3, 6, gs_kind)
    st, got, checks = launch_loss(i, gs)
    assert st == 0, st
    for c in checks:
        c("dit_loss_fwd_bwd")
    L.accept_loss(got, c64, c32, name=f"dit_loss[{C}x{hw},{gs_kind}]")
    # the three branches of the t == 0 rows produced gradients of their own: not all equal, not all zero
    v = got["d_out"][:3, C:].cpu()
    assert int((v != 0).sum()) >= 0.9 * int((c64["d_out"][:3, C:] != 0).sum()) > 0


@pytest.mark.parametrize("C,hw", L.LOSS_SHAPES)
def test_dit_loss_fwd_bwd_single_t0_row(C, hw):
    i, gs, c64, c32 = loss_ref(C, hw, 1, 0, "plus")
    assert i["t"].tolist() == [0]
    st, got, checks = launch_loss(i, gs)
    assert st == 0, st
    for c in checks:
        c("dit_loss_fwd_bwd n = 1")
    L.accept_loss(got, c64, c32, name=f"dit_loss1[{C}x{hw}]")


def test_dit_loss_refusals_write_nothing():
    i, gs, _, _ = loss_ref(4, 5, 3, 6, "plus")
    for kw in (dict(n=0), dict(x0_ptr=False)):
        st, _, checks = launch_loss(i, gs, **kw)
        assert st == ERR_ARG, (kw, st)
        for c in checks:
            R.untouched(c, f"dit_loss_fwd_bwd {kw}")
    for bad in ((0, 5), (4, 0)):
        j = dict(i, C=bad[0], hw=bad[1])
        n = 9
        mse, c_mse = R.guarded((n,), F32)
        st = _L().sfron_dit_loss_fwd_bwd(dev(i["x0"]).data_ptr(), dev(i["noise"]).data_ptr(), dev(i["out"]).data_ptr(), dev(i["t"]).data_ptr(),
                                         tab_dev().data_ptr(), n, j["C"], j["hw"], gs, mse.data_ptr(), mse.data_ptr(), mse.data_ptr(), _sp())
        sync()
        assert st == ERR_ARG, (bad, st)
        R.untouched(c_mse, f"dit_loss_fwd_bwd C, hw = {bad}")


# ================================================================================================ b. bit for bit
SIZES = [5, 252, 4096, 16396]            # per sample; 16396 passes the 64 x 256-thread grid row twice
T_ROWS = torch.tensor([0, 500, 999], dtype=I64)


def elementwise_inputs(chw, seed):
    g = gen(seed * 7919 + chw)
    return torch.rand(3, chw, generator=g) * 2 - 1, torch.randn(3, chw, generator=g), torch.randn(3, chw, generator=g) * 0.7


@pytest.mark.parametrize("chw", SIZES)
def test_q_sample_bit_exact(chw):
    x0, noise, _ = elementwise_inputs(chw, 1)
    want = L.q_sample(x0, noise, T_ROWS, tab_cpu(), F32)                    # a * x0 + b * noise: two products, one sum, each rounded
    xt, check = R.guarded((3, chw), F32)
    st = _L().sfron_q_sample(dev(x0).data_ptr(), dev(noise).data_ptr(), dev(T_ROWS).data_ptr(), tab_dev().data_ptr(), 3, chw, xt.data_ptr(), _sp())
    sync()
    assert st == 0, st
    check("q_sample")
    assert bits_equal(xt, want)
    R.bound32(xt, L.q_sample(x0, noise, T_ROWS, tab_cpu(), F64), want, "q_sample")
    xt2, check2 = R.guarded((3, chw), F32)
    st = _L().sfron_q_sample(dev(x0).data_ptr(), dev(noise).data_ptr(), dev(T_ROWS).data_ptr(), tab_dev().data_ptr(), 3, 0, xt2.data_ptr(), _sp())
    sync()
    assert st == ERR_ARG
    R.untouched(check2, "q_sample chw = 0")


@pytest.mark.parametrize("chw", SIZES)
def test_ddpm_q_sample_and_loss_bwd_bit_exact(chw):
    from oracle import sfron_ref
    x0, e, out = elementwise_inputs(chw, 2)
    abar = sfron_ref.ddpm_alphas_cumprod_fp32(sfron_ref.ddpm_get_betas())
    a = abar[T_ROWS].view(-1, 1)
    # the correctly rounded fp32 square roots (tests/test_gpu_ddpm_loss.py): torch's vectorised CPU sqrt is 1 ulp off for some entries
    want = x0 * a.double().sqrt().float() + e * (1.0 - a).double().sqrt().float()
    xt, check = R.guarded((3, chw), F32)
    st = _L().sfron_ddpm_q_sample(dev(x0).data_ptr(), dev(e).data_ptr(), dev(T_ROWS).data_ptr(), dev(abar).data_ptr(), 3, chw, xt.data_ptr(), _sp())
    sync()
    assert st == 0, st
    check("ddpm_q_sample")
    assert bits_equal(xt, want)
    R.bound32(xt, L.ddpm_q_sample(x0, e, T_ROWS, abar, F64), want, "ddpm_q_sample")
    coef = torch.tensor([0.25, -3.0e-3, 7.1], dtype=F32)
    want = L.ddpm_loss_bwd(e, out, coef, F32)                                # c * (out - e)
    d, check = R.guarded((3, chw), F32)
    st = _L().sfron_ddpm_loss_bwd(dev(e).data_ptr(), dev(out).data_ptr(), dev(coef).data_ptr(), 3, chw, d.data_ptr(), _sp())
    sync()
    assert st == 0, st
    check("ddpm_loss_bwd")
    assert bits_equal(d, want)
    d2, check2 = R.guarded((3, chw), F32)
    st = _L().sfron_ddpm_loss_bwd(dev(e).data_ptr(), dev(out).data_ptr(), None, 3, chw, d2.data_ptr(), _sp())
    sync()
    assert st == ERR_ARG
    R.untouched(check2, "ddpm_loss_bwd without coef")


@pytest.mark.parametrize("hw", [5, 63, 4099])
@pytest.mark.parametrize("cout,n_guided", [(8, 8), (8, 3), (8, 1), (6, 2)])
@pytest.mark.parametrize("n_total", [2, 6])
def test_cfg_combine_bit_exact_in_place(n_total, cout, n_guided, hw):
    g = gen(n_total * 1000 + cout * 100 + n_guided * 10 + hw)
    src = torch.randn(n_total, cout, hw, generator=g)
    for s in (1.5, 4.3):
        want = L.cfg_combine(src, n_guided, s, F32)                          # u + s * (c - u)
        buf, check = R.guarded((n_total, cout * hw), F32)
        buf.copy_(dev(src.view(n_total, -1)))
        st = _L().sfron_cfg_combine(buf.data_ptr(), n_total, cout, hw, n_guided, s, _sp())
        sync()
        assert st == 0, st
        check("cfg_combine")
        got = buf.view(n_total, cout, hw).cpu()
        assert bits_equal(got, want)
        assert bits_equal(got[:, n_guided:], src[:, n_guided:])              # untouched channels of both halves
        assert bits_equal(got[:n_total // 2, :n_guided], got[n_total // 2:, :n_guided])
        assert not torch.equal(got[:, :n_guided], src[:, :n_guided])


def test_cfg_combine_refusals_leave_the_buffer_unchanged():
    src = torch.randn(6, 8, 5, generator=gen(3))
    for n_total, cout, n_guided in ((5, 8, 3), (3, 8, 3), (6, 8, 0), (6, 8, 9), (0, 8, 3)):
        buf, check = R.guarded((6, 40), F32)
        buf.copy_(dev(src.view(6, -1)))
        st = _L().sfron_cfg_combine(buf.data_ptr(), n_total, cout, 5, n_guided, 1.5, _sp())
        sync()
        assert st == ERR_ARG, (n_total, cout, n_guided, st)
        check("cfg_combine refused")
        assert bits_equal(buf.view(6, 8, 5), src)


# ================================================================================================ c. p_sample
@pytest.mark.parametrize("with_pred", [False, True])
@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("n,C,hw,ts", [(3, 4, 64, (0, 500, 999)), (1, 4, 5, (0,)), (2, 4, 4099, (37, 0))])
def test_p_sample_against_float64(n, C, hw, ts, clip, with_pred):
    g = gen(n * 100003 + hw)
    t = torch.tensor(ts, dtype=I64)
    x = torch.randn(n, C, hw, generator=g)
    out = torch.cat([torch.randn(n, C, hw, generator=g), torch.rand(n, C, hw, generator=g) * 3 - 1.5], 1)
    noise = torch.randn(n, C, hw, generator=g)
    s64, p64 = L.p_sample(x, out, t, tab_cpu(), noise, clip, F64)
    s32, p32 = L.p_sample(x, out, t, tab_cpu(), noise, clip, F32)
    _, raw = L.p_sample(x, out, t, tab_cpu(), noise, 0, F64)
    share = float((raw.abs() > 1).double().mean())
    assert share > 0.2, share                                                # the clip matters on a fifth of the elements or more
    if clip:
        assert float(p64.abs().max()) == 1.0

    def run(nz):
        sample, c_s = R.guarded((n, C * hw), F32)
        pred, c_p = R.guarded((n, C * hw), F32)
        st = _L().sfron_p_sample(dev(x).data_ptr(), dev(out).data_ptr(), dev(t).data_ptr(), tab_dev().data_ptr(), dev(nz).data_ptr(), n, C, hw, clip,
                                 sample.data_ptr(), pred.data_ptr() if with_pred else None, _sp())
        sync()
        assert st == 0, st
        c_s("p_sample")
        c_p("p_sample pred")
        if not with_pred:
            R.untouched(c_p, "p_sample with pred_xstart = NULL")
        return sample.view(n, C, hw), pred.view(n, C, hw)
    sample, pred = run(noise)
    tag = f"p_sample[clip{clip}]"
    for k in range(n):
        L.checked32(sample[k], s64[k], s32[k], f"{tag}.sample.t{ts[k]}")
        if with_pred:
            L.checked32(pred[k], p64[k], p32[k], f"{tag}.pred.t{ts[k]}")
    if with_pred and clip:
        assert float(pred.abs().max()) == 1.0
    # a t == 0 row's sample is the mean: bit-identical whatever finite noise it is given
    sample2, _ = run(noise * -3.0 + 0.5)
    k0 = ts.index(0)
    assert bits_equal(sample[k0], sample2[k0])
    for k in range(n):
        if k != k0:
            assert not torch.equal(sample[k], sample2[k])


def test_p_sample_refusals_write_nothing():
    x = torch.randn(2, 4, 5, generator=gen(1))
    out, t = torch.randn(2, 8, 5, generator=gen(2)), torch.tensor([0, 3], dtype=I64)
    for n, C, hw, with_noise in ((0, 4, 5, True), (2, 0, 5, True), (2, 4, 0, True), (2, 4, 5, False)):
        sample, c_s = R.guarded((2, 20), F32)
        pred, c_p = R.guarded((2, 20), F32)
        st = _L().sfron_p_sample(dev(x).data_ptr(), dev(out).data_ptr(), dev(t).data_ptr(), tab_dev().data_ptr(), dev(x).data_ptr() if with_noise else None,
                                 n, C, hw, 1, sample.data_ptr(), pred.data_ptr(), _sp())
        sync()
        assert st == ERR_ARG, (n, C, hw, with_noise, st)
        R.untouched(c_s, "p_sample refused")
        R.untouched(c_p, "p_sample refused")


# ================================================================================================ d. layout
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("chan_last", [0, 1])
@pytest.mark.parametrize("n,C,H,W,p", L.LAYOUT_SHAPES)
def test_patchify_bit_exact(n, C, H, W, p, chan_last, pad):
    img = torch.randn(n, C, H, W, generator=gen(H * W + p + chan_last))
    K, T = C * p * p, (H // p) * (W // p)
    want = L.patchify(img, p, chan_last)
    rows, check = R.guarded((n * T, K), BF16, ld=K + pad)
    st = _L().sfron_patchify(dev(img).data_ptr(), n, C, H, W, p, chan_last, rows.data_ptr(), K + pad, _sp())
    sync()
    assert st == 0, st
    check("patchify")                                                        # the gap columns of ld = K + 8 included
    assert bits_equal(rows, want)


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("n,C,H,W,p", L.LAYOUT_SHAPES)
def test_unpatchify_bit_exact(n, C, H, W, p, pad):
    K, T = C * p * p, (H // p) * (W // p)
    wide = torch.randn(n * T, K + pad, generator=gen(H * W + p + 17))
    want = L.unpatchify(wide[:, :K], n, C, H, W, p)
    wide_d = dev(wide)                                                       # the input is a column slice of the wider buffer
    img, check = R.guarded((n, C * H * W), F32)
    st = _L().sfron_unpatchify(wide_d.data_ptr(), K + pad, n, C, H, W, p, img.data_ptr(), _sp())
    sync()
    assert st == 0, st
    check("unpatchify")
    assert bits_equal(img.view(n, C, H, W), want)
    # and back: the rows, rounded to bf16
    rows, check = R.guarded((n * T, K), BF16)
    st = _L().sfron_patchify(img.data_ptr(), n, C, H, W, p, 1, rows.data_ptr(), K, _sp())
    sync()
    assert st == 0, st
    check("patchify")
    assert bits_equal(rows, wide[:, :K].to(BF16))


def test_layout_refusals_write_nothing():
    img = dev(torch.randn(2, 4, 8, 8, generator=gen(5)))
    tok = dev(torch.randn(2 * 16, 16, generator=gen(6)))
    for H, W, p, ld in ((7, 8, 2, 16), (8, 7, 2, 16), (8, 8, 2, 15), (8, 8, 0, 16), (8, 8, 3, 36)):
        rows, c_rows = R.guarded((32, 16), BF16)
        out, c_out = R.guarded((2, 256), F32)
        st = _L().sfron_patchify(img.data_ptr(), 2, 4, H, W, p, 0, rows.data_ptr(), ld, _sp())
        st2 = _L().sfron_unpatchify(tok.data_ptr(), ld, 2, 4, H, W, p, out.data_ptr(), _sp())
        sync()
        assert st == ERR_ARG and st2 == ERR_ARG, (H, W, p, ld, st, st2)
        R.untouched(c_rows, "patchify refused")
        R.untouched(c_out, "unpatchify refused")


# ================================================================================================ e. DDPM loss
@pytest.mark.parametrize("n,chw", [(1, 1), (3, 255), (3, 257), (2, 3072), (2, 16384), (5, 252)])
def test_ddpm_sample_loss_against_float64_sums(n, chw):
    g = gen(n * 65537 + chw)
    e = torch.randn(n, chw, generator=g)
    out = e + torch.randn(n, chw, generator=g) * torch.logspace(-2, 0.5, n).view(-1, 1)
    per, check = R.guarded((n,), F32)
    st = _L().sfron_ddpm_sample_loss(dev(e).data_ptr(), dev(out).data_ptr(), n, chw, per.data_ptr(), _sp())
    sync()
    assert st == 0, st
    check("ddpm_sample_loss")
    w64, w32 = L.ddpm_sample_loss(e, out, F64), L.ddpm_sample_loss(e, out, F32)
    for k in range(n):                                                       # per sample: the losses span 1e-4 .. 10 per element
        L.checked32(per[k:k + 1], w64[k:k + 1], w32[k:k + 1], "ddpm_sample_loss")
    per2, check2 = R.guarded((n,), F32)
    st = _L().sfron_ddpm_sample_loss(dev(e).data_ptr(), dev(out).data_ptr(), n, 0, per2.data_ptr(), _sp())
    sync()
    assert st == ERR_ARG
    R.untouched(check2, "ddpm_sample_loss chw = 0")


def per_losses(n, zero=False):
    g = gen(n + (1000 if zero else 0))
    if n == 300:
        per = torch.logspace(-3, 3, n)[torch.randperm(n, generator=g)].float()        # 1e-3 .. 1e3
    else:
        per = (torch.rand(n, generator=g) * 3000 + 1).float()
    if zero:
        per[n // 3] = 0.0                                                    # weight 1 / 1e-8
    return per


def launch_coef(per, mode, lambd, scale, n_global, wsum_in=None, use_wsum=0):
    n = per.shape[0]
    coef, c_coef = R.guarded((n,), F32)
    loss, c_loss = R.guarded((1,), F32)
    wsum, c_wsum = R.guarded((1,), F32)
    if wsum_in is not None:
        wsum.copy_(dev(wsum_in.view(1)))
    before = wsum.clone()
    st = _L().sfron_ddpm_loss_coef(dev(per).data_ptr(), n, mode, lambd, scale, n_global, wsum.data_ptr(), use_wsum, coef.data_ptr(), loss.data_ptr(),
                                   _sp())
    sync()
    assert st == 0, st
    for c in (c_coef, c_loss, c_wsum):
        c("ddpm_loss_coef")
    if mode == 0 or use_wsum:
        assert bits_equal(wsum, before), "wsum was written"
    return coef, loss, wsum


@pytest.mark.parametrize("mult", [1, 4])
@pytest.mark.parametrize("n", [1, 8, 300])
def test_ddpm_loss_coef_simple(n, mult):
    per = per_losses(n)
    coef, loss, _ = launch_coef(per, 0, 0.0, 2.5, mult * n)
    c64, l64, _ = L.ddpm_loss_coef(per, 0, 0.0, 2.5, mult * n, F64)
    c32, l32, _ = L.ddpm_loss_coef(per, 0, 0.0, 2.5, mult * n, F32)
    L.checked32(coef, c64, c32, "ddpm_loss_coef.simple.coef")
    L.checked32(loss, l64.view(1), l32.view(1), "ddpm_loss_coef.simple.loss")


@pytest.mark.parametrize("lambd", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("n,zero", [(1, False), (8, False), (300, False), (8, True)])
def test_ddpm_loss_coef_adaptive(n, zero, lambd):
    per = per_losses(n, zero)
    coef, loss, wsum = launch_coef(per, 1, lambd, 1.0, n)
    c64, l64, w64 = L.ddpm_loss_coef(per, 1, lambd, 1.0, n, F64)
    c32, l32, w32 = L.ddpm_loss_coef(per, 1, lambd, 1.0, n, F32)
    tag = "ddpm_loss_coef.adaga" + (".zero" if zero else "")
    L.checked32(coef, c64, c32, tag + ".coef")
    L.checked32(loss, l64.view(1), l32.view(1), tag + ".loss")
    L.checked32(wsum, w64.view(1), w32.view(1), tag + ".wsum")
    if zero:
        assert float(w64) > 9e7                                               # the zero loss carries all the weight


@pytest.mark.parametrize("lambd", [0.5, 2.0])
def test_ddpm_loss_coef_with_the_summed_weights_of_a_split_batch(lambd):
    per = per_losses(300)
    parts = (per[:120], per[120:])
    sums = [launch_coef(p, 1, lambd, 1.0, 300)[2].cpu() for p in parts]
    total = sums[0] + sums[1]                                                # what the all-reduce forms: one fp32 sum of the two
    got = [launch_coef(p, 1, lambd, 1.0, 300, wsum_in=total, use_wsum=1) for p in parts]
    coef = torch.cat([g[0].cpu() for g in got])
    loss = got[0][1].cpu() + got[1][1].cpu()
    c64, l64, _ = L.ddpm_loss_coef(per, 1, lambd, 1.0, 300, F64)
    c32, l32, _ = L.ddpm_loss_coef(per, 1, lambd, 1.0, 300, F32)
    L.checked32(coef, c64, c32, "ddpm_loss_coef.split.coef")
    L.checked32(loss, l64.view(1), l32.view(1), "ddpm_loss_coef.split.loss")
    for g in got:
        assert bits_equal(g[2], total)                                       # bit-unchanged by the use_wsum = 1 call


def test_ddpm_loss_coef_refusals_write_nothing():
    per = dev(per_losses(8))
    for n, mode, n_global, with_wsum in ((0, 1, 8, True), (8, 2, 8, True), (8, 1, 7, True), (8, 1, 8, False)):
        coef, c_coef = R.guarded((8,), F32)
        loss, c_loss = R.guarded((1,), F32)
        wsum, c_wsum = R.guarded((1,), F32)
        st = _L().sfron_ddpm_loss_coef(per.data_ptr(), n, mode, 0.5, 1.0, n_global, wsum.data_ptr() if with_wsum else None, 0, coef.data_ptr(),
                                       loss.data_ptr(), _sp())
        sync()
        assert st == ERR_ARG, (n, mode, n_global, with_wsum, st)
        for c in (c_coef, c_loss, c_wsum):
            R.untouched(c, "ddpm_loss_coef refused")


# ================================================================================================ f. the step guard
GUARD_N = [1, 5, 256, 257, 1000]
NUM_CLASSES = 10
FLAGS0 = (3.0, 5.0, 7.0, 11.0)


def positions(n):
    """the first, the last, the 256th and the 257th position, where the vector has them"""
    return sorted({k for k in (0, n - 1, 255, 256) if k < n})


def flags_buffer():
    flags, check = R.guarded((4,), F32)
    flags.copy_(torch.tensor(FLAGS0, device=DEV))
    return flags, check


@pytest.mark.parametrize("n", GUARD_N)
def test_guard_inputs_clamps_and_counts(n):
    g = gen(n)
    y0 = torch.randint(0, NUM_CLASSES, (n,), generator=g)
    t0 = torch.randint(0, T_STEPS, (n,), generator=g)
    bad_y = (-1, NUM_CLASSES, 2 ** 40, -2 ** 40)          # the null-class index is no legal input label; a 32-bit read of +-2^40 sees 0
    bad_t = (-1, T_STEPS, 2 ** 40, -2 ** 40)
    flags, c_flags = flags_buffer()
    want = list(FLAGS0)

    def call(y, t):
        ys, c_y = R.guarded((n,), I64)
        ts, c_t = R.guarded((n,), I64)
        st = _L().sfron_guard_inputs(dev(y).data_ptr(), dev(t).data_ptr(), n, NUM_CLASSES, T_STEPS, ys.data_ptr(), ts.data_ptr(), flags.data_ptr(), _sp())
        sync()
        assert st == 0, st
        for c in (c_y, c_t, c_flags):
            c("guard_inputs")
        return ys.cpu(), ts.cpu()
    # clean inputs: outputs equal the inputs, all four flags bit-unchanged
    ys, ts = call(y0, t0)
    assert torch.equal(ys, y0) and torch.equal(ts, t0)
    assert bits_equal(flags, torch.tensor(want))
    pos = positions(n)
    for rot in range(6):                                    # every bad value visits every planted position
        y, t = y0.clone(), t0.clone()
        for j, k in enumerate(pos):
            if rot != 5:                                    # rot 4: only labels, rot 5: only one timestep -- the two counts differ
                y[k] = bad_y[(j + rot) % 4]
            if rot < 4 or (rot == 5 and k == pos[-1]):
                t[k] = bad_t[(j + rot + 1) % 4]
        wy, wt, by, bt = L.guard_inputs(y, t, NUM_CLASSES, T_STEPS)
        assert (by, bt) == ((len(pos), len(pos)) if rot < 4 else (len(pos), 0) if rot == 4 else (0, 1))
        ys, ts = call(y, t)
        assert torch.equal(ys, wy) and torch.equal(ts, wt)
        want[2] += by                                       # ... and a second call accumulates
        want[3] += bt
        assert bits_equal(flags, torch.tensor(want)), (flags.cpu().tolist(), want)
    # refused: nothing written
    ys, c_y = R.guarded((n,), I64)
    st = _L().sfron_guard_inputs(dev(y0).data_ptr(), dev(t0).data_ptr(), n, 0, T_STEPS, ys.data_ptr(), ys.data_ptr(), flags.data_ptr(), _sp())
    st2 = _L().sfron_guard_inputs(dev(y0).data_ptr(), dev(t0).data_ptr(), 0, NUM_CLASSES, T_STEPS, ys.data_ptr(), ys.data_ptr(), flags.data_ptr(), _sp())
    sync()
    assert st == ERR_ARG and st2 == ERR_ARG
    R.untouched(c_y, "guard_inputs refused")
    assert bits_equal(flags, torch.tensor(want))


FLT_MAX = 3.4028234663852886e38


@pytest.mark.parametrize("n", GUARD_N)
def test_guard_finite_counts_once_per_call(n):
    g = gen(n + 50)
    base = [torch.randn(n, generator=g) for _ in range(4)]
    base[0][0] = FLT_MAX                                    # the largest finite value and subnormals do not flag
    base[1][n - 1] = -FLT_MAX
    base[2][n // 2] = 1e-45
    base[3][0] = -1e-40
    flags, c_flags = flags_buffer()
    want = list(FLAGS0)

    def call(vecs, stats=None):
        p = [None if v is None else dev(v) for v in vecs]
        s = None if stats is None else dev(stats)
        st = _L().sfron_guard_finite(*[None if v is None else v.data_ptr() for v in p], n, None if s is None else s.data_ptr(), flags.data_ptr(), _sp())
        sync()
        assert st == 0, st
        c_flags("guard_finite")
        inc = L.guard_finite(vecs, stats)
        want[0] += inc[0]
        want[1] += inc[1]
        assert bits_equal(flags, torch.tensor(want)), (flags.cpu().tolist(), want)
        return inc
    assert call(base) == (0, 0)
    assert call(base, torch.tensor([1.5, float("nan"), float("inf"), 0.0])) == (0, 0)         # only stats[0] is the norm
    pos = sorted({k for k in (0, n - 1, 256) if k < n})
    for special in (float("nan"), float("inf"), -float("inf")):
        for which in range(4):
            for k in pos:
                vecs = [v.clone() for v in base]
                vecs[which][k] = special
                assert call(vecs) == (1, 0)
    # many at once: still one
    vecs = [v.clone() for v in base]
    for which in range(4):
        vecs[which][pos] = float("nan")
    assert call(vecs) == (1, 0)
    # vectors that are not passed do not count; a passed one behind a NULL does
    assert call([base[0], None, None, None]) == (0, 0)
    assert call([vecs[0], None, None, None]) == (1, 0)
    last = base[3].clone()
    last[n - 1] = float("inf")
    assert call([base[0], base[1], None, last]) == (1, 0)
    assert call([base[0], None, base[2], None]) == (0, 0)
    assert call([base[0], None, vecs[2], None]) == (1, 0)
    # the gradient norm
    assert call(base, torch.tensor([FLT_MAX])) == (0, 0)
    assert call(base, torch.tensor([float("nan")])) == (0, 1)
    assert call(base, torch.tensor([float("inf")])) == (0, 1)
    assert call(vecs, torch.tensor([-float("inf")])) == (1, 1)
    assert want[2:] == list(FLAGS0[2:])
    st = _L().sfron_guard_finite(None, None, None, None, n, None, flags.data_ptr(), _sp())
    st2 = _L().sfron_guard_finite(dev(base[0]).data_ptr(), None, None, None, 0, None, flags.data_ptr(), _sp())
    sync()
    assert st == ERR_ARG and st2 == ERR_ARG
    assert bits_equal(flags, torch.tensor(want))


def test_step_guard_raises_exactly_what_was_violated():
    from sfron import guard
    from sfron._lib import SfronError
    y = torch.tensor([1, 2, 3, 9], device=DEV)
    t = torch.tensor([0, 999, 5, 17], device=DEV)
    ok = torch.ones(4, device=DEV)
    nan = torch.tensor([1.0, float("nan"), 1.0, 1.0], device=DEV)

    def violate(g, k):
        if k == 0:
            g.check_finite((ok, nan))
        elif k == 1:
            g.check_finite((ok,), torch.tensor([float("inf"), 0.0], device=DEV))
        elif k == 2:
            ys, ts = g.check_inputs(torch.tensor([1, NUM_CLASSES, 3, -1], device=DEV), t, NUM_CLASSES, T_STEPS)
            assert ys.tolist() == [1, 9, 3, 0] and torch.equal(ts, t)
        else:
            ys, ts = g.check_inputs(y, torch.tensor([0, T_STEPS, 5, 17], device=DEV), NUM_CLASSES, T_STEPS)
            assert ts.tolist() == [0, 999, 5, 17] and torch.equal(ys, y)
    clean = guard.StepGuard(DEV)
    clean.poll()
    clean.poll(block=True)                                  # nothing published: returns
    for step_no in (1, 2):
        ys, ts = clean.check_inputs(y, t, NUM_CLASSES, T_STEPS)
        assert torch.equal(ys, y) and torch.equal(ts, t)
        clean.check_finite((ok, ok, ok, ok), torch.tensor([2.0, 1.0], device=DEV))
        clean.publish(step_no)
        clean.poll(block=True)
        clean.poll()
    assert clean.flags.tolist() == [0.0] * 4
    for ks in ((0,), (1,), (2,), (3,), (0, 3), (1, 2), (0, 1, 2, 3)):
        g = guard.StepGuard(DEV)
        for k in ks:
            violate(g, k)
        g.poll()                                            # violated, not yet published: returns
        g.poll(block=True)
        g.publish(41 + len(ks))
        with pytest.raises(SfronError) as e:
            g.poll(block=True)
        msg = str(e.value)
        assert f"by step {41 + len(ks)}" in msg, msg
        for k, reason in enumerate(guard.REASONS):
            assert (reason in msg) == (k in ks), (ks, msg)
        with pytest.raises(SfronError):                     # never reset
            g.poll(block=True)


RUNNER_CFG = dict(input_size=16, patch_size=2, in_channels=4, hidden_size=144, depth=3, num_heads=2, num_classes=10)       # "hd72" of test_gpu_dit.py


@pytest.mark.parametrize("case", ["clean", "label", "timestep", "nan"])
def test_runner_step_fails_loud(case):
    from oracle import dit_ref
    from sfron import data, diffusion, dit, guard, step
    from sfron._lib import SfronError
    B = 4
    torch.manual_seed(0)
    ref = dit_ref.DiT(**RUNNER_CFG)
    dit_ref.randomize_zero_init(ref, std=0.05, seed=1)
    model = dit.DiT(batch_size=B, **RUNNER_CFG)
    model.load_state_dict(ref.state_dict())
    model.train()
    runner = step.DiTSFRon(model, diffusion.create_diffusion(""), lr=1e-3, forget_alpha=0.5, grad_clip=1.0, ema_decay=0.99, mask=None, unlearn_loss="ga",
                           forget_class=3)
    kw = dict(global_batch=B, num_classes=RUNNER_CFG["num_classes"], forget_class=3, input_size=RUNNER_CFG["input_size"], device=DEV)
    f, r = data.synthetic_batch(5, 0, "forget", **kw), data.synthetic_batch(5, 0, "remain", **kw)
    if case == "label":
        f["y"][1] = RUNNER_CFG["num_classes"]
    elif case == "timestep":
        r["t"][2] = T_STEPS                                 # clamped by the runner's guard before any kernel indexes the table with it
    elif case == "nan":
        f["x0"][0, 1, 2, 3] = float("nan")
    out = runner.step(f, r)
    if case == "clean":
        runner.guard.poll(block=True)
        assert bool(torch.isfinite(out["forget_mse"]).all()) and runner.guard.flags.tolist() == [0.0] * 4
        return
    with pytest.raises(SfronError) as e:
        runner.guard.poll(block=True)
    msg = str(e.value)
    assert "by step 1" in msg, msg
    want = {"label": {2}, "timestep": {3}}.get(case)
    if want is not None:
        for k, reason in enumerate(guard.REASONS):
            assert (reason in msg) == (k in want), msg
        assert runner.guard.flags.tolist() == [0.0, 0.0, 1.0 if case == "label" else 0.0, 1.0 if case == "timestep" else 0.0]
    else:
        assert guard.REASONS[0] in msg and "outside" not in msg, msg
