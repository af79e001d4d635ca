"""GPU: every 3x3 convolution form of the U-Nets and the VAE (same / DDPM Downsample / SD Downsample / nearest-x2 Upsample), forward AND backward,
launched exactly as unet._conv3 and its backward closure launch them (through _lib and unet._conv_desc, no model in between), against the
float64 CPU reference of tests/test_conv_forms_cpu.py -- which also owns the case table and says which kernel path each case reaches.

Per (case, form):  sfron_conv_wprep -> sfron_conv_fwd (bias, sample_vec as a column slice of a wider matrix, resid on half the cases) ->
sfron_cast_rows_colsum (bf16 dy + d bias) -> sfron_conv_wgrad_splits / sfron_conv_wgrad / sfron_conv_wgrad_scatter (dW) -> the input gradient
(down*: dilate = 1, pad = 2 - pad; up: plain, then sfron_pool2_sum; same: plain) -> sfron_sample_colsum (d vec, with and without scratch).

Integer variant: all inputs are integers in -3 .. 3, so every partial sum is an integer below 2^24 (test_conv_forms_cpu.py checks that) and
every output must equal the reference with NO tolerance.  One wrong tap at one border, one dropped row of a column sum fails it.
Float variant: the bounds test_gpu_unet.test_conv3x3_forward_dgrad_wgrad already holds these kernels to,
    forward  rtol 2e-4, atol 2e-4 sqrt(9 c_in)      dW  rtol 3e-4, atol 3e-4 sqrt(rows)      dX  rtol 3e-4, atol 3e-4 sqrt(9 c_out)
and for a column sum of n fp32 terms  n 2^-23 sum |x|  per column: twice the first-order worst case (n - 1) 2^-24 sum |x| of ANY summation
order, computed from the inputs.

Outputs are pre-filled with NaN and followed by 64 guard elements whose bit pattern must survive; the wide d vec matrix must keep its columns
outside the slice.  Failures are reported by region (the four borders, the last rows of the last sample, then every element); every check prints
its largest error / bound ratio first (pytest -s)."""
import ctypes
import math

import pytest
import torch

import test_conv_forms_cpu as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = 1001                 # SFRON_ERR_ARG (csrc/common.h)
EPS = 2.0 ** -23
SENTINEL = -777.25
GUARD = 64
PATTERN = {4: (torch.int32, 0x5A5AA5A5), 2: (torch.int16, 0x5A5A)}


def _api():
    from sfron import _lib, unet
    return _lib.lib(), unet


def _sp():
    from sfron._lib import stream_ptr
    return stream_ptr()


def _ok(status, what):
    from sfron._lib import check
    check(status, what)


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
    """a launch that faulted leaves the device context unusable: end the session there instead of launching the remaining cases on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault in tests/test_gpu_conv_forms.py: {e}", returncode=3)


class Guarded:
    """n elements of NaN followed by 64 guard elements of a fixed bit pattern"""

    def __init__(self, n, dtype=torch.float32, fill=float("nan")):
        self.n = n
        self.full = torch.empty(n + GUARD, dtype=dtype, device=DEV)
        self.t = self.full[:n]
        self.t.fill_(fill)
        self.idt, self.pat = PATTERN[self.full.element_size()]
        self.full[n:].view(self.idt).fill_(self.pat)

    @property
    def ptr(self):
        return self.full.data_ptr()

    def assert_intact(self, what):
        assert bool((self.full[self.n:].view(self.idt) == self.pat).all()), f"{what}: wrote past its end"


def _bits(t):
    return t.contiguous().view(PATTERN[t.element_size()][0])


def _rows(x, cpad):
    """NCHW [B][C][H][W] -> NHWC rows [B*H*W][cpad] fp32, channels C.. zero"""
    B, C, H, W = x.shape
    r = torch.zeros(B * H * W, cpad)
    r[:, :C] = x.permute(0, 2, 3, 1).reshape(B * H * W, C)
    return r


def _check(got, ref, bound, what):
    """|got - ref| <= bound for every element (float64 on the CPU; bound a number or a tensor that broadcasts, 0 = exact).  Prints the largest
    error / bound ratio, names the worst element.  Returns the ratio."""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output ({int((~torch.isfinite(got)).sum())} of {got.numel()})"
    err = (got - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    over = err - bound
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = int(over.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), got.shape))
    n_over = int((over > 0).sum())
    print(f"[forms] {what}: max |err| {float(err.max()):.3e}, worst err/bound {float(ratio.max()):.3e}, {n_over} of {got.numel()} over")
    assert n_over == 0, (f"{what}: {n_over} of {got.numel()} elements out of bound; worst at {idx}: got {float(got.flatten()[worst])!r}, "
                         f"want {float(ref.flatten()[worst])!r}, bound {float(bound.flatten()[worst]):.3e}")
    return float(ratio.max())


def _regions(got, ref, bound, what):
    """got / ref / bound [B][h][w][c] (bound: the allowance per element, 0 = exact): the four borders and the last (up to) 256 rows of the last
    sample on their own, then every element.  Returns the largest error / bound ratio."""
    got, ref = got.detach().double().cpu(), ref.double()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    c = ref.shape[-1]
    for name, cut in (("top border", lambda t: t[:, 0]), ("bottom border", lambda t: t[:, -1]), ("left border", lambda t: t[:, :, 0]),
                      ("right border", lambda t: t[:, :, -1]), ("last rows of the last sample", lambda t: t[-1].reshape(-1, c)[-256:])):
        _check(cut(got), cut(ref), cut(bound), f"{what} {name}")
    return _check(got, ref, bound, what + " every element")


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


RATIOS = {}        # (form, output) -> worst err / bound ratio of the float variant, printed once per update


def _note(form, output, ratio):
    if ratio > RATIOS.get((form, output), -1.0):
        RATIOS[(form, output)] = ratio
        print(f"[forms-ratio] form={form} output={output} worst={ratio:.3e}")


# ------------------------------------------------------------------------------------------------ the convolution forms
@pytest.mark.parametrize("ints", [True, False], ids=["int", "float"])
@pytest.mark.parametrize("case,form", T.GRID, ids=T.GRID_IDS)
def test_conv_form_forward_and_backward(case, form, ints):
    L, unet = _api()
    B, H, W, ci, co, _ = case
    ho, wo, stride, pad, up = T.geometry(form, H, W)
    cip, cop = T.pad8(ci), T.pad8(co)
    rows, srows = B * ho * wo, B * H * W
    r = T.reference(case, form, ints)
    inp = r.inp
    tag = f"{'int' if ints else 'float'} {T.case_id(case)} {form}"
    z = 0.0 if ints else 1.0        # the integer variant: every bound is 0

    # ---- operands (sfron_conv_wprep): w_fwd [cop][9][cip] zero padded, w_dgrad [ci][9 flipped][cop]
    w_d = inp.w.to(DEV)
    wf = Guarded(cop * 9 * cip, torch.bfloat16)
    wd = Guarded(ci * 9 * cop, torch.bfloat16) if ci % 8 == 0 else None
    _ok(L.sfron_conv_wprep(w_d.data_ptr(), co, ci, 9, cop, cip, wf.ptr, wd.ptr if wd else None, _sp()), "conv_wprep")
    want_wf = torch.zeros(cop, 9, cip)
    want_wf[:co, :, :ci] = inp.wq.permute(0, 2, 3, 1).reshape(co, 9, ci)
    assert torch.equal(wf.t.view(cop, 9, cip).float().cpu(), want_wf), f"{tag}: w_fwd is not bf16(w) in [c_out_p][tap][c_in_p] with zero padding"
    wf.assert_intact(tag + " w_fwd")
    if wd:
        got_wd = wd.t.view(ci, 9, cop).float().cpu()
        assert bool(torch.isfinite(got_wd).all()) and float(got_wd[:, :, co:].abs().max() if cop != co else 0.0) == 0.0, f"{tag}: w_dgrad padding"
        wd.assert_intact(tag + " w_dgrad")

    # ---- forward: bias + sample_vec (columns 4 .. 4 + cop of a [B][cop + 8] matrix whose other columns hold 1e30) + resid
    xr = _rows(inp.x, cip).to(torch.bfloat16).to(DEV)
    bias_p = torch.zeros(cop)
    bias_p[:co] = inp.bias
    bias_p = bias_p.to(DEV)
    ldv = cop + 8
    vecw = torch.full((B, ldv), 1e30)
    vecw[:, 4:4 + cop] = 0.0
    vecw[:, 4:4 + co] = inp.vec
    vecw = vecw.to(DEV)
    resid = _rows(inp.resid, cop).to(DEV) if inp.resid is not None else None

    def forward():
        out = Guarded(rows * cop)
        d = unet._conv_desc(B, H, W, cip, ho, wo, cop, 9, stride, pad, up, 0, bias=bias_p, resid=resid, vec=vecw.data_ptr() + 16, ld_vec=ldv,
                            out_f32=out.t.view(rows, cop), ld_out=cop)
        assert bool(d.split_ws) == (9 * cip >= 2048), "unet._conv_desc arms split_ws by itself when taps * c_src >= 2048"
        _ok(L.sfron_conv_fwd(ctypes.byref(d), xr.data_ptr(), wf.ptr, _sp()), "conv_fwd")
        out.assert_intact(tag + " y")
        return out.t.view(B, ho, wo, cop)
    y = forward()
    assert torch.equal(_bits(forward()), _bits(y)), f"{tag}: two forward launches differ"
    ry = _nhwc(r.y)
    e = _regions(y[..., :co], ry, z * (2e-4 * math.sqrt(9 * ci) + 2e-4 * ry.abs()), tag + " y")
    if cop != co:
        assert float(y[..., co:].abs().max()) == 0.0, f"{tag}: padded output columns must be exactly 0"
    if not ints:
        _note(form, "y", e)

    # ---- dy -> bf16 operand + bias gradient
    dy_r = _rows(inp.dy, cop).to(DEV)
    dyb, dbias = Guarded(rows * cop, torch.bfloat16), Guarded(cop)
    if cop == co:
        part = Guarded(512 * cop)
        _ok(L.sfron_cast_rows_colsum(dy_r.data_ptr(), cop, rows, cop, dyb.ptr, part.ptr, 512, dbias.ptr, _sp()), "cast_rows_colsum")
        part.assert_intact(tag + " column-sum partials")
    else:           # conv_out: 3 or 4 channels computed as 8
        part = torch.empty(64 * cop, dtype=torch.float32, device=DEV)
        _ok(L.sfron_cast_rows_bf16(dy_r.data_ptr(), cop, rows, cop, dyb.ptr, _sp()), "cast_rows")
        unet.colsum_f32(dy_r, rows, cop, cop, dbias.t, part)
    dyb.assert_intact(tag + " dyb")
    dbias.assert_intact(tag + " d bias")
    assert torch.equal(_bits(dyb.t), _bits(dy_r.to(torch.bfloat16).flatten())), f"{tag}: dyb != dy.to(bfloat16)"
    dyd = inp.dy.double()
    e = _check(dbias.t[:co], r.dbias, z * rows * EPS * dyd.abs().sum(dim=(0, 2, 3)), tag + " d bias")
    if cop != co:
        assert float(dbias.t[co:].abs().max()) == 0.0
    if not ints:
        _note(form, "dbias", e)

    # ---- weight gradient, twice: slabs -> OIHW
    wdsc = unet._conv_desc(B, H, W, cip, ho, wo, cop, 9, stride, pad, up, 0)
    nsl = L.sfron_conv_wgrad_splits(ctypes.byref(wdsc))
    assert nsl >= 1
    slab = cop * 9 * cip

    def wgrad():
        dwg, dw = Guarded(nsl * slab), Guarded(co * ci * 9)
        _ok(L.sfron_conv_wgrad(ctypes.byref(wdsc), dyb.ptr, cop, xr.data_ptr(), dwg.ptr, _sp()), "conv_wgrad")
        _ok(L.sfron_conv_wgrad_scatter(dwg.ptr, co, ci, 9, cip, nsl, slab, dw.ptr, _sp()), "conv_wgrad_scatter")
        dwg.assert_intact(tag + " dW slabs")
        dw.assert_intact(tag + " dW")
        return dwg.t, dw.t.view(co, ci, 3, 3)
    dwg, dw = wgrad()
    dwg2, dw2 = wgrad()
    assert torch.equal(_bits(dwg), _bits(dwg2)) and torch.equal(_bits(dw), _bits(dw2)), f"{tag}: two weight-gradient launches differ ({nsl} slabs)"
    assert bool(torch.isfinite(dwg).all()), f"{tag}: a weight-gradient slab was left unwritten ({nsl} slabs)"
    slabs = dwg.view(nsl, cop, 9, cip)
    assert float(slabs[:, co:].abs().max() if cop != co else 0.0) == 0.0 and float(slabs[..., ci:].abs().max() if cip != ci else 0.0) == 0.0, \
        f"{tag}: padded rows / columns of the weight-gradient slabs must be exactly 0"
    for t in range(9):          # a wrong tap names itself
        _check(dw[:, :, t // 3, t % 3], r.dw[:, :, t // 3, t % 3], z * (3e-4 * math.sqrt(rows) + 3e-4 * r.dw[:, :, t // 3, t % 3].abs()),
               tag + f" dW tap ({t // 3}, {t % 3}) [{nsl} slabs]")
    e = _check(dw, r.dw, z * (3e-4 * math.sqrt(rows) + 3e-4 * r.dw.abs()), tag + " dW every element")
    if not ints:
        _note(form, "dW", e)

    # ---- d vec: per-sample column sums of dy into columns 4 .. 4 + cop of a [B][cop + 8] matrix, chunked (scratch) and direct
    bound_vec = z * (ho * wo) * EPS * dyd.abs().sum(dim=(2, 3))
    for with_scratch in (True, False):
        dvec = Guarded(B * ldv, fill=SENTINEL)
        dvw = dvec.t.view(B, ldv)
        dvw[:, 4:4 + cop] = float("nan")
        scratch = Guarded(B * 32 * cop) if with_scratch else None
        _ok(L.sfron_sample_colsum(dy_r.data_ptr(), cop, B, ho * wo, cop, dvec.ptr + 16, ldv, scratch.ptr if scratch else None,
                                  B * 32 * cop if scratch else 0, _sp()), "sample_colsum")
        dvec.assert_intact(tag + " d vec")
        if scratch:
            scratch.assert_intact(tag + " d vec scratch")
        assert bool((dvw[:, :4] == SENTINEL).all()) and bool((dvw[:, 4 + cop:] == SENTINEL).all()), f"{tag}: d vec wrote outside its column slice"
        e = _check(dvw[:, 4:4 + co], r.dvec, bound_vec, tag + f" d vec ({'scratch' if with_scratch else 'direct'})")
        if cop != co:
            assert float(dvw[:, 4 + co:4 + cop].abs().max()) == 0.0
        if not ints:
            _note(form, "dvec", e)

    # ---- input gradient
    if wd is None:
        return
    ds = Guarded(srows * ci)
    if form in T.DOWN:          # flipped kernel over the zero-dilated dY, padding 2 - pad
        dd = unet._conv_desc(B, ho, wo, cop, H, W, ci, 9, 1, 2 - pad, 0, 1, out_f32=ds.t.view(srows, ci), ld_out=ci)
        _ok(L.sfron_conv_fwd(ctypes.byref(dd), dyb.ptr, wd.ptr, _sp()), "conv_dgrad")
    elif form == "up":          # gradient wrt the upsampled image, then the 2 x 2 sums
        du = Guarded(rows * ci)
        dd = unet._conv_desc(B, ho, wo, cop, ho, wo, ci, 9, 1, 1, 0, 0, out_f32=du.t.view(rows, ci), ld_out=ci)
        _ok(L.sfron_conv_fwd(ctypes.byref(dd), dyb.ptr, wd.ptr, _sp()), "conv_dgrad")
        du.assert_intact(tag + " d upsampled")
        _ok(L.sfron_pool2_sum(du.ptr, B, H, W, ci, ds.ptr, 0, _sp()), "pool2_sum")
    else:
        dd = unet._conv_desc(B, ho, wo, cop, ho, wo, ci, 9, 1, 1, 0, 0, out_f32=ds.t.view(srows, ci), ld_out=ci)
        _ok(L.sfron_conv_fwd(ctypes.byref(dd), dyb.ptr, wd.ptr, _sp()), "conv_dgrad")
    assert bool(dd.split_ws) == (9 * cop >= 2048)
    ds.assert_intact(tag + " dX")
    rdx = _nhwc(r.dx)
    e = _regions(ds.t.view(B, H, W, ci), rdx, z * (3e-4 * math.sqrt(9 * co) + 3e-4 * rdx.abs()), tag + " dX")
    if not ints:
        _note(form, "dX", e)


def test_split_pending_with_a_bf16_output_is_refused_before_any_launch():
    """sfron_conv_desc.split_pending leaves fp32 slabs for a GroupNorm to finish into the fp32 output; with out_bf16 nothing would ever write the
    output.  The call must refuse (SFRON_ERR_ARG), leave *split_pending == 0 and touch neither the output nor split_ws."""
    L, unet = _api()
    B, S, C = 2, 6, 256
    rows = B * S * S
    g = torch.Generator().manual_seed(3)
    xr = torch.randint(-3, 4, (rows, C), generator=g).to(torch.bfloat16).to(DEV)
    wf = torch.randint(-3, 4, (C * 9 * C,), generator=g).to(torch.bfloat16).to(DEV)
    out, ws = Guarded(rows * C, torch.bfloat16), Guarded(4 * rows * C)
    pend = ctypes.c_int(7)
    d = unet._conv_desc(B, S, S, C, S, S, C, 9, 1, 1, 0, 0, out_bf16=out.t.view(rows, C), ld_out=C, pending=pend)
    assert d.split_ws and d.split_pending
    d.split_ws, d.split_ws_slabs = ws.ptr, 4
    assert L.sfron_conv_fwd(ctypes.byref(d), xr.data_ptr(), wf.data_ptr(), _sp()) == ERR_ARG
    torch.cuda.synchronize()
    assert pend.value == 0
    assert bool(torch.isnan(out.t).all()) and bool(torch.isnan(ws.t).all()), "a refused call wrote to its output or to split_ws"
    out.assert_intact("refused out_bf16")
    ws.assert_intact("refused split_ws")
    # the same description with an fp32 output is accepted and leaves its slabs pending
    out32 = Guarded(rows * C)
    d.out_bf16, d.out_f32 = None, out32.ptr
    _ok(L.sfron_conv_fwd(ctypes.byref(d), xr.data_ptr(), wf.data_ptr(), _sp()), "conv_fwd")
    assert 1 < pend.value <= 4 and bool(torch.isnan(out32.t).all())
    slabs = ws.t.view(4, rows, C)[:pend.value].double().sum(0).cpu()
    x = xr.float().cpu().view(B, S, S, C).permute(0, 3, 1, 2).double()
    w = wf.float().cpu().view(C, 3, 3, C).permute(0, 3, 1, 2).double()
    assert torch.equal(slabs.view(B, S, S, C), _nhwc(torch.nn.functional.conv2d(x, w, None, padding=1))), "the pending slabs do not add up to the convolution"
    ws.assert_intact("split_ws")


# ------------------------------------------------------------------------------------------------ the row kernels on their own grid
def _draw(g, ints, *shape):
    return torch.randint(-3, 4, shape, generator=g).float() if ints else torch.randn(*shape, generator=g)


@pytest.mark.parametrize("ints", [True, False], ids=["int", "float"])
@pytest.mark.parametrize("rows", [1, 37, 432, 4097])
@pytest.mark.parametrize("C", [8, 72, 320])
def test_cast_rows_colsum_and_its_two_step_form(C, rows, ints):
    """y = bf16(x) bit for bit (round to nearest even, as torch), column sums exact (integers) or within n 2^-23 sum |x|; the one-call and the
    partials + sfron_reduce_chunks forms agree bit for bit; *chunks_out <= max_partials; columns C .. ldx of x (1e30) are never read."""
    L, _ = _api()
    g = torch.Generator().manual_seed(C * 10000 + rows)
    for ldx in (C, C + 8):
        x = torch.full((rows, ldx), 1e30)
        x[:, :C] = _draw(g, ints, rows, C)
        ref = x[:, :C].double().sum(0)
        bound = (0.0 if ints else 1.0) * rows * EPS * x[:, :C].double().abs().sum(0)
        want_y = _bits(x[:, :C].contiguous().to(torch.bfloat16))
        xd = x.to(DEV)
        for mp in (1, 64):
            tag = f"cast_rows_colsum {'int' if ints else 'float'} C={C} rows={rows} ldx={ldx} max_partials={mp}"
            y1, p1, s1 = Guarded(rows * C, torch.bfloat16), Guarded(mp * C), Guarded(C)
            _ok(L.sfron_cast_rows_colsum(xd.data_ptr(), ldx, rows, C, y1.ptr, p1.ptr, mp, s1.ptr, _sp()), "cast_rows_colsum")
            y2, p2, s2, nch = Guarded(rows * C, torch.bfloat16), Guarded(mp * C), Guarded(C), ctypes.c_int(-1)
            _ok(L.sfron_cast_rows_colsum_partials(xd.data_ptr(), ldx, rows, C, y2.ptr, p2.ptr, mp, ctypes.byref(nch), _sp()), "cast_rows_colsum_partials")
            assert 1 <= nch.value <= mp, (tag, nch.value)
            _ok(L.sfron_reduce_chunks(p2.ptr, 1, nch.value, C, s2.ptr, C, 0, _sp()), "reduce_chunks")
            for o, name in ((y1, "y"), (p1, "partials"), (s1, "colsum"), (y2, "y (two-step)"), (p2, "partials (two-step)"), (s2, "colsum (two-step)")):
                o.assert_intact(f"{tag} {name}")
            assert torch.equal(_bits(y1.t).cpu().view(rows, C), want_y), f"{tag}: y != x.to(bfloat16)"
            assert torch.equal(_bits(y1.t), _bits(y2.t)) and torch.equal(_bits(s1.t), _bits(s2.t)), f"{tag}: the two entry points differ"
            assert torch.equal(_bits(p1.t[:nch.value * C]), _bits(p2.t[:nch.value * C]))
            assert bool(torch.isnan(p2.t[nch.value * C:]).all()), f"{tag}: partials beyond *chunks_out were written"
            _check(p2.t[:nch.value * C].view(nch.value, C).double().sum(0), ref, bound, tag + " sum of the partials")
            _check(s1.t, ref, bound, tag + " colsum")


@pytest.mark.parametrize("ints", [True, False], ids=["int", "float"])
@pytest.mark.parametrize("B,HW,C", [(1, 4, 8), (3, 60, 72), (4, 960, 128), (16, 144, 320)])
def test_sample_colsum_chunked_and_direct(B, HW, C, ints):
    """row chunks per sample nz = min(32, 512 / (ceil(C / 64) B), HW / 16): 0, 3, 32 and 6 at these shapes; nz <= 1 or no scratch = one launch"""
    L, _ = _api()
    g = torch.Generator().manual_seed(B * 1000 + HW + C)
    ld, ldo = C + 8, C + 12
    x = torch.full((B * HW, ld), 1e30)
    x[:, :C] = _draw(g, ints, B * HW, C)
    xs = x[:, :C].double().view(B, HW, C)
    ref, bound = xs.sum(1), (0.0 if ints else 1.0) * HW * EPS * xs.abs().sum(1)
    xd = x.to(DEV)
    for with_scratch in (True, False):
        tag = f"sample_colsum {'int' if ints else 'float'} B={B} HW={HW} C={C} {'scratch' if with_scratch else 'direct'}"
        out = Guarded(B * ldo, fill=SENTINEL)
        ow = out.t.view(B, ldo)
        ow[:, 4:4 + C] = float("nan")
        scratch = Guarded(B * 32 * C) if with_scratch else None
        _ok(L.sfron_sample_colsum(xd.data_ptr(), ld, B, HW, C, out.ptr + 16, ldo, scratch.ptr if scratch else None, B * 32 * C if scratch else 0, _sp()),
            "sample_colsum")
        out.assert_intact(tag)
        if scratch:
            scratch.assert_intact(tag + " scratch")
        assert bool((ow[:, :4] == SENTINEL).all()) and bool((ow[:, 4 + C:] == SENTINEL).all()), f"{tag}: wrote outside its column slice"
        _check(ow[:, 4:4 + C], ref, bound, tag)


@pytest.mark.parametrize("ints", [True, False], ids=["int", "float"])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("B,H,W,C", [(2, 1, 1, 8), (3, 6, 10, 4), (2, 12, 20, 64)])
def test_pool2_sum_overwrites_or_accumulates(B, H, W, C, accumulate, ints):
    """dx[b][h][w][c] (+)= the 2 x 2 block of dy [B][2H][2W][C]; 4 (5 with accumulate) fp32 terms per output"""
    L, _ = _api()
    g = torch.Generator().manual_seed(B + 10 * H + 100 * W + C)
    dy = _draw(g, ints, B, 2 * H, 2 * W, C)
    blocks = dy.double().view(B, H, 2, W, 2, C)
    ref, mag, n = blocks.sum(dim=(2, 4)), blocks.abs().sum(dim=(2, 4)), 4
    dx = Guarded(B * H * W * C)
    if accumulate:
        before = _draw(g, ints, B, H, W, C)
        dx.t.copy_(before.flatten())
        ref, mag, n = ref + before.double(), mag + before.double().abs(), 5
    _ok(L.sfron_pool2_sum(dy.to(DEV).data_ptr(), B, H, W, C, dx.ptr, accumulate, _sp()), "pool2_sum")
    tag = f"pool2_sum {'int' if ints else 'float'} {B}x{H}x{W}x{C} accumulate={accumulate}"
    dx.assert_intact(tag)
    _regions(dx.t.view(B, H, W, C), ref, (0.0 if ints else 1.0) * n * EPS * mag, tag)
