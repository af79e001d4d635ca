"""GPU: the row-wise and elementwise kernels of the DDPM U-Net and the SD / ldm transformer block (csrc/rows.hip), every dispatch form at the
smallest shape that reaches it, through the C ABI, against the restatements of tests/unet_rows_ref.py: fp32 outputs under bound32, bf16
outputs under bound_bf16 (the yardstick is the float32 CPU evaluation of the same expression, never the kernel), layout / cast / copy /
select / mask / axpby outputs bit for bit.  Every output lives in a guarded() buffer whose sentinels are checked after the call.  A
"misaligned" operand is a view one element (4 bytes; 2 for a bf16 output) into a 16-byte-aligned allocation: it sends a D % 4 == 0 shape
to the plain form, so the same shape runs in both forms and each is compared with the reference (they are not bit-equal to each other).

Kernels of rows.hip, and the case that reaches each:
  k_layernorm_fwd_r<2>        test_layernorm_fwd  D = 4 (one live lane), 256, 260 (one lane into the second chunk), 512; rows 1, 3, 5 at D = 260
  k_layernorm_fwd_r<3>        test_layernorm_fwd  D = 516, 640, 768; rows 1, 3, 5 at D = 640
  k_layernorm_fwd_r<5>        test_layernorm_fwd  D = 772, 1280
  k_layernorm_fwd             test_layernorm_fwd  D = 1284, 2048, 1, 63, 322; test_layernorm_fwd_misaligned  D = 320, 640 with x, gamma, beta or y
                              misaligned; the shifted rows (x = randn + 300, D = 260) in test_layernorm_fwd_shifted_rows (_r<2> and plain)
  k_layernorm_bwd_r<2|3|5>    test_layernorm_bwd  the same widths at rows = 37; (8196, 8): 20 rows per block, 16 in the last; (30724, 8): 64 rows per
                              block, 4 in the last; (3, 260): one short block; accumulate 0 / 1, extra NULL / given
  k_layernorm_bwd             test_layernorm_bwd  D = 1284, 2048 (64 KiB of LDS), 1, 63, 322, (3, 63); every vector width again with extra misaligned
                              test_layernorm_bwd_res_is_copy_then_bwd  both forms, bit for bit; test_layernorm_bwd_refusals  extra == dx, D = 2052
  k_geglu_fwd4 / k_geglu_bwd4 test_geglu  F = 4 (one live thread), 1024 (a full column block), 1028 (one live thread in the second), (F, rows) =
                              (8, 4099): 2 rows per block, one in the last
  k_geglu_fwd / k_geglu_bwd   test_geglu  F = 5; F = 8 with h, out / dh or d_out misaligned; (1023, 1030): the second grid-stride trip
  k_softmax_fwd / _bwd        test_softmax  n = 3 (61 idle lanes), 64, 65, 80 with 77 keys, 200 with 130 keys; rows 3, 5, 6, 37 (idle waves);
                              test_softmax_large_logits  30 randn at scale 1
  k_nchw_to_rows              test_layouts  c_pad = C, C + 1, C rounded up to 8 at (B, C, HW) = (2,3,5), (3,4,16), (2,130,7)
  k_nchw_to_rows_f32          test_layouts  ld = C, C + 5
  k_rows_to_nchw              test_layouts  ld = C, C + 5 over sentinel-filled pad columns
  k_image_u8_to_rows          (not here) tests/test_gpu_vae.py::test_image_kernel_is_the_torch_formula_bit_for_bit
  k_rows_to_image_u8          (not here) tests/test_gpu_vae_decoder.py::test_image_kernel_is_the_restated_formula_bit_for_bit (the three
                              rounding modes, the make_grid canvas)
  k_cast_rows4<false>         test_cast_rows  C = 4, 256, 260 at ldx = C, C + 4; rows 1, 7, 4101 (several row chunks, the last short)
  k_cast_rows                 test_cast_rows  C = 5; C = 260 at ldx = C + 2; C = 260 with x misaligned
  k_cast_rows4<true>          test_cast_rows_colsum  (100, 260) at ldx = 264
  k_copy_cols4 / k_copy_cols  test_copy_cols  the same ladder, accumulate 0 / 1, ldy > C
  k_copy_cols4x2              test_copy_cols2  C0 = 260, C1 = 8, the accumulate flags mixed; ldx1 = C1 + 1 falls back to two plain launches
  k_axpby                     test_axpby  n = 1, 257, 4096 * 256 + 1 (the grid-stride trip)
  k_sample_colsum             test_sample_colsum  one launch (HW = 5) and the row-chunked form with scratch (HW = 64: 4 chunks)
  k_pool2_sum                 test_pool2_sum  (2, 3, 5, 7), accumulate 0 / 1
  k_dropout_mask              test_dropout_mask  p = 0, 0.1, 0.5, 0.999; n = 1, 3, 4, 5, 1001, 4 * 4096 * 256 + 3; seeds, salts, counter 0 / 5
  k_dropout_mask_batch        test_dropout_mask_batch  items of 4, 7, 1001, 70001 bytes (70001 passes the 64-workgroup cap), pad bytes between
  k_ddpm_temb                 test_ddpm_timestep_embed  dim = 4, 128, 129 (zero last column), 512; t = 0 .. 7 and 37, 250, 999
  k_class_embed / _bwd        test_class_embed  D = 1, 300, 512; n = 1, 9; a repeated label, -1, n_classes; keep NULL / given

Found while writing this module, fixed with it: sfron_layernorm_bwd(_res) accepted D <= 4096 but asks for 32 D bytes of dynamic LDS without
raising the function's limit -- past 64 KiB above D = 2048.  The entry points now refuse D > 2048 (test_layernorm_bwd_refusals; D = 2048
itself runs in test_layernorm_bwd).

Mismatch shares (elements that differ from bf16(ref64), see the cap sets in tests/unet_rows_ref.py) of one run on an MI355X; RECORD
prints the current ones at teardown (pytest -s):
  softmax p, scaled logits within 16 of the row maximum   4.2e-4 (capped)      softmax ds from that p   4.2e-4 (capped)
  softmax p, logits 30 randn at scale 1                   5.8 %  (not capped)  softmax ds from that p   0.32 % (not capped)
  GEGLU forward, gate >= -2     vector 3.4e-5, plain 1.1e-5 (capped); over all elements up to 7.1 %, at the small shapes where the tail
                                values are most of the tensor
  GEGLU backward, gate >= -1    vector 2.2e-4 (d gate alone 4.4e-4), plain 3.0e-5 (capped)
  LayerNorm y                   5.2e-5 .. 1.1e-4 (capped); shifted rows 1.5 % (not capped: the float32 restatement alone has 1.7 %)
  timestep embedding            0 on the rows with t <= 7 (capped), 7.3e-4 over all rows
Largest error over bound (bf16 outputs, `excess`): 0.996.  fp32 outputs: error over the float32 restatement's own error at most 3.1 (LN
forward mean, _r<3>), with the bound at 4 plus four ulps."""
import functools
import math

import pytest
import torch

import unet_rows_ref as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = 1001          # csrc/common.h
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


def _L():
    from sfron import _lib
    return _lib.lib()


def _sp():
    from sfron._lib import stream_ptr
    return stream_ptr()


def dev(t):
    return t.contiguous().to(DEV)


def dev_mis(t):
    """the same values in a view one element into a fresh (aligned) allocation: 4 bytes off for fp32"""
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size()
    return v


def guarded_off(shape, dtype, off=1):
    """a guarded buffer whose view starts `off` elements past a 16-byte boundary; the elements before it count as guard"""
    flat, check = U.guarded((math.prod(shape) + off,), dtype)

    def check2(what=""):
        check(what)
        assert bool((flat[:off].view(check.full.dtype) == check.sentinel).all()), f"{what}: the elements before a misaligned output were written"

    check2.full, check2.sentinel = check.full, check.sentinel
    return flat[off:].view(shape), check2


def sync():
    torch.cuda.synchronize()


def p(t):
    return t.data_ptr() if t is not None else None


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
    """a launch that faulted leaves the device context unusable: end the session there instead of launching the remaining cases on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault in tests/test_gpu_unet_rows.py: {e}", returncode=3)


@pytest.fixture(scope="module", autouse=True)
def _print_record():
    yield
    print()
    for name in sorted(U.RECORD):
        print("RECORD", name, " ".join(f"{k}={v:.4g}" for k, v in sorted(U.RECORD[name].items())))


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ================================================================================================ a. LayerNorm forward
@functools.lru_cache(maxsize=None)
def ln_case(rows, D, eps, shifted=False):
    i = U.ln_inputs(rows, D, shifted)
    return i, U.layernorm_fwd(i["x"], i["gamma"], i["beta"], eps, F64), U.layernorm_fwd(i["x"], i["gamma"], i["beta"], eps, F32)


def run_ln_fwd(i, rows, D, eps, mis=None):
    put = lambda k: dev_mis(i[k]) if mis == k else dev(i[k])
    x, gamma, beta = put("x"), put("gamma"), put("beta")
    y, c_y = guarded_off((rows, D), BF16) if mis == "y" else U.guarded((rows, D), BF16)
    mean, c_m = U.guarded((rows,), F32)
    rstd, c_r = U.guarded((rows,), F32)
    st = _L().sfron_layernorm_fwd(p(x), p(gamma), p(beta), rows, D, eps, p(y), p(mean), p(rstd), _sp())
    assert st == 0, st
    sync()
    for c in (c_y, c_m, c_r):
        c(f"layernorm_fwd rows={rows} D={D} mis={mis}")
    return y, mean, rstd


def check_ln_fwd(got, r64, r32, tag, cap=True):
    none = None if cap else torch.zeros(r64[0].shape, dtype=torch.bool)
    U.bound_bf16(got[0], r64[0], r32[0], tag + ".y", cap_mask=none)
    U.bound32(got[1], r64[1], r32[1], tag + ".mean")
    U.bound32(got[2], r64[2], r32[2], tag + ".rstd")


@pytest.mark.parametrize("eps", U.LN_EPS)
@pytest.mark.parametrize("rows,D", U.LN_SHAPES)
def test_layernorm_fwd(rows, D, eps):
    i, r64, r32 = ln_case(rows, D, eps)
    check_ln_fwd(run_ln_fwd(i, rows, D, eps), r64, r32, "ln_fwd." + U.ln_form(D))


@pytest.mark.parametrize("mis", ["x", "gamma", "beta", "y"])
@pytest.mark.parametrize("D", U.LN_MISALIGNED_D)
def test_layernorm_fwd_misaligned(D, mis):
    rows, eps = 37, 1e-5
    i, r64, r32 = ln_case(rows, D, eps)
    check_ln_fwd(run_ln_fwd(i, rows, D, eps), r64, r32, "ln_fwd." + U.ln_form(D))
    check_ln_fwd(run_ln_fwd(i, rows, D, eps, mis=mis), r64, r32, "ln_fwd.plain")


def test_layernorm_fwd_shifted_rows():
    """x = randn + 300: mean^2 is 9e4 times the variance.  rstd and y hold the bound with the two-pass variance the kernels compute; y is
    held to the error bound alone (the float32 restatement itself misses the share cap here: tests/test_unet_rows_ref_cpu.py)"""
    rows, D, eps = 37, 260, 1e-5
    i, r64, r32 = ln_case(rows, D, eps, True)
    check_ln_fwd(run_ln_fwd(i, rows, D, eps), r64, r32, "ln_fwd.shifted", cap=False)
    check_ln_fwd(run_ln_fwd(i, rows, D, eps, mis="x"), r64, r32, "ln_fwd.shifted", cap=False)


# ================================================================================================ b. LayerNorm backward
LN_BWD_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def ln_bwd_case(rows, D):
    i = U.ln_inputs(rows, D)
    rpb = U.layernorm_rows_per_block(rows)
    _, m64, r64 = U.layernorm_fwd(i["x"], i["gamma"], i["beta"], LN_BWD_EPS, F64)
    ref = {(dt, acc, ex): U.layernorm_bwd(i["dy"], i["x"], i["gamma"], LN_BWD_EPS, i["dx0"], acc, i["extra"] if ex else None, rpb, dt)
           for dt in (F64, F32) for acc in (0, 1) for ex in (0, 1)}
    d = dict(dy=dev(i["dy"]), x=dev(i["x"]), gamma=dev(i["gamma"]), mean=dev(m64.float()), rstd=dev(r64.float()), dx0=dev(i["dx0"]),
             extra=dev(i["extra"]), extra_mis=dev_mis(i["extra"]))
    return i, rpb, ref, d


def run_ln_bwd(rows, D, d, rpb, acc, extra, res_entry=True, dx_in=None):
    """extra: None | "given" | "mis".  acc = 0: dx starts as NaN sentinels and must come out finite"""
    L = _L()
    nblk = -(-rows // rpb)
    dx, c_dx = U.guarded((rows, D), F32)
    if acc:
        dx.copy_(d["dx0"] if dx_in is None else dx_in)
    pg, c_pg = U.guarded((nblk, D), F32)
    pb, c_pb = U.guarded((nblk, D), F32)
    ex = {None: None, "given": d["extra"], "mis": d["extra_mis"]}[extra]
    if res_entry:
        st = L.sfron_layernorm_bwd_res(p(d["dy"]), p(d["x"]), p(d["gamma"]), p(d["mean"]), p(d["rstd"]), rows, D, p(dx), acc, p(ex), p(pg), p(pb),
                                       _sp())
    else:
        assert ex is None
        st = L.sfron_layernorm_bwd(p(d["dy"]), p(d["x"]), p(d["gamma"]), p(d["mean"]), p(d["rstd"]), rows, D, p(dx), acc, p(pg), p(pb), _sp())
    assert st == 0, st
    sync()
    for c in (c_dx, c_pg, c_pb):
        c(f"layernorm_bwd rows={rows} D={D} acc={acc} extra={extra}")
    return dx, pg, pb


@pytest.mark.parametrize("rows,D", U.LN_BWD_SHAPES)
def test_layernorm_bwd(rows, D):
    i, rpb, ref, d = ln_bwd_case(rows, D)
    assert _L().sfron_layernorm_rows_per_block(rows) == rpb
    form = U.ln_form(D)
    for acc in (0, 1):
        for extra in (None, "given", "mis"):
            for res_entry in ((False, True) if extra is None else (True,)):
                dx, pg, pb = run_ln_bwd(rows, D, d, rpb, acc, extra, res_entry)
                tag = "ln_bwd." + ("plain" if extra == "mis" else form)
                w64, w32 = ref[(F64, acc, int(extra is not None))], ref[(F32, acc, int(extra is not None))]
                U.bound32(dx, w64[0], w32[0], tag + ".dx")
                U.bound32(pg, w64[1], w32[1], tag + ".part_gamma")          # every block's row, the short last one included
                U.bound32(pb, w64[2], w32[2], tag + ".part_beta")


@pytest.mark.parametrize("rows,D", [(37, 260), (37, 640), (37, 1280), (37, 63), (37, 1284), (8196, 8)])
def test_layernorm_bwd_res_is_copy_then_bwd(rows, D):
    """include/sfron.h: the bits of a separate dx (+)= extra pass followed by sfron_layernorm_bwd, in the vector and the plain form"""
    i, rpb, ref, d = ln_bwd_case(rows, D)
    L = _L()
    for acc in (0, 1):
        fused = run_ln_bwd(rows, D, d, rpb, acc, "given")
        step, c_step = U.guarded((rows, D), F32)
        if acc:
            step.copy_(d["dx0"])
        assert L.sfron_copy_cols(p(d["extra"]), D, rows, D, p(step), D, acc, _sp()) == 0
        sync()
        c_step("copy_cols before layernorm_bwd")
        two = run_ln_bwd(rows, D, d, rpb, 1, None, res_entry=False, dx_in=step)
        for name, a, b in zip(("dx", "part_gamma", "part_beta"), fused, two):
            assert bits_equal(a, b), f"{name}: sfron_layernorm_bwd_res differs from copy + sfron_layernorm_bwd (accumulate = {acc}, {U.ln_form(D)})"


def test_layernorm_bwd_refusals():
    """extra == dx, and D > 2048 (the launch would ask for more than 64 KiB of dynamic LDS): SFRON_ERR_ARG before any launch, never a raw
    HIP status.  D = 2048, exactly 64 KiB, runs in test_layernorm_bwd."""
    L = _L()
    rows, Dm = 8, 2052
    z = lambda *s: torch.zeros(*s, device=DEV)
    dy, x, gamma, mean, rstd, extra = z(rows, Dm), z(rows, Dm), z(Dm), z(rows), z(rows), z(rows, Dm)
    bufs = [U.guarded(s, F32) for s in ((rows, Dm), (1, Dm), (1, Dm))]
    (dx, _), (pg, _), (pb, _) = bufs
    for acc in (0, 1):
        assert L.sfron_layernorm_bwd_res(p(dy), p(x), p(gamma), p(mean), p(rstd), rows, 260, p(dx), acc, p(dx), p(pg), p(pb), _sp()) == ERR_ARG
        for D in (2052, 4096, 0):
            assert L.sfron_layernorm_bwd_res(p(dy), p(x), p(gamma), p(mean), p(rstd), rows, D, p(dx), acc, p(extra), p(pg), p(pb), _sp()) == ERR_ARG
            assert L.sfron_layernorm_bwd(p(dy), p(x), p(gamma), p(mean), p(rstd), rows, D, p(dx), acc, p(pg), p(pb), _sp()) == ERR_ARG
        assert L.sfron_layernorm_bwd(p(dy), p(x), p(gamma), p(mean), p(rstd), 0, 260, p(dx), acc, p(pg), p(pb), _sp()) == ERR_ARG
    y, c_y = U.guarded((rows, Dm), BF16)
    assert L.sfron_layernorm_fwd(p(x), p(gamma), p(gamma), rows, 0, 1e-5, p(y), p(pg), p(pb), _sp()) == ERR_ARG
    assert L.sfron_layernorm_fwd(p(x), p(gamma), p(gamma), 0, 260, 1e-5, p(y), p(pg), p(pb), _sp()) == ERR_ARG
    sync()
    for _, c in bufs + [(y, c_y)]:
        U.untouched(c, "refused LayerNorm call")


# ================================================================================================ c. GEGLU
@functools.lru_cache(maxsize=None)
def geglu_case(F_, rows):
    h, d_out = U.geglu_inputs(rows, F_)
    return h, d_out, {dt: (U.geglu_fwd(h, dt), U.geglu_bwd(d_out, h, dt)) for dt in (F64, F32)}, U.geglu_cap_masks(h)


@pytest.mark.parametrize("F_,rows,mis", U.GEGLU_VECTOR + U.GEGLU_PLAIN)
def test_geglu(F_, rows, mis):
    L = _L()
    h, d_out, ref, (mask_f, mask_b) = geglu_case(F_, rows)
    form = "vector" if (F_, rows, mis) in U.GEGLU_VECTOR else "plain"
    assert (form == "vector") == (F_ % 4 == 0 and mis is None)
    hd = dev_mis(h) if mis == "h" else dev(h)
    dd = dev_mis(d_out) if mis == "d_out" else dev(d_out)
    out, c_out = guarded_off((rows, F_), BF16) if mis == "out" else U.guarded((rows, F_), BF16)
    assert L.sfron_geglu_fwd(p(hd), rows, F_, p(out), _sp()) == 0
    dh, c_dh = guarded_off((rows, 2 * F_), BF16) if mis == "out" else U.guarded((rows, 2 * F_), BF16)
    assert L.sfron_geglu_bwd(p(dd), p(hd), rows, F_, p(dh), _sp()) == 0
    sync()
    c_out(f"geglu_fwd F={F_} rows={rows} mis={mis}")
    c_dh(f"geglu_bwd F={F_} rows={rows} mis={mis}")
    # the tails (gate = 0, +-1e-3, +-3, +-6, +-10, +-40 in the first elements) are finite and inside the same bound as everything else
    U.bound_bf16(out, ref[F64][0], ref[F32][0], f"geglu_fwd.{form}", cap_mask=mask_f)
    U.bound_bf16(dh, ref[F64][1], ref[F32][1], f"geglu_bwd.{form}", cap_mask=mask_b)
    U.bound_bf16(dh[:, :F_].contiguous(), ref[F64][1][:, :F_], ref[F32][1][:, :F_], f"geglu_bwd.{form}.d_value", cap_mask=mask_b[:, :F_])
    U.bound_bf16(dh[:, F_:].contiguous(), ref[F64][1][:, F_:], ref[F32][1][:, F_:], f"geglu_bwd.{form}.d_gate", cap_mask=mask_b[:, F_:])


def test_geglu_refusals():
    L = _L()
    h = torch.zeros(4, 16, device=DEV)
    out, c_out = U.guarded((4, 16), BF16)
    for rows, F_ in ((0, 8), (4, 0)):
        assert L.sfron_geglu_fwd(p(h), rows, F_, p(out), _sp()) == ERR_ARG
        assert L.sfron_geglu_bwd(p(h), p(h), rows, F_, p(out), _sp()) == ERR_ARG
    assert L.sfron_geglu_fwd(None, 4, 8, p(out), _sp()) == ERR_ARG
    sync()
    U.untouched(c_out, "refused GEGLU call")


# ================================================================================================ d. softmax
def run_softmax(s, dp, rows, n, nv, scale):
    L = _L()
    sd, dpd = dev(s), dev(dp)
    pr, c_p = U.guarded((rows, n), BF16)
    assert L.sfron_softmax_fwd(p(sd), rows, n, nv, scale, p(pr), _sp()) == 0
    ds, c_ds = U.guarded((rows, n), BF16)
    assert L.sfron_softmax_bwd(p(pr), p(dpd), rows, n, scale, p(ds), _sp()) == 0
    sync()
    c_p("softmax_fwd")
    c_ds("softmax_bwd")
    return pr, ds


@pytest.mark.parametrize("rows,n,nv,scale", U.SOFTMAX_CASES)
def test_softmax(rows, n, nv, scale):
    s, dp = U.softmax_inputs(rows, n, nv, scale)
    pr, ds = run_softmax(s, dp, rows, n, nv, scale)
    U.bound_bf16(pr, U.softmax_fwd(s, nv, scale, F64), U.softmax_fwd(s, nv, scale, F32), "softmax_fwd")
    p16 = pr.cpu()
    assert bool((p16[:, nv:].view(torch.int16) == 0).all()), "the padded columns of p are not the bit pattern of +0"
    # the backward from the bf16 p the kernel was given
    U.bound_bf16(ds, U.softmax_bwd(p16, dp, scale, F64), U.softmax_bwd(p16, dp, scale, F32), "softmax_bwd")
    assert bool((ds.cpu()[:, nv:].float() == 0).all()), "the padded columns of ds are not zero"


def test_softmax_large_logits():
    """30 randn at scale 1: the fast exponential's relative error grows with its argument, so the mismatch share is recorded, not capped"""
    rows, n, nv, scale = U.SOFTMAX_LARGE
    s, dp = U.softmax_inputs(rows, n, nv, scale, large=True)
    pr, ds = run_softmax(s, dp, rows, n, nv, scale)
    none = torch.zeros(rows, n, dtype=torch.bool)
    U.bound_bf16(pr, U.softmax_fwd(s, nv, scale, F64), U.softmax_fwd(s, nv, scale, F32), "softmax_fwd.large", cap_mask=none)
    assert bool(((pr.cpu().float().sum(1) - 1).abs() <= 2 ** -6).all()), "a row of p does not sum to 1 within 2^-6"
    p16 = pr.cpu()
    U.bound_bf16(ds, U.softmax_bwd(p16, dp, scale, F64), U.softmax_bwd(p16, dp, scale, F32), "softmax_bwd.large", cap_mask=none)


def test_softmax_refusals():
    L = _L()
    s = torch.zeros(4, 8, device=DEV)
    pr, c_p = U.guarded((4, 8), BF16)
    for rows, n, nv in ((0, 8, 8), (4, 0, 0), (4, 8, 0), (4, 8, 9)):
        assert L.sfron_softmax_fwd(p(s), rows, n, nv, 1.0, p(pr), _sp()) == ERR_ARG
    for rows, n in ((0, 8), (4, 0)):
        assert L.sfron_softmax_bwd(p(s), p(s), rows, n, 1.0, p(pr), _sp()) == ERR_ARG
    sync()
    U.untouched(c_p, "refused softmax call")


# ================================================================================================ e. layouts
@pytest.mark.parametrize("B,C,HW", U.LAYOUT_SHAPES)
def test_layouts(B, C, HW):
    L = _L()
    g = torch.Generator().manual_seed(B * 1000 + C * 10 + HW)
    x = torch.randn(B, C, HW, generator=g)
    xd = dev(x)
    for c_pad in (C, C + 1, (C + 7) // 8 * 8):
        rows, check = U.guarded((B * HW, c_pad), BF16)
        assert L.sfron_nchw_to_rows_bf16(p(xd), B, C, HW, c_pad, p(rows), _sp()) == 0
        sync()
        check("nchw_to_rows_bf16")
        assert bits_equal(rows, U.nchw_to_rows(x, c_pad).to(BF16)), f"nchw_to_rows_bf16 c_pad={c_pad}"       # pad columns: the bits of +0
    for ld in (C, C + 5):
        rows, check = U.guarded((B * HW, ld), F32)
        assert L.sfron_nchw_to_rows_f32(p(xd), B, C, HW, ld, p(rows), _sp()) == 0
        sync()
        check("nchw_to_rows_f32")
        assert bits_equal(rows, U.nchw_to_rows(x, ld)), f"nchw_to_rows_f32 ld={ld}"
        src = torch.full((B * HW, ld), 12345.0)                     # pad columns that must not leak
        src[:, :C] = torch.randn(B * HW, C, generator=g)
        back, check = U.guarded((B, C, HW), F32)
        assert L.sfron_rows_to_nchw(p(dev(src)), ld, B, C, HW, p(back), _sp()) == 0
        sync()
        check("rows_to_nchw")
        assert bits_equal(back, U.rows_to_nchw(src, B, C, HW)), f"rows_to_nchw ld={ld}"
    r16, c16 = U.guarded((B * HW, C), BF16)
    r32, c32 = U.guarded((B * HW, C), F32)
    assert L.sfron_nchw_to_rows_bf16(p(xd), B, C, HW, C - 1, p(r16), _sp()) == ERR_ARG
    assert L.sfron_nchw_to_rows_f32(p(xd), B, C, HW, C - 1, p(r32), _sp()) == ERR_ARG
    assert L.sfron_rows_to_nchw(p(xd), C - 1, B, C, HW, p(r32), _sp()) == ERR_ARG
    sync()
    U.untouched(c16, "c_pad < C")
    U.untouched(c32, "ld < C")


# ================================================================================================ f. casts and copies
# (C, ldx - C, x misaligned): the float4 forms need C % 4 == 0, ld % 4 == 0 and 16-byte pointers
COPY_LADDER = [(4, 0, False), (4, 4, False), (256, 0, False), (256, 4, False), (260, 0, False), (260, 4, False),
               (5, 0, False), (260, 2, False), (260, 0, True)]
COPY_ROWS = (1, 7, 4101)


def strided_src(rows, C, ldx, seed, misaligned):
    full = U.tie_values(rows, ldx, seed)
    return full, (dev_mis(full) if misaligned else dev(full))


@pytest.mark.parametrize("C,pad,mis", COPY_LADDER)
def test_cast_rows(C, pad, mis):
    L = _L()
    for rows in COPY_ROWS:
        x, xd = strided_src(rows, C, C + pad, rows + C + pad, mis)
        y, check = U.guarded((rows, C), BF16)
        assert L.sfron_cast_rows_bf16(p(xd), C + pad, rows, C, p(y), _sp()) == 0
        sync()
        check("cast_rows_bf16")
        assert bits_equal(y, U.cast_rows(x[:, :C])), f"cast_rows_bf16 rows={rows}: not the RNE cast"
    y, check = U.guarded((4, C), BF16)
    assert L.sfron_cast_rows_bf16(p(xd), C - 1, 4, C, p(y), _sp()) == ERR_ARG
    sync()
    U.untouched(check, "ldx < C")


@pytest.mark.parametrize("C,pad,mis", COPY_LADDER)
def test_copy_cols(C, pad, mis):
    L = _L()
    ldy = C + (8 if (C + pad) % 4 == 0 and C % 4 == 0 else 3)
    for rows in COPY_ROWS:
        x, xd = strided_src(rows, C, C + pad, 3 * rows + C + pad, mis)
        y0 = torch.randn(rows, C, generator=torch.Generator().manual_seed(rows + C))
        for acc in (0, 1):
            y, check = U.guarded((rows, C), F32, ld=ldy)
            if acc:
                y.copy_(y0)
            assert L.sfron_copy_cols(p(xd), C + pad, rows, C, p(y), ldy, acc, _sp()) == 0
            sync()
            check(f"copy_cols acc={acc}")                        # the columns C .. ldy - 1 of y are guard elements
            assert bits_equal(y, y0 + x[:, :C] if acc else x[:, :C].clone()), f"copy_cols rows={rows} accumulate={acc}"
    y, check = U.guarded((4, C), F32, ld=ldy)
    assert L.sfron_copy_cols(p(xd), C - 1, 4, C, p(y), ldy, 0, _sp()) == ERR_ARG
    assert L.sfron_copy_cols(p(xd), C + pad, 4, C, p(y), C - 1, 0, _sp()) == ERR_ARG
    sync()
    U.untouched(check, "ld < C")


@pytest.mark.parametrize("ld1_extra", [0, 1])          # 1: ldx1 % 4 != 0 -> the two plain launches, the same result
@pytest.mark.parametrize("rows", [7, 4101])
def test_copy_cols2(rows, ld1_extra):
    L = _L()
    C0, C1 = 260, 8
    x0, x0d = strided_src(rows, C0, C0 + 4, rows, False)
    x1, x1d = strided_src(rows, C1, C1 + ld1_extra, rows + 1, False)
    g = torch.Generator().manual_seed(rows)
    y00, y10 = torch.randn(rows, C0, generator=g), torch.randn(rows, C1, generator=g)
    for acc0, acc1 in ((0, 1), (1, 0)):
        # the two column halves of ONE concatenated destination [rows][C0 + C1 + 4]
        ld = C0 + C1 + 4
        y, check = U.guarded((rows, C0 + C1), F32, ld=ld)
        y[:, :C0].copy_(y00)
        y[:, C0:].copy_(y10)
        assert L.sfron_copy_cols2(p(x0d), C0 + 4, C0, p(y), ld, acc0, p(x1d), C1 + ld1_extra, C1, p(y) + 4 * C0, ld, acc1, rows, _sp()) == 0
        sync()
        check("copy_cols2")
        want = torch.cat([y00 + x0[:, :C0] if acc0 else x0[:, :C0], y10 + x1[:, :C1] if acc1 else x1[:, :C1]], 1)
        assert bits_equal(y, want), f"copy_cols2 accumulate = ({acc0}, {acc1})"
    y, check = U.guarded((rows, C0 + C1), F32)
    assert L.sfron_copy_cols2(p(x0d), C0 - 1, C0, p(y), C0 + C1, 0, p(x1d), C1 + ld1_extra, C1, p(y) + 4 * C0, C0 + C1, 0, rows, _sp()) == ERR_ARG
    assert L.sfron_copy_cols2(p(x0d), C0 + 4, C0, p(y), C0 + C1, 0, p(x1d), C1 + ld1_extra, C1, p(y) + 4 * C0, C0 + C1, 0, 0, _sp()) == ERR_ARG
    sync()
    U.untouched(check, "refused copy_cols2")


def test_cast_rows_colsum():
    L = _L()
    rows, C, ldx, maxp = 100, 260, 264, 64
    x, xd = strided_src(rows, C, ldx, 5, False)
    y, c_y = U.guarded((rows, C), BF16)
    part, c_part = U.guarded((maxp, C), F32)
    col, c_col = U.guarded((C,), F32)
    assert L.sfron_cast_rows_colsum(p(xd), ldx, rows, C, p(y), p(part), maxp, p(col), _sp()) == 0
    sync()
    for c in (c_y, c_part, c_col):
        c("cast_rows_colsum")
    assert bits_equal(y, U.cast_rows(x[:, :C]))
    U.bound32(col, x[:, :C].double().sum(0), x[:, :C].sum(0), "cast_rows_colsum.colsum")
    y2, c_y2 = U.guarded((rows, C), BF16)
    assert L.sfron_cast_rows_colsum(p(xd), ldx + 1, rows, C, p(y2), p(part), maxp, p(col), _sp()) == ERR_ARG      # no scalar twin: refused
    sync()
    U.untouched(c_y2, "cast_rows_colsum at ldx % 4 != 0")


# ================================================================================================ g. small pieces
@pytest.mark.parametrize("n", [1, 257, 4096 * 256 + 1])
def test_axpby(n):
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    s = 7.5
    out, check = U.guarded((n,), F32)
    assert _L().sfron_axpby(p(dev(a)), p(dev(b)), 1 + s, -s, n, p(out), _sp()) == 0
    sync()
    check("axpby")
    assert bits_equal(out, U.axpby(a, b, 1 + s, -s)), "axpby is not two rounded products and one rounded sum"


@pytest.mark.parametrize("B,HW,C,ld,scratch", [(2, 5, 3, 3, False), (2, 64, 70, 72, True), (2, 64, 70, 72, False)])
def test_sample_colsum(B, HW, C, ld, scratch):
    g = torch.Generator().manual_seed(HW + C)
    x = torch.full((B * HW, ld), 1e6)
    x[:, :C] = torch.randn(B * HW, C, generator=g) + 0.25
    out, c_out = U.guarded((B, C), F32, ld=C + 2)
    ws, c_ws = U.guarded((B * 32 * C,), F32)
    assert _L().sfron_sample_colsum(p(dev(x)), ld, B, HW, C, p(out), C + 2, p(ws) if scratch else None, B * 32 * C if scratch else 0, _sp()) == 0
    sync()
    c_out("sample_colsum")
    c_ws("sample_colsum scratch")
    U.bound32(out, U.sample_colsum(x[:, :C], B, HW, F64), U.sample_colsum(x[:, :C], B, HW, F32), "sample_colsum")


def test_pool2_sum():
    B, H, W, C = 2, 3, 5, 7
    g = torch.Generator().manual_seed(2)
    dy, dx0 = torch.randn(B, 2 * H, 2 * W, C, generator=g), torch.randn(B, H, W, C, generator=g)
    for acc in (0, 1):
        dx, check = U.guarded((B, H, W, C), F32)
        if acc:
            dx.copy_(dx0)
        assert _L().sfron_pool2_sum(p(dev(dy)), B, H, W, C, p(dx), acc, _sp()) == 0
        sync()
        check("pool2_sum")
        add64, add32 = (dx0.double(), dx0) if acc else (0.0, 0.0)
        U.bound32(dx, U.pool2_sum(dy, F64) + add64, U.pool2_sum(dy, F32) + add32, "pool2_sum")


# ================================================================================================ h. dropout masks
SEED0, SEED1 = 0x0123456789ABCDEF, 0xFEDCBA9876543210
KEYS = [(SEED0, 3, 0), (SEED1, 3, 0), (SEED0, 11, 0), (SEED0, 3, 5), (SEED1, 11, 5)]         # (seed, salt, counter)


def run_mask(seed, salt, counter, n, prob):
    ctr = torch.tensor([counter], dtype=torch.int64, device=DEV)
    m, check = U.guarded((n,), torch.uint8)
    assert _L().sfron_dropout_mask(seed, p(ctr), salt, n, prob, p(m), _sp()) == 0
    sync()
    check(f"dropout_mask n={n}")
    return m.cpu()


@pytest.mark.parametrize("prob", [0.0, 0.1, 0.5, 0.999])
def test_dropout_mask(prob):
    seen = []
    for n in (1, 3, 4, 5, 1001):
        for seed, salt, counter in KEYS:
            got = run_mask(seed, salt, counter, n, prob)
            assert torch.equal(got, U.dropout_mask(seed, counter, salt, n, prob)), (n, hex(seed), salt, counter, prob)
            if n == 1001:
                seen.append(got)
    if prob == 0.0:
        assert all(bool(m.all()) for m in seen)
    elif prob < 0.9:
        assert all(not torch.equal(seen[0], m) for m in seen[1:]), "seed, salt and counter must each change the draw"
    n = 4 * 4096 * 256 + 3                     # the grid-stride trip and a ragged last quad
    seed, salt, counter = KEYS[-1]
    assert torch.equal(run_mask(seed, salt, counter, n, prob), U.dropout_mask(seed, counter, salt, n, prob)), (n, prob)


def test_dropout_mask_batch():
    L = _L()
    sizes, salts = (4, 7, 1001, 70001), (3, 11, 2 ** 40 + 1, 5)
    offs, at = [], 0
    for n in sizes:
        offs.append(at)
        at += (n + 3) // 4 * 4 + 4              # at least 4 pad bytes behind every item
    items = dev(torch.tensor([[s, n, o] for s, n, o in zip(salts, sizes, offs)], dtype=torch.int64))
    for prob, counter in ((0.1, 0), (0.5, 5)):
        ctr = torch.tensor([counter], dtype=torch.int64, device=DEV)
        buf, check = U.guarded((at,), torch.uint8)
        assert L.sfron_dropout_mask_batch(SEED1, p(ctr), p(items), len(sizes), max(sizes), prob, p(buf), _sp()) == 0
        sync()
        check("dropout_mask_batch")
        host = buf.cpu()
        pad = torch.ones(at, dtype=torch.bool)
        for s, n, o in zip(salts, sizes, offs):
            assert torch.equal(host[o:o + n], U.dropout_mask(SEED1, counter, s, n, prob)), f"item of {n} bytes"
            assert torch.equal(host[o:o + n], run_mask(SEED1, s, counter, n, prob))
            pad[o:o + n] = False
        assert bool((host[pad] == check.sentinel).all()), "pad bytes between the items were written"


def test_dropout_mask_refusals():
    L = _L()
    ctr = torch.zeros(1, dtype=torch.int64, device=DEV)
    m, check = U.guarded((64,), torch.uint8)
    items = dev(torch.tensor([[1, 8, 0]], dtype=torch.int64))
    for n, prob, ptr in ((0, 0.5, p(m)), (8, 1.0, p(m)), (8, -0.1, p(m)), (8, 0.5, p(m) + 1)):
        assert L.sfron_dropout_mask(SEED0, p(ctr), 1, n, prob, ptr, _sp()) == ERR_ARG
        assert L.sfron_dropout_mask_batch(SEED0, p(ctr), p(items), 1, n, prob, ptr, _sp()) == ERR_ARG
    assert L.sfron_dropout_mask_batch(SEED0, p(ctr), p(items), 0, 8, 0.5, p(m), _sp()) == ERR_ARG
    sync()
    U.untouched(check, "refused dropout call")


# ================================================================================================ i. DDPM conditioning
@pytest.mark.parametrize("dim", U.TEMB_DIMS)
def test_ddpm_timestep_embed(dim):
    L = _L()
    t = torch.tensor(U.TEMB_T_SMALL + U.TEMB_T_LARGE)
    n = t.numel()
    out, check = U.guarded((n, dim), BF16)
    assert L.sfron_ddpm_timestep_embed(p(dev(t)), n, dim, p(out), _sp()) == 0
    sync()
    check("ddpm_timestep_embed")
    mask = (t <= 7)[:, None].expand(-1, dim)            # the cap on the small timesteps only; the others get the error bound
    U.bound_bf16(out, U.ddpm_timestep_embed(t, dim, F64), U.ddpm_timestep_embed(t, dim, F32), "ddpm_timestep_embed", cap_mask=mask)
    if dim % 2:
        assert bool((out.cpu()[:, -1].view(torch.int16) == 0).all()), "the last column of an odd dim is not +0"
    for bad in (3, 2, 0):
        spare, c_spare = U.guarded((n, 4), BF16)
        assert L.sfron_ddpm_timestep_embed(p(dev(t)), n, bad, p(spare), _sp()) == ERR_ARG
        sync()
        U.untouched(c_spare, "dim < 4")


NC = 10


@pytest.mark.parametrize("D", [1, 300, 512])
@pytest.mark.parametrize("n", [1, 9])
def test_class_embed(n, D):
    L = _L()
    g = torch.Generator().manual_seed(n * 1009 + D)
    table, null = torch.randn(NC, D, generator=g), torch.randn(D, generator=g)
    label_sets = [torch.tensor([3, 3, -1, NC, 0, 9, 5, 3, 2])] if n == 9 else [torch.tensor([7]), torch.tensor([-1]), torch.tensor([NC])]
    keep_given = torch.tensor([1, 0, 1, 1, 1, 1, 0, 1, 1], dtype=torch.uint8)[:n] if n == 9 else torch.tensor([0], dtype=torch.uint8)
    d = torch.randn(n, D, generator=g)
    t0 = torch.randn(NC, D, generator=g)                # the backward adds onto a non-zero d_table
    td, nd, dd = dev(table), dev(null), dev(d)
    for c in label_sets:
        for keep in (None, keep_given):
            cd, kd = dev(c), dev(keep) if keep is not None else None
            out, c_out = U.guarded((n, D), BF16)
            assert L.sfron_class_embed_fwd(p(td), p(nd), p(cd), p(kd), NC, n, D, p(out), _sp()) == 0
            d_tab, c_dt = U.guarded((NC, D), F32)
            d_tab.copy_(t0)
            d_null, c_dn = U.guarded((D,), F32)
            d_null.fill_(777.0)                          # garbage that must be overwritten
            assert L.sfron_class_embed_bwd(p(dd), p(cd), p(kd), NC, n, D, p(d_tab), p(d_null), _sp()) == 0
            sync()
            for ck in (c_out, c_dt, c_dn):
                ck(f"class_embed n={n} D={D}")
            assert bits_equal(out, U.class_embed_fwd(table, null, c, keep, NC).to(BF16)), "class_embed_fwd is not bf16(table[c]) / bf16(null)"
            want_t, want_n = U.class_embed_bwd(d, c, keep, NC, t0, F32)
            assert bits_equal(d_tab, want_t), "class_embed_bwd: d_table is not the serial fp32 accumulation over the batch"
            assert bits_equal(d_null, want_n), "class_embed_bwd: d_null"
    out, c_out = U.guarded((n, D), BF16)
    assert L.sfron_class_embed_fwd(None, p(nd), p(cd), None, NC, n, D, p(out), _sp()) == ERR_ARG
    assert L.sfron_class_embed_fwd(p(td), None, p(cd), None, NC, n, D, p(out), _sp()) == ERR_ARG
    sync()
    U.untouched(c_out, "refused class_embed call")
