"""GPU: GroupNorm (+ swish) (+ dropout) forward and backward (csrc/groupnorm.hip), every kernel family and sub-form at the smallest shape
that reaches it, through the C ABI, against the restatements of tests/groupnorm_ref.py: y and the bf16 form of dx under bound_bf16, dx, the
per-sample parameter-gradient partials and the column sums under bound32 (the yardstick is the float32 CPU evaluation of the same
expression -- with serial sums over the pixels -- never the kernel), mean and rstd within the statistics tolerances the suite already uses
(tests/test_gpu_large_shapes.py: 1e-6 rtol + atol, 1e-4 rtol).  Every output, and the scratch, lives in a guarded() buffer whose sentinels
are checked after the call; operands with padded row strides carry NaN in their gap columns.

Which form a case reaches is decided by the restated rule of tests/groupnorm_ref.py (the class in each case's name), which
tests/test_groupnorm_ref_cpu.py holds to the library's own host functions; here every case asserts sfron_groupnorm_one_launch and
sfron_groupnorm_chunks against it.

  k_gn3_fwd / k_gn3_bwd <false>   8 groups per workgroup, 128 KB rule: 48x9x64 (256 row replicas, 9 rows), 48x25x1280 (12 replicas, 64 idle
                                  threads), 24x25x128 in 64 groups, 64x1024x128 (slab exactly 128 KB); 4 groups: 24x529x256, 64x9x48 in 12
                                  groups, 64x1025x128 (one pixel over the line); 2 groups: 12x529x512; 1 group: 6x529x1024, 192x9x16 in one
                                  group; 8 groups under the 512 KB rule: 48x729x384
  k_gn3_fwd / k_gn3_bwd <true>    test_src_forms_equal_finish_then_plain: one case of each of those five classes, 1 / 4 / 5 slabs
  k_gn2_stats / _apply,           47x9x64 (one workgroup short of the one-launch form), 3x9x64 (1 chunk), 3x100x320 (12 uneven chunks: the
  k_gn2_bwd_stats / _bwd_apply    8 + 4 partials loop), 3x1000x128 (32 chunks that do not divide HW), 3x72x2048 (the widest bwd_cast),
                                  2x25x4096 (64 KB of LDS), 3x25x64 in 64 groups, 3x9x4 and 3x9x256 in one group, 2x25x96 (3 channels per
                                  group: quads straddle groups)
  k_gn_fwd / k_gn_bwd             NULL scratch (48x9x64, 3x100x320, 3x9x256 in one group: one slot, 2x25x96: 85 slots and an idle thread),
                                  C % 4 != 0 (2x25x30 in 3 groups), 128 groups, C = 4128, ldx % 4 != 0, x 4 bytes off a 16-byte line

Every backward case runs: (A) swish, mask, a fresh dx -- twice, for identical bits, and as sfron_groupnorm_bwd_cast, whose bf16 operand must
be the rounding of (A)'s dx bit for bit with identical partials, whose column partials hold the sample's sum in chunk 0 and exact zeros in the
others under the one-launch form, and whose sums over the chunks are held to float64; (B) no swish, no mask, accumulate onto a non-zero dx
with ldx = C + 8, lddx = C + 12 and extra at ld_extra = C + 4, also as sfron_copy_cols + sfron_groupnorm_bwd(accumulate = 1), bit for bit;
(C) extra 4 bytes off a 16-byte line (the sfron_copy_cols fallback), accumulate = 0; (I) integer dy with a mask of scale 2 and no swish:
part_beta must equal the exact integer sums bit for bit -- a dropped or doubled pixel row cannot hide inside a tolerance.

Fixed with this module: sfron_groupnorm_bwd_res, _bwd_cast, _bwd_res_src and _bwd_cast_src now refuse ldx < C (and lddx < C where there is
a dx) with SFRON_ERR_ARG before any launch, as sfron_groupnorm_fwd always did (test_refusals).

Measured on an MI355X (RECORD prints the current figures at teardown, pytest -s).  Shares: elements that differ from bf16(ref64), cap
2e-3; ratios: max|got - ref64| over the float32 restatement's own error, bound 4 (+ 4 ulps of the largest value), largest over the
configurations A, B, C, I:
  class     y share   dx16 share   dx     part_gamma   part_beta   column sums
  gn3.8     1.1e-4    1.2e-4       1.03   1.27         1.00        1.18
  gn3.4     7.2e-5    1.1e-4       1.00   0.93         1.00        1.13
  gn3.2     2.9e-5    1.0e-4       0.62   0.50         0.50        0.47
  gn3.1     3.6e-5    1.8e-4       1.11   1.11         1.00        1.37
  gn3.8w    2.5e-5    9.0e-5       0.66   0.35         0.31        0.34
  gn2       5.0e-5    2.1e-4       1.21   1.23         1.18        1.32
  gn1       1.1e-4    -            1.21   1.02         1.00        -
Largest error over bound of a bf16 output (`excess`): 0.995.  part_beta of configuration I: 0 ulps in every class."""
import ctypes
import functools

import pytest
import torch

import groupnorm_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG, ERR_UNSUPPORTED = 1001, 1002          # csrc/common.h
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
NAN = float("nan")
BIG = 4 << 20                                  # elements: above this a case runs the configurations the issue asks for and no more


def _L():
    from sfron import _lib
    return _lib.lib()


def _sp():
    from sfron._lib import stream_ptr
    return stream_ptr()


def p(t):
    return t.data_ptr() if t is not None else None


def sync():
    torch.cuda.synchronize()


def dev(t):
    return t.contiguous().to(DEV)


def rows_in(t, ld, mis=False):
    """a [rows][C] input on the device with its rows `ld` elements apart, NaN in the gap columns; mis: 4 bytes past a 16-byte line"""
    rows, C = t.shape
    off = 1 if mis else 0
    buf = torch.full((rows * ld + 4,), NAN, dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + rows * ld].view(rows, ld)[:, :C]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
    """a launch that faulted leaves the device context unusable: end the session there instead of launching the remaining cases on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault in tests/test_gpu_groupnorm.py: {e}", returncode=3)


@pytest.fixture(scope="module", autouse=True)
def _print_record():
    yield
    print()
    for name in sorted(G.RECORD):
        print("RECORD", name, " ".join(f"{k}={v:.4g}" for k, v in sorted(G.RECORD[name].items())))


# ================================================================================================ device operands of a case
class Ops:
    """the device operands of one case and variant: x dense (rows C + ldx_pad apart, misaligned when the case says so) and strided (8 more),
    dy, the mask, dx0, extra at ld C + 4 and 4 bytes off a line, the float64 statistics rounded to float32, and the scratch"""

    def __init__(self, c, variant="randn"):
        self.c, self.i = c, G.gn_inputs(c, variant)
        i = self.i
        B, HW, C = c.B, c.HW, c.C
        self.rows = rows = B * HW
        flat = lambda t: t.reshape(rows, C)
        self.ldx, self.ldxs = C + c.ldx_pad, C + c.ldx_pad + 8
        self.x, self.xs = rows_in(flat(i["x"]), self.ldx, c.x_mis), rows_in(flat(i["x"]), self.ldxs, c.x_mis)
        self.gamma, self.beta = dev(i["gamma"]), dev(i["beta"])
        self.dy, self.mask, self.scale = dev(flat(i["dy"])), dev(flat(i["mask"])), i["scale"]
        self.dx0 = dev(flat(i["dx0"]))
        self.extra = rows_in(flat(i["extra"]), C + 4)
        self.extra_mis = rows_in(flat(i["extra"]), C, mis=True) if rows * C <= BIG else None
        m64, r64, _ = G._stats(i["x"], c.groups, G.EPS, F64)
        self.mean, self.rstd = dev(m64.float().reshape(-1)), dev(r64.float().reshape(-1))
        self.ws, self.c_ws = (G.guarded((G.scratch_bytes(B, HW, C, c.groups),), torch.uint8) if c.scratch else (None, None))
        self.nch = G.gn_chunks(B, HW)

    def check_ws(self, what):
        if self.c_ws is not None:
            self.c_ws(what + ": scratch")


@functools.lru_cache(maxsize=2)
def ops(c, variant="randn"):
    return Ops(c, variant)


def assert_class(c):
    L = _L()
    assert G.classify(c) == c.cls
    assert L.sfron_groupnorm_one_launch(c.B, c.HW, c.C, c.groups) == G.one_launch(c.B, c.HW, c.C, c.groups)
    if c.cls != "gn1":
        assert bool(G.one_launch(c.B, c.HW, c.C, c.groups)) == c.cls.startswith("gn3")
    assert L.sfron_groupnorm_chunks(c.B, c.HW) == G.gn_chunks(c.B, c.HW)
    assert L.sfron_groupnorm_scratch_bytes(c.B, c.HW, c.C, c.groups) == G.scratch_bytes(c.B, c.HW, c.C, c.groups)


# ================================================================================================ forward
def run_fwd(o, swish, masked, strided=False):
    c = o.c
    x, ldx = (o.xs, o.ldxs) if strided else (o.x, o.ldx)
    y, c_y = G.guarded((o.rows, c.C), BF16)
    mean, c_m = G.guarded((c.B * c.groups,), F32)
    rstd, c_r = G.guarded((c.B * c.groups,), F32)
    st = _L().sfron_groupnorm_fwd(p(x), ldx, p(o.gamma), p(o.beta), c.B, c.HW, c.C, c.groups, G.EPS, swish, p(o.mask) if masked else None,
                                  o.scale if masked else 1.0, p(y), p(mean), p(rstd), p(o.ws), _sp())
    assert st == 0, st
    sync()
    what = f"groupnorm_fwd {c.name} swish={swish} mask={masked} strided={strided}"
    for chk in (c_y, c_m, c_r):
        chk(what)
    o.check_ws(what)
    return y, mean, rstd


def fwd_refs(o, swish, masked):
    i, c = o.i, o.c
    mask, scale = (i["mask"], i["scale"]) if masked else (None, 1.0)
    return [G.groupnorm_fwd(i["x"], i["gamma"], i["beta"], c.groups, G.EPS, swish, mask, scale, dt) for dt in (F64, F32)]


def check_fwd(c, got, r64, r32):
    y, mean, rstd = got
    G.bound_bf16(y.view(c.B, c.HW, c.C), r64[0], r32[0], c.cls + ".y")
    G.stat_close(mean, r64[1], 1e-6, 1e-6, c.name + " mean")
    G.stat_close(rstd, r64[2], 1e-4, 0.0, c.name + " rstd")


@pytest.mark.parametrize("c", G.GPU_CASES, ids=lambda c: c.name)
def test_forward(c):
    assert_class(c)
    o = ops(c)
    for swish in (0, 1):
        for masked in (0, 1):
            r64, r32 = fwd_refs(o, swish, masked)
            got = run_fwd(o, swish, masked)
            check_fwd(c, got, r64, r32)
            if swish and masked:
                for strided in (0, 1):                       # the same bits again, and with x rows 8 elements further apart
                    again = run_fwd(o, swish, masked, strided=bool(strided))
                    for name, a, b in zip(("y", "mean", "rstd"), got, again):
                        assert bits_equal(a, b), f"{c.name}: {name} differs between two runs (strided x: {strided})"


@pytest.mark.parametrize("c", G.CONST_CASES, ids=lambda c: c.name)
def test_forward_constant_group(c):
    """one group of one sample constant: variance 0, rstd = eps^-1/2 = 1000, xhat = 0 and y = bf16(act(beta)) (* mask * scale) exactly"""
    o = ops(c, "const")
    b, g = o.i["const"]
    cg = c.C // c.groups
    for swish in (0, 1):
        for masked in (0, 1):
            r64, r32 = fwd_refs(o, swish, masked)
            y, mean, rstd = got = run_fwd(o, swish, masked)
            check_fwd(c, got, r64, r32)
            yg = y.view(c.B, c.HW, c.C)[b, :, g * cg:(g + 1) * cg].cpu()
            assert torch.equal(yg, G.to_bf16(r64[0][b, :, g * cg:(g + 1) * cg])), f"{c.name} swish={swish} mask={masked}: y of the constant group"
            if not masked:
                be = o.i["beta"][g * cg:(g + 1) * cg].double()
                assert torch.equal(yg, G.to_bf16(be / (1.0 + torch.exp(-be)) if swish else be).expand(c.HW, cg))
            assert abs(float(rstd.view(c.B, c.groups)[b, g]) - 1000.0) <= 1e-4 * 1000.0
            assert float(mean.view(c.B, c.groups)[b, g]) == 0.75


# ================================================================================================ backward
def run_bwd(o, swish, masked, acc, extra=None, strided=False, entry="res", dx_in=None):
    """extra: None | "given" (ld_extra = C + 4) | "mis" (4 bytes off a 16-byte line).  acc = 0: dx starts as NaN sentinels"""
    c, L = o.c, _L()
    x, ldx = (o.xs, o.ldxs) if strided else (o.x, o.ldx)
    lddx = c.C + (12 if strided else 0)
    dx, c_dx = G.guarded((o.rows, c.C), F32, ld=lddx)
    if acc:
        dx.copy_(o.dx0 if dx_in is None else dx_in)
    pg, c_pg = G.guarded((c.B, c.C), F32)
    pb, c_pb = G.guarded((c.B, c.C), F32)
    ex, ldex = {None: (None, 0), "given": (o.extra, c.C + 4), "mis": (o.extra_mis, c.C)}[extra]
    mask, scale = (p(o.mask), o.scale) if masked else (None, 1.0)
    if entry == "res":
        st = L.sfron_groupnorm_bwd_res(p(o.dy), p(x), ldx, p(o.gamma), p(o.beta), p(o.mean), p(o.rstd), c.B, c.HW, c.C, c.groups, swish, mask, scale,
                                       p(dx), lddx, acc, p(ex), ldex, p(pg), p(pb), p(o.ws), _sp())
    else:
        assert ex is None
        st = L.sfron_groupnorm_bwd(p(o.dy), p(x), ldx, p(o.gamma), p(o.beta), p(o.mean), p(o.rstd), c.B, c.HW, c.C, c.groups, swish, mask, scale,
                                   p(dx), lddx, acc, p(pg), p(pb), p(o.ws), _sp())
    assert st == 0, st
    sync()
    what = f"groupnorm_bwd {c.name} swish={swish} mask={masked} acc={acc} extra={extra} strided={strided}"
    for chk in (c_dx, c_pg, c_pb):
        chk(what)
    o.check_ws(what)
    return dx, pg, pb


def run_cast(o, swish, masked, strided=False, expect=0):
    c, L = o.c, _L()
    x, ldx = (o.xs, o.ldxs) if strided else (o.x, o.ldx)
    d16, c_16 = G.guarded((o.rows, c.C), BF16)
    cp, c_cp = G.guarded((c.B * o.nch, c.C), F32)
    pg, c_pg = G.guarded((c.B, c.C), F32)
    pb, c_pb = G.guarded((c.B, c.C), F32)
    mask, scale = (p(o.mask), o.scale) if masked else (None, 1.0)
    st = L.sfron_groupnorm_bwd_cast(p(o.dy), p(x), ldx, p(o.gamma), p(o.beta), p(o.mean), p(o.rstd), c.B, c.HW, c.C, c.groups, swish, mask, scale,
                                    p(d16), p(cp), p(pg), p(pb), p(o.ws), _sp())
    assert st == expect, st
    sync()
    what = f"groupnorm_bwd_cast {c.name} strided={strided}"
    for chk in (c_16, c_cp, c_pg, c_pb):
        if expect:
            G.untouched(chk, what)
        else:
            chk(what)
    o.check_ws(what)
    return d16, cp, pg, pb


def bwd_refs(o, swish, masked, acc, extra):
    i, c = o.i, o.c
    mask, scale = (i["mask"], i["scale"]) if masked else (None, 1.0)
    return [G.groupnorm_bwd(i["dy"], i["x"], i["gamma"], i["beta"], c.groups, G.EPS, swish, mask, scale, i["dx0"], acc, i["extra"] if extra else None, dt)
            for dt in (F64, F32)]


def check_bwd(c, got, w64, w32, tag):
    dx, pg, pb = got
    G.bound32(dx.reshape(c.B, c.HW, c.C), w64.dx, w32.dx, f"{c.cls}.{tag}.dx")
    G.bound32(pg, w64.pg, w32.pg, f"{c.cls}.{tag}.part_gamma")
    G.bound32(pb, w64.pb, w32.pb, f"{c.cls}.{tag}.part_beta")


@pytest.mark.parametrize("c", G.GPU_CASES, ids=lambda c: c.name)
def test_backward(c):
    assert_class(c)
    assert G.classify(c, ldx_more=8, lddx_more=12) == c.cls          # the padded strides of (B) stay in the same form
    o = ops(c)
    small = o.rows * c.C <= BIG
    # ---- (A) swish, mask, a fresh dx; twice; the bf16 operand form
    w64, w32 = bwd_refs(o, 1, 1, 0, False)
    a = run_bwd(o, 1, 1, 0, entry="plain")
    check_bwd(c, a, w64, w32, "A")
    for name, u, v in zip(("dx", "part_gamma", "part_beta"), a, run_bwd(o, 1, 1, 0)):
        assert bits_equal(u, v), f"{c.name}: {name} differs between two runs"
    cast_ok = bool(c.scratch and not c.x_mis and G.bwd_cast_ok(o.ldx, c.C, c.groups))
    assert cast_ok == (c.cls != "gn1" and c.C <= 2048)
    if cast_ok:
        d16, cp, pg, pb = run_cast(o, 1, 1)
        assert bits_equal(d16, a[0].to(BF16)), f"{c.name}: the bf16 operand is not the rounding of sfron_groupnorm_bwd's dx"
        assert bits_equal(pg, a[1]) and bits_equal(pb, a[2]), f"{c.name}: bwd_cast's parameter-gradient partials differ from bwd's"
        G.bound_bf16(d16.view(c.B, c.HW, c.C), w64.dx, w32.dx, c.cls + ".A.dx16")
        cp3 = cp.view(c.B, o.nch, c.C)
        G.bound32(cp3.double().sum(1), w64.colsum, w32.colsum, c.cls + ".A.colsum")
        if c.cls.startswith("gn3"):
            assert bool((cp3[:, 1:] == 0).all()) and not bool(torch.signbit(cp3[:, 1:]).any()), f"{c.name}: chunks 1.. of the column partials"
            G.bound32(cp3[:, 0], w64.colsum, w32.colsum, c.cls + ".A.colsum")
        for name, u, v in zip(("dx16", "col_partials", "part_gamma", "part_beta"), (d16, cp, pg, pb), run_cast(o, 1, 1, strided=True)):
            assert bits_equal(u, v), f"{c.name}: bwd_cast {name} differs with x rows 8 elements further apart"
    else:
        run_cast(o, 1, 1, expect=ERR_ARG)
    del w64, w32
    # ---- (B) no swish, no mask, accumulate, padded strides, extra; = copy_cols + bwd(accumulate = 1)
    w64, w32 = bwd_refs(o, 0, 0, 1, True)
    b = run_bwd(o, 0, 0, 1, extra="given", strided=True)
    check_bwd(c, b, w64, w32, "B")
    step, c_step = G.guarded((o.rows, c.C), F32, ld=c.C + 12)
    step.copy_(o.dx0)
    assert _L().sfron_copy_cols(p(o.extra), c.C + 4, o.rows, c.C, p(step), c.C + 12, 1, _sp()) == 0
    sync()
    c_step("copy_cols before groupnorm_bwd")
    two = run_bwd(o, 0, 0, 1, strided=True, entry="plain", dx_in=step)
    for name, u, v in zip(("dx", "part_gamma", "part_beta"), b, two):
        assert bits_equal(u, v), f"{c.name}: {name}: sfron_groupnorm_bwd_res differs from copy_cols + sfron_groupnorm_bwd(accumulate = 1)"
    del w64, w32
    # ---- (C) extra 4 bytes off a 16-byte line: copy_cols (accumulate = 0), then the kernel accumulates
    if small:
        w64, w32 = bwd_refs(o, 1, 1, 0, True)
        cc = run_bwd(o, 1, 1, 0, extra="mis")
        check_bwd(c, cc, w64, w32, "C")
        given = run_bwd(o, 1, 1, 0, extra="given")
        for name, u, v in zip(("dx", "part_gamma", "part_beta"), cc, given):
            assert bits_equal(u, v), f"{c.name}: {name}: the copy_cols fallback differs from the one-pass form"


@pytest.mark.parametrize("c", G.GPU_CASES, ids=lambda c: c.name)
def test_backward_integer_part_beta_is_exact(c):
    """dy small integers, the mask's scale 2, no swish: every dz is an integer, every partial sum of any order is exact in float32, so
    part_beta must be the exact sums bit for bit in all three families; dx and part_gamma under bound32 as usual"""
    o = ops(c, "int")
    w64, w32 = bwd_refs(o, 0, 1, 0, False)
    assert torch.equal(w64.pb, w64.pb.round()) and float((o.i["dy"].abs() * 2).sum(1).max()) < 2 ** 24
    got = run_bwd(o, 0, 1, 0)
    bad = got[2].cpu() != w64.pb.float()
    assert not bad.any(), f"{c.name}: {int(bad.sum())} of {bad.numel()} part_beta values are not the exact integer sums"
    check_bwd(c, got, w64, w32, "I")
    if c.scratch and not c.x_mis and G.bwd_cast_ok(o.ldx, c.C, c.groups):
        d16, cp, pg, pb = run_cast(o, 0, 1)
        assert bits_equal(pb, got[2]) and bits_equal(pg, got[1]) and bits_equal(d16, got[0].to(BF16))


# ================================================================================================ the _src forms
@pytest.mark.parametrize("c", G.SRC_CASES, ids=lambda c: c.name)
def test_src_forms_equal_finish_then_plain(c):
    """sfron_groupnorm_{fwd,bwd_res,bwd_cast}_src = sfron_split_finish followed by the plain entry point, bit for bit, at one case of every
    one-launch class, with 1, 4 and 5 slabs (the four-in-flight loop and its tail), with and without bias, per-sample vector and residual"""
    from sfron import _lib
    L = _L()
    assert_class(c)
    o = ops(c)
    B, HW, C, groups, rows = c.B, c.HW, c.C, c.groups, o.rows
    g = torch.Generator(device=DEV).manual_seed(C + HW)
    slabs = torch.randn(5, rows, C, generator=g, device=DEV) * 0.7
    bias, vec, resid = (torch.randn(C, generator=g, device=DEV), torch.randn(B, C + 8, generator=g, device=DEV),
                        torch.randn(rows, C, generator=g, device=DEV))     # sfron_split_finish: ld_resid == ld_out
    nch = o.nch
    for nsl in (1, 4, 5):
        for extras in (False, True):
            src = _lib.SplitSrc()
            src.slabs, src.n_slabs, src.slab_stride = slabs.data_ptr(), nsl, rows * C
            if extras:
                src.bias, src.sample_vec, src.ld_vec, src.resid, src.ld_resid = bias.data_ptr(), vec.data_ptr(), C + 8, resid.data_ptr(), C
            what = f"{c.name} slabs={nsl} extras={extras}"
            fin, c_fin = G.guarded((rows, C), F32)
            assert L.sfron_split_finish(ctypes.byref(src), rows, C, HW, p(fin), None, C, _sp()) == 0
            sync()
            c_fin("split_finish " + what)
            want = slabs[:nsl].double().sum(0)
            if extras:
                want = want + bias.double() + vec[:, :C].double().repeat_interleave(HW, 0) + resid.double()
            assert float((fin.double() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max())), "split_finish " + what
            del want
            # ---- forward: x = the finished tensor
            outs = []
            for form in ("plain", "src"):
                y, c_y = G.guarded((rows, C), BF16)
                mean, c_m = G.guarded((B * groups,), F32)
                rstd, c_r = G.guarded((B * groups,), F32)
                xw, c_x = G.guarded((rows, C), F32)
                if form == "plain":
                    st = L.sfron_groupnorm_fwd(p(fin), C, p(o.gamma), p(o.beta), B, HW, C, groups, G.EPS, 1, p(o.mask), o.scale, p(y), p(mean), p(rstd),
                                               p(o.ws), _sp())
                else:
                    st = L.sfron_groupnorm_fwd_src(ctypes.byref(src), p(xw), p(o.gamma), p(o.beta), B, HW, C, groups, G.EPS, 1, p(o.mask), o.scale, p(y),
                                                   p(mean), p(rstd), _sp())
                assert st == 0, (st, form, what)
                sync()
                for chk in (c_y, c_m, c_r, c_x):
                    chk(f"fwd {form} {what}")
                outs.append((fin if form == "plain" else xw, y, mean, rstd))
            for name, u, v in zip(("x", "y", "mean", "rstd"), *outs):
                assert bits_equal(u, v), f"fwd_src {what}: {name}"
            del outs
            # ---- backward: dy = the finished tensor; fp32 form with accumulate, extra and padded dx rows
            outs = []
            for form in ("plain", "src"):
                dx, c_dx = G.guarded((rows, C), F32, ld=C + 12)
                dx.copy_(o.dx0)
                pg, c_pg = G.guarded((B, C), F32)
                pb, c_pb = G.guarded((B, C), F32)
                dyw, c_dy = G.guarded((rows, C), F32)
                if form == "plain":
                    st = L.sfron_groupnorm_bwd_res(p(fin), p(o.xs), o.ldxs, p(o.gamma), p(o.beta), p(o.mean), p(o.rstd), B, HW, C, groups, 1, p(o.mask),
                                                   o.scale, p(dx), C + 12, 1, p(o.extra), C + 4, p(pg), p(pb), p(o.ws), _sp())
                else:
                    st = L.sfron_groupnorm_bwd_res_src(ctypes.byref(src), p(dyw), p(o.xs), o.ldxs, p(o.gamma), p(o.beta), p(o.mean), p(o.rstd), B, HW, C,
                                                       groups, 1, p(o.mask), o.scale, p(dx), C + 12, 1, p(o.extra), C + 4, p(pg), p(pb), _sp())
                assert st == 0, (st, form, what)
                sync()
                for chk in (c_dx, c_pg, c_pb, c_dy):
                    chk(f"bwd_res {form} {what}")
                outs.append((fin if form == "plain" else dyw, dx, pg, pb))
            for name, u, v in zip(("dy", "dx", "part_gamma", "part_beta"), *outs):
                assert bits_equal(u, v), f"bwd_res_src {what}: {name}"
            del outs
            # ---- backward, bf16 operand form
            outs = []
            for form in ("plain", "src"):
                d16, c_16 = G.guarded((rows, C), BF16)
                cp, c_cp = G.guarded((B * nch, C), F32)
                pg, c_pg = G.guarded((B, C), F32)
                pb, c_pb = G.guarded((B, C), F32)
                dyw, c_dy = G.guarded((rows, C), F32)
                if form == "plain":
                    st = L.sfron_groupnorm_bwd_cast(p(fin), p(o.x), o.ldx, p(o.gamma), p(o.beta), p(o.mean), p(o.rstd), B, HW, C, groups, 1, p(o.mask),
                                                    o.scale, p(d16), p(cp), p(pg), p(pb), p(o.ws), _sp())
                else:
                    st = L.sfron_groupnorm_bwd_cast_src(ctypes.byref(src), p(dyw), p(o.x), o.ldx, p(o.gamma), p(o.beta), p(o.mean), p(o.rstd), B, HW, C,
                                                        groups, 1, p(o.mask), o.scale, p(d16), p(cp), p(pg), p(pb), _sp())
                assert st == 0, (st, form, what)
                sync()
                for chk in (c_16, c_cp, c_pg, c_pb, c_dy):
                    chk(f"bwd_cast {form} {what}")
                outs.append((fin if form == "plain" else dyw, d16, cp, pg, pb))
            for name, u, v in zip(("dy", "dx16", "col_partials", "part_gamma", "part_beta"), *outs):
                assert bits_equal(u, v), f"bwd_cast_src {what}: {name}"
            del outs
            o.check_ws(what)


# ================================================================================================ refusals
def test_refusals():
    """SFRON_ERR_ARG (1001) before any launch for C % groups != 0, more than 256 channels per group, ldx < C, lddx < C, null pointers, and from
    bwd_cast for !bwd_cast_ok, a null scratch and misaligned pointers; SFRON_ERR_UNSUPPORTED (1002) from every _src form at a two-phase shape.
    Every output buffer still holds its sentinels afterwards.  The operands are sized for the largest shape a call claims."""
    from sfron import _lib
    L = _L()
    B, HW, C, G32 = 48, 9, 64, 32
    rows, wide = B * HW, 520
    z = lambda *s: torch.zeros(*s, device=DEV)
    x, dy, gamma, beta, mean, rstd, extra = z(rows * wide + 4), z(rows * wide + 4), z(wide), z(wide), z(B * 64), z(B * 64), z(rows * wide)
    mask = torch.ones(rows * wide, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(G.scratch_bytes(B, HW, wide, 64) // 8 + 2, dtype=F64, device=DEV)
    bufs = {k: G.guarded(s, dt) for k, (s, dt) in dict(y=((rows, wide), BF16), m=((B * 64,), F32), r=((B * 64,), F32), dx=((rows * wide + 4,), F32),
                                                      pg=((B, wide), F32), pb=((B, wide), F32), d16=((rows * wide + 4,), BF16),
                                                      cp=((B * 32, wide), F32), xw=((rows, wide), F32)).items()}
    y, m, r, dx, pg, pb, d16, cp, xw = (bufs[k][0] for k in ("y", "m", "r", "dx", "pg", "pb", "d16", "cp", "xw"))

    def fwd(x_=x, ldx=C, C_=C, groups=G32, ga=gamma, be=beta, y_=y, m_=m, r_=r, B_=B, HW_=HW):
        return L.sfron_groupnorm_fwd(p(x_), ldx, p(ga), p(be), B_, HW_, C_, groups, G.EPS, 1, p(mask), 1.5, p(y_), p(m_), p(r_), p(ws), _sp())

    def bwd(dy_=dy, x_=x, ldx=C, C_=C, groups=G32, ga=gamma, be=beta, m_=mean, r_=rstd, dx_=dx, lddx=C, ex=None, ldex=0, pg_=pg, pb_=pb, B_=B, HW_=HW):
        return L.sfron_groupnorm_bwd_res(p(dy_), p(x_), ldx, p(ga), p(be), p(m_), p(r_), B_, HW_, C_, groups, 1, p(mask), 1.5, p(dx_), lddx, 0, p(ex),
                                         ldex, p(pg_), p(pb_), p(ws), _sp())

    def cast(dy_=dy, x_=x, ldx=C, C_=C, groups=G32, ga=gamma, be=beta, m_=mean, r_=rstd, d16_=d16, cp_=cp, pg_=pg, pb_=pb, ws_=ws, B_=B, HW_=HW,
             mask_=mask):
        return L.sfron_groupnorm_bwd_cast(p(dy_), p(x_), ldx, p(ga), p(be), p(m_), p(r_), B_, HW_, C_, groups, 1, p(mask_), 1.5, p(d16_), p(cp_), p(pg_),
                                          p(pb_), p(ws_), _sp())

    bad_shapes = (dict(groups=5), dict(C_=516, ldx=516, groups=2), dict(ldx=C - 4), dict(B_=0), dict(HW_=0), dict(groups=0))
    for kw in bad_shapes:
        assert fwd(**kw) == ERR_ARG, ("fwd", kw)
        assert bwd(**kw) == ERR_ARG, ("bwd_res", kw)
        if "C_" not in kw:                       # the two-phase kernels bwd_cast runs have no channels-per-group limit of their own
            assert cast(**kw) == ERR_ARG, ("bwd_cast", kw)
    assert bwd(C_=516, ldx=516, lddx=516, groups=2) == ERR_ARG
    assert bwd(lddx=C - 4) == ERR_ARG and bwd(lddx=C - 1) == ERR_ARG and bwd(ldx=C - 1) == ERR_ARG and cast(ldx=C - 8) == ERR_ARG
    assert L.sfron_groupnorm_bwd(p(dy), p(x), C - 4, p(gamma), p(beta), p(mean), p(rstd), B, HW, C, G32, 1, None, 1.0, p(dx), C, 0, p(pg), p(pb), p(ws),
                                 _sp()) == ERR_ARG
    assert L.sfron_groupnorm_bwd(p(dy), p(x), C, p(gamma), p(beta), p(mean), p(rstd), B, HW, C, G32, 1, None, 1.0, p(dx), C - 4, 0, p(pg), p(pb), p(ws),
                                 _sp()) == ERR_ARG
    assert bwd(ex=extra, ldex=C - 4) == ERR_ARG and bwd(ex=dx, ldex=C) == ERR_ARG
    for k in ("x_", "ga", "be", "y_", "m_", "r_"):
        assert fwd(**{k: None}) == ERR_ARG, ("fwd null", k)
    for k in ("dy_", "x_", "ga", "be", "m_", "r_", "dx_", "pg_", "pb_"):
        assert bwd(**{k: None}) == ERR_ARG, ("bwd_res null", k)
    for k in ("dy_", "x_", "ga", "be", "m_", "r_", "d16_", "cp_", "pg_", "pb_", "ws_"):
        assert cast(**{k: None}) == ERR_ARG, ("bwd_cast null", k)
    # bwd_cast: !bwd_cast_ok (ldx % 4, C % 4, more than 64 groups, C > 2048 would need larger operands: the host function is held to the
    # restated rule on the CPU), misaligned x / dy / scratch (4 bytes), bf16 operand (2 bytes), mask (1 byte)
    assert cast(ldx=C + 2) == ERR_ARG and cast(C_=30, ldx=32, groups=3) == ERR_ARG and cast(C_=256, ldx=256, groups=128) == ERR_ARG
    assert cast(x_=x[1:]) == ERR_ARG and cast(dy_=dy[1:]) == ERR_ARG and cast(d16_=d16[1:]) == ERR_ARG and cast(mask_=mask[1:]) == ERR_ARG
    assert cast(ws_=ws.view(torch.float32)[1:]) == ERR_ARG
    # the _src forms: the same argument checks, and 1002 at a shape that takes the two-phase pair
    slabs = z(rows * C)
    src = _lib.SplitSrc()
    src.slabs, src.n_slabs, src.slab_stride = slabs.data_ptr(), 1, rows * C
    sref = ctypes.byref(src)

    def fwd_src(B_=B, C_=C, groups=G32, xw_=xw):
        return L.sfron_groupnorm_fwd_src(sref, p(xw_), p(gamma), p(beta), B_, HW, C_, groups, G.EPS, 1, None, 1.0, p(y), p(m), p(r), _sp())

    def res_src(B_=B, ldx=C, lddx=C, dyw=xw, dx_=dx):
        return L.sfron_groupnorm_bwd_res_src(sref, p(dyw), p(x), ldx, p(gamma), p(beta), p(mean), p(rstd), B_, HW, C, G32, 1, None, 1.0, p(dx_), lddx, 0, None,
                                             0, p(pg), p(pb), _sp())

    def cast_src(B_=B, ldx=C, dyw=xw):
        return L.sfron_groupnorm_bwd_cast_src(sref, p(dyw), p(x), ldx, p(gamma), p(beta), p(mean), p(rstd), B_, HW, C, G32, 1, None, 1.0, p(d16), p(cp), p(pg),
                                              p(pb), _sp())

    assert G.one_launch(B, HW, C, G32) == 1 and G.one_launch(3, HW, C, G32) == 0
    assert fwd_src(B_=3) == ERR_UNSUPPORTED and res_src(B_=3) == ERR_UNSUPPORTED and cast_src(B_=3) == ERR_UNSUPPORTED
    assert fwd_src(groups=5) == ERR_ARG and fwd_src(xw_=None) == ERR_ARG
    for kw in (dict(ldx=C - 4), dict(lddx=C - 4), dict(dx_=None), dict(dyw=None), dict(ldx=C + 2), dict(lddx=C + 2)):
        assert res_src(**kw) == ERR_ARG, ("bwd_res_src", kw)
        assert res_src(B_=3, **kw) == ERR_ARG, ("bwd_res_src at a two-phase shape", kw)
    for kw in (dict(ldx=C - 4), dict(dyw=None), dict(ldx=C + 2)):
        assert cast_src(**kw) == ERR_ARG, ("bwd_cast_src", kw)
    src.slabs = None
    assert fwd_src() == ERR_ARG and res_src() == ERR_ARG and cast_src() == ERR_ARG
    sync()
    for k, (_, chk) in bufs.items():
        G.untouched(chk, f"refused GroupNorm calls: {k}")
    assert float(ws.abs().max()) == 0.0
