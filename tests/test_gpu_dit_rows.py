"""GPU: the adaLN row, reduction and conditioning kernels of the DiT block (csrc/norm.hip, csrc/embed.hip, k_ln_mod_fwd_q in
csrc/fp8.hip), every dispatch form at the smallest shape that reaches it, through the C ABI, against the float64 restatements of
tests/dit_rows_ref.py under its bounds (bound32 / bound_bf16 / check_e4m3: the yardstick is the float32 CPU evaluation of the same
expression, never the kernel).  Every output lives in a guarded() buffer whose sentinels are checked after every call; B = 3 samples with
their own shift / scale / gate rows unless the form needs more rows.

Forms reached, and the shape that reaches each ((B, T, D), M = B T rows):
  k_ln_mod_fwd<1>, k_ln_mod_fwd_q<1>  (3,16,144) dead lanes in chunk 0; (3,5,1280) the widest row; (3,1,4) one live lane, M < 4 (idle waves);
                                      (3,16,256) / (3,16,260) exactly one chunk / one lane into the second; (2731,3,16) odd T at M >= 8192
  k_ln_mod_fwd<2>, k_ln_mod_fwd_q<2>  (16,256,64) M = 4096; (1366,6,16) M = 8196 with T % 4 != 0, M % 8 = 4: a half-idle last workgroup
  k_ln_mod_fwd<4>, k_ln_mod_fwd_q<4>  (32,256,64) M = 8192; (683,12,16) M = 8196: the last workgroup holds one wave with 4 rows
                                      large-M calls also bit-equal an RPW 1 call on their first 2048 rows
  k_ln_mod_fwd_q                      e4m3 bytes at scale 8 and 0.25, saturation at scale 128, act_amax word 0 (words 1, 2 untouched), NULL words,
                                      out / mean / rstd bit-equal to the unquantised entry; shifted rows (x = randn + 8) at D = 144, where a
                                      lane past the row end holds -mean rstd = -8 > every live output: the `live` masks
  k_row_bwd<LN|GATE|LN+GATE, combine> rows per chunk 32: T = 256; 16: T = 48, 16; 8: T = 24; 4: T = 12   (at D = 144; T = 256 also at 1152)
  k_row_bwd<..., no combine>          2 rows per wave: T = 6; 1: T = 5, 1                                  (at D = 144; T = 6 also at 1152)
  k_row_bwd width edges               D = 4 (one live lane), 256, 260, 768, 772 (the HALF = 3 boundary of the two-pass LDS combine), 1280, each
                                      at T = 16 (combine) and T = 6 (no combine); the fused entry with ldmod = 6 D != ldgate = 2 D + 4
  refusals                            D = 1284, D = 6, ldmod = 6 D + 2, M % T != 0: SFRON_ERR_ARG, nothing written
  k_reduce_chunks                     the per-sample sums of every partial buffer above (per = T / rows per chunk: 1 .. 8), ldout > D
  k_weighted_reduce                   (groups, per, D) = (3,4,1152), (1,1,4), (5,7,300), (2,16,256), ldw > D
  k_gated_bias_grads                  layers = 3, B = 3, D = 144 / 1152 with the engine's gate offsets, strided output
  k_colsum_partial<bf16,8|bf16,4|f32,4>  M = 1 .. 100 (the 16-row unroll, the 4-row tail, idle waves), N = 4 / 12 / 256 / 520, ld = N, N + 8,
                                      N + 4 (bf16: ld % 8 == 4 -> the 4-wide form), max_partials 1 / 64
  k_cond_fwd / k_cond_bwd             n = 1, 5, 32 (one full CB chunk), 33, 70 (three chunks), D = 4, 128, 300, 1152; label patterns below
  k_silu_fwd / k_silu_bwd             n = 1, 255, 257, 70000 over +-30, both outputs of the backward
  k_timestep_embed                    dim = 64, 256; ld = dim, dim + 8; odd dim refused

tests/dit_rows_ref.RECORD collects the largest error ratio / mismatch share per output; the module prints it at teardown (pytest -s)."""
import functools

import pytest
import torch

import dit_rows_ref as R

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


def sync():
    torch.cuda.synchronize()


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
    """a launch that faulted leaves the device context unusable: end the session there instead of launching the remaining cases on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault in tests/test_gpu_dit_rows.py: {e}", returncode=3)


@pytest.fixture(scope="module", autouse=True)
def _print_record():
    yield
    print()
    for name in sorted(R.RECORD):
        print("RECORD", name, " ".join(f"{k}={v:.4g}" for k, v in sorted(R.RECORD[name].items())))


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ================================================================================================ a. row forward
@functools.lru_cache(maxsize=None)
def fwd_case(B, T, D, shifted):
    i = R.row_inputs(B, T, D, shifted)
    return i, R.ln_modulate_fwd(i["x"], i["shift"], i["scale"], T, F64), R.ln_modulate_fwd(i["x"], i["shift"], i["scale"], T, F32)


def launch_fwd(i, T, M, D, q_scale=None, amax=None):
    """-> dict of guarded outputs (views) after the call, guards checked"""
    L = _L()
    x, mod = dev(i["x"][:M]), dev(i["mod"])
    shift, scale = mod.data_ptr() + 3 * D * 4, mod.data_ptr() + 4 * D * 4
    out, c_out = R.guarded((M, D), BF16)
    mean, c_mean = R.guarded((M,), F32)
    rstd, c_rstd = R.guarded((M,), F32)
    res = dict(out=out, mean=mean, rstd=rstd)
    checks = [c_out, c_mean, c_rstd]
    if q_scale is None:
        st = L.sfron_ln_modulate_fwd(x.data_ptr(), shift, scale, 6 * D, T, M, D, out.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _sp())
    else:
        out8, c_out8 = R.guarded((M, D), torch.uint8)
        res["out8"] = out8
        checks.append(c_out8)
        st = L.sfron_ln_modulate_fwd_q(x.data_ptr(), shift, scale, 6 * D, T, M, D, out.data_ptr(), out8.data_ptr(), q_scale, mean.data_ptr(),
                                       rstd.data_ptr(), amax.data_ptr() if amax is not None else None, _sp())
    assert st == 0, st
    sync()
    for c in checks:
        c("ln_modulate_fwd" + ("_q" if q_scale else ""))
    return res


def amax_words():
    w, check = R.guarded((3,), torch.int32)
    w.copy_(torch.tensor([0, 0x3F800000, 0x40000000], dtype=torch.int32))
    return w, check


def check_amax(w, check, want, what):
    check(what)
    host = w.cpu()
    assert host[1] == 0x3F800000 and host[2] == 0x40000000, f"{what}: words 1 / 2 were written"
    got = float(host[:1].view(F32))
    assert abs(got - want) <= 1e-5 * want, (what, got, want)
    return got


FWD_CASES = [(B, T, D, False) for B, T, D in R.FWD_SHAPES] + [(3, 16, 144, True), (3, 16, 260, True)]


@pytest.mark.parametrize("B,T,D,shifted", FWD_CASES)
def test_ln_modulate_fwd_and_its_quantising_twin(B, T, D, shifted):
    M = B * T
    i, (o64, m64, r64), (o32, m32, r32) = fwd_case(B, T, D, shifted)
    tag = "shifted." if shifted else ""
    plain = launch_fwd(i, T, M, D)
    R.bound_bf16(plain["out"], o64, o32, tag + "ln_fwd.out")
    R.bound32(plain["mean"], m64, m32, tag + "ln_fwd.mean")
    R.bound32(plain["rstd"], r64, r32, tag + "ln_fwd.rstd")
    qs = {}
    for s in (8.0, 0.25):
        w, cw = amax_words()
        q = qs[s] = launch_fwd(i, T, M, D, q_scale=s, amax=w)
        for k in ("out", "mean", "rstd"):
            assert bits_equal(q[k], plain[k]), f"ln_modulate_fwd_q {k} differs from the unquantised entry"
        R.check_e4m3(q["out8"], o64, o32, s, tag + "ln_fwd_q.e4m3")
        live = float((o64 * s).abs().max())
        got = check_amax(w, cw, live, "act_amax")
        if shifted:
            # a lane past the row end holds -mean rstd (1 + 0) + 0 = -8: above every live |out| here (see row_inputs)
            assert float((m64 * r64).abs().min()) > float(o64.abs().max())
            assert got <= live * (1 + 1e-5)
    if M >= 4096:       # the per-row arithmetic of the three templates is the same: an RPW 1 call on the first 2048 rows gives the same bits
        assert R.fwd_rpw(2048, T) == 1
        head_plain = launch_fwd(i, T, 2048, D)
        head = launch_fwd(i, T, 2048, D, q_scale=8.0, amax=None)
        for k in ("out", "mean", "rstd"):
            assert bits_equal(head[k], plain[k][:2048]) and bits_equal(head_plain[k], plain[k][:2048]), k
        assert bits_equal(head["out8"], qs[8.0]["out8"][:2048])


def test_ln_modulate_fwd_q_saturates_and_reports_the_unclipped_maximum():
    B, T, D = 3, 16, 144
    i, (o64, m64, r64), (o32, m32, r32) = fwd_case(B, T, D, False)
    s = 128.0
    assert float((o64 * s).abs().max()) > 1.5 * 448.0
    w, cw = amax_words()
    q = launch_fwd(i, T, B * T, D, q_scale=s, amax=w)
    R.check_e4m3(q["out8"], o64, o32, s, "ln_fwd_q.e4m3.saturating")
    dec = R.e4m3_decode(q["out8"])
    over = (o64 * s).abs() > 480.0          # past the last rounding boundary below the clamp
    assert int(over.sum()) > 10 and bool((dec[over] == 448.0 * torch.sign(o64[over])).all())
    check_amax(w, cw, float((o64 * s).abs().max()), "act_amax (saturating)")
    # no words: the same bytes
    q0 = launch_fwd(i, T, B * T, D, q_scale=s, amax=None)
    assert bits_equal(q0["out8"], q["out8"]) and bits_equal(q0["out"], q["out"])


def test_ln_modulate_fwd_refusals():
    L = _L()
    Dm = 1284
    x, mod = torch.zeros(48, Dm, device=DEV), torch.zeros(3, 6 * Dm + 8, device=DEV)
    out, c_out = R.guarded((48, Dm), BF16)
    out8, c_out8 = R.guarded((48, Dm), torch.uint8)
    mean, c_mean = R.guarded((48,), F32)
    rstd, c_rstd = R.guarded((48,), F32)
    for D, ldmod in ((1284, 6 * 1284), (6, 36), (144, 6 * 144 + 2)):
        sh, sc = mod.data_ptr() + 16, mod.data_ptr() + 32
        assert L.sfron_ln_modulate_fwd(x.data_ptr(), sh, sc, ldmod, 16, 48, D, out.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _sp()) == ERR_ARG
        assert L.sfron_ln_modulate_fwd_q(x.data_ptr(), sh, sc, ldmod, 16, 48, D, out.data_ptr(), out8.data_ptr(), 8.0, mean.data_ptr(),
                                         rstd.data_ptr(), None, _sp()) == ERR_ARG
    sync()
    for c in (c_out, c_out8, c_mean, c_rstd):
        R.untouched(c, "refused forward call")


# ================================================================================================ b. row backward
B3 = 3


@functools.lru_cache(maxsize=None)
def bwd_case(T, D, shifted):
    i = R.row_inputs(B3, T, D, shifted)
    rows = R.ROWS_PER_CHUNK[T]
    _, m64, r64 = R.ln_modulate_fwd(i["x"], i["shift"], i["scale"], T, F64)
    ref = {}
    for dt in (F64, F32):
        dln, ps, pc = R.ln_modulate_bwd(i["d_out"], i["x"], i["scale"], T, rows, dt)
        ref[dt] = dict(dln=dln, ps=ps, pc=pc, gate=R.gate_bwd(i["dx0"], i["branch"], i["gate"], T, rows, dt),
                       fused={acc: R.ln_gate_bwd(i["d_out"], i["x"], i["scale"], i["dx0"], acc, i["branch"], i["gate"], T, rows, dt)
                              for acc in (0, 1)})
    gbuf = torch.full((B3, 2 * D + 4), 7.0)           # the gate rows in a buffer of their own: ldgate = 2 D + 4 != ldmod = 6 D
    gbuf[:, 4:4 + D] = i["gate"]
    d = dict(x=dev(i["x"]), mod=dev(i["mod"]), d_out=dev(i["d_out"]), branch=dev(i["branch"]), dx0=dev(i["dx0"]), gbuf=dev(gbuf),
             mean=dev(m64.float()), rstd=dev(r64.float()))
    return i, rows, ref, d


class RowBwd:
    """one backward launch with every output guarded"""

    def __init__(self, T, D, d, rows, ln, gate, acc=1, dx_in=None):
        L = _L()
        M = B3 * T
        nchunk = M // rows
        self.checks = []

        def buf(shape, dtype):
            v, c = R.guarded(shape, dtype)
            self.checks.append(c)
            return v

        scale, ldmod = d["mod"].data_ptr() + 4 * D * 4, 6 * D
        gate_p, ldgate = d["gbuf"].data_ptr() + 16, 2 * D + 4
        if ln:
            self.dx = buf((M, D), F32)
            if acc:
                self.dx.copy_(d["dx0"] if dx_in is None else dx_in)
            self.ps, self.pc = buf((nchunk, D), F32), buf((nchunk, D), F32)
        else:
            self.dy = (d["dx0"] if dx_in is None else dx_in).clone()
        if gate:
            self.db = buf((M, D), BF16)
            self.pg, self.pd = buf((nchunk, D), F32), buf((nchunk, D), F32)
        p = lambda t: t.data_ptr()
        if ln and gate:
            st = L.sfron_ln_gate_bwd(p(d["d_out"]), p(d["x"]), p(d["mean"]), p(d["rstd"]), scale, ldmod, T, M, D, p(self.dx), acc, p(self.ps),
                                     p(self.pc), p(d["branch"]), gate_p, ldgate, p(self.db), p(self.pg), p(self.pd), _sp())
        elif ln:
            st = L.sfron_ln_modulate_bwd(p(d["d_out"]), p(d["x"]), p(d["mean"]), p(d["rstd"]), scale, ldmod, T, M, D, p(self.dx), acc,
                                         p(self.ps), p(self.pc), _sp())
        else:
            before = self.dy.clone()
            st = L.sfron_gate_bwd(p(self.dy), p(d["branch"]), gate_p, ldgate, T, M, D, p(self.db), p(self.pg), p(self.pd), _sp())
        assert st == 0, st
        sync()
        for c in self.checks:
            c(f"row backward ln={ln} gate={gate} T={T} D={D}")
        if not ln:
            assert bits_equal(self.dy, before), "sfron_gate_bwd changed its dy input"


def reduced(p, per, D):
    """sfron_reduce_chunks of a partial buffer into a guarded [B][D + 4] output -> the [B][D] block"""
    out, check = R.guarded((B3, D), F32, ld=D + 4)
    assert _L().sfron_reduce_chunks(p.data_ptr(), B3, per, D, out.data_ptr(), D + 4, 0, _sp()) == 0
    sync()
    check("reduce_chunks")
    return out


BWD_CASES = [(T, D, False) for T, D in R.BWD_SHAPES] + [(5, 144, True), (16, 260, True)]


@pytest.mark.parametrize("T,D,shifted", BWD_CASES)
def test_row_backward_against_the_reference(T, D, shifted):
    i, rows, ref, d = bwd_case(T, D, shifted)
    assert _L().sfron_rows_per_chunk(T) == rows
    per = T // rows
    r64, r32 = ref[F64], ref[F32]
    tag = "shifted." if shifted else ""
    for acc in (1, 0):
        k = RowBwd(T, D, d, rows, ln=True, gate=False, acc=acc)        # acc = 0: dx starts as NaN sentinels and must come out finite
        add64, add32 = (i["dx0"].double(), i["dx0"]) if acc else (0.0, 0.0)
        R.bound32(k.dx, r64["dln"] + add64, r32["dln"] + add32, tag + "ln_bwd.dx")
        R.bound32(k.ps, r64["ps"], r32["ps"], tag + "ln_bwd.p_shift")
        R.bound32(k.pc, r64["pc"], r32["pc"], tag + "ln_bwd.p_scale")
    R.bound32(reduced(k.ps, per, D), R.sample_sums(r64["ps"], B3), R.sample_sums(r32["ps"], B3), tag + "ln_bwd.d_shift")
    R.bound32(reduced(k.pc, per, D), R.sample_sums(r64["pc"], B3), R.sample_sums(r32["pc"], B3), tag + "ln_bwd.d_scale")
    g = RowBwd(T, D, d, rows, ln=False, gate=True)
    (db64, pg64, pd64), (db32, pg32, pd32) = r64["gate"], r32["gate"]
    R.bound_bf16(g.db, db64, db32, tag + "gate_bwd.d_branch")
    R.bound32(g.pg, pg64, pg32, tag + "gate_bwd.p_gate")
    R.bound32(g.pd, pd64, pd32, tag + "gate_bwd.p_dy")
    R.bound32(reduced(g.pg, per, D), R.sample_sums(pg64, B3), R.sample_sums(pg32, B3), tag + "gate_bwd.d_gate")
    R.bound32(reduced(g.pd, per, D), R.sample_sums(pd64, B3), R.sample_sums(pd32, B3), tag + "gate_bwd.sum_dy")


@pytest.mark.parametrize("T,D,shifted", BWD_CASES)
def test_fused_row_backward_equals_separate_and_the_reference(T, D, shifted):
    i, rows, ref, d = bwd_case(T, D, shifted)
    tag = "shifted." if shifted else ""
    for acc in (1, 0):
        f = RowBwd(T, D, d, rows, ln=True, gate=True, acc=acc)
        a = RowBwd(T, D, d, rows, ln=True, gate=False, acc=acc)
        b = RowBwd(T, D, d, rows, ln=False, gate=True, dx_in=a.dx)
        for name, u, v in (("dx", f.dx, a.dx), ("p_shift", f.ps, a.ps), ("p_scale", f.pc, a.pc), ("d_branch", f.db, b.db),
                           ("p_gate", f.pg, b.pg), ("p_dy", f.pd, b.pd)):
            assert bits_equal(u, v), f"fused {name} differs from the separate kernels (dx_accumulate = {acc})"
        w64, w32 = ref[F64]["fused"][acc], ref[F32]["fused"][acc]
        R.bound32(f.dx, w64[0], w32[0], tag + "ln_gate_bwd.dx")
        R.bound_bf16(f.db, w64[3], w32[3], tag + "ln_gate_bwd.d_branch")
        R.bound32(f.pg, w64[4], w32[4], tag + "ln_gate_bwd.p_gate")
        R.bound32(f.pd, w64[5], w32[5], tag + "ln_gate_bwd.p_dy")


def test_row_backward_refusals():
    L = _L()
    T, M, Dm = 16, 48, 1284
    z = lambda *s: torch.zeros(*s, device=DEV)
    d_out, branch = z(M, Dm).to(BF16), z(M, Dm).to(BF16)
    x, mean, rstd, mod = z(M, Dm), z(M), z(M), z(3, 6 * Dm + 8)
    bufs = [R.guarded(s, t) for s, t in (((M, Dm), F32), ((M, Dm), F32), ((M, Dm), F32), ((M, Dm), BF16), ((M, Dm), F32), ((M, Dm), F32))]
    (dx, _), (ps, _), (pc, _), (db, _), (pg, _), (pd, _) = bufs
    p = lambda t: t.data_ptr()
    sc = p(mod) + 16
    for D, ldmod, tokens in ((1284, 6 * 1284, T), (6, 36, T), (144, 6 * 144 + 2, T), (144, 6 * 144, 7)):
        for acc in (0, 1):
            assert L.sfron_ln_modulate_bwd(p(d_out), p(x), p(mean), p(rstd), sc, ldmod, tokens, M, D, p(dx), acc, p(ps), p(pc), _sp()) == ERR_ARG
            assert L.sfron_ln_gate_bwd(p(d_out), p(x), p(mean), p(rstd), sc, ldmod, tokens, M, D, p(dx), acc, p(ps), p(pc), p(branch), sc,
                                       ldmod, p(db), p(pg), p(pd), _sp()) == ERR_ARG
        assert L.sfron_gate_bwd(p(dx), p(branch), sc, ldmod, tokens, M, D, p(db), p(pg), p(pd), _sp()) == ERR_ARG
    # the fused entry checks ldgate on its own
    assert L.sfron_ln_gate_bwd(p(d_out), p(x), p(mean), p(rstd), sc, 6 * 144, T, M, 144, p(dx), 0, p(ps), p(pc), p(branch), sc, 2 * 144 + 2,
                               p(db), p(pg), p(pd), _sp()) == ERR_ARG
    sync()
    for _, c in bufs:
        R.untouched(c, "refused backward call")


# ================================================================================================ c. reductions
@pytest.mark.parametrize("groups,per,D", [(3, 4, 1152), (1, 1, 4), (5, 7, 300), (2, 16, 256)])
def test_weighted_reduce(groups, per, D):
    g = torch.Generator().manual_seed(groups * 100 + per + D)
    P = torch.randn(groups, per, D, generator=g)
    ldw = D + 4
    wbuf = torch.randn(groups, ldw, generator=g)
    w = wbuf[:, :D]
    Pd, wd = dev(P), dev(wbuf)
    res = []
    for _ in range(2):
        out, check = R.guarded((D,), F32)
        assert _L().sfron_weighted_reduce(Pd.data_ptr(), groups, per, D, wd.data_ptr(), ldw, out.data_ptr(), _sp()) == 0
        sync()
        check("weighted_reduce")
        res.append(out)
    assert bits_equal(res[0], res[1])
    R.bound32(res[0], R.weighted_reduce(P, w, F64), R.weighted_reduce(P, w, F32), "weighted_reduce")


@pytest.mark.parametrize("D", [144, 1152])
def test_gated_bias_grads(D):
    layers, B = 3, 3
    g = torch.Generator().manual_seed(D)
    ldg, gate_stride, gate_which = layers * 6 * D, 6 * D, 3 * D          # the engine's adaLN buffer: gate_msa = chunk 2, gate_mlp = chunk 5
    gbuf = torch.randn(B, ldg, generator=g)
    S = torch.randn(layers * 2 * B, D, generator=g)
    out_stride, which0, which1 = 5 * D + 8, 4, 3 * D + 8
    gflat = gbuf.reshape(-1)[2 * D:]
    r64 = R.gated_bias_grads(S, gflat, ldg, gate_stride, gate_which, layers, B, D, F64)
    r32 = R.gated_bias_grads(S, gflat, ldg, gate_stride, gate_which, layers, B, D, F32)
    Sd, gd = dev(S), dev(gbuf)
    res = []
    for _ in range(2):
        out, check = R.guarded((layers * out_stride,), F32)
        assert _L().sfron_gated_bias_grads(Sd.data_ptr(), gd.data_ptr() + 2 * D * 4, ldg, gate_stride, gate_which, layers, B, D, out.data_ptr(),
                                           out_stride, which0, which1, _sp()) == 0
        sync()
        check("gated_bias_grads")
        res.append(out)
    assert bits_equal(res[0], res[1])
    out = res[0]
    addressed = torch.zeros(layers * out_stride, dtype=torch.bool)
    got = torch.empty(layers, 2, D)
    for l in range(layers):
        for which, off in ((0, which0), (1, which1)):
            addressed[l * out_stride + off:l * out_stride + off + D] = True
            got[l, which] = out[l * out_stride + off:l * out_stride + off + D].cpu()
    rest = out.view(torch.int32).cpu()[~addressed]
    assert bool((rest == check.sentinel).all()), "elements outside the addressed rows were written"
    R.bound32(got, r64, r32, "gated_bias_grads")


COLSUM_FORMS = ([("bf16x8", N, N + e) for N in (256, 520) for e in (0, 8)]
                + [("bf16x4", N, N + e) for N in (4, 12) for e in (0, 8)] + [("bf16x4", N, N + 4) for N in (256, 520)]
                + [("f32", N, N + e) for N in (4, 256, 520) for e in (0, 8)])


@pytest.mark.parametrize("form,N,ld", COLSUM_FORMS)
def test_colsum_every_form(form, N, ld):
    L = _L()
    is_bf16 = form != "f32"
    assert (form == "bf16x8") == (is_bf16 and N % 8 == 0 and ld % 8 == 0)          # the launcher's rule
    g = torch.Generator().manual_seed(N * 7 + ld)
    for M in (1, 3, 31, 32, 33, 100):
        X = torch.full((M, ld), 1e4)                      # the pad columns hold a value that would show in any sum
        X[:, :N] = torch.randn(M, N, generator=g) + 0.25
        X = X.to(BF16) if is_bf16 else X
        Xd = dev(X)
        r64, r32 = R.colsum(X[:, :N], F64), R.colsum(X[:, :N], F32)
        for maxp in (1, 64):
            chunks = min(-(-M // 32), maxp)
            chunks = -(-M // -(-M // chunks))
            res = []
            for _ in range(2):
                part, c_part = R.guarded((maxp, N), F32)
                out, c_out = R.guarded((N,), F32)
                assert L.sfron_colsum(Xd.data_ptr(), int(is_bf16), M, N, ld, part.data_ptr(), maxp, out.data_ptr(), _sp()) == 0
                sync()
                c_part("colsum partials")
                c_out("colsum out")
                assert bool((part.view(torch.int32)[chunks:] == c_part.sentinel).all()), "partial rows past the chunk count were written"
                res.append((out, part[:chunks]))
            assert bits_equal(res[0][0], res[1][0]) and bits_equal(res[0][1], res[1][1])
            R.bound32(res[0][0], r64, r32, "colsum." + form)
            R.bound32(res[0][1].double().sum(0), r64, r32, "colsum." + form + ".partials")


# ================================================================================================ d. conditioning
NC = 10


def label_cases(n, g):
    y = torch.randint(0, NC, (n,), generator=g)
    some = (torch.rand(n, generator=g) < 0.4).to(torch.uint8)
    odd = y.clone()
    odd[0] = 2 ** 40
    if n >= 3:
        odd[n // 2], odd[n - 1] = -1, NC
    return [("all equal", torch.full((n,), 3), some), ("all distinct", torch.arange(n) % NC, torch.zeros(n, dtype=torch.uint8)),
            ("mixed repeats", y, some), ("all dropped", y, torch.ones(n, dtype=torch.uint8)), ("drop = NULL", y, None),
            ("labels -1, 10, 2^40", odd, None)]


@pytest.mark.parametrize("D", [4, 128, 300, 1152])
@pytest.mark.parametrize("n", [1, 5, 32, 33, 70])
def test_cond_fwd_bwd(n, D):
    L = _L()
    g = torch.Generator().manual_seed(n * 10007 + D)
    t_emb, table = torch.randn(n, D, generator=g), torch.randn(NC + 1, D, generator=g)
    d_silu = torch.randn(n, D, generator=g)
    table0 = torch.randn(NC + 1, D, generator=g)                      # d_table starts out random: the kernel accumulates onto it
    te_d, tab_d, ds_d = dev(t_emb), dev(table), dev(d_silu)
    for what, y, drop in label_cases(n, g):
        lab = R.labels_used(y, drop, NC)
        if what.startswith("labels"):
            assert lab[0] == NC and (n < 3 or (lab[n // 2] == NC and lab[n - 1] == NC))
        y_d = dev(y)
        drop_d = dev(drop) if drop is not None else None
        c, c_c = R.guarded((n, D), F32)
        sc, c_sc = R.guarded((n, D), BF16)
        assert L.sfron_cond_fwd(te_d.data_ptr(), tab_d.data_ptr(), y_d.data_ptr(), drop_d.data_ptr() if drop is not None else None, NC, n, D,
                                c.data_ptr(), sc.data_ptr(), _sp()) == 0
        sync()
        c_c(what)
        c_sc(what)
        c64, s64 = R.cond_fwd(t_emb, table, y, drop, NC, F64)
        c32, s32 = R.cond_fwd(t_emb, table, y, drop, NC, F32)
        assert torch.equal(c.cpu(), c32), f"{what}: c is one fp32 add"
        R.bound_bf16(sc, s64, s32, "cond_fwd.silu_c")
        d_c, c_dc = R.guarded((n, D), F32)
        d_tab, c_dt = R.guarded((NC + 1, D), F32)
        d_tab.copy_(table0)
        assert L.sfron_cond_bwd(ds_d.data_ptr(), c.data_ptr(), y_d.data_ptr(), drop_d.data_ptr() if drop is not None else None, NC, n, D,
                                d_c.data_ptr(), d_tab.data_ptr(), _sp()) == 0
        sync()
        c_dc(what)
        c_dt(what)
        dc64, dt64 = R.cond_bwd(d_silu, c32, y, drop, NC, table0, F64)
        dc32, dt32 = R.cond_bwd(d_silu, c32, y, drop, NC, table0, F32)
        R.bound32(d_c, dc64, dc32, "cond_bwd.d_c")
        R.bound32(d_tab, dt64, dt32, "cond_bwd.d_table")
        # the order include/sfron.h promises: the returned d_c rows added in batch order, in fp32, onto the table as it was
        seq, dch = table0.clone(), d_c.cpu()
        for b in range(n):
            seq[lab[b]] += dch[b]
        assert torch.equal(d_tab.cpu(), seq), f"{what}: d_table is not the batch-order fp32 accumulation of d_c"
        absent = torch.ones(NC + 1, dtype=torch.bool)
        absent[lab] = False
        assert bits_equal(d_tab.cpu()[absent], table0[absent]), f"{what}: rows of absent labels changed"


@pytest.mark.parametrize("n", [1, 255, 257, 70000])
def test_silu_fwd_bwd(n):
    L = _L()
    g = torch.Generator().manual_seed(n)
    x = torch.rand(n, generator=g) * 60 - 30
    x[0], x[-1] = -30.0, 30.0
    if n > 2:
        x[1] = 30.0
    dy = torch.randn(n, generator=g)
    xd, dyd = dev(x), dev(dy)
    y, c_y = R.guarded((n,), BF16)
    assert L.sfron_silu_fwd(xd.data_ptr(), n, y.data_ptr(), _sp()) == 0
    db, c_db = R.guarded((n,), BF16)
    df, c_df = R.guarded((n,), F32)
    assert L.sfron_silu_bwd(dyd.data_ptr(), xd.data_ptr(), n, db.data_ptr(), df.data_ptr(), _sp()) == 0
    sync()
    for c in (c_y, c_db, c_df):
        c("silu")
    assert not torch.isnan(y.float()).any() and not torch.isnan(df).any() and not torch.isnan(db.float()).any()
    R.bound_bf16(y, R.silu(x, F64), R.silu(x, F32), "silu_fwd")
    d64, d32 = dy.double() * R.silu_grad(x, F64), dy * R.silu_grad(x, F32)
    R.bound_bf16(db, d64, d32, "silu_bwd.bf16")
    R.bound32(df, d64, d32, "silu_bwd.f32")
    # one output at a time gives the same values
    db1, c1 = R.guarded((n,), BF16)
    df1, c2 = R.guarded((n,), F32)
    assert L.sfron_silu_bwd(dyd.data_ptr(), xd.data_ptr(), n, db1.data_ptr(), None, _sp()) == 0
    assert L.sfron_silu_bwd(dyd.data_ptr(), xd.data_ptr(), n, None, df1.data_ptr(), _sp()) == 0
    sync()
    c1("silu_bwd bf16 only")
    c2("silu_bwd fp32 only")
    assert bits_equal(db1, db) and bits_equal(df1, df)


@pytest.mark.parametrize("dim,extra", [(64, 0), (64, 8), (256, 0), (256, 8)])
def test_timestep_embed(dim, extra):
    L = _L()
    t = torch.tensor([0, 1, 2, 37, 500, 999])
    td = dev(t)
    out, check = R.guarded((6, dim), BF16, ld=dim + extra)
    assert L.sfron_timestep_embed(td.data_ptr(), 6, dim, out.data_ptr(), dim + extra, _sp()) == 0
    sync()
    check("timestep_embed")
    R.bound_bf16(out, R.timestep_embed(t, dim, F64), R.timestep_embed(t, dim, F32), "timestep_embed")
    spare, c_spare = R.guarded((6, dim), BF16)
    assert L.sfron_timestep_embed(td.data_ptr(), 6, dim - 1, spare.data_ptr(), dim, _sp()) == ERR_ARG
    sync()
    R.untouched(c_spare, "odd dim")
