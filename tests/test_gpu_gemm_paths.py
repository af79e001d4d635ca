"""GPU: every dispatch path of sfron_gemm_bf16 (csrc/gemm.hip) and sfron_bgemm_bf16 (csrc/conv.hip) at the smallest shape that reaches it,
on integer data -- every output must EQUAL the float64 reference, no tolerance -- through strided, guarded buffers: every operand and
output is a window inside a larger allocation (leading dimension > extent, column offset 8, batch strides larger than a matrix), operands
surrounded by 16384, outputs pre-filled with NaN and surrounded by a bit pattern that must survive (pad columns, 512 guard rows on both
sides, the gaps between batch matrices).  tests/test_gemm_paths_cpu.py owns the case tables, the path labels (a restatement of the
dispatchers' predicates), the layouts, the references, the proof that every result is exact in fp32 and the checkers (tested there against
faulty copies); this file only launches and compares.

Only the transcendental epilogues keep a tolerance -- the ones tests/test_gpu_gemm.py::test_epilogues and tests/test_gpu_text_encoder.py
already hold them to: GELU's activation (its pre-activation `aux` is exact), DGELU, QUICK_GELU and the one-byte GELU' codes.  They run on
the integer data (placement, guards) and on unit-scale data.

A failure names the region first: last tile row, last tile column, pad columns, guard rows, then every element (pytest -s prints nothing on
success: an exact comparison has no ratio to report)."""
import ctypes

import pytest
import torch

import test_gemm_paths_cpu as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = 1001          # csrc/common.h


def _api():
    from sfron import _lib, unet
    return _lib, _lib.lib(), unet


def _sp():
    from sfron._lib import stream_ptr
    return stream_ptr()


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
    """a launch that faulted leaves the device context unusable: end the session there instead of launching the remaining cases on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault in tests/test_gpu_gemm_paths.py: {e}", returncode=3)


class Dev:
    """a Win's host image on the device; .ptr = the address of the first window's first element"""

    def __init__(self, win):
        self.win = win
        self.t = win.full.to(DEV)
        self.ptr = self.t.data_ptr() + win.byte_offset

    @property
    def view(self):
        return self.t[self.win.base:]


def _dev(win):
    return Dev(win) if win is not None else None


def _p(d):
    return d.ptr if d is not None else None


def _untouched(d, what):
    assert torch.equal(d.t.view(T.PATTERN[d.win.es][0]), d.win.full.view(T.PATTERN[d.win.es][0]).to(DEV)), f"{what} was written to"


class _loader_waves:
    """run under sfron_gemm_loader_waves(n), restore the old value"""

    def __init__(self, L, n):
        self.L, self.n = L, n

    def __enter__(self):
        self.old = self.L.sfron_gemm_loader_waves(self.n)

    def __exit__(self, *a):
        self.L.sfron_gemm_loader_waves(self.old)


# ------------------------------------------------------------------------------------------------ sfron_bgemm_bf16
def _bg_desc(_lib, c, p, A, B, C, bias, vec, resid):
    d = _lib.BGemmDesc()
    d.A, d.B, d.M, d.N, d.K, d.lda, d.ldb = A.ptr, B.ptr, c.M, c.N, c.K, p.A.ld, p.B.ld
    d.a_transposed, d.b_transposed, d.batch, d.batch2 = c.a_t, c.b_t, c.batch, c.batch2
    if c.batch > 1:
        d.stride_a, d.stride_b, d.stride_c = p.A.stride, p.B.stride, p.C.stride
    if c.batch2 > 1:
        d.stride_a2, d.stride_b2, d.stride_c2 = p.A.stride2, p.B.stride2, p.C.stride2
    d.alpha, d.bias, d.ldc = c.alpha, _p(bias), p.C.ld
    if c.out == "f32":
        d.c_f32 = C.ptr
    else:
        d.c_bf16 = C.ptr
    d.resid, d.sample_vec, d.ld_vec, d.rows_per_sample, d.accumulate = _p(resid), _p(vec), (p.vec.ld if p.vec else 0), c.rps, int(c.epi == "acc")
    return d


def _bg_launch(c, p):
    _lib, L, unet = _api()
    A, B, C, bias, vec, resid = (_dev(w) for w in (p.A, p.B, p.C, p.bias, p.vec, p.resid))
    if c.scratch:        # as the models call it: unet.bgemm arms the split scratch by its own rule
        kw = dict(c_f32=C.view) if c.out == "f32" else dict(c_bf16=C.view)
        unet.bgemm(A.view, B.view, c.M, c.N, c.K, lda=p.A.ld, ldb=p.B.ld, a_t=bool(c.a_t), b_t=bool(c.b_t), batch=c.batch, sa=p.A.stride if c.batch > 1 else 0,
                   sb=p.B.stride if c.batch > 1 else 0, sc=p.C.stride if c.batch > 1 else 0, batch2=c.batch2, sa2=p.A.stride2 if c.batch2 > 1 else 0,
                   sb2=p.B.stride2 if c.batch2 > 1 else 0, sc2=p.C.stride2 if c.batch2 > 1 else 0, alpha=c.alpha, ldc=p.C.ld, **kw)
    else:
        d = _bg_desc(_lib, c, p, A, B, C, bias, vec, resid)
        assert L.sfron_bgemm_bf16(ctypes.byref(d), _sp()) == 0, c.id
    T.check(p.C, C.t, p.ref, c.id, tile=(256, 128))
    for name, x in (("A", A), ("B", B), ("bias", bias), ("sample_vec", vec), ("resid", resid)):
        if x is not None:
            _untouched(x, f"{c.id}: operand {name}")


@pytest.mark.parametrize("c", T.BG_CASES, ids=T.BG_IDS)
def test_bgemm_path(c):
    _, L, _ = _api()
    p = T.bg_problem(c)
    nk = T.bgemm_path(c)[1]
    if nk >= 8:      # the loader-wave form of the pipelined tiles (chosen at nk >= 8) and the shared form: same bits
        for form in (4, 10):
            with _loader_waves(L, form):
                _bg_launch(c, p)
    else:
        _bg_launch(c, p)


def _refusals():
    """one per argument rule at the head of sfron_bgemm_bf16: (name, layout (a_t, b_t), edit of the descriptor, expected status)"""
    def s(**kw):
        return lambda d: [setattr(d, k, v) for k, v in kw.items()]
    R = [("A-null", (0, 0), s(A=None)), ("B-null", (0, 0), s(B=None)), ("M-0", (0, 0), s(M=0)), ("N-0", (0, 0), s(N=0)), ("K-0", (0, 0), s(K=0)),
         ("batch-0", (0, 0), s(batch=0)), ("N%4", (0, 0), s(N=50)), ("lda%8", (0, 0), s(lda=84)), ("ldb%8", (0, 0), s(ldb=84)),
         ("A-misaligned", (0, 0), lambda d: setattr(d, "A", d.A + 8)), ("B-misaligned", (0, 0), lambda d: setattr(d, "B", d.B + 2)),
         ("stride_a%8", (0, 0), s(batch=2, stride_a=4, stride_b=0, stride_c=0)), ("stride_b%8", (0, 0), s(batch=2, stride_b=12)),
         ("stride_c%4", (0, 0), s(batch=2, stride_c=2)), ("K%8-direct", (0, 0), s(K=68)), ("K%8-b_t", (0, 1), s(K=68)), ("M%8-a_t", (1, 1), s(M=92)),
         ("N%8-b_t", (0, 1), s(N=52)), ("N%8-both_t", (1, 1), s(N=52)), ("stride_a2%8", (0, 0), s(batch2=2, stride_a2=4)),
         ("stride_b2%8", (0, 0), s(batch2=2, stride_b2=4)), ("stride_c2%4", (0, 0), s(batch2=2, stride_c2=2)), ("ldc%4", (0, 0), s(ldc=58)),
         ("no-output", (0, 0), s(c_f32=None, c_bf16=None)), ("both-outputs", (0, 0), "both"),
         # A stored [K][M] against a B that is not transposed (N % 8, K % 8 and M % 8 hold: this rule alone refuses it)
         ("a_t-without-b_t", (1, 1), s(b_transposed=0)),
         # the 2 GiB rule, per matrix: ((rows - 1) ld + columns) x element size of 96 rows passes 2^31 bytes; refused before any launch
         ("A-2GiB", (0, 0), s(lda=12_000_000)), ("A-2GiB-a_t", (1, 1), s(lda=16_000_000)), ("B-2GiB", (0, 0), s(ldb=20_000_000)),
         ("C-2GiB", (0, 0), s(ldc=6_000_000))]
    return [(n, lay, e, ERR_ARG) for n, lay, e in R]


@pytest.mark.parametrize("name,layout,edit,status", _refusals(), ids=[r[0] for r in _refusals()])
def test_bgemm_refuses(name, layout, edit, status):
    """each argument rule at the head of the entry point: SFRON_ERR_ARG, and not one byte of the NaN output or its guards touched.  The
    descriptor is first run unedited, so the edit alone is what is refused."""
    _lib, L, _ = _api()
    M, N, K = 96, 56, 72
    a_t, b_t = layout
    A = Dev(T.Win(*((K, M) if a_t else (M, K)), T.BF16).set(torch.ones((K, M) if a_t else (M, K))))
    B = Dev(T.Win(*((K, N) if b_t else (N, K)), T.BF16).set(torch.ones((K, N) if b_t else (N, K))))
    C = Dev(T.Win(M, N, T.F32, ld=N + 4, kind="output"))
    d = _lib.BGemmDesc()
    d.A, d.B, d.M, d.N, d.K, d.lda, d.ldb, d.a_transposed, d.b_transposed = A.ptr, B.ptr, M, N, K, A.win.ld, B.win.ld, a_t, b_t
    d.batch, d.alpha, d.c_f32, d.ldc = 1, 1.0, C.ptr, N + 4
    assert L.sfron_bgemm_bf16(ctypes.byref(d), _sp()) == 0          # the descriptor is accepted before the edit
    C = Dev(C.win)
    d.c_f32 = C.ptr
    if edit == "both":
        d.c_bf16 = C.ptr
    else:
        edit(d)
    assert L.sfron_bgemm_bf16(ctypes.byref(d), _sp()) == status, name
    torch.cuda.synchronize()
    _untouched(C, f"refusal {name}: the output")


# ------------------------------------------------------------------------------------------------ sfron_gemm_bf16
def _gemm_launch(c, p):
    _lib, L, _ = _api()
    a_t, b_t = T.LAYOUTS[c.layout]
    A, B, bias = Dev(p.A), Dev(p.B), _dev(p.bias)
    ins = {k: _dev(w) for k, w in p.ins.items()}
    outs = {k: Dev(w) for k, (w, _, _) in p.outs.items()}
    d = _lib.GemmDesc()
    d.A, d.B, d.M, d.N, d.K, d.lda, d.ldb, d.a_transposed, d.b_transposed = A.ptr, B.ptr, c.M, c.N, c.K, p.A.ld, p.B.ld, a_t, b_t
    d.epilogue, d.alpha, d.tokens, d.accumulate, d.tile_hint, d.split_k = c.epi, c.alpha, c.tokens, int(c.acc), c.hint, c.split_k
    if c.split_k > 1:
        d.c_f32, d.ldc_f32, d.split_stride = outs["slabs"].ptr, p.C.ld, p.C.stride
    else:
        d.bias = _p(bias)
    if "c_bf16" in outs:
        d.c_bf16, d.ldc_bf16 = outs["c_bf16"].ptr, outs["c_bf16"].win.ld
    if "c_f32" in outs:
        d.c_f32, d.ldc_f32 = outs["c_f32"].ptr, outs["c_f32"].win.ld
    aux = outs.get("aux") or ins.get("aux")
    if aux is not None:
        d.aux, d.ldaux = aux.ptr, aux.win.ld
    if "gate" in ins and c.split_k <= 1:
        d.gate, d.ldgate = ins["gate"].ptr, ins["gate"].win.ld
    if "resid" in ins and c.split_k <= 1:
        d.resid = ins["resid"].ptr
    if "pos" in ins:
        d.pos = ins["pos"].ptr
    keep = None
    if "a_rowsum" in outs:
        keep = torch.empty((c.N // 192) * c.M, dtype=torch.float32, device=DEV)
        d.a_rowsum, d.rowsum_ws = outs["a_rowsum"].ptr, keep.data_ptr()
    if "col_partials" in outs:
        d.col_partials = outs["col_partials"].ptr
    if "sumsq_partials" in outs:
        d.sumsq_partials, d.sumsq_mask = outs["sumsq_partials"].ptr, _p(ins.get("mask"))
    with _loader_waves(L, c.lw):
        status = L.sfron_gemm_bf16(ctypes.byref(d), _sp())
    assert status == 0, (c.id, status)
    t = T.HINT_TILE.get(c.hint, 1)
    tile = (T.TILE_BM[t], T.TILE_BN[t])
    for k, (w, ref, bound) in p.outs.items():
        # (sumsq_partials: fp64 sums of squares of exact values, partial b from the 192 x 192 tile of workgroup b: exact, tile by tile)
        T.check(w, outs[k].t, ref, f"{c.id}: {k}", bound=bound, tile=tile)
    for name, x in [("A", A), ("B", B), ("bias", bias)] + list(ins.items()):
        if x is not None:
            _untouched(x, f"{c.id}: operand {name}")
    if c.finish:
        _finish(c, p, L, outs["slabs"], ins)


def _finish(c, p, L, slabs, ins):
    """the three finish kernels of a split product on the packed slabs: summed in index order, epilogue applied once"""
    M, N, S = c.M, c.N, p.used
    fin = {k: Dev(w) for k, (w, _, _) in p.fin.items()}
    if c.finish == "reduce":
        rc = L.sfron_reduce_chunks(slabs.ptr, 1, S, M * N, fin["out"].ptr, M * N, 0, _sp())
    elif c.finish == "sum_bf16":
        rc = L.sfron_split_sum_bf16(slabs.ptr, S, M * N, p.C.stride, fin["out"].ptr, _sp())
    else:
        rc = L.sfron_split_gate_res(slabs.ptr, S, p.C.stride, _p(ins.get("bias2")), ins["gate"].ptr, ins["gate"].win.ld, c.tokens, ins["resid"].ptr,
                                    fin["out"].ptr, fin["branch"].ptr, M, N, _sp())
    assert rc == 0, (c.id, c.finish, rc)
    for k, (w, ref, bound) in p.fin.items():
        T.check(w, fin[k].t, ref, f"{c.id}: {c.finish} {k}", bound=bound)


def _group(*names):
    cs = [c for c in T.GEMM_CASES if c.group in names]
    return dict(argvalues=cs, ids=[c.id for c in cs])


@pytest.mark.parametrize("c", **_group("generic"))
def test_gemm_generic_kernel(c):
    _gemm_launch(c, T.gemm_problem(c))


@pytest.mark.parametrize("c", **_group("auto"))
def test_gemm_automatic_choice(c):
    _gemm_launch(c, T.gemm_problem(c))


@pytest.mark.parametrize("c", **_group("split"))
def test_gemm_split_k_slabs_and_finish_kernels(c):
    _gemm_launch(c, T.gemm_problem(c))


@pytest.mark.parametrize("c", **_group("linear"))
def test_gemm_linear_epilogues_through_the_tiles(c):
    _gemm_launch(c, T.gemm_problem(c))


@pytest.mark.parametrize("c", **_group("hint", "hint-misfit"))
def test_gemm_tile_hint(c):
    _gemm_launch(c, T.gemm_problem(c))


def test_gelu_q_activation_equals_the_bf16_pre_activation_form():
    """SFRON_EPI_GELU_Q and SFRON_EPI_GELU run the same operations on the same accumulators: the activation agrees bit for bit, through
    strided outputs as well (tests/test_gpu_gemm.py holds the packed form to the same)"""
    _lib, L, _ = _api()
    cq = next(c for c in T.GEMM_CASES if c.epi == T.EPI_GELU_Q and c.scaled)
    p = T.gemm_problem(cq)
    got = {}
    for epi, adt in ((T.EPI_GELU_Q, T.U8), (T.EPI_GELU, T.BF16)):
        A, B, bias = Dev(p.A), Dev(p.B), Dev(p.bias)
        cw = p.outs["c_bf16"][0]
        C, X = Dev(cw), Dev(T.Win(cq.M, cq.N, adt, ld=cq.N + 16, off=16, kind="output"))
        d = _lib.GemmDesc()
        d.A, d.B, d.M, d.N, d.K, d.lda, d.ldb, d.epilogue, d.alpha, d.bias = A.ptr, B.ptr, cq.M, cq.N, cq.K, p.A.ld, p.B.ld, epi, 1.0, bias.ptr
        d.c_bf16, d.ldc_bf16, d.aux, d.ldaux, d.tokens = C.ptr, cw.ld, X.ptr, cq.N + 16, 1
        assert L.sfron_gemm_bf16(ctypes.byref(d), _sp()) == 0
        got[epi] = C.t
    assert torch.equal(got[T.EPI_GELU_Q].view(torch.int16), got[T.EPI_GELU].view(torch.int16))
