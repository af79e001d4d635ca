"""CPU: the case tables, the strided + guarded buffer layouts, the float64 references, the exactness proofs and the checkers of
tests/test_gpu_gemm_paths.py (which imports this module).  Nothing here calls the library.

Two entry points carry almost every FLOP: sfron_gemm_bf16 (csrc/gemm.hip, the DiT blocks) and sfron_bgemm_bf16 (csrc/conv.hip: every Linear
and attention product of the U-Nets, the VAEs, the text encoder and the classifiers).  Each is a dispatcher over about a dozen kernels.  The
GPU file runs the smallest shape that reaches each of them

  * on INTEGER data: operands are integers in -3 .. 3 (exact in bf16); bias, sample_vec, resid, pos and prior output contents are multiples
    of 1/4; gate is an integer in -2 .. 2; alpha is 1, 0.5 or -2.  Every partial sum in any order is then a multiple of 1/8 far below 2^24 / 8,
    so every fp32 result, every split-K slab sum and every epilogue addition must EQUAL the float64 reference -- no tolerance.  bf16 outputs
    must equal the reference rounded once, to nearest even.  test_results_are_exact_in_fp32 proves the magnitude bound for every case from
    its inputs.  Only the transcendental epilogues (GELU's activation, DGELU, QUICK_GELU) keep the bounds tests/test_gpu_gemm.py::
    test_epilogues and tests/test_gpu_text_encoder.py already hold them to;
  * through STRIDED, GUARDED buffers (class Win): every operand and output is a window inside a larger allocation -- leading dimension =
    extent + 8 (outputs: N + 4, or N + 8), the window starts 8 elements into its row, batch strides exceed one matrix.  Around an operand
    lies 16384 (finite: a kernel that zero-fills the other operand's tail multiplies it by zero, a kernel that lets it reach an output is
    off by thousands); an output window starts as NaN, and its pad columns, 512 guard rows before and after and the gaps between batch
    matrices hold a bit pattern that must survive.  A whole unguarded 384 x 256 tile store still lands inside the allocation: a missing
    bound is a failed assertion, never a fault.

check_window reports by region (last tile row, last tile column, pad columns, guard rows, every element) and names the worst element; the
tests at the end of this file feed it faulty copies and assert that each is rejected with the right region named.

bgemm_path / gemm_path restate the two dispatchers' predicates (conv.hip: try_cgemm, try_cgemm_dt, tt_ok, the `fast` condition, the three
split conditions, unet.bgemm's split_ws rules; gemm.hip: pick_fast_tile, launch_any, skinny_ok, shortk_ok) in plain Python.  They only LABEL
a case; test_every_*_path_is_reached keeps the tables honest: whoever moves a threshold learns which path lost its case."""
from types import SimpleNamespace

import pytest
import torch

BIG = 16384.0                  # around every operand window
GUARD_ROWS = 512
PATTERN = {1: (torch.uint8, 0x5A), 2: (torch.int16, 0x5A5A), 4: (torch.int32, 0x5A5AA5A5), 8: (torch.int64, 0x5A5AA5A55A5AA5A5)}
BF16, F32, F64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8
EPI_BF16, EPI_F32, EPI_GELU, EPI_GATE_RES, EPI_DGELU, EPI_POS, EPI_GELU_Q, EPI_DGELU_Q, EPI_QUICK_GELU = 0, 1, 2, 3, 4, 5, 7, 8, 9
EPI_NAME = {0: "bf16", 1: "f32", 2: "gelu", 3: "gate_res", 4: "dgelu", 5: "pos", 7: "gelu_q", 8: "dgelu_q", 9: "quick_gelu"}
# the bounds the project already holds the transcendental epilogues to (tests/test_gpu_gemm.py::test_epilogues, test_gelu_pair_with_the_
# derivative_as_one_byte; tests/test_gpu_text_encoder.py QGELU_TOL)
GELU_RTOL, GELU_ATOL = 1e-2, 1e-2
DGELU_RTOL, DGELU_ATOL = 1e-2, 2e-3
QGELU_TOL = 6.5e-3             # |c - ref| / (1 + |ref|)
GELUQ_CODE_TOL = 0.5 / 196.0 + 2e-4


# ------------------------------------------------------------------------------------------------ strided, guarded buffers
class Win:
    """batch x batch2 windows of rows x cols inside one flat allocation; element (z, z2, r, c) at base + z stride + z2 stride2 + r ld + c.
    kind "operand": 16384 everywhere outside the windows.  kind "output": NaN inside (or `prior`), the bit pattern outside."""

    def __init__(self, rows, cols, dtype, *, ld=None, off=8, batch=1, stride=None, batch2=1, stride2=None, kind="operand", guard_rows=GUARD_ROWS):
        ld = cols + 8 if ld is None else ld
        if stride2 is None:
            stride2 = (rows + 8) * ld
        if stride is None:
            stride = (rows + 8) * ld if batch2 == 1 else batch2 * max(stride2, (rows + 8) * ld) + 8 * ld
        self.rows, self.cols, self.ld, self.off, self.batch, self.stride, self.batch2, self.stride2 = rows, cols, ld, off, batch, stride, batch2, stride2
        self.dtype, self.kind = dtype, kind
        ar = torch.arange
        self.idx = (guard_rows * ld + off + ar(batch).view(-1, 1, 1, 1) * stride + ar(batch2).view(1, -1, 1, 1) * stride2
                    + ar(rows).view(1, 1, -1, 1) * ld + ar(cols).view(1, 1, 1, -1))
        self.base = guard_rows * ld + off
        self.lo = guard_rows * ld                                       # first element of the first window row
        self.hi = (int(self.idx.max()) // ld + 1) * ld                   # one past the last window row
        self.total = self.hi + guard_rows * ld
        self.full = torch.empty(self.total, dtype=dtype)
        self.es = self.full.element_size()
        if kind == "operand":
            self.full.fill_(BIG if dtype.is_floating_point else 1)
        else:
            idt, pat = PATTERN[self.es]
            self.full.view(idt).fill_(pat)
            self.full[self.idx] = float("nan") if dtype.is_floating_point else 255

    def _outside(self):
        outside = torch.ones(self.total, dtype=torch.bool)
        outside[self.idx] = False
        return outside

    @property
    def pad_mask(self):
        """outside the windows, between the first and the last window row (built when a checker asks: not held)"""
        outside = self._outside()
        outside[:self.lo] = False
        outside[self.hi:] = False
        return outside

    @property
    def guard_mask(self):
        outside = self._outside()
        outside[self.lo:self.hi] = False
        return outside

    def set(self, values):
        self.full[self.idx] = values.reshape(self.idx.shape).to(self.dtype)
        return self

    def window(self, full=None):
        return (self.full if full is None else full)[self.idx]

    def expected(self, ref):
        """the whole allocation as it must look after the launch: `ref` in the windows, everything else untouched"""
        e = self.full.clone()
        e[self.idx] = ref.reshape(self.idx.shape).to(self.dtype)
        return e

    @property
    def byte_offset(self):
        return self.base * self.es


def _worst(err, bound):
    over = err - bound
    w = int(over.argmax())
    return w, tuple(int(i) for i in torch.unravel_index(torch.tensor(w), err.shape)), int((over > 0).sum())


def _compare(got, ref, bound, what, origin=(0, 0)):
    """origin: (row, column) of the cut's first element inside the window, so that the element named is the window's"""
    got, ref = got.double(), ref.double()
    at = lambda i: tuple(int(v) for v in i[:-2]) + (int(i[-2]) + origin[0], int(i[-1]) + origin[1])
    bad = ~torch.isfinite(got)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {got.numel()} not written or non-finite; first at {at(bad.nonzero()[0])}"
    err = (got - ref).abs()
    bound = torch.as_tensor(bound, dtype=F64).expand_as(err)
    w, idx, n_over = _worst(err, bound)
    idx = at(idx)
    assert n_over == 0, (f"{what}: {n_over} of {got.numel()} elements out of bound; worst at {idx}: got {float(got.flatten()[w])!r}, "
                         f"want {float(ref.flatten()[w])!r}, bound {float(bound.flatten()[w]):.3e}")
    return float(err.max())


def check_window(win, got_full, ref, what, *, bound=0.0, tile=(128, 128)):
    """`got_full`: the whole allocation after the launch (CPU).  ref [batch][batch2][rows][cols] float64; bound 0 = exact, else a number or a
    tensor like ref.  Region by region: last tile row, last tile column, pad columns, guard rows, every element."""
    assert got_full.shape == win.full.shape and got_full.dtype == win.dtype, (what, got_full.shape, got_full.dtype)
    ref = ref.reshape(win.idx.shape).double()
    got = got_full[win.idx]
    bound = torch.as_tensor(bound, dtype=F64).expand_as(ref)
    r0, c0 = (win.rows - 1) // tile[0] * tile[0], (win.cols - 1) // tile[1] * tile[1]
    _compare(got[:, :, r0:], ref[:, :, r0:], bound[:, :, r0:], f"{what}: last tile row (rows {r0}..{win.rows - 1})", (r0, 0))
    _compare(got[..., c0:], ref[..., c0:], bound[..., c0:], f"{what}: last tile column (columns {c0}..{win.cols - 1})", (0, c0))
    idt = PATTERN[win.es][0]
    gb, wb = got_full.view(idt), win.full.view(idt)
    for name, mask in (("pad columns", win.pad_mask), ("guard rows", win.guard_mask)):
        ch = (gb != wb) & mask
        if bool(ch.any()):
            p = int(ch.nonzero()[0])
            rel = p - win.lo
            raise AssertionError(f"{what}: {name}: {int(ch.sum())} elements outside the window were overwritten; first at flat offset {p} "
                                 f"(row {rel // win.ld} of the first window row, column {rel % win.ld - win.off} of the window): {got_full[p].item()!r}")
    return _compare(got, ref, bound, f"{what}: every element")


def check(win, got_full, ref, what, **kw):
    """fast path for the exact case, on whatever device the tensors are: the whole allocation equals the expected image.  Otherwise the
    region report on the CPU."""
    b = kw.get("bound", 0.0)
    if isinstance(b, float) and b == 0.0:
        want = win.expected(ref).to(got_full.device)
        if torch.equal(got_full, want):        # (== on floats: +-0 agree, a NaN left in a window does not)
            return 0.0
    return check_window(win, got_full.cpu(), ref, what, **kw)


# ------------------------------------------------------------------------------------------------ data
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, *shape, lim=3):
    return torch.randint(-lim, lim + 1, shape, generator=g).double()


def quarters(g, *shape):
    return torch.randint(-8, 9, shape, generator=g).double() / 4


def bf16_round(x):
    """float64 (exact in fp32) -> bf16, rounded once to nearest even, as float64"""
    return x.float().to(BF16).double()


def gelu_tanh(x):
    return torch.nn.functional.gelu(x, approximate="tanh")


def gelu_tanh_grad(x):
    x = x.clone().requires_grad_(True)
    gelu_tanh(x).sum().backward()
    return x.grad


# ================================================================================================ sfron_bgemm_bf16
BMG, BNG, BK = 128, 128, 64


def split_scratch_slabs(mn):
    """unet._split_scratch: the slab count a caller hands over"""
    return min(64, max(2, (64 << 20) // (4 * mn)))


def unet_scratch(c):
    """unet.bgemm's split_ws rule: 0 = none, else split_ws_slabs"""
    plain = c.epi == "none"
    small_rows = (not c.a_t) and c.b_t and c.M <= 128 and c.K >= 4096 and plain
    if ((c.a_t and c.b_t and c.K >= 2048) or small_rows) and c.out == "f32" and c.batch == 1 and c.batch2 == 1 and c.packed:
        return split_scratch_slabs(c.M * c.N)
    if c.a_t and c.b_t and c.out == "bf16" and c.batch * c.batch2 > 1 and c.K >= 1024 and c.M <= 128 and c.N <= 256:
        return split_scratch_slabs(c.M * c.N * c.batch * c.batch2) * c.batch * c.batch2
    return 0


def plan_splits(M, N, K, cap):
    tiles = -(-M // BMG) * -(-N // BNG)
    return max(1, min(512 // max(tiles, 1), K // 512, cap))


def tt_tiles(np_, nq):
    return -(-np_ // 256) * -(-nq // 128)


def tt_splits(tiles, K, cap, out_elems):
    best, best_t = 1, 1e30
    lim = min(K // 512, cap)
    for sp in range(1, max(lim, 1) + 1):
        rounds = (tiles * sp + 255) // 256
        t = rounds * (K / sp) * (1.4 / 64.0) + (sp if sp > 1 else 0) * float(out_elems) * 2e-6
        if t < best_t:
            best_t, best = t, sp
    return best


def _chunks(K, sp):
    kchunk = -(-(-(-K // sp)) // BK) * BK
    return kchunk, -(-K // kchunk)


def bgemm_path(c):
    """(path name, k-tiles per workgroup of a pipelined kernel or 0, number of splits, contraction rows per split)"""
    bf, single = c.out == "bf16", c.batch == 1 and c.batch2 == 1
    slabs = unet_scratch(c) if c.scratch else 0
    plain = c.epi == "none" and c.packed
    M, N, K = c.M, c.N, c.K
    if not c.a_t and not c.b_t:
        if single and M % 256 == 0 and K % BK == 0:                          # try_cgemm
            return ("direct/pipelined160" if N % 160 == 0 else "direct/pipelined128"), K // BK, 1, K
        return ("direct/generic" if single else "direct/batched"), 0, 1, K
    if not c.a_t and c.b_t:
        if single and M % 256 == 0 and K % BK == 0 and N % 8 == 0:           # try_cgemm_dt
            return "dt/pipelined", K // BK, 1, K
        if not bf and slabs and single and plain and K >= 4096:
            tiles = -(-M // BMG) * -(-N // BNG)
            sp = min(256 // tiles, K // 512, slabs)
            if sp > 1:
                return "dt/split", 0, _chunks(K, sp)[1], _chunks(K, sp)[0]
        if single:
            return ("dt/deep-unsplit" if K >= 4096 else "dt/generic"), 0, 1, K
        return "dt/batched", 0, 1, K
    assert c.a_t and c.b_t
    tt_ok = K % BK == 0 and M % 8 == 0 and N % 8 == 0 and not bf
    fast = not bf and single and tt_ok and M >= 64 and N >= 64 and K >= 256
    if not bf and slabs and single and plain:
        sp = tt_splits(tt_tiles(M, N), K, slabs, M * N) if fast else plan_splits(M, N, K, slabs)
        if sp > 1:
            kchunk, used = _chunks(K, sp)
            return ("tt/fast-split" if fast else "tt/generic-split"), (kchunk // BK if fast else 0), used, kchunk
    if fast:
        return "tt/fast", K // BK, 1, K
    if bf and slabs and not single and c.epi == "none" and c.alpha == 1.0 and K >= 1024:
        tiles = -(-M // BMG) * -(-N // BNG) * c.batch * c.batch2
        sp = min(512 // tiles, K // 256, 16)
        per = c.batch * c.batch2 * M * N
        if sp * per > slabs * M * N:
            sp = slabs * M * N // per
        if sp > 1:
            return "tt/head-split", 0, _chunks(K, sp)[1], _chunks(K, sp)[0]
    return ("tt/generic" if single else "tt/batched"), 0, 1, K


BG_PATHS = ("direct/pipelined160", "direct/pipelined128", "direct/generic", "direct/batched", "dt/pipelined", "dt/generic", "dt/batched",
            "dt/split", "dt/deep-unsplit", "tt/fast", "tt/fast-split", "tt/generic", "tt/generic-split", "tt/head-split", "tt/batched")

# (output, epilogue, alpha): the cross products the callers use.  "full<r>" = bias + sample_vec + resid with rows_per_sample r
EPIS_ALL = (("f32", "none", 1.0), ("bf16", "none", 1.0), ("f32", "bias", 1.0), ("bf16", "bias", 1.0), ("f32", "full64", 1.0), ("f32", "full96", 1.0),
            ("f32", "full512", 1.0), ("f32", "acc", 1.0), ("f32", "none", 0.5), ("bf16", "bias", -2.0), ("f32", "full96", -2.0))
EPIS_F32 = tuple(e for e in EPIS_ALL if e[0] == "f32")
EPIS_BATCH = (("f32", "none", 1.0), ("bf16", "none", 1.0), ("f32", "bias", 1.0), ("bf16", "none", 0.5), ("f32", "acc", -2.0))
PLAIN_F32 = (("f32", "none", 1.0),)
PLAIN_BF16 = (("bf16", "none", 1.0),)

# (expected path, a_t, b_t, (M, N, K), (batch, batch2), layout of the batch or None, variants, through unet.bgemm with scratch, packed output)
_BG_TABLE = [
    ("direct/pipelined160", 0, 0, (256, 160, 64), (1, 1), None, EPIS_ALL, False, False),
    ("direct/pipelined160", 0, 0, (256, 160, 128), (1, 1), None, EPIS_ALL[:2], False, False),
    ("direct/pipelined160", 0, 0, (512, 320, 192), (1, 1), None, EPIS_ALL, False, False),
    ("direct/pipelined160", 0, 0, (256, 160, 256), (1, 1), None, EPIS_ALL[:2], False, False),
    ("direct/pipelined160", 0, 0, (512, 160, 512), (1, 1), None, EPIS_ALL, False, False),
    ("direct/pipelined128", 0, 0, (256, 200, 128), (1, 1), None, EPIS_ALL, False, False),
    ("direct/pipelined128", 0, 0, (256, 132, 64), (1, 1), None, EPIS_ALL, False, False),
    ("direct/pipelined128", 0, 0, (512, 4, 64), (1, 1), None, EPIS_ALL, False, False),
    ("direct/pipelined128", 0, 0, (256, 200, 192), (1, 1), None, EPIS_ALL[:2], False, False),
    ("direct/pipelined128", 0, 0, (256, 132, 256), (1, 1), None, EPIS_ALL[:2], False, False),
    ("direct/pipelined128", 0, 0, (256, 128, 576), (1, 1), None, EPIS_ALL, False, False),
    ("direct/generic", 0, 0, (96, 52, 72), (1, 1), None, EPIS_ALL, False, False),
    ("direct/generic", 0, 0, (264, 136, 40), (1, 1), None, EPIS_ALL, False, False),
    ("direct/batched", 0, 0, (48, 48, 64), (3, 2), "qk", EPIS_BATCH, False, False),
    ("dt/pipelined", 0, 1, (256, 72, 64), (1, 1), None, EPIS_ALL, False, False),
    ("dt/pipelined", 0, 1, (256, 72, 128), (1, 1), None, EPIS_ALL[:2], False, False),
    ("dt/pipelined", 0, 1, (512, 200, 192), (1, 1), None, EPIS_ALL, False, False),
    ("dt/pipelined", 0, 1, (256, 136, 256), (1, 1), None, EPIS_ALL[:2], False, False),
    ("dt/pipelined", 0, 1, (256, 136, 512), (1, 1), None, EPIS_ALL, False, False),
    ("dt/generic", 0, 1, (96, 72, 40), (1, 1), None, EPIS_ALL, False, False),
    ("dt/batched", 0, 1, (48, 64, 48), (3, 1), "plain", EPIS_BATCH, False, False),
    ("dt/split", 0, 1, (8, 136, 4096), (1, 1), None, PLAIN_F32, True, True),
    ("dt/deep-unsplit", 0, 1, (8, 136, 4096), (1, 1), None, EPIS_ALL[:4], False, False),
    ("tt/fast", 1, 1, (64, 64, 256), (1, 1), None, EPIS_F32, False, False),
    ("tt/fast", 1, 1, (264, 136, 512), (1, 1), None, EPIS_F32, False, False),
    ("tt/fast", 1, 1, (72, 328, 320), (1, 1), None, EPIS_F32, False, False),
    ("tt/fast-split", 1, 1, (320, 192, 2048), (1, 1), None, PLAIN_F32, True, True),
    ("tt/fast-split", 1, 1, (64, 72, 4096 + 64), (1, 1), None, PLAIN_F32, True, True),
    ("tt/generic", 1, 1, (56, 72, 192), (1, 1), None, EPIS_ALL, False, False),
    ("tt/generic", 1, 1, (8, 16, 40), (1, 1), None, EPIS_ALL, False, False),
    ("tt/generic", 1, 1, (264, 136, 512), (1, 1), None, (("bf16", "none", 1.0), ("bf16", "bias", -2.0)), False, False),   # bf16 out: not the fast tile
    ("tt/generic-split", 1, 1, (56, 72, 2048), (1, 1), None, PLAIN_F32, True, True),
    ("tt/head-split", 1, 1, (80, 40, 1024), (2, 3), "heads", PLAIN_BF16, True, False),
    ("tt/head-split", 1, 1, (80, 40, 1088), (2, 3), "heads", PLAIN_BF16, True, False),
    ("tt/batched", 1, 1, (48, 64, 48), (5, 1), "plain", EPIS_BATCH, False, False),
]


def _bg_cases():
    out = []
    for path, a_t, b_t, (M, N, K), (batch, batch2), blay, variants, scratch, packed in _BG_TABLE:
        for o, epi, alpha in variants:
            c = SimpleNamespace(path=path, a_t=a_t, b_t=b_t, M=M, N=N, K=K, batch=batch, batch2=batch2, blay=blay, out=o, epi=epi, alpha=alpha,
                                scratch=scratch, packed=packed)
            c.rps = int(epi[4:]) if epi.startswith("full") else 0
            c.id = f"{path}-{M}x{N}x{K}" + (f"-b{batch}x{batch2}" if batch * batch2 > 1 else "") + f"-{o}-{epi}" + (f"-a{alpha}" if alpha != 1 else "")
            c.seed = len(out) + 1
            out.append(c)
    return out


BG_CASES = _bg_cases()
BG_IDS = [c.id for c in BG_CASES]


def bg_problem(c):
    """buffers (host images) and float64 reference of one case, built from the case's seed when asked for and not held: the same every time"""
    g = _gen(c.seed)
    M, N, K, nb, nb2 = c.M, c.N, c.K, c.batch, c.batch2
    ar, ac = (K, M) if c.a_t else (M, K)               # A as stored
    br, bc = (K, N) if c.b_t else (N, K)
    p = SimpleNamespace(case=c)
    if c.blay == "qk":          # q and k as column slices of a [tokens][3 C] matrix, C = heads * K: lda = ldb = 3 C; heads step by K columns
        C3 = 3 * nb2 * K
        p.A = Win(ar, ac, BF16, ld=C3, off=8, batch=nb, batch2=nb2, stride2=K, stride=(ar + 8) * C3)
        p.B = Win(br, bc, BF16, ld=C3, off=8 + nb2 * K, batch=nb, batch2=nb2, stride2=K, stride=(br + 8) * C3)
    elif c.blay == "heads":     # dK / dV of the cross-attention: both operands [tokens][heads * width (+ pad)], heads are column slices
        p.A = Win(ar, ac, BF16, ld=nb2 * ac + 8, batch=nb, batch2=nb2, stride2=ac, stride=(ar + 8) * (nb2 * ac + 8))
        p.B = Win(br, bc, BF16, ld=nb2 * bc + 8, batch=nb, batch2=nb2, stride2=bc, stride=(br + 8) * (nb2 * bc + 8))
    else:
        p.A = Win(ar, ac, BF16, batch=nb, batch2=nb2)
        p.B = Win(br, bc, BF16, batch=nb, batch2=nb2)
    a, b = ints(g, nb, nb2, ar, ac), ints(g, nb, nb2, br, bc)
    p.A.set(a), p.B.set(b)
    am = a.transpose(-1, -2) if c.a_t else a
    bm = b if c.b_t else b.transpose(-1, -2)
    odt = F32 if c.out == "f32" else BF16
    ldc = N if c.packed else N + (4 if c.out == "f32" else 8)
    p.C = Win(M, N, odt, ld=ldc, off=0 if c.packed else 8, batch=nb, batch2=nb2, kind="output")
    ref = c.alpha * (am @ bm)
    p.absprod = abs(c.alpha) * (am.abs() @ bm.abs())
    p.addend = 0.0
    p.bias = p.vec = p.resid = None
    if c.epi == "bias" or c.rps:
        bias = quarters(g, N)
        p.bias = Win(1, N, F32).set(bias)
        ref = ref + bias
        p.addend += 2.0
    if c.rps:
        ns = -(-M // c.rps)
        vec, resid = quarters(g, ns, N), quarters(g, nb, nb2, M, N)
        p.vec = Win(ns, N, F32).set(vec)                   # ld_vec = N + 8
        p.resid = Win(M, N, F32, ld=ldc, batch=nb, batch2=nb2, stride=p.C.stride, stride2=p.C.stride2).set(resid)
        ref = ref + vec[torch.arange(M) // c.rps] + resid
        p.addend += 4.0
    if c.epi == "acc":
        prior = quarters(g, nb, nb2, M, N)
        p.C.set(prior)
        ref = ref + prior
        p.addend += 2.0
    p.ref = ref if c.out == "f32" else bf16_round(ref)
    p.exact = ref
    return p


# ================================================================================================ sfron_gemm_bf16
TILE_BM = (0, 128, 256, 256, 384, 192, 256, 192, 256)
TILE_BN = (0, 128, 192, 256, 192, 192, 192, 192, 144)
HINT_TILE = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 7: 7, 21: 2, 22: 2, 32: 2, 35: 5, 36: 6, 42: 2, 45: 5, 55: 5, 62: 8}
HINTS = tuple(HINT_TILE)
LAYOUTS = {"fwd": (0, 0), "dgrad": (0, 1), "wgrad": (1, 1)}


def tile_fits(M, N, t):
    return 1 <= t < 9 and M % TILE_BM[t] == 0 and N % TILE_BN[t] == 0


def pick_fast_tile(M, N, K, kchunk, force, tr):
    fits = lambda t: tile_fits(M, N, t)
    if K % 64 or force < 0:
        return 0
    if kchunk != K:
        if force in (32, 35):
            return force if fits(force - 30) else 0
        if force != 0:
            return 0
        if tr == 2 and fits(5):
            return 55
        if tr <= 1 and fits(2):
            return 42
        return 0
    # (21 / 22, the timing ablations of tile 2 that skip work, exist in the SFRON_DEBUG_KNOBS build only: here they fall to `force > 10`)
    if force in (32, 35, 36):
        return force if fits(force - 30) else 0
    if force in (42, 45):
        return force if fits(force - 40) else 0
    if force == 55:
        return force if fits(5) else 0
    if force == 62:
        return force if fits(8) else (42 if fits(2) else 0)
    if force > 10:
        return 0
    if force > 0:
        return force if fits(force) else 0

    def eff(t):
        tiles = (M // TILE_BM[t]) * (N // TILE_BN[t])
        return tiles / (((tiles + 255) // 256) * 256)
    if tr == 2:
        return 55 if fits(5) else 0
    if tr <= 1 and fits(8) and K % 192 == 0 and (not fits(2) or eff(8) > eff(2) + 0.05):
        return 62
    if fits(2) and eff(2) >= 0.5:
        return 42 if (tr == 1 or K % 128 == 0) else 2
    return 1 if (tr == 0 and fits(1)) else 0


def launch_any(M, N, K, kchunk, tr, epi, force, lw=4, bsum=False):
    """the kernel launch_any<A_TR, B_TR, EPI> ends at: 'generic', 'fast<tile>', 'pipe<tile>/s<schedule>[/nl4][/bsum]'"""
    t = pick_fast_tile(M, N, K, kchunk, force, tr)
    even = kchunk % 128 == 0 and K % kchunk == 0
    if 1 <= t <= 7:
        return f"fast{t}"
    if t in (32, 35, 36):
        return f"pipe{t - 30}/s0"
    if t in (42, 45):
        return f"pipe{t - 40}/s{1 if even else 0}"
    if t == 62:
        if (tr == 0 and epi in (EPI_BF16, EPI_F32, EPI_GELU, EPI_GATE_RES, EPI_POS)) or (tr == 1 and epi in (EPI_BF16, EPI_F32, EPI_DGELU)):
            if kchunk == K and K % 192 == 0:
                return "pipe8/s2/nl4" if (lw == 4 and tr == 1) else "pipe8/s2"
        if not tile_fits(M, N, 2):
            return "generic"
        return "pipe2/s1" if (K % 128 == 0 and kchunk == K) else "pipe2/s0"
    if t == 55:
        if tr == 2 and epi == EPI_F32 and bsum:
            return "pipe5/s2/bsum"
        if (tr == 2 and epi in (EPI_BF16, EPI_F32)) or (tr == 0 and epi == EPI_BF16):
            nk = kchunk // 64
            if K % kchunk == 0 and nk >= 2 and (nk - 2) % 3 == 0:
                return "pipe5/s2/nl4" if (tr == 2 and lw == 4) else "pipe5/s2"
        return f"pipe5/s{1 if even else 0}"
    return "generic"


def pipe_tile_order(ntm, ntn, fbm, fbn):
    """(tile row, tile column) of workgroup 0, 1, .. of a pipelined tile (gemm.hip launch_pipe's group_m and k_gemm_pipe's walk: consecutive
    workgroups go round the 8 XCDs, each XCD takes a run of ids, ids sweep group_m tile rows by all tile columns)"""
    nblk = ntm * ntn
    gm = 1
    while gm * 2 <= ntm and (gm * 2) * (gm * 2) * fbm <= nblk / 8.0 * fbn * 1.5:
        gm *= 2
    q, r, order = nblk >> 3, nblk & 7, []
    for b in range(nblk):
        x, y = b & 7, b >> 3
        i = (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + y
        first_m = i // (gm * ntn) * gm
        gsz = min(ntm - first_m, gm)
        order.append((first_m + i % (gm * ntn) % gsz, i % (gm * ntn) // gsz))
    return order


def gemm_path(c):
    tr = sum(LAYOUTS[c.layout])
    kchunk = c.K if c.split_k <= 1 else -(-(-(-c.K // c.split_k)) // BK) * BK
    tag = "/split" if kchunk != c.K else ""
    if c.epi in (EPI_GELU_Q, EPI_DGELU_Q):
        return "pipe2/s1/q"
    if c.epi == EPI_QUICK_GELU:
        return "fast1" if c.hint in (0, 1) and c.K % 64 == 0 and tile_fits(c.M, c.N, 1) else "generic"
    if c.epi == EPI_F32 and tr == 0 and c.hint == 0 and kchunk == c.K and not c.acc and c.M <= 32 and c.N % 16 == 0 and c.K % 32 == 0 and c.K <= 2048:
        return "skinny"
    if c.epi == EPI_POS and c.hint == 0 and c.K <= 32 and c.N % 16 == 0 and not c.acc:
        return "shortk"
    return launch_any(c.M, c.N, c.K, kchunk, tr, c.epi, c.hint, c.lw, c.rowsum) + tag


GEMM_PATHS = ("generic", "generic/split", "fast1", "fast2", "fast3", "fast4", "fast5", "fast6", "fast7", "pipe2/s0",
              "pipe5/s0", "pipe6/s0", "pipe2/s1", "pipe5/s1", "pipe5/s2", "pipe5/s2/nl4", "pipe5/s2/bsum", "pipe8/s2", "pipe8/s2/nl4", "pipe2/s1/split",
              "pipe2/s0/split", "pipe5/s2/nl4/split", "pipe5/s0/split", "pipe2/s1/q", "skinny", "shortk")


def G(group, M, N, K, layout="fwd", epi=EPI_F32, hint=0, *, alpha=1.0, bias=False, acc=False, tokens=1, sep_resid=False, split_k=1, lw=4,
      rowsum=False, sumsq=None, colpart=False, ldpad=4, scaled=False, finish=None, deep=False):
    """one sfron_gemm_bf16 launch.  sumsq: None / 'all' / 'mask'; finish (split_k > 1, packed slabs): 'reduce' / 'sum_bf16' / 'gate_res';
    scaled: unit-scale random operands for the three transcendental epilogues (their existing bounds), else integers;
    deep (EPI_DGELU): the integer pre-activations in `aux` span -12 .. 12, past x = -10.06 where exp2 of the sigmoid's argument overflows"""
    c = SimpleNamespace(group=group, M=M, N=N, K=K, layout=layout, epi=epi, hint=hint, alpha=alpha, bias=bias, acc=acc, tokens=tokens,
                        sep_resid=sep_resid, split_k=split_k, lw=lw, rowsum=rowsum, sumsq=sumsq, colpart=colpart, ldpad=ldpad, scaled=scaled,
                        finish=finish, deep=deep)
    c.path = gemm_path(c)
    c.id = (f"{group}-{M}x{N}x{K}-{layout}-{EPI_NAME[epi]}-h{hint}" + (f"-a{alpha}" if alpha != 1 else "") + ("-bias" if bias else "") +
            ("-acc" if acc else "") + (f"-t{tokens}" if tokens != 1 else "") + ("-resid" if sep_resid else "") + (f"-s{split_k}" if split_k > 1 else "") +
            (f"-lw{lw}" if lw != 4 else "") + ("-rowsum" if rowsum else "") + (f"-sumsq_{sumsq}" if sumsq else "") + ("-colpart" if colpart else "") +
            (f"-ld{ldpad}" if ldpad != 4 else "") + ("-scaled" if scaled else "") + (f"-{finish}" if finish else "") +
            ("-deep" if deep else ""))
    return c


def _gemm_cases():
    cs = []
    # ---- the generic kernel, ragged in every dimension (wgrad needs M % 8, a transposed B needs N % 8: (8, 8, 8) there)
    for (M, N, K) in ((96, 160, 72), (136, 52, 40), (8, 4, 8)):
        for lay in LAYOUTS:
            n = N if lay == "fwd" else (N + 7) // 8 * 8
            cs += [G("generic", M, n, K, lay, EPI_BF16, -1), G("generic", M, n, K, lay, EPI_BF16, -1, bias=True, alpha=-2.0, ldpad=8),
                   G("generic", M, n, K, lay, EPI_F32, -1), G("generic", M, n, K, lay, EPI_F32, -1, bias=True),
                   G("generic", M, n, K, lay, EPI_F32, -1, acc=True), G("generic", M, n, K, lay, EPI_F32, -1, alpha=0.5, bias=True, acc=True)]
        for tok in (24, 64, 200):
            cs += [G("generic", M, N, K, "fwd", EPI_GATE_RES, -1, bias=True, tokens=tok), G("generic", M, N, K, "fwd", EPI_GATE_RES, -1, tokens=tok, sep_resid=True)]
        cs += [G("generic", M, N, K, "fwd", EPI_POS, -1, bias=True, tokens=24), G("generic", M, N, K, "fwd", EPI_POS, -1, tokens=8)]
        n8 = (N + 7) // 8 * 8
        for sc in (False, True):
            cs += [G("generic", M, N, K, "fwd", EPI_GELU, -1, bias=True, scaled=sc), G("generic", M, n8, K, "dgrad", EPI_DGELU, -1, scaled=sc),
                   G("generic", M, N, K, "fwd", EPI_QUICK_GELU, -1, bias=True, scaled=sc)]
    # ---- every tile hint the dispatcher accepts: 3 x 2 tiles; every K of the set (the label says which schedule each K gets, and where
    # the hint falls back); a shape the tile does not fit must take the generic kernel
    for h in HINTS:
        t = HINT_TILE[h]
        M, N = 3 * TILE_BM[t], 2 * TILE_BN[t]
        for lay in LAYOUTS:
            for i, K in enumerate((64, 128, 192, 320, 384, 576)):
                for epi in (EPI_F32, EPI_BF16):
                    cs.append(G("hint", M, N, K, lay, epi, h, ldpad=8 if i % 2 else 4))
            cs.append(G("hint-misfit", M + 8, N + 8, 64, lay, EPI_F32, h))
    # ---- the automatic choices
    for lay in ("fwd", "dgrad"):
        cs += [G("auto", 256, 144, 192, lay, EPI_F32), G("auto", 256, 144, 192, lay, EPI_BF16, bias=True), G("auto", 256, 144, 192, lay, EPI_BF16, lw=0, ldpad=8),
               G("auto", 256, 192, 128, lay, EPI_F32, bias=True), G("auto", 256, 192, 128, lay, EPI_BF16, ldpad=8),
               G("auto", 256, 192, 192, lay, EPI_F32), G("auto", 256, 192, 192, lay, EPI_BF16, bias=True)]
    cs += [G("auto", 192, 192, 128, "wgrad", EPI_F32), G("auto", 192, 192, 128, "wgrad", EPI_F32, lw=0), G("auto", 192, 192, 128, "wgrad", EPI_F32, acc=True, alpha=0.5),
           G("auto", 192, 192, 320, "wgrad", EPI_F32), G("auto", 192, 192, 320, "wgrad", EPI_F32, lw=0), G("auto", 192, 192, 320, "wgrad", EPI_BF16),
           G("auto", 192, 192, 320, "wgrad", EPI_F32, rowsum=True), G("auto", 192, 192, 320, "wgrad", EPI_F32, sumsq="all"),
           G("auto", 192, 192, 320, "wgrad", EPI_F32, sumsq="mask"), G("auto", 384, 192, 128, "wgrad", EPI_F32, sumsq="mask", alpha=0.5),
           G("auto", 768, 576, 128, "wgrad", EPI_F32, sumsq="mask"),             # 4 x 3 tiles: more than 8, so the walk over the XCDs reorders them
           G("auto", 128, 128, 64, "fwd", EPI_F32, bias=True), G("auto", 128, 128, 64, "fwd", EPI_BF16),
           G("auto", 32, 48, 64, "fwd", EPI_F32, bias=True), G("auto", 5, 16, 32, "fwd", EPI_F32), G("auto", 32, 48, 64, "fwd", EPI_F32, alpha=-2.0),
           G("auto", 96, 48, 16, "fwd", EPI_POS, bias=True, tokens=32), G("auto", 96, 48, 16, "fwd", EPI_POS, tokens=32, alpha=0.5),
           G("auto", 256, 192, 128, "dgrad", EPI_DGELU), G("auto", 256, 192, 128, "dgrad", EPI_DGELU, scaled=True, ldpad=8),
           # GELU' of pre-activations down to -12 in each of the three kernels that form it: generic, 128 x 128 tile, pipelined tile
           G("auto", 96, 160, 72, "dgrad", EPI_DGELU, -1, deep=True), G("auto", 256, 128, 64, "dgrad", EPI_DGELU, 1, deep=True),
           G("auto", 256, 192, 128, "dgrad", EPI_DGELU, 42, deep=True, ldpad=8),
           # the 256 x 192 tile is chosen by itself only where it fills half a round of 256 CUs: 128 tiles are the smallest such product
           G("auto", 2048, 3072, 128, "fwd", EPI_F32, bias=True), G("auto", 2048, 3072, 192, "fwd", EPI_BF16, ldpad=8),
           G("auto", 2048, 3072, 128, "dgrad", EPI_DGELU, colpart=True),
           G("auto", 256, 192, 128, "fwd", EPI_GELU, bias=True), G("auto", 256, 192, 128, "fwd", EPI_GELU, bias=True, scaled=True, ldpad=8),
           G("auto", 256, 192, 128, "fwd", EPI_GELU_Q, bias=True, ldpad=8), G("auto", 256, 192, 128, "fwd", EPI_GELU_Q, bias=True, ldpad=8, scaled=True),
           G("auto", 256, 192, 128, "dgrad", EPI_DGELU_Q, ldpad=8), G("auto", 256, 192, 128, "dgrad", EPI_DGELU_Q, ldpad=8, scaled=True),
           G("auto", 128, 128, 64, "fwd", EPI_QUICK_GELU, bias=True), G("auto", 128, 128, 64, "fwd", EPI_QUICK_GELU, bias=True, scaled=True)]
    # ---- split-K slabs, uneven last split: strided slabs checked one by one, packed slabs through the three finish kernels
    for (M, N, K, lay, S, h) in ((256, 192, 1024 + 128, "fwd", 4, 0), (256, 192, 1024 + 128, "dgrad", 4, 0), (256, 192, 1024 + 64, "fwd", 4, 0),
                                 (256, 192, 1024, "dgrad", 4, 0), (192, 192, 1280, "wgrad", 4, 0),
                                 (192, 192, 1024 + 128, "wgrad", 4, 0), (192, 192, 1024 + 64, "wgrad", 4, 0), (192, 192, 512, "wgrad", 3, 35),
                                 (136, 56, 1024 + 72, "fwd", 4, 0), (136, 56, 1024 + 64, "dgrad", 3, 0), (136, 56, 1024 + 64, "wgrad", 8, 0)):
        cs += [G("split", M, N, K, lay, EPI_F32, h, split_k=S), G("split", M, N, K, lay, EPI_F32, h, split_k=S, finish="reduce", ldpad=0)]
        if lay != "wgrad":
            cs.append(G("split", M, N, K, lay, EPI_F32, h, split_k=S, finish="sum_bf16", ldpad=0))
        if lay == "fwd":
            cs += [G("split", M, N, K, lay, EPI_F32, h, split_k=S, finish="gate_res", ldpad=0, tokens=64, bias=True),
                   G("split", M, N, K, lay, EPI_F32, h, split_k=S, finish="gate_res", ldpad=0, tokens=40)]
    # ---- the linear epilogues through tiles 1, 42, 62 and the generic kernel: tokens a multiple of the tile height, and not
    for (M, N, K, h) in ((256, 128, 64, 1), (512, 192, 128, 42), (512, 144, 192, 62), (512, 144, 192, -1)):
        bm = 128 if h == 1 else 256
        for tok in (bm, 2 * bm, 64, 200):
            cs += [G("linear", M, N, K, "fwd", EPI_GATE_RES, h, bias=True, tokens=tok), G("linear", M, N, K, "fwd", EPI_GATE_RES, h, tokens=tok, sep_resid=True, ldpad=8),
                   G("linear", M, N, K, "fwd", EPI_POS, h, bias=True, tokens=tok)]
    for i, c in enumerate(cs):
        c.seed = 1000 + i
    return cs


GEMM_CASES = _gemm_cases()
GEMM_IDS = [c.id for c in GEMM_CASES]


def colpart_bound(ref_terms):
    """a column partial is an fp32 sum over 256 rows of values each held to DGELU_RTOL |ref| + DGELU_ATOL"""
    return DGELU_RTOL * ref_terms.abs().sum(0) + DGELU_ATOL * ref_terms.shape[0]


def gemm_problem(c):
    """buffers (host images) and float64 references of one case, built from the case's seed when asked for and not held.
    p.outs: name -> (Win, ref, bound: 0 = exact, or a tensor)"""
    g = _gen(c.seed)
    M, N, K = c.M, c.N, c.K
    a_t, b_t = LAYOUTS[c.layout]
    p = SimpleNamespace(case=c, outs={}, ins={})
    if c.scaled:      # the scales of test_epilogues / test_gemm_quick_gelu_vs_torch: unit activations, weights ~ K^-1/2
        a = torch.randn((K, M) if a_t else (M, K), generator=g).to(BF16).double()
        b = (torch.randn((K, N) if b_t else (N, K), generator=g) * K ** -0.5).to(BF16).double()
    else:
        a, b = ints(g, *((K, M) if a_t else (M, K))), ints(g, *((K, N) if b_t else (N, K)))
    p.A, p.B = Win(*a.shape, BF16).set(a), Win(*b.shape, BF16).set(b)
    am, bm = (a.t() if a_t else a), (b if b_t else b.t())
    p.am, p.bm = am, bm
    res = c.alpha * (am @ bm)
    p.absprod, p.addend, p.gmax = abs(c.alpha) * (am.abs() @ bm.abs()), 0.0, 1.0
    p.bias = None
    if c.bias:
        bias = quarters(g, N) if not c.scaled else (torch.randn(N, generator=g) * 0.1).float().double()
        p.bias = Win(1, N, F32).set(bias)
        res = res + bias
        p.addend += 2.0
    ldf = ldb_ = N + c.ldpad
    ldx = ldf + 8                                                   # ldaux differs from ldc
    off = 8 if c.ldpad else 0
    out = lambda dt, ld, **kw: Win(M, N, dt, ld=ld, off=2 * off if dt is U8 else off, kind="output", **kw)      # (16-byte aligned in every type)
    e = c.epi
    if c.split_k > 1:
        kchunk = -(-(-(-K // c.split_k)) // BK) * BK
        used = -(-K // kchunk)
        slabs = torch.stack([am[:, s * kchunk:(s + 1) * kchunk] @ bm[s * kchunk:(s + 1) * kchunk] for s in range(used)]) * c.alpha
        p.used = used
        # (packed slabs lie M N apart, as the callers of the finish kernels keep them; strided ones leave a gap of guard rows)
        p.C = Win(M, N, F32, ld=ldf, off=off, batch=used, stride=(M + 8) * ldf if c.ldpad else M * N, kind="output")
        p.outs["slabs"] = (p.C, slabs, 0.0)
        total = slabs.sum(0)
        if c.finish == "reduce":
            p.fin = {"out": (Win(M, N, F32, ld=N, off=0, kind="output"), total, 0.0)}
        elif c.finish == "sum_bf16":
            p.fin = {"out": (Win(M, N, BF16, ld=N, off=0, kind="output"), bf16_round(total), 0.0)}
        elif c.finish == "gate_res":
            ns = -(-M // c.tokens)
            bias2 = quarters(g, N) if c.bias else None          # (the GEMM itself takes no bias when split: the finish adds it)
            gate, resid = ints(g, ns, N, lim=2), quarters(g, M, N)
            v = total + (bias2 if c.bias else 0.0)
            p.ins["gate"] = Win(ns, N, F32, ld=6 * N, off=2 * N).set(gate)
            p.ins["resid"] = Win(M, N, F32, ld=N, off=0).set(resid)
            p.ins["bias2"] = Win(1, N, F32).set(bias2) if c.bias else None
            p.fin = {"out": (Win(M, N, F32, ld=N, off=0, kind="output"), resid + gate[torch.arange(M) // c.tokens] * v, 0.0),
                     "branch": (Win(M, N, BF16, ld=N, off=0, kind="output"), bf16_round(v), 0.0)}
            p.gmax, p.addend = 2.0, p.addend + 4.0
        return p
    if e == EPI_BF16:
        p.outs["c_bf16"] = (out(BF16, ldb_), bf16_round(res), 0.0)
    elif e == EPI_F32:
        w = out(F32, ldf)
        if c.acc:
            prior = quarters(g, M, N)
            w.set(prior)
            res = res + prior
            p.addend += 2.0
        p.outs["c_f32"] = (w, res, 0.0)
        if c.rowsum:
            p.outs["a_rowsum"] = (Win(1, M, F32, ld=M, off=0, kind="output"), am.sum(1), 0.0)
        if c.sumsq:
            nt = (M // 192) * (N // 192)
            mask = torch.ones(M, N, dtype=U8) if c.sumsq == "all" else (torch.rand(M, N, generator=g) < 0.5).to(U8)
            if c.sumsq == "mask":
                p.ins["mask"] = Win(M, N, U8, ld=ldf, off=off).set(mask)      # same layout as c_f32
            sq = (res * mask.double()) ** 2
            # one partial per 192 x 192 tile, partial b from the tile that workgroup b of the grouped walk computes
            p.sumsq_tiles = sq.reshape(M // 192, 192, N // 192, 192).sum((1, 3))
            order = pipe_tile_order(M // 192, N // 192, 192, 192)
            p.outs["sumsq_partials"] = (Win(1, nt, F64, ld=nt, off=0, kind="output"), torch.stack([p.sumsq_tiles[tm, tn] for tm, tn in order]), 0.0)
    elif e in (EPI_GELU, EPI_GELU_Q):
        act = gelu_tanh(res)
        p.outs["c_bf16"] = (out(BF16, ldb_), act, GELU_RTOL * act.abs() + GELU_ATOL)
        if e == EPI_GELU:
            p.outs["aux"] = (out(BF16, ldx), bf16_round(res), 0.0) if not c.scaled else (out(BF16, ldx), res, GELU_RTOL * res.abs() + GELU_ATOL)
        else:
            # (the integer run has pre-activations far below -10.06, where exp2 of the sigmoid's argument overflows: GELU' is 0 there, code 29)
            p.outs["aux"] = (out(U8, ldx), (gelu_tanh_grad(res) + 0.15) * 196.0, GELUQ_CODE_TOL * 196.0)
    elif e == EPI_GATE_RES:
        ns = -(-M // c.tokens)
        gate, resid = ints(g, ns, N, lim=2), quarters(g, M, N)
        p.ins["gate"] = Win(ns, N, F32, ld=6 * N, off=2 * N).set(gate)
        w = out(F32, ldf)
        if c.sep_resid:
            p.ins["resid"] = Win(M, N, F32, ld=ldf, off=off).set(resid)
        else:
            w.set(resid)
        p.outs["c_f32"] = (w, resid + gate[torch.arange(M) // c.tokens] * res, 0.0)
        p.outs["aux"] = (out(BF16, ldx), bf16_round(res), 0.0)
        p.gmax, p.addend = 2.0, p.addend + 2.0
    elif e in (EPI_DGELU, EPI_DGELU_Q):
        if e == EPI_DGELU:
            pre = ints(g, M, N, lim=12 if c.deep else 3) if not c.scaled else torch.randn(M, N, generator=g).to(BF16).double()
            p.ins["aux"] = Win(M, N, BF16, ld=ldx, off=off).set(pre)
            gp = gelu_tanh_grad(pre)
            atol = DGELU_ATOL
        else:
            codes = torch.randint(0, 252, (M, N), generator=g)
            p.ins["aux"] = Win(M, N, U8, ld=ldx, off=2 * off).set(codes)
            gp = codes.double() / 196.0 - 0.15           # decoded exactly: only the bf16 rounding of the product remains
            atol = DGELU_ATOL
        want = res * gp
        p.outs["c_bf16"] = (out(BF16, ldb_), want, DGELU_RTOL * want.abs() + atol)
        if c.colpart:
            rows = M // 256
            p.outs["col_partials"] = (Win(rows, N, F32, ld=N, off=0, kind="output"), want.reshape(rows, 256, N).sum(1),
                                      torch.stack([colpart_bound(want[r * 256:(r + 1) * 256]) for r in range(rows)]))
    elif e == EPI_POS:
        pos = quarters(g, c.tokens, N)
        p.ins["pos"] = Win(c.tokens, N, F32, ld=N, off=0).set(pos)         # pos is packed [tokens][N] by definition
        p.outs["c_f32"] = (out(F32, ldf), res + pos[torch.arange(M) % c.tokens], 0.0)
        p.addend += 2.0
    elif e == EPI_QUICK_GELU:
        want = res * torch.sigmoid(1.702 * res)
        p.outs["c_bf16"] = (out(BF16, ldb_), want, QGELU_TOL * (1 + want.abs()))
    else:
        raise ValueError(e)
    return p


# ================================================================================================ the CPU tests
def test_every_bgemm_path_is_reached_and_labelled():
    seen, uneven = {}, set()
    for c in BG_CASES:
        path, nk, splits, kchunk = bgemm_path(c)
        if splits > 1 and c.K % kchunk:
            uneven.add(path)
        assert path == c.path, f"{c.id}: the table says {c.path}, the dispatcher's predicates say {path}"
        seen.setdefault(path, []).append((c, nk, splits))
        if c.scratch:
            assert unet_scratch(c) > 0 and splits > 1, f"{c.id}: unet.bgemm would not arm the scratch / the product would not split"
    missing = [p for p in BG_PATHS if p not in seen]
    assert not missing, f"no case reaches {missing}"
    # the pipelined kernels at 1, 2, 3, 4 and >= 8 k-tiles (three-slot prologue = whole loop, ring wrap, loader-wave form at nk >= 8)
    for path, need in (("direct/pipelined160", {1, 2, 3, 4}), ("direct/pipelined128", {1, 2, 3, 4}), ("dt/pipelined", {1, 2, 3, 4}), ("tt/fast", {4})):
        nks = {nk for _, nk, _ in seen[path]}
        assert need <= nks and max(nks) >= 8, (path, sorted(nks))
    assert any(nk >= 8 for _, nk, _ in seen["tt/fast-split"])
    # an uneven last split on each split route
    assert {"tt/fast-split", "tt/head-split"} <= uneven, uneven
    for r in (64, 96, 512):
        assert any(c.rps == r for c in BG_CASES)
    assert {c.alpha for c in BG_CASES} == {1.0, 0.5, -2.0}


def test_every_gemm_path_is_reached_and_labelled():
    seen = {c.path for c in GEMM_CASES}
    missing = [p for p in GEMM_PATHS if p not in seen]
    assert not missing, f"no case reaches {missing}"
    by = lambda **kw: [c for c in GEMM_CASES if all(getattr(c, k) == v for k, v in kw.items())]
    for h in HINTS:                                  # every hint reaches its own tile, and the generic kernel where the tile does not fit
        own = {c.path for c in by(group="hint", hint=h)}
        t = HINT_TILE[h]
        if h in (21, 22):        # accepted, and the generic kernel's result: the ablation kernels are not in the product build
            assert own == {"generic"}, (h, own)
            continue
        assert any(p.startswith(f"fast{t}") or p.startswith(f"pipe{t}") for p in own), (h, own)
        assert {c.path for c in by(group="hint-misfit", hint=h)} == {"generic"}, h
    # the automatic choices the issue names
    want = {(256, 144, 192, "fwd"): "pipe8/s2", (256, 144, 192, "dgrad"): "pipe8/s2/nl4", (256, 192, 128, "fwd"): "generic", (256, 192, 192, "fwd"): "generic",
            (256, 192, 128, "dgrad"): "generic", (256, 192, 192, "dgrad"): "generic",
            (2048, 3072, 128, "fwd"): "pipe2/s1", (192, 192, 128, "wgrad"): "pipe5/s2/nl4", (192, 192, 320, "wgrad"): "pipe5/s2/nl4", (128, 128, 64, "fwd"): "fast1",
            (32, 48, 64, "fwd"): "skinny", (5, 16, 32, "fwd"): "skinny"}
    for (M, N, K, lay), path in want.items():
        got = {c.path for c in by(group="auto", M=M, N=N, K=K, layout=lay, epi=EPI_F32, lw=4, rowsum=False, acc=False)}
        assert got == {path}, ((M, N, K, lay), got, path)
    assert {c.path for c in by(group="auto", epi=EPI_POS)} == {"shortk"}
    assert {c.path for c in by(rowsum=True)} == {"pipe5/s2/bsum"} and {c.path for c in by(colpart=True)} == {"pipe2/s1"}
    assert {c.path for c in by(group="auto", M=2048, K=192)} == {"fast2"}
    assert [c.path for c in by(deep=True)] == ["generic", "fast1", "pipe2/s1"]
    for ntm, ntn in ((1, 1), (2, 1), (4, 3), (5, 16), (16, 12)):       # the walk visits every tile once
        assert sorted(pipe_tile_order(ntm, ntn, 192, 192)) == [(m, n) for m in range(ntm) for n in range(ntn)]
    assert pipe_tile_order(4, 3, 192, 192) != sorted(pipe_tile_order(4, 3, 192, 192))
    for tok_case in by(group="linear"):
        assert tok_case.path in ("fast1", "pipe2/s1", "pipe8/s2", "generic"), tok_case.id
    assert len(set(GEMM_IDS)) == len(GEMM_IDS) and len(set(BG_IDS)) == len(BG_IDS)


def test_results_are_exact_in_fp32():
    """the precondition of 'no tolerance': every result and every partial sum of it, in any order, is a multiple of 1/8 (operands integers,
    alpha >= 1/2 in steps of 1/2, addends multiples of 1/4, gate an integer) whose magnitude is below max row sum of |A| |B| x |alpha| x |gate|
    + the addends -- and 8 x that bound is below 2^24, so fp32 holds every one of them exactly.  Runs every reference once."""
    worst = 0.0
    for c in BG_CASES:
        p = bg_problem(c)
        bound = float(p.absprod.max()) + p.addend
        assert float(p.exact.abs().max()) <= bound and bound * 8 < 2 ** 24, (c.id, bound)
        assert bool((p.exact * 8 == (p.exact * 8).round()).all()), c.id
        assert p.A.ld % 8 == 0 and p.B.ld % 8 == 0 and p.C.ld % 4 == 0 and (c.packed or p.C.ld > c.N), c.id
        worst = max(worst, bound)
    for c in GEMM_CASES:
        p = gemm_problem(c)
        if c.scaled:
            continue
        bound = float(p.absprod.max()) * p.gmax + p.addend
        assert bound * 8 < 2 ** 24, (c.id, bound)
        worst = max(worst, bound)
        for name, (w, ref, tol) in list(p.outs.items()) + list(getattr(p, "fin", {}).items()):
            if ref is None or not (isinstance(tol, float) and tol == 0.0) or w.dtype is BF16:
                continue
            if name == "sumsq_partials":
                assert torch.equal(ref.sort().values, p.sumsq_tiles.flatten().sort().values), c.id
                continue
            assert float(ref.abs().max()) <= bound and bool((ref * 8 == (ref * 8).round()).all()), (c.id, name)
        if c.sumsq:        # squares of multiples of 1/2, summed over a tile in fp64: exact far below 2^53
            assert float(p.sumsq_tiles.max()) * 4 < 2 ** 53 and bool((p.sumsq_tiles * 4 == (p.sumsq_tiles * 4).round()).all())
            # (the kernel adds a lane's 3 x 6 x 4 = 72 squares in fp32 before it widens: integers, or multiples of 1/4 under alpha = 1/2, whose sum stays exact)
            q2 = 4 if c.alpha == 0.5 else 1
            assert 72 * float(p.outs["c_f32"][1].abs().max()) ** 2 * q2 < 2 ** 24, c.id
    print(f"largest magnitude bound of any case: {worst:.0f} (x 8 = {worst * 8:.0f} < 2^24 = {2 ** 24})")


# ---- the checkers: a correct tensor passes, each kind of fault is rejected with its region named
def _demo(dtype=F32):
    g = _gen(7)
    w = Win(200, 136, dtype, ld=140, batch=2, kind="output")
    ref = ints(g, 2, 1, 200, 136, lim=40)
    return w, ref, w.expected(ref)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_checker_accepts_a_correct_output(dtype):
    w, ref, good = _demo(dtype)
    assert check(w, good, ref, "demo") == 0.0
    assert check_window(w, good, ref, "demo") == 0.0
    assert check_window(w, good, ref + 0.25 * (dtype is BF16), "demo", bound=0.5) <= 0.5


@pytest.mark.parametrize("where,region", [((0, 0, 5, 7), "every element"), ((1, 0, 199, 3), "last tile row"), ((0, 0, 3, 135), "last tile column"),
                                           ((1, 0, 128, 128), "last tile row")])
def test_checker_rejects_one_element_off_by_one(where, region):
    w, ref, good = _demo()
    bad = good.clone()
    bad[w.idx[where]] += 1.0
    with pytest.raises(AssertionError, match=region) as e:
        check(w, bad, ref, "demo")
    assert str(where) in str(e.value)           # the worst element is named
    bad = good.clone()
    bad[w.idx[where]] = float("nan")            # ... and an element the kernel never wrote
    with pytest.raises(AssertionError, match=region):
        check(w, bad, ref, "demo")


def test_checker_rejects_a_changed_guard_element_and_a_pad_column():
    w, ref, good = _demo()
    for pos, region in ((3, "guard rows"), (w.total - 1, "guard rows"), (w.lo - 1, "guard rows"), (w.hi, "guard rows"),
                        (int(w.idx[0, 0, 10, 135]) + 1, "pad columns"), (int(w.idx[1, 0, 0, 0]) - 1, "pad columns"),
                        (int(w.idx[0, 0, 199, 0]) + w.ld, "pad columns")):          # the gap between two batch matrices
        bad = good.clone()
        bad[pos] = 0.0
        with pytest.raises(AssertionError, match=region):
            check(w, bad, ref, "demo")
        bad = good.clone()
        bad.view(torch.int32)[pos] ^= 1                                                # one bit
        with pytest.raises(AssertionError, match=region):
            check(w, bad, ref, "demo")


def test_checker_rejects_a_value_that_includes_a_pad_column_product():
    """an operand's pad holds 16384: one product of it with the smallest non-zero operand value moves an output by 16384"""
    w, ref, good = _demo()
    for where, region in (((0, 0, 64, 130), "last tile column"), ((1, 0, 192, 0), "last tile row"), ((1, 0, 17, 64), "every element")):
        bad = good.clone()
        bad[w.idx[where]] += BIG * 1.0
        with pytest.raises(AssertionError, match=region):
            check(w, bad, ref, "demo")
    # and under the loosest tolerance any output here has, it is still thousands of bounds away
    with pytest.raises(AssertionError, match="every element"):
        check(w, bad, ref, "demo", bound=GELU_RTOL * ref.abs() + GELU_ATOL)


def test_operand_windows_are_surrounded_by_large_finite_values():
    p = bg_problem(BG_CASES[0])
    for w in (p.A, p.B):
        outside = torch.ones(w.total, dtype=torch.bool)
        outside[w.idx] = False
        assert bool((w.full[outside].float() == BIG).all()) and float(w.window().abs().max()) <= 3
        assert w.total - w.hi >= 512 * w.ld and w.lo >= 512 * w.ld and w.byte_offset % 16 == 0
    assert bool(torch.isnan(p.C.window()).all()) and p.C.total - p.C.hi >= 384 * p.C.ld + 256
