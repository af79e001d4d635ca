"""GPU parity of every scheduling path of the optimizer sweep (sweep.py FlatAdam.step, csrc/sweep.hip).

The arithmetic of the sweep is per element and independent of the grid (adam_one / ema_one, library built with -ffp-contract=off), so
every path that uses the same clip coefficient must leave THE SAME BITS as the plain one-launch sweep.  The plain sweep in turn is
held to torch.optim.AdamW + clip_grad_norm_ + the two EMA forms on the CPU (section A).  No model: one synthetic arena of 200 003
floats laid out like a DiT arena in miniature.

  A  the plain path against torch where test_gpu_sweep_loss.py does not pin it: weight decay, g2, the in-sweep EMA forms, mask
     bytes other than 0/1, refused arguments
  B  sfron_masked_clip_adam_wg, ranges=, split= (head / stream / max_workgroups / defer / ada_side / quant), pipeline=, lowrank,
     fused_sumsq against the plain sweep, bit for bit
  C  sfron_clip_coef, sfron_sumsq_masked, sfron_fisher_accum_clipped, sfron_cast_bf16 on their own
"""
import collections
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")

# ---- the arena: embedders | one low-rank matrix | six blocks of three tensors | a final layer whose length is no multiple of 4
N = 200_003
EMB = (0, 10_000)
NM, D, R = 64, 128, 5                                   # R = 5: the tail of the 8-row trip of lowrank_grad is live
ADA = (EMB[1], EMB[1] + NM * D)                         # [10 000, 18 192)
BLOCK = 24_576
BLOCKS = [(ADA[1] + i * BLOCK, ADA[1] + (i + 1) * BLOCK) for i in range(6)]
REST = (BLOCKS[-1][1], N)                               # 34 355 elements: the scalar tail of the kernels is live
_TLEN = (12_288, 8_196, 4_092)                          # three tensors per block, multiples of 4 (sfron_masked_clip_adam_q)
TENSORS = [[(lo + sum(_TLEN[:j]), lo + sum(_TLEN[:j + 1]), 3 * i + j) for j in range(3)] for i, (lo, _) in enumerate(BLOCKS)]
SAT = 10                                                # the tensor whose e4m3 scale makes most of it saturate at 448
SCALES = [2.0 ** (12 if si == SAT else si - 10) for si in range(18)]      # distinct powers of two: a wrong scale index shows
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
KEYS = ("p", "m", "v", "ema", "wbf")

# one step() call: gradient magnitude, clip threshold (None = unclipped), mask on/off, EMA mode (0 = no EMA arena passed) and decay
Step = collections.namedtuple("Step", "mag max_norm use_mask ema_mode ema_decay")
FORGET_ON = Step(3.0, 1.0, True, 0, 0.0)                # DiT forget stage, clip active
FORGET_OFF = Step(1e-3, 1.0, True, 0, 0.0)              # ... clip inactive (coefficient exactly 1)
REMAIN = Step(0.1, None, False, 1, 0.9999)              # DiT remain stage: no mask, no clip, EMA fused
SCHED = (FORGET_ON, REMAIN, FORGET_OFF, REMAIN)
FORGET_EMA = Step(3.0, 1.0, True, 1, 0.9999)


@functools.lru_cache(maxsize=None)
def _arena():
    gen = torch.Generator().manual_seed(20)
    return dict(p0=torch.randn(N, generator=gen), ema0=torch.randn(N, generator=gen), mask=(torch.rand(N, generator=gen) < 0.5).to(torch.uint8))


@functools.lru_cache(maxsize=None)
def _grad(i, mag, seed=1, n=N):
    """the gradient of step i (CPU, fresh per step; seed 2 = the second arena of the g2 tests)"""
    return torch.randn(n, generator=torch.Generator().manual_seed(1000 * seed + i)) * mag


@functools.lru_cache(maxsize=None)
def _factors(i):
    gen = torch.Generator().manual_seed(500 + i)
    return (torch.randn(R, NM, generator=gen) * 0.1).to(torch.bfloat16), torch.randn(R, D, generator=gen).to(torch.bfloat16)


class _State:
    """The arenas of one run and the FlatAdam over them (bf16 shadow and EMA arena always attached)."""

    def __init__(self, wd=0.0, ranges=None, mask=None):
        from sfron import sweep
        a = _arena()
        self.p = a["p0"].to(DEV)
        self.g = torch.zeros(N, device=DEV)
        self.ema = a["ema0"].to(DEV)
        self.wbf = torch.full((N,), 7.0, dtype=torch.bfloat16, device=DEV)
        self.mask = (a["mask"] if mask is None else mask).to(DEV)
        self.opt = sweep.FlatAdam(self.p, self.g, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, mask=self.mask, w_bf16=self.wbf, ranges=ranges)
        self.keep = []                                   # tensors the kernels of a step read: alive until the run ends

    def snap(self):
        o = self.opt
        return dict(p=self.p.clone(), m=o.m.clone(), v=o.v.clone(), ema=self.ema.clone(), wbf=self.wbf.clone(), stats=o.stats.clone())

    def kw(self, s):
        return dict(max_norm=s.max_norm, use_mask=s.use_mask, ema=self.ema if s.ema_mode else None, ema_decay=s.ema_decay, ema_mode=s.ema_mode)

    def lowrank(self, i):
        dmod, sc = (t.to(DEV) for t in _factors(i))
        self.keep += [dmod, sc]
        return dict(lo=ADA[0], NM=NM, D=D, R=R, dmod=dmod, sc=sc)


def _plain_step(st, i, s, g):
    st.g.copy_(g)
    st.opt.step(**st.kw(s))


def _drive(sched, stepper=_plain_step, lowrank=False, **state_kw):
    """Run ``sched`` through ``stepper``; returns the snapshots [initial, after step 0, after step 1, ...].  Before every clipped step
    the statistics are NaN: a sweep that reads the coefficient before k_clip_coef has written it poisons p."""
    st = _State(**state_kw)
    snaps = [st.snap()]
    for i, s in enumerate(sched):
        if s.max_norm is not None:
            st.opt.stats.fill_(NAN)
        if lowrank:
            st.opt.lowrank = st.lowrank(i)
        stepper(st, i, s, _grad(i, s.mag))
        torch.cuda.synchronize()
        snaps.append(st.snap())
    assert st.opt.step_count == len(sched)
    return snaps


@functools.lru_cache(maxsize=None)
def plain(sched=SCHED, lowrank=False, wd=0.0):
    """The comparison object of every path: FlatAdam.step() with no split / pipeline / ranges (snapshots of p, m, v, ema, w_bf16, stats
    after every step; shared, never written)."""
    return _drive(sched, lowrank=lowrank, wd=wd)


def _same(got, want, keys=KEYS, lo=0, hi=N, what=""):
    for k in keys:
        a, b = got[k][lo:hi], want[k][lo:hi]
        assert torch.equal(a, b), (what, k, lo, hi, int((a != b).sum()))


def _same_stats(got, want):
    assert torch.equal(got["stats"][:3], want["stats"][:3]), (got["stats"], want["stats"])       # [3] is never written


def _finite(snap):
    for k in KEYS:
        assert torch.isfinite(snap[k].float()).all(), k


@functools.lru_cache(maxsize=None)
def _torch_ref(sched, wd=0.0, g2=False, n=N):
    """torch.optim.AdamW + mask + clip_grad_norm_ + EMA on the CPU in fp32: (p, m, v, ema, [norm per step])"""
    from oracle import sweep_ref
    a = _arena()
    ref = sweep_ref.AdamRef([a["p0"][:n]], lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, adamw=True)
    ema, norms = [a["ema0"][:n].clone()], []
    for i, s in enumerate(sched):
        g = _grad(i, s.mag, 1, n).clone()
        if g2:
            g = g + _grad(i, s.mag, 2, n)
        if s.use_mask:
            sweep_ref.apply_mask_([g], [a["mask"][:n].bool()])
        norms.append(float(sweep_ref.clip_grad_norm_([g], s.max_norm)) if s.max_norm is not None else None)
        ref.step([g])
        if s.ema_mode == 1:
            sweep_ref.ema_update_dit_(ema, [ref.params[0].data], s.ema_decay)
        elif s.ema_mode == 2:
            sweep_ref.ema_update_ddpm_(ema, [ref.params[0].data], s.ema_decay)
    m, v, steps = ref.state(0)
    assert steps == len(sched)
    return ref.params[0].detach(), m, v, ema[0], norms


def _close_to_torch(snap, ref, ema=True):
    """the bounds test_two_stage_sweep_vs_torch holds these kernels to"""
    p, m, v, e, _ = ref
    np.testing.assert_allclose(snap["p"].cpu().numpy(), p.numpy(), rtol=2e-6, atol=2e-7)
    np.testing.assert_allclose(snap["m"].cpu().numpy(), m.numpy(), rtol=2e-6, atol=1e-8)
    np.testing.assert_allclose(snap["v"].cpu().numpy(), v.numpy(), rtol=2e-6, atol=1e-12)
    if ema:
        np.testing.assert_allclose(snap["ema"].cpu().numpy(), e.numpy(), rtol=2e-6, atol=2e-7)
    assert torch.equal(snap["wbf"].cpu(), snap["p"].cpu().to(torch.bfloat16))


def _norms_match(snaps, sched, norms):
    for i, s in enumerate(sched):
        if s.max_norm is not None:          # torch accumulates the norm in fp32, the kernel in fp64
            assert abs(snaps[i + 1]["stats"][0].item() - norms[i]) <= 1e-5 * norms[i], (i, snaps[i + 1]["stats"], norms[i])


# =====================================================================================================================================
# A. the plain path against torch
# =====================================================================================================================================

@pytest.mark.parametrize("wd", [0.01, 10.0])
def test_plain_adamw_weight_decay_vs_torch(wd):
    """decay_mul multiplies p, and only p, before the Adam update (torch.optim.AdamW: param.mul_(1 - lr * wd)).  At weight_decay = 0.01
    a decay that also reached the update term would move p by lr * wd * lr = 1e-8 per step, under the bounds; at 10.0 (decay_mul = 0.99)
    it is 1e-5 per step and shows."""
    sched = (FORGET_EMA, FORGET_EMA._replace(mag=1e-3), FORGET_EMA)             # clip on, off, on
    snaps = plain(sched, wd=wd)
    ref = _torch_ref(sched, wd=wd)
    _norms_match(snaps, sched, ref[4])
    _close_to_torch(snaps[-1], ref)
    assert snaps[2]["stats"][1].item() == 1.0 and snaps[3]["stats"][1].item() < 0.01
    # and the decay is really there: without it p differs by ~ lr * wd * |p| per step, fifty times the bound above
    assert not np.allclose(snaps[-1]["p"].cpu().numpy(), _torch_ref(sched)[0].numpy(), rtol=2e-6, atol=2e-7)


def test_plain_g2_vs_torch():
    """a second gradient arena (micro-batch chains): the step is on g + g2, the clip norm is the norm of the masked SUM."""
    sched = (FORGET_EMA, REMAIN, FORGET_EMA._replace(mag=1e-3))

    def stepper(st, i, s, g):
        st.g.copy_(g)
        g2 = _grad(i, s.mag, 2).to(DEV)
        st.keep.append(g2)
        st.opt.g2 = g2
        st.opt.step(**st.kw(s))
        st.opt.g2 = None
    snaps = _drive(sched, stepper)
    ref = _torch_ref(sched, g2=True)
    _norms_match(snaps, sched, ref[4])
    _close_to_torch(snaps[-1], ref)
    assert not torch.equal(snaps[-1]["p"], plain(sched)[-1]["p"])


def test_plain_ema_modes_vs_torch():
    """the in-sweep EMA, DDPM form (mode 2: (1 - mu) p + mu shadow) and DiT form (mode 1), and the stand-alone sfron_ema_update mode 1"""
    from sfron import sweep
    from oracle import sweep_ref
    sched = (Step(3.0, 1.0, True, 2, 0.9999), Step(0.1, None, False, 2, 0.9999), Step(1e-3, 1.0, True, 1, 0.9999), FORGET_ON)
    snaps = plain(sched)
    ref = _torch_ref(sched)
    _norms_match(snaps, sched, ref[4])
    _close_to_torch(snaps[-1], ref)
    assert torch.equal(snaps[-1]["ema"], snaps[-2]["ema"]) and not torch.equal(snaps[1]["ema"], snaps[0]["ema"])   # mode 0 leaves the arena alone
    a = _arena()
    for n in (5, 77_777):
        want = [a["ema0"][:n].clone()]
        sweep_ref.ema_update_dit_(want, [a["p0"][:n]], 0.9999)
        got = a["ema0"][:n].to(DEV)
        sweep.ema_update(got, a["p0"][:n].to(DEV), 0.9999, mode=1)
        np.testing.assert_allclose(got.cpu().numpy(), want[0].numpy(), rtol=2e-6, atol=2e-7)


@pytest.mark.parametrize("lowrank", [False, True])
def test_mask_bytes_other_than_one_mean_keep(lowrank):
    """every non-zero mask byte keeps the gradient, in the norm pre-pass and in the update, vector body and scalar tail alike"""
    gen = torch.Generator().manual_seed(4)
    pos = torch.cat([torch.randperm(N, generator=gen)[:300], torch.arange(ADA[0], ADA[0] + 40), torch.arange(N - 3, N)])
    one, odd = _arena()["mask"].clone(), _arena()["mask"].clone()
    one[pos] = 1
    odd[pos[0::2]] = 2
    odd[pos[1::2]] = 255
    sched = (FORGET_EMA, FORGET_EMA._replace(mag=1e-3))
    want = _drive(sched, lowrank=lowrank, mask=one)
    got = _drive(sched, lowrank=lowrank, mask=odd)
    for a, b in zip(got[1:], want[1:]):
        _same(a, b)
        _same_stats(a, b)
    assert not torch.equal(want[-1]["p"], plain(sched, lowrank=lowrank)[-1]["p"])      # those bytes matter


def test_refused_arguments_leave_the_arenas_alone():
    from sfron import _lib, sweep
    from sfron._lib import ERR_ARG, SfronError, ptr, stream_ptr
    L = _lib.lib()
    n = 1024
    gen = torch.Generator().manual_seed(6)
    t = {k: torch.randn(n + 8, generator=gen).to(DEV) for k in ("p", "g", "m", "v", "ema")}
    t["v"].abs_()
    t["mask"] = (torch.rand(n + 8, generator=gen) < 0.5).to(torch.uint8).to(DEV)
    t["wbf"] = torch.full((n + 8,), 7.0, dtype=torch.bfloat16, device=DEV)
    t["w8"] = torch.full((n + 8,), 0xAA, dtype=torch.uint8, device=DEV)
    t["part"] = torch.full((8,), 3.0, dtype=torch.float64, device=DEV)
    scale = torch.ones(1, device=DEV)
    before = {k: x.clone() for k, x in t.items()}
    hyper = (0.9, 0.999, 1e-8, 1e-2, 0.03, 1.0)
    s = stream_ptr()

    def adam(p, mask, cnt):
        return L.sfron_masked_clip_adam(ptr(p), ptr(t["g"][:cnt]), None, ptr(t["m"][:cnt]), ptr(t["v"][:cnt]), ptr(mask), None, cnt, *hyper,
                                        ptr(t["wbf"][:cnt]), ptr(t["ema"][:cnt]), 0.99, 1, s)
    assert adam(t["p"][1:n + 1], t["mask"][:n], n) == ERR_ARG                  # p four bytes off a 16-byte boundary
    assert adam(t["p"][:n], t["mask"][1:n + 1], n) == ERR_ARG                  # mask view at an odd offset
    nb = ctypes.c_int(-5)
    assert L.sfron_sumsq_masked(ptr(t["g"][:n]), None, ptr(t["mask"][1:n + 1]), n, ptr(t["part"]), ctypes.byref(nb), s) == ERR_ARG and nb.value == -5
    assert L.sfron_masked_clip_adam_wg(ptr(t["p"][:n]), ptr(t["g"][:n]), ptr(t["g"][1:n + 1]), ptr(t["m"][:n]), ptr(t["v"][:n]), None, None, n, *hyper,
                                       ptr(t["wbf"][:n]), ptr(t["ema"][:n]), 0.99, 1, 2, s) == ERR_ARG       # g2 misaligned
    for cnt in (n - 2, n - 1):                                                 # the e4m3 shadow is written four bytes at a time: n % 4 == 0 only
        assert L.sfron_masked_clip_adam_q(ptr(t["p"][:cnt]), ptr(t["g"][:cnt]), ptr(t["m"][:cnt]), ptr(t["v"][:cnt]), None, None, cnt, *hyper,
                                          ptr(t["wbf"][:cnt]), ptr(t["ema"][:cnt]), 0.99, 1, ptr(t["w8"][:cnt]), ptr(scale), 0, s) == ERR_ARG
    # the same refusal through the host class is an exception, not a quiet no-op
    opt = sweep.FlatAdam(t["p"][1:n + 1], t["g"][1:n + 1], lr=LR, w_bf16=t["wbf"][:n])
    with pytest.raises(SfronError):
        opt.step()
    torch.cuda.synchronize()
    for k, x in t.items():
        assert torch.equal(x, before[k]), k
    # and the accepted call does move them (the refusals above are not a dead library)
    assert adam(t["p"][:n], t["mask"][:n], n) == 0
    torch.cuda.synchronize()
    assert not torch.equal(t["p"], before["p"]) and torch.equal(t["p"][n:], before["p"][n:])


# =====================================================================================================================================
# B. every scheduling path equals the plain sweep, bit for bit
# =====================================================================================================================================

def _hyper(t):
    """the scalar arguments FlatAdam.step() forms for step number t (weight decay 0, EMA mode 1 at 0.9999)"""
    return (BETAS[0], BETAS[1], EPS, LR / (1 - BETAS[0] ** t), math.sqrt(1 - BETAS[1] ** t), 1.0)


@pytest.mark.parametrize("cap", [1, 2, 3, 768, 0])
def test_wg_on_one_block_range_equals_plain(cap):
    """sfron_masked_clip_adam_wg with a bounded grid on ONE block range, coefficient from the real norm pre-pass"""
    from sfron import _lib
    from sfron._lib import check, ptr, stream_ptr
    L = _lib.lib()
    want = plain((FORGET_EMA,))
    st = _State()
    st.g.copy_(_grad(0, FORGET_EMA.mag))
    st.opt.stats.fill_(NAN)
    st.opt.grad_norm_clip_coef(1.0, True)
    lo, hi = BLOCKS[2]
    o = st.opt
    check(L.sfron_masked_clip_adam_wg(ptr(st.p[lo:hi]), ptr(st.g[lo:hi]), None, ptr(o.m[lo:hi]), ptr(o.v[lo:hi]), ptr(st.mask[lo:hi]), ptr(o.stats),
                                      hi - lo, *_hyper(1), ptr(st.wbf[lo:hi]), ptr(st.ema[lo:hi]), 0.9999, 1, cap, stream_ptr()), "wg")
    torch.cuda.synchronize()
    got = st.snap()
    _same_stats(got, want[1])
    _same(got, want[1], lo=lo, hi=hi)
    _same(got, want[0], hi=lo)                       # nothing outside the range moved
    _same(got, want[0], lo=hi)
    assert not torch.equal(got["p"][lo:hi], want[0]["p"][lo:hi])


def test_wg_bounded_grids_two_strides_and_a_tail():
    """n = two full strides of the 768-workgroup grid (768 x 256 float4) plus one float4 plus one scalar: every bounded grid leaves the
    bits of the full grid, and the full grid is torch's AdamW."""
    from oracle import sweep_ref
    from sfron import _lib
    from sfron._lib import check, ptr, stream_ptr
    L = _lib.lib()
    n = 786_432 * 2 + 5
    gen = torch.Generator().manual_seed(8)
    p0, e0, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 3.0
    mask = torch.rand(n, generator=gen) < 0.5
    gd, md = g.to(DEV), mask.to(torch.uint8).to(DEV)
    part = torch.empty(L.sfron_sweep_partials_len(), dtype=torch.float64, device=DEV)
    stats = torch.full((4,), NAN, device=DEV)
    nb = ctypes.c_int(0)
    check(L.sfron_sumsq_masked(ptr(gd), None, ptr(md), n, ptr(part), ctypes.byref(nb), stream_ptr()), "sumsq")
    check(L.sfron_clip_coef(ptr(part), nb.value, 1.0, ptr(stats), stream_ptr()), "clip")
    outs = {}
    for cap in (0, 1, 2, 3, 768):
        p, m, v, ema = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), e0.to(DEV)
        wbf = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV)
        check(L.sfron_masked_clip_adam_wg(ptr(p), ptr(gd), None, ptr(m), ptr(v), ptr(md), ptr(stats), n, *_hyper(1), ptr(wbf), ptr(ema), 0.9999, 1,
                                          cap, stream_ptr()), "wg")
        torch.cuda.synchronize()
        outs[cap] = dict(p=p, m=m, v=v, ema=ema, wbf=wbf)
    for cap in (1, 2, 3, 768):
        _same(outs[cap], outs[0], hi=n, what=cap)
    ref = sweep_ref.AdamRef([p0], lr=LR, betas=BETAS, eps=EPS, adamw=True)
    gm = g * mask
    norm = float(sweep_ref.clip_grad_norm_([gm], 1.0))
    ref.step([gm])
    er = [e0.clone()]
    sweep_ref.ema_update_dit_(er, [ref.params[0].data], 0.9999)
    assert abs(stats[0].item() - norm) <= 1e-5 * norm
    _close_to_torch(outs[0], (ref.params[0].detach(), ref.state(0)[0], ref.state(0)[1], er[0], None))


def test_ranges_sweep_only_their_share():
    """ranges= at construction (SD "xattn"): unclipped steps stream only those ranges; the rest of every arena keeps its bits"""
    rngs = [(0, 4_096), BLOCKS[1], (BLOCKS[3][0] + 8, BLOCKS[4][1] - 16), (REST[0], REST[0] + 8_000)]
    assert all(lo % 8 == 0 and hi % 8 == 0 for lo, hi in rngs)
    sched = (REMAIN, REMAIN._replace(use_mask=True), REMAIN._replace(ema_mode=2))
    want = plain(sched)
    got = _drive(sched, ranges=rngs)
    edge = 0
    for lo, hi in rngs:
        _same(got[-1], want[0], lo=edge, hi=lo, what="outside")
        _same(got[-1], want[-1], lo=lo, hi=hi, what="inside")
        edge = hi
    _same(got[-1], want[0], lo=edge, what="outside")
    assert not torch.equal(want[-1]["p"][rngs[1][1]:rngs[2][0]], want[0]["p"][rngs[1][1]:rngs[2][0]])


def _split_stepper(side, head, cap, extra=None):
    """step(split=...) over the six block ranges, one fresh event per block; the caller's stream then waits for all of them (and for the
    adaLN matrix) before the next gradients overwrite the arena"""
    def stepper(st, i, s, g):
        st.g.copy_(g)
        split = dict(ranges=BLOCKS, stream=side, events=[torch.cuda.Event() for _ in BLOCKS], head=head, max_workgroups=cap)
        split.update(extra(st) if extra is not None else {})
        st.opt.step(split=split, **st.kw(s))
        st.last_split = split
        cur = torch.cuda.current_stream()
        for ev in split["events"]:
            cur.wait_event(ev)
        if split.get("ada_done") is not None:
            cur.wait_event(split["ada_done"])
    return stepper


@pytest.mark.parametrize("cap", [0, 2])
@pytest.mark.parametrize("head", [0, 2, 6])
def test_split_two_streams_equals_plain(head, cap):
    """split=: the first `head` block ranges on the caller's stream, the rest on a second stream behind the clip coefficient, one event
    per block; clipped forget form and unclipped remain form with EMA, two iterations"""
    want = plain(SCHED)
    main, side = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(main):
        got = _drive(SCHED, _split_stepper(side, head, cap))
    for a, b in zip(got[1:], want[1:]):
        _same(a, b, what=(head, cap))
        _same_stats(a, b)


def test_split_refuses_a_second_gradient_arena():
    """the block-range launches of split= read one gradient arena; with g2 set they would drop it without a word: refused before any launch"""
    st = _State()
    st.g.copy_(_grad(0, 0.1))
    st.opt.g2 = _grad(0, 0.1, 2).to(DEV)
    before = st.snap()
    with pytest.raises(AssertionError):
        st.opt.step(split=dict(ranges=BLOCKS, stream=None, quant=None), **st.kw(REMAIN))
    torch.cuda.synchronize()
    _same(st.snap(), before)


def test_split_deferred_side_ranges():
    """defer=True: step() leaves the side-stream ranges to the caller -- they keep their old bits until take_deferred()() has run"""
    head = 2
    want = plain(SCHED)
    main, side = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(main):
        st = _State()
        for i, s in enumerate(SCHED):
            if s.max_norm is not None:
                st.opt.stats.fill_(NAN)
            st.g.copy_(_grad(i, s.mag))
            split = dict(ranges=BLOCKS, stream=side, events=[torch.cuda.Event() for _ in BLOCKS], head=head, max_workgroups=2, defer=True)
            st.opt.step(split=split, **st.kw(s))
            torch.cuda.synchronize()
            mid = st.snap()
            lo, hi = BLOCKS[head][0], BLOCKS[-1][1]
            _same(mid, want[i], lo=lo, hi=hi, what="deferred ranges: old bits")
            _same(mid, want[i + 1], hi=lo, what="head ranges and the arena in front: new bits")
            _same(mid, want[i + 1], lo=hi, what="the arena behind the blocks: new bits")
            _same_stats(mid, want[i + 1])
            fn = st.opt.take_deferred()
            assert callable(fn)
            fn()
            for ev in split["events"]:
                main.wait_event(ev)
            torch.cuda.synchronize()
            _same(st.snap(), want[i + 1], what="after the deferred launch")
            assert st.opt.take_deferred() is None
        # nothing to defer (every range is a head range): step() launches all of it and leaves no callable behind
        st.g.copy_(_grad(4, 0.1))
        st.opt.step(split=dict(ranges=BLOCKS, stream=side, events=[torch.cuda.Event() for _ in BLOCKS], head=6, defer=True), **st.kw(REMAIN))
        assert st.opt.take_deferred() is None
        torch.cuda.synchronize()


@pytest.mark.parametrize("ada_side,with_stream", [(True, True), (False, True), (True, False)])
def test_split_lowrank_ada_side_equals_lowrank_plain(ada_side, with_stream):
    """the factored adaLN gradient under split=: swept on the second stream in front of the block ranges (ada_side) or on the caller's"""
    want = plain(SCHED, lowrank=True)
    assert not torch.equal(want[-1]["p"][ADA[0]:ADA[1]], plain(SCHED)[-1]["p"][ADA[0]:ADA[1]])     # the factors, not the gradient arena
    main, side = torch.cuda.Stream(), torch.cuda.Stream()
    dones = []
    step = _split_stepper(side if with_stream else None, 2, 2, lambda st: dict(ada_side=ada_side))

    def stepper(st, i, s, g):
        step(st, i, s, g)
        dones.append(st.last_split["ada_done"])
        assert st.opt.lowrank is None                    # cleared by step()
    torch.cuda.synchronize()
    with torch.cuda.stream(main):
        got = _drive(SCHED, stepper, lowrank=True)
    for a, b in zip(got[1:], want[1:]):
        _same(a, b, what=(ada_side, with_stream))
        _same_stats(a, b)
    assert len(dones) == len(SCHED)
    for ev in dones:
        assert isinstance(ev, torch.cuda.Event) if (ada_side and with_stream) else ev is None


def _e4m3_equal(got, want):
    return ((got == want) | (((got & 0x7F) == 0) & ((want & 0x7F) == 0))).all()       # +0 / -0 are the same value


@pytest.mark.parametrize("with_stream,head", [(False, 0), (True, 2), (True, 0)])
def test_split_quant_equals_plain_and_writes_the_e4m3_shadow(with_stream, head):
    """config 5: one sfron_masked_clip_adam_q launch per tensor, which also leaves e4m3(new p * that tensor's scale)"""
    from oracle import fp8_ref
    want = plain(SCHED)
    main, side = torch.cuda.Stream(), torch.cuda.Stream()
    w8 = torch.full((N,), 0xAA, dtype=torch.uint8, device=DEV)
    scales = torch.tensor(SCALES, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(main):
        got = _drive(SCHED, _split_stepper(side if with_stream else None, head, 2,
                                           lambda st: dict(quant=dict(tensors=TENSORS, w8=w8, scales=scales))))
    for a, b in zip(got[1:], want[1:]):
        _same(a, b, what=(with_stream, head))
        _same_stats(a, b)
    w8c, pc = w8.cpu(), got[-1]["p"].cpu()
    assert (w8c[:BLOCKS[0][0]] == 0xAA).all() and (w8c[BLOCKS[-1][1]:] == 0xAA).all()
    sat = 0
    for blk in TENSORS:
        for tlo, thi, si in blk:
            want8 = fp8_ref.e4m3_bytes(pc[tlo:thi], SCALES[si])
            assert _e4m3_equal(w8c[tlo:thi], want8), (tlo, thi, si, int((w8c[tlo:thi] != want8).sum()))
            if si == SAT:
                sat = int(((want8 & 0x7F) == 0x7E).sum())
            elif si + 1 < len(SCALES) and si + 1 != SAT:      # the neighbour's scale gives other bytes: a wrong index would show
                assert not _e4m3_equal(w8c[tlo:thi], fp8_ref.e4m3_bytes(pc[tlo:thi], SCALES[si + 1]))
    assert sat > (TENSORS[SAT // 3][SAT % 3][1] - TENSORS[SAT // 3][SAT % 3][0]) // 2      # that tensor sits at +-448


BUCKETS = [(0, 50_000), (50_000, 120_004), (120_004, BLOCKS[-1][1]), (BLOCKS[-1][1], N)]


def _pipeline_stepper(comm):
    def stepper(st, i, s, g):
        cur = torch.cuda.current_stream()
        src = g.to(DEV)
        st.keep.append(src)
        st.g.fill_(NAN)                              # a bucket read before its event has fired is NaN
        ready = torch.cuda.Event()
        ready.record(cur)
        comm.wait_event(ready)
        pipe = []
        with torch.cuda.stream(comm):
            for lo, hi in BUCKETS:
                st.g[lo:hi].copy_(src[lo:hi])
                ev = torch.cuda.Event()
                ev.record(comm)
                pipe.append((lo, hi, ev))
        st.opt.step(pipeline=pipe, **st.kw(s))
    return stepper


def test_pipeline_unclipped_equals_plain():
    sched = (REMAIN, REMAIN._replace(use_mask=True), REMAIN)
    want = plain(sched)
    main, comm = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(main):
        got = _drive(sched, _pipeline_stepper(comm))
    for a, b in zip(got[1:], want[1:]):
        _same(a, b)


def test_pipeline_clipped_vs_torch():
    """Clipped, the norm is summed per bucket: the fp64 partials are grouped differently from the one-launch pre-pass, so the coefficient
    may move by an fp32 ulp and bit identity with the plain sweep is not owed.  Held to the torch bounds instead."""
    sched = (FORGET_EMA, REMAIN, FORGET_EMA._replace(mag=1e-3))
    main, comm = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(main):
        got = _drive(sched, _pipeline_stepper(comm))
    ref = _torch_ref(sched)
    _norms_match(got, sched, ref[4])
    for snap in got:
        _finite(snap)
    _close_to_torch(got[-1], ref)
    want = plain(sched)
    for i, s in enumerate(sched):
        if s.max_norm is not None:
            a, b = got[i + 1]["stats"][0].item(), want[i + 1]["stats"][0].item()
            assert abs(a - b) <= 1e-5 * b


def test_fused_sumsq_norm_equals_unfused():
    """fused_sumsq: the block ranges' masked sums of squares arrive as fp64 partials (here from torch), the embedders and the final layer
    go through the device range table, the adaLN matrix through its factors."""
    from sfron import _lib
    L = _lib.lib()
    st = _State()
    g = _grad(0, 3.0).clone()
    g[N - (N & 3):] = 0          # sfron_sumsq_masked_ranges takes multiples of 4 (the engine's tensors are): the arena's last 3 floats carry no gradient here
    st.g.copy_(g)
    st.opt.lowrank = st.lowrank(0)
    st.opt.stats.fill_(NAN)
    st.opt.grad_norm_clip_coef(1.0, True)
    torch.cuda.synchronize()
    unfused = st.opt.stats.clone()
    assert unfused[1].item() < 0.1
    rows = [(EMB[0], EMB[1] - EMB[0]), (REST[0], 20_000), (REST[0] + 20_000, (REST[1] - REST[0] - 20_000) & ~3)]
    assert all(off % 4 == 0 and ln % 4 == 0 and ln <= 65_536 for off, ln in rows)
    tab = torch.tensor(rows, dtype=torch.int64, device=DEV)
    n_gemm = len(BLOCKS)
    buf = torch.full((n_gemm + len(rows) + NM // 8 + 4,), NAN, dtype=torch.float64, device=DEV)
    md = st.mask.double()
    for i, (lo, hi) in enumerate(BLOCKS):
        buf[i] = (st.g[lo:hi].double() * md[lo:hi]).pow(2).sum()
    st.opt.stats.fill_(NAN)
    st.opt.fused_sumsq = dict(partials=buf[:n_gemm], buffer=buf, ranges=tab, n_ranges=len(rows))
    st.opt.step(max_norm=1.0, use_mask=True, ema=st.ema, ema_decay=0.9999, ema_mode=1)
    torch.cuda.synchronize()
    assert st.opt.fused_sumsq is None and st.opt.lowrank is None
    fused = st.opt.stats
    assert abs(fused[0].item() - unfused[0].item()) <= 1e-5 * unfused[0].item(), (fused, unfused)
    assert torch.isnan(buf[n_gemm + len(rows) + NM // 8:]).all() and torch.isfinite(buf[:n_gemm + len(rows) + NM // 8]).all()
    # the update itself: the unfused low-rank step on the same gradients.  The two coefficients may differ in the last place (other
    # grouping of the fp64 sums), which moves p by ~1e-7 * lr: the torch bounds of section A, not bit identity.
    def stepper(s2, i, s, _g):
        s2.g.copy_(g)
        s2.opt.step(**s2.kw(s))
    want = _drive((FORGET_EMA,), stepper, lowrank=True)[1]
    got = st.snap()
    _finite(got)
    for k, atol in (("p", 2e-7), ("m", 1e-8), ("v", 1e-12), ("ema", 2e-7)):
        np.testing.assert_allclose(got[k].cpu().numpy(), want[k].cpu().numpy(), rtol=2e-6, atol=atol)
    assert torch.equal(got["wbf"], got["p"].to(torch.bfloat16))


# =====================================================================================================================================
# C. the small kernels
# =====================================================================================================================================

@pytest.mark.parametrize("nblk", [1, 63, 1024, 1025, 3072, 3073, 4096, 4097, 26_000])
def test_clip_coef_every_loop_form(nblk):
    """k_clip_coef: 1024 threads, a 4-way unrolled loop entered only above 3072 partials, then a plain one.  The fp64 summation order is
    not torch's, so the sum and the norm are held to one fp32 ulp of the rounded float64 reference; the coefficient is exact."""
    from sfron import _lib
    from sfron._lib import check, ptr, stream_ptr
    L = _lib.lib()
    gen = torch.Generator().manual_seed(nblk)
    vals = 10.0 ** (torch.rand(nblk, dtype=torch.float64, generator=gen) * 10.0 - 5.0)          # ten decades
    buf = torch.full((nblk + 4200,), NAN, dtype=torch.float64)                                    # a read past nblk shows
    buf[:nblk] = vals
    bufd = buf.to(DEV)
    t = vals.sum().item()
    t32, n32 = np.float32(t), np.float32(math.sqrt(t))
    for max_norm, clipped in ((0.5 * float(n32), True), (2.0 * float(n32), False)):
        stats = torch.full((4,), NAN, device=DEV)
        check(L.sfron_clip_coef(ptr(bufd), nblk, max_norm, ptr(stats), stream_ptr()), "clip_coef")
        s = stats.cpu().numpy()
        assert abs(s[2] - t32) <= np.spacing(t32) and abs(s[0] - n32) <= np.spacing(n32), (s, t32, n32)
        if clipped:
            assert s[1] == np.float32(max_norm) / (s[0] + np.float32(1e-6)) and s[1] < 1.0, s
        else:
            assert s[1] == 1.0, s
        assert np.isnan(s[3])
    stats = torch.full((4,), NAN, device=DEV)
    check(L.sfron_clip_coef(ptr(torch.zeros(nblk, dtype=torch.float64, device=DEV)), nblk, 1.0, ptr(stats), stream_ptr()), "clip_coef")
    assert stats[:3].cpu().tolist() == [0.0, 1.0, 0.0]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 2_097_157])
def test_sumsq_masked_partials(n):
    """sfron_sumsq_masked: the grid (2 097 157 floats reach the 2048-workgroup cap and stride), the scalar tail, g2 and the mask"""
    from sfron import _lib
    from sfron._lib import check, ptr, stream_ptr
    L = _lib.lib()
    gen = torch.Generator().manual_seed(n)
    g, g2 = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.5
    mask = (torch.rand(n, generator=gen) < 0.5).to(torch.uint8)
    mask[-1] = 1                                                          # n = 1: a sum that is not trivially zero
    if n > 2048 * 256 * 4:
        # the one float4 that a workgroup reaches on its SECOND trip, and the scalar behind it, weigh ~2e-3 of the sum: a grid that does
        # not stride misses the bound (at unit size five floats in two million would pass it unnoticed)
        g[2048 * 256 * 4:] = 30.0
        mask[2048 * 256 * 4:] = 1
    gd, g2d, md = g.to(DEV), g2.to(DEV), mask.to(DEV)
    want_nblk = max(1, min(2048, -(-(n >> 2) // 256)))
    for use_g2 in (False, True):
        for use_mask in (False, True):
            part = torch.full((2048 + 2,), -7.0, dtype=torch.float64, device=DEV)
            nb = ctypes.c_int(0)
            check(L.sfron_sumsq_masked(ptr(gd), ptr(g2d) if use_g2 else None, ptr(md) if use_mask else None, n, ptr(part), ctypes.byref(nb),
                                       stream_ptr()), "sumsq_masked")
            assert nb.value == want_nblk
            pc = part.cpu()
            assert (pc[nb.value:] == -7.0).all() and (pc[:nb.value] >= 0).all()
            x = ((g + g2) if use_g2 else g).double()                      # the sum of the two arenas is an fp32 add, as in the kernel
            if use_mask:
                x = x * mask.double()
            ref = x.pow(2).sum().item()
            assert ref > 0 and abs(pc[:nb.value].sum().item() - ref) <= 1e-6 * ref, (use_g2, use_mask, pc[:nb.value].sum().item(), ref)


@pytest.mark.parametrize("n", [5, 77_777])
def test_fisher_accum_clipped_vs_torch(n):
    """the DDPM Fisher: F += ((g + g2) * clip coefficient)^2 / n_iters, coefficient from a real sfron_clip_coef with the clip active"""
    from sfron import _lib
    from sfron._lib import check, ptr, stream_ptr
    L = _lib.lib()
    gen = torch.Generator().manual_seed(n)
    part = torch.empty(L.sfron_sweep_partials_len(), dtype=torch.float64, device=DEV)
    for use_g2, use_stats in ((False, True), (True, True), (True, False), (False, False)):
        F = torch.rand(n, generator=gen) * 1e-3
        Fd = F.to(DEV)
        for _ in range(3):
            g, g2 = torch.randn(n, generator=gen) * 3.0, torch.randn(n, generator=gen) * 3.0
            gd, g2d = g.to(DEV), (g2.to(DEV) if use_g2 else None)
            coef = torch.tensor(1.0)
            stats = None
            if use_stats:
                stats = torch.full((4,), NAN, device=DEV)
                nb = ctypes.c_int(0)
                check(L.sfron_sumsq_masked(ptr(gd), ptr(g2d), None, n, ptr(part), ctypes.byref(nb), stream_ptr()), "sumsq")
                check(L.sfron_clip_coef(ptr(part), nb.value, 1.0, ptr(stats), stream_ptr()), "clip")
                coef = stats[1].cpu()
                assert coef.item() < 0.7                                  # the clip is active
            check(L.sfron_fisher_accum_clipped(ptr(Fd), ptr(gd), ptr(g2d), ptr(stats), n, 3.0, stream_ptr()), "fisher_accum_clipped")
            x = (g + g2) if use_g2 else g
            F += ((x * coef) ** 2) / 3
        np.testing.assert_allclose(Fd.cpu().numpy(), F.numpy(), rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 2_097_157])
def test_cast_bf16_bit_exact(n):
    """sfron_cast_bf16 against torch's fp32 -> bf16 (round to nearest even), vector body and scalar tail, specials included"""
    from sfron import sweep
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen) * torch.logspace(-42, 38, n if n > 1 else 2)[:n]           # subnormals ... the top binade
    bits = [0x00000000, 0x80000000,                    # +-0
            0x00000001, 0x807FFFFF, 0x00400000,        # fp32 subnormals (bf16 keeps the exponent range: they stay subnormal or round to the smallest normal)
            0x3F808000, 0x3F818000, 0xBF808000,        # exact ties: to even downwards, to even upwards, negative
            0x3F80FFFF, 0x3FFFFFFF, 0x7EFFFFFF,        # round up, round up into the next binade
            0x7F800000, 0xFF800000,                    # +-Inf
            0x7F7FFFFF, 0xFF7FFFFF,                    # +-3.4e38: rounds to Inf
            0x7FC00000, 0xFFC00001, 0x7F800001]        # NaNs
    sp = torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())
    k = min(n, sp.numel())
    x[:k] = sp.roll(-(n + 4))[:k]                      # the small sizes each start somewhere else in the list (n = 1, 3: at a tie)
    if n > 2 * sp.numel():
        x[-sp.numel():] = sp.roll(-8)                  # the three exact ties last: they pass through the scalar tail
    dst = torch.full((n + 2,), 7.0, dtype=torch.bfloat16, device=DEV)
    sweep.cast_bf16(x.to(DEV), dst[:n])
    torch.cuda.synchronize()
    got, want = dst.cpu(), x.to(torch.bfloat16)
    assert (got[n:] == 7.0).all()
    gb, wb = got[:n].view(torch.int16), want.view(torch.int16)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got[:n]), nan)
    assert torch.equal(gb[~nan], wb[~nan]), int((gb[~nan] != wb[~nan]).sum())
