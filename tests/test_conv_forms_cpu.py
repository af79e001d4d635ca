"""CPU: the case table and the float64 reference of tests/test_gpu_conv_forms.py (which imports this module), and the two properties of
the table that the GPU test relies on.

Every 3x3 convolution of the DDPM U-Net, the SD v1 U-Net and the VAE is one of four forms:
  same    pad 1
  down0   the DDPM Downsample: F.pad(x, (0, 1, 0, 1)), then stride 2, pad 0   (DDPM/models/diffusion.py:76-80)
  down1   the SD Downsample: stride 2, pad 1                                  (sd_unet.py, openaimodel.py Downsample)
  up      nearest x2, then pad 1                                              (DDPM/models/diffusion.py:56-60)
`reference` is torch.nn.functional in float64 on the CPU with autograd; it never calls the library.  It returns y (with bias, a per-sample
vector vec[b][c] and an optional resid added), dX, dW, d bias and d vec (the per-sample sum of dy over the pixels).

The integer variant draws inputs, weights, bias, vec, resid and dy from the integers -3 .. 3: bf16 holds them exactly and, as long as every
result stays below 2^24, so does every fp32 partial sum in any order -- the GPU test then demands equality with no tolerance.
test_integer_results_stay_below_2_to_24 is that precondition.  test_every_class_is_reached_under_every_form keeps the table honest: the
kernel path a (case, form) reaches is computed from shape predicates restated here (csrc/conv.hip: sfron_conv_fwd, conv_wgrad_pipelined,
unet._conv_desc), so an edit of the table cannot silently drop a path."""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

FORMS = ("same", "down0", "down1", "up")
DOWN = ("down0", "down1")

# (B, H, W, c_in, c_out, forms)
CASES = [
    # pipelined tiles: output rows % 256 == 0, channels % 64 == 0
    (16, 12, 12, 64, 64, FORMS),
    (4, 24, 40, 64, 128, FORMS),      # H != W; down*: 12 x 20 outputs, the weight-gradient tile takes K = 960 with w_out = 20, h_out = 12
    (1, 48, 48, 128, 320, FORMS),     # the 160-column tile
    (4, 40, 24, 64, 192, FORMS),      # H > W, ragged 128-column tile
    # generic tile
    (3, 12, 12, 32, 64, FORMS),       # 432 rows: not % 256, and not % 64 for the weight gradient
    (3, 6, 10, 64, 64, FORMS),        # 180 rows, K < 256
    (2, 4, 4, 64, 64, FORMS),         # small image
    (2, 2, 2, 64, 64, FORMS),         # down*: a 1 x 1 output; up starts from 2 x 2
    # padded channels
    (3, 12, 20, 3, 64, ("same",)),    # no input gradient (the model keeps no dgrad operand)
    (3, 12, 20, 64, 3, ("same",)),    # c_out padded to 8
    (2, 12, 12, 4, 320, ("same",)),   # SD conv_in (c_in padded to 8)
    (2, 12, 12, 320, 4, ("same",)),   # SD conv_out
    # split contraction: taps * c_src >= 2048 and few output tiles (unet._conv_desc arms split_ws by itself)
    (16, 12, 12, 256, 128, FORMS),    # pipelined + split
    (2, 6, 6, 256, 256, FORMS),       # generic + split
    # beyond the issue's table: with the cases above no stride-2 FORWARD has rows % 256 == 0 (576, 960, 576, 960 rows), so the pipelined
    # tile's stride-2 source addressing would only be run at the power-of-two sizes of test_gpu_unet.py.  12 x 12 outputs, 2304 rows.
    (16, 24, 24, 64, 64, DOWN),
]


def pad8(n):
    return (n + 7) // 8 * 8


def geometry(form, H, W):
    """(h_out, w_out, stride, pad, upsample) as unet._conv3 / sd_unet pass them to sfron_conv_desc"""
    if form == "same":
        return H, W, 1, 1, 0
    if form == "down0":
        return H // 2, W // 2, 2, 0, 0
    if form == "down1":
        return (H - 1) // 2 + 1, (W - 1) // 2 + 1, 2, 1, 0
    if form == "up":
        return 2 * H, 2 * W, 1, 1, 1
    raise ValueError(form)


def has_resid(case):
    """resid on every other case of the table"""
    return CASES.index(case) % 2 == 0


def case_id(case):
    B, H, W, ci, co, _ = case
    return f"{B}x{H}x{W}-{ci}to{co}"


GRID = [(case, form) for case in CASES for form in case[5]]
GRID_IDS = [f"{case_id(case)}-{form}" for case, form in GRID]


def inputs(case, form, ints):
    """x [B][ci][H][W], w [co][ci][3][3] (the fp32 master; wq = what the kernels multiply with, its bf16 rounding), bias [co], vec [B][co],
    resid [B][co][ho][wo] or None, dy [B][co][ho][wo] -- float32 on the CPU, x / wq / dy exact in bf16."""
    B, H, W, ci, co, _ = case
    ho, wo = geometry(form, H, W)[:2]
    g = torch.Generator().manual_seed(1000 * CASES.index(case) + 10 * FORMS.index(form) + int(ints))
    if ints:
        def draw(*shape):
            return torch.randint(-3, 4, shape, generator=g).float()
        x, w, bias, vec, dy = draw(B, ci, H, W), draw(co, ci, 3, 3), draw(co), draw(B, co), draw(B, co, ho, wo)
        resid = draw(B, co, ho, wo) if has_resid(case) else None
    else:
        x = torch.randn(B, ci, H, W, generator=g).to(torch.bfloat16).float()
        w = torch.randn(co, ci, 3, 3, generator=g) * 0.1
        bias, vec = torch.randn(co, generator=g) * 0.1, torch.randn(B, co, generator=g) * 0.5
        dy = (torch.randn(B, co, ho, wo, generator=g) * 0.1).to(torch.bfloat16).float()
        resid = torch.randn(B, co, ho, wo, generator=g) if has_resid(case) else None
    return SimpleNamespace(x=x, w=w, wq=w.to(torch.bfloat16).float(), bias=bias, vec=vec, resid=resid, dy=dy)


def conv_ref(x, w, form):
    if form == "same":
        return F.conv2d(x, w, None, padding=1)
    if form == "down0":
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, None, stride=2, padding=0)
    if form == "down1":
        return F.conv2d(x, w, None, stride=2, padding=1)
    if form == "up":
        return F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, None, padding=1)
    raise ValueError(form)


@functools.lru_cache(maxsize=4)
def reference(case, form, ints):
    """float64 on the CPU, autograd: (inputs, y, dX, dW, d bias, d vec).  Never modified by a caller.  (The whole grid takes under 3 s to
    compute and 370 MiB to keep, so only the last few are kept.)"""
    inp = inputs(case, form, ints)
    x, w, bias, vec = (t.double().requires_grad_(True) for t in (inp.x, inp.wq, inp.bias, inp.vec))
    y = conv_ref(x, w, form) + bias.view(1, -1, 1, 1) + vec[:, :, None, None]
    if inp.resid is not None:
        y = y + inp.resid.double()
    y.backward(inp.dy.double())
    return SimpleNamespace(inp=inp, y=y.detach(), dx=x.grad, dw=w.grad, dbias=bias.grad, dvec=vec.grad)


# ------------------------------------------------------------------------------------------------ which kernel path a (case, form) reaches
def classes(case, form):
    """The paths of csrc/conv.hip that the three products of this (case, form) take, from the shapes alone:
      forward          rows = B h_out w_out outputs, contraction over 9 * pad8(c_in):  pipelined tile iff rows % 256 == 0 and pad8(c_in) % 64 == 0
      input gradient   a convolution of dy (source channels pad8(c_out)) with B H W outputs (down*: over the zero-dilated dy; up: B h_out w_out
                       outputs, then the 2 x 2 sums); only when c_in % 8 == 0;  pipelined iff its rows % 256 == 0 and pad8(c_out) % 64 == 0
      weight gradient  contraction over K = B h_out w_out pixels:  pipelined iff K % 64 == 0, K >= 256, pad8(c_out) >= 64, h_out, w_out >= 2
      split            unet._conv_desc arms split_ws when 9 * (source channels) >= 2048"""
    B, H, W, ci, co, _ = case
    ho, wo = geometry(form, H, W)[:2]
    cip, cop = pad8(ci), pad8(co)
    rows = B * ho * wo
    got = set()
    got.add("fwd pipelined" if rows % 256 == 0 and cip % 64 == 0 else "fwd generic")
    K = rows
    got.add("wgrad pipelined" if K % 64 == 0 and K >= 256 and cop >= 64 and ho >= 2 and wo >= 2 else "wgrad generic")
    if 9 * cip >= 2048:
        got.add("fwd split")
    if ci % 8 == 0:
        drows = B * H * W if form in DOWN else rows
        got.add("dgrad pipelined" if drows % 256 == 0 and cop % 64 == 0 else "dgrad generic")
        if 9 * cop >= 2048:
            got.add("dgrad split")
    else:
        got.add("no dgrad")
    if cip != ci:
        got.add("padded c_in")
    if cop != co:
        got.add("padded c_out")
    if H != W:
        got.add("H != W")
    if any(s & (s - 1) for s in (ho, wo)):
        got.add("not a power of two")
    return got


EVERY_FORM = {"fwd pipelined", "fwd generic", "dgrad pipelined", "dgrad generic", "wgrad pipelined", "wgrad generic", "fwd split", "dgrad split",
              "H != W", "not a power of two"}
SAME_ONLY = {"padded c_in", "padded c_out", "no dgrad"}       # conv_in / conv_out of the models are plain pad-1 convolutions


@pytest.mark.parametrize("form", FORMS)
def test_every_class_is_reached_under_every_form(form):
    reached = set()
    for case, f in GRID:
        if f == form:
            reached |= classes(case, f)
    want = EVERY_FORM | (SAME_ONLY if form == "same" else set())
    assert want <= reached, f"{form}: no case of the table reaches {sorted(want - reached)}"


def test_the_pipelined_weight_gradient_divides_by_20_and_12():
    """the case the issue names: a 12 x 20 output grid, K = 960, so the (b, ho, wo) decode of the pipelined weight-gradient tile divides by
    numbers that are no powers of two and differ from each other"""
    case = CASES[1]
    for form in DOWN:
        ho, wo = geometry(form, case[1], case[2])[:2]
        assert (ho, wo, case[0] * ho * wo) == (12, 20, 960) and "wgrad pipelined" in classes(case, form)


def test_table_is_the_issues_and_resid_is_on_half_of_it():
    assert len(CASES) == 15 and len(set(CASES)) == 15
    assert sum(has_resid(c) for c in CASES[:14]) == 7
    assert has_resid(CASES[12]) != has_resid(CASES[13])        # one split case finishes with resid, one without
    for B, H, W, ci, co, forms in CASES:
        assert H % 2 == 0 and W % 2 == 0 and set(forms) <= set(FORMS)


@pytest.mark.parametrize("case,form", GRID, ids=GRID_IDS)
def test_integer_results_stay_below_2_to_24(case, form):
    """every result of the integer variant is an integer far below 2^24 (so fp32 holds every partial sum of it exactly, given that the
    partial sums of 9 * c_in or B * h_out * w_out terms of magnitude <= 9 are below 2^24 as well: 9 * 9 * 320 and 9 * 9216 are)"""
    r = reference(case, form, True)
    B, H, W, ci, co, _ = case
    ho, wo = geometry(form, H, W)[:2]
    assert 9 * 9 * max(ci, co) + 9 < 2 ** 24 and 9 * B * ho * wo < 2 ** 24
    for name in ("y", "dx", "dw", "dbias", "dvec"):
        t = getattr(r, name)
        assert bool((t == t.round()).all()), name
        assert float(t.abs().max()) < 2 ** 24, (name, float(t.abs().max()))
    assert torch.equal(r.dvec, r.inp.dy.double().sum(dim=(2, 3)))
    assert torch.equal(r.dbias, r.inp.dy.double().sum(dim=(0, 2, 3)))
