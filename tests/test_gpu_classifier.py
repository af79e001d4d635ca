"""GPU: the classifier evaluators -- every kernel of csrc/classify.hip on its own, the 1x1 stride-2 convolution form the ResNet shortcuts add,
whole ResNet-34 / ResNet-50 forward passes against the fp32 torch restatement on the CPU (tests/resnet_torch_ref.py), and the two evaluators
end to end.

Bounds.  Data movement and max / ReLU are bit-exact.  The 1x1 stride-2 form is held to the forward bound of tests/test_gpu_conv_forms.py
(rtol 2e-4, atol 2e-4 sqrt(taps c_in) against float64 on bf16-rounded operands).  The head: (HW + C) 2^-23 sum |terms| per logit, the
first-order bound of any fp32 summation order.  The metrics: 4 x the largest error torch's own fp32 softmax (entropy) shows against
float64 on the same logits, plus one fp32 ulp of the largest value compared; indices exact.  Whole networks: logit rel-L2 against the fp32
restatement <= 2 x e_emul, where e_emul is the rel-L2 between the fp32 restatement and the same restatement with BatchNorm folded and
every convolution input rounded to bf16 -- computed here on the CPU, from the reference alone; the factor 2 leaves room for the fp32
accumulation order, a wrong layer gives O(1).  Every check prints its figures first (pytest -s)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import resnet_torch_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_PAD = 152
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HALF = (0.5, 0.5, 0.5)


def _L():
    from sfron import _lib
    return _lib.lib()


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
        pytest.exit(f"GPU fault in tests/test_gpu_classifier.py: {e}", returncode=3)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _normalise(u8_nhwc, mean, std):
    """ToTensor + Normalize in fp32, as torchvision does it: (x / 255 - mean) / std"""
    x = u8_nhwc.permute(0, 3, 1, 2).to(torch.float32) / 255
    return (x - torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)) / torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)


def _f32(v):
    return [float(np.float32(x)) for x in v]


# ------------------------------------------------------------------------------------------------ the stem's patch matrix
def _unfold_rows(xn):
    """F.unfold of a normalised image as the patch matrix: rows (b, ho, wo), column (kh * 7 + kw) * 3 + c, bf16"""
    B = xn.shape[0]
    u = F.unfold(xn.to(torch.bfloat16).to(torch.float32), 7, padding=3, stride=2)          # [B][c * 49 + tap][L]
    L = u.shape[2]
    return u.view(B, 3, 49, L).permute(0, 3, 2, 1).reshape(B * L, 147).to(torch.bfloat16)


@pytest.mark.parametrize("shape", [(2, 18, 14), (1, 7, 9)])
@pytest.mark.parametrize("mean,std", [(HALF, HALF), (IMAGENET_MEAN, IMAGENET_STD)], ids=["half", "imagenet"])
def test_patches7_is_unfold_of_the_normalised_image(shape, mean, std):
    B, H, W = shape
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    assert (Ho, Wo) == {(18, 14): (9, 7), (7, 9): (4, 5)}[(H, W)]
    u8 = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(H))
    u8[0, 0, 0] = 0                      # byte 0 in a corner: its normalised value is not the padding's 0
    u8[0, -1, -1] = 255
    xn = _normalise(u8, mean, std)
    want = _unfold_rows(xn)
    rows = B * Ho * Wo
    got = torch.full((rows, K_PAD), float("nan"), dtype=torch.bfloat16, device=DEV)
    img = u8.to(DEV)
    _ok(_L().sfron_image_u8_patches7(img.data_ptr(), B, H, W, *_f32(mean), *_f32(std), K_PAD, got.data_ptr(), _sp()), "image_u8_patches7")
    assert torch.equal(_bits(got[:, :147]), _bits(want)), "patch matrix differs from F.unfold of the normalised image"
    assert int(_bits(got[:, 147:]).abs().max()) == 0, "columns 147 .. k_pad - 1 must be +0"
    # positions outside the image: exactly +0.0, not the normalised byte 0
    ones =F.unfold(torch.ones(B, 3, H, W), 7, padding=3, stride=2)
    pad = ones.view(B, 3, 49, -1).permute(0, 3, 2, 1).reshape(rows, 147) == 0
    assert bool(pad.any()) and int(_bits(got[:, :147])[pad].abs().max()) == 0
    # the NCHW entry point on the same normalised values
    got2 = torch.full((rows, K_PAD), float("nan"), dtype=torch.bfloat16, device=DEV)
    xd = xn.to(DEV).contiguous()
    _ok(_L().sfron_nchw_patches7(xd.data_ptr(), B, H, W, K_PAD, got2.data_ptr(), _sp()), "nchw_patches7")
    assert torch.equal(_bits(got2), _bits(got))
    if mean == HALF:                     # the centre tap is the pixel itself: the bits of sfron_image_u8_to_rows_bf16
        r8 = torch.empty(B * H * W, 8, dtype=torch.bfloat16, device=DEV)
        _ok(_L().sfron_image_u8_to_rows_bf16(img.data_ptr(), B, H, W, None, 8, r8.data_ptr(), _sp()), "image_u8_to_rows_bf16")
        centre = got.view(B, Ho, Wo, K_PAD)[..., 72:75]
        assert torch.equal(_bits(centre), _bits(r8.view(B, H, W, 8)[:, 0::2, 0::2, :3]))


# ------------------------------------------------------------------------------------------------ ReLU and the max-pool
@pytest.mark.parametrize("shape", [(2, 9, 7), (1, 8, 8)])
@pytest.mark.parametrize("C", [8, 24, 12])            # 8 and 24: eight channels per thread; 12: four
@pytest.mark.parametrize("relu,negative", [(1, False), (0, False), (0, True)])
def test_relu_maxpool3s2_is_max_pool2d(shape, C, relu, negative):
    B, H, W = shape
    ld = C + 8
    x = torch.randn(B, H, W, ld, generator=torch.Generator().manual_seed(C + H))
    if negative:                         # all negative, no ReLU: a pad treated as 0 would win every border window
        x = -x.abs() - 0.5
    xc = x[..., :C].permute(0, 3, 1, 2)
    want = F.max_pool2d(F.relu(xc) if relu else xc, 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    Ho, Wo = want.shape[1], want.shape[2]
    xd = x.to(DEV)
    yb = torch.full((B, Ho, Wo, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    yf = torch.full((B, Ho, Wo, C), float("nan"), dtype=torch.float32, device=DEV)
    _ok(_L().sfron_relu_maxpool3s2(xd.data_ptr(), ld, B, H, W, C, relu, yb.data_ptr(), yf.data_ptr(), _sp()), "relu_maxpool3s2")
    assert torch.equal(_bits(yf), _bits(want))
    assert torch.equal(_bits(yb), _bits(want.to(torch.bfloat16)))
    if negative:
        assert float(yf.max()) < 0.0
    # either output alone
    yb2, yf2 = torch.zeros_like(yb), torch.zeros_like(yf)
    _ok(_L().sfron_relu_maxpool3s2(xd.data_ptr(), ld, B, H, W, C, relu, yb2.data_ptr(), None, _sp()), "relu_maxpool3s2 bf16")
    _ok(_L().sfron_relu_maxpool3s2(xd.data_ptr(), ld, B, H, W, C, relu, None, yf2.data_ptr(), _sp()), "relu_maxpool3s2 fp32")
    assert torch.equal(_bits(yb2), _bits(yb)) and torch.equal(_bits(yf2), _bits(yf))


def test_relu_rows_bits_minus_zero_and_aliasing():
    rows, C, ld = 5, 24, 32
    x = torch.randn(rows, ld, generator=torch.Generator().manual_seed(3))
    x[0, 0], x[1, 3], x[4, 23] = -0.0, 0.0, -1e-30
    want = torch.relu(x[:, :C])                        # torch keeps -0.0
    assert int(_bits(want)[0, 0]) == -2 ** 31
    xd = x.to(DEV)
    yb = torch.full((rows, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    yf = torch.full((rows, ld), -7.0, dtype=torch.float32, device=DEV)
    _ok(_L().sfron_relu_rows(xd.data_ptr(), ld, rows, C, yb.data_ptr(), yf.data_ptr(), _sp()), "relu_rows")
    assert torch.equal(_bits(yf[:, :C]), _bits(want)) and bool((yf[:, C:] == -7.0).all())
    assert torch.equal(_bits(yb), _bits(want.to(torch.bfloat16)))
    assert torch.equal(_bits(xd), _bits(x))
    # in place: y_f32 is x
    _ok(_L().sfron_relu_rows(xd.data_ptr(), ld, rows, C, yb.data_ptr(), xd.data_ptr(), _sp()), "relu_rows in place")
    assert torch.equal(_bits(xd[:, :C]), _bits(want)) and torch.equal(_bits(xd[:, C:]), _bits(x[:, C:]))
    assert torch.equal(_bits(yb), _bits(want.to(torch.bfloat16)))


# ------------------------------------------------------------------------------------------------ the shortcut's convolution form
@pytest.mark.parametrize("case", [(2, 8, 8, 64, 128), (3, 7, 5, 64, 128), (16, 16, 16, 256, 512)], ids=lambda c: "x".join(map(str, c)))
def test_conv_1x1_stride_2(case):
    """taps = 1, stride = 2, pad = 0 of sfron_conv_fwd, launched as resnet.ResNet._conv launches it (bias + fp32 residual): the generic
    tile (rows 32 and 36) and the pipelined one (rows 1024, a multiple of 256)."""
    from sfron import unet
    B, H, W, ci, co = case
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    rows = B * ho * wo
    g = torch.Generator().manual_seed(ci + H)
    x = torch.randn(B, ci, H, W, generator=g).to(torch.bfloat16)
    w = torch.randn(co, ci, 1, 1, generator=g).to(torch.bfloat16)
    bias = torch.randn(co, generator=g)
    resid = torch.randn(rows, co, generator=g)
    ref = F.conv2d(x.double(), w.double(), bias.double(), stride=2).permute(0, 2, 3, 1).reshape(rows, co) + resid.double()
    assert ref.shape[0] == rows
    xr = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wd, bd, rd = w.view(co, ci).contiguous().to(DEV), bias.to(DEV), resid.to(DEV)

    def run():
        out = torch.full((rows, co), float("nan"), dtype=torch.float32, device=DEV)
        d = unet._conv_desc(B, H, W, ci, ho, wo, co, 1, 2, 0, 0, 0, bias=bd, resid=rd, out_f32=out, ld_out=co)
        _ok(_L().sfron_conv_fwd(ctypes.byref(d), xr.data_ptr(), wd.data_ptr(), _sp()), "conv_fwd 1x1 stride 2")
        return out
    y = run()
    assert torch.equal(_bits(run()), _bits(y))
    err = (y.double().cpu() - ref).abs()
    bound = 2e-4 * math.sqrt(ci) + 2e-4 * ref.abs()
    print(f"[classifier] conv 1x1 s2 {case}: max |err| {float(err.max()):.3e}, worst err/bound {float((err / bound).max()):.3e}")
    assert bool(torch.isfinite(y).all()) and bool((err <= bound).all())


# ------------------------------------------------------------------------------------------------ the head
@pytest.mark.parametrize("case", [(3, 4, 512, 10), (2, 49, 2048, 1000), (1, 1, 64, 7)], ids=lambda c: "x".join(map(str, c)))
def test_pool_fc_against_fp64(case):
    B, HW, C, n = case
    ld = C + 4
    g = torch.Generator().manual_seed(C)
    x = torch.randn(B * HW, ld, generator=g).abs() + 0.1 * torch.randn(B * HW, ld, generator=g)
    w = torch.randn(n, C, generator=g) / math.sqrt(C)
    b = torch.randn(n, generator=g)
    xs = x[:, :C].double().view(B, HW, C)
    pooled64 = xs.mean(1)
    want = pooled64 @ w.double().T + b.double()
    terms = (xs.abs().sum(1) / HW) @ w.double().abs().T + b.double().abs()
    bound = (HW + C) * 2.0 ** -23 * terms
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)

    def run():
        pooled = torch.full((B, C), float("nan"), device=DEV)
        logits = torch.full((B, n), float("nan"), device=DEV)
        _ok(_L().sfron_pool_fc(xd.data_ptr(), ld, B, HW, C, wd.data_ptr(), bd.data_ptr(), n, pooled.data_ptr(), logits.data_ptr(), _sp()), "pool_fc")
        return pooled, logits
    p1, l1 = run()
    p2, l2 = run()
    assert torch.equal(_bits(l1), _bits(l2)) and torch.equal(_bits(p1), _bits(p2)), "two calls differ"
    err = (l1.double().cpu() - want).abs()
    print(f"[classifier] pool_fc {case}: max |err| {float(err.max()):.3e}, worst err/bound {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all())
    assert bool(((p1.double().cpu() - pooled64).abs() <= HW * 2.0 ** -23 * xs.abs().sum(1) / HW).all())
    # without a bias
    logits = torch.empty(B, n, device=DEV)
    _ok(_L().sfron_pool_fc(xd.data_ptr(), ld, B, HW, C, wd.data_ptr(), None, n, p1.data_ptr(), logits.data_ptr(), _sp()), "pool_fc no bias")
    assert bool(((logits.double().cpu() - (want - b.double())).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------ the metrics
def _metric_logits(B, n, seed):
    """distinct, well-spaced values: a scaled permutation per row"""
    g = torch.Generator().manual_seed(seed)
    scale = {10: 0.9, 1000: 0.03, 7: 1.3}[n]
    return torch.stack([torch.randperm(n, generator=g).to(torch.float32) * scale - 3.0 for _ in range(B)])


def _metrics_reference(lg):
    l64 = lg.double()
    p64 = torch.softmax(l64, 1)
    ent64 = -(torch.where(p64 > 0, p64 * torch.log(p64.clamp_min(1e-300)), torch.zeros_like(p64))).sum(1)
    p32 = torch.softmax(lg, 1)
    ent32 = -(torch.where(p32 > 0, p32 * torch.log(p32), torch.zeros_like(p32))).sum(1)
    e_p = float((p32.double() - p64).abs().max())
    e_ent = float((ent32.double() - ent64).abs().max())
    return p64, ent64, e_p, e_ent


def _ulp(v):
    return float(np.spacing(np.float32(v)))


METRIC_FIGURES = {}


@pytest.mark.parametrize("B,n", [(5, 10), (3, 1000), (1, 7)])
def test_classify_metrics_against_fp64(B, n):
    from sfron import classify
    lg = _metric_logits(B, n, n)
    target, topk = (3, 5)
    if B == 5:
        lg[1, 4] = lg[1].min() - 200.0          # a gap of 200: this probability is exactly 0 in fp32
        lg[2, 7] = lg[2, 2] = lg[2].max() + 1.0  # two equal maxima: the lower index wins
    p64, ent64, e_p, e_ent = _metrics_reference(lg)
    order = torch.sort(lg.double(), dim=1, descending=True, stable=True).indices[:, :topk]
    m = classify.classify_metrics(lg.to(DEV), target=target, topk=topk, want_probs=True)
    probs, ent = m["probs"].double().cpu(), m["entropy"].double().cpu()
    bound_p = 4 * e_p + _ulp(float(p64.max()))
    bound_e = 4 * e_ent + _ulp(float(ent64.max()))
    err_p, err_e = float((probs - p64).abs().max()), float((ent - ent64).abs().max())
    print(f"[classifier] metrics [{B}][{n}]: probs |err| {err_p:.3e} (torch fp32 {e_p:.3e}, bound {bound_p:.3e}); "
          f"entropy |err| {err_e:.3e} (torch fp32 {e_ent:.3e}, bound {bound_e:.3e})")
    METRIC_FIGURES[(B, n)] = (err_p, e_p, err_e, e_ent)
    assert bool(torch.isfinite(m["entropy"]).all()), "entropy must stay finite when a probability is 0"
    assert err_p <= bound_p and err_e <= bound_e
    if B == 5:
        assert float(m["probs"][1, 4]) == 0.0 and float(torch.softmax(lg, 1)[1, 4]) == 0.0
        assert bool(torch.isnan(-(torch.softmax(lg, 1) * torch.log(torch.softmax(lg, 1))).sum(1)[1])), "the reference's expression is NaN here"
        assert m["topk_i"][2, :2].tolist() == [2, 7] and int(m["argmax"][2]) == 2
    assert torch.equal(m["topk_i"].cpu().long(), order), "top-k indices"
    assert torch.equal(m["argmax"].cpu().long(), order[:, 0])
    assert torch.equal(_bits(m["topk_p"]), _bits(torch.gather(m["probs"].cpu(), 1, order))), "top-k scores are the probabilities at those indices"
    assert torch.equal(_bits(m["p_target"]), _bits(m["probs"][:, target]))
    # every output is optional; a wider row stride
    wide = torch.full((B, n + 3), 1e30)
    wide[:, :n] = lg
    ent2 = torch.empty(B, device=DEV)
    _ok(_L().sfron_classify_metrics(wide.to(DEV).data_ptr(), n + 3, B, n, 0, 0, None, ent2.data_ptr(), None, None, None, None, _sp()), "metrics")
    assert torch.equal(_bits(ent2), _bits(m["entropy"]))


def test_validate_arithmetic_on_the_fixture_logits(golden_dir):
    """the three numbers of the reference's validate() on its own recorded logits, 7 samples at batch 3 (a short last batch)"""
    from sfron import classify
    z = np.load(os.path.join(golden_dir, "classifier_eval.npz"))
    for run in (0, 1):
        batches = [torch.from_numpy(z[f"run{run}_logits{k}"]) for k in range(3)]
        assert [b.shape[0] for b in batches] == [3, 3, 1]
        got = classify.evaluate_logit_batches((b.to(DEV) for b in batches), 7, int(z[f"run{run}_label"]))
        want = dict(zip(classify.RESULT_COLUMNS, z[f"run{run}_numbers"]))
        allg = torch.cat(batches)
        _, _, e_p, e_ent = _metrics_reference(allg)
        print(f"[classifier] validate run {run}: {got} want {want}")
        assert got["accuracy of forgotten class"] == want["accuracy of forgotten class"]
        assert abs(got["entropy"] - want["entropy"]) <= 2 * (4 * e_ent + _ulp(want["entropy"]))        # ours and the reference's fp32, each within
        assert abs(got["prob of forgotten class"] - want["prob of forgotten class"]) <= 2 * (4 * e_p + _ulp(1.0))


# ------------------------------------------------------------------------------------------------ whole networks
def _images(n, size, seed):
    """n pictures as unlike each other as pictures get (black, white, red, blue, a fine checkerboard, noise, a colour ramp, green; a little
    noise on each): a random network's pooled features are nearly parallel for all inputs, these spread them furthest"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    one, zero = np.ones((size, size)) * 255.0, np.zeros((size, size))
    base = [np.stack([zero, zero, zero], -1), np.stack([one, one, one], -1), np.stack([one, zero, zero], -1), np.stack([zero, zero, one], -1),
            np.stack([((xx // 2 + yy // 2) % 2) * 255.0] * 3, -1), rng.integers(0, 256, (size, size, 3)).astype(np.float64),
            np.stack([xx * 255.0 / size, yy * 255.0 / size, 255.0 - xx * 255.0 / size], -1), np.stack([zero, one, zero], -1)]
    return [np.clip(base[i % len(base)] + rng.normal(0, 6, (size, size, 3)), 0, 255).astype(np.uint8) for i in range(n)]


_NETS = {}


def _net(name):
    """(torch restatement with seeded weights, our model with the same weights), built once"""
    if name not in _NETS:
        from sfron import resnet
        ncls = 10 if name == "resnet34" else 1000
        probe = [_normalise(torch.from_numpy(np.stack(_images(b, s, 5))), HALF, HALF) for s, b in ((64, 3), (224, 2))]
        ref = R.randomize(getattr(R, name)(ncls), seed=34 if name == "resnet34" else 50, logit_cap=20.0 if name == "resnet50" else None, probe=probe)
        ours = getattr(resnet, name)(ncls, device=DEV)
        ours.load_state_dict(ref.state_dict())
        _NETS[name] = (ref, ours)
    return _NETS[name]


NET_FIGURES = {}


@pytest.mark.parametrize("size,batch", [(64, 3), (224, 2)])
@pytest.mark.parametrize("name", ["resnet34", "resnet50"])
def test_whole_network_against_the_fp32_restatement(name, size, batch):
    ref, ours = _net(name)
    u8 = torch.from_numpy(np.stack(_images(batch, size, 5)))
    x = _normalise(u8, HALF, HALF)
    with torch.no_grad():
        want = ref(x)
    emul = R.Emulated(ref)(x)
    e_emul = R.rel_l2(emul, want)
    got = ours.forward_u8(u8.to(DEV), HALF, HALF)
    assert got.shape == want.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    e_gpu, e_gpu_emul = R.rel_l2(got.cpu(), want), R.rel_l2(got.cpu(), emul)
    print(f"[classifier] {name} {size}px batch {batch}: e_emul {e_emul:.3e}, GPU vs fp32 {e_gpu:.3e}, GPU vs emulation {e_gpu_emul:.3e}, "
          f"max |logit| {float(want.abs().max()):.2f}")
    NET_FIGURES[(name, size)] = (e_emul, e_gpu, e_gpu_emul)
    if name == "resnet50":
        assert float(want.abs().max()) <= 20.0
    assert e_gpu <= 2 * e_emul
    # model(x) on the same normalised values: the same patch matrix, the same bits
    assert torch.equal(_bits(ours(x)), _bits(got))
    assert sorted(ours.state_dict()) == sorted(ref.state_dict()) and torch.equal(ours.state_dict()["fc.weight"], ref.state_dict()["fc.weight"])


@pytest.mark.parametrize("name", ["resnet34", "resnet50"])
def test_three_chunks_equal_three_calls(name):
    ref, ours = _net(name)
    u8 = torch.from_numpy(np.stack(_images(5, 64, 9))).to(DEV)
    keep = ours.max_chunk_bytes
    try:
        ours.max_chunk_bytes = 2 * ours.per_sample_bytes(64, 64) + 1
        assert ours.chunk_size(64, 64) == 2
        chunked = ours.forward_u8(u8)
    finally:
        ours.max_chunk_bytes = keep
    assert ours.chunk_size(64, 64) > 5
    parts = torch.cat([ours.forward_u8(u8[0:2]), ours.forward_u8(u8[2:4]), ours.forward_u8(u8[4:5])])
    assert torch.equal(_bits(chunked), _bits(parts))


# ------------------------------------------------------------------------------------------------ the evaluators end to end
def _planted_head(ref, feats, top):
    """fc from the reference's own pooled features: rows 0 .. n-1 = top * pinv(F)^T, no bias, so that on the fp32 reference image i has logit
    `top` in class i and 0 in every other class.  (Rows that are scaled, centred features -- logit[i][c] = s <f_i - m, f_c - m> -- do not
    separate these networks' features: the bf16 emulation moves those logits by 1.7 % of the largest, its top-2 gaps are 0.03 .. 0.6 against
    a needed 20 x error of 2 .. 5, for every seed tried; the features of a random ResNet are nearly parallel, and the emulation's error lies
    along their differences.)  Rows beyond the images stay 0."""
    n = feats.shape[0]
    with torch.no_grad():
        ref.fc.weight.zero_()
        ref.fc.bias.zero_()
        ref.fc.weight[:n] = (top * torch.linalg.pinv(feats.double()).T).float()
    return ref


def _entropy(logits):
    p = torch.softmax(logits.double(), 1)
    return -(torch.where(p > 0, p * torch.log(p.clamp_min(1e-300)), torch.zeros_like(p))).sum(1)


def test_classifier_evaluation_end_to_end(tmp_path):
    """7 PNGs of 32 x 32 in an a/b/c/d folder at batch 3 through classifier_evaluation, against the reference pipeline on the CPU (Pillow
    resize to 224, Normalize(0.5, 0.5), the fp32 restatement, validate's arithmetic in float64).  Entropy and probability: within 2 x the
    mean absolute per-image deviation the bf16 emulation shows from the fp32 restatement (the emulation's signed sum can cancel to nothing
    by chance; its per-image deviations cannot)."""
    from sfron import classify, resnet
    folder = tmp_path / "a" / "b" / "c" / "d"
    os.makedirs(folder)
    pics = _images(7, 32, 21)
    for i, a in enumerate(pics):
        Image.fromarray(a).save(folder / f"{i:03d}.png")
    label = 0
    x = _normalise(torch.from_numpy(np.stack([np.asarray(Image.fromarray(a).resize((224, 224), Image.BILINEAR)) for a in pics])), HALF, HALF)
    ref = R.randomize(R.resnet34(10), seed=7)
    with torch.no_grad():
        ref = _planted_head(ref, ref.features(x), 6.0)
        want = ref(x)
    emul = R.Emulated(ref)(x)
    # preconditions, on the reference alone
    pred = want.argmax(1)
    e_logit = float((emul - want).abs().max())
    top2 = torch.sort(want, 1, descending=True).values
    gap = float((top2[:, 0] - top2[:, 1]).min())
    print(f"[classifier] e2e resnet34: predictions {pred.tolist()}, smallest top-2 gap {gap:.3f}, largest emulation logit error {e_logit:.4f}")
    assert len(set(pred.tolist())) >= 4 and bool((pred == label).any()) and bool((pred != label).any())
    assert gap >= 20 * e_logit
    n = 7
    p_ref, p_em = torch.softmax(want.double(), 1)[:, label], torch.softmax(emul.double(), 1)[:, label]
    want_res = {"entropy": float(_entropy(want).sum() / n), "prob of forgotten class": float(p_ref.sum() / n),
                "accuracy of forgotten class": float((pred == label).sum() / n)}
    tol_ent = 2 * float((_entropy(emul) - _entropy(want)).abs().mean())
    tol_p = 2 * float((p_em - p_ref).abs().mean())

    ours = resnet.resnet34(10, device=DEV).load_state_dict(ref.state_dict())
    csv_path = str(tmp_path / "results" / "result.csv")
    sample_path = str(folder)
    got = classify.classifier_evaluation(ours, sample_path, label_of_forgotten_class=label, batch_size=3, img_size=224, csv_path=csv_path)
    print(f"[classifier] e2e resnet34: got {got}, want {want_res}, tolerances entropy {tol_ent:.3e} prob {tol_p:.3e}")
    assert got["accuracy of forgotten class"] == pytest.approx(want_res["accuracy of forgotten class"], abs=1e-6)
    assert abs(got["entropy"] - want_res["entropy"]) <= tol_ent
    assert abs(got["prob of forgotten class"] - want_res["prob of forgotten class"]) <= tol_p
    lines = open(csv_path).read().splitlines()
    assert lines[0] == ",entropy,prob of forgotten class,accuracy of forgotten class"
    assert lines[1] == "a/b," + ",".join(repr(got[c]) for c in classify.RESULT_COLUMNS) and len(lines) == 2
    got2 = classify.classifier_evaluation(ours, sample_path, label_of_forgotten_class=int(pred[-1]) if int(pred[-1]) != label else int(pred[0]),
                                          batch_size=4, img_size=224, csv_path=csv_path)
    lines = open(csv_path).read().splitlines()
    assert len(lines) == 2 and lines[1] == "a/b," + ",".join(repr(got2[c]) for c in classify.RESULT_COLUMNS)
    assert got2["entropy"] == pytest.approx(got["entropy"], rel=1e-5) and got2 != got
    # the GPU loader's bytes are Pillow's
    files = classify.image_paths(sample_path)
    u8 = classify.load_images_u8(files, (224, 224), device=DEV)
    assert torch.equal(u8.cpu(), torch.from_numpy(np.stack([classify.transform_host(Image.open(f), (224, 224)) for f in files])))


def test_imageclassify_end_to_end(tmp_path):
    """4 PNGs of 64 x 64 named {case}_{k}.png and a 3-row prompts file through imageclassify, against the reference pipeline on the CPU
    (Pillow bilinear resize to 232, centre crop 224, ImageNet mean / std, the fp32 restatement, softmax, top-5)."""
    from sfron import classify, resnet
    folder = tmp_path / "sd_run"
    os.makedirs(folder)
    names = ["0_0.png", "0_1.png", "2_0.png", "7_0.png"]
    pics = _images(4, 64, 33)
    for nme, a in zip(names, pics):
        Image.fromarray(a).save(folder / nme)
    (folder / "notes.txt").write_text("not a picture")
    prompts = tmp_path / "prompts.csv"
    prompts.write_text("case_number,prompt,evaluation_seed,class\n0,Image of a tench,42,tench\n1,Image of a church,7,church\n"
                       "2,Image of a parachute,9,parachute\n")
    host = np.stack([classify.transform_host(Image.fromarray(a), 232, crop=224) for a in pics])
    direct = np.stack([np.asarray(Image.fromarray(a).resize((232, 232), Image.BILINEAR).crop((4, 4, 228, 228))) for a in pics])
    assert np.array_equal(host, direct)
    x = _normalise(torch.from_numpy(host), IMAGENET_MEAN, IMAGENET_STD)
    ref = R.randomize(R.resnet50(1000), seed=7)
    with torch.no_grad():
        ref = _planted_head(ref, ref.features(x), 24.0)
        # the other 996 classes: no weights, a bias that is a permutation of 14, 13, 12, ... -- their logits are the bias itself in both
        # pipelines, exactly, so only a gap next to a planted class can move
        g = torch.Generator().manual_seed(2)
        ref.fc.bias[4:] = 14.0 - torch.randperm(996, generator=g).float()
        want = ref(x)
    emul = R.Emulated(ref)(x)
    e_logit = float((emul - want).abs().max())
    srt = torch.sort(want, 1, descending=True)
    gap = float((srt.values[:, 0] - srt.values[:, 1]).min())
    planted = want[:, :4]
    others = float((srt.values[:, 5:6] - torch.where(torch.eye(4, dtype=torch.bool), torch.full_like(planted, -1e9), planted)).min())
    print(f"[classifier] e2e resnet50: top-6 {srt.indices[:, :6].tolist()}, smallest top-2 gap {gap:.3f}, the sixth logit above the other planted "
          f"classes by {others:.3f}, largest emulation logit error {e_logit:.4f}")
    # preconditions on the reference alone: rank 1 is the image's planted class, ranks 2 .. 6 are bias-only classes (exact in both pipelines, in
    # distinct steps of 1), and every gap next to a logit that carries the network's error is 20 x the emulation's logit error
    assert srt.indices[:, 0].tolist() == [0, 1, 2, 3] and bool((srt.indices[:, 1:6] >= 4).all())
    assert gap >= 20 * e_logit and others >= 20 * e_logit

    ours = resnet.resnet50(1000, device=DEV).load_state_dict(ref.state_dict())
    res = classify.imageclassify(ours, str(folder), str(prompts), topk=5, batch_size=3)
    assert res["case_number"] == [0, 0, 2, 7]
    ids = torch.tensor([res[f"index_top{k}"] for k in range(1, 6)]).T
    assert torch.equal(ids, srt.indices[:, :5]), "top-5 indices"
    assert all(res[f"category_top{k}"] == res[f"index_top{k}"] for k in range(1, 6))
    # the scores against float64 softmax of the model's own logits, within the metrics bound
    lg = ours.forward_u8(classify.load_images_u8([str(folder / n) for n in names], 232, crop=224, device=DEV), IMAGENET_MEAN, IMAGENET_STD).cpu()
    p64, _, e_p, _ = _metrics_reference(lg)
    scores = torch.tensor([[float(v) for v in res[f"scores_top{k}"]] for k in range(1, 6)], dtype=torch.float64).T
    err = float((scores - torch.gather(p64, 1, ids)).abs().max())
    print(f"[classifier] e2e resnet50: scores |err| {err:.3e}, torch fp32 {e_p:.3e}")
    assert err <= 4 * e_p + _ulp(float(p64.max()))
    # the joined file: the prompts that have pictures, at the default path
    out = folder / "sd_run_classification.csv"
    lines = out.read_text().splitlines()
    assert lines[0].startswith(",case_number,prompt,evaluation_seed,class,category_top1,index_top1,scores_top1,") and lines[0].endswith("scores_top5")
    assert [ln.split(",")[:3] for ln in lines[1:]] == [["0", "0", "Image of a tench"], ["1", "0", "Image of a tench"], ["2", "2", "Image of a parachute"]]
    named = classify.imageclassify(ours, str(folder), str(prompts), save_path=str(tmp_path / "named.csv"), topk=2,
                                   categories=[f"class{i}" for i in range(1000)])
    assert named["category_top1"] == [f"class{i}" for i in named["index_top1"]] and named["index_top1"] == res["index_top1"]
