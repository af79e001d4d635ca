"""GPU: the DDPM guided sampler (csrc/ddpm_sample.hip, sfron.unet.Conditional_Model.forward_pair, sfron.ddpm.DDPMSampler) and the runner's
sample modes (sfron.ddpm_sample).

(1) sfron_ddpm_guided_step bit for bit against sfron_axpby + sfron_ddim_step, sfron_ddpm_sampler_advance, refusals; (2) the batch-2B
pair forward against the oracle and against the two-pass mode="test"; (3) the sampler's arithmetic against the reference's own outputs
(tests/golden/ddpm_sampler.npz); (4) the captured step against the eager loop, bit for bit; (5) sfron_images_normalize_u8 byte for byte
against images.make_grid_u8 per image; (6) the drivers down to the PNG files; (7) sampling between SFR-on steps changes nothing.
Every kernel output sits between guard regions."""
import functools
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from test_gpu_unet import SMALL, _pair, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = 1001
GUARD = 64


class Guarded:
    """A device buffer of n elements between two guard regions of a value no kernel here produces."""

    def __init__(self, n, dtype=torch.float32, fill=-777.25):
        self.n, self.fill = n, fill
        self.whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        self.t = self.whole[GUARD:GUARD + n]

    def intact(self):
        return bool((self.whole[:GUARD] == self.fill).all()) and bool((self.whole[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.whole == self.fill).all())


def _L():
    from sfron import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _tables(eta):
    from sfron import ddpm
    b = ddpm.get_beta_schedule(device=DEV)
    rows, ts = ddpm.generalized_coefficients(ddpm._abar_host(b), ddpm.sampling_sequence("uniform", 1000, 6), eta)
    return rows, torch.tensor(rows, dtype=torch.float32, device=DEV), torch.tensor(ts, dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------------------------------------ (1) the step kernel
@pytest.mark.parametrize("n", [1, 7, 2304, 4099])
def test_guided_step_is_bit_equal_to_axpby_then_ddim_step(n):
    L = _L()
    g = torch.Generator().manual_seed(n)
    x, ec, en, nz = (torch.randn(n, generator=g).to(DEV) for _ in range(4))
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    for eta in (0.0, 0.5):
        rows, coef, _ = _tables(eta)
        steps = len(rows)
        noise = nz if eta else None
        for k in (0, steps - 1):
            idx.fill_(k)
            for s in (2.0, -1.0, 0.1, 7.3, None):                    # 0.1 / 7.3: not exact in fp32 -- 1.0 + s is rounded once, from the double
                if s is None:
                    e = ec
                else:
                    e = torch.empty_like(ec)
                    assert L.sfron_axpby(ec.data_ptr(), en.data_ptr(), 1.0 + s, -float(s), n, e.data_ptr(), _stream()) == 0
                want_x, want_x0 = torch.empty_like(x), torch.empty_like(x)
                assert L.sfron_ddim_step(x.data_ptr(), e.data_ptr(), noise.data_ptr() if eta else None, n, *rows[k], want_x.data_ptr(),
                                         want_x0.data_ptr(), _stream()) == 0
                args = (ec.data_ptr(), en.data_ptr() if s is not None else None, noise.data_ptr() if eta else None, s if s is not None else 2.0,
                        coef.data_ptr(), steps, idx.data_ptr(), n)
                out, x0 = Guarded(n), Guarded(n)
                assert L.sfron_ddpm_guided_step(x.data_ptr(), *args, out.t.data_ptr(), x0.t.data_ptr(), _stream()) == 0
                assert torch.equal(out.t, want_x) and torch.equal(x0.t, want_x0), (n, eta, k, s)
                assert out.intact() and x0.intact()
                out2 = Guarded(n)                                                   # without x0_pred
                assert L.sfron_ddpm_guided_step(x.data_ptr(), *args, out2.t.data_ptr(), None, _stream()) == 0
                assert torch.equal(out2.t, want_x) and out2.intact()
                xa = Guarded(n)                                                     # x_next aliasing x
                xa.t.copy_(x)
                assert L.sfron_ddpm_guided_step(xa.t.data_ptr(), *args, xa.t.data_ptr(), None, _stream()) == 0
                assert torch.equal(xa.t, want_x) and xa.intact()
    # an index outside the table is clamped into it
    rows, coef, _ = _tables(0.5)
    want = {}
    for k in (0, len(rows) - 1):
        idx.fill_(k)
        want[k] = torch.empty_like(x)
        assert L.sfron_ddpm_guided_step(x.data_ptr(), ec.data_ptr(), en.data_ptr(), nz.data_ptr(), 2.0, coef.data_ptr(), len(rows), idx.data_ptr(),
                                        n, want[k].data_ptr(), None, _stream()) == 0
    for bad, k in ((len(rows), len(rows) - 1), (1 << 20, len(rows) - 1), (-3, 0)):
        idx.fill_(bad)
        got = Guarded(n)
        assert L.sfron_ddpm_guided_step(x.data_ptr(), ec.data_ptr(), en.data_ptr(), nz.data_ptr(), 2.0, coef.data_ptr(), len(rows), idx.data_ptr(),
                                        n, got.t.data_ptr(), None, _stream()) == 0
        assert torch.equal(got.t, want[k]) and got.intact(), bad


def test_sampler_advance_moves_the_index_and_writes_the_next_timestep():
    L = _L()
    _, _, tseq = _tables(0.0)
    steps = tseq.numel()
    idx = Guarded(1, torch.int32, fill=-9)
    for nt in (1, 6, 300):                                         # 300: more entries than the workgroup has threads
        t = Guarded(nt)
        for k in (0, 3, steps - 2):
            idx.t.fill_(k)
            assert L.sfron_ddpm_sampler_advance(tseq.data_ptr(), steps, idx.t.data_ptr(), t.t.data_ptr(), nt, _stream()) == 0
            assert int(idx.t) == k + 1 and bool((t.t == tseq[k + 1]).all()) and t.intact() and idx.intact()
        idx.t.fill_(steps - 1)                                      # behind the last step: the index reaches `steps`, t keeps the last timestep
        assert L.sfron_ddpm_sampler_advance(tseq.data_ptr(), steps, idx.t.data_ptr(), t.t.data_ptr(), nt, _stream()) == 0
        assert int(idx.t) == steps and bool((t.t == tseq[steps - 1]).all()) and t.intact()
        assert L.sfron_ddpm_sampler_advance(tseq.data_ptr(), steps, idx.t.data_ptr(), t.t.data_ptr(), nt, _stream()) == 0
        assert int(idx.t) == steps                                  # and stays there


def test_refusals_come_before_any_launch():
    L = _L()
    rows, coef, tseq = _tables(0.0)
    n, steps = 100, len(rows)
    x, e = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, x0 = Guarded(n), Guarded(n)
    P = lambda t: t.data_ptr()
    bad = [
        (None, P(e), None, None, 2.0, P(coef), steps, P(idx), n, P(out.t), P(x0.t)),            # no x
        (P(x), None, None, None, 2.0, P(coef), steps, P(idx), n, P(out.t), P(x0.t)),            # no eps
        (P(x), P(e), None, None, 2.0, None, steps, P(idx), n, P(out.t), P(x0.t)),               # no table
        (P(x), P(e), None, None, 2.0, P(coef), steps, None, n, P(out.t), P(x0.t)),              # no index
        (P(x), P(e), None, None, 2.0, P(coef), 0, P(idx), n, P(out.t), P(x0.t)),                # an empty table
        (P(x), P(e), None, None, 2.0, P(coef), steps, P(idx), 0, P(out.t), P(x0.t)),            # no elements
        (P(x), P(e), None, None, float("nan"), P(coef), steps, P(idx), n, P(out.t), P(x0.t)),   # a scale that is no number
        (P(x), P(e), None, None, 2.0, P(coef), steps, P(idx), n, None, P(x0.t)),                # no output
        (P(x), P(e), None, None, 2.0, P(coef), steps, P(idx), n, P(out.t), P(out.t)),           # x0_pred on top of x_next
    ]
    for a in bad:
        assert L.sfron_ddpm_guided_step(*a, _stream()) == ERR_ARG, a
    assert L.sfron_ddpm_guided_step(P(x), P(e), None, None, 2.0, P(coef), steps, P(idx), n, P(out.t), P(x), _stream()) == ERR_ARG
    t = Guarded(8)
    for a in [(None, steps, P(idx), P(t.t), 8), (P(tseq), 0, P(idx), P(t.t), 8), (P(tseq), steps, None, P(t.t), 8),
              (P(tseq), steps, P(idx), None, 8), (P(tseq), steps, P(idx), P(t.t), 0)]:
        assert L.sfron_ddpm_sampler_advance(*a, _stream()) == ERR_ARG, a
    u8 = Guarded(2 * 4 * 4 * 3, torch.uint8, fill=77)
    img = torch.rand(2, 3, 4, 4, device=DEV)
    for a in [(None, 2, 4, 4, P(u8.t)), (P(img), 0, 4, 4, P(u8.t)), (P(img), 2, 0, 4, P(u8.t)), (P(img), 2, 4, -1, P(u8.t)), (P(img), 2, 4, 4, None),
              (P(img), 1 << 20, 32, 32, P(u8.t))]:                  # the last: 2^30 * 3 bytes of image
        assert L.sfron_images_normalize_u8(*a, _stream()) == ERR_ARG, a
    torch.cuda.synchronize()
    assert out.untouched() and x0.untouched() and t.untouched() and u8.untouched() and int(idx) == 0


# ------------------------------------------------------------------------------------------------ (2) the pair forward
def test_pair_forward_against_the_oracle_and_the_two_pass_form():
    """One pass at batch 2B against the oracle (the bounds of test_gpu_unet.test_unet_test_mode_guidance_matches_oracle) and against the
    two-pass mode="test": the pair is no farther from the two-pass output than that output is from the oracle (both measured here) --
    in fact bit-equal to it at this shape, which is asserted.
    The model stays in TRAIN mode: the pair runs without dropout and leaves the mode and the dropout counter alone."""
    L = _L()
    ref, model = _pair(SMALL, seed=5)
    ref.eval()
    g = torch.Generator().manual_seed(6)
    x, t, c = torch.randn(3, 3, 16, 16, generator=g), torch.tensor([0.0, 500.0, 999.0]), torch.tensor([1, 9, 4])
    with torch.no_grad():
        want = ref(x, t, c, mode="test", cond_scale=2.0)
        want0 = ref(x, t, c, mode="test", cond_scale=0)
    xd, td, cd = x.to(DEV), t.to(DEV), c.to(DEV)
    model.train()
    with torch.no_grad():
        model(xd, td, cd, mode="train")                             # a training pass: the dropout counter exists and stands at 1
    counter, plans = model._drop_counter.clone(), sorted(model._drop_plans)
    ec, en = model.forward_pair(xd, td, cd)
    ec0, none = model.forward_pair(xd, td, cd, with_null=False)
    assert model.training and torch.equal(model._drop_counter, counter) and sorted(model._drop_plans) == plans
    assert none is None and ec.shape == en.shape == ec0.shape == (3, 3, 16, 16) and not ec.requires_grad
    assert ec._base is not None and ec._base is en._base            # two views of one tensor
    mix = Guarded(ec.numel())
    assert L.sfron_axpby(ec.contiguous().data_ptr(), en.contiguous().data_ptr(), 3.0, -2.0, ec.numel(), mix.t.data_ptr(), _stream()) == 0
    got = mix.t.view_as(ec)
    e2, e0 = _rel(got, want), _rel(ec0, want0)
    model.eval()
    two, two0 = model(xd, td, cd, mode="test", cond_scale=2.0), model(xd, td, cd, mode="test", cond_scale=0)
    two_n = model._forward(xd, td, cd, keep_mask=torch.zeros(3, dtype=torch.uint8, device=DEV))       # the two-pass form's null pass
    pe, pn = model.forward_pair(xd, td, cd)                          # eval mode: the same bits as in train mode (no dropout either way)
    assert torch.equal(pe, ec) and torch.equal(pn, en)
    d_pair, d_two = _rel(got, two), _rel(two, want)
    print(f"pair forward: vs oracle {e2:.3e} (scale 2) {e0:.3e} (scale 0); pair vs two-pass {d_pair:.3e}, two-pass vs oracle {d_two:.3e}; "
          f"bit-equal halves: {torch.equal(ec0, two0)}, guided: {torch.equal(got, two)}")
    assert e2 < 2e-2 and e0 < 1.5e-2 and mix.intact()
    assert d_pair <= d_two
    # measured: at this shape the halves of the batch-2B pass carry the very bits of the two batch-B passes, so
    # that is what is held -- halves, guided mix, and the conditional-only pass
    assert torch.equal(ec, two0) and torch.equal(en, two_n) and torch.equal(got, two) and torch.equal(ec0, two0)


# ------------------------------------------------------------------------------------------------ (3) the sampler's arithmetic
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_sampler_matches_the_reference_trajectory(eta):
    """The stub model and outputs of tests/golden/ddpm_sampler.npz (DDPM/functions/denoising.py:72-95 run by the reference), through
    last=False, at the tolerance test_gpu_ddpm_loss.test_ddpm_generalized_sampler_matches_reference uses."""
    from sfron import ddpm
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "ddpm_sampler.npz"))
    x, c, A = torch.from_numpy(g["x"]), torch.from_numpy(g["c"]), torch.from_numpy(g["A"]).to(DEV)
    model = lambda xt, t, cc, cond_scale=3.0, mode="test": (torch.einsum("oc,nchw->nohw", A, xt) * torch.cos(t / 300.0).view(-1, 1, 1, 1)
                                                            + 0.01 * cc.view(-1, 1, 1, 1) * cond_scale)
    b = ddpm.get_beta_schedule(device=DEV)
    s = ddpm.DDPMSampler(model, b, timesteps=10, eta=eta, generator=torch.Generator().manual_seed(13))     # the reference's CPU draws
    assert s.seq == list(g["seq"])
    xs, x0s = s.sample_image(x.to(DEV), c.to(DEV), 2.0, last=False)
    assert len(xs) == 11 and len(x0s) == 10
    np.testing.assert_allclose(xs[-1].cpu().numpy(), g[f"last_eta{eta}"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(xs[5].cpu().numpy(), g[f"x_mid_eta{eta}"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(x0s[0].cpu().numpy(), g[f"x0_first_eta{eta}"], rtol=2e-5, atol=2e-5)
    s2 = ddpm.DDPMSampler(model, b, timesteps=10, eta=eta, generator=torch.Generator().manual_seed(13))
    last = s2.sample_image(x.to(DEV), c.to(DEV), 2.0)                # last=True keeps only the current x: the same bits
    assert torch.equal(last, xs[-1])


# ------------------------------------------------------------------------------------------------ (4) eager against graph
@functools.lru_cache(maxsize=None)
def _small_model():
    _, model = _pair(SMALL, seed=5)
    model.eval()
    return model


@pytest.mark.parametrize("cond_scale", [2.0, 0.0])
@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("skip_type,timesteps", [("uniform", 6), ("quad", 5)])
def test_captured_step_replays_to_the_eager_bits(skip_type, timesteps, eta, cond_scale):
    from sfron import ddpm
    model = _small_model()
    b = ddpm.get_beta_schedule(device=DEV)
    g = torch.Generator().manual_seed(31)
    batches = [(torch.randn(n, 3, 16, 16, generator=g).to(DEV), torch.randint(0, 10, (n,), generator=g).to(DEV)) for n in (3, 3, 2)]
    outs = {}
    for graph in (False, True):
        s = ddpm.DDPMSampler(model, b, skip_type=skip_type, timesteps=timesteps, eta=eta, graph=graph,
                             generator=torch.Generator(device=DEV).manual_seed(77))
        assert len(s.seq) == (7 if skip_type == "uniform" else 5)
        outs[graph] = [s.sample_image(x, c, cond_scale) for x, c in batches]
        if graph:
            assert s._g is not None and s._g["graph"] is not None and s._g["key"][0] == (3, 3, 16, 16)      # one graph; batch 2 ran eagerly
    torch.cuda.synchronize()
    for k, (a, bb) in enumerate(zip(outs[False], outs[True])):
        assert torch.isfinite(a).all() and torch.equal(a, bb), (k, (a - bb).abs().max().item())
    assert not torch.equal(outs[False][0], outs[False][1])


# ------------------------------------------------------------------------------------------------ (5) per-image normalised bytes
@pytest.mark.parametrize("H,W", [(32, 32), (16, 16), (5, 7)])
def test_images_normalize_u8_is_make_grid_per_image(H, W):
    from sfron import ddpm_sample, images
    g = torch.Generator().manual_seed(H * W)
    x = torch.rand(5, 3, H, W, generator=g)
    x[1] = 0.37                                                      # a constant image: hi = lo + 1e-5
    x[2] = x[2] * 0.5 + 0.2
    x[2, 2, H - 1, W - 1] = 0.95                                     # the maximum in the last element,
    x[3] = x[3] * 0.5 + 0.2
    x[3, 2, H - 1, W - 1] = 0.01                                     # the minimum in the last element
    x[4] = x[4] * 3.0 - 1.0                                          # values outside [0, 1]: the image's own range, not a fixed one
    x = x.to(DEV)
    B = x.shape[0]
    out = Guarded(B * H * W * 3, torch.uint8, fill=113)
    assert _L().sfron_images_normalize_u8(x.data_ptr(), B, H, W, out.t.data_ptr(), _stream()) == 0
    got = out.t.view(B, H, W, 3)
    for k in range(B):
        want = images.make_grid_u8(x[k:k + 1], normalize=True)
        assert want.shape == (H, W, 3) and torch.equal(got[k], want), k
    assert out.intact() and bool((got[1] == 0).all()) and int(got[2].max()) == 255 and int(got[3].min()) == 0
    assert torch.equal(ddpm_sample.images_normalize_u8(x), got)
    # the documented divergence: a constant image whose lo + 1e-5 rounds back to lo, and an image without a finite value, get bytes of 0
    # (sfron_rows_to_image_u8 refuses such a range); their neighbours in the batch are scaled as ever
    y = x[:3].clone()
    y[0] = 300.0
    y[1] = float("nan")
    out2 = Guarded(3 * H * W * 3, torch.uint8, fill=113)
    assert _L().sfron_images_normalize_u8(y.data_ptr(), 3, H, W, out2.t.data_ptr(), _stream()) == 0
    got2 = out2.t.view(3, H, W, 3)
    assert bool((got2[:2] == 0).all()) and torch.equal(got2[2], got[2]) and out2.intact()


# ------------------------------------------------------------------------------------------------ (6) the drivers
class _Recording:
    """A sampler that keeps what it returned."""

    def __init__(self, sampler):
        self.s, self.out = sampler, []

    def sample_image(self, x, c, cond_scale, last=True):
        self.out.append(self.s.sample_image(x, c, cond_scale, last=last))
        return self.out[-1]


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_drivers_write_the_reference_files(tmp_path):
    from sfron import ddpm, ddpm_sample, images
    model = _small_model()
    cfg = NS(data=NS(channels=3, image_size=16, n_classes=10, rescaled=True, logit_transform=False), sampling=NS(batch_size=2),
             training=NS(visualization_samples=10))
    rec = _Recording(ddpm.DDPMSampler(model, ddpm.get_beta_schedule(device=DEV), timesteps=3))
    gen = torch.Generator(device=DEV).manual_seed(3)
    root = str(tmp_path)

    def check_files(paths):
        k = 0
        for x in rec.out:
            want = ddpm_sample.images_normalize_u8(ddpm_sample.inverse_data_transform(cfg, x)).cpu().numpy()
            for img in want:
                assert np.array_equal(_png(paths[k]), img), paths[k]
                k += 1
        assert k == len(paths)
        rec.out.clear()

    d = ddpm_sample.sample_fid(rec, cfg, root, 2.0, "1,4", 3, device=DEV, generator=gen)
    assert d == os.path.join(root, "fid_samples_guidance_2.0") and sorted(os.listdir(d), key=lambda s: int(s[:-4])) == [f"{k}.png" for k in range(6)]
    assert [tuple(x.shape) for x in rec.out] == [(2, 3, 16, 16), (1, 3, 16, 16)] * 2
    check_files([os.path.join(d, f"{k}.png") for k in range(6)])

    d = ddpm_sample.sample_classes(rec, cfg, root, 2.0, "1,4", 3, device=DEV, generator=gen)
    assert sorted(os.listdir(d)) == ["1", "4"]
    assert sorted(os.listdir(os.path.join(d, "1"))) == ["0.png", "1.png", "2.png"] and sorted(os.listdir(os.path.join(d, "4"))) == ["3.png", "4.png", "5.png"]
    check_files([os.path.join(d, "1", f"{k}.png") for k in range(3)] + [os.path.join(d, "4", f"{k}.png") for k in range(3, 6)])

    d = ddpm_sample.sample_one_class(rec, cfg, root, 2.0, 7, device=DEV, generator=gen, total_n_samples=3)
    assert d == os.path.join(root, "class_7") and sorted(os.listdir(d)) == ["0.png", "1.png", "2.png"]
    check_files([os.path.join(d, f"{k}.png") for k in range(3)])

    p = ddpm_sample.sample_visualization(rec, cfg, "2.0", 2.0, root, device=DEV, generator=gen)
    assert p == os.path.join(root, "sample-2.0.png") and len(rec.out) == 5                    # 10 // 2 rounds of 2
    Hc, Wc = images.grid_geometry(10, 16, 16, nrow=1, padding=0)[:2]
    sheet = _png(p)
    assert sheet.shape == (Hc, Wc, 3) == (160, 16, 3)
    allx = ddpm_sample.inverse_data_transform(cfg, torch.cat(rec.out))
    assert np.array_equal(sheet, images.make_grid_u8(allx, nrow=1, padding=0, normalize=True).cpu().numpy())


# ------------------------------------------------------------------------------------------------ (7) non-interference
@pytest.mark.parametrize("use_graphs", [False, True])
def test_sampling_between_sfron_steps_changes_nothing(use_graphs):
    """Four DDPMSFRon steps (dropout ON: its masks follow the model's own counter) with sampling in the gaps behind steps 0 and 1 against
    four steps alone: parameters, Adam moments and the EMA shadow bit-equal.  With use_graphs the gap behind step 0 is the one in front of
    the step that CAPTURES the stages (StageGraph warm-up 1), and steps 2 and 3 replay them: a sampler that left the model's "convolution
    operands are stale" flag cleared would capture a forget stage without its re-layout, and every replay would run on the operands of
    the weights before the last update.  The SAME graph sampler serves both gaps -- its captured step replays after the weights have
    changed -- and is held to a fresh eager sampler each time."""
    from sfron import ddpm
    from test_gpu_unet import _synthetic
    B, n_it = 4, 4
    g = torch.Generator().manual_seed(61)
    batches = []
    for it in range(n_it):
        pair = []
        for stream in ("forget", "remain"):
            b = _synthetic(it, stream, B, g)
            b["x0"], b["e"] = b["x0"][:, :, :16, :16].contiguous(), b["e"][:, :, :16, :16].contiguous()
            b["keep_mask"] = (torch.rand(B, generator=g) >= 0.1).to(torch.uint8)
            pair.append({k: v.to(DEV) for k, v in b.items()})
        batches.append(pair)
    xs = torch.randn(3, 3, 16, 16, generator=g).to(DEV)
    cs = torch.tensor([0, 3, 7], device=DEV)
    res, pictures = [], []
    for sample in (False, True):
        _, model = _pair(SMALL, seed=60)                            # (seeds torch: the dropout seed follows torch.initial_seed())
        run = ddpm.DDPMSFRon(model, lr=1e-4, forget_alpha=10.0, grad_clip=1.0, ema_rate=1e-4, unlearn_loss="ga", n_iters=n_it, use_graphs=use_graphs)
        graph_sampler = run.sampler(timesteps=3, graph=True) if sample else None
        for it in range(n_it):
            run.step(it, *batches[it])
            if sample and it < 2:
                dirty = model._conv_dirty
                want = run.sampler(timesteps=3).sample_image(xs, cs, 2.0)                    # a fresh eager sampler on the current weights
                got = [graph_sampler.sample_image(xs, cs, 2.0) for _ in range(2)]            # gap 0: capture, then replays; gap 1: replays only
                assert torch.isfinite(want).all() and torch.equal(got[0], want) and torch.equal(got[1], want)
                assert model.training and model._conv_dirty == dirty and model.auto_prep is False
                pictures.append(want)
        if sample:
            assert graph_sampler._g is not None and graph_sampler._g["graph"] is not None
            assert not torch.equal(pictures[0], pictures[1])        # the weights moved between the gaps, and the replayed step saw it
        if use_graphs:
            assert run._graphs["forget"].graph is not None and run._graphs["forget"].calls == n_it          # captured at step 1, replayed at 2 and 3
        torch.cuda.synchronize()
        res.append((run.flat.p.clone(), run.opt.m.clone(), run.opt.v.clone(), run.shadow.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ (8) the checkpoint loader
def test_load_sampling_model_round_trips_a_runner_checkpoint():
    """DDPMSFRon.checkpoint() -> load_sampling_model: weights="model" gives the live parameters, weights="ema" the EMA shadow (a rate of
    0.5 keeps it well away from the weights), with plain and with DataParallel-style "module." keys; the loaded model is in eval mode
    and computes what the live one does; a checkpoint without an EMA entry refuses weights="ema" by name."""
    from sfron import ddpm, ddpm_sample, unet
    from test_gpu_unet import _synthetic
    cfg = unet.config_namespace(ch_mult=[1, 2], num_res_blocks=1, attn_resolutions=[8], image_size=16)
    g = torch.Generator().manual_seed(71)
    pair = []
    for stream in ("forget", "remain"):
        b = _synthetic(0, stream, 4, g)
        b["x0"], b["e"] = b["x0"][:, :, :16, :16].contiguous(), b["e"][:, :, :16, :16].contiguous()
        pair.append({k: v.to(DEV) for k, v in b.items()})
    _, model = _pair(SMALL, seed=70)
    run = ddpm.DDPMSFRon(model, lr=1e-3, ema_rate=0.5, unlearn_loss="ga", n_iters=2)
    run.step(0, *pair)
    states = run.checkpoint(1)
    live, shadow = run.flat.named_views(run.flat.p), run.ema_state_dict()
    assert any(not torch.equal(live[n], shadow[n]) for n in live)
    prefixed = [{"module." + k: v for k, v in states[0].items()}] + states[1:]
    x, t, c = torch.randn(2, 3, 16, 16, device=DEV), torch.tensor([10.0, 900.0], device=DEV), torch.tensor([2, 5], device=DEV)
    for st in (states, prefixed):
        m_raw = ddpm_sample.load_sampling_model(st, cfg, weights="model", device=DEV)
        m_ema = ddpm_sample.load_sampling_model(st, cfg, weights="ema", device=DEV)
        assert not m_raw.training and not m_ema.training
        for n, p in m_raw.named_parameters():
            assert torch.equal(p, live[n]), n
        for n, p in m_ema.named_parameters():
            assert torch.equal(p, shadow[n]), n
        assert torch.equal(m_raw.params_bf16, model.params_bf16)                             # the bf16 shadow the kernels read was re-cast
        ec, en = m_raw.forward_pair(x, t, c)
        wc, wn = model.forward_pair(x, t, c)
        assert torch.equal(ec, wc) and torch.equal(en, wn)
        assert not torch.equal(m_ema.forward_pair(x, t, c)[0], wc)
    no_ema = ddpm.DDPMSFRon(_pair(SMALL, seed=70)[1], ema_rate=None).checkpoint(0)
    assert len(no_ema) == 3
    with pytest.raises(ValueError, match="no EMA entry"):
        ddpm_sample.load_sampling_model(no_ema, cfg, weights="ema", device=DEV)
    assert ddpm_sample.load_sampling_model(no_ema, cfg, weights="model", device=DEV) is not None
    with pytest.raises(ValueError):
        ddpm_sample.load_sampling_model(states, cfg, weights="shadow", device=DEV)
