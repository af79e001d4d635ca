"""GPU: the SD image / prompt front end on the MI355X -- the resample kernel against Pillow bit for bit, sd_transform_gpu against the host
route, LatentDiffusion.get_input / shared_step over the small VAE, the fixture CLIP encoder and a SMALL UNet, the nsfw_removal and
generate_fisher drivers against SDSFRon.step / SDFisherAccumulator fed by hand, and setup_model over a synthetic CompVis checkpoint.

Every comparison here is bitwise (torch.equal): the kernel is integer arithmetic specified bit for bit, and the drivers are compared
with the same components called by hand in the same order on an identically seeded model, whose repeatability the suite already asserts
bitwise (test_gpu_vae.py::test_chunked_batch_agrees_and_calls_repeat_bitwise, test_gpu_sd.py::test_sd_unet_forward_backward_bitwise_reproducible,
VAEEncoder.encode = sfron_latent_sample over moments())."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from test_sd_front_end_cpu import CASES, FILTERS, PIL_FILTER, case_image
from test_vae_cpu import images_to_input

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0xA5


def _window(n):
    """A crop window strictly inside an axis of n outputs (n >= 3): (first, count)."""
    first = max(1, n // 5)
    return first, max(1, n - first - max(1, n // 7))


def _guarded(n, lead):
    """n bytes between two guard regions; the payload starts ``lead`` bytes into the allocation (odd: not dword-aligned)."""
    buf = torch.full((lead + n + 64,), GUARD, dtype=torch.uint8, device=DEV)
    return buf, buf[lead:lead + n]


def _guards_intact(buf, lead, n):
    return bool((buf[:lead] == GUARD).all()) and bool((buf[lead + n:] == GUARD).all())


# ------------------------------------------------------------------------------------------------ 1. the kernel
# the CPU cases (odd source widths: unaligned rows; (9, 7) -> (64, 64): bounds clipped at both edges; (16, 16) -> (16, 40) and
# (64, 64) -> (64, 64): identity axes; (140, 71) -> (12, 6): bicubic ksize 49, lanczos 73; every other case saturated to {0, 255}) and one
# whose column span does not fit the staged LDS span for the wide filters ((5, 12001) -> (5, 4): the rows are read from global memory)
GPU_CASES = CASES + [((5, 12001), (5, 4))]


@pytest.mark.parametrize("filt", FILTERS)
def test_kernel_equals_pillow_resize_window_bit_for_bit(filt):
    from sfron import _lib, resample
    for ci, ((H, W), (oh, ow)) in enumerate(GPU_CASES):
        a = case_image(ci, H, W)
        fy, ny = _window(oh)
        fx, nx = _window(ow)
        want = np.asarray(Image.fromarray(a).resize((ow, oh), PIL_FILTER[filt]))[fy:fy + ny, fx:fx + nx]
        tx, ty = resample.resample_tables(W, ow, filt, fx, nx), resample.resample_tables(H, oh, filt, fy, ny)
        y0, y1 = ty.rows()
        n_tmp, n_dst = (y1 - y0) * nx * 3, ny * nx * 3
        sbuf, src = _guarded(H * W * 3, 1 + ci % 4)                 # the source starts at every alignment
        src.copy_(torch.from_numpy(a).reshape(-1))
        tbuf, tmp = _guarded(n_tmp, 13)
        dbuf, dst = _guarded(n_dst, 7)
        assert resample.image_resample_u8(src, H, W, tx, ty, tmp, dst, tmp_bytes=n_tmp) == 0, (ci, filt)
        torch.cuda.synchronize()
        got = dst.cpu().numpy().reshape(ny, nx, 3)
        assert np.array_equal(got, want), (ci, filt, int(np.abs(got.astype(int) - want).max()))
        assert _guards_intact(tbuf, 13, n_tmp) and _guards_intact(dbuf, 7, n_dst), (ci, filt)
        assert np.array_equal(sbuf.cpu().numpy()[1 + ci % 4:1 + ci % 4 + H * W * 3].reshape(H, W, 3), a)


def test_kernel_refusals_leave_the_outputs_untouched():
    from sfron import _lib, resample
    from sfron._lib import ptr, stream_ptr
    H, W, oh, ow = 37, 53, 16, 23
    a = case_image(0, H, W)
    tx, ty = resample.resample_tables(W, ow, "bicubic", 2, 17), resample.resample_tables(H, oh, "bicubic", 3, 10)
    y0, y1 = ty.rows()
    n_tmp, n_dst = (y1 - y0) * 17 * 3, 10 * 17 * 3
    src = torch.from_numpy(a).to(DEV).reshape(-1)
    tbuf, tmp = _guarded(n_tmp, 4)
    dbuf, dst = _guarded(n_dst, 4)
    untouched = lambda: bool((dbuf == GUARD).all()) and bool((tbuf == GUARD).all())
    E = _lib.ERR_ARG
    # through the wrapper: a null pointer, tmp_bytes one byte short, bounds outside the source
    assert resample.image_resample_u8(src, H, W, tx, ty, tmp, None, tmp_bytes=n_tmp) == E
    assert resample.image_resample_u8(None, H, W, tx, ty, tmp, dst, tmp_bytes=n_tmp) == E
    assert resample.image_resample_u8(src, H, W, tx, ty, None, dst, tmp_bytes=n_tmp) == E
    assert resample.image_resample_u8(src, H, W, tx, ty, tmp, dst, tmp_bytes=n_tmp - 1) == E
    assert resample.image_resample_u8(src, y1 - 1, W, tx, ty, tmp, dst, tmp_bytes=n_tmp) == E          # the last row read is y1 - 1
    assert resample.image_resample_u8(src, H, tx.rows()[1] - 1, tx, ty, tmp, dst, tmp_bytes=n_tmp) == E
    # the entry point itself: null pointers, zero / negative extents, ksize 0, tmp_bytes below one row
    (kx, bx), (ky, by) = tx.device(DEV), ty.device(DEV)
    good = [ptr(src), H, W, ptr(kx), ptr(bx), tx.ksize, ptr(ky), ptr(by), ty.ksize, 17, 10, ptr(tmp), n_tmp, ptr(dst)]
    L = _lib.lib()
    for pos in (0, 3, 4, 6, 7, 11, 13):
        bad = list(good)
        bad[pos] = None
        assert L.sfron_image_resample_u8(*bad, stream_ptr()) == E, pos
    for pos in (1, 2, 5, 8, 9, 10):
        for v in (0, -1):
            bad = list(good)
            bad[pos] = v
            assert L.sfron_image_resample_u8(*bad, stream_ptr()) == E, (pos, v)
    bad = list(good)
    bad[12] = 17 * 3 - 1
    assert L.sfron_image_resample_u8(*bad, stream_ptr()) == E
    torch.cuda.synchronize()
    assert untouched()
    assert L.sfron_image_resample_u8(*good, stream_ptr()) == 0                     # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    want = np.asarray(Image.fromarray(a).resize((ow, oh), Image.BICUBIC))[3:13, 2:19]
    assert np.array_equal(dst.cpu().numpy().reshape(10, 17, 3), want)


# ------------------------------------------------------------------------------------------------ 2. the transform
def _mixed_images(seed=3):
    rng = np.random.default_rng(seed)
    rgb = lambda h, w: Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8))
    return [rgb(41, 97), rgb(90, 37), rgb(32, 50), Image.fromarray(rng.integers(0, 256, size=(45, 70), dtype=np.uint8)),
            Image.fromarray(rng.integers(0, 256, size=(60, 39, 4), dtype=np.uint8)), rgb(300, 201)]


def test_sd_transform_gpu_equals_the_host_route():
    from sfron import resample
    imgs = _mixed_images()
    assert [i.mode for i in imgs] == ["RGB", "RGB", "RGB", "L", "RGBA", "RGB"]
    for interp in ("bicubic", "lanczos"):
        want = torch.from_numpy(np.stack([resample.sd_transform(i, 32, interp) for i in imgs]))
        got = resample.sd_transform_gpu(imgs, 32, interp, device=DEV)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (6, 32, 32, 3) and got.is_cuda
        assert torch.equal(got.cpu(), want), interp
    # host arrays in, a caller's output buffer, and the staging buffers reused by a second, larger call
    arrs = [np.asarray(i) for i in imgs[:3]] * 3
    out = torch.zeros(9, 32, 32, 3, dtype=torch.uint8, device=DEV)
    assert resample.sd_transform_gpu(arrs, 32, out=out) is out
    want = torch.from_numpy(np.stack([resample.sd_transform(i, 32) for i in imgs[:3]] * 3))
    assert torch.equal(out.cpu(), want)


# ------------------------------------------------------------------------------------------------ 3. the models
S_IMG, S_LAT = 32, 8
PROMPT_F, PROMPT_P = "a photo of a nude person", "a photo of a person wearing clothes"


@pytest.fixture(scope="module")
def stages(golden_dir, tmp_path_factory):
    """The small VAE encoder / decoder of the fixtures (32 px -> 8 x 8 latents) and the fixture CLIP encoder; read-only, shared."""
    from test_gpu_text_encoder import fixture_encoder
    from test_gpu_vae import small_encoder
    from test_gpu_vae_decoder import small_decoder
    fx = dict(np.load(os.path.join(golden_dir, "vae_encoder.npz")))
    dfx = dict(np.load(os.path.join(golden_dir, "vae_decoder.npz")))
    tfx = dict(np.load(os.path.join(golden_dir, "text_encoder.npz")))
    return dict(enc=small_encoder(fx), dec=small_decoder(dfx), cond=fixture_encoder(tfx, str(tmp_path_factory.mktemp("tok"))), fx=fx, dfx=dfx,
                tfx=tfx)


def _unet(stages, seed):
    from test_gpu_sd import SMALL, _pair
    return _pair(dict(SMALL, context_dim=stages["cond"].D), seed=seed)[1]


def _ldm(stages, seed):
    from sfron import sd
    return sd.LatentDiffusion(_unet(stages, seed), first_stage_decoder=stages["dec"], cond_stage_model=stages["cond"],
                              first_stage_encoder=stages["enc"])


def _arena_equal(model, a, b):
    return [n for n in model.index if not torch.equal(model.view(a, n), model.view(b, n))]


def test_get_input_equals_the_components(stages):
    enc, cond = stages["enc"], stages["cond"]
    ldm = _ldm(stages, 70)
    g = torch.Generator().manual_seed(71)
    u8 = torch.randint(0, 256, (3, S_IMG, S_IMG, 3), generator=g, dtype=torch.uint8)
    eps = torch.randn(3, 4, S_LAT, S_LAT, generator=g).to(DEV)
    prompts = [PROMPT_F, PROMPT_P, ""]
    nchw = images_to_input(u8, None).to(DEV)                              # fp32 [B, 3, H, W]: the bytes the uint8 input kernel forms
    z_want, c_want = enc.encode(u8, eps=eps), cond.encode(prompts)
    assert tuple(z_want.shape) == (3, 4, S_LAT, S_LAT)
    for name, x in (("uint8", u8.to(DEV)), ("nchw view", nchw.permute(0, 2, 3, 1)), ("nhwc", nchw.permute(0, 2, 3, 1).contiguous()),
                    ("uint8 host", u8)):
        z, c = ldm.get_input({"jpg": x, "txt": prompts}, "jpg", eps=eps)
        assert torch.equal(z, z_want), name
        assert torch.equal(c, c_want), name
    z1, c1, x1 = ldm.get_input({"jpg": nchw.permute(0, 2, 3, 1), "txt": prompts}, "jpg", bs=1, eps=eps[:1], return_x=True)
    assert torch.equal(z1, enc.encode(u8[:1], eps=eps[:1])) and torch.equal(c1, c_want[:1]) and torch.equal(x1, nchw[:1])
    # the posterior object, and a generator in place of eps
    post = ldm.encode_first_stage(u8.to(DEV))
    assert torch.equal(post.parameters, enc.moments(u8)) and torch.equal(post.mode(), post.parameters[:, :4])
    assert torch.equal(ldm.get_first_stage_encoding(post, eps=eps), z_want)
    assert torch.equal(post.sample(eps=eps), enc.encode(u8, eps=eps, scale=1.0))
    ga, gb = torch.Generator(device=DEV).manual_seed(5), torch.Generator(device=DEV).manual_seed(5)
    za = ldm.get_input({"jpg": u8, "txt": prompts}, "jpg", generator=ga)[0]
    assert torch.equal(za, enc.encode(u8, eps=torch.randn(3, 4, S_LAT, S_LAT, generator=gb, device=DEV)))
    # xrec through the attached decoder
    z, c, x, xrec = ldm.get_input({"jpg": u8, "txt": prompts}, "jpg", eps=eps, return_first_stage_outputs=True)
    assert torch.equal(xrec, stages["dec"].decode(z_want)) and torch.equal(x, images_to_input(u8.to(DEV), None))      # (the formula, on the device)


def test_shared_step_equals_p_losses_with_the_same_draws(stages):
    g = torch.Generator().manual_seed(72)
    u8 = torch.randint(0, 256, (2, S_IMG, S_IMG, 3), generator=g, dtype=torch.uint8)
    batch = {"jpg": images_to_input(u8, None).to(DEV).permute(0, 2, 3, 1), "txt": [PROMPT_P, PROMPT_P]}
    a = _ldm(stages, 73).train()
    loss_a, d = a.shared_step(batch, generator=torch.Generator(device=DEV).manual_seed(9))
    loss_a.backward()
    assert "train/loss_simple" in d
    b = _ldm(stages, 73).train()
    gen = torch.Generator(device=DEV).manual_seed(9)
    eps = torch.randn(2, 4, S_LAT, S_LAT, generator=gen, device=DEV)                        # the documented order: eps, t, noise
    t = torch.randint(0, 1000, (2,), generator=gen, device=DEV).long()
    noise = torch.randn(2, 4, S_LAT, S_LAT, generator=gen, device=DEV)
    z, c = stages["enc"].encode(u8, eps=eps), stages["cond"].encode([PROMPT_P, PROMPT_P])
    loss_b, _ = b.p_losses(z, c, t, noise)
    loss_b.backward()
    assert loss_a.item() == loss_b.item()
    ma, mb = a.model.diffusion_model, b.model.diffusion_model
    bad = [n for n in ma.index if not torch.equal(ma.view(ma.grads, n), mb.view(mb.grads, n))]
    assert not bad, bad[:8]
    assert float(ma.grads.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 4. loader and drivers
def _write_folder(root, n, seed):
    """n images of mixed sizes and modes (RGB, L, RGBA, P) as PNG files."""
    rng = np.random.default_rng(seed)
    os.makedirs(root)
    sizes = [(40, 61), (70, 33), (32, 32), (45, 90), (128, 50)]
    for i in range(n):
        h, w = sizes[(i + seed) % len(sizes)]
        img = Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8))
        if i % 5 == 1:
            img = img.convert("L")
        elif i % 5 == 2:
            img = img.convert("RGBA")
        elif i % 5 == 4:
            img = img.quantize(32)
        img.save(os.path.join(root, f"im_{i:02d}.png"))
    return str(root)


def _host_images(folder):
    from sfron import latents, resample
    return [torch.from_numpy(resample.sd_transform(Image.open(f), S_IMG)) for f in latents.class_files(folder)]


def _batches(images, bs, n):
    """cycle(DataLoader(images, bs)): n batches, the last of a pass short."""
    per = [images[i:i + bs] for i in range(0, len(images), bs)]
    return [torch.stack(per[i % len(per)]) for i in range(n)]


def test_concept_image_loader_on_the_device(tmp_path):
    from sfron import sd
    folder = _write_folder(tmp_path / "f", 5, 1)
    want = _batches(_host_images(folder), 2, 7)
    for gpu_resize in (True, False):
        ld = sd.ConceptImageLoader(folder, 2, image_size=S_IMG, gpu_resize=gpu_resize, workers=4, device=DEV)
        assert len(ld) == 3
        for i, w in enumerate(want):
            got = ld.next()
            assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), w), (gpu_resize, i)
            assert torch.equal(ld.host_batch(i), w)


@pytest.mark.parametrize("method", ("xattn", "full"))
def test_nsfw_removal_driver_equals_steps_fed_by_hand(stages, tmp_path, method):
    from sfron import sd
    enc, cond = stages["enc"], stages["cond"]
    f_dir, r_dir = _write_folder(tmp_path / "forget", 5, 2), _write_folder(tmp_path / "remain", 3, 3)
    n_iters, bs, seed, hp = 4, 2, 11, dict(lr=1e-4, forget_alpha=0.7, remain_alpha=1.3)
    # the driver: iteration 3 takes the short forget batch, iteration 2 the short remain batch, iteration 4 wraps the forget folder around
    ldm = _ldm(stages, 80)
    fl = sd.ConceptImageLoader(f_dir, bs, image_size=S_IMG, gpu_resize=True, workers=4, device=DEV)
    rl = sd.ConceptImageLoader(r_dir, bs, image_size=S_IMG, gpu_resize=True, workers=4, device=DEV)
    saved = []
    run, f_hist, r_hist = sd.nsfw_removal(ldm, fl, rl, n_iters, method, seed=seed, log_every=2, save_every=2,
                                          on_save=lambda r, s: saved.append(s), **hp)
    torch.cuda.synchronize()
    assert saved == [2, 4] and len(f_hist) == len(r_hist) == n_iters and all(isinstance(v, float) for v in f_hist + r_hist)
    # by hand: Pillow's transform, moments + two draws, SDSFRon.step
    from sfron import _lib
    from sfron._lib import check, ptr, stream_ptr

    def draw(mom, eps):
        n = mom.shape[0]
        out = torch.empty(n, 4, S_LAT, S_LAT, dtype=torch.float32, device=DEV)
        check(_lib.lib().sfron_latent_sample(ptr(mom), ptr(eps), n, 4, S_LAT * S_LAT, 0.18215, ptr(out), stream_ptr()), "latent_sample")
        return out

    model = _unet(stages, 80)
    hand = sd.SDSFRon(model, train_method=method, **hp)
    fb, rb = _batches(_host_images(f_dir), bs, n_iters), _batches(_host_images(r_dir), bs, n_iters)
    assert [b.shape[0] for b in fb] == [2, 2, 1, 2] and [b.shape[0] for b in rb] == [2, 1, 2, 1]
    gen = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda n: torch.randn(n, 4, S_LAT, S_LAT, generator=gen, device=DEV)
    ti = lambda n: torch.randint(0, 1000, (n,), generator=gen, device=DEV).long()
    ctx = lambda p, n: cond.encode([p] * n)
    f_want, r_want = [], []
    for xf, xr in zip(fb, rb):
        n, nr = xf.shape[0], xr.shape[0]
        mom = enc.moments(xf)
        x_f, x_p = draw(mom, rn(n)), draw(mom, rn(n))                        # eps_f, eps_p
        t, noise = ti(n), rn(n)
        x_r = draw(enc.moments(xr), rn(nr))                                  # eps_r
        t_r, noise_r = ti(nr), rn(nr)
        out = hand.step(dict(x_f=x_f, x_p=x_p, c_f=ctx(PROMPT_F, n), c_p=ctx(PROMPT_P, n), t=t, noise=noise),
                        dict(x=x_r, c=ctx(PROMPT_P, nr), t=t_r, noise=noise_r))
        f_want.append(out["forget_loss"].item())
        r_want.append(out["remain_loss"].item())
    torch.cuda.synchronize()
    assert f_hist == f_want and r_hist == r_want
    got = run.unet
    assert torch.equal(got.params, model.params)
    assert torch.equal(run.opt.m, hand.opt.m) and torch.equal(run.opt.v, hand.opt.v)
    assert run.opt.step_count == hand.opt.step_count == 2 * n_iters


def test_fisher_driver_equals_the_accumulator_fed_by_hand(stages, tmp_path):
    from sfron import fisher, sd
    enc, cond = stages["enc"], stages["cond"]
    f_dir, r_dir = _write_folder(tmp_path / "forget", 3, 4), _write_folder(tmp_path / "remain", 2, 5)
    ldm = _ldm(stages, 90)
    fl = sd.ConceptImageLoader(f_dir, 2, image_size=S_IMG, gpu_resize=True, workers=4, device=DEV)
    rl = sd.ConceptImageLoader(r_dir, 2, image_size=S_IMG, gpu_resize=True, workers=4, device=DEV)
    got_f, got_r = fisher.sd_generate_fisher(ldm, fl, rl, c_guidance=7.5, forget_prompt=PROMPT_F, remain_prompt=PROMPT_P, seed=13)
    model = _unet(stages, 90)
    sched = sd.LDMSchedule(device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(13)
    want = []
    for folder, prompt in ((f_dir, PROMPT_F), (r_dir, PROMPT_P)):
        images = _host_images(folder)
        nb = (len(images) + 1) // 2
        acc = fisher.SDFisherAccumulator(model, sched, n_batches=nb, c_guidance=7.5)
        for x in _batches(images, 2, nb):
            n = x.shape[0]
            eps = torch.randn(n, 4, S_LAT, S_LAT, generator=gen, device=DEV)
            t = torch.randint(0, 1000, (n,), generator=gen, device=DEV).long()
            noise = torch.randn(n, 4, S_LAT, S_LAT, generator=gen, device=DEV)
            acc.accumulate(dict(x=enc.encode(x, eps=eps), c=cond.encode([prompt] * n), c_null=cond.encode([""] * n), t=t, noise=noise))
        want.append(acc.state_dict())
    for got, w in ((got_f, want[0]), (got_r, want[1])):
        assert list(got.keys()) == list(w.keys())
        bad = [k for k in w if not torch.equal(got[k], w[k])]
        assert not bad, bad[:8]
        assert sum(float(v.sum()) for v in got.values()) > 0
    assert not torch.equal(got_f[next(iter(got_f))], got_r[next(iter(got_r))])


def test_setup_model_from_a_synthetic_compvis_checkpoint(stages, tmp_path):
    from test_gpu_sd import SMALL
    from test_gpu_text_encoder import fixture_tokenizer
    from test_gpu_vae import _ldm_format as enc_format
    from test_gpu_vae_decoder import _ldm_format as dec_format
    from test_text_encoder_cpu import fixture_config, fixture_weights
    from test_vae_cpu import small_config, small_weights
    from test_vae_decoder_cpu import small_decoder_config, small_decoder_weights
    from sfron import sd
    ldm = _ldm(stages, 95)
    unet = ldm.model.diffusion_model
    ckpt = {"model.diffusion_model." + k: v for k, v in unet.state_dict().items()}
    ckpt.update({"first_stage_model." + k: v for k, v in enc_format(small_weights(stages["fx"])).items()})
    ckpt.update({"first_stage_model." + k: v for k, v in dec_format(small_decoder_weights(stages["dfx"])).items()})
    ckpt.update({"cond_stage_model.transformer." + k: v for k, v in fixture_weights(stages["tfx"]).items()})
    ckpt["model_ema.decay"] = torch.tensor(0.9999)                          # a key no part owns
    path = str(tmp_path / "model.ckpt")
    torch.save({"state_dict": ckpt, "global_step": 0}, path)
    assert small_config(stages["fx"]) == small_decoder_config(stages["dfx"])
    _, heads = fixture_config(stages["tfx"])
    kw = dict(vae_kwargs=small_config(stages["fx"]), text_kwargs=dict(heads=heads), **dict(SMALL, context_dim=stages["cond"].D))
    tok = fixture_tokenizer(stages["tfx"], str(tmp_path))
    g = torch.Generator().manual_seed(96)
    u8 = torch.randint(0, 256, (2, S_IMG, S_IMG, 3), generator=g, dtype=torch.uint8)
    eps = torch.randn(2, 4, S_LAT, S_LAT, generator=g).to(DEV)
    t = torch.randint(0, 1000, (2,), generator=g).to(DEV)
    batch = {"jpg": u8, "txt": [PROMPT_F, "a photo"]}
    z_want, c_want = ldm.get_input(batch, "jpg", eps=eps)
    with torch.no_grad():
        out_want = ldm.apply_model(z_want, t, c_want)
    for src in (path, {"state_dict": ckpt}, ckpt):
        built = sd.setup_model(src, tok, device=DEV, **kw)
        assert built.first_stage_encoder is not None and built.first_stage_decoder is not None and built.cond_stage_model is not None
        z, c = built.get_input(batch, "jpg", eps=eps)
        assert torch.equal(z, z_want) and torch.equal(c, c_want)
        with torch.no_grad():
            assert torch.equal(built.apply_model(z, t, c), out_want)
        assert torch.equal(built.decode_first_stage(z), ldm.decode_first_stage(z_want))
    with pytest.raises(KeyError, match="first_stage_model"):
        sd.setup_model({k: v for k, v in ckpt.items() if not k.startswith("first_stage_model.")}, tok, device=DEV, **kw)
