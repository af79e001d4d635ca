"""GPU: the native KL-f8 VAE encoder (sfron.vae) and the image front-end (sfron.latents) on the MI355X.

Yardsticks: torch formulas for the two new kernels (bitwise where the issue pins bits), the reference fixture tests/golden/vae_encoder.npz
for a small configuration, and the plain-torch fp32 restatement of tests/test_vae_cpu.py for the full KL-f8 encoder.

Tolerances of the bf16 encoder against fp32 (moments: relative RMS error and cosine over all of them; std = exp(0.5 clamp(logvar)):
relative RMS error), stated from the first MI355X run of these tests with a margin of about 3x:
    small configuration vs the reference fixture ........ measured rel-RMS 5.9e-3, std 2.1e-3, cosine 0.99998  -> bound 2e-2, cosine >= 0.9995
    KL-f8, random weights, 256 px (B 2) / 512 px (B 1) .. measured rel-RMS 8.4e-3 / 8.8e-3, std 2.4e-3 / 2.2e-3, cosine 0.99996
                                                          -> bound 3e-2, cosine >= 0.999
    chunked vs one chunk; image route vs cache route .... measured 0 (bitwise) -> bound 1e-3
"""
import json
import os

import numpy as np
import pytest
import torch

from test_vae_cpu import encoder_fp32, images_to_input, random_weights, small_config, small_weights

pytestmark = pytest.mark.gpu
DEV = "cuda"

TOL_SMALL, COS_SMALL = 2e-2, 0.9995
TOL_FULL, COS_FULL = 3e-2, 0.999
TOL_SAME = 1e-3


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "vae_encoder.npz")))


def stats(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    z = want.shape[1] // 2
    rel = float((got - want).norm() / want.norm())
    cos = float(torch.dot(got.flatten(), want.flatten()) / (got.norm() * want.norm()))
    sd = lambda m: torch.exp(0.5 * m[:, z:].clamp(-30, 20))
    rel_std = float((sd(got) - sd(want)).norm() / sd(want).norm())
    return dict(rel_rms=rel, cos=cos, rel_std=rel_std)


def report(name, s):
    print(f"VAE-METRIC {name} {json.dumps(s)}")


def _ldm_format(w):
    return {("encoder." + k if not k.startswith("quant_conv.") else k): v for k, v in w.items()}


def small_encoder(fx, **kw):
    from sfron import vae
    return vae.VAEEncoder.from_state_dict(_ldm_format(small_weights(fx)), **small_config(fx), **kw)


# ------------------------------------------------------------------------------------------------ 1. image kernel
def test_image_kernel_is_the_torch_formula_bit_for_bit():
    from sfron import _lib
    from sfron._lib import check, ptr, stream_ptr
    g = torch.Generator().manual_seed(1)
    u8 = torch.randint(0, 256, (3, 37, 53, 3), generator=g, dtype=torch.uint8)
    u8[0, 0, :3] = torch.tensor([[0, 255, 127], [128, 1, 254], [64, 191, 3]], dtype=torch.uint8)
    for flip in (None, torch.tensor([1, 0, 1], dtype=torch.uint8)):
        rows = torch.full((3 * 37 * 53, 8), 7.0, dtype=torch.bfloat16, device=DEV)
        d_img = u8.to(DEV)
        d_flip = flip.to(DEV) if flip is not None else None
        check(_lib.lib().sfron_image_u8_to_rows_bf16(ptr(d_img), 3, 37, 53, ptr(d_flip), 8, ptr(rows), stream_ptr()), "image_u8_to_rows")
        want = torch.zeros(3 * 37 * 53, 8, dtype=torch.bfloat16)
        want[:, :3] = images_to_input(u8, flip).permute(0, 2, 3, 1).reshape(-1, 3).bfloat16()
        assert torch.equal(rows.cpu().view(torch.int16), want.view(torch.int16)), flip


# ------------------------------------------------------------------------------------------------ 2. tail kernel
def test_tail_kernel_quant_conv_sample_and_fp16():
    from sfron import _lib
    from sfron._lib import check, ptr, stream_ptr
    L = _lib.lib()
    g = torch.Generator().manual_seed(2)
    B, hw, ld, z = 3, 17 * 19, 12, 4
    rows = (torch.randn(B * hw, ld, generator=g) * 4).to(DEV)
    rows[: hw // 3, 4:8] += 60.0                   # logvar beyond the clamp at 20 (and fp16's range) for a part of sample 0
    rows[hw: hw + hw // 3, 4:8] -= 90.0            # and below -30
    w = (torch.randn(2 * z, 2 * z, 1, 1, generator=g) * 0.5).to(DEV)
    b = torch.randn(2 * z, generator=g).to(DEV)
    eps = torch.randn(B, z, 17, 19, generator=g).to(DEV)
    mom = torch.empty(B, 2 * z, 17, 19, device=DEV)
    m16 = torch.empty(B, 2 * z, 17, 19, dtype=torch.float16, device=DEV)
    lat = torch.empty(B, z, 17, 19, device=DEV)
    check(L.sfron_vae_moments(ptr(rows), ld, B, hw, 2 * z, ptr(w), ptr(b), ptr(mom), ptr(m16), ptr(eps), 0.18215, ptr(lat), stream_ptr()),
          "vae_moments")
    x = rows[:, :2 * z].double().cpu()
    want = (x @ w.view(2 * z, 2 * z).double().cpu().T + b.double().cpu()).view(B, hw, 2 * z).permute(0, 2, 1).reshape(B, 2 * z, 17, 19)
    err = float((mom.double().cpu() - want).abs().max() / want.abs().max())
    assert err <= 1e-6, err
    ref = torch.empty_like(lat)
    check(L.sfron_latent_sample(ptr(mom), ptr(eps), B, z, hw, 0.18215, ptr(ref), stream_ptr()), "latent_sample")
    assert torch.equal(lat.view(torch.int32), ref.view(torch.int32))
    assert torch.equal(m16.view(torch.int16), mom.half().view(torch.int16))
    # moments only / fp16 only / latent only: the same bits
    m2 = torch.empty_like(mom)
    check(L.sfron_vae_moments(ptr(rows), ld, B, hw, 2 * z, ptr(w), ptr(b), ptr(m2), None, None, 1.0, None, stream_ptr()), "vae_moments")
    lat2 = torch.empty_like(lat)
    check(L.sfron_vae_moments(ptr(rows), ld, B, hw, 2 * z, ptr(w), ptr(b), None, None, ptr(eps), 0.18215, ptr(lat2), stream_ptr()), "vae_moments")
    assert torch.equal(m2.view(torch.int32), mom.view(torch.int32)) and torch.equal(lat2.view(torch.int32), lat.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 3. small configuration vs the reference
def test_small_config_matches_the_reference_fixture(fx):
    enc = small_encoder(fx)
    got = enc.moments(torch.from_numpy(fx["small_images_u8"]))
    s = stats(got, torch.from_numpy(fx["small_moments"]))
    report("small_vs_reference", s)
    assert s["rel_rms"] <= TOL_SMALL and s["rel_std"] <= TOL_SMALL and s["cos"] >= COS_SMALL, s
    # fp32 NCHW input (SD callers, transforms output) takes the same path after the layout kernel
    got2 = enc.moments(images_to_input(fx["small_images_u8"]).to(DEV))
    assert torch.equal(got2, got)
    # the posterior sample for the reference's eps
    lat = enc.encode(torch.from_numpy(fx["small_images_u8"]), eps=torch.from_numpy(fx["small_eps"]), scale=1.0)
    s2 = stats(torch.cat([lat, lat], 1), torch.cat([torch.from_numpy(fx["small_sample"])] * 2, 1))
    assert s2["rel_rms"] <= TOL_SMALL, s2


# ------------------------------------------------------------------------------------------------ 4. the full KL-f8 encoder
@pytest.mark.parametrize("size,batch", [(256, 2), (512, 1)])
def test_full_kl_f8_vs_fp32(size, batch):
    from sfron import vae
    specs, _ = vae.encoder_plan()
    w = random_weights(specs, seed=10 + size)
    enc = vae.VAEEncoder.from_state_dict(_ldm_format(w))
    g = torch.Generator().manual_seed(size)
    u8 = torch.randint(0, 256, (batch, size, size, 3), generator=g, dtype=torch.uint8)
    got = enc.moments(u8)
    want = encoder_fp32(w, images_to_input(u8), (1, 2, 4, 4), 2)
    assert got.shape == (batch, 8, size // 8, size // 8)
    s = stats(got, want)
    report(f"kl_f8_{size}px_b{batch}", s)
    assert s["rel_rms"] <= TOL_FULL and s["rel_std"] <= TOL_FULL and s["cos"] >= COS_FULL, s


# ------------------------------------------------------------------------------------------------ 5. chunking and determinism
def test_chunked_batch_agrees_and_calls_repeat_bitwise(fx):
    enc1 = small_encoder(fx)
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (5, 64, 64, 3), generator=g, dtype=torch.uint8)
    flip = torch.tensor([0, 1, 1, 0, 1], dtype=torch.uint8)
    one = enc1.moments(u8, flip=flip)
    assert enc1.chunk_size(64, 64) >= 5
    enc2 = small_encoder(fx, max_chunk_bytes=2 * enc1.per_sample_bytes(64, 64))
    assert enc2.chunk_size(64, 64) == 2                 # 3 chunks: 2 + 2 + 1
    many = enc2.moments(u8, flip=flip)
    s = stats(many, one)
    report("chunked_vs_one", s)
    assert s["rel_rms"] <= TOL_SAME and s["rel_std"] <= TOL_SAME, s
    again = enc2.moments(u8, flip=flip)
    assert torch.equal(again, many)
    assert torch.equal(enc1.moments(u8, flip=flip), one)
    # encode() is sfron_latent_sample over moments(), bit for bit
    eps = torch.randn(5, 4, 16, 16, generator=g)
    lat, mom = enc1.encode(u8, eps=eps, flip=flip, return_moments=True)
    assert torch.equal(mom, one)
    from sfron import _lib
    from sfron._lib import check, ptr, stream_ptr
    ref = torch.empty_like(lat)
    e = eps.to(DEV)
    check(_lib.lib().sfron_latent_sample(ptr(mom), ptr(e), 5, 4, 256, 0.18215, ptr(ref), stream_ptr()), "latent_sample")
    assert torch.equal(lat, ref)
    # the 2 GiB invariant is checked before launching
    with pytest.raises(ValueError):
        small_encoder(fx).chunk_size(8192 * 4, 8192 * 4)


# ------------------------------------------------------------------------------------------------ 6. weight formats
def test_weight_formats_give_bitwise_equal_moments(fx, tmp_path):
    from safetensors.torch import save_file
    from sfron import vae
    from test_vae_cpu import _formats
    w = small_weights(fx)
    cfg = small_config(fx)
    u8 = torch.from_numpy(fx["small_images_u8"])
    outs = {}
    for name, sd in _formats(w, fx).items():
        outs[name] = vae.VAEEncoder.from_state_dict(sd, **cfg).moments(u8)
    d = tmp_path / "diffusers_vae"
    d.mkdir()
    save_file({k: v.contiguous() for k, v in _formats(w, fx)["diffusers_new"].items()}, str(d / "diffusion_pytorch_model.safetensors"))
    json.dump({"block_out_channels": [32, 64, 128], "layers_per_block": 1, "latent_channels": 4, "in_channels": 3}, open(d / "config.json", "w"))
    outs["from_pretrained_dir"] = vae.VAEEncoder.from_pretrained(str(d), attn_resolutions=cfg["attn_resolutions"],
                                                                 resolution=cfg["resolution"]).moments(u8)
    torch.save(_formats(w, fx)["compvis"], str(tmp_path / "model.ckpt"))
    outs["from_pretrained_ckpt"] = vae.VAEEncoder.from_pretrained(str(tmp_path / "model.ckpt"), **cfg).moments(u8)
    ref = outs.pop("ldm")
    for name, m in outs.items():
        assert torch.equal(m, ref), name


# ------------------------------------------------------------------------------------------------ 7. ImageFolder -> both routes
def _image_folder(root, classes=("cat", "dog", "eel"), per_class=(5, 4, 6)):
    from PIL import Image
    rng = np.random.default_rng(7)
    sizes = [(70, 97), (131, 66), (64, 64), (150, 140), (81, 95), (77, 201)]
    for ci, (c, n) in enumerate(zip(classes, per_class)):
        d = root / "train" / c
        d.mkdir(parents=True)
        for i in range(n):
            h, w = sizes[(i + ci) % len(sizes)]
            img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
            Image.fromarray(img).save(d / f"img_{i:02d}.png")
    (root / "train" / "dog" / "notes.txt").write_text("not an image")
    return str(root)


def test_image_folder_cache_route_and_online_route_agree(fx, tmp_path):
    from sfron import latents
    data = _image_folder(tmp_path / "data")
    enc = small_encoder(fx)
    counts = latents.encode_image_folder(data, enc, str(tmp_path / "cache"), image_size=64, batch=4, workers=4)
    assert counts == {"cat": 5, "dog": 4, "eel": 6}
    cache = latents.LatentCache(str(tmp_path / "cache"))
    gb, seed = 4, 9
    lat = latents.UnlearnLatentLoader(cache, 1, gb, seed=seed)
    img = latents.UnlearnImageLoader(data, 1, enc, gb, seed=seed, image_size=64, flip_prob=0.0, workers=4)
    worst = 0.0
    for step in range(3):
        for stream in ("forget", "remain"):
            a, b = lat.next(stream), img.next(stream)
            for k in ("y", "t", "noise", "drop"):
                assert torch.equal(a[k], b[k]), (step, stream, k)
            s = stats(torch.cat([a["x0"], a["x0"]], 1), torch.cat([b["x0"], b["x0"]], 1))
            worst = max(worst, s["rel_rms"])
    report("cache_vs_online_route", dict(rel_rms=worst))
    assert worst <= TOL_SAME
    # flips: the same seed draws the same flips; ranks of world 2 reassemble the world-1 batch
    on = latents.UnlearnImageLoader(data, 1, enc, gb, seed=seed, image_size=64, flip_prob=0.5, workers=4)
    on2 = latents.UnlearnImageLoader(data, 1, enc, gb, seed=seed, image_size=64, flip_prob=0.5, workers=4)
    flips = []
    for step in range(4):
        h1, h2 = on.host_batch("remain", step), on2.host_batch("remain", step)
        assert torch.equal(h1["flip"], h2["flip"]) and torch.equal(h1["images"], h2["images"])
        flips.append(h1["flip"])
    assert 0 < int(torch.cat(flips).sum()) < 16
    r0 = latents.UnlearnImageLoader(data, 1, enc, gb, rank=0, world=2, seed=seed, image_size=64, flip_prob=0.5, workers=2)
    r1 = latents.UnlearnImageLoader(data, 1, enc, gb, rank=1, world=2, seed=seed, image_size=64, flip_prob=0.5, workers=2)
    for step in range(2):
        full, p0, p1 = on.next("remain"), r0.next("remain"), r1.next("remain")
        for k in ("y", "t", "noise", "drop"):
            assert torch.equal(full[k][0::2], p0[k]) and torch.equal(full[k][1::2], p1[k]), (step, k)
        x = torch.empty_like(full["x0"])
        x[0::2], x[1::2] = p0["x0"], p1["x0"]
        s = stats(torch.cat([x, x], 1), torch.cat([full["x0"], full["x0"]], 1))
        assert s["rel_rms"] <= TOL_SAME, s


# ------------------------------------------------------------------------------------------------ 8. the step fed by the online route
def test_dit_step_fed_by_the_image_loader(fx, tmp_path):
    from sfron import diffusion, dit, latents, step
    data = _image_folder(tmp_path / "data")
    enc = small_encoder(fx)
    torch.manual_seed(0)
    model = dit.DiT(batch_size=4, input_size=16, patch_size=2, in_channels=4, hidden_size=128, depth=2, num_heads=2, num_classes=3)
    model.train()
    runner = step.DiTSFRon(model, diffusion.create_diffusion(""), lr=1e-4, forget_alpha=0.5)
    loader = latents.UnlearnImageLoader(data, 0, enc, 4, seed=1, image_size=64, workers=4)
    for _ in range(2):
        out = runner.step(loader.next("forget"), loader.next("remain"))
        torch.cuda.synchronize()
        fm, rm = out["forget_mse"].mean().item(), out["remain_mse"].mean().item()
        assert np.isfinite(fm) and np.isfinite(rm), (fm, rm)
