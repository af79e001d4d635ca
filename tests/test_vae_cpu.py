"""CPU: the KL-f8 VAE encoder's host side -- structure, weight formats, centre crop, ctypes prototypes -- against
tests/golden/vae_encoder.npz (made by tests/golden/make_vae_golden.py from the reference Encoder, convertModels.py and DiT/forget.py).
``encoder_fp32`` here is a plain-torch restatement of the encoder over canonical (ldm) names; the GPU tests use it as their fp32 yardstick."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "vae_encoder.npz")))


def small_config(fx):
    c = fx["small_config"]
    return dict(ch=int(c[0]), num_res_blocks=int(c[1]), z_channels=int(c[2]), resolution=int(c[3]), ch_mult=tuple(int(v) for v in c[4:]),
                attn_resolutions=tuple(int(v) for v in fx["small_attn_resolutions"]))


def small_weights(fx):
    """The fixture's weights, regenerated from its seed (make_vae_golden.gen_weights) and checked against the stored per-key sums."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_vae_golden", os.path.join(ROOT, "tests", "golden", "make_vae_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    shapes = {str(k): tuple(int(d) for d in str(s).split(",")) for k, s in zip(fx["small_keys"], fx["small_shapes"])}
    w = mg.gen_weights(shapes)
    for k, s in zip(fx["small_keys"], fx["small_weight_sums"]):
        assert abs(float(w[str(k)].double().sum()) - float(s)) <= 1e-9 * max(1.0, abs(float(s))), k
    return {str(k): w[str(k)] for k in fx["small_keys"]}


def random_weights(specs, seed=0):
    """Random weights for any configuration (conv N(0, 1/fan_in), GroupNorm 1 + 0.1 N, biases 0.1 N), fp32 CPU."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, shp in specs.items():
        r = torch.randn(shp, generator=g)
        out[k] = r / float(np.prod(shp[1:])) ** 0.5 if k.endswith(".weight") and len(shp) == 4 else (1 + 0.1 * r if k.endswith(".weight") else 0.1 * r)
    return out


def images_to_input(u8, flip=None):
    """ToTensor + Normalize(0.5, 0.5) of uint8 HWC images (optionally mirrored), fp32 NCHW."""
    x = torch.as_tensor(u8)
    if flip is not None:
        x = torch.where(torch.as_tensor(flip).bool().view(-1, 1, 1, 1), x.flip(2), x)
    return (x.permute(0, 3, 1, 2).float() / 255.0 - 0.5) / 0.5


def encoder_fp32(w, x, ch_mult, num_res_blocks, attn_names=()):
    """Plain-torch fp32 restatement: the ldm Encoder (model.py:379-492) + quant_conv over canonical weights -> moments [B, 2z, h, w]."""
    def gn(h, n, swish):
        h = F.group_norm(h, 32, w[n + ".weight"], w[n + ".bias"], eps=1e-6)
        return h * torch.sigmoid(h) if swish else h

    def conv(h, n, stride=1, pad=1):
        return F.conv2d(h, w[n + ".weight"], w[n + ".bias"], stride=stride, padding=pad)

    def res(h, n):
        t = conv(gn(h, n + ".norm1", True), n + ".conv1")
        t = conv(gn(t, n + ".norm2", True), n + ".conv2")
        sc = conv(h, n + ".nin_shortcut", pad=0) if n + ".nin_shortcut.weight" in w else h
        return sc + t

    def attn(h, n):
        b, c, hh, ww = h.shape
        t = gn(h, n + ".norm", False)
        q, k, v = (conv(t, n + "." + s, pad=0).reshape(b, c, hh * ww) for s in "qkv")
        a = torch.softmax(torch.bmm(q.permute(0, 2, 1), k) * (int(c) ** -0.5), dim=2)
        o = torch.bmm(v, a.permute(0, 2, 1)).reshape(b, c, hh, ww)
        return h + conv(o, n + ".proj_out", pad=0)

    h = conv(x, "conv_in")
    for lvl in range(len(ch_mult)):
        for ib in range(num_res_blocks):
            h = res(h, f"down.{lvl}.block.{ib}")
            if f"down.{lvl}.attn.{ib}" in attn_names:
                h = attn(h, f"down.{lvl}.attn.{ib}")
        if lvl != len(ch_mult) - 1:
            h = conv(F.pad(h, (0, 1, 0, 1)), f"down.{lvl}.downsample.conv", stride=2, pad=0)
    h = attn(res(h, "mid.block_1"), "mid.attn_1")
    h = res(h, "mid.block_2")
    h = conv(gn(h, "norm_out", True), "conv_out")
    return conv(h, "quant_conv", pad=0)


def attn_names_of(specs):
    return tuple(sorted({k.rsplit(".", 2)[0] for k in specs if k.startswith("down.") and ".attn." in k}))


# ------------------------------------------------------------------------------------------------ tests
def test_plan_matches_the_reference_keys_and_parameter_count(fx):
    from sfron import vae
    specs, _ = vae.encoder_plan(**small_config(fx))
    assert list(specs) == [str(k) for k in fx["small_keys"]]
    assert [",".join(map(str, s)) for s in specs.values()] == [str(s) for s in fx["small_shapes"]]
    v1, _ = vae.encoder_plan()
    n = sum(int(np.prod(s)) for s in v1.values())
    assert n == 34_163_592 + 72                         # the v1 Encoder + quant_conv
    assert sorted(v1) == sorted(str(k) for k in fx["keymap_ldm"])


def test_encoder_flops():
    from sfron import vae
    assert abs(vae.encoder_flops(256, 256) / 1e9 - 272.7) < 0.05
    assert abs(vae.encoder_flops(512, 512) / 1e9 - 1116.7) < 0.1


def test_fp32_restatement_reproduces_the_reference_moments(fx):
    from sfron import vae
    cfg = small_config(fx)
    specs, _ = vae.encoder_plan(**cfg)
    w = small_weights(fx)
    got = encoder_fp32(w, images_to_input(fx["small_images_u8"]), cfg["ch_mult"], cfg["num_res_blocks"], attn_names_of(specs))
    want = torch.from_numpy(fx["small_moments"])
    assert got.shape == want.shape
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-5


def test_posterior_sample_formula(fx):
    """DiagonalGaussianDistribution.sample() for the fixture's eps == the expression of sfron_latent_sample / sfron_vae_moments."""
    m = torch.from_numpy(fx["small_moments"])
    mean, lv = m.chunk(2, dim=1)
    got = mean + torch.exp(0.5 * lv.clamp(-30.0, 20.0)) * torch.from_numpy(fx["small_eps"])
    assert torch.equal(got, torch.from_numpy(fx["small_sample"]))


def _formats(can, fx):
    """The canonical dict in the four supported namings (+ decoder keys that must be ignored)."""
    from sfron import vae
    ldm = {"encoder." + k if not k.startswith("quant_conv.") else k: v for k, v in can.items()}
    ldm["decoder.conv_in.weight"] = torch.zeros(3)
    ldm["post_quant_conv.bias"] = torch.zeros(8)
    compvis = {"state_dict": {"first_stage_model." + k: v for k, v in ldm.items()}, "global_step": 0}
    out = {"ldm": ldm, "compvis": compvis}
    for new in (False, True):
        d = {}
        for k, v in can.items():
            dk = vae._diffusers_name(k, new)
            d[dk] = v[:, :, 0, 0] if ".attn" in k and k.endswith(".weight") and v.dim() == 4 else v   # diffusers attention: Linear
        d["decoder.mid_block.attentions.0.to_q.weight"] = torch.zeros(2, 2)
        out["diffusers_new" if new else "diffusers_old"] = d
    return out


def test_canonical_state_dict_maps_every_format_to_the_same_tensors(fx):
    from sfron import vae
    specs, _ = vae.encoder_plan()
    can = random_weights(specs, seed=3)
    for name, sd in _formats(can, fx).items():
        got = vae.canonical_state_dict(sd, specs)
        assert list(got) == list(specs), name
        for k in specs:
            assert torch.equal(got[k], can[k]), (name, k)
    small = vae.encoder_plan(**small_config(fx))[0]
    can = random_weights(small, seed=4)                    # a configuration with a down-level attention
    for name, sd in _formats(can, fx).items():
        got = vae.canonical_state_dict(sd, small)
        assert all(torch.equal(got[k], can[k]) for k in small), name


def test_canonical_state_dict_refuses_incomplete_and_unknown_sets():
    from sfron import vae
    specs, _ = vae.encoder_plan()
    can = random_weights(specs, seed=5)
    sd = {"encoder." + k if not k.startswith("quant_conv.") else k: v for k, v in can.items()}
    del sd["encoder.mid.attn_1.k.weight"]
    with pytest.raises(KeyError, match="mid.attn_1.k.weight"):
        vae.canonical_state_dict(sd, specs)
    sd2 = {"encoder." + k if not k.startswith("quant_conv.") else k: v for k, v in can.items()}
    sd2["encoder.down.9.block.0.conv1.weight"] = torch.zeros(1)
    with pytest.raises(KeyError, match="down.9.block.0.conv1.weight"):
        vae.canonical_state_dict(sd2, specs)
    with pytest.raises(KeyError):
        vae.canonical_state_dict({"model.diffusion_model.x": torch.zeros(1)}, specs)


def test_diffusers_key_map_agrees_with_the_reference_converter(fx):
    from sfron import vae
    specs, _ = vae.encoder_plan()
    ref = dict(zip((str(k) for k in fx["keymap_ldm"]), (str(k) for k in fx["keymap_diffusers"])))
    assert sorted(ref) == sorted(specs)
    ours = vae.diffusers_key_map(specs)
    assert ours == {k: ref[k] for k in ours}
    # the converter hands the attention q / k / v / proj weights over as Linear [C, C]: canonical_state_dict takes them back
    rank = dict(zip((str(k) for k in fx["keymap_ldm"]), (int(r) for r in fx["keymap_rank"])))
    assert {k for k, r in rank.items() if r == 2} == {k for k in specs if k.startswith("mid.attn_1.") and k.endswith(".weight")
                                                         and not k.startswith("mid.attn_1.norm")}


def test_center_crop_arr_matches_the_reference(fx):
    from PIL import Image
    from sfron import latents
    for i in range(int(fx["crop_count"])):
        got = np.asarray(latents.center_crop_arr(Image.fromarray(fx[f"crop_in_{i}"]), int(fx["crop_size"])))
        assert np.array_equal(got, fx[f"crop_out_{i}"]), i


def test_class_files_follow_imagefolder_order(tmp_path):
    from sfron import latents
    d = tmp_path / "c"
    (d / "sub").mkdir(parents=True)
    for n in ("b.PNG", "a.jpg", "z.txt", "sub/0.png", "c.webp"):
        (d / n).write_bytes(b"")
    got = [os.path.relpath(p, d) for p in latents.class_files(str(d))]
    assert got == ["a.jpg", "b.PNG", "c.webp", os.path.join("sub", "0.png")]


def _header_protos():
    txt = open(os.path.join(ROOT, "include", "sfron.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name in ("sfron_image_u8_to_rows_bf16", "sfron_vae_moments"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, name
        out[name] = [a.strip() for a in m.group(1).split(",")]
    return out


def test_new_prototypes_have_matching_ctypes_declarations():
    import ctypes
    from sfron import _lib
    for name, args in _header_protos().items():
        res, argtypes = _lib._PROTOS[name]
        assert res is ctypes.c_int
        assert len(argtypes) == len(args), name
        for a, t in zip(args, argtypes):
            assert ("*" in a) == (t is ctypes.c_void_p), (name, a, t)
