"""CPU: the KL-f8 VAE decoder's host side -- structure, weight formats, FLOP count, grid geometry, ctypes prototypes -- against
tests/golden/vae_decoder.npz (made by tests/golden/make_vae_decoder_golden.py from the reference Decoder and convertModels.py).

``decoder_fp32`` here is a plain-torch restatement of post_quant_conv + the ldm Decoder over canonical names; the GPU tests use it as
their fp32 yardstick.  ``save_image_u8`` / ``round_u8`` / ``make_grid_u8_ref`` restate the two byte conversions and the grid layout
as include/sfron.h states them (torchvision make_grid + save_image; diffusers / SD generate-images.py).  torchvision and diffusers are
absent from the reference tree and from this environment: **parity unpinned** at this boundary, as for timm."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_vae_cpu import random_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dfx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "vae_decoder.npz")))


def small_decoder_config(fx):
    c = fx["small_config"]
    return dict(ch=int(c[0]), num_res_blocks=int(c[1]), z_channels=int(c[2]), resolution=int(c[3]), ch_mult=tuple(int(v) for v in c[4:]),
                attn_resolutions=tuple(int(v) for v in fx["small_attn_resolutions"]))


def small_decoder_weights(fx):
    """The fixture's weights, regenerated from its seed (make_vae_golden.gen_weights with make_vae_decoder_golden.DECODER_SEED) and
    checked against the stored per-key sums."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_vae_golden", os.path.join(ROOT, "tests", "golden", "make_vae_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    shapes = {str(k): tuple(int(d) for d in str(s).split(",")) for k, s in zip(fx["small_keys"], fx["small_shapes"])}
    w = mg.gen_weights(shapes, seed=20261017)
    for k, s in zip(fx["small_keys"], fx["small_weight_sums"]):
        assert abs(float(w[str(k)].double().sum()) - float(s)) <= 1e-9 * max(1.0, abs(float(s))), k
    return {str(k): w[str(k)] for k in fx["small_keys"]}


def decoder_attn_names(specs):
    return tuple(sorted({k.rsplit(".", 2)[0] for k in specs if k.startswith("up.") and ".attn." in k}))


def decoder_fp32(w, z, scale, ch_mult, num_res_blocks, attn_names=()):
    """Plain-torch fp32 restatement: AutoencoderKL.decode (autoencoder.py:385-389) = Decoder (model.py:496-626) of
    post_quant_conv(z / scale) over canonical weights -> [B, out_ch, H, W]."""
    def gn(h, n, swish):
        h = F.group_norm(h, 32, w[n + ".weight"], w[n + ".bias"], eps=1e-6)
        return h * torch.sigmoid(h) if swish else h

    def conv(h, n, pad=1):
        return F.conv2d(h, w[n + ".weight"], w[n + ".bias"], padding=pad)

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

    h = conv(z / scale, "post_quant_conv", pad=0)
    h = conv(h, "conv_in")
    h = res(attn(res(h, "mid.block_1"), "mid.attn_1"), "mid.block_2")
    for lvl in reversed(range(len(ch_mult))):
        for ib in range(num_res_blocks + 1):
            h = res(h, f"up.{lvl}.block.{ib}")
            if f"up.{lvl}.attn.{ib}" in attn_names:
                h = attn(h, f"up.{lvl}.attn.{ib}")
        if lvl != 0:
            h = conv(F.interpolate(h, scale_factor=2.0, mode="nearest"), f"up.{lvl}.upsample.conv")
    return conv(gn(h, "norm_out", True), "conv_out")


# ------------------------------------------------------------------------------------------------ byte formulas (unpinned restatements)
def save_image_u8(x, lo=-1.0, hi=1.0):
    """make_grid(normalize=True, value_range=(lo, hi)) + save_image, fp32 step by step: v = (clamp(x, lo, hi) - lo) / (hi - lo);
    u = trunc(clamp(v * 255 + 0.5, 0, 255)) with v * 255 and + 0.5 rounded separately."""
    x = torch.as_tensor(x, dtype=torch.float32)
    v = (x.clamp(lo, hi) - torch.tensor(lo, dtype=torch.float32)) / torch.tensor(hi - lo, dtype=torch.float32)
    t = v * torch.tensor(255.0, dtype=torch.float32)
    t = t + torch.tensor(0.5, dtype=torch.float32)
    return t.clamp(0.0, 255.0).to(torch.uint8)


def round_u8(x):
    """diffusers / SD/eval-scripts/generate-images.py: v = clamp(x / 2 + 0.5, 0, 1); u = round_half_even(v * 255) (numpy round)."""
    x = torch.as_tensor(x, dtype=torch.float32)
    v = (x / torch.tensor(2.0) + torch.tensor(0.5)).clamp(0.0, 1.0)
    return torch.round(v * torch.tensor(255.0, dtype=torch.float32)).to(torch.uint8)


def make_grid_u8_ref(u8, nrow, padding=2):
    """make_grid's layout for uint8 HWC images [B, H, W, 3] whose pad value maps to byte 0: xmaps = min(nrow, B) columns,
    ceil(B / xmaps) rows, cells (H + padding) x (W + padding) behind a padding-pixel outer border; B == 1 gives the bare image."""
    B, H, W, _ = u8.shape
    if B == 1:
        return u8[0].clone()
    xmaps = min(nrow, B)
    ymaps = int(math.ceil(B / xmaps))
    hh, ww = H + padding, W + padding
    out = torch.zeros(ymaps * hh + padding, xmaps * ww + padding, 3, dtype=torch.uint8)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= B:
                break
            out[y * hh + padding: y * hh + padding + H, x * ww + padding: x * ww + padding + W] = u8[k]
            k += 1
    return out


# ------------------------------------------------------------------------------------------------ tests
def test_plan_matches_the_reference_keys_order_and_parameter_count(dfx):
    from sfron import vae
    specs, ops = vae.decoder_plan(**small_decoder_config(dfx))
    assert list(specs) == [str(k) for k in dfx["small_keys"]]
    assert [",".join(map(str, s)) for s in specs.values()] == [str(s) for s in dfx["small_shapes"]]
    v1, ops1 = vae.decoder_plan()
    assert list(v1) == [str(k) for k in dfx["v1_decoder_keys"]]
    assert sum(int(np.prod(s)) for s in v1.values()) == 49_490_179 + 20          # the v1 Decoder + post_quant_conv
    # execution order: the top level first, an Upsample on every level but 0
    assert [o[1] for o in ops1 if o[0] == "up"] == ["up.3.upsample.conv", "up.2.upsample.conv", "up.1.upsample.conv"]
    assert ops1[0] == ("conv_in", 4, 512) and ops1[-1] == ("out", 128)
    assert [o[1] for o in ops if o[0] == "attn"] == ["mid.attn_1", "up.2.attn.0", "up.2.attn.1"]


def test_decoder_flops():
    from sfron import vae
    assert abs(vae.decoder_flops(256, 256) / 1e9 - 622.2) < 0.05
    assert abs(vae.decoder_flops(512, 512) / 1e9 - 2514.5) < 0.1
    assert 2.2 < vae.decoder_flops(256, 256) / vae.encoder_flops(256, 256) < 2.4


def test_fp32_restatement_reproduces_the_reference_decoder(dfx):
    from sfron import vae
    cfg = small_decoder_config(dfx)
    specs, _ = vae.decoder_plan(**cfg)
    w = small_decoder_weights(dfx)
    z = torch.from_numpy(dfx["small_latents"])
    scale = float(dfx["small_scale"])
    pq = F.conv2d(z / scale, w["post_quant_conv.weight"], w["post_quant_conv.bias"])
    want_pq = torch.from_numpy(dfx["small_post_quant"])
    assert float((pq - want_pq).abs().max() / want_pq.abs().max()) <= 1e-6
    got = decoder_fp32(w, z, scale, cfg["ch_mult"], cfg["num_res_blocks"], decoder_attn_names(specs))
    want = torch.from_numpy(dfx["small_decoded"])
    assert got.shape == want.shape == (2, 3, 64, 64)
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-5


def test_diffusers_key_map_agrees_with_the_reference_converter(dfx):
    from sfron import vae
    specs, _ = vae.decoder_plan()
    ref = dict(zip((str(k) for k in dfx["keymap_ldm"]), (str(k) for k in dfx["keymap_diffusers"])))
    assert sorted(ref) == sorted(specs)
    assert vae.diffusers_decoder_key_map(specs) == {k: ref[k] for k in specs}
    # the other attention naming differs only in the attention projection names
    new = vae.diffusers_decoder_key_map(specs, new_attn=True)
    ren = {".query.": ".to_q.", ".key.": ".to_k.", ".value.": ".to_v.", ".proj_attn.": ".to_out.0."}
    for k in specs:
        want = ref[k]
        for a, b in ren.items():
            want = want.replace(a, b)
        assert new[k] == want, k
    rank = dict(zip((str(k) for k in dfx["keymap_ldm"]), (int(r) for r in dfx["keymap_rank"])))
    assert {k for k, r in rank.items() if r == 2} == {k for k in specs if k.startswith("mid.attn_1.") and k.endswith(".weight")
                                                         and not k.startswith("mid.attn_1.norm")}


def decoder_formats(can, with_encoder=None):
    """The canonical decoder dict in the four supported namings (+ encoder keys that must be ignored)."""
    from sfron import vae
    levels = 1 + max(int(k.split(".")[1]) for k in can if k.startswith("up."))
    ldm = {"decoder." + k if not k.startswith("post_quant_conv.") else k: v for k, v in can.items()}
    ldm["encoder.conv_in.weight"] = torch.zeros(3)
    ldm["quant_conv.bias"] = torch.zeros(8)
    compvis = {"state_dict": {"first_stage_model." + k: v for k, v in ldm.items()}, "global_step": 0}
    out = {"ldm": ldm, "compvis": compvis}
    for new in (False, True):
        d = {}
        for k, v in can.items():
            dk = vae._diffusers_decoder_name(k, levels, new)
            d[dk] = v[:, :, 0, 0] if ".attn" in k and k.endswith(".weight") and v.dim() == 4 else v   # diffusers attention: Linear
        d["encoder.mid_block.attentions.0.to_q.weight"] = torch.zeros(2, 2)
        out["diffusers_new" if new else "diffusers_old"] = d
    return out


def test_canonical_decoder_state_dict_maps_every_format_to_the_same_tensors(dfx):
    from sfron import vae
    for specs, seed in ((vae.decoder_plan()[0], 3), (vae.decoder_plan(**small_decoder_config(dfx))[0], 4)):
        can = random_weights(specs, seed=seed)
        for name, sd in decoder_formats(can).items():
            got = vae.canonical_decoder_state_dict(sd, specs)
            assert list(got) == list(specs), name
            for k in specs:
                assert torch.equal(got[k], can[k]), (name, k)


def test_canonical_decoder_state_dict_refuses_incomplete_and_unknown_sets():
    from sfron import vae
    specs, _ = vae.decoder_plan()
    can = random_weights(specs, seed=5)
    sd = {"decoder." + k if not k.startswith("post_quant_conv.") else k: v for k, v in can.items()}
    del sd["decoder.up.2.upsample.conv.weight"]
    with pytest.raises(KeyError, match="up.2.upsample.conv.weight"):
        vae.canonical_decoder_state_dict(sd, specs)
    sd2 = {"decoder." + k if not k.startswith("post_quant_conv.") else k: v for k, v in can.items()}
    sd2["decoder.up.9.block.0.conv1.weight"] = torch.zeros(1)
    with pytest.raises(KeyError, match="up.9.block.0.conv1.weight"):
        vae.canonical_decoder_state_dict(sd2, specs)
    dif = decoder_formats(can)["diffusers_old"]
    dif["decoder.up_blocks.0.strange.0.weight"] = torch.zeros(1)
    with pytest.raises(KeyError, match="up_blocks.0.strange"):
        vae.canonical_decoder_state_dict(dif, specs)
    sd3 = dict(sd2)
    del sd3["decoder.up.9.block.0.conv1.weight"]
    sd3["decoder.conv_out.weight"] = torch.zeros(3, 128, 1, 1)
    with pytest.raises(ValueError, match="conv_out.weight"):
        vae.canonical_decoder_state_dict(sd3, specs)
    with pytest.raises(KeyError):
        vae.canonical_decoder_state_dict({"model.diffusion_model.x": torch.zeros(1)}, specs)


def _full_autoencoder_formats(ecan, dcan):
    """One full AutoencoderKL state (encoder + quant_conv + decoder + post_quant_conv) in the four supported namings."""
    from sfron import vae
    levels = 1 + max(int(k.split(".")[1]) for k in dcan if k.startswith("up."))
    ldm = {("encoder." + k if not k.startswith("quant_conv.") else k): v for k, v in ecan.items()}
    ldm.update({("decoder." + k if not k.startswith("post_quant_conv.") else k): v for k, v in dcan.items()})
    out = {"ldm": ldm, "compvis": {"state_dict": {"first_stage_model." + k: v for k, v in ldm.items()}}}
    lin = lambda k, v: v[:, :, 0, 0] if ".attn" in k and k.endswith(".weight") and v.dim() == 4 else v
    for new in (False, True):
        d = {vae._diffusers_name(k, new): lin(k, v) for k, v in ecan.items()}
        d.update({vae._diffusers_decoder_name(k, levels, new): lin(k, v) for k, v in dcan.items()})
        out["diffusers_new" if new else "diffusers_old"] = d
    return out


def test_encoder_and_decoder_halves_of_one_autoencoder_dict():
    """One full AutoencoderKL dict feeds both canonicalisers; each takes its own half and ignores the other."""
    from sfron import vae
    especs, _ = vae.encoder_plan()
    dspecs, _ = vae.decoder_plan()
    ecan, dcan = random_weights(especs, seed=6), random_weights(dspecs, seed=7)
    for name, full in _full_autoencoder_formats(ecan, dcan).items():
        e = vae.canonical_state_dict(full, especs)
        d = vae.canonical_decoder_state_dict(full, dspecs)
        assert all(torch.equal(e[k], ecan[k]) for k in especs), name
        assert all(torch.equal(d[k], dcan[k]) for k in dspecs), name


def test_load_autoencoder_reads_one_file_for_both_halves(tmp_path, monkeypatch):
    """vae.load_autoencoder: the file is read once and both halves are built from that one state (constructors stubbed: no GPU)."""
    from sfron import vae
    especs, _ = vae.encoder_plan()
    dspecs, _ = vae.decoder_plan()
    ecan, dcan = random_weights(especs, seed=8), random_weights(dspecs, seed=9)
    path = tmp_path / "vae.ckpt"
    torch.save(_full_autoencoder_formats(ecan, dcan)["compvis"], str(path))
    reads = []
    real = vae.load_state_file
    monkeypatch.setattr(vae, "load_state_file", lambda p: reads.append(p) or real(p))
    monkeypatch.setattr(vae.VAEEncoder, "from_state_dict", classmethod(lambda cls, sd, **kw: ("enc", sd, kw)))
    monkeypatch.setattr(vae.VAEDecoder, "from_state_dict", classmethod(lambda cls, sd, **kw: ("dec", sd, kw)))
    enc, dec = vae.load_autoencoder(str(path), ch=128, out_ch=3, in_channels=3)
    assert reads == [str(path)] and enc[0] == "enc" and dec[0] == "dec" and enc[1] is dec[1]
    assert enc[2] == dict(ch=128, in_channels=3) and dec[2] == dict(ch=128, out_ch=3)
    d = vae.canonical_decoder_state_dict(dec[1], dspecs)
    e = vae.canonical_state_dict(enc[1], especs)
    assert all(torch.equal(d[k], dcan[k]) for k in dspecs) and all(torch.equal(e[k], ecan[k]) for k in especs)


@pytest.mark.parametrize("n,nrow", [(1, 5), (2, 5), (5, 5), (7, 3), (10, 5), (10, 4), (3, 8)])
def test_grid_geometry_follows_make_grid(n, nrow):
    from sfron import images
    H, W, p = 5, 7, 2
    u8 = torch.arange(n * H * W * 3, dtype=torch.int64).remainder(251).add(1).to(torch.uint8).view(n, H, W, 3)
    g = make_grid_u8_ref(u8, nrow, p)
    Hc, Wc, xmaps, ymaps = images.grid_geometry(n, H, W, nrow, p)
    assert (Hc, Wc) == tuple(g.shape[:2])
    if n == 1:
        assert torch.equal(g, u8[0])
        return
    assert xmaps == min(nrow, n) and ymaps == -(-n // xmaps)
    assert int((g == 0).all(-1).sum()) == Hc * Wc - n * H * W        # every pad pixel and empty cell is byte 0, no image pixel is
    # the last row is partial when xmaps does not divide n: its empty cells are pad
    if n % xmaps:
        y0 = (ymaps - 1) * (H + p) + p
        x0 = (n % xmaps) * (W + p) + p
        assert int(g[y0:y0 + H, x0:].sum()) == 0


def test_byte_formulas_on_chosen_values():
    x = torch.tensor([-3.0, -1.0, -0.999, 0.0, 0.5, 1.0, 1.0001, 7.0, 0.00196, -0.00196])
    s = save_image_u8(x)
    r = round_u8(x)
    assert s.tolist()[:2] == [0, 0] and s.tolist()[5:8] == [255, 255, 255] and s[3] == 128
    assert r.tolist()[:2] == [0, 0] and r.tolist()[5:8] == [255, 255, 255] and r[3] == 128          # 127.5 rounds to even
    # + 0.5 then truncation is round-half-up of v * 255, not numpy's half-to-even
    v = torch.tensor([0.5, 0.0], dtype=torch.float32) * 2 - 1
    assert save_image_u8(v).tolist() == [128, 0] and round_u8(v).tolist() == [128, 0]


def _header_protos():
    txt = open(os.path.join(ROOT, "include", "sfron.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name in ("sfron_vae_latent_in", "sfron_rows_to_image_u8"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, name
        out[name] = [a.strip() for a in m.group(1).split(",")]
    return out


def test_new_prototypes_have_matching_ctypes_declarations():
    import ctypes
    from sfron import _lib, images
    for name, args in _header_protos().items():
        res, argtypes = _lib._PROTOS[name]
        assert res is ctypes.c_int
        assert len(argtypes) == len(args), name
        for a, t in zip(args, argtypes):
            assert ("*" in a) == (t is ctypes.c_void_p), (name, a, t)
            if "*" not in a:
                want = {"int": ctypes.c_int, "float": ctypes.c_float}[a.split()[0]]
                assert t is want, (name, a, t)
    hdr = open(os.path.join(ROOT, "include", "sfron.h")).read()
    m = re.search(r"enum \{ SFRON_IMAGE_SAVE_IMAGE = (\d+), SFRON_IMAGE_ROUND = (\d+) \};", hdr)
    assert m and images._MODES == {"save_image": int(m.group(1)), "round": int(m.group(2))}


def test_latent_diffusion_decode_first_stage_without_a_decoder_still_refuses():
    from sfron import sd

    class _U:
        device_ = torch.device("cpu")

    ld = sd.LatentDiffusion.__new__(sd.LatentDiffusion)
    ld.first_stage_decoder = None
    with pytest.raises(NotImplementedError):
        ld.decode_first_stage(torch.zeros(1, 4, 2, 2))
    with pytest.raises(NotImplementedError):
        ld.get_input({}, "jpg")

    class _Dec:
        def decode(self, z, scale):
            return ("decoded", z, scale)

    ld.first_stage_decoder = _Dec()
    z = torch.ones(1, 4, 2, 2)
    out = ld.decode_first_stage(z)
    assert out[0] == "decoded" and out[1] is z and out[2] == 0.18215
