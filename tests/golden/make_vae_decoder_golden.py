#!/usr/bin/env python3
"""Generate tests/golden/vae_decoder.npz by IMPORTING the reference (build container only; the reference never travels to the GPU box).

Run:  python tests/golden/make_vae_decoder_golden.py
Contents (inputs + expected outputs only -- no reference source text):
  small_*    SD/ldm/modules/diffusionmodules/model.py Decoder at a small config (SMALL below: ch 32, ch_mult 1,2,4, one res block,
             attention at 16 px, z 4, 16 x 16 latents -> 64 px, batch 2) with AutoencoderKL's post_quant_conv in front
             (SD/ldm/models/autoencoder.py:385-389: decode(z) = decoder(post_quant_conv(z))).  Weights are drawn from a seeded CPU
             generator key by key in sorted order (make_vae_golden.gen_weights, DECODER_SEED: the tests regenerate them; per-key sums
             pin the draw).  Stored: the latents, post_quant_conv(latents / SCALE) and the decoder output.
  keymap_*   SD/train-scripts/convertModels.py convert_ldm_vae_checkpoint on the v1 ddconfig: ldm decoder key -> diffusers key (+ the
             diffusers tensor rank: its attention weights become Linear [C, C]).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_vae_golden as mg  # noqa: E402

OUT = os.path.join(HERE, "vae_decoder.npz")
SMALL = dict(ch=32, out_ch=3, ch_mult=(1, 2, 4), num_res_blocks=1, attn_resolutions=[16], dropout=0.0, in_channels=3, resolution=64,
             z_channels=4, double_z=True)
DECODER_SEED = 20261017
SCALE = 0.18215


def gen_small(model, out):
    dec = model.Decoder(**SMALL)
    zc = SMALL["z_channels"]
    pq = torch.nn.Conv2d(zc, zc, 1)
    shapes = {k: tuple(v.shape) for k, v in dec.state_dict().items()}
    shapes.update({"post_quant_conv." + k: tuple(v.shape) for k, v in pq.state_dict().items()})
    w = mg.gen_weights(shapes, seed=DECODER_SEED)
    dec.load_state_dict({k: w[k] for k in dec.state_dict()})
    pq.load_state_dict({k: w["post_quant_conv." + k] for k in pq.state_dict()})
    keys = list(dec.state_dict()) + ["post_quant_conv." + k for k in pq.state_dict()]
    assert keys == [n for n, _ in dec.named_parameters()] + ["post_quant_conv.weight", "post_quant_conv.bias"]
    out["small_keys"] = np.array(keys)
    out["small_shapes"] = np.array([",".join(str(d) for d in shapes[k]) for k in keys])
    out["small_weight_sums"] = np.array([float(w[k].double().sum()) for k in keys])
    g = torch.Generator().manual_seed(8)
    z = torch.randn(2, zc, 16, 16, generator=g) * 0.8          # about the scale of DiT latents (0.18215 * posterior samples)
    with torch.no_grad():
        y = pq(z / SCALE)
        img = dec(y)
    out["small_latents"] = z.numpy()
    out["small_post_quant"] = y.numpy()
    out["small_decoded"] = img.numpy()
    out["small_scale"] = np.array(SCALE, dtype=np.float32)
    out["small_config"] = np.array([SMALL["ch"], SMALL["num_res_blocks"], SMALL["z_channels"], SMALL["resolution"]] + list(SMALL["ch_mult"]))
    out["small_attn_resolutions"] = np.array(SMALL["attn_resolutions"])
    print("small config: decoded", tuple(img.shape), "range", float(img.min()), float(img.max()), "std", float(img.std()))


def gen_keymap(model, out):
    mg._stub("omegaconf", "diffusers", "diffusers.pipelines", "diffusers.pipelines.latent_diffusion", "diffusers.pipelines.paint_by_example",
             "diffusers.pipelines.stable_diffusion", "diffusers.pipelines.latent_diffusion.pipeline_latent_diffusion", "transformers")
    conv = mg._load("ref_convert_models", os.path.join(mg.REF, "SD", "train-scripts", "convertModels.py"))
    with torch.device("meta"):
        enc, dec = model.Encoder(**mg.V1), model.Decoder(**mg.V1)
    ckpt, names = {}, []

    # each tensor is one element per dimension holding its own index: the converter's renames and rank changes are what is recorded
    def add(prefix, sd):
        for k, v in sd.items():
            ckpt["first_stage_model." + prefix + k] = torch.full((1,) * v.dim(), float(len(names)))
            names.append(prefix + k)
    add("encoder.", enc.state_dict())
    add("decoder.", dec.state_dict())
    for k, shp in (("quant_conv.weight", (1, 1, 1, 1)), ("quant_conv.bias", (1,)), ("post_quant_conv.weight", (1, 1, 1, 1)),
                   ("post_quant_conv.bias", (1,))):
        ckpt["first_stage_model." + k] = torch.full(shp, float(len(names)))
        names.append(k)
    new = conv.convert_ldm_vae_checkpoint(ckpt, {})
    ldm, dif, rank = [], [], []
    for k, v in new.items():
        src = names[int(v.reshape(-1)[0])]
        if src.startswith("decoder.") or src.startswith("post_quant_conv."):
            ldm.append(src[len("decoder."):] if src.startswith("decoder.") else src)
            dif.append(k)
            rank.append(v.dim())
    out["keymap_ldm"], out["keymap_diffusers"], out["keymap_rank"] = np.array(ldm), np.array(dif), np.array(rank)
    out["v1_decoder_keys"] = np.array(list(dec.state_dict()) + ["post_quant_conv.weight", "post_quant_conv.bias"])
    print("key map:", len(ldm), "decoder keys")


if __name__ == "__main__":
    torch.set_num_threads(4)
    out = {}
    model, _ = mg.import_ref_model()
    gen_small(model, out)
    gen_keymap(model, out)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
