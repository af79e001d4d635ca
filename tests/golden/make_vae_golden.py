#!/usr/bin/env python3
"""Generate tests/golden/vae_encoder.npz by IMPORTING the reference (build container only; the reference never travels to the GPU box).

Run:  python tests/golden/make_vae_golden.py
Contents (inputs + expected outputs only -- no reference source text):
  small_*    SD/ldm/modules/diffusionmodules/model.py Encoder at a small config (SMALL below: ch 32, ch_mult 1,2,4, one res block,
             attention at 16 px, 64 px input, batch 2) with weights drawn from a seeded CPU generator key by key in sorted order
             (gen_weights: the tests regenerate them; per-key sums pin the draw), uint8 input images, the conv_out output, the
             quant_conv output (= posterior moments) and ldm/modules/distributions DiagonalGaussianDistribution.sample() for the eps
             it drew.
  keymap_*   SD/train-scripts/convertModels.py convert_ldm_vae_checkpoint on the v1 ddconfig: ldm encoder key -> diffusers key (+ the
             diffusers tensor rank: its attention weights become Linear [C, C]).
  crop_*     DiT/forget.py center_crop_arr on generated images (odd sizes, one BOX-halving case, portrait, landscape).
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "vae_encoder.npz")

SMALL = dict(ch=32, out_ch=3, ch_mult=(1, 2, 4), num_res_blocks=1, attn_resolutions=[16], dropout=0.0, in_channels=3, resolution=64,
             z_channels=4, double_z=True)
V1 = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4], num_res_blocks=2,
          attn_resolutions=[], dropout=0.0)
WEIGHT_SEED = 20261016
CROP_SIZE = 64
CROP_SHAPES = [(99, 65), (150, 200), (133, 71), (71, 133), (67, 67)]     # (height, width): odd, BOX path, portrait, landscape, square


def gen_weights(shapes, seed=WEIGHT_SEED):
    """Encoder + quant_conv weights, key by key in sorted order from one CPU generator: conv / linear weights N(0, 1/fan_in),
    GroupNorm weights 1 + 0.1 N, biases 0.1 N (shared with the tests, which regenerate the same tensors)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k in sorted(shapes):
        shp = tuple(shapes[k])
        r = torch.randn(shp, generator=g, dtype=torch.float32)
        if k.endswith(".weight") and len(shp) == 4:
            out[k] = r / float(np.prod(shp[1:])) ** 0.5
        elif k.endswith(".weight"):
            out[k] = 1.0 + 0.1 * r
        else:
            out[k] = 0.1 * r
    return out


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class _Stub(types.ModuleType):
    """Stand-in for a package absent here: every attribute is an empty class (the reference only needs the names at import time)."""
    def __getattr__(self, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return type(n, (), {})


def _stub(*names):
    for n in names:
        sys.modules[n] = _Stub(n)


def import_ref_model():
    sys.path.insert(0, os.path.join(REF, "SD"))
    model = importlib.import_module("ldm.modules.diffusionmodules.model")
    dist = importlib.import_module("ldm.modules.distributions.distributions")
    return model, dist


def gen_small(model, dist, out):
    enc = model.Encoder(**SMALL)
    z2 = 2 * SMALL["z_channels"]
    quant = torch.nn.Conv2d(z2, z2, 1)
    shapes = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    shapes.update({"quant_conv." + k: tuple(v.shape) for k, v in quant.state_dict().items()})
    w = gen_weights(shapes)
    enc.load_state_dict({k: w[k] for k in enc.state_dict()})
    quant.load_state_dict({k: w["quant_conv." + k] for k in quant.state_dict()})
    keys = list(enc.state_dict()) + ["quant_conv." + k for k in quant.state_dict()]
    out["small_keys"] = np.array(keys)
    out["small_shapes"] = np.array([",".join(str(d) for d in shapes[k]) for k in keys])
    out["small_weight_sums"] = np.array([float(w[k].double().sum()) for k in keys])
    rng = np.random.default_rng(5)
    u8 = rng.integers(0, 256, size=(2, 64, 64, 3), dtype=np.uint8)
    out["small_images_u8"] = u8
    x = (torch.from_numpy(u8).permute(0, 3, 1, 2).float() / 255.0 - 0.5) / 0.5        # ToTensor + Normalize(0.5, 0.5)
    with torch.no_grad():
        h = enc(x)
        mom = quant(h)
        post = dist.DiagonalGaussianDistribution(mom)
        torch.manual_seed(123)
        eps = torch.randn(post.mean.shape)
        torch.manual_seed(123)
        smp = post.sample()
    out["small_conv_out"] = h.numpy()
    out["small_moments"] = mom.numpy()
    out["small_eps"] = eps.numpy()
    out["small_sample"] = smp.numpy()
    out["small_config"] = np.array([SMALL["ch"], SMALL["num_res_blocks"], SMALL["z_channels"], SMALL["resolution"]] + list(SMALL["ch_mult"]))
    out["small_attn_resolutions"] = np.array(SMALL["attn_resolutions"])
    print("small config: moments", mom.shape, "|moments| max", float(mom.abs().max()), "logvar range",
          float(mom[:, 4:].min()), float(mom[:, 4:].max()))


def gen_keymap(model, out):
    _stub("omegaconf", "diffusers", "diffusers.pipelines", "diffusers.pipelines.latent_diffusion", "diffusers.pipelines.paint_by_example",
          "diffusers.pipelines.stable_diffusion", "diffusers.pipelines.latent_diffusion.pipeline_latent_diffusion", "transformers")
    conv = _load("ref_convert_models", os.path.join(REF, "SD", "train-scripts", "convertModels.py"))
    with torch.device("meta"):
        enc, dec = model.Encoder(**V1), model.Decoder(**V1)
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
        if src.startswith("encoder.") or src.startswith("quant_conv."):
            ldm.append(src[len("encoder."):] if src.startswith("encoder.") else src)
            dif.append(k)
            rank.append(v.dim())
    out["keymap_ldm"], out["keymap_diffusers"], out["keymap_rank"] = np.array(ldm), np.array(dif), np.array(rank)
    print("key map:", len(ldm), "encoder keys")


def gen_crops(out):
    _stub("torchvision", "torchvision.datasets", "torchvision.datasets.utils", "torchvision.transforms", "torchvision.utils", "diffusers",
          "diffusers.models", "timm", "timm.models", "timm.models.vision_transformer")
    sys.path.insert(0, os.path.join(REF, "DiT"))
    forget = _load("ref_dit_forget", os.path.join(REF, "DiT", "forget.py"))
    from PIL import Image
    rng = np.random.default_rng(11)
    for i, (h, w) in enumerate(CROP_SHAPES):
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 7) % 256], -1)
        img = np.clip(base + rng.integers(-40, 41, size=(h, w, 3)), 0, 255).astype(np.uint8)
        out[f"crop_in_{i}"] = img
        out[f"crop_out_{i}"] = np.asarray(forget.center_crop_arr(Image.fromarray(img), CROP_SIZE))
    out["crop_size"] = np.array(CROP_SIZE)
    out["crop_count"] = np.array(len(CROP_SHAPES))


if __name__ == "__main__":
    torch.set_num_threads(4)
    out = {}
    model, dist = import_ref_model()
    gen_small(model, dist, out)
    gen_keymap(model, out)
    gen_crops(out)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
