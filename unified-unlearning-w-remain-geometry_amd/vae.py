"""The KL-f8 VAE encoder (image -> posterior moments -> latent) over the HIP kernels of csrc/conv.hip / groupnorm.hip / rows.hip / embed.hip, forward only.

Restates SD/ldm/modules/diffusionmodules/model.py ``Encoder`` (conv_in, per level ``num_res_blocks`` ResnetBlocks [+ AttnBlocks] and a
(0,1,0,1)-padded stride-2 Downsample, mid ResnetBlock / AttnBlock / ResnetBlock, GroupNorm + swish + conv_out) followed by the
``quant_conv`` of ``AutoencoderKL`` and ``DiagonalGaussianDistribution.sample() * 0.18215`` -- what DiT/forget.py:265-267,305-307
(``vae.encode(x).latent_dist.sample().mul_(0.18215)``) and SD/train-scripts/nsfw_removal.py (``encode_first_stage``) run inside the
step.  No tape, no autograd: activations are NHWC fp32 rows between blocks and bf16 where they feed a product, in a few ping-pong
workspaces reused across calls, on the current stream.

The decoder (``VAEDecoder``) is the other direction on the same blocks: ``post_quant_conv(z / scale)`` (one launch of
sfron_vae_latent_in), the ldm ``Decoder`` (conv_in, mid ResnetBlock / AttnBlock / ResnetBlock, per level from the top down
``num_res_blocks + 1`` ResnetBlocks [+ AttnBlocks] and a nearest x2 Upsample + 3x3 conv on every level but 0, GroupNorm + swish +
conv_out), then fp32 NCHW images or the uint8 bytes of save_image / diffusers (sfron_rows_to_image_u8, optionally as the make_grid canvas)
-- what DiT/forget.py:114-145 and SD/eval-scripts/generate-images.py:181-192 run through ``vae.decode``.

Chunk invariant: the products take their operands through buffer resources sized by a 32-bit byte count (k_cgemm, conv.hip) and an
``int`` row count, so the library REFUSES an operand of 2 GiB or more (sfron_conv_fwd, sfron_conv_wgrad, sfron_bgemm_bf16, sfron_gemm_bf16
and the GroupNorm launchers return SFRON_ERR_ARG before any launch; DESIGN.md section 7 lists every entry point and its verdict).  A batch is
therefore run in chunks of samples whose largest operand stays under ``max_chunk_bytes`` (default 1 GiB: 32 images at 256 px, 8 at 512 px
for the encoder; 16 and 4 for the decoder, whose largest operand is the 256-channel level after the last upsample), and every launch
asserts its operands are below 2 GiB, so the caller sees which tensor is too large rather than a status code.
"""
import ctypes
import json
import os
from collections import OrderedDict

import numpy as np
import torch

from ._lib import check, lib as _L, ptr, stream_ptr
from .forward_net import ForwardNet, guard
from .unet import _conv_desc, _pad8, bgemm

GN_EPS = 1e-6


# ------------------------------------------------------------------------------------------------ structure and weight formats
# Parameter specs of the blocks both plans are made of, appended to ``dst`` in the modules' registration order; ``res`` also notes its op.
def _conv_spec(dst, name, o, i, k):
    dst.extend([(name + ".weight", (o, i, k, k)), (name + ".bias", (o,))])


def _gn_spec(dst, name, c):
    dst.extend([(name + ".weight", (c,)), (name + ".bias", (c,))])


def _res_spec(dst, ops, name, cin, cout):
    _gn_spec(dst, name + ".norm1", cin)
    _conv_spec(dst, name + ".conv1", cout, cin, 3)
    _gn_spec(dst, name + ".norm2", cout)
    _conv_spec(dst, name + ".conv2", cout, cout, 3)
    if cin != cout:
        _conv_spec(dst, name + ".nin_shortcut", cout, cin, 1)
    ops.append(("res", name, cin, cout))


def _attn_spec(dst, name, c):
    _gn_spec(dst, name + ".norm", c)
    for w in ("q", "k", "v", "proj_out"):
        _conv_spec(dst, name + "." + w, c, c, 1)


def encoder_plan(ch=128, ch_mult=(1, 2, 4, 4), num_res_blocks=2, z_channels=4, in_channels=3, attn_resolutions=(), resolution=256):
    """(parameter specs in Encoder.named_parameters() order + quant_conv, op list) of the reference Encoder's construction
    (model.py:379-466).  Ops: ("conv_in",), ("res", name, cin, cout), ("attn", name, c), ("down", name, c), ("out", c)."""
    P, ops = [], []
    _conv_spec(P, "conv_in", ch, in_channels, 3)
    ops.append(("conv_in",))
    cur, in_mult, block_in = resolution, (1,) + tuple(ch_mult), ch
    for lvl in range(len(ch_mult)):
        block_in, block_out = ch * in_mult[lvl], ch * ch_mult[lvl]
        attns = []
        for ib in range(num_res_blocks):
            _res_spec(P, ops, f"down.{lvl}.block.{ib}", block_in, block_out)
            block_in = block_out
            if cur in attn_resolutions:
                attns.append(f"down.{lvl}.attn.{ib}")
                ops.append(("attn", attns[-1], block_in))
        for a in attns:                              # the attn ModuleList is registered after the block ModuleList
            _attn_spec(P, a, block_in)
        if lvl != len(ch_mult) - 1:
            _conv_spec(P, f"down.{lvl}.downsample.conv", block_in, block_in, 3)
            ops.append(("down", f"down.{lvl}.downsample.conv", block_in))
            cur //= 2
    # the ModuleList ops above interleave blocks and attentions in execution order; parameters follow registration order
    _res_spec(P, ops, "mid.block_1", block_in, block_in)
    _attn_spec(P, "mid.attn_1", block_in)
    ops.append(("attn", "mid.attn_1", block_in))
    _res_spec(P, ops, "mid.block_2", block_in, block_in)
    _gn_spec(P, "norm_out", block_in)
    _conv_spec(P, "conv_out", 2 * z_channels, block_in, 3)
    ops.append(("out", block_in))
    _conv_spec(P, "quant_conv", 2 * z_channels, 2 * z_channels, 1)
    return OrderedDict(P), ops


_ATTN_DIFFUSERS = {"norm": "group_norm", "q": "query", "k": "key", "v": "value", "proj_out": "proj_attn"}
_ATTN_DIFFUSERS_NEW = {"norm": "group_norm", "q": "to_q", "k": "to_k", "v": "to_v", "proj_out": "to_out.0"}


def _diffusers_name(name, new_attn):
    """ldm Encoder name (no prefix) -> diffusers AutoencoderKL name (with its encoder. prefix)."""
    if name.startswith("quant_conv."):
        return name
    parts = name.split(".")
    if parts[0] == "norm_out":
        return "encoder.conv_norm_out." + parts[1]
    if parts[0] in ("conv_in", "conv_out"):
        return "encoder." + name
    if parts[0] == "down":
        lvl, kind = parts[1], parts[2]
        if kind == "block":
            sub = parts[4].replace("nin_shortcut", "conv_shortcut")
            return f"encoder.down_blocks.{lvl}.resnets.{parts[3]}.{sub}.{parts[5]}"
        if kind == "downsample":
            return f"encoder.down_blocks.{lvl}.downsamplers.0.conv.{parts[4]}"
        if kind == "attn":
            m = _ATTN_DIFFUSERS_NEW if new_attn else _ATTN_DIFFUSERS
            return f"encoder.down_blocks.{lvl}.attentions.{parts[3]}.{m[parts[4]]}.{parts[5]}"
    if parts[0] == "mid":
        if parts[1].startswith("block_"):
            sub = parts[2].replace("nin_shortcut", "conv_shortcut")
            return f"encoder.mid_block.resnets.{int(parts[1][6:]) - 1}.{sub}.{parts[3]}"
        if parts[1] == "attn_1":
            m = _ATTN_DIFFUSERS_NEW if new_attn else _ATTN_DIFFUSERS
            return f"encoder.mid_block.attentions.0.{m[parts[2]]}.{parts[3]}"
    raise KeyError(name)


def diffusers_key_map(specs, new_attn=False):
    """{ldm name: diffusers name} for every canonical key (what SD/train-scripts/convertModels.py:594 convert_ldm_vae_checkpoint does
    to the encoder half of a CompVis VAE)."""
    return OrderedDict((n, _diffusers_name(n, new_attn)) for n in specs)


_ATTN_LDM = {v: k for m in (_ATTN_DIFFUSERS, _ATTN_DIFFUSERS_NEW) for k, v in m.items()}


def _ldm_name(key):
    """diffusers AutoencoderKL name -> ldm Encoder name (None for keys outside the encoder: decoder, post_quant_conv)."""
    if key.startswith("quant_conv."):
        return key
    if not key.startswith("encoder."):
        return None
    p = key[len("encoder."):].split(".")
    if p[0] == "conv_norm_out":
        return "norm_out." + p[1]
    if p[0] in ("conv_in", "conv_out"):
        return ".".join(p)
    if p[0] == "down_blocks" and p[2] == "resnets":
        return f"down.{p[1]}.block.{p[3]}.{p[4].replace('conv_shortcut', 'nin_shortcut')}.{p[5]}"
    if p[0] == "down_blocks" and p[2] == "downsamplers":
        return f"down.{p[1]}.downsample.conv.{p[5]}"
    if p[0] == "down_blocks" and p[2] == "attentions":
        return f"down.{p[1]}.attn.{p[3]}.{_ATTN_LDM['.'.join(p[4:-1])]}.{p[-1]}"
    if p[0] == "mid_block" and p[1] == "resnets":
        return f"mid.block_{int(p[2]) + 1}.{p[3].replace('conv_shortcut', 'nin_shortcut')}.{p[4]}"
    if p[0] == "mid_block" and p[1] == "attentions":
        return f"mid.attn_1.{_ATTN_LDM['.'.join(p[3:-1])]}.{p[-1]}"
    raise KeyError(f"unknown diffusers VAE encoder key {key!r}")


def _canonical(sd, specs, side, conv, blocks, mapper):
    """What canonical_state_dict / canonical_decoder_state_dict do.  side: "encoder" | "decoder", the key prefix and the word in the
    messages; conv: the AutoencoderKL convolution kept with it; blocks: the diffusers block list that tells diffusers keys apart;
    mapper(sd) -> the function diffusers key -> ldm name (None: not this side's)."""
    if "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    if any(k.startswith("first_stage_model.") for k in sd):
        sd = {k[len("first_stage_model."):]: v for k, v in sd.items() if k.startswith("first_stage_model.")}
    pre = side + "."
    if any(k.startswith((pre + blocks, pre + "mid_block.", pre + "conv_norm_out.")) for k in sd):
        name = mapper(sd)
    else:
        name = lambda k: k[len(pre):] if k.startswith(pre) else (k if k.startswith(conv + ".") else None)
    out = OrderedDict()
    for k, v in sd.items():
        n = name(k)
        if n is None:
            continue
        t = torch.as_tensor(v).detach().to("cpu", torch.float32)
        if t.dim() == 2 and ".attn" in n and n.endswith(".weight"):          # diffusers Linear -> 1x1 conv
            t = t.reshape(t.shape[0], t.shape[1], 1, 1)
        out[n] = t
    if not out:
        raise KeyError(f"not a VAE state dict: no {side}.* / {conv}.* / first_stage_model.* keys (first keys: {list(sd)[:5]})")
    if specs is not None:
        missing = [n for n in specs if n not in out]
        extra = [n for n in out if n not in specs]
        if missing or extra:
            raise KeyError(f"VAE {side} state dict does not match the configuration: missing {missing[:8]}"
                           f"{' ...' if len(missing) > 8 else ''}, unexpected {extra[:8]}")
        for n, shp in specs.items():
            if tuple(out[n].shape) != tuple(shp):
                raise ValueError(f"{n}: shape {tuple(out[n].shape)}, the configuration needs {tuple(shp)}")
        out = OrderedDict((n, out[n]) for n in specs)
    return out


def canonical_state_dict(sd, specs=None):
    """Any supported VAE state dict -> {ldm Encoder name (no prefix) | quant_conv.*: fp32 CPU tensor}, shaped as the ldm modules.
    Formats: ldm AutoencoderKL (encoder.* + quant_conv.*), a CompVis LDM checkpoint (first_stage_model.*, optionally under
    "state_dict"), diffusers AutoencoderKL (query/key/value/proj_attn or to_q/to_k/to_v/to_out.0 attention names; its Linear [C, C]
    attention weights become 1x1 convolutions).  Decoder keys are ignored.  ``specs`` (encoder_plan's) checks names and shapes: an
    incomplete or unknown key set raises and names the keys."""
    return _canonical(sd, specs, "encoder", "quant_conv", "down_blocks.", lambda sd: _ldm_name)


def decoder_plan(ch=128, ch_mult=(1, 2, 4, 4), num_res_blocks=2, z_channels=4, out_ch=3, attn_resolutions=(), resolution=256):
    """(parameter specs in Decoder.named_parameters() order + post_quant_conv, op list in execution order) of the reference Decoder
    (model.py:496-626) and AutoencoderKL's post_quant_conv (autoencoder.py:385-389).  The up levels run from the top down but are
    registered from level 0 up (``self.up.insert(0, up)``).  Ops: ("conv_in", zc, c), ("res", name, cin, cout), ("attn", name, c),
    ("up", name, c) (nearest x2 + 3x3 conv, model.py:44-57), ("out", c)."""
    P, ops = [], []
    nl = len(ch_mult)
    block_in = ch * ch_mult[nl - 1]
    cur = resolution // 2 ** (nl - 1)
    _conv_spec(P, "conv_in", block_in, z_channels, 3)
    ops.append(("conv_in", z_channels, block_in))
    _res_spec(P, ops, "mid.block_1", block_in, block_in)
    _attn_spec(P, "mid.attn_1", block_in)
    ops.append(("attn", "mid.attn_1", block_in))
    _res_spec(P, ops, "mid.block_2", block_in, block_in)
    levels = {}
    for lvl in reversed(range(nl)):
        L, attns = [], []
        block_out = ch * ch_mult[lvl]
        for ib in range(num_res_blocks + 1):
            _res_spec(L, ops, f"up.{lvl}.block.{ib}", block_in, block_out)
            block_in = block_out
            if cur in attn_resolutions:
                attns.append(f"up.{lvl}.attn.{ib}")
                ops.append(("attn", attns[-1], block_in))
        for a in attns:                              # the attn ModuleList is registered after the block ModuleList
            _attn_spec(L, a, block_in)
        if lvl != 0:
            _conv_spec(L, f"up.{lvl}.upsample.conv", block_in, block_in, 3)
            ops.append(("up", f"up.{lvl}.upsample.conv", block_in))
            cur *= 2
        levels[lvl] = L
    for lvl in range(nl):                            # registration order: up.0 first
        P.extend(levels[lvl])
    _gn_spec(P, "norm_out", block_in)
    _conv_spec(P, "conv_out", out_ch, block_in, 3)
    ops.append(("out", block_in))
    _conv_spec(P, "post_quant_conv", z_channels, z_channels, 1)
    return OrderedDict(P), ops


def _levels(specs):
    return 1 + max(int(n.split(".")[1]) for n in specs if n.startswith("up."))


def _diffusers_decoder_name(name, levels, new_attn):
    """ldm Decoder name (no prefix) -> diffusers AutoencoderKL name (decoder. prefix); diffusers numbers the up blocks from the top:
    up_blocks.j is ldm up.{levels-1-j}."""
    if name.startswith("post_quant_conv."):
        return name
    parts = name.split(".")
    if parts[0] == "norm_out":
        return "decoder.conv_norm_out." + parts[1]
    if parts[0] in ("conv_in", "conv_out"):
        return "decoder." + name
    if parts[0] == "up":
        j, kind = levels - 1 - int(parts[1]), parts[2]
        if kind == "block":
            sub = parts[4].replace("nin_shortcut", "conv_shortcut")
            return f"decoder.up_blocks.{j}.resnets.{parts[3]}.{sub}.{parts[5]}"
        if kind == "upsample":
            return f"decoder.up_blocks.{j}.upsamplers.0.conv.{parts[4]}"
        if kind == "attn":
            m = _ATTN_DIFFUSERS_NEW if new_attn else _ATTN_DIFFUSERS
            return f"decoder.up_blocks.{j}.attentions.{parts[3]}.{m[parts[4]]}.{parts[5]}"
    if parts[0] == "mid":
        return "decoder." + _diffusers_name(name, new_attn)[len("encoder."):]
    raise KeyError(name)


def diffusers_decoder_key_map(specs, new_attn=False):
    """{ldm name: diffusers name} for every canonical decoder key (the decoder half of convertModels.py:594
    convert_ldm_vae_checkpoint)."""
    nl = _levels(specs)
    return OrderedDict((n, _diffusers_decoder_name(n, nl, new_attn)) for n in specs)


def _ldm_decoder_name(key, levels):
    """diffusers AutoencoderKL name -> ldm Decoder name (None for keys outside the decoder: encoder, quant_conv)."""
    if key.startswith("post_quant_conv."):
        return key
    if not key.startswith("decoder."):
        return None
    p = key[len("decoder."):].split(".")
    if p[0] == "conv_norm_out":
        return "norm_out." + p[1]
    if p[0] in ("conv_in", "conv_out"):
        return ".".join(p)
    if p[0] == "up_blocks":
        lvl = levels - 1 - int(p[1])
        if p[2] == "resnets":
            return f"up.{lvl}.block.{p[3]}.{p[4].replace('conv_shortcut', 'nin_shortcut')}.{p[5]}"
        if p[2] == "upsamplers":
            return f"up.{lvl}.upsample.conv.{p[5]}"
        if p[2] == "attentions":
            return f"up.{lvl}.attn.{p[3]}.{_ATTN_LDM['.'.join(p[4:-1])]}.{p[-1]}"
    if p[0] == "mid_block":
        return _ldm_name("encoder." + ".".join(p))
    raise KeyError(f"unknown diffusers VAE decoder key {key!r}")


def canonical_decoder_state_dict(sd, specs=None):
    """Any supported VAE state dict -> {ldm Decoder name (no prefix) | post_quant_conv.*: fp32 CPU tensor}, shaped as the ldm modules.
    The formats of ``canonical_state_dict`` (ldm AutoencoderKL decoder.* + post_quant_conv.*, CompVis first_stage_model.*, diffusers with
    either attention naming; Linear [C, C] attention weights become 1x1 convolutions).  Encoder keys are ignored.  ``specs``
    (decoder_plan's) checks names and shapes: an incomplete or unknown key set raises and names the keys."""
    def mapper(sd):
        levels = _levels(specs) if specs is not None else \
            1 + max([int(k.split(".")[2]) for k in sd if k.startswith("decoder.up_blocks.")] or [0])
        return lambda k: _ldm_decoder_name(k, levels)
    return _canonical(sd, specs, "decoder", "post_quant_conv", "up_blocks.", mapper)


def load_state_file(path):
    """A diffusers directory (config.json + diffusion_pytorch_model.safetensors | .bin) or one .ckpt / .pt / .bin / .safetensors file ->
    (state dict, config dict or None)."""
    cfg = None
    if os.path.isdir(path):
        cp = os.path.join(path, "config.json")
        cfg = json.load(open(cp)) if os.path.isfile(cp) else None
        for fn in ("diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.bin"):
            if os.path.isfile(os.path.join(path, fn)):
                path = os.path.join(path, fn)
                break
        else:
            raise FileNotFoundError(f"{path}: no diffusion_pytorch_model.safetensors / .bin")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path, device="cpu"), cfg
    return torch.load(path, map_location="cpu", weights_only=False), cfg


# ------------------------------------------------------------------------------------------------ the encoder
class _VAENet(ForwardNet):
    """What the encoder and the decoder share: the weight arena (fp32 + bf16 copy, conv_wprep operands), the grown-never-shrunk
    workspaces and the forward blocks over the HIP kernels.  A subclass sets ``specs`` / ``ops`` and calls ``_arena``."""

    _CONFIG_KEYS = (("layers_per_block", "num_res_blocks"), ("latent_channels", "z_channels"))

    def _arena(self):
        # arena: q / k / v of each attention as one [3C][C] matrix + [3C] bias, everything else in order; tensors at multiples of 8
        groups = []
        for op in self.ops:
            if op[0] == "attn":
                groups.append([op[1] + f".{w}.weight" for w in "qkv"])
                groups.append([op[1] + f".{w}.bias" for w in "qkv"])
        off, index = 0, {}
        for grp in groups + [[n] for n in self.specs]:
            for n in grp:
                if n not in index:
                    index[n] = off
                    off += int(np.prod(self.specs[n]))
            off = _pad8(off)
        self.index, self.n_total = index, off
        self.params = torch.zeros(off, dtype=torch.float32, device=self.dev)
        self.params_bf16 = torch.zeros(off, dtype=torch.bfloat16, device=self.dev)
        self.conv3 = OrderedDict()
        for n, shp in self.specs.items():
            if n.endswith(".weight") and len(shp) == 4 and shp[2] == 3:
                co, ci = shp[0], shp[1]
                self.conv3[n[:-7]] = dict(co=co, ci=ci, cop=_pad8(co), cip=_pad8(ci),
                                          fwd=torch.zeros(_pad8(co) * 9 * _pad8(ci), dtype=torch.bfloat16, device=self.dev))
        self._zero_bias = {}

    # ---------------------------------------------------------------- weights
    @classmethod
    def from_state_dict(cls, sd, **kw):
        m = cls(**kw)
        m.load_state_dict(sd)
        return m

    @classmethod
    def _config_kwargs(cls, cfg, kw):
        """diffusers config.json -> constructor keywords (explicit keywords win)."""
        if cfg is not None:
            bo = cfg.get("block_out_channels")
            if bo:
                kw.setdefault("ch", bo[0])
                kw.setdefault("ch_mult", tuple(b // bo[0] for b in bo))
            for src, dst in cls._CONFIG_KEYS:
                if src in cfg:
                    kw.setdefault(dst, cfg[src])
        return kw

    @classmethod
    def from_pretrained(cls, path, **kw):
        """A diffusers AutoencoderKL directory or a single .ckpt / .pt / .safetensors (ldm, CompVis or diffusers keys)."""
        sd, cfg = load_state_file(path)
        return cls.from_state_dict(sd, **cls._config_kwargs(cfg, kw))

    def state_dict(self):
        return OrderedDict((n, self.view(n).detach().cpu().clone()) for n in self.specs)

    def load_state_dict(self, sd):
        can = self._canonical(sd)
        with torch.no_grad():
            for n, v in can.items():
                self.view(n).copy_(v.to(self.dev))
        check(_L().sfron_cast_bf16(ptr(self.params), ptr(self.params_bf16), self.n_total, stream_ptr()), "cast_bf16")
        for base, v in self.conv3.items():
            check(_L().sfron_conv_wprep(self._p(base + ".weight"), v["co"], v["ci"], 9, v["cop"], v["cip"], ptr(v["fwd"]), None, stream_ptr()),
                  "conv_wprep")
            if v["cop"] != v["co"]:
                b = torch.zeros(v["cop"], dtype=torch.float32, device=self.dev)
                b[:v["co"]] = self.view(base + ".bias")
                self._zero_bias[base] = b
        return self

    # ---------------------------------------------------------------- blocks (forward only)
    def _gn(self, x, B, HW, C, name, swish, out_key):
        y = self._buf(out_key, B * HW * C, torch.bfloat16)
        mean = self._buf("gn_mean", B * 32, torch.float32)
        rstd = self._buf("gn_rstd", B * 32, torch.float32)
        ws = self._buf("gn_ws", _L().sfron_groupnorm_scratch_bytes(B, HW, C, 32) // 4 + 4, torch.float32)
        guard(x, y)
        check(_L().sfron_groupnorm_fwd(ptr(x), C, self._p(name + ".weight"), self._p(name + ".bias"), B, HW, C, 32, GN_EPS, int(swish), None, 1.0,
                                       ptr(y), ptr(mean), ptr(rstd), ptr(ws), stream_ptr()), "groupnorm_fwd")
        return y

    def _conv3(self, src, B, hs, ws, name, ho, wo, out_key, stride=1, pad=1, resid=None, up=0):
        v = self.conv3[name]
        out = self._buf(out_key, B * ho * wo * v["cop"], torch.float32).view(B * ho * wo, v["cop"])
        bias = self._zero_bias.get(name)
        bias = self._p(name + ".bias") if bias is None else bias
        guard(src, out, resid)
        d = _conv_desc(B, hs, ws, v["cip"], ho, wo, v["cop"], 9, stride, pad, up, 0, bias=bias, resid=resid, out_f32=out, ld_out=v["cop"])
        check(_L().sfron_conv_fwd(ctypes.byref(d), ptr(src), ptr(v["fwd"]), stream_ptr()), "conv_fwd")
        return out

    def _cast(self, x, rows, C, key):
        y = self._buf(key, rows * C, torch.bfloat16)
        guard(x, y)
        check(_L().sfron_cast_rows_bf16(ptr(x), C, rows, C, ptr(y), stream_ptr()), "cast_rows")
        return y

    def _resblock(self, x, B, H, W, name, cin, cout, out_key):
        """model.py:117-137 with temb None and dropout off: x + conv2(swish(norm2(conv1(swish(norm1(x)))))), 1x1 shortcut if cin != cout."""
        HW = H * W
        a1 = self._gn(x, B, HW, cin, name + ".norm1", True, "bf_a")
        h1 = self._conv3(a1, B, H, W, name + ".conv1", H, W, "f_h")
        a2 = self._gn(h1, B, HW, cout, name + ".norm2", True, "bf_a")
        if cin != cout:
            xb = self._cast(x, B * HW, cin, "bf_b")
            sc = self._buf("f_sc", B * HW * cout, torch.float32)
            guard(xb, sc)
            bgemm(xb, self._w(name + ".nin_shortcut.weight"), B * HW, cout, cin, lda=cin, ldb=cin, bias=self._p(name + ".nin_shortcut.bias"),
                  c_f32=sc, ldc=cout)
        else:
            sc = x
        return self._conv3(a2, B, H, W, name + ".conv2", H, W, out_key, resid=sc)

    def _attn(self, x, B, H, W, name, C, out_key):
        """model.py:166-190: x + proj_out(softmax(q k^T / sqrt(C)) v), single head, q / k / v as one [3C][C] product."""
        T, rows = H * W, B * H * W
        hn = self._gn(x, B, T, C, name + ".norm", False, "bf_a")
        qkv = self._buf("bf_qkv", rows * 3 * C, torch.bfloat16)
        guard(hn, qkv)
        bgemm(hn, self._w(name + ".q.weight"), rows, 3 * C, C, lda=C, ldb=C, bias=self._p(name + ".q.bias"), c_bf16=qkv, ldc=3 * C)
        q, k, v = qkv.data_ptr(), qkv.data_ptr() + 2 * C, qkv.data_ptr() + 4 * C
        S = self._buf("f_s", B * T * T, torch.float32)
        guard(S)
        bgemm(q, k, T, T, C, lda=3 * C, ldb=3 * C, batch=B, sa=T * 3 * C, sb=T * 3 * C, sc=T * T, c_f32=S, ldc=T)
        Pm = self._buf("bf_p", B * T * T, torch.bfloat16)
        check(_L().sfron_softmax_fwd(ptr(S), B * T, T, T, float(int(C) ** (-0.5)), ptr(Pm), stream_ptr()), "softmax_fwd")
        O = self._buf("bf_b", rows * C, torch.bfloat16)
        bgemm(Pm, v, T, C, T, lda=T, ldb=3 * C, b_t=True, batch=B, sa=T * T, sb=T * 3 * C, sc=T * C, c_bf16=O, ldc=C)
        out = self._buf(out_key, rows * C, torch.float32)
        guard(O, out, x)
        bgemm(O, self._w(name + ".proj_out.weight"), rows, C, C, lda=C, ldb=C, bias=self._p(name + ".proj_out.bias"), c_f32=out, ldc=C, resid=x)
        return out


class VAEEncoder(_VAENet):
    """image -> VAE posterior moments / latent on the GPU.  ``moments(images)`` gives [B, 2z, H/8, W/8] fp32 (mean || logvar);
    ``encode(images)`` the scaled posterior sample.  images: uint8 [B, H, W, 3] (host or device; ``flip`` uint8/bool [B] mirrors a
    sample) or fp32 [B, 3, H, W] in [-1, 1]."""

    _CONFIG_KEYS = _VAENet._CONFIG_KEYS + (("in_channels", "in_channels"),)
    _UNTILED = " (tiled encoding is not supported)"

    def __init__(self, ch=128, ch_mult=(1, 2, 4, 4), num_res_blocks=2, z_channels=4, in_channels=3, attn_resolutions=(), device="cuda",
                 max_chunk_bytes=1 << 30, resolution=256):
        super().__init__(device)
        if ch % 32:
            raise ValueError("GroupNorm(32) needs ch % 32 == 0")
        self.ch, self.ch_mult, self.z, self.in_channels = ch, tuple(ch_mult), z_channels, in_channels
        self.max_chunk_bytes = int(max_chunk_bytes)
        self.specs, self.ops = encoder_plan(ch, ch_mult, num_res_blocks, z_channels, in_channels, attn_resolutions, resolution)
        self._arena()

    def _canonical(self, sd):
        return canonical_state_dict(sd, self.specs)

    def per_sample_bytes(self, H, W):
        """Bytes of the largest operand one sample contributes to a launch (fp32 activations; attention scores; the input)."""
        big, res_h, res_w = max(H * W * 8 * 2, H * W * 3), H, W
        for op in self.ops:
            if op[0] == "conv_in":
                big = max(big, res_h * res_w * self.ch * 4)
            elif op[0] == "res":
                big = max(big, res_h * res_w * max(op[2], op[3]) * 4)
            elif op[0] == "attn":
                T = res_h * res_w
                big = max(big, T * T * 4, T * 3 * op[2] * 2, T * op[2] * 4)
            elif op[0] == "down":
                res_h, res_w = res_h // 2, res_w // 2
        return big

    def _chunk(self, images, flip, lo, hi, mom_f32, mom_f16, eps, scale, lat):
        """Encoder + quant_conv (+ posterior sample) of samples [lo, hi) of the batch, results written at their batch offset."""
        L, B = _L(), hi - lo
        if images.dtype == torch.uint8:
            H, W = images.shape[1], images.shape[2]
            xr = self._buf("bf_in", B * H * W * 8, torch.bfloat16)
            src = images[lo:hi]
            guard(src, xr)
            check(L.sfron_image_u8_to_rows_bf16(ptr(src), B, H, W, ptr(flip[lo:hi]) if flip is not None else None, 8, ptr(xr), stream_ptr()),
                  "image_u8_to_rows_bf16")
        else:
            H, W = images.shape[2], images.shape[3]
            xr = self._buf("bf_in", B * H * W * 8, torch.bfloat16)
            src = images[lo:hi]
            guard(src, xr)
            check(L.sfron_nchw_to_rows_bf16(ptr(src), B, self.in_channels, H * W, 8, ptr(xr), stream_ptr()), "nchw_to_rows")
        cur, spare = "f_x0", "f_x1"
        x = self._conv3(xr, B, H, W, "conv_in", H, W, cur)
        h, w = H, W
        for op in self.ops[1:]:
            if op[0] == "res":
                x = self._resblock(x, B, h, w, op[1], op[2], op[3], spare)
            elif op[0] == "attn":
                x = self._attn(x, B, h, w, op[1], op[2], spare)
            elif op[0] == "down":
                xb = self._cast(x, B * h * w, op[2], "bf_b")
                x = self._conv3(xb, B, h, w, op[1], h // 2, w // 2, spare, stride=2, pad=0)
                h, w = h // 2, w // 2
            elif op[0] == "out":
                a = self._gn(x, B, h * w, op[1], "norm_out", True, "bf_a")
                x = self._conv3(a, B, h, w, "conv_out", h, w, "f_h")
                continue
            cur, spare = spare, cur
        z2, hw = 2 * self.z, h * w
        v = self.conv3["conv_out"]
        sl = lambda t, c: None if t is None else t.data_ptr() + t.element_size() * lo * c * hw
        check(L.sfron_vae_moments(ptr(x), v["cop"], B, hw, z2, self._p("quant_conv.weight"), self._p("quant_conv.bias"), sl(mom_f32, z2),
                                  sl(mom_f16, z2), sl(eps, self.z), float(scale), sl(lat, self.z), stream_ptr()), "vae_moments")

    def _prepare(self, images, flip):
        if images.dtype == torch.uint8:
            if images.dim() != 4 or images.shape[3] != 3:
                raise ValueError(f"uint8 images must be [B, H, W, 3], got {tuple(images.shape)}")
            H, W = images.shape[1], images.shape[2]
            images = images.to(self.dev, non_blocking=True).contiguous()
            if flip is not None:
                flip = torch.as_tensor(flip).to(device=self.dev, dtype=torch.uint8).contiguous()
                if flip.shape != (images.shape[0],):
                    raise ValueError("flip must be [B]")
        elif images.dtype == torch.float32:
            if images.dim() != 4 or images.shape[1] != self.in_channels:
                raise ValueError(f"fp32 images must be [B, {self.in_channels}, H, W], got {tuple(images.shape)}")
            if flip is not None:
                raise ValueError("flip applies to uint8 HWC images; flip fp32 NCHW input before the call")
            H, W = images.shape[2], images.shape[3]
            images = images.to(self.dev).contiguous()
        else:
            raise TypeError(f"images must be uint8 [B,H,W,3] or fp32 [B,3,H,W], got {images.dtype}")
        f = 1 << (len(self.ch_mult) - 1)
        if H % f or W % f:
            raise ValueError(f"image size {H}x{W} is not a multiple of {f}")
        return images, flip, H, W, f

    @torch.no_grad()
    def moments(self, images, flip=None, dtype=torch.float32):
        """[B, 2z, H/8, W/8] posterior moments (mean || logvar) on the device, fp32 (or fp16, rounded in the kernel)."""
        images, flip, H, W, f = self._prepare(images, flip)
        B = images.shape[0]
        if dtype not in (torch.float32, torch.float16):
            raise TypeError("moments dtype: float32 or float16")
        out = torch.empty(B, 2 * self.z, H // f, W // f, dtype=dtype, device=self.dev)
        n = self.chunk_size(H, W)
        for lo in range(0, B, n):
            self._chunk(images, flip, lo, min(B, lo + n), out if dtype == torch.float32 else None, out if dtype == torch.float16 else None,
                        None, 1.0, None)
        return out

    @torch.no_grad()
    def encode(self, images, eps=None, generator=None, flip=None, scale=0.18215, return_moments=False):
        """scale * (mean + exp(0.5 clamp(logvar, -30, 20)) * eps): vae.encode(x).latent_dist.sample().mul_(scale), eps ~ N(0, 1) drawn
        from ``generator`` (on its device) when not given.  Bit-identical to sfron_latent_sample over ``moments()``."""
        images, flip, H, W, f = self._prepare(images, flip)
        B, h, w = images.shape[0], H // f, W // f
        if eps is None:
            gdev = generator.device if generator is not None else self.dev
            eps = torch.randn(B, self.z, h, w, generator=generator, device=gdev)
        eps = eps.to(self.dev, torch.float32).contiguous()
        if tuple(eps.shape) != (B, self.z, h, w):
            raise ValueError(f"eps must be {(B, self.z, h, w)}, got {tuple(eps.shape)}")
        mom = torch.empty(B, 2 * self.z, h, w, dtype=torch.float32, device=self.dev)
        lat = torch.empty(B, self.z, h, w, dtype=torch.float32, device=self.dev)
        n = self.chunk_size(H, W)
        for lo in range(0, B, n):
            self._chunk(images, flip, lo, min(B, lo + n), mom, None, eps, scale, lat)
        return (lat, mom) if return_moments else lat


def encoder_flops(H, W, ch=128, ch_mult=(1, 2, 4, 4), num_res_blocks=2, z_channels=4, in_channels=3, attn_resolutions=(), resolution=256):
    """Algorithmic FLOPs of one image: 2 * pixels * Cout * Cin * k^2 per convolution (+ quant_conv) and 4 T^2 C per attention."""
    specs, ops = encoder_plan(ch, ch_mult, num_res_blocks, z_channels, in_channels, attn_resolutions, resolution)
    total, h, w = 0.0, H, W
    for op in ops:
        if op[0] == "conv_in":
            total += 2.0 * h * w * ch * in_channels * 9
        elif op[0] == "res":
            _, name, cin, cout = op
            total += 2.0 * h * w * (cout * cin * 9 + cout * cout * 9 + (cout * cin if cin != cout else 0))
        elif op[0] == "attn":
            T, C = h * w, op[2]
            total += 2.0 * T * C * 4 * C + 4.0 * T * T * C
        elif op[0] == "down":
            h, w = h // 2, w // 2
            total += 2.0 * h * w * op[2] * op[2] * 9
        elif op[0] == "out":
            total += 2.0 * h * w * 2 * z_channels * op[1] * 9 + 2.0 * h * w * (2 * z_channels) ** 2
    return total


# ------------------------------------------------------------------------------------------------ the decoder
class VAEDecoder(_VAENet):
    """latent -> image on the GPU: post_quant_conv(z / scale) + the ldm Decoder, forward only.  ``decode(z)`` gives fp32 [B, 3, H, W]
    (``vae.decode(z / 0.18215).sample``); ``decode_u8`` the uint8 bytes a PNG holds, per image or as the make_grid canvas."""

    _CONFIG_KEYS = _VAENet._CONFIG_KEYS + (("out_channels", "out_ch"),)
    _UNTILED = " (tiled decoding is not supported)"

    def __init__(self, ch=128, ch_mult=(1, 2, 4, 4), num_res_blocks=2, z_channels=4, out_ch=3, attn_resolutions=(), device="cuda",
                 max_chunk_bytes=1 << 30, resolution=256):
        super().__init__(device)
        if ch % 32:
            raise ValueError("GroupNorm(32) needs ch % 32 == 0")
        if z_channels > 16:
            raise ValueError("sfron_vae_latent_in takes at most 16 latent channels")
        self.ch, self.ch_mult, self.z, self.out_ch = ch, tuple(ch_mult), z_channels, out_ch
        self.max_chunk_bytes = int(max_chunk_bytes)
        self.specs, self.ops = decoder_plan(ch, ch_mult, num_res_blocks, z_channels, out_ch, attn_resolutions, resolution)
        self.factor = 1 << (len(self.ch_mult) - 1)
        self._arena()

    def _canonical(self, sd):
        return canonical_decoder_state_dict(sd, self.specs)

    def per_sample_bytes(self, H, W):
        """Bytes of the largest operand one sample contributes to a launch, for an H x W output image (fp32 activations, the upsampled
        convolution outputs, attention scores, the conv_out rows)."""
        h, w = H // self.factor, W // self.factor
        big = max(h * w * self.z * 4, h * w * _pad8(self.z) * 2, H * W * _pad8(self.out_ch) * 4)
        for op in self.ops:
            if op[0] == "conv_in":
                big = max(big, h * w * op[2] * 4)
            elif op[0] == "res":
                big = max(big, h * w * max(op[2], op[3]) * 4)
            elif op[0] == "attn":
                T = h * w
                big = max(big, T * T * 4, T * 3 * op[2] * 2, T * op[2] * 4)
            elif op[0] == "up":
                h, w = 2 * h, 2 * w
                big = max(big, h * w * op[2] * 4)
        return big

    def _chunk(self, z, lo, hi, scale):
        """post_quant_conv + Decoder of samples [lo, hi): returns the conv_out rows [B*H*W][8] fp32 (a workspace view)."""
        L, B = _L(), hi - lo
        h, w = z.shape[2], z.shape[3]
        v = self.conv3["conv_in"]
        zr = self._buf("bf_in", B * h * w * v["cip"], torch.bfloat16)
        src = z[lo:hi]
        guard(src, zr)
        check(L.sfron_vae_latent_in(ptr(src), B, self.z, h * w, self._p("post_quant_conv.weight"), self._p("post_quant_conv.bias"),
                                    float(scale), v["cip"], ptr(zr), None, stream_ptr()), "vae_latent_in")
        cur, spare = "f_x0", "f_x1"
        x = self._conv3(zr, B, h, w, "conv_in", h, w, cur)
        for op in self.ops[1:]:
            if op[0] == "res":
                x = self._resblock(x, B, h, w, op[1], op[2], op[3], spare)
            elif op[0] == "attn":
                x = self._attn(x, B, h, w, op[1], op[2], spare)
            elif op[0] == "up":
                xb = self._cast(x, B * h * w, op[2], "bf_b")
                x = self._conv3(xb, B, h, w, op[1], 2 * h, 2 * w, spare, up=1)
                h, w = 2 * h, 2 * w
            elif op[0] == "out":
                a = self._gn(x, B, h * w, op[1], "norm_out", True, "bf_a")
                x = self._conv3(a, B, h, w, "conv_out", h, w, "f_h")
                continue
            cur, spare = spare, cur
        return x

    def _prepare(self, z):
        z = torch.as_tensor(z)
        if z.dim() != 4 or z.shape[1] != self.z:
            raise ValueError(f"latents must be [B, {self.z}, h, w], got {tuple(z.shape)}")
        z = z.to(self.dev, torch.float32).contiguous()
        return z, z.shape[0], z.shape[2] * self.factor, z.shape[3] * self.factor

    @torch.no_grad()
    def decode(self, z, scale=0.18215):
        """[B, out_ch, H, W] fp32 on the device: Decoder(post_quant_conv(z / scale)), H = h * 8 for KL-f8."""
        z, B, H, W = self._prepare(z)
        out = torch.empty(B, self.out_ch, H, W, dtype=torch.float32, device=self.dev)
        n = self.chunk_size(H, W)
        for lo in range(0, B, n):
            hi = min(B, lo + n)
            rows = self._chunk(z, lo, hi, scale)
            dst = out[lo:hi]
            guard(rows, dst)
            check(_L().sfron_rows_to_nchw(ptr(rows), rows.shape[1], hi - lo, self.out_ch, H * W, ptr(dst), stream_ptr()), "rows_to_nchw")
        return out

    @torch.no_grad()
    def decode_u8(self, z, scale=0.18215, mode="save_image", nrow=0, padding=2, value_range=(-1.0, 1.0)):
        """uint8 on the device.  mode "save_image": torchvision save_image(normalize=True, value_range) bytes; "round": the diffusers /
        SD generate-images.py bytes ((x / 2 + 0.5).clamp(0, 1) * 255, rounded half to even); "trunc": the DiT/sample_ddp.py:132 bytes
        (clamp(127.5 * x + 128, 0, 255) truncated; value_range unused).  nrow == 0: [B, H, W, 3]; nrow > 0: the make_grid(nrow, padding)
        canvas [Hc, Wc, 3] (images.grid_geometry)."""
        from .images import grid_geometry, image_mode
        if self.out_ch != 3:
            raise ValueError("decode_u8 writes RGB: out_ch must be 3")
        m = image_mode(mode)
        z, B, H, W = self._prepare(z)
        lo_v, hi_v = (float(value_range[0]), float(value_range[1]))
        if nrow > 0:
            Hc, Wc = grid_geometry(B, H, W, nrow, padding)[:2]
            out = torch.empty(Hc, Wc, 3, dtype=torch.uint8, device=self.dev)
        else:
            out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=self.dev)
        n = self.chunk_size(H, W)
        for lo in range(0, B, n):
            hi = min(B, lo + n)
            rows = self._chunk(z, lo, hi, scale)
            guard(rows, out)
            check(_L().sfron_rows_to_image_u8(ptr(rows), rows.shape[1], hi - lo, H, W, m, lo_v, hi_v, int(nrow), int(padding), lo, B,
                                               ptr(out), stream_ptr()), "rows_to_image_u8")
        return out


def load_autoencoder(src, **kw):
    """(VAEEncoder, VAEDecoder) from ONE AutoencoderKL state: a path (read once, as from_pretrained) or a state dict in any supported
    format.  Keywords common to both (ch, ch_mult, num_res_blocks, z_channels, attn_resolutions, resolution, device, max_chunk_bytes) go
    to both; in_channels to the encoder, out_ch to the decoder."""
    cfg = None
    sd = src
    if isinstance(src, (str, os.PathLike)):
        sd, cfg = load_state_file(os.fspath(src))
    enc_kw = {k: v for k, v in kw.items() if k != "out_ch"}
    dec_kw = {k: v for k, v in kw.items() if k != "in_channels"}
    enc = VAEEncoder.from_state_dict(sd, **VAEEncoder._config_kwargs(cfg, enc_kw))
    dec = VAEDecoder.from_state_dict(sd, **VAEDecoder._config_kwargs(cfg, dec_kw))
    return enc, dec


def decoder_flops(H, W, ch=128, ch_mult=(1, 2, 4, 4), num_res_blocks=2, z_channels=4, out_ch=3, attn_resolutions=(), resolution=256):
    """Algorithmic FLOPs of decoding one H x W image: 2 * pixels * Cout * Cin * k^2 per convolution (post_quant_conv included; an
    Upsample's convolution at the doubled resolution) and 4 T^2 C per attention."""
    specs, ops = decoder_plan(ch, ch_mult, num_res_blocks, z_channels, out_ch, attn_resolutions, resolution)
    f = 1 << (len(ch_mult) - 1)
    h, w = H // f, W // f
    total = 2.0 * h * w * z_channels * z_channels
    for op in ops:
        if op[0] == "conv_in":
            total += 2.0 * h * w * op[2] * op[1] * 9
        elif op[0] == "res":
            _, name, cin, cout = op
            total += 2.0 * h * w * (cout * cin * 9 + cout * cout * 9 + (cout * cin if cin != cout else 0))
        elif op[0] == "attn":
            T, C = h * w, op[2]
            total += 2.0 * T * C * 4 * C + 4.0 * T * T * C
        elif op[0] == "up":
            h, w = 2 * h, 2 * w
            total += 2.0 * h * w * op[2] * op[2] * 9
        elif op[0] == "out":
            total += 2.0 * h * w * out_ch * op[1] * 9
    return total
