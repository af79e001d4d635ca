"""The CLIP text encoder of SD v1 (prompt -> [B, 77, 768] cross-attention context) over the HIP kernels of csrc/text.hip and gemm.hip,
forward only.

Restates SD/ldm/modules/encoders/modules.py ``FrozenCLIPEmbedder`` (:230-266): the tokenizer call with truncation=True,
max_length=77, padding="max_length", then transformers ``CLIPTextModel(input_ids=tokens).last_hidden_state`` -- token + position
embedding, pre-LN layers ``x += out_proj(causal_attn(ln1(x)))``, ``x += fc2(quick_gelu(fc1(ln2(x))))``, a final LayerNorm.  No padding mask
(the reference passes no attention_mask); the causal mask is the only one.

Tokenizer: ``CLIPTokenizer`` restates the byte-level BPE of transformers' CLIPTokenizer with the standard library only.  Text cleanup is
what transformers does without ``ftfy``: NFC, every whitespace run -> one space, lower case.  ``ftfy.fix_text`` (mojibake repair) is NOT
restated: text that ftfy would change can tokenize differently from an ftfy-equipped reference.

Weights live in one fp32 arena (matrices first, q / k / v of a layer concatenated into one [3D][D] matrix + [3D] bias) and a bf16 shadow
of the matrix region the products read.  Activations live in workspaces grown on demand and reused by every later call, on the current
stream.  Operand bound: the products address their operands with 32-bit byte counts, so every launch asserts that no operand reaches 2 GiB
(forward_net.py's rule); at width 768 that is about 350 000 prompts per call, far beyond any batch this is meant for.
"""
import ctypes
import json
import os
import unicodedata
from collections import OrderedDict
from functools import lru_cache

import numpy as np
import torch

from . import _lib
from ._lib import check, lib as _L, ptr, stream_ptr
from .forward_net import ForwardNet, guard

BOS, EOS = "<|startoftext|>", "<|endoftext|>"
LN_EPS = 1e-5
HEAD_DIM = 64
MAX_T = 128                   # sfron_attn_causal_fwd


# ------------------------------------------------------------------------------------------------ tokenizer
@lru_cache()
def bytes_to_unicode():
    """The byte -> printable character map of GPT-2 / CLIP byte-level BPE."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, [chr(c) for c in cs]))


_CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")


def _is_letter(c):
    return unicodedata.category(c).startswith("L")


def _is_number(c):
    return unicodedata.category(c).startswith("N")


def normalize(text):
    """transformers' CLIP normalizer without ftfy: NFC, whitespace runs -> one space, lower case."""
    text = unicodedata.normalize("NFC", text)
    out, prev_space = [], False
    for c in text:
        if c.isspace():
            if not prev_space:
                out.append(" ")
            prev_space = True
        else:
            out.append(c)
            prev_space = False
    return "".join(out).lower()


def pretokenize(text):
    """The CLIP split pattern  <|startoftext|>|<|endoftext|>|'s|'t|'re|'ve|'m|'ll|'d|[\\p{L}]+|[\\p{N}]|[^\\s\\p{L}\\p{N}]+  over normalized
    text (whitespace between pieces dropped), with the letter / number classes taken from unicodedata categories."""
    pieces, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if c.isspace():
            i += 1
            continue
        for lit in (BOS, EOS) + _CONTRACTIONS:
            if text.startswith(lit, i):
                pieces.append(lit)
                i += len(lit)
                break
        else:
            j = i + 1
            if _is_letter(c):
                while j < n and _is_letter(text[j]):
                    j += 1
            elif not _is_number(c):
                while j < n and not (text[j].isspace() or _is_letter(text[j]) or _is_number(text[j])):
                    j += 1
            pieces.append(text[i:j])
            i = j
    return pieces


class CLIPTokenizer:
    """Byte-level BPE of CLIP (transformers CLIPTokenizer) over a ``vocab.json`` / ``merges.txt`` pair.  ``__call__(texts)`` gives int64
    ids [B, max_length] as the reference's call (modules.py:247-262): BOS, at most max_length - 2 tokens, EOS, pad tokens after.  A
    literal ``<|endoftext|>`` / ``<|startoftext|>`` in the text is the special token."""

    def __init__(self, vocab_json, merges_txt, pad_token=EOS):
        with open(vocab_json, encoding="utf-8") as f:
            self.encoder = json.load(f)
        with open(merges_txt, encoding="utf-8") as f:
            lines = f.read().strip().split("\n")
        merges = [tuple(m.split()) for m in lines if m and not m.startswith("#version")]
        self.bpe_ranks = {m: i for i, m in enumerate(merges) if len(m) == 2}
        self.byte_encoder = bytes_to_unicode()
        self.bos_id, self.eos_id, self.pad_id = self.encoder[BOS], self.encoder[EOS], self.encoder[pad_token]
        self.unk_id = self.encoder[EOS]
        self._cache = {}

    @classmethod
    def from_pretrained(cls, path, **kw):
        """A directory holding vocab.json + merges.txt (a diffusers ``tokenizer/`` folder or the hub's openai/clip-vit-large-patch14)."""
        return cls(os.path.join(path, "vocab.json"), os.path.join(path, "merges.txt"), **kw)

    def bpe(self, piece):
        if piece in self._cache:
            return self._cache[piece]
        word = list(piece[:-1]) + [piece[-1] + "</w>"]
        while len(word) > 1:
            best = min(((self.bpe_ranks.get((a, b), 1 << 62), k) for k, (a, b) in enumerate(zip(word, word[1:]))))
            if best[0] == 1 << 62:
                break
            a, b = word[best[1]], word[best[1] + 1]
            merged, k = [], 0
            while k < len(word):
                if k < len(word) - 1 and word[k] == a and word[k + 1] == b:
                    merged.append(a + b)
                    k += 2
                else:
                    merged.append(word[k])
                    k += 1
            word = merged
        self._cache[piece] = word
        return word

    def encode(self, text):
        """Token ids of one text, without BOS / EOS."""
        ids = []
        for seg, special in self._split_special(text):
            if special:
                ids.append(self.encoder[seg])
                continue
            for piece in pretokenize(normalize(seg)):
                mapped = "".join(self.byte_encoder[b] for b in piece.encode("utf-8"))
                ids.extend(self.encoder.get(t, self.unk_id) for t in self.bpe(mapped))
        return ids

    @staticmethod
    def _split_special(text):
        out, i = [], 0
        while True:
            hits = [(text.find(s, i), s) for s in (BOS, EOS)]
            hits = [(p, s) for p, s in hits if p >= 0]
            if not hits:
                out.append((text[i:], False))
                return out
            p, s = min(hits)
            out.append((text[i:p], False))
            out.append((s, True))
            i = p + len(s)

    def __call__(self, texts, max_length=77):
        if isinstance(texts, str):
            texts = [texts]
        out = np.full((len(texts), max_length), self.pad_id, dtype=np.int64)
        for b, t in enumerate(texts):
            ids = [self.bos_id] + self.encode(t)[:max_length - 2] + [self.eos_id]
            out[b, :len(ids)] = ids
        return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------ weight formats
# CompVis LDM checkpoints (FrozenCLIPEmbedder.transformer: with / without the text_model level, by transformers version), HF CLIPTextModel
# checkpoints, and the bare CLIPTextTransformer names recent transformers versions give CLIPTextModel.state_dict()
_PREFIXES = ("cond_stage_model.transformer.text_model.", "cond_stage_model.transformer.", "text_model.", "")


def _strip(sd):
    """Any supported naming -> {HF name without the text_model. prefix: tensor}; position_ids and foreign keys dropped."""
    if "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    out = {}
    for k, v in sd.items():
        for p in _PREFIXES:
            if k.startswith(p):
                n = k[len(p):]
                if n.startswith("text_model."):
                    n = n[len("text_model."):]
                if n.startswith(("embeddings.", "encoder.", "final_layer_norm.")) and not n.endswith("position_ids"):
                    out[n] = v
                break
    if not out:
        raise KeyError(f"not a CLIP text encoder state dict: no text_model.* / cond_stage_model.transformer.* keys (first keys: {list(sd)[:5]})")
    return out


def config_from_state_dict(sd):
    """(vocab, max_position, width, layers, mlp) read off the tensor shapes of any supported naming."""
    s = _strip(sd)
    tok = s["embeddings.token_embedding.weight"]
    layers = 1 + max(int(k.split(".")[2]) for k in s if k.startswith("encoder.layers."))
    return dict(vocab_size=int(tok.shape[0]), max_position=int(s["embeddings.position_embedding.weight"].shape[0]), width=int(tok.shape[1]),
                layers=layers, mlp=int(s["encoder.layers.0.mlp.fc1.weight"].shape[0]))


def param_specs(vocab_size=49408, max_position=77, width=768, layers=12, mlp=3072):
    """Canonical arena entries in arena order: the matrices (qkv [3D][D], out_proj, fc1, fc2 per layer) first -- the region the bf16
    shadow copies -- then embeddings, biases and LayerNorms.  Returns (OrderedDict name -> shape, number of matrix entries)."""
    D, F = width, mlp
    P = []
    for i in range(layers):
        L = f"encoder.layers.{i}."
        P += [(L + "self_attn.qkv_proj.weight", (3 * D, D)), (L + "self_attn.out_proj.weight", (D, D)), (L + "mlp.fc1.weight", (F, D)),
              (L + "mlp.fc2.weight", (D, F))]
    n_mat = len(P)
    P += [("embeddings.token_embedding.weight", (vocab_size, D)), ("embeddings.position_embedding.weight", (max_position, D))]
    for i in range(layers):
        L = f"encoder.layers.{i}."
        P += [(L + "layer_norm1.weight", (D,)), (L + "layer_norm1.bias", (D,)), (L + "self_attn.qkv_proj.bias", (3 * D,)),
              (L + "self_attn.out_proj.bias", (D,)), (L + "layer_norm2.weight", (D,)), (L + "layer_norm2.bias", (D,)),
              (L + "mlp.fc1.bias", (F,)), (L + "mlp.fc2.bias", (D,))]
    P += [("final_layer_norm.weight", (D,)), ("final_layer_norm.bias", (D,))]
    return OrderedDict(P), n_mat


def canonical_state_dict(sd, specs=None):
    """HF ``text_model.*``, CompVis ``cond_stage_model.transformer.text_model.*`` or the older ``cond_stage_model.transformer.*`` ->
    {canonical name: fp32 CPU tensor} in arena order, q / k / v concatenated (q rows first, then k, then v).  Missing, unexpected or
    misshaped keys raise."""
    s = {k: torch.as_tensor(v).detach().to("cpu", torch.float32) for k, v in _strip(sd).items()}
    if specs is None:
        specs, _ = param_specs(**config_from_state_dict(sd))
    out, used = OrderedDict(), set()
    for n, shp in specs.items():
        if ".qkv_proj." in n:
            parts = [n.replace("qkv_proj", w) for w in ("q_proj", "k_proj", "v_proj")]
            miss = [p for p in parts if p not in s]
            if miss:
                raise KeyError(f"CLIP text encoder state dict: missing {miss}")
            t = torch.cat([s[p] for p in parts], 0)
            used.update(parts)
        else:
            if n not in s:
                raise KeyError(f"CLIP text encoder state dict: missing {n}")
            t = s[n]
            used.add(n)
        if tuple(t.shape) != tuple(shp):
            raise ValueError(f"{n}: shape {tuple(t.shape)}, the configuration needs {tuple(shp)}")
        out[n] = t
    extra = sorted(set(s) - used)
    if extra:
        raise KeyError(f"CLIP text encoder state dict: unexpected keys {extra[:8]}")
    return out


def arena_offsets(specs):
    """{name: element offset} of the arena (each entry at a multiple of 8 elements: 16-byte aligned bf16 rows) and the total length."""
    off, index = 0, {}
    for n, shp in specs.items():
        index[n] = off
        off += (int(np.prod(shp)) + 7) // 8 * 8
    return index, off


def pack_arena(canon, specs):
    """Canonical state dict -> the flat fp32 arena (CPU)."""
    index, total = arena_offsets(specs)
    flat = torch.zeros(total, dtype=torch.float32)
    for n, t in canon.items():
        flat[index[n]:index[n] + t.numel()] = t.reshape(-1)
    return flat


def load_state_file(path):
    """A transformers CLIPTextModel directory (model.safetensors | pytorch_model.bin), a diffusers root (text_encoder/ inside) or one
    .ckpt / .pt / .bin / .safetensors file -> state dict."""
    from .vae import load_state_file as _vae_load
    if os.path.isdir(path):
        if os.path.isdir(os.path.join(path, "text_encoder")):
            path = os.path.join(path, "text_encoder")
        for fn in ("model.safetensors", "pytorch_model.bin"):
            if os.path.isfile(os.path.join(path, fn)):
                path = os.path.join(path, fn)
                break
        else:
            raise FileNotFoundError(f"{path}: no model.safetensors / pytorch_model.bin")
    return _vae_load(path)[0]


# ------------------------------------------------------------------------------------------------ the encoder
class CLIPTextEncoder(ForwardNet):
    """prompts -> fp32 [B, 77, D] last_hidden_state on the GPU (FrozenCLIPEmbedder.encode).  ``encode_ids(ids)`` runs the transformer on
    int64 ids [B, T] (T <= 77); ``encode(texts)`` tokenizes first (needs ``tokenizer``); ``__call__`` = encode."""

    def __init__(self, vocab_size=49408, max_position=77, width=768, layers=12, heads=None, mlp=3072, tokenizer=None, max_length=77,
                 device="cuda"):
        super().__init__(device)
        heads = width // HEAD_DIM if heads is None else heads
        if heads * HEAD_DIM != width:
            raise ValueError(f"width {width} with {heads} heads: the attention kernel takes head_dim {HEAD_DIM} only")
        if max_length > min(max_position, MAX_T):
            raise ValueError(f"max_length {max_length}: at most {min(max_position, MAX_T)} positions")
        self.vocab, self.max_position, self.D, self.L, self.H, self.F = vocab_size, max_position, width, layers, heads, mlp
        self.tokenizer, self.max_length = tokenizer, max_length
        self.specs, n_mat = param_specs(vocab_size, max_position, width, layers, mlp)
        self.index, self.n_total = arena_offsets(self.specs)
        names = list(self.specs)
        self.n_mat = self.index[names[n_mat]]                    # the matrices are the arena's prefix
        self.params = torch.zeros(self.n_total, dtype=torch.float32, device=self.dev)
        self.params_bf16 = torch.zeros(self.n_mat, dtype=torch.bfloat16, device=self.dev)

    # ---------------------------------------------------------------- weights
    @classmethod
    def from_state_dict(cls, sd, **kw):
        cfg = config_from_state_dict(sd)
        cfg.update(kw)
        return cls(**cfg).load_state_dict(sd)

    @classmethod
    def from_pretrained(cls, path, tokenizer_path=None, **kw):
        """A diffusers root (text_encoder/ + tokenizer/), a transformers CLIPTextModel directory, or a CompVis .ckpt with
        ``tokenizer_path`` (a directory holding vocab.json + merges.txt)."""
        sd = load_state_file(path)
        if tokenizer_path is None and os.path.isdir(path):
            for cand in (os.path.join(path, "tokenizer"), path):
                if os.path.isfile(os.path.join(cand, "vocab.json")):
                    tokenizer_path = cand
                    break
        if tokenizer_path is not None and "tokenizer" not in kw:
            kw["tokenizer"] = CLIPTokenizer.from_pretrained(tokenizer_path)
        return cls.from_state_dict(sd, **kw)

    def load_state_dict(self, sd):
        flat = pack_arena(canonical_state_dict(sd, self.specs), self.specs)
        with torch.no_grad():
            self.params.copy_(flat.to(self.dev))
        check(_L().sfron_cast_bf16(ptr(self.params), ptr(self.params_bf16), self.n_mat, stream_ptr()), "cast_bf16")
        return self

    # ---------------------------------------------------------------- forward
    def _gemm(self, a, w, M, N, K, bias, epi, c_bf16=None, c_f32=None, accumulate=0):
        guard(a, c_bf16, c_f32)
        d = _lib.GemmDesc(A=a.data_ptr(), B=w, M=M, N=N, K=K, lda=K, ldb=K, epilogue=epi, alpha=1.0, bias=bias,
                          c_bf16=c_bf16.data_ptr() if c_bf16 is not None else None, ldc_bf16=N,
                          c_f32=c_f32.data_ptr() if c_f32 is not None else None, ldc_f32=N, tokens=1, accumulate=accumulate)
        check(_L().sfron_gemm_bf16(ctypes.byref(d), stream_ptr()), "gemm_bf16")

    def _ln(self, x, rows, name):
        y = self._buf("bf_h", rows * self.D, torch.bfloat16)
        mean, rstd = self._buf("ln_mean", rows, torch.float32), self._buf("ln_rstd", rows, torch.float32)
        guard(x, y)
        check(_L().sfron_layernorm_fwd(ptr(x), self._p(name + ".weight"), self._p(name + ".bias"), rows, self.D, LN_EPS, ptr(y), ptr(mean),
                                       ptr(rstd), stream_ptr()), "layernorm_fwd")
        return y

    def encode_ids(self, ids, check_ids=True):
        """int64 ids [B, T] (host or device) -> fp32 [B, T, D] last_hidden_state, on the current stream.  check_ids: read the embedding
        kernel's error word back (one synchronisation) and raise on an id outside the vocabulary; False leaves the call asynchronous
        (such a token's row then starts from zeros)."""
        ids = torch.as_tensor(ids)
        if ids.dim() == 1:
            ids = ids[None]
        B, T = ids.shape
        if T < 1 or T > min(self.max_position, MAX_T):
            raise ValueError(f"{T} positions: the encoder takes 1 .. {min(self.max_position, MAX_T)}")
        ids = ids.to(self.dev, torch.int64).contiguous()
        D, F, rows = self.D, self.F, B * T
        x = self._buf("f_x", rows * D, torch.float32)
        err = self._buf("err", 1, torch.int32)
        err.zero_()
        guard(x)
        check(_L().sfron_clip_embed(ptr(ids), B, T, self._p("embeddings.token_embedding.weight"), self.vocab,
                                    self._p("embeddings.position_embedding.weight"), D, ptr(x), ptr(err), stream_ptr()), "clip_embed")
        qkv = self._buf("bf_qkv", rows * 3 * D, torch.bfloat16)
        o = self._buf("bf_o", rows * D, torch.bfloat16)
        a = self._buf("bf_a", rows * F, torch.bfloat16)
        for i in range(self.L):
            L = f"encoder.layers.{i}."
            h = self._ln(x, rows, L + "layer_norm1")
            self._gemm(h, self._w(L + "self_attn.qkv_proj.weight"), rows, 3 * D, D, self._p(L + "self_attn.qkv_proj.bias"), _lib.EPI_BF16, c_bf16=qkv)
            guard(qkv, o)
            check(_L().sfron_attn_causal_fwd(ptr(qkv), ptr(o), B, T, self.H, HEAD_DIM, stream_ptr()), "attn_causal_fwd")
            self._gemm(o, self._w(L + "self_attn.out_proj.weight"), rows, D, D, self._p(L + "self_attn.out_proj.bias"), _lib.EPI_F32, c_f32=x,
                       accumulate=1)
            h = self._ln(x, rows, L + "layer_norm2")
            self._gemm(h, self._w(L + "mlp.fc1.weight"), rows, F, D, self._p(L + "mlp.fc1.bias"), _lib.EPI_QUICK_GELU, c_bf16=a)
            self._gemm(a, self._w(L + "mlp.fc2.weight"), rows, D, F, self._p(L + "mlp.fc2.bias"), _lib.EPI_F32, c_f32=x, accumulate=1)
        out = torch.empty(B, T, D, dtype=torch.float32, device=self.dev)
        guard(out)
        check(_L().sfron_layernorm_fwd_f32(ptr(x), self._p("final_layer_norm.weight"), self._p("final_layer_norm.bias"), rows, D, LN_EPS,
                                           ptr(out), stream_ptr()), "layernorm_fwd_f32")
        if check_ids and int(err.item()):
            raise ValueError(f"token id outside [0, {self.vocab}) in the input")
        return out

    def encode(self, texts):
        if self.tokenizer is None:
            raise ValueError("encode(texts) needs a tokenizer (CLIPTextEncoder(tokenizer=...) or from_pretrained); encode_ids takes ids")
        return self.encode_ids(self.tokenizer(texts, max_length=self.max_length))

    __call__ = encode


def load_text_encoder(src, tokenizer=None, **kw):
    """CLIPTextEncoder from a path (as from_pretrained; ``tokenizer`` may then be a vocab.json + merges.txt directory) or a state dict in
    any supported naming (``tokenizer`` a CLIPTokenizer or such a directory)."""
    if isinstance(tokenizer, (str, os.PathLike)):
        tokenizer = CLIPTokenizer.from_pretrained(os.fspath(tokenizer))
    if tokenizer is not None:
        kw["tokenizer"] = tokenizer
    if isinstance(src, (str, os.PathLike)):
        return CLIPTextEncoder.from_pretrained(os.fspath(src), **kw)
    return CLIPTextEncoder.from_state_dict(src, **kw)


def encoder_flops(T=77, width=768, layers=12, mlp=3072):
    """Algorithmic FLOPs of one prompt: 2 T D (3D + D + 2F) per layer for the products and 2 T^2 D for QK^T and PV (the causal half)."""
    return layers * (2.0 * T * width * (4 * width + 2 * mlp) + 2.0 * T * T * width)
