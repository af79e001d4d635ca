#!/usr/bin/env python3
"""Generate tests/golden/text_encoder.npz by IMPORTING the reference (build container only; the reference never travels to the GPU box).

Run:  python tests/golden/make_text_encoder_golden.py
The reference is SD/ldm/modules/encoders/modules.py FrozenCLIPEmbedder (:230-266), built with __new__ around
  - a transformers CLIPTokenizer over a SYNTHETIC vocabulary (the 256-character byte alphabet, its </w> forms, MERGES merges learned
    here from a small English corpus, the two special tokens) -- the real 49408-entry vocabulary is not available offline;
  - a seeded CLIPTextModel of width 128, 2 heads of 64, 2 layers, MLP 512, quick_gelu, 77 positions.
Its forward(prompts) gives last_hidden_state.  Contents (data only):
  vocab_json, merges_txt   the tokenizer files (text)
  prompts, ids             the prompts and the reference tokenizer's ids [P, 77]
  hidden                   last_hidden_state [P, 77, 128] fp32
  w_keys, w_scale, w_offset, w_q_<i>   weights in HF CLIPTextModel naming: tensor i = w_offset[i] + w_scale[i] * w_q_<i> (int8; the
                           scales are powers of two, so the fp32 weights the reference ran with are reproduced exactly)
  config                   [vocab, positions, width, layers, heads, mlp]
"""
import importlib
import json
import os
import sys
import tempfile
from collections import Counter

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_vae_golden as mg  # noqa: E402

OUT = os.path.join(HERE, "text_encoder.npz")
MERGES = 400
SEED = 20261018
CONFIG = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=77,
              hidden_act="quick_gelu", layer_norm_eps=1e-5)

CORPUS = """a photo of a person wearing clothes. a photo of a nude person. a painting of a cat sitting on a mat in the garden.
the quick brown fox jumps over the lazy dog. an astronaut riding a horse on the moon, highly detailed, trending on artstation.
a portrait of a woman with long hair, oil on canvas. a city street at night with neon lights and rain. there is the house where
they lived. the people are walking in the park with their dogs and children. a beautiful landscape with mountains, rivers and
forests under a blue sky. photograph of an old man reading the newspaper. the weather is nice and the sun is shining.
it is what it is, and that is that. this is the best picture of the year. these pictures were taken in the summer of the nineties.
"""

PROMPTS = [
    "a photo of a nude person",
    "a photo of a person wearing clothes",
    "A PHOTO OF A Cat On The MOON",
    "the 1990s were 2000 years after year 10",
    "don't stop, it's what we'll do; they've been there, I'm sure you'd agree",
    "wow!!! really?!... (yes) -- #hashtag @user $100 & more...",
    "a   cat\n\n on   a\tmat  ",
    "café naïve résumé Ωμέγα русский 日本語 emoji 🙂",
    "",
    "a photo <|endoftext|> of a dog",
    ("a very long prompt about a painting of a beautiful landscape with mountains, rivers and forests under a blue sky, an old man "
     "reading the newspaper in the park while the people are walking with their dogs and children on a summer day of the nineties, "
     "highly detailed, trending on artstation, oil on canvas, neon lights and rain at night in the city street"),
]


def _ours():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import sfron.text as T    # noqa: the restated pre-tokenizer is only used to LEARN merges; the ids below come from transformers
    return T


def learn_vocab(T):
    be = T.bytes_to_unicode()
    words = Counter()
    for piece in T.pretokenize(T.normalize(CORPUS)):
        mapped = "".join(be[b] for b in piece.encode("utf-8"))
        words[tuple(mapped[:-1]) + (mapped[-1] + "</w>",)] += 1
    merges = []
    for _ in range(MERGES):
        pairs = Counter()
        for w, c in words.items():
            for a, b in zip(w, w[1:]):
                pairs[(a, b)] += c
        if not pairs:
            break
        best = max(sorted(pairs), key=lambda p: pairs[p])
        merges.append(best)
        nw = Counter()
        for w, c in words.items():
            out, k = [], 0
            while k < len(w):
                if k < len(w) - 1 and (w[k], w[k + 1]) == best:
                    out.append(w[k] + w[k + 1])
                    k += 2
                else:
                    out.append(w[k])
                    k += 1
            nw[tuple(out)] += c
        words = nw
    alphabet = list(be.values())
    vocab = alphabet + [c + "</w>" for c in alphabet] + ["".join(m) for m in merges] + ["<|startoftext|>", "<|endoftext|>"]
    assert len(set(vocab)) == len(vocab)
    vocab_json = json.dumps({t: i for i, t in enumerate(vocab)}, ensure_ascii=False)
    merges_txt = "#version: 0.2\n" + "\n".join(f"{a} {b}" for a, b in merges) + "\n"
    return vocab_json, merges_txt, len(vocab)


def quantized_weights(shapes):
    """HF name -> (int8 q, scale, offset), drawn key by key in sorted order from one seeded CPU generator."""
    g = torch.Generator().manual_seed(SEED)
    out = {}
    for k in sorted(shapes):
        shp = shapes[k]
        q = torch.clamp(torch.round(torch.randn(shp, generator=g) * 40.0), -127, 127).to(torch.int8)
        if "token_embedding" in k:
            scale, off = 2.0 ** -6, 0.0
        elif "position_embedding" in k:
            scale, off = 2.0 ** -7, 0.0
        elif "layer_norm" in k and k.endswith(".weight"):
            scale, off = 2.0 ** -9, 1.0
        elif k.endswith(".bias"):
            scale, off = 2.0 ** -8, 0.0
        elif "fc2" in k:
            scale, off = 2.0 ** -10, 0.0
        else:
            scale, off = 2.0 ** -9, 0.0
        out[k] = (q, scale, off)
    return out


def main():
    T = _ours()
    mg._stub("clip", "kornia", "kornia.augmentation")
    sys.path.insert(0, os.path.join(mg.REF, "SD"))
    modules = importlib.import_module("ldm.modules.encoders.modules")
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTokenizer

    vocab_json, merges_txt, nvocab = learn_vocab(T)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "vocab.json"), "w", encoding="utf-8").write(vocab_json)
        open(os.path.join(d, "merges.txt"), "w", encoding="utf-8").write(merges_txt)
        tok = CLIPTokenizer.from_pretrained(d)
    cfg = CLIPTextConfig(vocab_size=nvocab, bos_token_id=nvocab - 2, eos_token_id=nvocab - 1, pad_token_id=nvocab - 1, **CONFIG)
    model = CLIPTextModel(cfg).eval()
    sd = {k: v for k, v in model.state_dict().items() if not k.endswith("position_ids")}
    qw = quantized_weights({k: tuple(v.shape) for k, v in sd.items()})
    model.load_state_dict({k: qw[k][2] + qw[k][1] * qw[k][0].float() for k in sd}, strict=False)

    emb = modules.FrozenCLIPEmbedder.__new__(modules.FrozenCLIPEmbedder)
    torch.nn.Module.__init__(emb)
    emb.tokenizer, emb.transformer, emb.device, emb.max_length = tok, model, "cpu", 77
    emb.freeze()
    with torch.no_grad():
        hidden = emb.forward(PROMPTS)
    ids = tok(PROMPTS, truncation=True, max_length=77, return_length=True, return_overflowing_tokens=False, padding="max_length",
              return_tensors="pt")["input_ids"]

    out = dict(vocab_json=np.array(vocab_json), merges_txt=np.array(merges_txt), prompts=np.array(PROMPTS), ids=ids.numpy().astype(np.int64),
               hidden=hidden.numpy().astype(np.float32),
               config=np.array([nvocab, 77, CONFIG["hidden_size"], CONFIG["num_hidden_layers"], CONFIG["num_attention_heads"],
                                CONFIG["intermediate_size"]]))
    keys = sorted(qw)
    out["w_keys"] = np.array(keys)
    out["w_scale"] = np.array([qw[k][1] for k in keys], dtype=np.float32)
    out["w_offset"] = np.array([qw[k][2] for k in keys], dtype=np.float32)
    for i, k in enumerate(keys):
        out[f"w_q_{i}"] = qw[k][0].numpy()
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: vocab {nvocab}, ids {tuple(ids.shape)}, hidden {tuple(hidden.shape)} std {float(hidden.std()):.3f}, "
          f"{os.path.getsize(OUT) / 1024:.0f} KB")
    for p, row in zip(PROMPTS, ids.tolist()):
        n = row.index(nvocab - 1) + 1 if (nvocab - 1) in row else 77
        print(f"  {n:3d} tokens  {p[:60]!r}")


if __name__ == "__main__":
    main()
