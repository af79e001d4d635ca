"""CPU: the CLIP text encoder's host side -- tokenizer, weight namings, the canonical arena, an fp32 restatement, the C ABI -- against
tests/golden/text_encoder.npz (made by tests/golden/make_text_encoder_golden.py from the reference FrozenCLIPEmbedder over a synthetic
vocabulary and a small seeded CLIPTextModel).  ``clip_fp32`` here is a plain-torch restatement of the transformer over canonical names;
the GPU tests use it as their fp32 yardstick."""
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tfx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "text_encoder.npz")))


def fixture_weights(tfx):
    """HF CLIPTextModel state dict (text_model.* names) of the fixture: offset + scale * int8, exactly the reference's fp32 weights."""
    return {"text_model." + str(k) if not str(k).startswith("text_model.") else str(k): float(tfx["w_offset"][i]) + float(tfx["w_scale"][i]) * torch.from_numpy(tfx[f"w_q_{i}"]).float()
            for i, k in enumerate(tfx["w_keys"])}


def fixture_config(tfx):
    v, p, d, n, h, f = (int(x) for x in tfx["config"])
    return dict(vocab_size=v, max_position=p, width=d, layers=n, mlp=f), h


def fixture_tokenizer(tfx, tmp_dir):
    from sfron import text
    with open(os.path.join(tmp_dir, "vocab.json"), "w", encoding="utf-8") as f:
        f.write(str(tfx["vocab_json"]))
    with open(os.path.join(tmp_dir, "merges.txt"), "w", encoding="utf-8") as f:
        f.write(str(tfx["merges_txt"]))
    return text.CLIPTokenizer.from_pretrained(tmp_dir)


def clip_fp32(canon, ids, layers, heads, eps=1e-5):
    """fp32 restatement of CLIPTextModel.last_hidden_state over a canonical state dict (q / k / v concatenated): pre-LN layers,
    causal softmax attention, quick_gelu MLP, final LayerNorm.  ids int64 [B, T]."""
    F = torch.nn.functional
    ids = torch.as_tensor(ids)
    B, T = ids.shape
    x = canon["embeddings.token_embedding.weight"][ids] + canon["embeddings.position_embedding.weight"][:T]
    D = x.shape[-1]
    hd = D // heads
    mask = torch.full((T, T), float("-inf"), dtype=x.dtype, device=x.device).triu(1)
    for i in range(layers):
        L = f"encoder.layers.{i}."
        h = F.layer_norm(x, (D,), canon[L + "layer_norm1.weight"], canon[L + "layer_norm1.bias"], eps)
        qkv = h @ canon[L + "self_attn.qkv_proj.weight"].T + canon[L + "self_attn.qkv_proj.bias"]
        q, k, v = (t.reshape(B, T, heads, hd).transpose(1, 2) for t in qkv.split(D, -1))
        a = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5 + mask, -1) @ v
        x = x + a.transpose(1, 2).reshape(B, T, D) @ canon[L + "self_attn.out_proj.weight"].T + canon[L + "self_attn.out_proj.bias"]
        h = F.layer_norm(x, (D,), canon[L + "layer_norm2.weight"], canon[L + "layer_norm2.bias"], eps)
        h = h @ canon[L + "mlp.fc1.weight"].T + canon[L + "mlp.fc1.bias"]
        h = h * torch.sigmoid(1.702 * h)
        x = x + h @ canon[L + "mlp.fc2.weight"].T + canon[L + "mlp.fc2.bias"]
    return F.layer_norm(x, (D,), canon["final_layer_norm.weight"], canon["final_layer_norm.bias"], eps)


# ------------------------------------------------------------------------------------------------ tokenizer
def test_tokenizer_matches_reference_ids(tfx, tmp_path):
    tok = fixture_tokenizer(tfx, str(tmp_path))
    prompts = [str(p) for p in tfx["prompts"]]
    got = tok(prompts).numpy()
    assert got.dtype == np.int64 and got.shape == tfx["ids"].shape == (len(prompts), 77)
    for i, p in enumerate(prompts):
        assert np.array_equal(got[i], tfx["ids"][i]), (p, got[i][:24], tfx["ids"][i][:24])
    # the call semantics the fixture pins: BOS first, EOS after the text, pad (= EOS) after that, truncation keeps BOS + 75 + EOS
    assert (got[:, 0] == tok.bos_id).all()
    assert list(got[prompts.index("")][:3]) == [tok.bos_id, tok.eos_id, tok.pad_id]
    long_row = got[-1]
    assert long_row[-1] == tok.eos_id and tok.eos_id not in long_row[1:76]
    lit = got[prompts.index("a photo <|endoftext|> of a dog")]
    assert tok.eos_id in lit[1:6]                         # the literal special token is one id, not its characters
    assert np.array_equal(tok(prompts[0]).numpy(), got[:1])


def test_pretokenizer_classes():
    from sfron import text
    assert text.pretokenize(text.normalize("Don't  STOP!!1990s ÉTÉ")) == ["don", "'t", "stop", "!!", "1", "9", "9", "0", "s", "été"]
    assert text.normalize("a \t\n b") == "a b"


# ------------------------------------------------------------------------------------------------ weight namings
def _namings(w):
    hf = dict(w)
    hf["text_model.embeddings.position_ids"] = torch.arange(77)[None]
    compvis = {"cond_stage_model.transformer." + k: v for k, v in hf.items()}
    compvis["model.diffusion_model.out.0.weight"] = torch.zeros(3)             # other parts of an LDM checkpoint are ignored
    old = {"cond_stage_model.transformer." + k[len("text_model."):]: v for k, v in hf.items()}
    bare = {k[len("text_model."):]: v for k, v in hf.items()}                 # CLIPTextModel.state_dict() of recent transformers
    return hf, {"state_dict": compvis}, old, bare


def test_weight_namings_give_one_arena(tfx):
    from sfron import text
    cfg, _ = fixture_config(tfx)
    specs, n_mat = text.param_specs(**cfg)
    w = fixture_weights(tfx)
    arenas = []
    for sd in _namings(w):
        assert text.config_from_state_dict(sd) == cfg
        canon = text.canonical_state_dict(sd, specs)
        assert list(canon) == list(specs)
        arenas.append(text.pack_arena(canon, specs))
    assert all(torch.equal(arenas[0], a) for a in arenas[1:])
    index, total = text.arena_offsets(specs)
    assert total == arenas[0].numel() and all(off % 8 == 0 for off in index.values())
    # q rows first, then k, then v -- the column order sfron_attn_causal_fwd reads (which * D + head * 64 + d)
    D = cfg["width"]
    for i in range(cfg["layers"]):
        L = f"encoder.layers.{i}.self_attn."
        qkv = arenas[0][index[L + "qkv_proj.weight"]:][:3 * D * D].view(3 * D, D)
        bqkv = arenas[0][index[L + "qkv_proj.bias"]:][:3 * D]
        for j, nm in enumerate(("q_proj", "k_proj", "v_proj")):
            assert torch.equal(qkv[j * D:(j + 1) * D], w[f"text_model.{L}{nm}.weight"])
            assert torch.equal(bqkv[j * D:(j + 1) * D], w[f"text_model.{L}{nm}.bias"])
    # the matrices are the arena's prefix (the bf16 shadow copies exactly that region)
    names = list(specs)
    assert all(".weight" in n and len(specs[n]) == 2 for n in names[:n_mat])
    assert max(index[n] for n in names[:n_mat]) < index[names[n_mat]]


def test_missing_and_misshaped_keys_are_refused(tfx):
    from sfron import text
    cfg, _ = fixture_config(tfx)
    specs, _ = text.param_specs(**cfg)
    w = fixture_weights(tfx)
    bad = dict(w)
    del bad["text_model.encoder.layers.1.self_attn.k_proj.weight"]
    with pytest.raises(KeyError):
        text.canonical_state_dict(bad, specs)
    bad = dict(w)
    bad["text_model.encoder.layers.0.mlp.fc1.bias"] = torch.zeros(7)
    with pytest.raises(ValueError):
        text.canonical_state_dict(bad, specs)
    bad = dict(w)
    bad["text_model.encoder.layers.0.mlp.fc3.weight"] = torch.zeros(1)
    with pytest.raises(KeyError):
        text.canonical_state_dict(bad, specs)
    with pytest.raises(KeyError):
        text.canonical_state_dict({"first_stage_model.encoder.conv_in.weight": torch.zeros(1)}, specs)


# ------------------------------------------------------------------------------------------------ the transformer, restated
def test_fp32_restatement_reproduces_reference(tfx):
    from sfron import text
    cfg, heads = fixture_config(tfx)
    specs, _ = text.param_specs(**cfg)
    canon = text.canonical_state_dict(fixture_weights(tfx), specs)
    got = clip_fp32(canon, torch.from_numpy(tfx["ids"]), cfg["layers"], heads)
    want = torch.from_numpy(tfx["hidden"])
    err = (got - want).abs().max().item()
    assert err < 1e-4, err        # measured 2e-6 (fp32 against fp32; different summation order)


def test_flop_count():
    from sfron import text
    f = text.encoder_flops()
    assert 12.5e9 < f < 13.5e9, f          # ~13 GFLOP per prompt at ViT-L/14


# ------------------------------------------------------------------------------------------------ C ABI and bindings
def test_header_and_bindings_declare_the_entry_points():
    from sfron import _lib
    hdr = open(os.path.join(ROOT, "include", "sfron.h")).read()
    for name in ("sfron_clip_embed", "sfron_attn_causal_fwd", "sfron_layernorm_fwd_f32"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _lib.declared_symbols(), name
    m = re.search(r"SFRON_EPI_QUICK_GELU = (\d+)", hdr)
    assert m and int(m.group(1)) == _lib.EPI_QUICK_GELU == 9
    assert _lib.ABI_VERSION == 17


# ------------------------------------------------------------------------------------------------ LatentDiffusion.get_learned_conditioning
def test_get_learned_conditioning_delegates_or_raises():
    from sfron import sd
    unet = types.SimpleNamespace(device_=torch.device("cpu"))
    sched = types.SimpleNamespace(num_timesteps=1000)
    bare = sd.LatentDiffusion(unet, schedule=sched)
    with pytest.raises(NotImplementedError):
        bare.get_learned_conditioning(["a photo of a person"])

    class _Enc:
        def encode(self, c):
            return ("encoded", tuple(c))

    ld = sd.LatentDiffusion(unet, schedule=sched, cond_stage_model=_Enc())
    assert ld.get_learned_conditioning(["a", "b"]) == ("encoded", ("a", "b"))
    for f in (ld.get_input, ld.shared_step, ld.encode_first_stage):
        with pytest.raises(NotImplementedError):
            f({}, "jpg")
