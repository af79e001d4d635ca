"""CPU: the host side of the ldm DDIM sampler (sfron.ddim) and the prompt-to-image driver (sfron.sd.generate_images).

ABI surface of sfron_xattn_fwd / sfron_ddim_cfg_step (header <-> ctypes), the schedule tables against the reference's
(tests/golden/ddim.npz, made by tests/golden/make_ddim_golden.py: bit for bit after rounding to fp32, the dtypes the reference ends up
with included), the NotImplementedError guards, and the CSV driver's file naming / seed handling with the sampler mocked."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "ddim.npz"))


def host_model():
    """what DDIMSampler reads of LatentDiffusion, on the CPU (the fp32 tables of sd.LDMSchedule)"""
    from sfron import sd
    s = sd.LDMSchedule(device="cpu")
    return types.SimpleNamespace(num_timesteps=s.num_timesteps, betas=s.betas, alphas_cumprod=s.alphas_cumprod,
                                 alphas_cumprod_prev=s.alphas_cumprod_prev, device=torch.device("cpu"))


def test_new_symbols_header_and_ctypes_agree():
    from sfron import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfron.h")).read(), flags=re.S)
    for name in ("sfron_xattn_fwd", "sfron_ddim_cfg_step"):
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, f"{name} is not declared in include/sfron.h"
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib._PROTOS[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for at, p in zip(args, params):
            if "*" in p:
                assert at is ctypes.c_void_p, (name, p, at)
            else:
                assert at is {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}[p.split()[0]], (name, p, at)
    assert _lib.ABI_VERSION == 17          # additive: the ABI version stays


def test_schedule_tables_equal_the_reference(G):
    from sfron import ddim
    names = sorted({k.split("/")[1] for k in G.files if k.startswith("sched/")})
    assert names == ["10_0.5_uniform", "12_0.0_quad", "50_0.0_uniform", "7_1.0_uniform"]
    for name in names:
        S, eta, discr = name.split("_")
        s = ddim.DDIMSampler(host_model())
        s.make_schedule(int(S), ddim_discretize=discr, ddim_eta=float(eta), verbose=False)
        pre = f"sched/{name}/"
        assert s.ddim_timesteps.dtype == G[pre + "timesteps"].dtype and np.array_equal(s.ddim_timesteps, G[pre + "timesteps"])
        for key, got in (("alphas", s.ddim_alphas), ("alphas_prev", s.ddim_alphas_prev), ("sigmas", s.ddim_sigmas),
                         ("sqrt_one_minus_alphas", s.ddim_sqrt_one_minus_alphas)):
            got = got.numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
            want = G[pre + key]
            assert got.dtype == want.dtype, (name, key, got.dtype, want.dtype)
            assert np.array_equal(got.astype(np.float32), want.astype(np.float32)), (name, key)
    # the +1 shift and alphas_prev[0] = alphas_cumprod[0]
    s = ddim.DDIMSampler(host_model())
    s.make_schedule(50)
    assert s.ddim_timesteps[0] == 1 and s.ddim_timesteps[-1] == 981
    assert np.float32(s.ddim_alphas_prev[0]) == s.model.alphas_cumprod[0].numpy()


def test_unbuilt_arguments_raise_naming_the_argument():
    from sfron import ddim
    s = ddim.DDIMSampler(host_model())
    base = dict(S=4, batch_size=1, shape=(4, 8, 8), conditioning=torch.zeros(1, 5, 24))
    one = torch.ones(1, 4, 8, 8)
    for kw, word in ((dict(mask=one), "mask"), (dict(x0=one), "x0"), (dict(score_corrector=object()), "score_corrector"),
                     (dict(quantize_x0=True), "quantize_x0"), (dict(dynamic_threshold=0.5), "dynamic_threshold"),
                     (dict(noise_dropout=0.1), "noise_dropout"), (dict(ddim_use_original_steps=True), "ddim_use_original_steps")):
        with pytest.raises(NotImplementedError, match=word):
            s.sample(**base, **kw)
    with pytest.raises(NotImplementedError, match="encode"):
        s.encode(one, None, 3)
    s.make_schedule(4)
    with pytest.raises(NotImplementedError, match="use_original_steps"):
        s.p_sample_ddim(one, torch.zeros(1, 5, 24), torch.zeros(1, dtype=torch.long), 0, use_original_steps=True)
    with pytest.raises(NotImplementedError, match="use_original_steps"):
        s.decode(one, None, 2, use_original_steps=True)
    with pytest.raises(NotImplementedError):
        ddim.make_ddim_timesteps("cosine", 10, 1000)


def test_sampler_refuses_cpu_model_outputs():
    """no CPU fall-back of the update: a model that answers on the CPU is an error, not an eager step"""
    from sfron import _lib, ddim
    m = host_model()
    m.apply_model = lambda x, t, c: x
    with pytest.raises(_lib.SfronError):
        ddim.DDIMSampler(m).sample(S=4, batch_size=1, shape=(4, 8, 8), conditioning=torch.zeros(1, 5, 24), x_T=torch.zeros(1, 4, 8, 8))


def test_chunked_runs_slice_their_operands():
    """the DDIM twin of test_plms_cpu's test of the same name: both samplers run their chunks through one driver"""
    from sfron import ddim
    s = ddim.DDIMSampler(host_model())
    s.chunk_size = lambda batch_size, shape: 2
    B = 5
    g = torch.Generator().manual_seed(1)
    x_T, cond, uc = torch.randn(B, 4, 8, 8, generator=g), torch.randn(B, 5, 24, generator=g), torch.randn(B, 5, 24, generator=g)
    noise = torch.randn(4, B, 4, 8, 8, generator=g)
    seen = []

    def ddim_sampling(cond, shape, **kw):
        seen.append(dict(cond=cond, shape=shape, **kw))
        return kw["x_T"] + 1, {"x_inter": [kw["x_T"], kw["x_T"] + 1], "pred_x0": [kw["x_T"], kw["x_T"] - 1]}
    s.ddim_sampling = ddim_sampling
    smp, inter = s.sample(S=4, batch_size=B, shape=(4, 8, 8), conditioning=cond, unconditional_conditioning=uc, x_T=x_T, eta=0.5,
                          step_noise=noise, unconditional_guidance_scale=2.0, log_every_t=1, temperature=0.7, t_start=3, till_T=1,
                          verbose=False)
    assert len(s.ddim_timesteps) == 4 and np.all(np.asarray(s.ddim_sigmas, dtype=np.float64)[1:] > 0)          # an eta > 0 schedule
    assert [c["shape"] for c in seen] == [(2, 4, 8, 8), (2, 4, 8, 8), (1, 4, 8, 8)]
    for c, (lo, hi) in zip(seen, ((0, 2), (2, 4), (4, 5))):
        assert torch.equal(c["cond"], cond[lo:hi]) and torch.equal(c["unconditional_conditioning"], uc[lo:hi])
        assert torch.equal(c["x_T"], x_T[lo:hi])
        for k in range(4):
            assert torch.equal(c["step_noise"][k], noise[k][lo:hi])
        assert c["t_start"] == 3 and c["till_T"] == 1 and c["temperature"] == 0.7 and c["log_every_t"] == 1
        assert c["unconditional_guidance_scale"] == 2.0
    assert torch.equal(smp, x_T + 1)
    assert len(inter["x_inter"]) == len(inter["pred_x0"]) == 2
    assert torch.equal(inter["x_inter"][0], x_T) and torch.equal(inter["x_inter"][1], x_T + 1)
    assert torch.equal(inter["pred_x0"][0], x_T) and torch.equal(inter["pred_x0"][1], x_T - 1)
    # nothing is sliced that is not there
    seen.clear()
    s.sample(S=4, batch_size=B, shape=(4, 8, 8), conditioning=cond, x_T=x_T, verbose=False)
    assert len(seen) == 3 and all(c["step_noise"] is None and c["unconditional_conditioning"] is None for c in seen)


def test_generate_images_file_names_and_seeds(tmp_path, monkeypatch):
    from sfron import sd
    csv_path = tmp_path / "prompts.csv"
    csv_path.write_text('case_number,prompt,evaluation_seed,extra\n3,"a cat, sitting",11,x\n7,a dog,12,y\n9,a bird,13,z\n')
    seen = []

    class Sampler:
        def sample(self, S, conditioning, batch_size, shape, x_T, unconditional_guidance_scale, unconditional_conditioning, eta, **kw):
            seen.append(dict(S=S, c=conditioning, B=batch_size, shape=tuple(shape), x_T=x_T.clone(), g=unconditional_guidance_scale,
                             uc=unconditional_conditioning, eta=eta, kw=kw))
            return x_T, {}

    prompts = []

    def cond(p):
        prompts.append(list(p))
        return torch.zeros(len(p), 77, 8)
    model = types.SimpleNamespace(device=torch.device("cpu"), get_learned_conditioning=cond)
    monkeypatch.setattr(sd, "decode_images_u8", lambda model, z: torch.zeros(z.shape[0], 16, 16, 3, dtype=torch.uint8))
    out = sd.generate_images(model, str(csv_path), str(tmp_path / "out"), guidance_scale=7.5, image_size=16, ddim_steps=5, num_samples=2,
                             from_case=5, rounds=3, sampler=Sampler())
    want = [f"{case}_{i * 10 + k}.png" for case in (7, 9) for i in range(3) for k in range(2)]
    assert [os.path.basename(p) for p in out] == want
    assert sorted(os.listdir(tmp_path / "out")) == sorted(want)
    from PIL import Image
    assert Image.open(out[0]).size == (16, 16)
    # seeds: torch.manual_seed(seed) once per row, then one CPU draw per round from that generator
    assert len(seen) == 6
    for r, seed in enumerate((12, 13)):
        g = torch.manual_seed(seed)
        for i in range(3):
            call = seen[3 * r + i]
            assert torch.equal(call["x_T"], torch.randn((2, 4, 2, 2), generator=g))
            assert call["S"] == 5 and call["B"] == 2 and call["shape"] == (4, 2, 2) and call["g"] == 7.5 and call["eta"] == 0.0
            assert call["uc"].shape == (2, 77, 8) and call["kw"]["t_start"] == -1
    assert ["a dog"] * 2 in prompts and [""] * 2 in prompts and ["a cat, sitting"] * 2 not in prompts


def test_sample_model_returns_intermediates_only_when_asked():
    from sfron import sd

    class Sampler:
        def sample(self, **kw):
            self.kw = kw
            return "z", "inter"
    model = types.SimpleNamespace(get_learned_conditioning=lambda p: ("uc", len(p)))
    s = Sampler()
    assert sd.sample_model(model, s, "c", 64, 32, 7, 1.0, 0.5) == "z"
    assert s.kw["unconditional_conditioning"] is None and s.kw["shape"] == [4, 8, 4] and s.kw["log_every_t"] == 100 and s.kw["eta"] == 0.5
    assert sd.sample_model(model, s, "c", 64, 64, 7, 3.0, 0.0, n_samples=3, log_every_t=2, t_start=5, till_T=1) == ("z", "inter")
    assert s.kw["unconditional_conditioning"] == ("uc", 3) and s.kw["log_every_t"] == 2 and s.kw["t_start"] == 5 and s.kw["till_T"] == 1
