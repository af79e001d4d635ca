"""CPU: the host side of the native DiT sampler (sfron.dit_sample, the DDIM API of sfron.diffusion.GaussianDiffusion).

The ABI surface of the two new entry points and their refusals (SFRON_ERR_ARG before any launch: no GPU is touched), the three new columns
of the sampler table against the reference's fp64 arrays (tests/golden/dit_sampler.npz), the bookkeeping of DiT/sample_ddp.py restated as
``fid_plan`` / ``sample_folder_name`` / ``create_npz_from_sample_folder``, and the byte rule of SFRON_IMAGE_TRUNC."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sfron_dit_sample_step", "sfron_dit_sampler_advance")


# ------------------------------------------------------------------------------------------------ ABI
def test_new_prototypes_in_header_and_binding_and_abi_stays_16():
    from sfron import _lib
    L = _lib.lib()
    assert L.sfron_abi_version() == 17 and _lib.ABI_VERSION == 17          # additive: the ABI version stays
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfron.h")).read(), flags=re.S)
    kinds = {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double, "int": ctypes.c_int}
    for name in NEW:
        assert getattr(L, name) is not None and name in _lib.declared_symbols()
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, f"{name} is not declared in include/sfron.h"
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib._PROTOS[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for at, p in zip(args, params):
            assert at is (ctypes.c_void_p if "*" in p else kinds[p.split()[0]]), (name, p, at)
    m = re.search(r"enum \{ SFRON_DIT_SAMPLE_DDPM = (\d+), SFRON_DIT_SAMPLE_DDIM = (\d+), SFRON_DIT_SAMPLE_DDIM_REVERSE = (\d+) \};", hdr)
    assert m and tuple(int(v) for v in m.groups()) == (_lib.DIT_SAMPLE_DDPM, _lib.DIT_SAMPLE_DDIM, _lib.DIT_SAMPLE_DDIM_REVERSE)
    from sfron import images
    m = re.search(r"enum \{ SFRON_IMAGE_TRUNC = (\d+) \};", hdr)
    assert m and int(m.group(1)) == images.IMAGE_TRUNC == images.image_mode("trunc") == 2
    assert images.image_mode("save_image") == 0 and images.image_mode("round") == 1
    with pytest.raises(ValueError):
        images.image_mode("floor")


# never dereferenced: every call below is refused before a launch.  Distinct 256-byte "buffers" inside one host allocation.
_HOST = (ctypes.c_char * 4096)()
_P = [ctypes.addressof(_HOST) + 256 * k for k in range(12)]


def _step_args(**kw):
    a = dict(x=_P[0], model_out=_P[1], t=_P[2], stab=_P[3], noise=_P[4], n=2, c=4, hw=8, guided=1, n_guided=3, cfg_scale=4.0, mode=0, eta=0.0,
             clip=0, sample=_P[5], dup=_P[6], pred=_P[7])
    a.update(kw)
    return [a[k] for k in ("x", "model_out", "t", "stab", "noise", "n", "c", "hw", "guided", "n_guided", "cfg_scale", "mode", "eta", "clip",
                           "sample", "dup", "pred")] + [None]


@pytest.mark.parametrize("bad", [
    dict(x=None), dict(model_out=None), dict(t=None), dict(stab=None), dict(sample=None),                 # a null required pointer
    dict(n=0), dict(c=0), dict(hw=-1),                                                                     # a non-positive extent
    dict(n_guided=-1), dict(n_guided=5),                                                                   # outside [0, C]
    dict(cfg_scale=float("nan")), dict(cfg_scale=float("inf")), dict(eta=float("nan")), dict(eta=float("-inf")),
    dict(mode=3), dict(mode=-1),                                                                           # an unknown mode
    dict(mode=0, noise=None), dict(mode=1, eta=0.5, noise=None),                                           # the mode needs a noise tensor
    dict(mode=2, eta=0.5),                                                                                 # the reverse ODE is eta == 0 only
    dict(pred=_P[0]), dict(pred=_P[5]), dict(dup=_P[0]), dict(dup=_P[5]), dict(pred=_P[6]),                # only sample may alias x
    dict(n=1 << 12, c=1 << 10, hw=1 << 9), dict(n=65536, c=1, hw=1),                                      # an int product / the grid
], ids=lambda b: ",".join(f"{k}={'P%d' % _P.index(v) if v in _P else v}" for k, v in b.items()))   # a buffer by its index: an address differs per run
def test_step_refusals_come_before_any_launch(bad):
    from sfron import _lib
    assert _lib.lib().sfron_dit_sample_step(*_step_args(**bad)) == _lib.ERR_ARG


def test_advance_refusals_come_before_any_launch():
    from sfron import _lib
    L = _lib.lib()
    good = dict(order=_P[0], tmap=_P[1], steps=5, map_len=5, step=_P[2], t_idx=_P[3], n=3, t_model=_P[4], rows=6)
    keys = list(good)
    for bad in (dict(order=None), dict(tmap=None), dict(step=None), dict(t_idx=None), dict(t_model=None), dict(steps=0), dict(map_len=0),
                dict(n=0), dict(rows=-2)):
        a = dict(good, **bad)
        assert L.sfron_dit_sampler_advance(*[a[k] for k in keys], None) == _lib.ERR_ARG, bad


def test_trunc_image_mode_refusals_are_those_of_the_other_modes():
    from sfron import _lib
    L = _lib.lib()
    assert L.sfron_rows_to_image_u8(None, 4, 1, 2, 2, 2, 0.0, 0.0, 0, 0, 0, 1, _P[1], None) == _lib.ERR_ARG
    assert L.sfron_rows_to_image_u8(_P[0], 4, 1, 2, 2, 3, -1.0, 1.0, 0, 0, 0, 1, _P[1], None) == _lib.ERR_ARG          # no mode 3


# ------------------------------------------------------------------------------------------------ the sampler table
def test_sampler_table_columns_are_the_reference_fp64_arrays_rounded_once(golden_dir):
    from sfron import diffusion
    g = np.load(os.path.join(golden_dir, "dit_sampler.npz"))
    d = diffusion.create_diffusion("10", device="cpu")
    np.testing.assert_array_equal(d.tables["alphas_cumprod_prev"], g["ac_prev10"])
    np.testing.assert_array_equal(d.tables["alphas_cumprod_next"], g["ac_next10"])
    stab = d.sampler_tab.numpy()
    assert stab.shape == (10, 11) and stab.dtype == np.float32
    assert d.tab.shape == (10, 8) and np.array_equal(stab[:, :8].view(np.uint32), d.tab.numpy().view(np.uint32))     # tab is not widened
    assert np.array_equal(stab[:, 8].view(np.uint32), d.tables["alphas_cumprod"].astype(np.float32).view(np.uint32))
    assert np.array_equal(stab[:, 9].view(np.uint32), g["ac_prev10"].astype(np.float32).view(np.uint32))
    assert np.array_equal(stab[:, 10].view(np.uint32), g["ac_next10"].astype(np.float32).view(np.uint32))
    assert stab[0, 9] == 1.0 and stab[-1, 10] == 0.0
    assert d.timestep_map == list(g["map_10"])
    assert diffusion.create_diffusion("ddim25", device="cpu").timestep_map == list(g["map_ddim25"])


def test_ddim_api_refuses_what_is_not_built():
    from sfron import diffusion
    d = diffusion.create_diffusion("10", device="cpu")
    x, t = torch.zeros(1, 4, 2, 2), torch.zeros(1, dtype=torch.int64)
    for fn in (d.ddim_sample, d.ddim_reverse_sample):
        with pytest.raises(NotImplementedError):
            fn(lambda *a, **k: None, x, t, denoised_fn=lambda v: v)
        with pytest.raises(NotImplementedError):
            fn(lambda *a, **k: None, x, t, cond_fn=lambda *a, **k: None)
    with pytest.raises(AssertionError):
        d.ddim_reverse_sample(lambda *a, **k: None, x, t, eta=0.5)


# ------------------------------------------------------------------------------------------------ sample_ddp.py bookkeeping
@pytest.mark.parametrize("num,n,world", [(50_000, 32, 8), (10, 4, 3), (7, 2, 1)])
def test_fid_plan_covers_every_file_index_once(num, n, world):
    import math
    from sfron import dit_sample
    seen = []
    for rank in range(world):
        p = dit_sample.fid_plan(num, n, world, rank)
        assert p["total_samples"] == int(math.ceil(num / (n * world)) * (n * world)) >= num          # the reference's ceil
        assert p["iterations"] * n * world == p["total_samples"] and p["global_batch"] == n * world
        seen += [p["index"](i, j) for j in range(p["iterations"]) for i in range(n)]
    assert sorted(seen) == list(range(p["total_samples"]))


def test_fid_plan_keeps_the_divisibility_asserts_and_refuses_bad_shapes(monkeypatch):
    import math
    from sfron import dit_sample
    for bad in ((10, 0, 1, 0), (10, 4, 0, 0), (10, 4, 2, 2), (10, 4, 2, -1), (0, 4, 1, 0)):
        with pytest.raises((ValueError, AssertionError)):
            dit_sample.fid_plan(*bad)
    # the two asserts of sample_ddp.py:101-103 hold by construction of the ceil; they are there, and fire, when that construction breaks
    monkeypatch.setattr(dit_sample.math, "ceil", lambda v: math.floor(v) + 0.5)
    with pytest.raises(AssertionError, match="divisible"):
        dit_sample.fid_plan(10, 3, 2, 0)


def test_sample_folder_name_is_the_reference_string():
    from sfron import dit_sample
    assert dit_sample.sample_folder_name("DiT-XL/2", None, 256, "ema", 1.5, 0) == "DiT-XL-2-pretrained-size-256-vae-ema-cfg-1.5-seed-0"
    assert (dit_sample.sample_folder_name("DiT-B/4", "/data/runs/003/0050000.pt", 512, "mse", 4.0, 7)
            == "DiT-B-4-0050000-size-512-vae-mse-cfg-4.0-seed-7")


def test_create_npz_from_sample_folder(tmp_path):
    from sfron import dit_sample, images
    rng = np.random.default_rng(3)
    imgs = rng.integers(0, 256, size=(7, 4, 4, 3), dtype=np.uint8)
    d = str(tmp_path / "samples")
    for i, im in enumerate(imgs):
        images.write_png(torch.from_numpy(im), os.path.join(d, f"{i:06d}.png"))
    path = dit_sample.create_npz_from_sample_folder(d, 6)                   # the first six of seven files
    assert path == d + ".npz"
    arr = np.load(path)["arr_0"]
    assert arr.shape == (6, 4, 4, 3) and arr.dtype == np.uint8 and np.array_equal(arr, imgs[:6])


# ------------------------------------------------------------------------------------------------ the TRUNC byte rule
def trunc_u8_f64(x):
    """sample_ddp.py:132 in float64: clamp(127.5 x + 128, 0, 255) truncated.  For fp32 inputs whose fp32 product and sum are exact or do
    not cross an integer -- every value the tests use -- the fp32 kernel gives the same byte."""
    return np.floor(np.clip(127.5 * np.asarray(x, dtype=np.float64) + 128.0, 0.0, 255.0)).astype(np.uint8)


def test_trunc_byte_rule_at_the_edges():
    x = np.array([-1.004, -1.0, -0.5 / 127.5, 0.0, 1.0 - 1.0 / 255.0, 1.0, 1.01], dtype=np.float32)
    # 127.5 x + 128: -0.01 -> 0 (clamped); 0.5 -> 0; 127.5 -> 127 (no rounding up); 128 -> 128; 255 -> 255; 255.5, 256.8 -> 255 (clamped)
    assert trunc_u8_f64(x).tolist() == [0, 0, 127, 128, 255, 255, 255]
    assert trunc_u8_f64(np.float32(1.0 - 1.5 / 255.0)).item() == 254 and trunc_u8_f64(np.float32(-1.0 + 1.0 / 64.0)).item() == 2
    # truncation, not rounding: one level below SFRON_IMAGE_ROUND's byte wherever the fraction is >= 0.5
    assert trunc_u8_f64(np.float32(0.5)).item() == 191 and trunc_u8_f64(np.float32(-0.5)).item() == 64
