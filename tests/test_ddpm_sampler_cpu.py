"""CPU: the host side of the DDPM guided sampler (sfron.ddpm.DDPMSampler) and of the runner's sample modes (sfron.ddpm_sample).

create_class_labels against the reference's answers (tests/golden/ddpm_sample.npz); the timestep sequences of
Diffusion.sample_image (DDPM/runners/diffusion.py:831-842); the coefficient table against DDPM/functions/denoising.py:85-92 written out
here in torch's fp32 0-dim tensor math; the n_rounds / n_left / img_id / directory bookkeeping of the per-image modes and the chunking
of sample_visualization over a stub sampler and recording writers (no GPU: the drivers take the writer as an argument); the ABI
surface of the three new entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sfron_ddpm_guided_step", "sfron_ddpm_sampler_advance", "sfron_images_normalize_u8")


def test_create_class_labels_matches_the_reference(golden_dir):
    from sfron import ddpm_sample
    g = np.load(os.path.join(golden_dir, "ddpm_sample.npz"))
    assert list(g["strings"]) == ["x0", "0", "1,3,5", "x2,x7"]
    for k, s in enumerate(g["strings"]):
        classes, excluded = ddpm_sample.create_class_labels(str(s), n_classes=int(g["n_classes"]))
        assert classes == list(g[f"classes_{k}"]) and excluded == list(g[f"excluded_{k}"]), s
        assert all(type(v) is int for v in classes + excluded)


def test_uniform_sequence_keeps_the_reference_length():
    from sfron import ddpm
    assert ddpm.sampling_sequence("uniform", 1000, 1000) == list(range(1000))
    assert ddpm.sampling_sequence("uniform", 1000, 100) == list(range(0, 1000, 10))
    s6 = ddpm.sampling_sequence("uniform", 1000, 6)                 # skip = 1000 // 6 = 166: SEVEN entries
    assert s6 == [0, 166, 332, 498, 664, 830, 996] and len(s6) == 7
    with pytest.raises(NotImplementedError):
        ddpm.sampling_sequence("linear", 1000, 10)


def test_quad_sequence():
    from sfron import ddpm
    for n in (10, 1000):
        want = [int(s) for s in list(np.linspace(0, np.sqrt(1000 * 0.8), n) ** 2)]
        got = ddpm.sampling_sequence("quad", 1000, n)
        assert got == want and len(got) == n and got[0] == 0 and got[-1] in (799, 800)
        assert all(type(v) is int for v in got)
    assert ddpm.sampling_sequence("quad", 1000, 10)[:4] == [0, 9, 39, 88]          # (k sqrt(800) / 9)^2 floored


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_coefficient_table_is_the_reference_arithmetic(eta):
    """denoising.py:81-92 with compute_alpha's table (alpha_bar(-1) = 1 in front): every row of the table, the last step (j = -1)
    included, equals the fp32 0-dim tensor expressions of the reference, value for value."""
    from sfron import ddpm
    b = torch.from_numpy(np.linspace(1e-4, 2e-2, 1000, dtype=np.float64)).float()
    abar = torch.cat([torch.ones(1), (1 - b).cumprod(0)])
    seq = ddpm.sampling_sequence("uniform", 1000, 6)
    rows, ts = ddpm.generalized_coefficients(abar, seq, eta)
    assert ts == seq[::-1] and len(rows) == 7
    seq_next = [-1] + seq[:-1]
    for row, i, j in zip(rows, reversed(seq), reversed(seq_next)):
        at, at_next = abar[i + 1], abar[j + 1]
        c1 = eta * ((1 - at / at_next) * (1 - at_next) / (1 - at)).sqrt()
        c2 = ((1 - at_next) - c1 ** 2).sqrt()
        want = (float((1 - at).sqrt()), float(at.sqrt()), float(at_next.sqrt()), float(c1), float(c2))
        assert row == want, (i, j)
        assert row == ddpm.generalized_row(abar, i, j, eta)            # what generalized_steps_conditional hands sfron_ddim_step
        assert all(np.float32(v) == v for v in row)                    # fp32 values: the device table holds them exactly
    assert rows[-1][2:] == (1.0, 0.0, 0.0)                             # j = -1: alpha_bar_next = 1, so x_next = x0 whatever eta
    assert all((r[3] == 0.0) == (eta == 0.0) for r in rows[:-1])


def test_a_zero_divisor_row_is_refused_on_the_host():
    from sfron import _lib, ddpm
    abar = torch.tensor([1.0, 0.5, 0.0])
    with pytest.raises(_lib.SfronError):
        ddpm.generalized_coefficients(abar, [0, 1], 0.0)


def test_ddpm_noisy_raises_and_names_the_survey_entry():
    from sfron import ddpm
    with pytest.raises(NotImplementedError, match="Q16"):
        ddpm.DDPMSampler(None, None, sample_type="ddpm_noisy")
    with pytest.raises(NotImplementedError):
        ddpm.DDPMSampler(None, None, sample_type="ancestral")


# ------------------------------------------------------------------------------------------------ drivers over a stub sampler
class _StubSampler:
    def __init__(self):
        self.calls = []

    def sample_image(self, x, c, cond_scale, last=True):
        self.calls.append((tuple(x.shape), c.tolist(), cond_scale))
        return x * 0.1 + c.view(-1, 1, 1, 1).float()


def _config(batch, vis=20, n_classes=10):
    from types import SimpleNamespace as NS
    return NS(data=NS(channels=3, image_size=4, n_classes=n_classes, rescaled=True, logit_transform=False),
              sampling=NS(batch_size=batch), training=NS(visualization_samples=vis))


class _Recorder:
    def __init__(self):
        self.paths, self.batches = [], []

    def __call__(self, x, paths):
        assert x.shape[0] == len(paths) and float(x.min()) >= 0.0 and float(x.max()) <= 1.0          # inverse_data_transform-ed
        self.paths += list(paths)
        self.batches.append(x.shape[0])


def test_sample_fid_bookkeeping(tmp_path):
    from sfron import ddpm_sample
    s, rec = _StubSampler(), _Recorder()
    d = ddpm_sample.sample_fid(s, _config(4), str(tmp_path), 2.0, "x0,x1,x2,x3,x4,x5,x6", 7, device="cpu", save=rec)
    assert d == os.path.join(str(tmp_path), "fid_samples_guidance_2.0_excluded_class_0_1_2_3_4_5_6") and os.path.isdir(d)
    assert rec.batches == [4, 3] * 3                                     # n_rounds = 7 // 4 + 1, n_left 7 -> 3
    assert rec.paths == [os.path.join(d, f"{k}.png") for k in range(21)]  # one img_id across the classes
    assert [c[1] for c in s.calls] == [[7] * 4, [7] * 3, [8] * 4, [8] * 3, [9] * 4, [9] * 3] and all(c[2] == 2.0 for c in s.calls)
    assert s.calls[0][0] == (4, 3, 4, 4)
    rec2 = _Recorder()
    d2 = ddpm_sample.sample_fid(s, _config(4), str(tmp_path), -1, "1,4", 8, device="cpu", save=rec2)
    assert os.path.basename(d2) == "fid_samples_guidance_-1" and rec2.batches == [4, 4, 4, 4] and len(rec2.paths) == 16


def test_sample_classes_bookkeeping(tmp_path):
    from sfron import ddpm_sample
    s, rec = _StubSampler(), _Recorder()
    d = ddpm_sample.sample_classes(s, _config(2), str(tmp_path), 2.0, "1,4", 3, device="cpu", save=rec)
    assert d == os.path.join(str(tmp_path), "class_samples") and os.path.isdir(os.path.join(d, "1")) and os.path.isdir(os.path.join(d, "4"))
    assert rec.batches == [2, 1, 2, 1]
    assert rec.paths == [os.path.join(d, "1", f"{k}.png") for k in range(3)] + [os.path.join(d, "4", f"{k}.png") for k in range(3, 6)]


def test_sample_one_class_bookkeeping(tmp_path):
    from sfron import ddpm_sample
    s, rec = _StubSampler(), _Recorder()
    d = ddpm_sample.sample_one_class(s, _config(128), str(tmp_path), 0.0, 3, device="cpu", save=rec)
    assert d == os.path.join(str(tmp_path), "class_3")
    assert rec.batches == [128, 128, 128, 116] and len(rec.paths) == 500                # 500 samples, the short last round
    assert rec.paths[0] == os.path.join(d, "0.png") and rec.paths[-1] == os.path.join(d, "499.png")
    assert all(c[1] == [3] * c[0][0] for c in s.calls)


@pytest.mark.parametrize("batch,rounds", [(8, [10, 10]), (20, [20]), (64, [20])])
def test_sample_visualization_chunking(tmp_path, batch, rounds):
    """n_rounds = total // batch for batch < total, else 1; labels repeat_interleave-d and torch.chunk-ed; ONE sheet, nrow = samples per
    class, padding 0, normalised over the whole batch."""
    from sfron import ddpm_sample
    s, seen = _StubSampler(), {}

    def grid(x, path, **kw):
        seen.update(x=x, path=path, kw=kw)
    p = ddpm_sample.sample_visualization(s, _config(batch, vis=20), "2.0", 2.0, str(tmp_path), device="cpu", save_grid=grid)
    assert p == seen["path"] == os.path.join(str(tmp_path), "sample-2.0.png")
    assert seen["kw"] == dict(nrow=2, padding=0, normalize=True) and seen["x"].shape == (20, 3, 4, 4)
    assert [c[0][0] for c in s.calls] == rounds
    assert sum((c[1] for c in s.calls), []) == [k // 2 for k in range(20)]


def test_inverse_data_transform_branches():
    from types import SimpleNamespace as NS
    from sfron import ddpm_sample
    x = torch.tensor([-3.0, -1.0, 0.0, 0.5, 2.0]).view(1, 1, 1, 5)
    cfg = NS(data=NS(rescaled=True, logit_transform=False))
    assert torch.equal(ddpm_sample.inverse_data_transform(cfg, x), torch.clamp((x + 1.0) / 2.0, 0.0, 1.0))
    cfg = NS(data=NS(rescaled=True, logit_transform=True))               # logit wins over rescaled
    assert torch.equal(ddpm_sample.inverse_data_transform(cfg, x), torch.sigmoid(x))
    cfg = NS(data=NS(rescaled=False, logit_transform=False), image_mean=torch.full((1, 1, 5), 0.25))
    assert torch.equal(ddpm_sample.inverse_data_transform(cfg, x), torch.clamp(x + 0.25, 0.0, 1.0))


# ------------------------------------------------------------------------------------------------ ABI
def test_new_prototypes_in_header_and_binding_and_abi_stays_16():
    from sfron import _lib
    L = _lib.lib()
    assert L.sfron_abi_version() == 17 and _lib.ABI_VERSION == 17          # additive: the ABI version stays
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfron.h")).read(), flags=re.S)
    kinds = {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double, "int": ctypes.c_int}
    for name in NEW:
        assert getattr(L, name) is not None
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, f"{name} is not declared in include/sfron.h"
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib._PROTOS[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for at, p in zip(args, params):
            assert at is (ctypes.c_void_p if "*" in p else kinds[p.split()[0]]), (name, p, at)
