"""sfron.fid end to end on the GPU: two folders of tiny PNGs (12 and 9 files) and the same bytes as ``.npz`` files, at feature 64 and 192 --
9 and 12 samples against 64 and 192 dimensions, so every covariance is rank deficient on purpose -- against ``FIDStatistics`` of the features
of the bf16-operand emulation (tests/inception_torch_ref.py) with numpy's mean and covariance.

Tolerance.  The GPU path computes what the emulation computes up to the accumulation order; the emulation itself differs from the fp32
restatement by the bf16 rounding of the operands.  What that rounding does to the FID of these very inputs, |FID(emulation) - FID(fp32)|, is
computed here, and twice that is the bound on |FID(GPU) - FID(emulation)| -- the 2 x e_emul rule of tests/test_gpu_classifier.py applied
to the distance.  The FID of a folder against itself must stay below the same bound."""
import os
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import inception_torch_ref as ref

gpu = pytest.mark.gpu
DEV = "cuda:0"
N_REAL, N_FAKE, SIDE = 12, 9, 24


def make_images():
    g = torch.Generator().manual_seed(5)
    real = torch.randint(0, 256, (N_REAL, SIDE, SIDE, 3), generator=g, dtype=torch.uint8)
    fake = (torch.randint(0, 256, (N_FAKE, SIDE, SIDE, 3), generator=g, dtype=torch.uint8).float() * 0.8 + 40).clamp(0, 255).to(torch.uint8)
    return real, fake


def np_stats(f):
    from sfron import fid
    f = f.double().numpy()
    return fid.FIDStatistics(np.mean(f, axis=0), np.cov(f, rowvar=False))


def dist(a, b):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return a.frechet_distance(b)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from sfron import inception
    root = tmp_path_factory.mktemp("fid")
    real, fake = make_images()
    for name, arr in (("real", real), ("fake", fake)):
        os.makedirs(root / name)
        for i, a in enumerate(arr.numpy()):          # sorted file order == array order
            Image.fromarray(a).save(str(root / name / f"{i:03d}.png"))
        np.savez(str(root / f"{name}.npz"), arr_0=arr.numpy())
    m = ref.randomize(ref.FIDInceptionV3(), 11, probe=real[:2])
    ckpt = str(root / "inception.pt")
    torch.save(m.state_dict(), ckpt)
    emu = ref.Emulated(m)
    with torch.no_grad():
        feats = {"fp32": (m(real, upto=192), m(fake, upto=192)), "emul": (emu(real, upto=192), emu(fake, upto=192))}
    net = inception.InceptionV3(device=DEV).load_state_dict(m.state_dict())
    return root, ckpt, net, feats


@gpu
@pytest.mark.parametrize("feature", [64, 192])
def test_fid_folders_and_npz_against_the_emulation(setup, feature):
    from sfron import fid
    root, ckpt, net, feats = setup
    want = dist(np_stats(feats["emul"][1][feature]), np_stats(feats["emul"][0][feature]))
    fp32 = dist(np_stats(feats["fp32"][1][feature]), np_stats(feats["fp32"][0][feature]))
    tol = 2 * abs(want - fp32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got_folders = fid.fid_folders(str(root / "real"), str(root / "fake"), feature=feature, model=net)
        got_npz = fid.fid_npz(str(root / "real.npz"), str(root / "fake.npz"), feature=feature, model=net)
        same = fid.fid_folders(str(root / "real"), str(root / "real"), feature=feature, model=net)
    print(f"feature {feature}: FID emulation {want!r}, fp32 {fp32!r}, bound {tol:.3e}; folders {got_folders!r} (diff {abs(got_folders - want):.3e}), "
          f"npz {got_npz!r} (diff {abs(got_npz - want):.3e}), folder against itself {same:.3e}")
    assert tol > 0
    assert abs(got_folders - want) <= tol
    assert abs(got_npz - want) <= tol
    assert abs(same) < tol


@gpu
def test_checkpoint_path_saved_statistics_and_resize(setup):
    from sfron import fid
    root, ckpt, net, feats = setup
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = fid.fid_npz(str(root / "real.npz"), str(root / "fake.npz"), feature=64, model=net)
        b = fid.fid_npz(str(root / "real.npz"), str(root / "fake.npz"), feature=64, checkpoint=ckpt)          # the documented route
        assert a == b
        st = fid.InceptionFeatures(net, 64).add_npz(str(root / "real.npz")).statistics()
        st.save(str(root / "real_stats.npz"))
        assert fid.fid_npz(str(root / "real_stats.npz"), str(root / "fake.npz"), feature=64, model=net) == a
        with pytest.raises(ValueError, match="width"):
            fid.fid_npz(str(root / "real_stats.npz"), str(root / "fake.npz"), feature=192, model=net)
        # image_size: the Pillow-exact resize of resample.py first (setup_fid_data's bicubic Resize), then the same path
        r = fid.fid_folders(str(root / "real"), str(root / "fake"), feature=64, image_size=32, model=net)
        real, fake = (torch.stack([torch.from_numpy(np.asarray(Image.fromarray(x).resize((32, 32), Image.BICUBIC))) for x in arr.numpy()])
                      for arr in (torch.from_numpy(np.load(str(root / "real.npz"))["arr_0"]), torch.from_numpy(np.load(str(root / "fake.npz"))["arr_0"])))
        want = fid.InceptionFeatures(net, 64).add_images(fake).statistics().frechet_distance(fid.InceptionFeatures(net, 64).add_images(real).statistics())
        assert r == want
    ex = fid.InceptionFeatures(net, 64, batch_size=5).add_folder(str(root / "real"))          # batches of 5, 5 and 2: the same rows
    whole = fid.InceptionFeatures(net, 64).add_npz(str(root / "real.npz"))
    assert ex.n == N_REAL and ex.features().shape == (N_REAL, 64) and ex.features().is_cuda
    assert torch.equal(ex.features().cpu(), whole.features().cpu())


@gpu
def test_refusals(setup, tmp_path):
    from sfron import fid
    root, ckpt, net, feats = setup
    with pytest.raises(ValueError, match="checkpoint"):
        fid.fid_folders(str(root / "real"), str(root / "fake"), feature=64)
    with pytest.raises(ValueError, match="checkpoint"):
        fid.fid_npz(str(root / "real.npz"), str(root / "fake.npz"))
    for feature in (0, 100, 1008):
        with pytest.raises(ValueError, match="feature"):
            fid.fid_folders(str(root / "real"), str(root / "fake"), feature=feature, model=net)
        with pytest.raises(ValueError, match="feature"):
            fid.InceptionFeatures(net, feature)
    os.makedirs(tmp_path / "empty")
    with pytest.raises(FileNotFoundError):
        fid.fid_folders(str(tmp_path / "empty"), str(root / "fake"), feature=64, model=net)
    np.savez(str(tmp_path / "none.npz"), arr_0=np.zeros((0, 8, 8, 3), np.uint8))
    with pytest.raises(ValueError):
        fid.fid_npz(str(root / "real.npz"), str(tmp_path / "none.npz"), feature=64, model=net)
    with pytest.raises(ValueError):
        fid.feature_statistics(torch.zeros(1, 64, device=DEV))
