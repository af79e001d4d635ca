"""Writes tests/golden/ddpm_data.npz from the reference's own DDPM/dataset/__init__.py:

    python tests/golden/make_ddpm_data_golden.py --reference <checkout of the reference project>

The reference module imports torchvision, which this project's environment does not have; stub modules stand in for ``torchvision``,
``torchvision.transforms``, ``torchvision.transforms.functional`` and ``torchvision.datasets`` while it is imported.  Recorded:

  data_transform      all 24 forms (uniform x gaussian x {rescaled, logit, neither} x with / without image_mean) on one input of 2 images
                      [1][16][16] whose first holds every byte value 0..255 (X = byte / 255, ToTensor's division).  The generator is
                      re-seeded before every call and the draws are re-made afterwards in the reference's order (rand_like, then
                      randn_like), so ``u``, ``n_alone`` (gaussian only) and ``n_after_u`` (both) are the numbers the call used.
  get_forget_dataset  on a stub CIFAR10 of 23 items (labels i % 4, label 1 dropped) whose transform counts its calls: the remain / forget
                      order, the flip each kept item got, len() of both loaders at batch size 4 (short last batches), the number of
                      transform calls after construction and after two epochs over both loaders (unchanged: the flip is frozen).
  antithetic t        ``cat([t, T - t - 1])[:n]`` (runners/diffusion.py:132-135) for n = 1, 2, 5, 128 with the randint draws.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

N_ITEMS, LABEL_TO_DROP, BATCH, SEED = 23, 1, 4, 1234
CALLS = {"flip": 0, "to_tensor": 0}


class _Compose:
    def __init__(self, ts):
        self.ts = ts

    def __call__(self, x):
        for t in self.ts:
            x = t(x)
        return x


class _Resize:
    def __init__(self, size):
        self.size = size

    def __call__(self, x):
        return x


class _Flip:                                      # torchvision's rule: ``if torch.rand(1) < self.p: return hflip(img)``
    def __init__(self, p=0.5):
        self.p = p

    def __call__(self, x):
        CALLS["flip"] += 1
        return x.flip(-1) if torch.rand(1) < self.p else x


class _ToTensor:
    def __call__(self, x):
        CALLS["to_tensor"] += 1
        return x.float().div(255)


class _StubCIFAR10:
    """23 uint8 images [3][4][4]: channel 0 holds the item's number, channel 1 a ramp along the width (tells a flip), labels i % 4"""

    def __init__(self, root, train=True, download=False, transform=None):
        self.transform = transform
        self.targets = [i % 4 for i in range(N_ITEMS)]

    def __len__(self):
        return N_ITEMS

    def __getitem__(self, i):
        if i >= N_ITEMS:
            raise IndexError(i)
        img = torch.zeros(3, 4, 4, dtype=torch.uint8)
        img[0] = i
        img[1] = torch.arange(4, dtype=torch.uint8)[None, :]
        return self.transform(img), self.targets[i]


def load_reference(root):
    for name in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional", "torchvision.datasets"):
        sys.modules.setdefault(name, types.ModuleType(name))
    tv, tr, ds = sys.modules["torchvision"], sys.modules["torchvision.transforms"], sys.modules["torchvision.datasets"]
    tv.transforms, tv.datasets, tr.functional = tr, ds, sys.modules["torchvision.transforms.functional"]
    tr.Compose, tr.Resize, tr.RandomHorizontalFlip, tr.ToTensor = _Compose, _Resize, _Flip, _ToTensor
    ds.CIFAR10, ds.STL10, ds.ImageFolder = _StubCIFAR10, None, None
    spec = importlib.util.spec_from_file_location("ref_ddpm_dataset", os.path.join(root, "DDPM", "dataset", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record_data_transform(mod, out):
    g = torch.Generator().manual_seed(5)
    bytes_ = torch.stack([torch.arange(256, dtype=torch.uint8).view(1, 16, 16),
                          torch.randint(0, 256, (1, 16, 16), generator=g, dtype=torch.uint8)])
    X = bytes_.float().div(255)
    mean = torch.rand(1, 16, 16, generator=g)
    out["dt_bytes"], out["dt_image_mean"] = bytes_.numpy(), mean.numpy()
    for uni in (0, 1):
        for gau in (0, 1):
            for mode in ("rescaled", "logit", "neither"):
                for with_mean in (0, 1):
                    cfg = types.SimpleNamespace(data=types.SimpleNamespace(uniform_dequantization=bool(uni), gaussian_dequantization=bool(gau),
                                                                           rescaled=mode == "rescaled", logit_transform=mode == "logit"))
                    if with_mean:
                        cfg.image_mean = mean
                    torch.manual_seed(SEED)
                    out[f"dt_u{uni}_g{gau}_{mode}_m{with_mean}"] = mod.data_transform(cfg, X.clone()).numpy()
    torch.manual_seed(SEED)
    out["dt_u"] = torch.rand_like(X).numpy()
    out["dt_n_after_u"] = torch.randn_like(X).numpy()
    torch.manual_seed(SEED)
    out["dt_n_alone"] = torch.randn_like(X).numpy()


def record_split(mod, out):
    cfg = types.SimpleNamespace(data=types.SimpleNamespace(random_flip=True, image_size=4, dataset="CIFAR10", path="unused", num_workers=0),
                                training=types.SimpleNamespace(batch_size=BATCH))
    torch.manual_seed(SEED)
    remain, forget = mod.get_forget_dataset(None, cfg, LABEL_TO_DROP)
    out["split_calls_after_construction"] = np.array([CALLS["flip"], CALLS["to_tensor"]])
    for name, loader in (("remain", remain), ("forget", forget)):
        items = loader.dataset
        out[f"split_{name}_ids"] = np.array([int(round(float(x[0, 0, 0]) * 255)) for x, _ in items])
        out[f"split_{name}_labels"] = np.array([c for _, c in items])
        out[f"split_{name}_flipped"] = np.array([int(round(float(x[1, 0, 0]) * 255)) == 3 for x, _ in items])
        out[f"split_{name}_len"] = np.array(len(loader))
        for epoch in range(2):
            sizes, ids, flipped = [], [], []
            for x, c in loader:
                sizes.append(x.shape[0])
                ids.extend(int(round(float(v) * 255)) for v in x[:, 0, 0, 0])
                flipped.extend(int(round(float(v) * 255)) == 3 for v in x[:, 1, 0, 0])
            out[f"split_{name}_epoch{epoch}_sizes"] = np.array(sizes)
            out[f"split_{name}_epoch{epoch}_ids"] = np.array(ids)
            out[f"split_{name}_epoch{epoch}_flipped"] = np.array(flipped)
    out["split_calls_after_epochs"] = np.array([CALLS["flip"], CALLS["to_tensor"]])
    out["split_n_items"], out["split_label_to_drop"], out["split_batch"] = np.array(N_ITEMS), np.array(LABEL_TO_DROP), np.array(BATCH)


def record_antithetic(out, T=1000):
    torch.manual_seed(SEED)
    for n in (1, 2, 5, 128):
        t_half = torch.randint(low=0, high=T, size=(n // 2 + 1,))
        out[f"t_half_{n}"] = t_half.numpy()
        out[f"t_{n}"] = torch.cat([t_half, T - t_half - 1], dim=0)[:n].numpy()
    out["t_T"] = np.array(T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "ddpm_data.npz"))
    a = ap.parse_args()
    mod = load_reference(os.path.abspath(a.reference))
    out = {}
    record_data_transform(mod, out)
    record_split(mod, out)
    record_antithetic(out)
    np.savez(a.out, **out)
    print(f"wrote {a.out}: {len(out)} arrays, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
