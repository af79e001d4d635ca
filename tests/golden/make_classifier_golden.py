"""Writes tests/golden/classifier_eval.npz from the reference's own DDPM/classifier_evaluation.py:

    python tests/golden/make_classifier_golden.py --reference <checkout of the reference project>

The reference module imports torchvision, which this project's environment does not have; ``validate`` and ``ImagePathDataset`` never touch
it, so stub modules stand in for ``torchvision`` and ``torchvision.transforms`` while it is imported.  Recorded:

  validate        two runs in a temporary working directory on a tiny seeded nn.Linear "classifier", 7 samples at batch 3 (a short last
                  batch): the logits per batch, the three numbers, and the text of results/cifar10/forget/result.csv after the first run
                  (one row inserted) and after the second (the same row updated).
  ImagePathDataset  the file order in a made-up folder with mixed extensions and a non-image file.
"""
import argparse
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

FILES = ["10.png", "2.png", "b.jpg", "a.jpeg", "A.png", "z.bmp", "m.webp", "notes.txt", "c.tiff", "0001.png", "x.PNG", "d.ppm"]
SAMPLE_PATH = "runs/cifar10/forget_run/fid_samples_guidance_2.0/class_0"


def load_reference(root):
    for name in ("torchvision", "torchvision.transforms"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    spec = importlib.util.spec_from_file_location("ref_classifier_evaluation", os.path.join(root, "DDPM", "classifier_evaluation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.device = torch.device("cpu")              # a global the script sets under __main__
    return mod


def run_validate(mod, seed, label, data):
    torch.manual_seed(seed)
    model = torch.nn.Linear(data.shape[1], 10)
    with torch.no_grad():
        model.weight.mul_(6.0)
    loader = torch.utils.data.DataLoader(data, batch_size=3)
    args = types.SimpleNamespace(label_of_forgotten_class=label, sample_path=SAMPLE_PATH)
    with torch.no_grad():
        logits = [model(b).clone() for b in loader]
        mod.validate(model, loader, args)
    text = open("results/cifar10/forget/result.csv").read()
    row = [ln for ln in text.splitlines() if ln.startswith(SAMPLE_PATH.split("/")[-4] + "/")][0].split(",")
    return logits, np.array([float(v) for v in row[1:4]], dtype=np.float64), text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "classifier_eval.npz"))
    a = ap.parse_args()
    mod = load_reference(os.path.abspath(a.reference))
    out = {"extensions": np.array(sorted(mod.IMAGE_EXTENSIONS)), "sample_path": np.array(SAMPLE_PATH)}
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            os.makedirs("results/cifar10/forget")
            data = torch.randn(7, 12, generator=torch.Generator().manual_seed(11))
            for run, (seed, label) in enumerate(((3, 0), (4, 2))):
                logits, numbers, text = run_validate(mod, seed, label, data)
                for k, lg in enumerate(logits):
                    out[f"run{run}_logits{k}"] = lg.numpy()
                out[f"run{run}_numbers"] = numbers
                out[f"run{run}_label"] = np.array(label)
                out[f"run{run}_csv"] = np.array(text)
            os.makedirs("folder/sub.png")
            for f in FILES:
                open(os.path.join("folder", f), "wb").close()
            ds = mod.ImagePathDataset("folder")
            out["folder_files"] = np.array(FILES)
            out["folder_order"] = np.array([p.name for p in ds.files])
        finally:
            os.chdir(here)
    np.savez(a.out, **out)
    print(f"wrote {a.out}: {sorted(out)}")


if __name__ == "__main__":
    main()
