"""Generates tests/golden/ddpm_sample.npz: ``create_class_labels`` of the reference (DDPM/functions/__init__.py:127-134), imported and
called, for the strings "x0", "0", "1,3,5", "x2,x7" with n_classes 10.  Per string (index k): ``classes_k`` and ``excluded_k`` as int64
arrays; ``strings`` holds the inputs.  DDPM/functions loads without torchvision; the runner module and the dataset module do not, so the
sample drivers and inverse_data_transform have no fixture.

Run:  python tests/golden/make_ddpm_sample_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
STRINGS = ("x0", "0", "1,3,5", "x2,x7")


def main():
    sys.path.insert(0, os.path.join(REF, "DDPM"))
    from functions import create_class_labels
    out = {"strings": np.array(STRINGS), "n_classes": np.int64(10)}
    for k, s in enumerate(STRINGS):
        classes, excluded = create_class_labels(s, n_classes=10)
        out[f"classes_{k}"] = np.asarray(classes, dtype=np.int64)
        out[f"excluded_{k}"] = np.asarray(excluded, dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "ddpm_sample.npz"), **out)


if __name__ == "__main__":
    main()
