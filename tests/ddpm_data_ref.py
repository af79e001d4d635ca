"""What the DDPM data-path tests share (tests/test_ddpm_data_cpu.py, tests/test_gpu_ddpm_data.py, tests/test_gpu_ddpm_train.py): the 24
forms of data_transform, their configs, and the check of the logit forms."""
from types import SimpleNamespace as NS

import torch

import dit_rows_ref as R

MODES = ("rescaled", "logit", "neither")
FORMS = [(u, g, m, mean) for u in (0, 1) for g in (0, 1) for m in MODES for mean in (0, 1)]
assert len(FORMS) == 24 and sum(f[2] != "logit" for f in FORMS) == 16


def form_config(u, g, mode, mean=None, **data):
    cfg = NS(data=NS(uniform_dequantization=bool(u), gaussian_dequantization=bool(g), rescaled=mode == "rescaled",
                     logit_transform=mode == "logit", **data))
    if mean is not None:
        cfg.image_mean = mean
    return cfg


def logit_refs(cfg, X, u, n, dtype):
    """A logit form on the CPU, in ``dtype`` from the fp32 ``image`` on: every op up to ``image = lam + (1 - 2 lam) X`` is fp32 as the
    reference forms it (those ops are the bit-equal forms), the logarithms, their difference and the mean's subtraction are ``dtype``."""
    from sfron import ddpm_data
    pre = NS(data=NS(**dict(vars(cfg.data), logit_transform=False)))
    x = ddpm_data.data_transform(pre, X.cpu(), u=None if u is None else u.cpu(), n=None if n is None else n.cpu())
    image = ddpm_data.LOGIT_LAM + (1 - 2 * ddpm_data.LOGIT_LAM) * x
    out = torch.log(image.to(dtype)) - torch.log1p(-image.to(dtype))
    return out - cfg.image_mean.cpu().to(dtype)[None] if hasattr(cfg, "image_mean") else out


def check_logit(got, ref64, ref32, name):
    """``bound32`` (its MARGIN) over the elements the reference leaves finite.  Gaussian dequantization is not clamped, so a byte near 0 or
    255 can put ``image`` outside (0, 1), where the reference's own result is NaN (or an infinity at exactly 0 or 1) -- bound32 takes
    finite values only.  ``image`` is exact, so such an element is the same kind of non-finite value for the kernel: those must match as
    they are.  Returns the number of non-finite elements."""
    got, ref64, ref32 = got.detach().cpu(), ref64.cpu(), ref32.cpu()
    fin = torch.isfinite(ref64)
    assert torch.equal(torch.isfinite(ref32), fin), name
    assert torch.equal(torch.isfinite(got), fin), f"{name}: finite where the reference is not, or the reverse"
    assert torch.equal(torch.isnan(got), torch.isnan(ref64)), name
    inf = torch.isinf(ref64)
    assert torch.equal(got[inf].double(), ref64[inf]), name
    R.bound32(got[fin], ref64[fin], ref32[fin], name=name)
    return int((~fin).sum())
