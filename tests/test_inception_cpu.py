"""sfron.inception on the CPU: the plan against the torch restatement (tests/inception_torch_ref.py), the widths, the new C symbols in header
and prototypes, and the teeth of the network-level GPU test: each of the three FID variants, switched off in the restatement, must move the
2048-wide features further than the bound that test applies (2 * e_emul)."""
import os
import re

import pytest
import torch

import inception_torch_ref as ref
from sfron import _lib, inception

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sfron_patch_rows", "sfron_resize_tf1_u8", "sfron_pool3", "sfron_global_avgpool", "sfron_feature_stats")


def images():
    g = torch.Generator().manual_seed(3)
    return (torch.randint(0, 256, (2, 32, 32, 3), generator=g, dtype=torch.uint8),
            torch.randint(0, 256, (3, 40, 56, 3), generator=g, dtype=torch.uint8))


@pytest.fixture(scope="module")
def model():
    return ref.randomize(ref.FIDInceptionV3(), 11, probe=images()[0])


def feats(m, tap=2048):
    with torch.no_grad():
        return torch.cat([m(x)[tap] for x in images()])


def test_plan_matches_restatement():
    specs, convs, stem, blocks = inception.inception_plan()
    sd = ref.FIDInceptionV3().state_dict()
    assert list(specs) == list(sd)
    for k, shp in specs.items():
        assert tuple(sd[k].shape) == tuple(shp), k
    assert len(convs) == 94
    assert specs["fc.weight"] == (1008, 2048)


def test_widths(model):
    specs, convs, stem, blocks = inception.inception_plan()
    assert inception.TAPS == (64, 192, 768, 2048)
    assert [b[2] for b in blocks] == [256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048] == list(inception.BLOCK_WIDTHS)
    assert [s[1] for s in stem if s[0] == "tap"] == [64, 192]
    for name, cin, width, branches in blocks:          # the columns the branches write add up to the block width
        cols = 0
        for br in branches:
            last = br[-1]
            cols += cin if last[0] == "max2" else sum(convs[i][2] for i in last[1:])
        assert cols == width, name
    with torch.no_grad():
        out, ws = model.taps(images()[0], widths=True)
    assert ws == list(inception.BLOCK_WIDTHS)
    assert {k: v.shape[1] for k, v in out.items()} == {t: t for t in inception.TAPS}


def test_every_convolution_has_a_product():
    """1x1 and 3x3 with one pad go to sfron_conv_fwd, the rest to the patch matrix; the forms the GPU test covers are the forms in the net."""
    specs, convs, stem, blocks = inception.inception_plan()
    patch_forms = {cv[3:] for cv in convs if not inception._direct(cv)}
    assert patch_forms == {(1, 7, 1, 0, 3), (7, 1, 1, 3, 0), (1, 3, 1, 0, 1), (3, 1, 1, 1, 0), (5, 5, 1, 2, 2), (3, 3, 2, 0, 0)}
    assert {cv[3:] for cv in convs if inception._direct(cv)} == {(1, 1, 1, 0, 0), (3, 3, 1, 0, 0), (3, 3, 1, 1, 1), (3, 3, 2, 0, 0)}
    assert all(cv[1] % 8 == 0 for cv in convs[1:]) and convs[0][1] == 3


def test_flops():
    full, first = inception.flops(), inception.flops(64)
    assert 11.0e9 < full < 12.0e9 and 1.0e9 < first < 1.5e9          # 5.7 GMAC: the published figure for Inception-v3 at 299 x 299
    assert first < inception.flops(192) < inception.flops(768) < full


def test_symbols_in_header_and_prototypes():
    assert _lib.ABI_VERSION == 17
    with open(os.path.join(ROOT, "unified-unlearning-w-remain-geometry_amd", "csrc", "api.hip")) as f:
        assert "sfron_abi_version(void) { return 17; }" in f.read()
    with open(os.path.join(ROOT, "include", "sfron.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/sfron.h"
        assert name in _lib._PROTOS, name
        assert len(_lib._PROTOS[name][1]) == m.group(1).count(",") + 1, name
    for name in ("SFRON_POOL_MAX_S2 = 0", "SFRON_POOL_MAX_S1 = 1", "SFRON_POOL_AVG_S1 = 2"):
        assert name in header
    assert (_lib.POOL_MAX_S2, _lib.POOL_MAX_S1, _lib.POOL_AVG_S1) == (0, 1, 2)


def test_no_cpu_fallback():
    with pytest.raises(_lib.SfronError):
        inception.InceptionV3(device="cpu")


def test_variants_have_teeth(model):
    """The network-level GPU test accepts rel_l2 <= 2 * e_emul at every tap.  Each FID variant switched off must lie further away than that
    at the 2048 tap, or that test could not tell it from the true net.  All three separate here (count_include_pad 4.1e-2, average pool in
    Mixed_7c 1.2e-1, half-pixel resize 1.7e-2 against 2 * e_emul = 8.3e-3), so none is carried by its exact kernel test alone -- though each
    has one (tests/test_gpu_inception.py: the pool divisors, the max pool, the resize rule)."""
    truth = feats(model)
    emu = ref.Emulated(model)
    e_emul = ref.rel_l2(torch.cat([emu(x)[2048] for x in images()]), truth)
    print(f"e_emul(2048) = {e_emul:.3e}")
    assert 0 < e_emul < 2e-2
    for kw in (dict(count_include_pad=True), dict(last_pool="avg"), dict(resize="half_pixel")):
        v = ref.FIDInceptionV3(**kw)
        v.load_state_dict(model.state_dict())
        d = ref.rel_l2(feats(v.eval()), truth)
        print(kw, f"{d:.3e}")
        assert d > 2 * e_emul, (kw, d, e_emul)
