"""CPU: the classifier evaluators without a GPU -- BatchNorm folding, the state-dict contract of sfron.resnet against the torch restatement
(tests/resnet_torch_ref.py), the file listing and the CSV texts against the fixture recorded from the reference's own
DDPM/classifier_evaluation.py (tests/golden/classifier_eval.npz, written by tests/golden/make_classifier_golden.py), the prompts join against
pandas, the chunk arithmetic, the ABI of csrc/classify.hip and its argument refusals (which precede any launch), and the evaluators' resize
against Pillow."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import resnet_torch_ref as R
from test_sd_front_end_cpu import apply_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sfron_image_u8_patches7", "sfron_nchw_patches7", "sfron_relu_maxpool3s2", "sfron_relu_rows", "sfron_pool_fc", "sfron_classify_metrics")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from sfron import _lib
    return _lib


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "classifier_eval.npz"))


# ------------------------------------------------------------------------------------------------ the model's contract
def test_bn_folding_matches_batchnorm_eval_in_fp64():
    from sfron import resnet
    g = torch.Generator().manual_seed(0)
    conv = torch.nn.Conv2d(5, 7, 3, 2, 1, bias=False).double()
    bn = torch.nn.BatchNorm2d(7).double().eval()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g, dtype=torch.float64))
        bn.weight.copy_(torch.rand(7, generator=g, dtype=torch.float64) + 0.5)
        bn.bias.copy_(torch.randn(7, generator=g, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(7, generator=g, dtype=torch.float64))
        bn.running_var.copy_(torch.rand(7, generator=g, dtype=torch.float64) + 0.5)
        x = torch.randn(2, 5, 9, 8, generator=g, dtype=torch.float64)
        want = bn(conv(x))
        w, b = resnet.fold_bn(conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)
        got = torch.nn.functional.conv2d(x, w, b, 2, 1)
    assert w.dtype == b.dtype == torch.float64
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-12


@pytest.mark.parametrize("name,ncls,convs,downs", [("resnet34", 10, 36, 3), ("resnet50", 1000, 53, 4)])
def test_state_dict_keys_are_torchvisions(name, ncls, convs, downs):
    from sfron import resnet
    ours = getattr(resnet, name)(ncls)
    ref = getattr(R, name)(ncls)
    sd = ref.state_dict()
    assert list(ours.specs) == list(sd.keys())
    assert all(tuple(ours.specs[k]) == tuple(v.shape) for k, v in sd.items())
    assert len(ours.convs) == convs == sum(isinstance(m, torch.nn.Conv2d) for m in ref.modules())
    assert sum(".downsample." in c[0] for c in ours.convs) == downs
    # v1.5: in Bottleneck the stride sits on the 3x3
    if name == "resnet50":
        by = {c[0]: c for c in ours.convs}
        assert by["layer2.0.conv1"][5] == 1 and by["layer2.0.conv2"][5] == 2 and by["layer2.0.downsample.0"][4:7] == (1, 2, 0)
    # a module. prefix is accepted; the canonical dict carries the plain names
    can = ours._canonical({"module." + k: v for k, v in sd.items()})
    assert list(can) == list(sd.keys())
    assert all(torch.equal(can[k], sd[k]) for k in sd)


def test_load_state_dict_names_missing_and_unexpected_keys():
    from sfron import resnet
    m = resnet.resnet34(10)
    sd = R.resnet34(10).state_dict()
    bad = dict(sd)
    del bad["layer2.0.downsample.0.weight"], bad["fc.bias"]
    with pytest.raises(KeyError) as e:
        m.load_state_dict(bad)
    assert "layer2.0.downsample.0.weight" in str(e.value) and "fc.bias" in str(e.value) and "missing" in str(e.value)
    bad = dict(sd)
    bad["layer9.0.conv1.weight"] = torch.zeros(1)
    with pytest.raises(KeyError) as e:
        m.load_state_dict(bad)
    assert "layer9.0.conv1.weight" in str(e.value) and "unexpected" in str(e.value)
    with pytest.raises(NotImplementedError):
        m.train()
    assert m.eval() is m and m.train(False) is m


def test_chunk_size_arithmetic_at_224():
    from sfron import resnet
    patch = 112 * 112 * 152 * 2                 # the stem's patch matrix: the largest operand of one 224 px sample
    for ctor in (resnet.resnet34, resnet.resnet50):
        m = ctor(10)
        assert m.per_sample_bytes(224, 224) == patch
        assert 112 * 112 * 64 * 4 < patch and 56 * 56 * 256 * 4 < patch
        assert m.chunk_size(224, 224) == (1 << 30) // patch == 281
        small = ctor(10, max_chunk_bytes=2 * patch + 5)
        assert small.chunk_size(224, 224) == 2
        assert ctor(10, max_chunk_bytes=1).chunk_size(224, 224) == 1
    # at 64 px ResNet-50's widest fp32 activation (layer1: 16 x 16 x 256) passes the patch matrix
    assert resnet.resnet50().per_sample_bytes(64, 64) == max(32 * 32 * 152 * 2, 16 * 16 * 256 * 4)
    assert resnet.resnet_flops(resnet.Bottleneck, [3, 4, 6, 3], 1000, 224, 224) == pytest.approx(2 * 4.09e9, rel=0.01)
    assert resnet.resnet_flops(resnet.BasicBlock, [3, 4, 6, 3], 1000, 224, 224) == pytest.approx(2 * 3.66e9, rel=0.01)


# ------------------------------------------------------------------------------------------------ the reference's listing and CSV
def test_image_paths_order_is_the_references(golden, tmp_path):
    from sfron import classify
    assert sorted(classify.IMAGE_EXTENSIONS) == [str(s) for s in golden["extensions"]]
    os.makedirs(tmp_path / "sub.png")
    for f in golden["folder_files"]:
        open(tmp_path / str(f), "wb").close()
    got = [p.name for p in classify.image_paths(str(tmp_path))]
    assert got == [str(s) for s in golden["folder_order"]]
    assert "notes.txt" not in got and "x.PNG" not in got


def test_result_csv_insert_then_update_is_pandas_text(golden, tmp_path):
    from sfron import classify
    path = str(tmp_path / "results" / "cifar10" / "forget" / "result.csv")
    parts = str(golden["sample_path"]).split("/")
    name = parts[-4] + "/" + parts[-3]
    for run in (0, 1):
        res = dict(zip(classify.RESULT_COLUMNS, (float(v) for v in golden[f"run{run}_numbers"])))
        text = classify.update_result_csv(path, name, res)
        assert text == str(golden[f"run{run}_csv"]) == open(path).read()
    # another run's row is appended, the first stays
    classify.update_result_csv(path, "cifar10/other", {"entropy": 0.5, "prob of forgotten class": 0.25, "accuracy of forgotten class": 1.0})
    lines = open(path).read().splitlines()
    assert len(lines) == 3 and lines[1] == str(golden["run1_csv"]).splitlines()[1] and lines[2] == "cifar10/other,0.5,0.25,1.0"


def test_prompts_join_is_pandas_merge(tmp_path):
    pd = pytest.importorskip("pandas")
    from sfron import classify
    prompts = tmp_path / "prompts.csv"
    prompts.write_text('case_number,prompt,evaluation_seed,class\n0,"Image of a tench, fish",42,tench\n1,Image of a church,7,church\n'
                       "2,Image of a parachute,9,parachute\n5,unused,1,none\n")
    names = ["0_0.png", "0_1.png", "2_0.png", "10_0.jpg", "1.png"]
    rng = np.random.default_rng(0)
    res = {"case_number": [classify.case_number(n) for n in names]}
    assert res["case_number"] == [0, 0, 2, 10, 1]
    for k in (1, 2):
        idx = [int(v) for v in rng.integers(0, 1000, len(names))]
        res[f"category_top{k}"] = idx
        res[f"index_top{k}"] = idx
        res[f"scores_top{k}"] = list(rng.random(len(names)).astype(np.float32))
    ours = tmp_path / "ours.csv"
    header, rows = classify.join_prompts(str(prompts), res, str(ours))
    df = pd.read_csv(prompts)
    df["case_number"] = df["case_number"].astype("int")
    theirs = tmp_path / "theirs.csv"
    pd.merge(df, pd.DataFrame(res)).to_csv(theirs)
    assert ours.read_text() == theirs.read_text()
    assert [r[1] for r in rows] == ["0", "0", "1", "2"]          # the prompts that have pictures, in the prompts file's order


# ------------------------------------------------------------------------------------------------ the ABI of csrc/classify.hip
_CTYPE = {"const uint8_t*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "uint16_t*": ctypes.c_void_p,
          "int32_t*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


def test_header_and_ctypes_prototypes_agree(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfron.h")).read(), flags=re.S)
    assert built.ABI_VERSION == 17 and built.lib().sfron_abi_version() == 17
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/sfron.h"
        want = []
        for arg in m.group(1).split(","):
            typ = re.sub(r"\s+", " ", arg.strip()).rsplit(" ", 1)[0].replace(" *", "*")
            want.append(_CTYPE[typ])
        res, args = built._PROTOS[name]
        assert res is ctypes.c_int and list(args) == want, name
        assert hasattr(built.lib(), name)


def test_new_entry_points_refuse_bad_arguments_before_any_launch(built):
    """A null pointer, a zero extent and an operand of 2 GiB or more: SFRON_ERR_ARG.  The addresses are made up -- nothing may be launched."""
    L, E = built.lib(), built.ERR_ARG
    A, B_, C_, D_ = 0x10000, 0x20000, 0x30000, 0x40000
    half = (0.5,) * 6
    # (H + 6 - 7) / 2 + 1 = 16384 rows and columns per sample at 32768 px: 4 samples x 152 columns x 2 bytes = 2^31 + ...
    for bad in [(None, 1, 8, 8, *half, 152, B_), (A, 1, 8, 8, *half, 152, None), (A, 0, 8, 8, *half, 152, B_), (A, 1, 0, 8, *half, 152, B_),
                (A, 1, 8, 8, *half, 144, B_), (A, 1, 8, 8, *half, 156, B_), (A, 4, 32768, 32768, *half, 152, B_)]:
        assert L.sfron_image_u8_patches7(*bad, None) == E, bad
    for bad in [(None, 1, 8, 8, 152, B_), (A, 1, 8, 8, 152, None), (A, 1, 8, 0, 152, B_), (A, 1, 8, 8, 152, B_ + 2), (A, 4, 32768, 32768, 152, B_)]:
        assert L.sfron_nchw_patches7(*bad, None) == E, bad
    for bad in [(None, 64, 1, 8, 8, 64, 1, B_, C_), (A, 64, 1, 8, 8, 64, 1, None, None), (A, 64, 0, 8, 8, 64, 1, B_, C_), (A, 64, 1, 8, 8, 0, 1, B_, C_),
                (A, 32, 1, 8, 8, 64, 1, B_, C_), (A, 64, 1, 8, 8, 62, 1, B_, C_), (A, 64, 2, 2048, 2048, 64, 1, B_, C_)]:
        assert L.sfron_relu_maxpool3s2(*bad, None) == E, bad
    for bad in [(None, 64, 8, 64, B_, C_), (A, 64, 8, 64, None, None), (A, 64, 0, 64, B_, C_), (A, 64, 8, 0, B_, C_), (A, 64, 1 << 23, 64, B_, C_)]:
        assert L.sfron_relu_rows(*bad, None) == E, bad
    for bad in [(None, 64, 1, 4, 64, B_, C_, 10, D_, A), (A, 64, 1, 4, 64, None, C_, 10, D_, A), (A, 64, 1, 4, 64, B_, C_, 10, None, A),
                (A, 64, 1, 4, 64, B_, C_, 10, D_, None), (A, 64, 0, 4, 64, B_, C_, 10, D_, A), (A, 64, 1, 0, 64, B_, C_, 10, D_, A),
                (A, 64, 1, 4, 64, B_, C_, 0, D_, A), (A, 2048, 512, 512, 2048, B_, C_, 10, D_, A), (A, 2048, 1, 1, 2048, B_, C_, 1 << 18, D_, A)]:
        assert L.sfron_pool_fc(*bad, None) == E, bad
    for bad in [(None, 10, 2, 10, 0, 5, A, B_, C_, D_, A, B_), (A, 10, 0, 10, 0, 5, A, B_, C_, D_, A, B_), (A, 10, 2, 0, 0, 0, A, B_, C_, D_, A, B_),
                (A, 8, 2, 10, 0, 5, A, B_, C_, D_, A, B_), (A, 10, 2, 10, 10, 5, A, B_, C_, D_, A, B_), (A, 10, 2, 10, 0, 9, A, B_, C_, D_, A, B_),
                (A, 10, 2, 10, 0, 5, A, B_, C_, D_, None, B_), (A, 1 << 20, 1 << 9, 1 << 20, 0, 5, A, B_, C_, D_, A, B_)]:
        assert L.sfron_classify_metrics(*bad, None) == E, bad


# ------------------------------------------------------------------------------------------------ the evaluators' resize
def _picture(h, w, seed):
    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8))


@pytest.mark.parametrize("h,w", [(32, 32), (40, 24), (512, 512), (24, 40)])
def test_resize_and_crop_bytes_are_pillows(h, w):
    from sfron import classify, resample
    img = _picture(h, w, h * 1000 + w)
    a = np.asarray(img)
    # Resize((224, 224)): both axes on their own
    want = np.asarray(img.resize((224, 224), Image.BILINEAR))
    assert np.array_equal(classify.transform_host(img, (224, 224)), want)
    tx, ty = classify.resize_tables(w, h, (224, 224))
    assert np.array_equal(apply_spec(a, tx.coeffs, tx.bounds, ty.coeffs, ty.bounds), want)
    # Resize(232) -> CenterCrop(224): the short side becomes 232, the long side int(232 * long / short)
    short, long = min(h, w), max(h, w)
    nl = int(232 * long / short)
    nw, nh = (232, nl) if w <= h else (nl, 232)
    top, left = int(round((nh - 224) / 2.0)), int(round((nw - 224) / 2.0))
    want = np.asarray(img.resize((nw, nh), Image.BILINEAR).crop((left, top, left + 224, top + 224)))
    assert want.shape == (224, 224, 3)
    assert np.array_equal(classify.transform_host(img, 232, crop=224), want)
    tx, ty = classify.resize_tables(w, h, 232, crop=224)
    assert np.array_equal(apply_spec(a, tx.coeffs, tx.bounds, ty.coeffs, ty.bounds), want)
    # the defaulted argument leaves the SD transform as it was
    assert resample.center_crop_offsets(300, 260, 256) == resample.center_crop_offsets(300, 260, 256, 256) == (22, 2)
    assert resample.center_crop_offsets(232, 386, 232, 224) == (4, 81)
    # a palette image is converted before it is resized, as ImagePathDataset does
    pal = img.convert("P")
    assert np.array_equal(classify.transform_host(pal, (224, 224)), np.asarray(pal.convert("RGB").resize((224, 224), Image.BILINEAR)))
