"""CPU: the host side of the DDPM data path (sfron.ddpm_data, csrc/ddpm_data.hip's entry point).

The reference's own data_transform, get_forget_dataset and antithetic draw, recorded in tests/golden/ddpm_data.npz by
tests/golden/make_ddpm_data_golden.py, against ``ddpm_data.data_transform`` (exact on the 16 forms without the logit; the 8 logit forms
under ``dit_rows_ref.bound32``), ``split_forget``, the loader's ``len`` / epochs / flip modes / rank slices and ``antithetic_t``; the two
dataset readers on tiny directories written here; the new symbol's prototype with the ABI version still 16, and its refusals (they come
before any launch, so no GPU is touched)."""
import ctypes
import os
import pickle
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from ddpm_data_ref import FORMS, check_logit, form_config, logit_refs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sfron_ddpm_batch_u8"


@pytest.fixture(scope="module")
def G(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ddpm_data.npz")))


def form_noise(G, u, g):
    return (torch.from_numpy(G["dt_u"]) if u else None,
            torch.from_numpy(G["dt_n_after_u"] if u else G["dt_n_alone"]) if g else None)


# ------------------------------------------------------------------------------------------------ data_transform against the fixture
def test_fixture_holds_every_byte_value(G):
    assert sorted(G["dt_bytes"][0].reshape(-1).tolist()) == list(range(256))
    assert len([k for k in G if k.startswith("dt_u") and "_m" in k]) == 24


@pytest.mark.parametrize("u,g,mode,with_mean", FORMS, ids=lambda v: str(v))
def test_data_transform_against_the_reference(G, u, g, mode, with_mean):
    from sfron import ddpm_data
    X = torch.from_numpy(G["dt_bytes"]).float() / 255
    cfg = form_config(u, g, mode, torch.from_numpy(G["dt_image_mean"]) if with_mean else None)
    un, nn = form_noise(G, u, g)
    want = torch.from_numpy(G[f"dt_u{u}_g{g}_{mode}_m{with_mean}"])
    got = ddpm_data.data_transform(cfg, X, u=un, n=nn)
    assert got.dtype == torch.float32 and got.shape == want.shape
    if mode != "logit":
        assert torch.equal(got, want)
    else:
        check_logit(got, logit_refs(cfg, X, un, nn, torch.float64), want, f"logit u{u} g{g} m{with_mean}")
    # drawn inside, from a generator re-seeded as the fixture's was: the reference's order of draws
    gen = torch.Generator().manual_seed(1234)
    again = ddpm_data.data_transform(cfg, X, generator=gen)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))


# ------------------------------------------------------------------------------------------------ split, loader, antithetic t
def test_split_forget_is_the_reference_order(G):
    from sfron import ddpm_data
    labels = [i % 4 for i in range(int(G["split_n_items"]))]
    for lab in (labels, np.array(labels), torch.tensor(labels)):
        remain, forget = ddpm_data.split_forget(lab, int(G["split_label_to_drop"]))
        assert remain.dtype == torch.int64 and remain.tolist() == G["split_remain_ids"].tolist()
        assert forget.tolist() == G["split_forget_ids"].tolist()
    assert [labels[i] for i in remain.tolist()] == G["split_remain_labels"].tolist()


def tiny_dataset(n=23, C=3, H=4, W=4, device="cpu"):
    from sfron import ddpm_data
    img = torch.zeros(n, C, H, W, dtype=torch.uint8)
    img[:, 0] = torch.arange(n, dtype=torch.uint8)[:, None, None]
    img[:, 1] = torch.arange(W, dtype=torch.uint8)[None, None, :]
    return ddpm_data.ResidentDataset(img, torch.arange(n) % 4, device=device)


def loader_of(ds, idx, bs, flip, seed=3, rank=0, world=1, **data):
    from sfron import ddpm_data
    cfg = NS(data=NS(random_flip=flip is not None, **data))
    return ddpm_data.DDPMBatchLoader(ds, idx, bs, cfg, 1000, torch.Generator().manual_seed(seed), flip=flip, rank=rank, world=world)


def test_len_and_epochs_with_a_short_last_batch(G):
    from sfron import ddpm_data
    ds = tiny_dataset()
    remain, forget = ddpm_data.split_forget(ds.labels_host, 1)
    for name, idx in (("remain", remain), ("forget", forget)):
        ld = loader_of(ds, idx, int(G["split_batch"]), None)
        assert len(ld) == int(G[f"split_{name}_len"])
        epochs = [list(ld.index_batches()) for _ in range(2)]
        for ep in epochs:
            assert [b[0].shape[0] for b in ep] == G[f"split_{name}_epoch0_sizes"].tolist()        # drop_last=False
            assert sorted(torch.cat([b[0] for b in ep]).tolist()) == sorted(G[f"split_{name}_epoch0_ids"].tolist())
            assert all(b[1] is None for b in ep)
        assert torch.cat([b[0] for b in epochs[0]]).tolist() != torch.cat([b[0] for b in epochs[1]]).tolist()   # a fresh permutation
    # the documented order of draws: one randperm per epoch, nothing else without flips
    g = torch.Generator().manual_seed(3)
    want = [forget[torch.randperm(len(forget), generator=g)] for _ in range(2)]
    ld = loader_of(ds, forget, 4, None)
    for w in want:
        assert torch.cat([b[0] for b in ld.index_batches()]).tolist() == w.tolist()


def test_flip_modes(G):
    """frozen: one draw per image at construction, the same flag in every epoch -- what the fixture shows of get_forget_dataset, whose
    transform ran 2 N times while the two lists were built (each comprehension walks the whole dataset) and never again over two epochs.
    per_access: a draw per batch."""
    assert G["split_calls_after_construction"].tolist() == G["split_calls_after_epochs"].tolist() == [46, 46]
    for name in ("remain", "forget"):
        frozen = dict(zip(G[f"split_{name}_ids"].tolist(), G[f"split_{name}_flipped"].tolist()))
        for ep in (0, 1):
            assert dict(zip(G[f"split_{name}_epoch{ep}_ids"].tolist(), G[f"split_{name}_epoch{ep}_flipped"].tolist())) == frozen
    ds = tiny_dataset()
    idx = torch.tensor([0, 2, 3, 4, 6, 7, 8, 10, 11])
    g = torch.Generator().manual_seed(3)
    flags = (torch.rand(len(idx), generator=g) < 0.5)
    ld = loader_of(ds, idx, 4, "frozen")
    assert ld.frozen.dtype == torch.uint8 and ld.frozen.bool().tolist() == flags.tolist()
    want = dict(zip(idx.tolist(), flags.tolist()))
    for _ in range(2):
        for i, f in ld.index_batches():
            assert [want[k] for k in i.tolist()] == f.bool().tolist()
    ld = loader_of(ds, idx, 4, "per_access")
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(len(idx), generator=g)
    for k, (i, f) in enumerate(ld.index_batches()):
        assert i.tolist() == idx[perm[4 * k:4 * k + 4]].tolist()
        assert f.bool().tolist() == (torch.rand(i.shape[0], generator=g) < 0.5).tolist()
    from sfron import ddpm_data
    for random_flip, want_mode in ((True, "frozen"), (False, None)):              # the default follows config.data.random_flip
        ld = ddpm_data.DDPMBatchLoader(ds, idx, 4, NS(data=NS(random_flip=random_flip)), 1000, torch.Generator().manual_seed(3))
        assert ld.flip == want_mode
    with pytest.raises(ValueError):
        loader_of(ds, idx, 4, "sometimes")


@pytest.mark.parametrize("n", [1, 2, 5, 128])
def test_antithetic_t(G, n):
    from sfron import ddpm_data
    t = ddpm_data.antithetic_t(torch.from_numpy(G[f"t_half_{n}"]), int(G["t_T"]), n)
    assert t.dtype == torch.int64 and t.tolist() == G[f"t_{n}"].tolist()


def test_draw_order_and_rank_union():
    """the per-batch draws come in the documented order, and the ranks' slices of the global batch tile it"""
    ds = tiny_dataset()
    idx = torch.arange(23)
    ld = loader_of(ds, idx, 5, None, uniform_dequantization=True, gaussian_dequantization=True)
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(23, generator=g)
    batches = list(ld.index_batches())                       # consumes the permutation only
    assert batches[0][0].tolist() == perm[:5].tolist()
    u, n, e, t_half = ld.draws(5)
    shape = (5, 3, 4, 4)
    assert torch.equal(u, torch.rand(shape, generator=g)) and torch.equal(n, torch.randn(shape, generator=g))
    assert torch.equal(e, torch.randn(shape, generator=g)) and torch.equal(t_half, torch.randint(0, 1000, (3,), generator=g))
    world = 3
    full = [b[0] for b in loader_of(ds, idx, 5, None).index_batches()]
    for k, whole in enumerate(full):
        got = torch.empty_like(whole)
        for r in range(world):
            ld = loader_of(ds, idx, 5, None, rank=r, world=world)
            got[r::world] = ld.rank_rows(list(ld.index_batches())[k][0])
        assert torch.equal(got, whole)


def test_cycle_runs_past_an_epoch():
    from sfron import ddpm_data

    class Two:
        def __iter__(self):
            return iter([1, 2])
    it = ddpm_data.cycle(Two())
    assert [next(it) for _ in range(5)] == [1, 2, 1, 2, 1]


# ------------------------------------------------------------------------------------------------ the readers
def test_load_cifar10(tmp_path):
    from sfron import ddpm_data
    with pytest.raises(FileNotFoundError, match=re.escape(str(tmp_path))):
        ddpm_data.load_cifar10(str(tmp_path))
    root = tmp_path / "cifar-10-batches-py"
    root.mkdir()
    rng = np.random.default_rng(0)
    want_x, want_y = [], []
    for name in list(ddpm_data.CIFAR10_TRAIN) + list(ddpm_data.CIFAR10_TEST):
        data = rng.integers(0, 256, (3, 3072), dtype=np.uint8)
        labels = rng.integers(0, 10, 3).tolist()
        with open(root / name, "wb") as f:
            pickle.dump({"data": data, "labels": labels, "filenames": ["a", "b", "c"]}, f)
        want_x.append(data)
        want_y.extend(labels)
    x, y = ddpm_data.load_cifar10(str(tmp_path), train=True)
    assert x.dtype == np.uint8 and x.shape == (15, 3, 32, 32) and y.dtype == np.int64
    assert np.array_equal(x.reshape(15, 3072), np.vstack(want_x[:5])) and y.tolist() == want_y[:15]
    assert x[4, 1, 2, 3] == want_x[1][1, 1024 + 2 * 32 + 3]                      # planar RGB, rows of 32
    x, y = ddpm_data.load_cifar10(str(tmp_path), train=False)
    assert np.array_equal(x.reshape(3, 3072), want_x[5]) and y.tolist() == want_y[15:]
    with pytest.raises(NotImplementedError, match="STL10"):
        ddpm_data.load_dataset(NS(data=NS(dataset="STL10", path=str(tmp_path))))


def test_load_image_folder(tmp_path):
    from PIL import Image
    from sfron import ddpm_data
    rng = np.random.default_rng(1)
    files = {"b/2.png": (8, 8), "b/10.png": (8, 8), "a/x.png": (20, 16), "a/sub/y.png": (8, 8), "c/z.bmp": (8, 8)}      # (w, h)
    arrays = {}
    for rel, (w, h) in files.items():
        os.makedirs(tmp_path / os.path.dirname(rel), exist_ok=True)
        arrays[rel] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(arrays[rel]).save(tmp_path / rel)
    (tmp_path / "a" / "notes.txt").write_text("not an image")
    Image.fromarray(arrays["b/2.png"][:, :, 0]).save(tmp_path / "b" / "grey.png")        # mode L: .convert("RGB")
    with pytest.raises(ValueError, match="one size"):
        ddpm_data.load_image_folder(str(tmp_path), 8)                            # a/x.png becomes 10 x 8
    os.remove(tmp_path / "a" / "x.png")
    Image.fromarray(rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)).save(tmp_path / "a" / "x.png")
    big = np.array(Image.open(tmp_path / "a" / "x.png").convert("RGB"))
    x, y = ddpm_data.load_image_folder(str(tmp_path), 8)
    # ImageFolder: classes sorted; per class the walk's directories sorted, files sorted as strings ("10.png" < "2.png")
    order = ["a/x.png", "a/sub/y.png", "b/10.png", "b/2.png", "b/grey.png", "c/z.bmp"]
    assert x.shape == (6, 3, 8, 8) and x.dtype == np.uint8 and y.tolist() == [0, 0, 1, 1, 1, 2]
    for k, rel in enumerate(order):
        if rel == "a/x.png":
            want = np.array(Image.fromarray(big).resize((8, 8), Image.BILINEAR))          # the resize, Pillow's bytes
        elif rel == "b/grey.png":
            want = np.repeat(arrays["b/2.png"][:, :, :1], 3, axis=2)
        else:
            want = arrays[rel]                                                            # the short side matches: untouched
        assert np.array_equal(x[k], want.transpose(2, 0, 1)), rel
    with pytest.raises(FileNotFoundError, match="nowhere"):
        ddpm_data.load_image_folder(str(tmp_path / "nowhere"), 8)


# ------------------------------------------------------------------------------------------------ the entry point
def test_prototype_in_header_and_binding_and_abi_stays_16():
    from sfron import _lib
    L = _lib.lib()
    assert L.sfron_abi_version() == 17 and _lib.ABI_VERSION == 17
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfron.h")).read(), flags=re.S)
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int}
    assert getattr(L, NAME) is not None and NAME in _lib.declared_symbols()
    m = re.search(r"\bint\s+" + NAME + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m, f"{NAME} is not declared in include/sfron.h"
    params = [p.strip() for p in m.group(1).split(",")]
    res, args = _lib._PROTOS[NAME]
    assert res is ctypes.c_int and len(args) == len(params)
    for at, p in zip(args, params):
        assert at is (ctypes.c_void_p if "*" in p else kinds[p.split()[0]]), (p, at)
    assert (_lib.DDPM_DATA_PLAIN, _lib.DDPM_DATA_RESCALED, _lib.DDPM_DATA_LOGIT) == (0, 1, 2)


_P = [0x1000 * (k + 1) for k in range(11)]
GOOD = dict(images=_P[0], labels=_P[1], N=23, C=3, H=8, W=12, idx=_P[2], flip=_P[3], B=5, uni=1, u=_P[4], gau=1, n=_P[5], mode=2,
            mean=_P[6], t_half=_P[7], T=1000, x0=_P[8], c=_P[9], t=_P[10])
BAD = [dict(images=None), dict(labels=None), dict(idx=None), dict(x0=None), dict(c=None), dict(N=0), dict(C=0), dict(H=-1), dict(W=0),
       dict(B=0), dict(B=1 << 20, C=8, H=16, W=16), dict(T=0), dict(T=-5), dict(u=None), dict(n=None), dict(t=None), dict(t_half=None),
       dict(mode=3), dict(mode=-1)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_refusals_come_before_any_launch(bad):
    """every pointer is made up: a call that got as far as a launch would not return SFRON_ERR_ARG"""
    from sfron import _lib
    a = dict(GOOD, **bad)
    assert _lib.lib().sfron_ddpm_batch_u8(*[a[k] for k in GOOD], None) == _lib.ERR_ARG
