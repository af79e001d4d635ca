"""GPU: sfron_ddpm_batch_u8 (csrc/ddpm_data.hip) against the torch expression of the reference on the same inputs, evaluated on the CPU
(ToTensor's division runs there in the reference), with the outputs in guarded buffers.

Per (C, H, W) and N: B = 1, 2, 5, 128; flip flags all 0, all 1, mixed (and no flag vector); all 24 forms of data_transform.  The 16 forms
without the logit are bit-equal.  The 8 logit forms: the fp32 ``image`` is exact, ref64 is the float64 log / log1p of it, ref32 the same
in torch fp32 on the CPU, under ``dit_rows_ref.bound32`` with its MARGIN (``ddpm_data_ref.check_logit``: over the elements the reference
leaves finite; the others must be the same non-finite values).  c and t are exact (t against the torch cat / slice).

Measured on an MI355X (the DDPM-DATA-METRIC lines, -s): over all shapes the logit forms' largest error is 4.4 times the CPU fp32
expression's own distance from float64 and 2.9 ulps of the largest value (about 14): inside bound32's MARGIN * yard + 4 ulps."""
import pytest
import torch

import dit_rows_ref as R
from ddpm_data_ref import FORMS, check_logit, form_config, logit_refs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 1000
# the vector path at CIFAR's shape, a small aligned case, W % 4 == 2, an odd width with one channel, and 16 x 16 (768 elements: less than
# one workgroup's chunk; 3072 is three chunks)
SHAPES = [(3, 32, 32), (3, 8, 12), (3, 6, 10), (1, 5, 7), (3, 16, 16)]
BATCHES = (1, 2, 5, 128)


def bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def make_dataset(N, C, H, W, seed=0, offset=0):
    from sfron import ddpm_data
    g = torch.Generator().manual_seed(1000 * seed + 97 * N + 31 * C + 7 * H + W)
    img = torch.randint(0, 256, (N, C, H, W), generator=g, dtype=torch.uint8)
    img.view(-1)[:min(256, img.numel())] = torch.arange(min(256, img.numel()), dtype=torch.uint8)     # every byte value where it fits
    labels = torch.randint(0, 10, (N,), generator=g)
    ds = ddpm_data.ResidentDataset(img, labels, device=DEV)
    if offset:            # the same bytes at an address that is not 4-byte aligned
        raw = torch.empty(img.numel() + 16, dtype=torch.uint8, device=DEV)
        raw[offset:offset + img.numel()] = ds.images.view(-1)
        ds.images = raw[offset:offset + img.numel()].view(N, C, H, W)
        assert ds.images.data_ptr() % 4 == offset % 4 and ds.images.is_contiguous()
    return ds, img, labels


def indices(N, B, g):
    """0, N - 1 and a repeat, unsorted, as far as B has room"""
    idx = torch.randint(0, N, (B,), generator=g)
    if B >= 2:
        idx[0], idx[B - 1] = N - 1, 0
    if B >= 3:
        idx[B // 2] = idx[0]
    return idx


def flag_sets(B, g):
    return {"none": None, "zeros": torch.zeros(B, dtype=torch.uint8), "ones": torch.ones(B, dtype=torch.uint8),
            "mixed": (torch.arange(B) % 2 == 0).to(torch.uint8) * 7}              # any non-zero byte is a flip


def cpu_image(img, idx, flip):
    x = img[idx]
    if flip is not None:
        x = torch.where(flip.bool()[:, None, None, None], x.flip(3), x)
    return x.float() / 255


@pytest.mark.parametrize("N", [1, 23])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_the_torch_expression(shape, N):
    from sfron import ddpm_data
    C, H, W = shape
    ds, img, labels = make_dataset(N, C, H, W)
    g = torch.Generator().manual_seed(N + W)
    mean = torch.rand(C, H, W, generator=g)
    nonfinite = launches = 0
    for B in BATCHES:
        idx = indices(N, B, g)
        u, n = torch.rand(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
        t_half = torch.randint(0, T, (B // 2 + 1,), generator=g)
        want_t = torch.cat([t_half, T - t_half - 1], dim=0)[:B]
        x0, ck_x = R.guarded((B, C, H, W), torch.float32)
        c, ck_c = R.guarded((B,), torch.int64)
        t, ck_t = R.guarded((B,), torch.int64)
        ud, nd, td, idxd = u.to(DEV), n.to(DEV), t_half.to(DEV), idx.to(DEV)
        for fname, flip in flag_sets(B, g).items():
            X = cpu_image(img, idx, flip)
            for uq, gq, mode, with_mean in FORMS:
                cfg = form_config(uq, gq, mode, mean if with_mean else None)
                name = f"{shape} N{N} B{B} flip {fname} u{uq} g{gq} {mode} mean{with_mean}"
                x0.fill_(123.0), c.fill_(-7), t.fill_(-7)
                ddpm_data.ddpm_batch_u8(ds, idxd, None if flip is None else flip.to(DEV), cfg, T, u=ud, n=nd, t_half=td, out=(x0, c, t))
                launches += 1
                ck_x(name), ck_c(name), ck_t(name)
                assert torch.equal(c.cpu(), labels[idx]) and torch.equal(t.cpu(), want_t), name
                un, nn = (u if uq else None), (n if gq else None)
                if mode != "logit":
                    assert torch.equal(bits(x0), bits(ddpm_data.data_transform(cfg, X, u=un, n=nn))), name
                else:
                    nonfinite += check_logit(x0, logit_refs(cfg, X, un, nn, torch.float64), logit_refs(cfg, X, un, nn, torch.float32), name)
    assert launches == len(BATCHES) * 4 * 24
    rec = [d for k, d in R.RECORD.items() if k.startswith(f"{shape} N{N} ")]
    print(f"DDPM-DATA-METRIC {shape} N{N}: {launches} launches, {nonfinite} non-finite logit elements matched, logit forms worst "
          f"err / yard {max(d.get('ratio', 0.0) for d in rec):.3f}, worst err in ulps of the largest value {max(d['ulps_of_max'] for d in rec):.3f}")


def test_without_t_and_two_runs_give_equal_bits():
    from sfron import ddpm_data
    ds, img, labels = make_dataset(23, 3, 32, 32, seed=1)
    g = torch.Generator().manual_seed(5)
    B = 128
    idx, flip = indices(23, B, g).to(DEV), (torch.rand(B, generator=g) < 0.5).to(torch.uint8).to(DEV)
    u, n = torch.rand(B, 3, 32, 32, generator=g).to(DEV), torch.randn(B, 3, 32, 32, generator=g).to(DEV)
    cfg = form_config(1, 1, "logit", torch.rand(3, 32, 32, generator=g))
    t_half = torch.randint(0, T, (B // 2 + 1,), generator=g).to(DEV)
    a = ddpm_data.ddpm_batch_u8(ds, idx, flip, cfg, T, u=u, n=n, t_half=t_half)
    b = ddpm_data.ddpm_batch_u8(ds, idx, flip, cfg, T, u=u, n=n, t_half=t_half)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    x0, c, t = ddpm_data.ddpm_batch_u8(ds, idx, flip, cfg, T, u=u, n=n)            # t_half and t both absent
    assert t is None and torch.equal(bits(x0), bits(a[0])) and torch.equal(c, a[1])
    # the torch route on the device (batch_torch): the same 16 exact forms hold there too for this form's exact part
    cfg2 = form_config(1, 1, "rescaled")
    got = ddpm_data.ddpm_batch_u8(ds, idx, flip, cfg2, T, u=u, n=n, t_half=t_half)
    want = ddpm_data.batch_torch(ds, idx, flip, cfg2, T, u=u, n=n, t_half=t_half)
    assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


@pytest.mark.parametrize("offset", [1, 2])
def test_misaligned_rows_take_the_one_pixel_path_with_the_same_bits(offset):
    from sfron import ddpm_data
    ds, img, labels = make_dataset(5, 3, 8, 12, seed=2)
    ds_off, _, _ = make_dataset(5, 3, 8, 12, seed=2, offset=offset)
    g = torch.Generator().manual_seed(9)
    idx = torch.tensor([4, 0, 2, 4, 1]).to(DEV)
    flip = torch.tensor([1, 0, 1, 0, 1], dtype=torch.uint8).to(DEV)
    u = torch.rand(5, 3, 8, 12, generator=g).to(DEV)
    cfg = form_config(1, 0, "rescaled")
    x0, ck = R.guarded((5, 3, 8, 12), torch.float32)
    c, t = torch.empty(5, dtype=torch.int64, device=DEV), None
    ddpm_data.ddpm_batch_u8(ds_off, idx, flip, cfg, T, u=u, out=(x0, c, t))
    ck("misaligned images")
    want = ddpm_data.ddpm_batch_u8(ds, idx, flip, cfg, T, u=u)
    assert torch.equal(bits(x0), bits(want[0])) and torch.equal(c, want[1])
    # a misaligned u (4-byte aligned only)
    raw = torch.empty(u.numel() + 4, dtype=torch.float32, device=DEV)
    raw[1:1 + u.numel()] = u.view(-1)
    u_off = raw[1:1 + u.numel()].view(u.shape)
    assert u_off.data_ptr() % 16 == 4
    got = ddpm_data.ddpm_batch_u8(ds, idx, flip, cfg, T, u=u_off)
    assert torch.equal(bits(got[0]), bits(want[0]))


def test_refusals_leave_the_outputs_untouched():
    from sfron import _lib
    from sfron._lib import ptr
    ds, img, labels = make_dataset(23, 3, 8, 12)
    B = 5
    idx, flip = torch.zeros(B, dtype=torch.int64, device=DEV), torch.zeros(B, dtype=torch.uint8, device=DEV)
    u, n = torch.zeros(B, 3, 8, 12, device=DEV), torch.zeros(B, 3, 8, 12, device=DEV)
    mean, t_half = torch.zeros(3, 8, 12, device=DEV), torch.zeros(B // 2 + 1, dtype=torch.int64, device=DEV)
    x0, ck_x = R.guarded((B, 3, 8, 12), torch.float32)
    c, ck_c = R.guarded((B,), torch.int64)
    t, ck_t = R.guarded((B,), torch.int64)
    good = dict(images=ptr(ds.images), labels=ptr(ds.labels), N=23, C=3, H=8, W=12, idx=ptr(idx), flip=ptr(flip), B=B, uni=1, u=ptr(u), gau=1,
                n=ptr(n), mode=2, mean=ptr(mean), t_half=ptr(t_half), T=T, x0=ptr(x0), c=ptr(c), t=ptr(t))
    bad = [dict(images=None), dict(labels=None), dict(idx=None), dict(x0=None), dict(c=None), dict(N=0), dict(C=0), dict(H=0), dict(W=-3),
           dict(B=0), dict(B=-1), dict(B=1 << 24), dict(T=0), dict(u=None), dict(n=None), dict(t=None), dict(t_half=None), dict(mode=3)]
    L = _lib.lib()
    for b in bad:
        a = dict(good, **b)
        assert L.sfron_ddpm_batch_u8(*[a[k] for k in good], _lib.stream_ptr()) == _lib.ERR_ARG, b
    torch.cuda.synchronize()
    for ck in (ck_x, ck_c, ck_t):
        R.untouched(ck, "refused call")


@pytest.mark.parametrize("shape", [(3, 8, 12), (1, 5, 7)], ids=["vector", "one-pixel"])
def test_an_index_outside_the_dataset_reads_nothing(shape):
    """idx is device data: a bad value cannot be refused.  Its row is NaN, its label -1, every other row and everything outside the outputs
    is as without it, and StepGuard names the label."""
    from sfron import ddpm_data, guard
    from sfron._lib import SfronError
    C, H, W = shape
    N, B = 23, 6
    ds, img, labels = make_dataset(N, C, H, W, seed=3)
    good = torch.tensor([22, 0, 5, 5, 17, 3])
    bad_rows = {1: -1, 3: N, 4: 1 << 40}
    idx = good.clone()
    for r, v in bad_rows.items():
        idx[r] = v
    g = torch.Generator().manual_seed(4)
    u = torch.rand(B, C, H, W, generator=g).to(DEV)
    flip = torch.tensor([1, 1, 0, 0, 1, 0], dtype=torch.uint8).to(DEV)
    t_half = torch.randint(0, T, (B // 2 + 1,), generator=g).to(DEV)
    cfg = form_config(1, 0, "rescaled", torch.rand(C, H, W, generator=g))
    want = ddpm_data.ddpm_batch_u8(ds, good.to(DEV), flip, cfg, T, u=u, t_half=t_half)
    x0, ck_x = R.guarded((B, C, H, W), torch.float32)
    c, ck_c = R.guarded((B,), torch.int64)
    t, ck_t = R.guarded((B,), torch.int64)
    ddpm_data.ddpm_batch_u8(ds, idx.to(DEV), flip, cfg, T, u=u, t_half=t_half, out=(x0, c, t))
    ck_x("bad index"), ck_c("bad index"), ck_t("bad index")
    for r in range(B):
        if r in bad_rows:
            assert bool(torch.isnan(x0[r]).all()) and int(c[r]) == -1, r
        else:
            assert torch.equal(bits(x0[r]), bits(want[0][r])) and int(c[r]) == int(want[1][r]), r
    assert torch.equal(t, want[2])
    sg = guard.StepGuard(DEV)
    sg.check_inputs(c.clone(), t.clone(), 10, T)
    sg.publish(0)
    with pytest.raises(SfronError, match="label outside"):
        sg.poll(block=True)


def test_loader_batches_are_reproducible_with_plain_torch_calls():
    """the documented order of draws: frozen flags at construction, a permutation per epoch, then per batch u, n, e, t_half.  23 images
    at batch 5 over two epochs: short last batches, a fresh permutation"""
    from sfron import ddpm_data
    ds, img, labels = make_dataset(23, 3, 16, 16, seed=5)
    remain, forget = ddpm_data.split_forget(torch.arange(23) % 4, 1)              # 17 and 6 images: short last batches of 2 and 1
    assert len(remain) == 17
    cfg = form_config(1, 1, "rescaled", random_flip=True)
    for flip_mode in ("frozen", "per_access", None):
        ld = ddpm_data.DDPMBatchLoader(ds, remain, 5, cfg, T, torch.Generator(device=DEV).manual_seed(11), flip=flip_mode)
        g = torch.Generator(device=DEV).manual_seed(11)
        ind = remain.to(DEV)
        n = len(remain)
        frozen = (torch.rand(n, generator=g, device=DEV) < 0.5).to(torch.uint8) if flip_mode == "frozen" else None
        assert len(ld) == (n + 4) // 5
        for epoch in range(2):
            perm = torch.randperm(n, generator=g, device=DEV)
            seen = 0
            for i, batch in enumerate(ld):
                pos = perm[5 * i:5 * i + 5]
                B = pos.shape[0]
                flip = frozen[pos] if flip_mode == "frozen" else None
                if flip_mode == "per_access":
                    flip = (torch.rand(B, generator=g, device=DEV) < 0.5).to(torch.uint8)
                u = torch.rand(B, 3, 16, 16, generator=g, device=DEV)
                nz = torch.randn(B, 3, 16, 16, generator=g, device=DEV)
                e = torch.randn(B, 3, 16, 16, generator=g, device=DEV)
                t_half = torch.randint(0, T, (B // 2 + 1,), generator=g, device=DEV)
                x0, c, t = ddpm_data.batch_torch(ds, ind[pos], flip, cfg, T, u=u, n=nz, t_half=t_half)
                assert sorted(batch) == ["c", "e", "t", "x0"]
                assert torch.equal(bits(batch["x0"]), bits(x0)) and torch.equal(batch["c"], c) and torch.equal(batch["t"], t)
                assert torch.equal(batch["e"], e) and batch["x0"].shape == (B, 3, 16, 16)
                seen += B
            assert seen == n and i == len(ld) - 1 and B == n % 5 == 2
    # rank / world: the ranks' rows tile the world = 1 batch
    full = next(iter(ddpm_data.DDPMBatchLoader(ds, remain, 5, cfg, T, torch.Generator(device=DEV).manual_seed(11), flip="frozen")))
    for r in range(2):
        part = next(iter(ddpm_data.DDPMBatchLoader(ds, remain, 5, cfg, T, torch.Generator(device=DEV).manual_seed(11), flip="frozen", rank=r,
                                                   world=2)))
        for k in ("x0", "c", "t", "e"):
            assert torch.equal(part[k], full[k][r::2]), (r, k)


def test_image_folder_resize_on_the_device_gives_the_host_route_bytes(tmp_path):
    import os

    import numpy as np
    from PIL import Image
    from sfron import ddpm_data
    rng = np.random.default_rng(2)
    for rel, (w, h) in {"a/big.png": (24, 24), "a/same.png": (12, 12), "b/wide.png": (20, 20)}.items():
        os.makedirs(tmp_path / os.path.dirname(rel), exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp_path / rel)
    host_x, host_y = ddpm_data.load_image_folder(str(tmp_path), 12)
    dev_x, dev_y = ddpm_data.load_image_folder(str(tmp_path), 12, device=DEV)
    assert host_x.shape == (3, 3, 12, 12) and np.array_equal(dev_x, host_x) and dev_y.tolist() == host_y.tolist() == [0, 0, 1]
