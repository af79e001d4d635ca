"""GPU: ADM's centre crop on the MI355X, a whole batch per launch -- sfron_image_resample_batch_u8 against Pillow's center_crop_arr bit
for bit, the generic entry point against Image.resize windows, its refusals, resample.center_crop_gpu, and the DiT image loader /
encode_image_folder with gpu_resize on against the host route.

Every comparison is bitwise: the kernels are integer arithmetic specified bit for bit, and the loaders hand identical bytes to the same
encoder, whose repeatability the suite already asserts bitwise (test_gpu_vae.py::test_chunked_batch_agrees_and_calls_repeat_bitwise)."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from test_center_crop_cpu import SHAPES, S, pillow_crop, source
from test_gpu_sd_front_end import GPU_CASES, GUARD, _guarded, _guards_intact, _window
from test_sd_front_end_cpu import FILTERS, PIL_FILTER, case_image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def crops():
    """The sources and Pillow's crops of the 19 shapes, computed once; read-only."""
    srcs = [source(ci) for ci in range(len(SHAPES))]
    return srcs, [pillow_crop(a) for a in srcs]


def _pool_at_every_alignment(srcs):
    """Byte offsets that put source i at residue (5 i + 1) mod 16 (every residue mod 4 and mod 16 over the batch), and the pool."""
    offs, at = [], 0
    for i, a in enumerate(srcs):
        at += ((5 * i + 1) - at) % 16
        offs.append(at)
        at += a.size
    pool = np.full(at + 3, GUARD, dtype=np.uint8)
    for a, o in zip(srcs, offs):
        pool[o:o + a.size] = a.reshape(-1)
    return offs, pool


# ------------------------------------------------------------------------------------------------ 1. the entry point
def test_whole_batch_equals_pillow_bit_for_bit_between_guards(crops):
    from sfron import resample
    srcs, want = crops
    offs, pool_h = _pool_at_every_alignment(srcs)
    assert {o % 4 for o in offs} == {0, 1, 2, 3}
    plans = [resample.center_crop_plan(a.shape[1], a.shape[0], S) for a in srcs]
    bp = resample.plan_batch([p.stages for p in plans], src_off=offs)
    assert bp.n_levels == 8                                                     # three halvings in the batch: 2 * (1 + 3) launches for 19 images
    pool = torch.from_numpy(pool_h).to(DEV)
    wbuf, work = _guarded(bp.work_bytes, 13)
    obuf, out = _guarded(bp.out_bytes, 7)
    assert resample.image_resample_batch_u8(bp, pool, work, out) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(len(srcs), S, S, 3)
    for ci, w in enumerate(want):
        assert np.array_equal(got[ci], w), (SHAPES[ci], int(np.abs(got[ci].astype(int) - w).max()))
    assert _guards_intact(wbuf, 13, bp.work_bytes) and _guards_intact(obuf, 7, bp.out_bytes)
    assert np.array_equal(pool.cpu().numpy(), pool_h)
    none = [ci for ci, p in enumerate(plans) if p.halvings == 0]
    assert len(none) == 6 and resample.plan_batch([plans[ci].stages for ci in none]).n_levels == 2


def test_batches_of_one_and_three_and_reversed_give_the_same_bytes(crops):
    from sfron import resample
    srcs, want = crops
    n = len(srcs)
    full = resample.center_crop_gpu(srcs, S, device=DEV)
    assert full.dtype == torch.uint8 and tuple(full.shape) == (n, S, S, 3) and full.is_cuda
    assert np.array_equal(full.cpu().numpy(), np.stack(want))
    rev = resample.center_crop_gpu([Image.fromarray(a) for a in srcs[::-1]], S, device=DEV)          # PIL images in, reversed
    assert torch.equal(rev.flip(0), full)
    for lo in range(0, n, 3):
        assert torch.equal(resample.center_crop_gpu(srcs[lo:lo + 3], S, device=DEV), full[lo:lo + 3]), lo
    for ci in (0, 1, 8, 13, 17):
        assert torch.equal(resample.center_crop_gpu([srcs[ci]], S, device=DEV)[0], full[ci]), ci
    out = torch.zeros(n, S, S, 3, dtype=torch.uint8, device=DEV)
    assert resample.center_crop_gpu(srcs, S, out=out) is out and torch.equal(out, full)
    with pytest.raises(ValueError):
        resample.center_crop_gpu(srcs, S, out=out[:3])
    with pytest.raises(ValueError):
        resample.center_crop_gpu([Image.fromarray(srcs[0]).convert("L")], S, device=DEV)


def test_generic_batch_mixes_filters_and_a_span_beyond_the_staging():
    """One stage per image: windows of Image.resize at the shapes of the single-image kernel test, the filter changing from image to
    image; (5, 12001) -> (5, 4) under lanczos does not fit the staged span and reads global memory."""
    from sfron import resample
    chains, srcs, want = [], [], []
    for ci, ((H, W), (oh, ow)) in enumerate(GPU_CASES):
        filt = "lanczos" if (H, W) == (5, 12001) else FILTERS[ci % len(FILTERS)]
        a = case_image(ci, H, W)
        (fy, ny), (fx, nx) = _window(oh), _window(ow)
        want.append(np.asarray(Image.fromarray(a).resize((ow, oh), PIL_FILTER[filt]))[fy:fy + ny, fx:fx + nx])
        chains.append([resample.Stage(resample.resample_tables(W, ow, filt, fx, nx), resample.resample_tables(H, oh, filt, fy, ny), 0, 0, W, H)])
        srcs.append(a)
    assert len({c[0].tx.ksize for c in chains}) > 3
    offs, pool_h = _pool_at_every_alignment(srcs)
    bp = resample.plan_batch(chains, src_off=offs)
    assert bp.n_levels == 2
    wbuf, work = _guarded(bp.work_bytes, 5)
    obuf, out = _guarded(bp.out_bytes, 3)
    assert resample.image_resample_batch_u8(bp, torch.from_numpy(pool_h).to(DEV), work, out) == 0
    torch.cuda.synchronize()
    got, at = out.cpu().numpy(), 0
    for ci, w in enumerate(want):
        g = got[at:at + w.size].reshape(w.shape)
        assert np.array_equal(g, w), (ci, int(np.abs(g.astype(int) - w).max()))
        at += w.size
    assert at == bp.out_bytes and _guards_intact(wbuf, 5, bp.work_bytes) and _guards_intact(obuf, 3, bp.out_bytes)


def test_entry_point_refusals_leave_the_outputs_untouched(crops):
    from sfron import _lib, resample
    from sfron._lib import ptr, stream_ptr
    srcs, want = crops
    pick = [3, 1, 6]                                                           # one, no and two halvings
    bp = resample.plan_batch([resample.center_crop_plan(srcs[ci].shape[1], srcs[ci].shape[0], S).stages for ci in pick])
    host = np.zeros(bp.host_bytes, dtype=np.uint8)
    bp.fill(host, [srcs[ci] for ci in pick])
    pool = torch.from_numpy(host[bp.pool_at:]).to(DEV)
    tables, passes = torch.from_numpy(bp.tables).to(DEV), torch.from_numpy(bp.passes).to(DEV)
    wbuf, work = _guarded(bp.work_bytes, 4)
    obuf, out = _guarded(bp.out_bytes, 4)
    untouched = lambda: bool((wbuf == GUARD).all()) and bool((obuf == GUARD).all())
    E, L = _lib.ERR_ARG, _lib.lib()
    lf, lr, lc = bp.level_first, bp.level_rows, bp.level_cols
    a = lambda v: v.ctypes.data
    good = [ptr(pool), bp.pool_bytes, ptr(tables), bp.tables.size, ptr(passes), bp.passes.shape[0], a(lf), a(lr), a(lc), bp.n_levels,
            ptr(work), bp.work_bytes, ptr(out), bp.out_bytes]
    for pos in (0, 2, 4, 6, 7, 8, 10, 12):                                     # every pointer, null
        bad = list(good)
        bad[pos] = None
        assert L.sfron_image_resample_batch_u8(*bad, stream_ptr()) == E, pos
    for pos in (1, 3, 5, 9, 11, 13):                                           # every count and size, zero and negative
        for v in (0, -1):
            bad = list(good)
            bad[pos] = v
            assert L.sfron_image_resample_batch_u8(*bad, stream_ptr()) == E, (pos, v)
    for arr_pos, edit in ((6, lambda v: v.__setitem__(2, v[1])), (6, lambda v: v.__setitem__(0, 1)), (6, lambda v: v.__setitem__(-1, v[-1] + 1)),
                          (7, lambda v: v.__setitem__(1, 0)), (8, lambda v: v.__setitem__(0, -3))):       # level lists that do not ascend / extents
        arr = [lf, lr, lc][arr_pos - 6].copy()
        edit(arr)
        bad = list(good)
        bad[arr_pos] = a(arr)
        assert L.sfron_image_resample_batch_u8(*bad, stream_ptr()) == E, arr_pos
    bad = list(good)
    bad[9] = bp.n_levels - 1                                                   # an odd level count
    assert L.sfron_image_resample_batch_u8(*bad, stream_ptr()) == E
    # sizes one byte below what the largest extents imply
    for pos, need in ((1, 3 * int(lr[0])), (11, 3 * int(max(lr[0::2].max(), lc[0::2].max()))), (13, max(3 * int(lr[-1]), int(lc[-1])))):
        bad = list(good)
        bad[pos] = need - 1
        assert L.sfron_image_resample_batch_u8(*bad, stream_ptr()) == E, pos
    torch.cuda.synchronize()
    assert untouched()
    assert L.sfron_image_resample_batch_u8(*good, stream_ptr()) == 0           # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(len(pick), S, S, 3)
    for i, ci in enumerate(pick):
        assert np.array_equal(got[i], want[ci]), ci
    assert _guards_intact(wbuf, 4, bp.work_bytes) and _guards_intact(obuf, 4, bp.out_bytes)


# ------------------------------------------------------------------------------------------------ 2. the loaders
@pytest.fixture(scope="module")
def folder_and_encoder(golden_dir, tmp_path_factory):
    from test_gpu_vae import _image_folder, small_encoder
    fx = dict(np.load(os.path.join(golden_dir, "vae_encoder.npz")))
    return _image_folder(tmp_path_factory.mktemp("crop") / "data"), small_encoder(fx)


@pytest.mark.parametrize("rank,world", ((0, 1), (0, 2), (1, 2)))
def test_image_loader_gpu_resize_equals_the_host_route(folder_and_encoder, rank, world):
    from sfron import latents
    data, enc = folder_and_encoder
    kw = dict(seed=9, image_size=64, flip_prob=0.5, workers=4, rank=rank, world=world)
    host = latents.UnlearnImageLoader(data, 1, enc, 4, gpu_resize=False, **kw)
    gpu = latents.UnlearnImageLoader(data, 1, enc, 4, gpu_resize=True, **kw)
    for step in range(3):
        for stream in ("forget", "remain"):
            a, b = host.next(stream), gpu.next(stream)
            for k in ("x0", "y", "t", "noise", "drop"):
                assert torch.equal(a[k], b[k]), (step, stream, k)
    # the host side: the decoded sources in place of the cropped images, every other field unchanged
    ha, hb = host.host_batch("remain", 1), gpu.host_batch("remain", 1)
    assert sorted(set(ha) - {"images"}) == sorted(set(hb) - {"sources"}) and "images" not in hb and "sources" not in ha
    for k in ("flip", "eps", "y", "t", "noise", "drop"):
        assert torch.equal(ha[k], hb[k]), k
    assert len(hb["sources"]) == ha["images"].shape[0] == 4 // world
    for src, img in zip(hb["sources"], ha["images"]):
        assert src.dtype == np.uint8 and src.ndim == 3 and np.array_equal(pillow_crop(src, 64), img.numpy())
    assert len({s.shape for s in hb["sources"]}) > 1


def test_encode_image_folder_writes_the_same_shards_on_both_routes(folder_and_encoder, tmp_path):
    from sfron import latents
    data, enc = folder_and_encoder
    counts = {}
    for route in (False, True):
        counts[route] = latents.encode_image_folder(data, enc, str(tmp_path / f"cache{int(route)}"), image_size=64, batch=4, workers=4,
                                                    gpu_resize=route)
    assert counts[False] == counts[True] == {"cat": 5, "dog": 4, "eel": 6}
    for name in ("cat.npy", "dog.npy", "eel.npy", "index.json"):
        a, b = (open(tmp_path / f"cache{r}" / name, "rb").read() for r in (0, 1))
        assert a == b and len(a) > 0, name
