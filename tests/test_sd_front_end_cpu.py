"""CPU: the SD image / prompt front end -- Pillow's resampling tables restated on the host (sfron.resample), the transform of the SD
scripts against the Pillow composition, LatentDiffusion.get_input's contract over stub encoders, the concept image loader's batching
and the new ABI entry.  Pillow itself is the yardstick of the tables: the integer arithmetic is deterministic, so equality is bitwise."""
import os
import re
import types

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, W) -> (oh, ow): down- and up-scaling, one axis unchanged, both unchanged, bounds clipped at both edges ((9, 7) -> (64, 64)),
# a heavy down-scale ((140, 71) -> (12, 6): bicubic ksize 49, lanczos 73)
CASES = [((37, 53), (16, 23)), ((53, 37), (64, 45)), ((97, 131), (32, 43)), ((16, 16), (16, 40)), ((200, 301), (64, 96)), ((9, 7), (64, 64)),
         ((333, 500), (128, 192)), ((64, 64), (64, 64)), ((140, 71), (12, 6))]
FILTERS = ("box", "bilinear", "bicubic", "lanczos")
PIL_FILTER = {"box": Image.BOX, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


def case_image(ci, H, W):
    """Random bytes; every other case quantised to {0, 255} so that both ends of the clamp are reached."""
    a = np.random.default_rng(100 + ci).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    return ((a > 127) * 255).astype(np.uint8) if ci % 2 else a


def apply_spec(src, kx, bx, ky, by):
    """The two passes exactly as specified: ss = 2^21 + sum src[xmin + x] * k[x] in int32, out = clamp(ss >> 22, 0, 255); horizontal
    first, to uint8, over the source rows the vertical pass reads."""
    y0, y1 = int(by[0, 0]), int(by[-1, 0] + by[-1, 1])
    tmp = np.zeros((y1 - y0, bx.shape[0], 3), dtype=np.uint8)
    for xx in range(bx.shape[0]):
        lo, n = int(bx[xx, 0]), int(bx[xx, 1])
        ss = (1 << 21) + (src[y0:y1, lo:lo + n].astype(np.int32) * kx[xx, :n].astype(np.int32)[None, :, None]).sum(axis=1, dtype=np.int32)
        tmp[:, xx] = np.clip(ss >> 22, 0, 255)
    out = np.zeros((by.shape[0], bx.shape[0], 3), dtype=np.uint8)
    for yy in range(by.shape[0]):
        lo, n = int(by[yy, 0]) - y0, int(by[yy, 1])
        ss = (1 << 21) + (tmp[lo:lo + n].astype(np.int32) * ky[yy, :n].astype(np.int32)[:, None, None]).sum(axis=0, dtype=np.int32)
        out[yy] = np.clip(ss >> 22, 0, 255)
    return out


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_tables_reproduce_pillow_resize_bit_for_bit(ci, filt):
    from sfron import resample
    (H, W), (oh, ow) = CASES[ci]
    a = case_image(ci, H, W)
    want = np.asarray(Image.fromarray(a).resize((ow, oh), PIL_FILTER[filt]))
    kx, bx, ksx = resample.resample_tables(W, ow, filt)
    ky, by, ksy = resample.resample_tables(H, oh, filt)
    assert kx.shape == (ow, ksx) and bx.shape == (ow, 2) and ky.shape == (oh, ksy) and by.shape == (oh, 2)
    assert kx.dtype == bx.dtype == np.int32
    got = apply_spec(a, kx, bx, ky, by)
    assert np.array_equal(got, want), int(np.abs(got.astype(int) - want).max())
    if ci % 2:
        assert got.min() == 0 and got.max() == 255
    # a window of the tables is the same window of the image (what the folded crop relies on)
    fy, fx, ny, nx = oh // 3, ow // 4, max(1, oh // 2), max(1, ow // 2)
    tx, ty = resample.resample_tables(W, ow, filt, fx, nx), resample.resample_tables(H, oh, filt, fy, ny)
    assert np.array_equal(apply_spec(a, tx.coeffs, tx.bounds, ty.coeffs, ty.bounds), want[fy:fy + ny, fx:fx + nx])


def test_table_shapes_identity_and_ksize():
    from sfron import resample
    for filt in FILTERS:             # an axis that keeps its size: the tap on the output's own source index is exactly 2^22, every other 0
        k, b, ks = resample.resample_tables(64, 64, filt)
        dense = np.zeros((64, 64 + ks), dtype=np.int64)
        for i in range(64):
            dense[i, b[i, 0]:b[i, 0] + b[i, 1]] = k[i, :b[i, 1]]
        assert np.array_equal(dense[:, :64], np.eye(64, dtype=np.int64) << 22), filt
    k, b, ks = resample.resample_tables(64, 64, "box")
    assert ks == 3 and np.array_equal(b[:, 1], np.ones(64))                          # box: a single tap
    assert resample.resample_tables(2048, 512, "bicubic").ksize == 17                # ceil(2 * 4) * 2 + 1
    assert resample.resample_tables(500, 12, "lanczos").ksize == 251                 # ceil(3 * 500 / 12) * 2 + 1
    assert resample.resample_tables(1120, 64, "bicubic").ksize == 71
    with pytest.raises(ValueError):
        resample.resample_tables(10, 10, "nearest")
    with pytest.raises(ValueError):
        resample.resample_tables(10, 10, "box", 5, 6)


# ------------------------------------------------------------------------------------------------ the transform
def test_size_and_crop_rules_worked_values():
    from sfron import resample
    assert resample.resized_size(640, 480, 512) == (682, 512)          # landscape: int(512 * 640 / 480) = int(682.67)
    assert resample.resized_size(480, 640, 512) == (512, 682)          # portrait
    assert resample.resized_size(500, 375, 512) == (682, 512)
    assert resample.resized_size(2048, 1536, 512) == (682, 512)
    assert resample.resized_size(512, 700, 512) == (512, 700)          # the short side already equals size: unchanged
    assert resample.resized_size(300, 300, 64) == (64, 64)
    assert resample.resized_size(97, 41, 32) == (75, 32)               # int(32 * 97 / 41) = int(75.7)
    assert resample.center_crop_offsets(512, 682, 512) == (0, 85)
    assert resample.center_crop_offsets(683, 512, 512) == (86, 0)      # round(85.5) = 86: python rounds half to even
    assert resample.center_crop_offsets(681, 512, 512) == (84, 0)      # round(84.5) = 84
    assert resample.center_crop_offsets(32, 75, 32) == (0, 22)         # round(21.5) = 22


def _mode_images():
    rng = np.random.default_rng(5)
    rgb = lambda h, w: Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8))
    out = {"rgb_landscape": rgb(41, 97), "rgb_portrait": rgb(90, 37), "rgb_short_side_is_size": rgb(32, 50), "rgb_square_up": rgb(9, 9),
           "L": Image.fromarray(rng.integers(0, 256, size=(45, 70), dtype=np.uint8)),
           "RGBA": Image.fromarray(rng.integers(0, 256, size=(60, 39, 4), dtype=np.uint8)),
           "P": rgb(51, 80).quantize(16)}
    assert out["L"].mode == "L" and out["RGBA"].mode == "RGBA" and out["P"].mode == "P"
    return out


@pytest.mark.parametrize("interp", ("bicubic", "bilinear", "lanczos"))
def test_sd_transform_is_the_pillow_composition(interp):
    from sfron import resample
    S = 32
    for name, img in _mode_images().items():
        w, h = img.size
        nw, nh = resample.resized_size(w, h, S)
        assert min(nw, nh) == S
        ref = img if (nw, nh) == (w, h) else img.resize((nw, nh), PIL_FILTER[interp])        # Resize
        top, left = resample.center_crop_offsets(nh, nw, S)
        ref = np.asarray(ref.crop((left, top, left + S, top + S)).convert("RGB"))             # CenterCrop, then convert("RGB")
        got = resample.sd_transform(img, S, interp)
        assert got.dtype == np.uint8 and got.shape == (S, S, 3)
        assert np.array_equal(got, ref), name
        if img.mode in ("RGB", "L"):          # what the device route computes for these modes: the window of the tables
            a = np.asarray(img.convert("RGB"))
            tx, ty = resample.window_tables(w, h, S, interp)
            assert np.array_equal(apply_spec(a, tx.coeffs, tx.bounds, ty.coeffs, ty.bounds), ref), name


def test_image_resample_wrapper_refuses_bad_tables_before_the_library():
    """The checks that need the tables' contents sit in the wrapper and answer before the library is reached (no GPU here)."""
    from sfron import _lib, resample
    tx, ty = resample.resample_tables(20, 8, "bicubic"), resample.resample_tables(30, 8, "bicubic")
    assert resample.image_resample_u8(None, 29, 20, tx, ty, None, None, tmp_bytes=1 << 20) == _lib.ERR_ARG       # rows reach past Hs = 29
    assert resample.image_resample_u8(None, 30, 19, tx, ty, None, None, tmp_bytes=1 << 20) == _lib.ERR_ARG       # columns reach past Ws = 19
    y0, y1 = ty.rows()
    assert resample.image_resample_u8(None, 30, 20, tx, ty, None, None, tmp_bytes=(y1 - y0) * 8 * 3 - 1) == _lib.ERR_ARG
    bad = resample.Tables(ty.coeffs, ty.bounds[::-1].copy(), ty.ksize)
    assert resample.image_resample_u8(None, 30, 20, tx, bad, None, None, tmp_bytes=1 << 20) == _lib.ERR_ARG      # descending row bounds


# ------------------------------------------------------------------------------------------------ LatentDiffusion
class _Enc:
    def __init__(self):
        self.seen = []

    def moments(self, x):
        self.seen.append(x)
        return torch.zeros(x.shape[0], 8, 2, 2)


class _Cond:
    def encode(self, c):
        return torch.arange(len(c), dtype=torch.float32).view(-1, 1, 1).expand(len(c), 77, 4)


class _Dec:
    def decode(self, z, scale):
        return ("xrec", scale)


def _ld(**kw):
    from sfron import sd

    class LD(sd.LatentDiffusion):
        def get_first_stage_encoding(self, encoder_posterior, eps=None, generator=None):       # (the sample is a device kernel)
            return encoder_posterior.parameters[:, :4] + 1.0

    unet = types.SimpleNamespace(device_=torch.device("cpu"))
    return LD(unet, schedule=types.SimpleNamespace(num_timesteps=1000), **kw)


def test_front_end_raises_without_an_encoder_whatever_it_is_given():
    bare = _ld()
    with_cond = _ld(cond_stage_model=_Cond(), first_stage_decoder=_Dec())
    for ld in (bare, with_cond):
        for f in (ld.get_input, ld.shared_step, ld.encode_first_stage):
            for args, kw in (((), {}), (({}, "jpg"), {}), (({"jpg": None}, "jpg"), {}), ((1, 2, 3, 4), {"generator": None})):
                with pytest.raises(NotImplementedError):
                    f(*args, **kw)


def test_get_input_contract_over_stub_encoders():
    enc = _Enc()
    ld = _ld(first_stage_encoder=enc, cond_stage_model=_Cond(), first_stage_decoder=_Dec())
    nchw = torch.randn(3, 3, 8, 8)
    prompts = ["a", "b", "c"]
    batch = {"jpg": nchw.permute(0, 2, 3, 1), "txt": prompts}
    out = ld.get_input(batch, "jpg")
    assert isinstance(out, list) and len(out) == 2
    z, c = out
    assert tuple(z.shape) == (3, 4, 2, 2) and tuple(c.shape) == (3, 77, 4)
    # the permuted view of NCHW storage reaches the encoder as that storage, not as a copy
    assert enc.seen[-1].data_ptr() == nchw.data_ptr() and tuple(enc.seen[-1].shape) == (3, 3, 8, 8) and enc.seen[-1].is_contiguous()
    # a real NHWC tensor is permuted and made contiguous
    nhwc = nchw.permute(0, 2, 3, 1).contiguous()
    ld.get_input({"jpg": nhwc, "txt": prompts}, "jpg")
    assert enc.seen[-1].data_ptr() != nhwc.data_ptr() and enc.seen[-1].is_contiguous() and torch.equal(enc.seen[-1], nchw)
    # uint8 [B, H, W, 3] goes through as it is
    u8 = torch.randint(0, 256, (3, 8, 8, 3), dtype=torch.uint8)
    ld.get_input({"jpg": u8, "txt": prompts}, "jpg")
    assert enc.seen[-1].dtype == torch.uint8 and enc.seen[-1].data_ptr() == u8.data_ptr()
    # the extras, in the reference's order: z, c, [x, xrec], [x], [xc]
    full = ld.get_input(batch, "jpg", return_first_stage_outputs=True, return_x=True, return_original_cond=True)
    assert len(full) == 6
    assert torch.equal(full[2], nchw) and full[3] == ("xrec", ld.scale_factor) and torch.equal(full[4], nchw) and full[5] is prompts
    z2, c2, x2 = ld.get_input(batch, "jpg", return_x=True)
    assert torch.equal(x2, nchw)
    z3, c3, xc3 = ld.get_input(batch, "jpg", return_original_cond=True)
    assert xc3 is prompts
    zu, cu, xu = ld.get_input({"jpg": u8, "txt": prompts}, "jpg", return_x=True)
    assert torch.equal(xu, (u8.permute(0, 3, 1, 2).float() / 255.0 - 0.5) / 0.5)          # ToTensor + Normalize(0.5, 0.5)
    # bs slices the images before the encoder and the contexts after the cond stage; the prompts come back whole
    zb, cb, xb, xcb = ld.get_input(batch, "jpg", bs=2, return_x=True, return_original_cond=True)
    assert zb.shape[0] == 2 and cb.shape[0] == 2 and torch.equal(cb, c[:2]) and torch.equal(xb, nchw[:2]) and xcb is prompts
    assert enc.seen[-1].shape[0] == 2
    # outside the v1 configuration
    for key in ("class_label", "jpg", "caption"):
        with pytest.raises(NotImplementedError, match=key):
            ld.get_input(dict(batch, caption=prompts, class_label=[0, 1, 2]), "jpg", cond_key=key)
    ld.model.conditioning_key = "concat"
    with pytest.raises(NotImplementedError, match="concat"):
        ld.get_input(batch, "jpg")
    # without a cond stage the prompt half raises as before
    with pytest.raises(NotImplementedError):
        _ld(first_stage_encoder=_Enc()).get_input(batch, "jpg")


def test_encode_first_stage_gives_the_posterior_members():
    from sfron import sd
    ld = _ld(first_stage_encoder=_Enc())
    post = ld.encode_first_stage(torch.zeros(2, 3, 8, 8))
    assert isinstance(post, sd.DiagonalGaussianPosterior)
    post.parameters[:, 4:] = 50.0
    assert tuple(post.mean.shape) == (2, 4, 2, 2) and post.mode() is not None and torch.equal(post.mode(), post.parameters[:, :4])
    assert float(post.logvar.max()) == 20.0                                 # clamped as ldm's DiagonalGaussianDistribution
    assert callable(post.sample)


# ------------------------------------------------------------------------------------------------ loader
def _folder(root, n, seed):
    rng = np.random.default_rng(seed)
    os.makedirs(root / "sub")
    sizes = [(20, 31), (40, 17), (16, 16), (33, 33), (18, 50), (27, 22), (64, 19)]
    names = []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        name = (("sub/" if i % 3 == 2 else "") + f"img_{(7 * i) % 10:02d}.png")
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(root / name)
        names.append(name)
    (root / "notes.txt").write_text("not an image")
    return names


def test_concept_image_loader_order_short_batch_wrap_and_rank_split(tmp_path):
    from sfron import latents, resample, sd
    _folder(tmp_path, 5, 1)
    files = latents.class_files(str(tmp_path))
    assert len(files) == 5
    ld = sd.ConceptImageLoader(str(tmp_path), 2, image_size=16, gpu_resize=False, workers=2, device="cpu")
    assert len(ld) == 3 and ld.files == files
    want = [resample.sd_transform(Image.open(f), 16) for f in files]
    ids = [[0, 1], [2, 3], [4], [0, 1], [2, 3], [4], [0, 1]]                   # the last batch of a pass is short, then the pass starts over
    for i, idx in enumerate(ids):
        assert ld.batch_files(i) == [files[j] for j in idx]
        hb = ld.host_batch(i)
        assert hb.dtype == torch.uint8 and tuple(hb.shape) == (len(idx), 16, 16, 3)
        assert np.array_equal(hb.numpy(), np.stack([want[j] for j in idx])), i
    r0 = sd.ConceptImageLoader(str(tmp_path), 2, image_size=16, gpu_resize=False, workers=2, rank=0, world=2, device="cpu")
    r1 = sd.ConceptImageLoader(str(tmp_path), 2, image_size=16, gpu_resize=False, workers=2, rank=1, world=2, device="cpu")
    for i in range(4):
        whole, a, b = ld.host_batch(i), r0.host_batch(i), r1.host_batch(i)
        assert a.shape[0] + b.shape[0] == whole.shape[0]
        assert torch.equal(whole[0::2], a) and torch.equal(whole[1::2], b)     # the shares interleave to the world = 1 batch
    with pytest.raises(FileNotFoundError):
        sd.ConceptImageLoader(str(tmp_path / "sub" / "nothing"), 2)


# ------------------------------------------------------------------------------------------------ ABI
def test_header_and_bindings_declare_the_resample_entry():
    from sfron import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfron.h")).read(), flags=re.S)
    m = re.search(r"\bint sfron_image_resample_u8\((.*?)\)\s*;", hdr, flags=re.S)
    assert m
    params = [p.strip() for p in m.group(1).split(",")]
    res, args = _lib._PROTOS["sfron_image_resample_u8"]
    assert len(params) == len(args) == 15
    assert "sfron_image_resample_u8" in _lib.declared_symbols()
    assert _lib.ABI_VERSION == 17
    assert _lib.ERR_ARG == 1001
