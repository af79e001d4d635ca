"""GPU: the drivers of sfron.ddpm_train fed by ddpm_data.DDPMBatchLoader against the same classes fed by hand.

A tiny net (ch_mult [1, 2], one res block, attention at 8, 16 px), 23 images, batch 5: the forget split (8 images) gives batches of
5, 3 and -- a new epoch, a new permutation -- 5 in three iterations.  The hand-made batches are torch ops in the documented order of
draws from a generator seeded like the loader's, with the image arithmetic done on the CPU (where the reference runs ToTensor); the model
is built twice from one torch seed, so its own draws (initialisation, dropout, classifier-free keep masks) are the same in both runs.
Parameters, Adam moments and the EMA shadow must then be bit-equal."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 1000
N, BS, DROP = 23, 5, 1


def make_config():
    from sfron import ddpm_data, unet
    cfg = unet.config_namespace(ch_mult=[1, 2], num_res_blocks=1, attn_resolutions=[8], image_size=16)
    return ddpm_data.config_with_data(cfg, channels=3, random_flip=True, uniform_dequantization=True, gaussian_dequantization=False,
                                      rescaled=True, logit_transform=False)


@pytest.fixture(scope="module")
def world():
    from sfron import ddpm, ddpm_data
    g = torch.Generator().manual_seed(17)
    img = torch.randint(0, 256, (N, 3, 16, 16), generator=g, dtype=torch.uint8)
    labels = torch.arange(N) % 3
    ds = ddpm_data.ResidentDataset(img, labels, device=DEV)
    remain, forget = ddpm_data.split_forget(labels, DROP)
    assert len(forget) == 8 and len(remain) == 15
    return dict(cfg=make_config(), ds=ds, img=img, labels=labels, remain=remain, forget=forget, betas=ddpm.get_beta_schedule(device=DEV))


def loader(w, indices, seed, flip="frozen"):
    from sfron import ddpm_data
    return ddpm_data.DDPMBatchLoader(w["ds"], indices, BS, w["cfg"], T, torch.Generator(device=DEV).manual_seed(seed), flip=flip)


def by_hand(w, indices, seed, flip="frozen"):
    """the loader's batches without the loader and without the kernel, epochs without end"""
    from sfron import ddpm_data
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = len(indices)
    frozen = (torch.rand(n, generator=g, device=DEV) < 0.5) if flip == "frozen" else None
    while True:
        perm = torch.randperm(n, generator=g, device=DEV)
        for i in range((n + BS - 1) // BS):
            pos = perm[BS * i:BS * i + BS].cpu()
            B = pos.shape[0]
            if flip == "frozen":
                fl = frozen.cpu()[pos]
            elif flip == "per_access":
                fl = (torch.rand(B, generator=g, device=DEV) < 0.5).cpu()
            u = torch.rand(B, 3, 16, 16, generator=g, device=DEV)
            e = torch.randn(B, 3, 16, 16, generator=g, device=DEV)
            t_half = torch.randint(0, T, (B // 2 + 1,), generator=g, device=DEV)
            idx = indices[pos]
            x = w["img"][idx]
            x = torch.where(fl[:, None, None, None], x.flip(3), x).float() / 255
            x0 = ddpm_data.data_transform(w["cfg"], x, u=u.cpu())
            yield {"x0": x0.to(DEV), "c": w["labels"][idx].to(DEV), "t": torch.cat([t_half, T - t_half - 1], dim=0)[:B], "e": e}


def build_model(w, seed=50):
    from sfron import unet
    torch.manual_seed(seed)
    return unet.Conditional_Model(w["cfg"], device=DEV)


def state(run):
    torch.cuda.synchronize()
    return {"p": run.flat.p.clone(), "m": run.opt.m.clone(), "v": run.opt.v.clone(), "ema": run.shadow.clone()}


def assert_same(a, b):
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def random_mask(model, seed=3):
    g = torch.Generator().manual_seed(seed)
    return {"module." + n: (torch.rand(p.shape, generator=g) < 0.5) for n, p in model.named_parameters()}


@pytest.mark.parametrize("method,loss", [("ron", "adaga"), ("joint", "ga")])
def test_sfron_forget_equals_the_hand_fed_step(world, method, loss, tmp_path):
    from sfron import ddpm, ddpm_train
    w, n_it = world, 3
    kw = dict(lr=1e-3, forget_alpha=10.0, remain_alpha=0.5, grad_clip=1.0, ema_rate=0.5, unlearn_loss=loss, method=method, lambd=0.5,
              decay_forget_alpha=True)
    model = build_model(w)
    mask = random_mask(model)
    mask_path = str(tmp_path / "mask.pt")
    torch.save(mask, mask_path)
    lines = []
    run = ddpm_train.sfron_forget(model, w["cfg"], loader(w, w["forget"], 1), loader(w, w["remain"], 2), n_iters=n_it, mask_path=mask_path,
                                  betas=w["betas"], log_freq=1, log=lines.append, **kw)
    got = state(run)
    assert len(lines) == n_it and lines[0].startswith("step:0000, remain L:") and "forget a:10.00000000" in lines[0]
    model2 = build_model(w)
    run2 = ddpm.DDPMSFRon(model2, w["betas"], mask=mask, n_iters=n_it, **kw)
    hf, hr = by_hand(w, w["forget"], 1), by_hand(w, w["remain"], 2)
    sizes = []
    for step in range(n_it):
        f, r = next(hf), next(hr)
        sizes.append(f["x0"].shape[0])
        run2.step(step, f, r)
    assert sizes == [5, 3, 5]                                # a short batch, then a new epoch
    want = state(run2)
    assert not torch.equal(want["p"], want["ema"]) and bool(torch.isfinite(want["p"]).all())
    assert_same(got, want)


def test_train_equals_the_hand_fed_one_stage_update(world):
    from sfron import ddpm, ddpm_train
    w = world
    everything = torch.arange(N)
    lines = []
    run = ddpm_train.train(build_model(w), w["cfg"], loader(w, everything, 4, flip="per_access"), n_iters=2, lr=1e-3, ema_rate=0.5,
                           betas=w["betas"], log_freq=1, log=lines.append)
    got = state(run)
    assert len(lines) == 2 and lines[1].startswith("step: 1, loss: ")
    run2 = ddpm.DDPMSFRon(build_model(w), w["betas"], lr=1e-3, ema_rate=0.5, n_iters=2)
    hand = by_hand(w, everything, 4, flip="per_access")
    for _ in range(2):                                       # loss -> backward -> clip -> Adam -> EMA, from the pieces of step()
        batch = next(hand)
        run2.model.train()
        run2._remain_pass(**{k: batch.get(k) for k in ("x0", "c", "t", "e", "keep_mask")})
        run2.opt.step(max_norm=run2.grad_clip, use_mask=False, ema=run2.shadow, ema_decay=run2.mu, ema_mode=2)
        run2._weights_updated()
    want = state(run2)
    assert not torch.equal(want["p"], want["ema"])
    assert_same(got, want)
    # retrain is the same loop over the remain split
    a = state(ddpm_train.retrain(build_model(w), w["cfg"], loader(w, w["remain"], 2), n_iters=1, lr=1e-3, ema_rate=0.5, betas=w["betas"]))
    run3 = ddpm.DDPMSFRon(build_model(w), w["betas"], lr=1e-3, ema_rate=0.5, n_iters=1)
    run3.train_step(next(by_hand(w, w["remain"], 2)))
    assert_same(a, state(run3))


def test_generate_fisher_equals_the_hand_fed_accumulator(world, tmp_path):
    from sfron import ddpm_train, fisher
    w = world
    model = build_model(w)
    fl, rl = loader(w, w["forget"], 1), loader(w, w["remain"], 2)
    paths = ddpm_train.generate_fisher(model, w["cfg"], fl, rl, str(tmp_path), label_to_forget=DROP, cond_scale=2.0, betas=w["betas"],
                                       log=lambda s: None)
    assert paths == (os.path.join(str(tmp_path), f"mask_{DROP}", "forget_fisher.pt"), os.path.join(str(tmp_path), f"mask_{DROP}", "remain_fisher.pt"))
    model2 = build_model(w)
    for path, indices, seed, n_batches in ((paths[0], w["forget"], 1, 2), (paths[1], w["remain"], 2, 3)):
        acc = fisher.DDPMFisherAccumulator(model2, w["betas"], n_batches=n_batches, cond_scale=2.0, grad_clip=1.0)
        hand = by_hand(w, indices, seed)
        for _ in range(n_batches):
            acc.accumulate(next(hand))
        want, got = acc.state_dict(), torch.load(path)
        assert list(got) == list(want) and all(k.startswith("module.") for k in got)
        assert any(float(v.abs().max()) > 0 for v in want.values())
        for k in want:
            assert torch.equal(got[k], want[k]), k
    masks = fisher.masks_from_fisher(torch.load(paths[0]), torch.load(paths[1]), 0.5, device=DEV)      # ready for the mask generation
    assert set(masks) == set(want)


def test_snapshot_writes_a_checkpoint_the_sampler_loads(world, tmp_path):
    from types import SimpleNamespace as NS

    from sfron import ddpm_sample, ddpm_train
    w = world
    cfg = NS(**vars(w["cfg"]))
    cfg.training, cfg.sampling = NS(visualization_samples=10), NS(batch_size=5)
    ckpt_dir, sample_dir = str(tmp_path / "ckpts"), str(tmp_path / "samples")
    run = ddpm_train.sfron_forget(build_model(w), cfg, loader(w, w["forget"], 1), loader(w, w["remain"], 2), n_iters=2, lr=1e-3, ema_rate=0.5,
                                  unlearn_loss="ga", betas=w["betas"], log_freq=0, snapshot_freq=2, ckpt_dir=ckpt_dir, sample_dir=sample_dir,
                                  sampler_kwargs=dict(timesteps=2))
    states = torch.load(os.path.join(ckpt_dir, "ckpt.pth"), map_location=DEV)
    assert len(states) == 4 and states[2] == 1
    assert os.path.getsize(os.path.join(sample_dir, "sample-1.png")) > 0
    ema = ddpm_sample.load_sampling_model(states, cfg, weights="ema", device=DEV)
    raw = ddpm_sample.load_sampling_model(states, cfg, weights="model", device=DEV)
    shadow, live = run.ema_state_dict(), run.flat.named_views(run.flat.p)
    for n, p in ema.named_parameters():
        assert torch.equal(p, shadow[n]), n
    for n, p in raw.named_parameters():
        assert torch.equal(p, live[n]), n
