"""The four driver loops of DDPM/runners/diffusion.py around ``ddpm.DDPMSFRon`` and ``fisher.DDPMFisherAccumulator``, fed by
``ddpm_data.DDPMBatchLoader``:

``train``            :101-177   one stage per iteration on the whole training set (loader flip mode "per_access")
``retrain``          :179-260   the same on the remain split
``sfron_forget``     :1038-1208 the SFR-on iteration, forget stage then remain stage
``generate_fisher``  :1210-1364 the forget loop, then the remain loop -> forget_fisher.pt / remain_fisher.pt

All take the native ``unet.Conditional_Model``, a config namespace and loaders; what the reference reads from ``args`` and from yml
sections ``unet.config_namespace`` does not carry (training, optim, sampling) comes in as keywords, with the config's value as the
default where it has one.  Every ``snapshot_freq`` steps they ``torch.save`` ``DDPMSFRon.checkpoint(step)`` to ``ckpt_dir/ckpt.pth``
and, when ``sample_dir`` is given, draw ``ddpm_sample.sample_visualization`` from the EMA weights through ``load_sampling_model`` -- the
reference samples from ``ema_helper.ema_copy(model)``.  The log lines are the reference's.
"""
import logging
import os
import time

import torch

from . import ddpm, ddpm_data, ddpm_sample, fisher


def _get(config, section, name, default=None):
    return getattr(getattr(config, section, None), name, default)


def _pick(value, config, section, name, default=None):
    return value if value is not None else _get(config, section, name, default)


def betas_of(config, device):
    d = config.diffusion
    return ddpm.get_beta_schedule(getattr(d, "beta_schedule", "linear"), beta_start=getattr(d, "beta_start", 1e-4),
                                  beta_end=getattr(d, "beta_end", 2e-2), num_diffusion_timesteps=d.num_diffusion_timesteps, device=device)


def load_ema(runner, ema_state):
    """EMAHelper.load_state_dict(states[-1]) (:1068): the shadow of a checkpoint into the runner's."""
    views = runner.flat.named_views(runner.shadow)
    for k, v in ema_state.items():
        name = k[len("module."):] if k.startswith("module.") else k
        if name in views:
            views[name].copy_(v)


def snapshot(runner, config, step, ckpt_dir, sample_dir=None, cond_scale=2.0, sampler_kwargs=None, generator=None):
    """The snapshot block the loops share (:159-177): the checkpoint list to ``ckpt_dir/ckpt.pth``; with ``sample_dir`` the sheet
    ``sample-{step}.png`` from the EMA weights (the raw ones when the run keeps no EMA).  Returns the checkpoint's path."""
    states = runner.checkpoint(step)
    os.makedirs(ckpt_dir, exist_ok=True)
    path = os.path.join(ckpt_dir, "ckpt.pth")
    torch.save(states, path)
    if sample_dir is not None:
        dev = runner.flat.p.device
        test_model = ddpm_sample.load_sampling_model(states, config, weights="ema" if runner.shadow is not None else "model", device=dev)
        kw = dict(timesteps=_get(config, "sampling", "timesteps", 1000), skip_type=_get(config, "sampling", "skip_type", "uniform"),
                  eta=_get(config, "sampling", "eta", 0.0))
        kw.update(sampler_kwargs or {})
        os.makedirs(sample_dir, exist_ok=True)
        ddpm_sample.sample_visualization(ddpm.DDPMSampler(test_model, runner.b, generator=generator, **kw), config, step, cond_scale, sample_dir,
                                         device=dev, generator=generator)
        del test_model
    return path


def _runner(model, config, lr, grad_clip, ema_rate, betas, **kw):
    dev = model.device_
    if ema_rate is None and _get(config, "model", "ema", False):
        ema_rate = _get(config, "model", "ema_rate", 0.9999)
    return ddpm.DDPMSFRon(model, betas if betas is not None else betas_of(config, dev), lr=_pick(lr, config, "optim", "lr", 1e-4),
                          grad_clip=_pick(grad_clip, config, "optim", "grad_clip", 1.0), ema_rate=ema_rate,
                          cond_drop_prob=_get(config, "model", "cond_drop_prob", 0.1), n_classes=_get(config, "data", "n_classes", 10), **kw)


def _one_stage(model, config, loader, n_iters, lr, grad_clip, ema_rate, betas, use_graphs, fused_attn, log_freq, snapshot_freq, ckpt_dir,
               sample_dir, cond_scale, sampler_kwargs, log):
    n_iters = _pick(n_iters, config, "training", "n_iters")
    log_freq = _pick(log_freq, config, "training", "log_freq", 100)
    snapshot_freq = _pick(snapshot_freq, config, "training", "snapshot_freq", 0)
    runner = _runner(model, config, lr, grad_clip, ema_rate, betas, n_iters=n_iters, use_graphs=use_graphs, fused_attn=fused_attn)
    it = ddpm_data.cycle(loader)
    start = time.time()
    for step in range(n_iters):
        out = runner.train_step(next(it))
        if log_freq and (step + 1) % log_freq == 0:
            end = time.time()
            log(f"step: {step}, loss: {out['loss'].item()}, time: {end-start}")
            start = time.time()
        if snapshot_freq and (step + 1) % snapshot_freq == 0:
            snapshot(runner, config, step, ckpt_dir, sample_dir, cond_scale, sampler_kwargs)
    return runner


def train(model, config, loader, n_iters=None, lr=None, grad_clip=None, ema_rate=None, betas=None, use_graphs=False, fused_attn=False,
          log_freq=None, snapshot_freq=None, ckpt_dir=None, sample_dir=None, cond_scale=2.0, sampler_kwargs=None, log=logging.info):
    """Diffusion.train (:101-177): loss, clip, Adam, EMA per iteration over ``cycle(loader)``.  ``loader``: a DDPMBatchLoader over the
    whole dataset with flip "per_access" (get_dataset redraws the flip on every access).  Returns the DDPMSFRon that holds the state."""
    return _one_stage(model, config, loader, n_iters, lr, grad_clip, ema_rate, betas, use_graphs, fused_attn, log_freq, snapshot_freq,
                      ckpt_dir, sample_dir, cond_scale, sampler_kwargs, log)


def retrain(model, config, remain_loader, **kw):
    """Diffusion.retrain (:179-260): ``train`` over the remain split of get_forget_dataset (loader flip "frozen").  Keywords: train's."""
    return train(model, config, remain_loader, **kw)


def sfron_forget(model, config, forget_loader, remain_loader, n_iters=None, lr=None, forget_alpha=10.0, remain_alpha=1.0, grad_clip=None,
                 ema_rate=None, ema_state=None, mask=None, mask_path=None, unlearn_loss="adaga", method="ron", lambd=None,
                 decay_forget_alpha=True, label_to_forget=0, betas=None, use_graphs=False, fused_attn=False, log_freq=None,
                 snapshot_freq=None, ckpt_dir=None, sample_dir=None, cond_scale=2.0, sampler_kwargs=None, log=logging.info):
    """Diffusion.sfron_forget (:1038-1208) from its loop on: the model already holds ``states[0]``; ``ema_state`` is ``states[-1]``
    (EMAHelper.load_state_dict).  Every keyword of DDPMSFRon passes through; ``mask_path`` is ``torch.load``-ed as the reference does
    (``mask`` hands the dict over directly).  Per iteration the forget batch is drawn first, then the remain batch, each from its own
    ``cycle(loader)``.  Returns the DDPMSFRon."""
    n_iters = _pick(n_iters, config, "training", "n_iters")
    log_freq = _pick(log_freq, config, "training", "log_freq", 100)
    snapshot_freq = _pick(snapshot_freq, config, "training", "snapshot_freq", 0)
    if mask is None and mask_path:
        mask = torch.load(mask_path)
    runner = _runner(model, config, lr, grad_clip, ema_rate, betas, forget_alpha=forget_alpha, remain_alpha=remain_alpha, mask=mask,
                     unlearn_loss=unlearn_loss, lambd=_pick(lambd, config, "training", "lambd", 0.5), n_iters=n_iters,
                     decay_forget_alpha=decay_forget_alpha, label_to_forget=label_to_forget, use_graphs=use_graphs, method=method,
                     fused_attn=fused_attn)
    if ema_state is not None and runner.shadow is not None:
        load_ema(runner, ema_state)
    forget_it, remain_it = ddpm_data.cycle(forget_loader), ddpm_data.cycle(remain_loader)
    start = time.time()
    for step in range(n_iters):
        forget = next(forget_it)
        remain = next(remain_it)
        out = runner.step(step, forget, remain)
        if log_freq and (step + 1) % log_freq == 0:
            end = time.time()
            log(f"step:{step:04d}, remain L:{out['remain_loss'].item():.4f}, remain a:{remain_alpha}, forget L:{out['forget_loss'].item():.4f}, "
                f"forget a:{out['alpha']:.8f}, time:{end-start:.2f}")
            start = time.time()
        if snapshot_freq and (step + 1) % snapshot_freq == 0:
            snapshot(runner, config, step, ckpt_dir, sample_dir, cond_scale, sampler_kwargs)
    return runner


def generate_fisher(model, config, forget_loader, remain_loader, ckpt_folder, label_to_forget=0, cond_scale=2.0, grad_clip=None, betas=None,
                    log_freq=None, log=logging.info):
    """Diffusion.generate_fisher (:1210-1364): one pass over the forget loader, then one over the remain loader, each into a
    DDPMFisherAccumulator with n_batches = len(loader); ``ckpt_folder/mask_{label}/forget_fisher.pt`` and ``remain_fisher.pt`` hold the
    ``module.`` names, ready for ``fisher.masks_from_fisher``.  Returns the two paths."""
    log("Generating fisher of diffusion to achieve gradient sparsity.")
    mask_path = os.path.join(ckpt_folder, f"mask_{label_to_forget}")
    os.makedirs(mask_path, exist_ok=True)
    log_freq = _pick(log_freq, config, "training", "log_freq", 100)
    b = betas if betas is not None else betas_of(config, model.device_)
    paths = []
    for kind, loader in (("Forget", forget_loader), ("Remain", remain_loader)):
        acc = fisher.DDPMFisherAccumulator(model, b, n_batches=len(loader), cond_scale=cond_scale,
                                           grad_clip=_pick(grad_clip, config, "optim", "grad_clip", 1.0))
        start_time, running, train_steps, log_steps = time.time(), 0.0, 0, 0
        for batch in loader:
            running = running + acc.accumulate(batch)
            log_steps += 1
            train_steps += 1
            if log_freq and train_steps % log_freq == 0:
                end_time = time.time()
                log(f"{kind} (step={train_steps:07d}) Loss: {float(running) / log_steps:.4f} Train Steps/Sec: {log_steps / (end_time - start_time):.2f}")
                running, log_steps, start_time = 0.0, 0, time.time()
        paths.append(os.path.join(mask_path, f"{kind.lower()}_fisher.pt"))
        torch.save(acc.state_dict(), paths[-1])
    return tuple(paths)
