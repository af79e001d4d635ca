"""Host side of the DDPM (CIFAR-10) epsilon loss (csrc/loss.hip, "DDPM" section).

API mirror of /root/reference/DDPM/functions/losses.py:
  ``noise_estimation_loss_conditional(model, x0, t, c, e, b, cond_drop_prob=0.1, keepdim=False)`` (:22-38),
  ``loss_registry_conditional["simple"]`` (:45-47), ``adaptive_loss(loss_fn, model, x0, t, c, e, b, lambd)`` (:49-69),
  ``cosine_lr_scheduler(alpha, step, n_steps)`` (:71-72), and of ``get_beta_schedule`` for the schedule cifar10_sfron.yml
  uses (DDPM/runners/diffusion.py:36-66: fp64 linspace -> fp32 tensor).
The denoiser is any ``model(x_t, t.float(), c, mode="train", cond_drop_prob=...)`` callable whose output takes part in
autograd; everything around it (alphas_cumprod, q-sample, per-sample sums, adaptive weights, the gradient handed to the
denoiser's backward) runs in the HIP library.  With ``dp_group`` the adaptive weights are normalised over the GLOBAL
batch (one all-reduce of a scalar).
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr


def get_beta_schedule(beta_schedule="linear", *, beta_start=1e-4, beta_end=2e-2, num_diffusion_timesteps=1000, device="cuda"):
    if beta_schedule != "linear":
        raise NotImplementedError("cifar10_sfron.yml uses the linear schedule")
    return torch.from_numpy(np.linspace(beta_start, beta_end, num_diffusion_timesteps, dtype=np.float64)).float().to(device)


def alphas_cumprod(b):
    """(1 - b).cumprod(0) in fp32 (functions/losses.py:25, recomputed there on every call).  A schedule that a runner has pinned with
    ``pin_alphas_cumprod`` answers from that copy while the tensor is unchanged: the one-workgroup sequential product costs 70 us per call,
    twice per SFR-on step."""
    memo = getattr(b, "_sfron_abar", None)
    if memo is not None and memo[0] == b._version:
        return memo[1]
    out = torch.empty_like(b)
    check(_lib.lib().sfron_ddpm_alphas_cumprod(ptr(b), b.numel(), ptr(out), stream_ptr()), "ddpm_alphas_cumprod")
    return out


def pin_alphas_cumprod(b):
    """Compute alphas_cumprod(b) once, eagerly (outside any stage graph: the copy must outlive every capture), and attach it to ``b``."""
    b._sfron_abar = None
    b._sfron_abar = (b._version, alphas_cumprod(b))
    return b


def q_sample(x0, e, t, abar):
    x0, e = x0.contiguous(), e.contiguous()
    xt = torch.empty_like(x0)
    check(_lib.lib().sfron_ddpm_q_sample(ptr(x0), ptr(e), ptr(t), ptr(abar), x0.shape[0], x0[0].numel(), ptr(xt), stream_ptr()),
          "ddpm_q_sample")
    return xt


class _SampleLoss(torch.autograd.Function):
    """per_sample[i] = sum_chw (e - out)^2 ; backward: d out_i = g_i * 2 (out_i - e_i) through sfron_ddpm_loss_bwd."""

    @staticmethod
    def forward(ctx, out, e):
        out, e = out.contiguous(), e.contiguous()
        n, chw = out.shape[0], out[0].numel()
        per = torch.empty(n, dtype=torch.float32, device=out.device)
        check(_lib.lib().sfron_ddpm_sample_loss(ptr(e), ptr(out), n, chw, ptr(per), stream_ptr()), "ddpm_sample_loss")
        ctx.save_for_backward(out, e)
        return per

    @staticmethod
    def backward(ctx, g):
        out, e = ctx.saved_tensors
        coef = (2.0 * g).contiguous().float()
        d = torch.empty_like(out)
        check(_lib.lib().sfron_ddpm_loss_bwd(ptr(e), ptr(out), ptr(coef), out.shape[0], out[0].numel(), ptr(d), stream_ptr()),
              "ddpm_loss_bwd")
        return d, None


class _Reduce(torch.autograd.Function):
    """loss = mean(per) ("simple") or sum(w*per)/sum(w) with detached adaptive weights ("adaga"); the backward hands
    per-sample coefficients to _SampleLoss (coef_i / 2 = d loss / d per_i)."""

    @staticmethod
    def forward(ctx, per, mode, lambd, dp_group):
        n = per.shape[0]
        world = torch.distributed.get_world_size(dp_group) if dp_group is not None else 1
        coef = torch.empty_like(per)
        loss = torch.empty((), dtype=torch.float32, device=per.device)
        wsum = torch.zeros((), dtype=torch.float32, device=per.device)
        L = _lib.lib()
        check(L.sfron_ddpm_loss_coef(ptr(per), n, mode, float(lambd), 1.0, n * world, ptr(wsum), 0, ptr(coef), ptr(loss),
                                     stream_ptr()), "ddpm_loss_coef")
        if mode == 1 and dp_group is not None:
            torch.distributed.all_reduce(wsum, group=dp_group)
            check(L.sfron_ddpm_loss_coef(ptr(per), n, mode, float(lambd), 1.0, n * world, ptr(wsum), 1, ptr(coef), ptr(loss),
                                         stream_ptr()), "ddpm_loss_coef")
        ctx.save_for_backward(coef)
        return loss

    @staticmethod
    def backward(ctx, g):
        (coef,) = ctx.saved_tensors
        return coef * (0.5 * g), None, None, None


def noise_estimation_loss_conditional(model, x0, t, c, e, b, cond_drop_prob=0.1, keepdim=False, dp_group=None):
    abar = alphas_cumprod(b)
    x = q_sample(x0, e, t, abar)
    output = model(x, t.float(), c, cond_drop_prob=cond_drop_prob, mode="train")
    per = _SampleLoss.apply(output, e)
    if keepdim:
        return per
    return _Reduce.apply(per, 0, 0.0, dp_group)


loss_registry_conditional = {"simple": noise_estimation_loss_conditional}


def adaptive_loss(loss_fn, model, x0, t, c, e, b, lambd=0.5, dp_group=None):
    per = loss_fn(model, x0, t, c, e, b, keepdim=True)
    return _Reduce.apply(per, 1, lambd, dp_group)


def cosine_lr_scheduler(alpha, step, n_steps):
    return alpha * (1 + math.cos(math.pi * step / n_steps)) / 2


def compute_alpha(beta, t):
    """DDPM/functions/denoising.py:4-7 (host-side, tiny): alpha_bar of timestep t with alpha_bar(-1) = 1."""
    beta = torch.cat([torch.zeros(1, device=beta.device), beta], dim=0)
    return alphas_cumprod(beta).index_select(0, t + 1)


def generalized_row(abar, i, j, eta):
    """(s1, s2, s3, c1, c2) of one generalized step from timestep i to j (j = -1: the last step) in the meaning of sfron_ddim_step:
    DDPM/functions/denoising.py:85-92 in torch's fp32 0-dim tensor math.  ``abar``: CPU fp32 [T + 1], alpha_bar of timestep t at index
    t + 1 and alpha_bar(-1) = 1 at index 0.  A step whose s2 = sqrt(alpha_bar_i) is 0 would divide by zero on the device: refused here."""
    at, at_next = abar[i + 1], abar[j + 1]                                                 # fp32 0-dim tensors: torch's scalar math
    c1 = eta * ((1 - at / at_next) * (1 - at_next) / (1 - at)).sqrt()
    c2 = ((1 - at_next) - c1 ** 2).sqrt()
    row = (float((1 - at).sqrt()), float(at.sqrt()), float(at_next.sqrt()), float(c1), float(c2))
    if row[1] == 0.0:
        raise _lib.SfronError(f"generalized step {i} -> {j}: sqrt(alpha_bar) is 0, the update would divide by it")
    return row


def generalized_coefficients(abar, seq, eta=0.0):
    """The coefficient table of a whole sampling run, in execution order (``seq`` reversed): a list of (s1, s2, s3, c1, c2) rows and the
    list of timesteps the model sees.  The ONE host helper behind generalized_steps_conditional and DDPMSampler."""
    seq = [int(s) for s in seq]
    seq_next = [-1] + seq[:-1]
    eta = float(eta)
    steps = list(zip(reversed(seq), reversed(seq_next)))
    return [generalized_row(abar, i, j, eta) for i, j in steps], [i for i, _ in steps]


def _abar_host(b):
    return torch.cat([torch.ones(1, device=b.device), alphas_cumprod(b)]).cpu()           # index t+1; alpha_bar(-1) = 1


def generalized_steps_conditional(x, c, seq, model, b, cond_scale=3.0, step_noise=None, **kwargs):
    """DDPM/functions/denoising.py:72-95: the classifier-free-guided generalized (DDIM, ``eta``) sampler the runner's snapshot
    path uses.  Returns (xs, x0_preds) like the reference (tensors stay on the device).  The denoiser is the caller's
    ``model(x, t, c, cond_scale=..., mode="test")``; the update runs in sfron_ddim_step.  ``step_noise[k]`` optionally fixes
    the k-th ``randn_like`` draw.  The coefficients of all steps are formed before the first one (generalized_coefficients: the same fp32
    values as step by step); one difference from the earlier form: a step whose sqrt(alpha_bar) is 0 -- no schedule of the reference
    has one -- now raises SfronError before anything runs instead of being refused by sfron_ddim_step when the loop reaches it."""
    eta = float(kwargs.get("eta", 0))
    rows, ts = generalized_coefficients(_abar_host(b), seq, eta)
    with torch.no_grad():
        n = x.size(0)
        xs, x0_preds = [x], []
        for k, (i, (s1, s2, s3, c1, c2)) in enumerate(zip(ts, rows)):
            t = (torch.ones(n) * i).to(x.device)
            et = model(xs[-1], t, c, cond_scale=cond_scale, mode="test").contiguous().float()
            noise = None
            if eta != 0.0:
                noise = (torch.randn_like(x) if step_noise is None else step_noise[k]).contiguous()
            xt = xs[-1].contiguous().float()
            x_next, x0 = torch.empty_like(xt), torch.empty_like(xt)
            check(_lib.lib().sfron_ddim_step(ptr(xt), ptr(et), ptr(noise), xt.numel(), s1, s2, s3, c1, c2, ptr(x_next), ptr(x0), stream_ptr()),
                  "ddim_step")
            x0_preds.append(x0)
            xs.append(x_next)
    return xs, x0_preds


def sampling_sequence(skip_type="uniform", num_timesteps=1000, timesteps=1000):
    """The timestep sequence of Diffusion.sample_image (DDPM/runners/diffusion.py:831-842), ascending.  "uniform":
    range(0, T, T // timesteps) -- MORE than ``timesteps`` entries where T % timesteps != 0, as the reference has it; "quad":
    int(linspace(0, sqrt(0.8 T), timesteps)[k] ** 2)."""
    if skip_type == "uniform":
        return list(range(0, num_timesteps, num_timesteps // timesteps))
    if skip_type == "quad":
        return [int(s) for s in list(np.linspace(0, np.sqrt(num_timesteps * 0.8), timesteps) ** 2)]
    raise NotImplementedError(f"skip_type {skip_type!r} (DDPM/runners/diffusion.py:831-844 defines 'uniform' and 'quad')")


class DDPMSampler:
    """Diffusion.sample_image (DDPM/runners/diffusion.py:825-872) for sample_type "generalized": classifier-free-guided DDIM-style
    sampling whose step is ONE guided forward pass and ONE fused update launch (sfron_ddpm_guided_step), with the step's coefficients
    and timestep read on the device through a step index that sfron_ddpm_sampler_advance moves -- so one captured step replays for the
    whole run (``graph=True``).

    model: ``sfron.unet.Conditional_Model`` (anything with ``forward_pair``) takes the batch-2B route -- both guidance branches in one
    pass, dropout off whatever the model's mode; ``cond_scale == 0`` runs the conditional branch alone at batch B.  Any other callable is
    called as ``model(x, t, c, cond_scale=..., mode="test")`` and its combined epsilon goes through the same kernel.  Negative scales are
    legal (sample.py itself uses -1).
    eta != 0: each step's noise is drawn from ``generator`` (on its device; None: the default generator of the images' device) into one
    static buffer, in step order.
    graph: capture one step (pair forward, guided step, advance) after an eager first step and replay it; at most ONE graph per sampler,
    for the first (batch shape, cond_scale) it sees -- any other batch (the short last round) runs eagerly.  ``last=False`` runs eagerly
    too (it keeps every step's tensors).  Default False.
    sample_type "ddpm_noisy" is not available: the reference imports a name that does not exist there."""

    def __init__(self, model, betas, sample_type="generalized", skip_type="uniform", timesteps=1000, eta=0.0, graph=False, generator=None):
        if sample_type == "ddpm_noisy":
            raise NotImplementedError("sample_type 'ddpm_noisy': DDPM/runners/diffusion.py:865 imports ddpm_steps_conditional, which "
                                      "functions/denoising.py does not define (SURVEY.md section 9 Q16)")
        if sample_type != "generalized":
            raise NotImplementedError(f"sample_type {sample_type!r}")
        self.model, self.eta, self.graph, self.generator = model, float(eta), bool(graph), generator
        self.seq = sampling_sequence(skip_type, int(betas.numel()), int(timesteps))
        rows, ts = generalized_coefficients(_abar_host(betas), self.seq, self.eta)
        dev = betas.device
        self.steps = len(rows)
        self.coef = torch.tensor(rows, dtype=torch.float32, device=dev).contiguous()            # [steps][5]
        self.tseq = torch.tensor(ts, dtype=torch.float32, device=dev)
        self.step_idx = torch.zeros(1, dtype=torch.int32, device=dev)
        self._pair = hasattr(model, "forward_pair")
        self._g = None                    # the one captured step: dict(key, graph, x, t, c, noise)

    # one step on the buffers it is given: model pass, guided update, advance.  Stream-ordered device work only.
    def _step(self, x, t, c, noise, cond_scale, x_next, x0_pred):
        L = _lib.lib()
        if self._pair:
            ec, en = self.model.forward_pair(x, t, c, with_null=cond_scale != 0)
        else:
            ec, en = self.model(x, t, c, cond_scale=cond_scale, mode="test").contiguous().float(), None
        check(L.sfron_ddpm_guided_step(ptr(x), ptr(ec), ptr(en), ptr(noise), float(cond_scale), ptr(self.coef), self.steps, ptr(self.step_idx),
                                       x.numel(), ptr(x_next), ptr(x0_pred), stream_ptr()), "ddpm_guided_step")
        check(L.sfron_ddpm_sampler_advance(ptr(self.tseq), self.steps, ptr(self.step_idx), ptr(t), t.numel(), stream_ptr()), "ddpm_sampler_advance")

    def _draw(self, noise):
        g = self.generator
        if g is not None and g.device != noise.device:
            noise.copy_(torch.randn(noise.shape, generator=g, device=g.device))
        else:
            noise.normal_(generator=g)

    def _capture(self, st, cond_scale):
        import gc
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        # graphs.StageGraph's capture discipline: no cyclic collection while the stream captures, a private memory pool
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(graph, pool=torch.cuda.graph_pool_handle()):
                self._step(st["x"], st["t"], st["c"], st["noise"], cond_scale, st["x"], None)
        finally:
            if gc_was_on:
                gc.enable()
        st["graph"] = graph

    @torch.no_grad()
    def sample_image(self, x, c, cond_scale, last=True):
        """x: the starting noise [B, C, H, W]; c: int64 labels [B].  last=True: the final image batch; last=False: (xs, x0_preds), the lists
        generalized_steps_conditional returns (xs[0] is ``x``)."""
        cond_scale = float(cond_scale)
        x = x.float().contiguous()
        c = c.contiguous()
        B = x.shape[0]
        m = self.model
        prep = hasattr(m, "_prep_conv_weights")
        if prep:
            # the weights do not change while a run samples: re-lay the convolution operands once (if the model asks for it) instead of
            # in every pass, and hand the model back as it was -- its "operands are stale" flag included: a training loop that captures
            # its next stage into a graph decides by that flag whether the graph re-lays them
            was_auto, was_dirty = m.auto_prep, getattr(m, "_conv_dirty", True)
            m._prep_conv_weights()
            m.auto_prep = False
        try:
            key = (tuple(x.shape), c.dtype, cond_scale)
            use_graph = self.graph and last and (self._g is None or self._g["key"] == key)
            self.step_idx.zero_()
            if use_graph and self._g is not None:
                st = self._g
                st["x"].copy_(x)
                st["c"].copy_(c)
                st["t"].fill_(float(self.seq[-1]))
            else:
                st = dict(key=key, graph=None, x=x.clone(), c=c.clone(), t=torch.full((B,), float(self.seq[-1]), dtype=torch.float32, device=x.device),
                          noise=torch.empty_like(x) if self.eta != 0.0 else None)
            if not last:
                xs, x0s = [x], []
                for _ in range(self.steps):
                    if st["noise"] is not None:
                        self._draw(st["noise"])
                    x_next, x0 = torch.empty_like(x), torch.empty_like(x)
                    self._step(xs[-1], st["t"], st["c"], st["noise"], cond_scale, x_next, x0)
                    xs.append(x_next)
                    x0s.append(x0)
                return xs, x0s
            for k in range(self.steps):
                if st["noise"] is not None:
                    self._draw(st["noise"])
                if use_graph and st["graph"] is not None:
                    st["graph"].replay()
                    continue
                self._step(st["x"], st["t"], st["c"], st["noise"], cond_scale, st["x"], None)
                if use_graph and k == 0 and self.steps > 1:          # the eager first step was the warm-up
                    self._capture(st, cond_scale)
                    self._g = st
            return st["x"].clone() if st is self._g else st["x"]
        finally:
            if prep:
                m.auto_prep, m._conv_dirty = was_auto, was_dirty


# ----------------------------------------------------------------------------------------------------------------------
class FlatParams:
    """Re-homes the trainable parameters of ANY autograd module in one flat fp32 arena (parameters and their .grad
    become views), so that the mask -> clip -> Adam -> EMA sweep of csrc/sweep.hip runs over it in two launches per
    stage instead of the reference's per-tensor loops (DDPM/runners/diffusion.py:1126-1138,1169-1180)."""

    def __init__(self, model):
        self.names, self.params = [], []
        for n, p in model.named_parameters():
            if p.requires_grad:
                self.names.append(n)
                self.params.append(p)
        self.w_bf16 = None
        if hasattr(model, "flat_arena"):
            # sfron.unet.Conditional_Model: the parameters already live in one arena (with a gradient arena and a bf16 weight
            # shadow at the same offsets) -- adopt it
            self.p, self.g, self.w_bf16, index = model.flat_arena()
            self.offsets = [index[n][0] for n in self.names]
            self.n = self.p.numel()
            return
        dev = self.params[0].device
        self.offsets, off = [], 0
        for p in self.params:
            self.offsets.append(off)
            off += (p.numel() + 7) // 8 * 8                       # 16-byte aligned tensors
        self.n = off
        self.p = torch.zeros(off, dtype=torch.float32, device=dev)
        self.g = torch.zeros(off, dtype=torch.float32, device=dev)
        for p, o in zip(self.params, self.offsets):
            k = p.numel()
            self.p[o:o + k].copy_(p.data.reshape(-1))
            p.data = self.p[o:o + k].view(p.shape)
            p.grad = self.g[o:o + k].view(p.shape)                # autograd accumulates in place into the arena

    def mask_arena(self, mask):
        """name -> bool tensor / python int (DDPM/generate_fisher_mask.py:39-46; keys with or without 'module.')."""
        arena = torch.zeros(self.n, dtype=torch.uint8, device=self.p.device)     # arena padding stays masked out
        for n, p, o in zip(self.names, self.params, self.offsets):
            m = mask.get(n, mask.get("module." + n))
            if m is None:
                raise KeyError(f"saliency mask has no entry for {n}")
            if isinstance(m, int):
                arena[o:o + p.numel()] = 1 if m else 0
            else:
                arena[o:o + p.numel()] = m.reshape(-1).to(device=self.p.device, dtype=torch.uint8)
        return arena

    def named_views(self, flat):
        return {n: flat[o:o + p.numel()].view(p.shape) for n, p, o in zip(self.names, self.params, self.offsets)}


class DDPMSFRon:
    """The SFR-on iteration of DDPM/runners/diffusion.py:1075-1180 (method "ron"): cosine-decayed alpha, forget loss
    "ga" / "adaga" -> mask -> clip -> Adam, remain loss -> clip -> Adam, EMAHelper update.  The denoiser is the caller's
    autograd module (``model(x, t_float, c, mode="train", cond_drop_prob=...)``); loss, gradient hand-off and the whole
    parameter sweep run in the HIP library.  ``step(forget, remain)`` takes dicts with x0 (already data_transform-ed),
    c, t, e."""

    def __init__(self, model, betas=None, lr=1e-4, forget_alpha=10.0, remain_alpha=1.0, grad_clip=1.0, ema_rate=None, mask=None,
                 unlearn_loss="adaga", lambd=0.5, n_iters=50, decay_forget_alpha=True, cond_drop_prob=0.1, process_group=None,
                 label_to_forget=0, n_classes=10, use_graphs=False, method="ron", fused_attn=False):
        """fused_attn: run the denoiser's AttnBlocks on the fused self-attention kernels of csrc/wattn.hip
        (Conditional_Model.fused_attention); opt-in, the default launches are unchanged."""
        from . import dp, sweep
        self.use_graphs, self._graphs, self._pool = bool(use_graphs), {}, None
        # method "joint" (runners/diffusion.py:1160-1167): ONE clipped Adam step per iteration on remain_alpha * remain_loss +
        # alpha * forget_loss, both back-propagated from the same weights; the reference's mask loop there runs on the stale gradients
        # of the previous step, just before zero_grad(), so the mask does not touch the update
        if method not in ("ron", "joint"):
            raise ValueError(f"unsupported method {method!r} (DDPM/runners/diffusion.py:1121,1154-1167 defines 'ron' and 'joint')")
        self.method, self._g_forget = method, None
        if unlearn_loss not in ("ga", "adaga", "rl"):
            raise ValueError(f"unsupported unlearn_loss {unlearn_loss!r} (DDPM/runners/diffusion.py:1095-1120 defines ga, rl, adaga)")
        self.label_to_forget, self.n_classes = label_to_forget, n_classes
        self.model, self.flat = model, FlatParams(model)
        if fused_attn:
            if not hasattr(model, "fused_attention"):
                raise ValueError("fused_attn needs the native Conditional_Model (it has no effect on another denoiser)")
            model.fused_attention = True
        dev = self.flat.p.device
        self.b = pin_alphas_cumprod(betas if betas is not None else get_beta_schedule(device=dev))
        self.forget_alpha, self.remain_alpha, self.grad_clip = forget_alpha, remain_alpha, grad_clip
        self.unlearn_loss, self.lambd, self.n_iters, self.decay = unlearn_loss, lambd, n_iters, decay_forget_alpha
        self.cond_drop_prob, self.pg, self._dp = cond_drop_prob, process_group, dp
        self.world = dp.world_size(process_group)
        marena = self.flat.mask_arena(mask) if mask is not None else None
        # DDPM/functions/__init__.py:9-18 with cifar10_sfron.yml:48-56: Adam, wd 0, betas (0.9, 0.999), eps 1e-8
        self.opt = sweep.FlatAdam(self.flat.p, self.flat.g, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, adamw=True, mask=marena,
                                  w_bf16=self.flat.w_bf16)
        self.mu = ema_rate
        self.shadow = self.flat.p.clone() if ema_rate is not None else None       # EMAHelper.register (models/ema.py:11-15)

    def _loss(self, batch, kind):
        fn = loss_registry_conditional["simple"]
        extra = {}
        if batch.get("keep_mask") is not None:      # explicit classifier-free keep mask (tests; the reference draws it inside the model)
            extra["keep_mask"] = batch["keep_mask"]
        wrapped = lambda x, tf, c, cond_drop_prob=0.1, mode="train": self.model(x, tf, c, cond_drop_prob=self.cond_drop_prob, mode=mode, **extra)
        if kind == "rl":
            # runners/diffusion.py:1101-1113: criteria(pseudo, output) = mean over ALL elements of (pseudo - output)^2, the pseudo
            # branch detached; both branches see the same x_t.  The per-sample sums and their gradient are the HIP loss kernels.
            x = q_sample(batch["x0"], batch["e"], batch["t"], alphas_cumprod(self.b))
            tf = batch["t"].float()
            output = wrapped(x, tf, batch["c"])
            pseudo_c = torch.full_like(batch["c"], (self.label_to_forget + 1) % self.n_classes)
            with torch.no_grad():
                pseudo = wrapped(x, tf, pseudo_c)
            per = _SampleLoss.apply(output, pseudo)
            return _Reduce.apply(per, 0, 0.0, self.pg if self.world > 1 else None) / float(output[0].numel())
        args = (wrapped, batch["x0"], batch["t"], batch["c"], batch["e"], self.b)
        pg = self.pg if self.world > 1 else None
        if kind == "adaga":
            return adaptive_loss(fn, *args, lambd=self.lambd, dp_group=pg)
        return fn(*args, dp_group=pg)

    def _weights_updated(self):
        if hasattr(self.model, "weights_updated"):                # native U-Net: re-lay the bf16 conv operands once per Adam step
            self.model.auto_prep = False
            self.model.weights_updated()

    def _backward(self, loss):
        self.flat.g.zero_()                                       # optimizer.zero_grad()
        loss.backward()

    # the two stages (forward pass(es), loss, backward pass): stream-ordered device work only, so each can replay as one HIP graph
    # (sfron.graphs); the decayed forget alpha arrives as a device scalar
    def _forget_pass(self, alpha, **batch):
        if self.unlearn_loss == "rl":
            ori_forget = self._loss(batch, "rl")
        else:
            ori_forget = -self._loss(batch, "adaga" if self.unlearn_loss == "adaga" else "simple")
        self._backward(alpha * ori_forget)
        return ori_forget.detach()

    def _remain_pass(self, **batch):
        ori_remain = self._loss(batch, "simple")
        self._backward(self.remain_alpha * ori_remain)
        return ori_remain.detach()

    def _stage(self, name, fn, **inputs):
        # the adaga normaliser of a data-parallel run is a collective in the middle of the stage: those runs stay eager
        if not self.use_graphs or (self.world > 1 and self.unlearn_loss == "adaga" and name == "forget"):
            return fn(**inputs)
        if name not in self._graphs:
            from . import graphs
            if self._pool is None:
                self._pool = graphs.shared_pool()
            self._graphs[name] = graphs.StageGraph(fn, warmup=1, pool=self._pool)
        return self._graphs[name](**inputs)

    def step(self, step_idx, forget, remain):
        alpha = cosine_lr_scheduler(self.forget_alpha, step_idx, self.n_iters) if self.decay else self.forget_alpha
        self.model.train()
        keys = ("x0", "c", "t", "e", "keep_mask")
        a_dev = torch.full((), float(alpha), dtype=torch.float32, device=self.flat.p.device) if self.use_graphs else alpha
        ori_forget = self._stage("forget", self._forget_pass, alpha=a_dev, **{k: forget.get(k) for k in keys})
        if self.method == "joint":
            # the forget stage's gradient is parked (the remain stage zeroes the arena) and handed to the sweep as its second gradient
            # arena: the norm pre-pass and the Adam kernel add the two (csrc/sweep.hip g2)
            if self._g_forget is None:
                self._g_forget = torch.empty_like(self.flat.g)
            self._g_forget.copy_(self.flat.g)
        else:
            if self.world > 1:
                self._dp.allreduce_flat_(self.flat.g, 64 << 20, self.pg)
            self.opt.step(max_norm=self.grad_clip, use_mask=True)
            self._weights_updated()
        ori_remain = self._stage("remain", self._remain_pass, **{k: remain.get(k) for k in keys})
        if self.method == "joint":
            if self.world > 1:
                self.flat.g.add_(self._g_forget)
            else:
                self.opt.g2 = self._g_forget
        if self.world > 1:
            self._dp.allreduce_flat_(self.flat.g, 64 << 20, self.pg)
        self.opt.step(max_norm=self.grad_clip, use_mask=False, ema=self.shadow, ema_decay=self.mu if self.mu is not None else 0.0, ema_mode=2)
        self.opt.g2 = None
        self._weights_updated()
        return {"forget_loss": ori_forget, "remain_loss": ori_remain, "alpha": alpha}

    def _train_pass(self, **batch):
        loss = self._loss(batch, "simple")
        self._backward(loss)
        return loss.detach()

    def train_step(self, batch):
        """One iteration of ``train`` / ``retrain`` (DDPM/runners/diffusion.py:121-157, :202-237): the plain loss on one batch, clip, Adam,
        EMA update -- the remain stage of ``step`` without remain_alpha, in the same one-launch sweep.  The mask plays no part."""
        self.model.train()
        keys = ("x0", "c", "t", "e", "keep_mask")
        loss = self._stage("train", self._train_pass, **{k: batch.get(k) for k in keys})
        if self.world > 1:
            self._dp.allreduce_flat_(self.flat.g, 64 << 20, self.pg)
        self.opt.step(max_norm=self.grad_clip, use_mask=False, ema=self.shadow, ema_decay=self.mu if self.mu is not None else 0.0, ema_mode=2)
        self._weights_updated()
        return {"loss": loss}

    def sampler(self, **kwargs):
        """A DDPMSampler over the LIVE model and this runner's schedule (keywords: DDPMSampler's).  Sampling between two ``step`` calls
        leaves the next step as it would have been, with ``use_graphs`` or without: no dropout draw, no change of mode, and the model's
        record of whether its convolution operands are stale is handed back as found (the next stage, eager or being captured, re-lays
        them exactly where it would have)."""
        return DDPMSampler(self.model, self.b, **kwargs)

    def ema_state_dict(self):
        return {n: v.clone() for n, v in self.flat.named_views(self.shadow).items()}

    def checkpoint(self, step):
        """[model.state_dict(), optimizer.state_dict(), step, ema_helper.state_dict()] as DDPM/runners/diffusion.py:160-171 saves
        it; the optimizer entry is in torch.optim.Adam's layout over ``model.parameters()``."""
        names = [n for n, _ in self.model.named_parameters()]
        m, v = self.flat.named_views(self.opt.m), self.flat.named_views(self.opt.v)
        state = {i: {"step": torch.tensor(float(self.opt.step_count)), "exp_avg": m[n].clone(), "exp_avg_sq": v[n].clone()}
                 for i, n in enumerate(names) if n in m and self.opt.step_count > 0}
        group = {"lr": self.opt.lr, "betas": tuple(self.opt.betas), "eps": self.opt.eps, "weight_decay": 0.0, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": False, "params": list(range(len(names)))}
        states = [{k: t.clone() for k, t in self.model.state_dict().items()}, {"state": state, "param_groups": [group]}, step]
        if self.shadow is not None:
            states.append(self.ema_state_dict())
        return states
