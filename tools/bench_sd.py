#!/usr/bin/env python3
"""BASELINE config 4 on the HIP path: SD v1 UNet nsfw_removal SFR-on iterations/s (batch 2, 64x64 latents, 77-token context).
    python tools/bench_sd.py [--steps 5] [--batch 2] [--method full|xattn]
    python tools/bench_sd.py --fused-xattn [--batch 8] [--steps 5]     both train methods, SDSFRon(fused_xattn=False) and (fused_xattn=True) taking turns
                                                                      in one process, five rounds: minimum and spread of each
    python tools/bench_sd.py --fused-wide-attn [--batch 8]             the same A-B of SDSFRon(fused_wide_attn=...) (csrc/wattn.hip)
    python tools/bench_sd.py --from-images [--batch 8] [--steps 5]     the driver loop sd.nsfw_removal from image folders: synthetic 768x1024
                                                                      photographs written with Pillow into a temporary folder, the KL-f8
                                                                      encoder with random weights, host resize and GPU resize in turn, and
                                                                      the same loop fed with resident latents"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
ap = argparse.ArgumentParser(); ap.add_argument("--steps", type=int, default=5); ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--method", default="full")
ap.add_argument("--eager", action="store_true", help="no HIP-graph replay of the stages")
ap.add_argument("--fused-xattn", action="store_true", help="A-B of the fused differentiable cross-attention (flag off = the default path)")
ap.add_argument("--fused-wide-attn", action="store_true", help="A-B of the fused wide-head self-attention (flag off = the default path)")
ap.add_argument("--from-images", action="store_true", help="time sd.nsfw_removal over image folders (front end included)")
a = ap.parse_args()
AB = ("fused_xattn", "fused_cross_attention_train") if a.fused_xattn else ("fused_wide_attn", "fused_wide_self_attention") if a.fused_wide_attn else None
from sfron import sd, sd_unet
if os.environ.get("SFRON_FUSE_SPLIT_FINISH"):       # A-B knob: 0 = every split convolution finishes its own output (before round 6, late)
    from sfron import unet as _u2; _u2._TapeNet.FUSE_SPLIT_FINISH = os.environ["SFRON_FUSE_SPLIT_FINISH"] != "0"
if os.environ.get("SFRON_BATCH_REDUCTIONS"):        # A-B knob: 0 = every parameter-gradient finish as its own launch (before round 6)
    from sfron import unet as _u; _u._TapeNet.BATCH_REDUCTIONS = os.environ["SFRON_BATCH_REDUCTIONS"] != "0"
if os.environ.get("SFRON_LOADER_WAVES"):            # A-B knob: 10 = convolution tiles in the shared-wave form
    from sfron import _lib as _L; _L.lib().sfron_gemm_loader_waves(int(os.environ["SFRON_LOADER_WAVES"]))
DEV = "cuda"
torch.manual_seed(0)
model = sd_unet.UNetModel()
g = torch.Generator().manual_seed(1)
with torch.no_grad():
    for p in model.parameters():
        if not bool(p.any()):
            p.copy_((torch.randn(p.shape, generator=g) * 0.02).to(p.device))
model.sync_bf16()
B = a.batch if not (AB and a.batch == 2) else 8
gd = torch.Generator(device=DEV).manual_seed(2)
rn = lambda *s: torch.randn(*s, device=DEV, generator=gd)
c_f, c_p = rn(1, 77, 768).expand(B, -1, -1).contiguous(), rn(1, 77, 768).expand(B, -1, -1).contiguous()
def batch():
    xf = rn(B, 4, 64, 64)
    return (dict(x_f=xf, x_p=xf, c_f=c_f, c_p=c_p, t=torch.randint(0, 1000, (B,), device=DEV, generator=gd), noise=rn(B, 4, 64, 64)),
            dict(x=rn(B, 4, 64, 64), c=c_p, t=torch.randint(0, 1000, (B,), device=DEV, generator=gd), noise=rn(B, 4, 64, 64)))
bts = [batch() for _ in range(2)]
if a.from_images:
    # the driver loop with the front end in it.  Prompt contexts are encoded once before the loop, so a stand-in cond stage (fixed random
    # [n, 77, 768]) leaves the timed part unchanged; the VAE encoder runs at its real size on random weights.
    import tempfile
    import numpy as np
    from PIL import Image
    from sfron import vae
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_resample import photograph
    enc = vae.VAEEncoder()
    gw = torch.Generator().manual_seed(3)
    enc.load_state_dict({("encoder." + n if not n.startswith("quant_conv.") else n): (torch.randn(shp, generator=gw) * (0.02 if len(shp) > 1 else 0.1)
                                                                                     + (1.0 if "norm" in n and n.endswith("weight") else 0.0))
                         for n, shp in enc.specs.items()})

    class _Cond:
        def encode(self, prompts):
            return rn(1, 77, 768).expand(len(prompts), -1, -1).contiguous()

    ldm = sd.LatentDiffusion(model, cond_stage_model=_Cond(), first_stage_encoder=enc)
    warm = 3
    with tempfile.TemporaryDirectory() as d:
        for name in ("forget", "remain"):
            os.makedirs(os.path.join(d, name))
            for i in range(2 * B):
                photograph(768, 1024, i + (100 if name == "remain" else 0)).save(os.path.join(d, name, f"{i:03d}.jpg"), quality=92)
        res = {}
        for gpu_resize in (False, True, False, True):
            fl = sd.ConceptImageLoader(os.path.join(d, "forget"), B, gpu_resize=gpu_resize)
            rl = sd.ConceptImageLoader(os.path.join(d, "remain"), B, gpu_resize=gpu_resize)
            marks = {}

            def mark(runner, step):
                if step in (warm, warm + a.steps):
                    torch.cuda.synchronize(); marks[step] = time.time()
            sd.nsfw_removal(ldm, fl, rl, warm + a.steps, a.method, use_graphs=not a.eager, log_every=0, save_every=1, on_save=mark)
            res.setdefault(gpu_resize, []).append((marks[warm + a.steps] - marks[warm]) / a.steps * 1e3)
    run = sd.SDSFRon(model, lr=1e-5, train_method=a.method, use_graphs=not a.eager)
    for i in range(warm): run.step(*bts[i % 2])
    torch.cuda.synchronize(); t0 = time.time()
    for i in range(a.steps): run.step(*bts[i % 2])
    torch.cuda.synchronize(); lat = (time.time() - t0) / a.steps * 1e3
    print(f"SD v1 nsfw_removal from image folders (768x1024 JPEG -> 512 px), batch {B}, train_method {a.method}, "
          f"{'eager' if a.eager else 'graph replay'}, ms per iteration over {a.steps} (two runs each): host resize {res[False][0]:.1f} / {res[False][1]:.1f}, "
          f"GPU resize {res[True][0]:.1f} / {res[True][1]:.1f}; resident latents (SDSFRon.step alone) {lat:.1f}")
    sys.exit(0)
if AB:
    # one model, one runner per mode (each with its own graphs); the switch is read when a stage is run eagerly or captured
    for method in ("full", "xattn"):
        runs = {}
        for on in (False, True):
            setattr(model, AB[1], False)
            runs[on] = sd.SDSFRon(model, lr=1e-5, train_method=method, use_graphs=not a.eager, **{AB[0]: on})
        times = {False: [], True: []}
        for rnd in range(6):                           # round 0 warms up (and captures)
            for on in (False, True):
                setattr(model, AB[1], on)
                torch.cuda.synchronize(); t0 = time.time()
                for i in range(a.steps): runs[on].step(*bts[i % 2])
                torch.cuda.synchronize()
                if rnd:
                    times[on].append((time.time() - t0) / a.steps * 1e3)
        off, on = times[False], times[True]
        print(f"SD v1 SFR-on iteration, batch {B}, train_method {method}: flag off min {min(off):.1f} ms (spread {max(off) - min(off):.1f}), "
              f"{AB[0]} min {min(on):.1f} ms (spread {max(on) - min(on):.1f}), difference {min(on) - min(off):+.1f} ms")
        del runs
    sys.exit(0)
run = sd.SDSFRon(model, lr=1e-5, train_method=a.method, use_graphs=not a.eager)
for i in range(2): run.step(*bts[i % 2])
torch.cuda.synchronize(); t0 = time.time()
for i in range(a.steps): run.step(*bts[i % 2])
torch.cuda.synchronize(); dt = (time.time() - t0) / a.steps
t1 = time.time()
for i in range(2): run.step(*bts[i % 2])
host = (time.time() - t1) / 2
print(f"SD v1 UNet SFR-on iteration, batch {B}, train_method {a.method}, {'eager' if a.eager else 'graph replay'}: {dt * 1e3:.0f} ms = {1 / dt:.2f} it/s (host enqueue {host * 1e3:.0f} ms)")
