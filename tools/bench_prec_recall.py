#!/usr/bin/env python3
"""Time precision / recall and the Inception Score (sfron.evaluator over csrc/manifold.hip) at D = 2048: ``manifold_radii`` of one set,
``evaluate_pr`` of two sets and the score of N x 1008 logits, each against the same work as torch ops on the device in the reference's
schedule (fp32 ``mm`` + ``topk`` / comparisons in 10 000-row blocks).  HIP events around each call, warm-up first; --rounds rounds of
--iters calls, a round's time is its median call; prints one JSON line per N with the median and the spread of the rounds and the
product's TFLOP/s (2 N^2 D per distance matrix).
    python tools/bench_prec_recall.py [--n 10000 50000] [--d 2048] [--iters 3] [--warmup 1] [--rounds 3] [--no-torch]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

PEAK_F32_MATRIX = 157.3e12          # MI355X fp32 matrix peak, FLOP/s
BLOCK = 10000


def timed(fn, iters, rounds):
    out = []
    for _ in range(rounds):
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        out.append(statistics.median(ts))
    return out


def torch_distances(u, nu, v, nv):
    return torch.clamp_min(nu[:, None] - 2 * (u @ v.T) + nv[None, :], 0)


def torch_radii(x, k=3):
    n = (x * x).sum(1)
    out = []
    for b in range(0, len(x), BLOCK):
        d = torch.cat([torch_distances(x[b:b + BLOCK], n[b:b + BLOCK], x[c:c + BLOCK], n[c:c + BLOCK]) for c in range(0, len(x), BLOCK)], 1)
        out.append(torch.topk(d, k + 1, dim=1, largest=False).values[:, k:k + 1])
    return torch.cat(out)


def torch_pr(x1, r1, x2, r2):
    n1, n2 = (x1 * x1).sum(1), (x2 * x2).sum(1)
    s1 = torch.zeros(len(x1), dtype=torch.bool, device=x1.device)
    s2 = torch.zeros(len(x2), dtype=torch.bool, device=x1.device)
    for b in range(0, len(x1), BLOCK):
        for c in range(0, len(x2), BLOCK):
            d = torch_distances(x1[b:b + BLOCK], n1[b:b + BLOCK], x2[c:c + BLOCK], n2[c:c + BLOCK])
            s1[b:b + BLOCK] |= (d <= r2[c:c + BLOCK, 0][None, :]).any(1)
            s2[c:c + BLOCK] |= (d <= r1[b:b + BLOCK, 0][:, None]).any(0)
    return s2.double().mean(), s1.double().mean()


def torch_is(logits, split=5000):
    p = torch.softmax(logits, 1)
    scores = []
    for i in range(0, len(p), split):
        part = p[i:i + split]
        kl = part * (torch.log(part) - torch.log(part.mean(0, keepdim=True)))
        scores.append(torch.exp(kl.sum(1).mean()))
    return torch.stack(scores).mean()


def summary(rounds):
    med = statistics.median(rounds)
    return {"ms": round(med, 3), "ms_rounds": [round(r, 3) for r in rounds], "spread": round((max(rounds) - min(rounds)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10000, 50000])
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    from sfron import evaluator
    est = evaluator.ManifoldEstimator()
    for n in a.n:
        g = torch.Generator().manual_seed(n)
        x1 = (torch.randn(n, 4, generator=g) @ torch.randn(4, a.d, generator=g) / 2 + 0.02 * torch.randn(n, a.d, generator=g) + 0.5).cuda()
        x2 = (1.15 * torch.randn(n, 4, generator=g) @ torch.randn(4, a.d, generator=g) / 2 + 0.02 * torch.randn(n, a.d, generator=g) + 0.5).cuda()
        logits = (4 * torch.randn(n, 1008, generator=g)).cuda()
        r1, r2 = est.manifold_radii(x1), est.manifold_radii(x2)
        flop = 2.0 * n * n * a.d
        out = {"metric": "ManifoldEstimator.manifold_radii / evaluate_pr and inception_scores", "n": n, "d": a.d, "peak_f32_matrix_flops": PEAK_F32_MATRIX}
        jobs = {"manifold_radii": lambda: est.manifold_radii(x1), "evaluate_pr": lambda: est.evaluate_pr(x1, r1, x2, r2),
                "inception_score": lambda: evaluator.inception_scores(logits).mean().item()}
        if not a.no_torch:
            jobs.update({"torch_radii": lambda: torch_radii(x1), "torch_pr": lambda: [v.item() for v in torch_pr(x1, r1, x2, r2)],
                         "torch_is": lambda: torch_is(logits).item()})
        for name, fn in jobs.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            out[name] = summary(timed(fn, a.iters, a.rounds))
            if name.endswith(("radii", "pr")):
                out[name]["tflops"] = round(flop / out[name]["ms"] / 1e9, 1)
                out[name]["frac_peak"] = round(flop / out[name]["ms"] / 1e-3 / PEAK_F32_MATRIX, 4)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
