"""Writes tests/golden/evaluator.npz from the reference's own DDPM/evaluator.py:

    python tests/golden/make_evaluator_golden.py --reference <checkout of the reference project>

The reference module is imported under stub modules as make_fid_golden.py imports it.  Its OWN ``ManifoldEstimator.manifold_radii`` /
``evaluate_pr`` / ``_numpy_partition`` and ``Evaluator.compute_inception_score`` produce every recorded result.  Its two TensorFlow pieces
get stand-ins written here: a ``DistanceBlock`` whose ``pairwise_distances`` / ``less_thans`` are the fp32 expressions of the reference's
graph in numpy (tests/prec_recall_ref.py), and a session whose ``run`` returns ``softmax(acts @ w)`` in fp32.

Precision / recall cases are integer lattices (six random centres in lo..hi, each coordinate redrawn with probability p, p different for
the two sets): every dot product and norm is an integer below 2^24, every distance exact in fp32 in any summation order, so the file is
a yardstick without a tolerance; integer distances tie often, which puts ``<=`` and the k-th selection to work.  A case is REFUSED unless
precision and recall lie strictly between 0 and 1, at least one d == r tie exists, and the ``<`` variant and the k - 1 / k + 1 variants
each give a different (precision, recall) pair.  Inputs are stored as int8.

  <inputs>/x1, x2           int8 [N1][D], [N2][D] for inputs A .. E
  <entry>/inputs            which inputs;  <entry>/nhood, clamp (-1 = None), batches (row, col)
  <entry>/radii1, radii2    fp32 [N][K];  in1 [N1][K2], in2 [N2][K1] bool;  precision [K1], recall [K2] fp64
  <entry>/ties              the number of d == r pairs (nhood 3 entries)
  is/acts                   int8 [1203][2048] (a lattice in 0..2 around six centres with disjoint supports);  is/w_block int8 [16][1008], tiled 128 times along k and multiplied by
                            is/scale (fp32) it is the head's matrix w [2048][1008]: |logit| <= 20, no probability underflows
  is37/.., is1203/..        n, split_size (5000 and 500: three splits, the last short), ref32 = the reference's float, ref64 = the same
                            formula in fp64
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import prec_recall_ref as ref                      # noqa: E402
from make_fid_golden import load_evaluator        # noqa: E402

SEED = 20260114
# inputs: N1, N2, D, lo, hi, p1, p2
INPUTS = {"A": (300, 260, 64, -2, 2, 0.25, 0.35), "B": (1100, 900, 64, -2, 2, 0.25, 0.35), "C": (300, 260, 192, -2, 2, 0.05, 0.07),
          "D": (257, 129, 2048, -1, 1, 0.004, 0.006), "E": (513, 385, 2048, -2, 2, 0.003, 0.004)}
# entry: inputs, nhood, clamp, (row_batch, col_batch)
ENTRIES = {"a": ("A", (3,), None, (10000, 10000)), "a_k235": ("A", (2, 3, 5), None, (10000, 10000)),
           "a_clamp50": ("A", (3,), 50, (10000, 10000)), "b": ("B", (3,), None, (10000, 10000)), "c_chunk": ("C", (3,), None, (128, 96)),
           "d": ("D", (3,), None, (10000, 10000)), "e": ("E", (3,), None, (10000, 10000))}


class NumpyDistanceBlock:
    """DistanceBlock's fp32 branch: the graph's expressions in numpy."""
    strict = False

    def __init__(self, session):
        self.session = session

    def pairwise_distances(self, U, V):
        return ref.pairwise(U, V, np.float32)

    def less_thans(self, batch_1, radii_1, batch_2, radii_2):
        dist32 = ref.pairwise(batch_1, batch_2, np.float32)[..., None]
        if self.strict:
            return np.any(dist32 < radii_2, axis=1), np.any(dist32 < radii_1[:, None], axis=0)
        return np.any(dist32 <= radii_2, axis=1), np.any(dist32 <= radii_1[:, None], axis=0)


class StrictDistanceBlock(NumpyDistanceBlock):
    strict = True


class SoftmaxSession:
    """sess.run(self.softmax, {self.softmax_input: acts}) -> softmax(acts @ w) in fp32."""

    def __init__(self, w, key):
        self.w, self.key = w, key

    def run(self, fetch, feed_dict):
        return ref.softmax_rows(np.asarray(feed_dict[self.key], dtype=np.float32) @ self.w).astype(np.float32)


def run_reference(ev, block, x1, x2, nhood, clamp, batches):
    ev.DistanceBlock = block
    est = ev.ManifoldEstimator(None, row_batch_size=batches[0], col_batch_size=batches[1], nhood_sizes=list(nhood), clamp_to_percentile=clamp)
    r1, r2 = est.manifold_radii(x1), est.manifold_radii(x2)
    s1 = np.zeros([len(x1), r2.shape[1]], dtype=bool)
    s2 = np.zeros([len(x2), r1.shape[1]], dtype=bool)
    for b1 in range(0, len(x1), batches[0]):               # evaluate_pr's loop, to keep the flag arrays it reduces
        for b2 in range(0, len(x2), batches[1]):
            i1, i2 = est.distance_block.less_thans(x1[b1:b1 + batches[0]], r1[b1:b1 + batches[0]], x2[b2:b2 + batches[1]], r2[b2:b2 + batches[1]])
            s1[b1:b1 + batches[0]] |= i1
            s2[b2:b2 + batches[1]] |= i2
    precision, recall = est.evaluate_pr(x1, r1, x2, r2)
    assert np.array_equal(precision, np.mean(s2.astype(np.float64), axis=0)) and np.array_equal(recall, np.mean(s1.astype(np.float64), axis=0))
    return dict(radii1=r1, radii2=r2, in1=s1, in2=s2, precision=precision, recall=recall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "evaluator.npz"))
    args = ap.parse_args()
    ev = load_evaluator(args.reference)
    out = {}
    data = {}
    for i, (key, (n1, n2, D, lo, hi, p1, p2)) in enumerate(INPUTS.items()):
        rng = np.random.default_rng(SEED + i)
        x1, centres = ref.lattice(n1, D, lo, hi, p1, rng)
        x2, _ = ref.lattice(n2, D, lo, hi, p2, rng, centres)
        assert max(float(np.sum(np.square(x), 1).max()) for x in (x1, x2)) * 4 < 2 ** 24
        data[key] = (x1, x2)
        out[key + "/x1"], out[key + "/x2"] = x1.astype(np.int8), x2.astype(np.int8)
        base = run_reference(ev, NumpyDistanceBlock, x1, x2, (3,), None, (10000, 10000))
        pair = (float(base["precision"][0]), float(base["recall"][0]))
        d = ref.pairwise(x1, x2, np.float32)
        ties = int((d == base["radii2"][:, 0][None]).sum() + (d == base["radii1"][:, 0][:, None]).sum())
        variants = {"<": run_reference(ev, StrictDistanceBlock, x1, x2, (3,), None, (10000, 10000)),
                    "k=2": run_reference(ev, NumpyDistanceBlock, x1, x2, (2,), None, (10000, 10000)),
                    "k=4": run_reference(ev, NumpyDistanceBlock, x1, x2, (4,), None, (10000, 10000))}
        vp = {k: (float(v["precision"][0]), float(v["recall"][0])) for k, v in variants.items()}
        print(f"inputs {key}: precision {pair[0]:.3f} recall {pair[1]:.3f}, {ties} d == r ties, variants {vp}")
        if not (0 < pair[0] < 1 and 0 < pair[1] < 1):
            raise SystemExit(f"inputs {key}: precision / recall {pair} not strictly between 0 and 1: pick another seed")
        if ties < 1:
            raise SystemExit(f"inputs {key}: no d == r tie: pick another seed")
        for k, v in vp.items():
            if v == pair:
                raise SystemExit(f"inputs {key}: the {k} variant gives the same pair {v}: pick another seed")
        out[key + "/ties"] = np.int64(ties)
    for name, (src, nhood, clamp, batches) in ENTRIES.items():
        x1, x2 = data[src]
        res = run_reference(ev, NumpyDistanceBlock, x1, x2, nhood, clamp, batches)
        mine = ref.evaluate(x1, x2, nhood, np.float32, clamp)
        for k, v in res.items():
            assert np.array_equal(v, mine[k]), (name, k)          # the restatement of tests/prec_recall_ref.py agrees
            out[f"{name}/{k}"] = v
        out[name + "/inputs"] = np.str_(src)
        out[name + "/nhood"] = np.asarray(nhood, dtype=np.int32)
        out[name + "/clamp"] = np.float64(-1 if clamp is None else clamp)
        out[name + "/batches"] = np.asarray(batches, dtype=np.int64)
        print(f"entry {name}: precision {res['precision']} recall {res['recall']}")

    # ---- Inception Score
    rng = np.random.default_rng(SEED + 100)
    # centre c is non-zero only where (k % 16) % 6 == c: against the 16-row period of w the six centres get six different logit rows
    centres = rng.integers(0, 3, (6, 2048)) * (((np.arange(2048) % 16) % 6)[None, :] == np.arange(6)[:, None])
    acts, _ = ref.lattice(1203, 2048, 0, 2, 0.003, rng, centres)
    w_block = rng.integers(-2, 3, (16, 1008)).astype(np.int8)
    w_int = np.tile(w_block.astype(np.float32), (128, 1))
    scale = np.float32(20.0 / np.abs(acts.astype(np.float64) @ w_int.astype(np.float64)).max() * (1 - 2.0 ** -10))
    w = (w_int * scale).astype(np.float32)
    out["is/acts"], out["is/w_block"], out["is/scale"] = acts.astype(np.int8), w_block, scale
    e = object.__new__(ev.Evaluator)
    e.softmax_input, e.softmax, e.softmax_batch_size = "softmax_input", "softmax", 512
    e.sess = SoftmaxSession(w, e.softmax_input)
    for name, n, split in (("is37", 37, 5000), ("is1203", 1203, 500)):
        a = acts[:n]
        z = a @ w
        assert np.abs(z).max() <= 20 and ref.softmax_rows(z).min() > 0, (np.abs(z).max(), ref.softmax_rows(z).min())
        ref32 = e.compute_inception_score(a, split_size=split)
        ref64 = ref.inception_score(a, w, split, np.float64)
        assert ref32 == ref.inception_score(a, w, split, np.float32)
        out[name + "/n"], out[name + "/split_size"] = np.int64(n), np.int64(split)
        out[name + "/ref32"], out[name + "/ref64"] = np.float64(ref32), np.float64(ref64)
        print(f"{name}: reference {ref32!r}, fp64 {ref64!r}, |diff| {abs(ref32 - ref64):.3e}")
    np.savez_compressed(args.out, **out)
    size = os.path.getsize(args.out)
    print("wrote", args.out, size, "bytes")
    assert size < (1 << 20), "a committed file stays under 1 MiB"


if __name__ == "__main__":
    main()
