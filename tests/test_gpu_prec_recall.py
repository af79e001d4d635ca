"""csrc/manifold.hip and sfron.evaluator on the GPU.

Lattice entries of tests/golden/evaluator.npz (the reference's own ManifoldEstimator on integer inputs: every distance exact in fp32):
radii, both flag arrays, precision and recall BIT-EQUAL, through the C entry points on guarded buffers and through the Python layer.
Chunked launches, permuted rows and padded rows (NaN sentinels in the gaps) give the same bits.  Edge shapes -- one past the 128-row /
128-column tile and its 32-wide results, widths that are no multiple of the 32-column k step, four radii with nhood up to 7, duplicate
points -- against the numpy restatement on integer inputs, exactly.

Float features: radii under bound32 against fp64 with the numpy fp32 restatement as the yardstick; a flag must equal the fp64 decision
wherever the closest any of its pairs comes to its radius exceeds the fp32 restatement's largest distance error on that case; the rest is
left out (at most 1 % of the flags; the share is printed with -s).  A point's distance to itself is exactly 0 on float features too: with
radii of 0 every point of a set without duplicates is found inside its own sphere, and nothing else is.

sfron_gemm_nt_f32: exact on integer operands; Gaussian operands under bound32 with margin 2, the yardstick being the fp32 CPU product
(``A @ B.T``) against fp64.

Inception Score: the fixture's cases under bound32 (reference = the fp64 value, yardstick = the reference implementation's float); one
end-to-end case over the random-weight network of tests/inception_torch_ref.py against the torch head WITHOUT its bias in fp64 on the
same features (yardstick: the same formula in fp32)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import inception_torch_ref as iref
import prec_recall_ref as ref
from dit_rows_ref import RECORD, bound32, guarded, untouched

gpu = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = 1001


def L():
    from sfron import _lib
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev_rows(x, ld=None):
    """x (numpy [n][D]) in a guarded device buffer with rows ld apart."""
    v, chk = guarded(x.shape, torch.float32, ld=ld, device=DEV)
    v.copy_(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)))
    return v, chk


def raw_radii(x, nhood, batches=(0, 0), ld=None):
    v, cx = dev_rows(x, ld)
    N, D = x.shape
    nbytes = L().sfron_manifold_radii_workspace(N, batches[0], batches[1])
    ws, cw = guarded((nbytes // 4,), torch.float32, device=DEV)
    out, co = guarded((N, len(nhood)), torch.float32, device=DEV)
    nh = (ctypes.c_int * len(nhood))(*nhood)
    st = L().sfron_manifold_radii_batched(v.data_ptr(), N, D, v.stride(0), batches[0], batches[1], nh, len(nhood), out.data_ptr(), ws.data_ptr(),
                                          nbytes, stream())
    assert st == 0, st
    torch.cuda.synchronize()
    for c in (cx, cw, co):
        c("manifold_radii")
    return out.cpu().numpy().copy()


def raw_pr(x1, r1, x2, r2, ld1=None, ld2=None):
    v1, c1 = dev_rows(x1, ld1)
    v2, c2 = dev_rows(x2, ld2)
    g1, cr1 = dev_rows(r1)
    g2, cr2 = dev_rows(r2)
    in1, ci1 = guarded((len(x1), r2.shape[1]), torch.uint8, device=DEV)
    in2, ci2 = guarded((len(x2), r1.shape[1]), torch.uint8, device=DEV)
    in1.zero_()
    in2.zero_()
    st = L().sfron_manifold_pr(v1.data_ptr(), len(x1), g1.data_ptr(), r1.shape[1], v2.data_ptr(), len(x2), g2.data_ptr(), r2.shape[1], x1.shape[1],
                               v1.stride(0), v2.stride(0), in1.data_ptr(), in2.data_ptr(), stream())
    assert st == 0, st
    torch.cuda.synchronize()
    for c in (c1, c2, cr1, cr2, ci1, ci2):
        c("manifold_pr")
    a, b = in1.cpu().numpy().copy(), in2.cpu().numpy().copy()
    assert set(np.unique(a)) <= {0, 1} and set(np.unique(b)) <= {0, 1}
    return a.astype(bool), b.astype(bool)


def api(x1, x2, nhood=(3,), clamp=None, batches=(10000, 10000)):
    from sfron import evaluator
    est = evaluator.ManifoldEstimator(row_batch_size=batches[0], col_batch_size=batches[1], nhood_sizes=nhood, clamp_to_percentile=clamp)
    t1, t2 = (x if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(DEV) for x in (x1, x2))
    r1, r2 = est.manifold_radii(t1), est.manifold_radii(t2)
    assert r1.is_cuda and r1.dtype == torch.float32 and r1.shape == (t1.shape[0], len(nhood))
    in1, in2 = est.status(t1, r1, t2, r2)
    p, r = est.evaluate_pr(t1, r1, t2, r2)
    assert p.dtype == np.float64 and r.dtype == np.float64
    return dict(radii1=r1.cpu().numpy(), radii2=r2.cpu().numpy(), in1=in1.cpu().numpy().astype(bool), in2=in2.cpu().numpy().astype(bool),
                precision=p, recall=r)


def same_bits(a, b, what):
    for k in ("radii1", "radii2"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), (what, k)
    for k in ("in1", "in2", "precision", "recall"):
        assert np.array_equal(a[k], b[k]), (what, k)


# ------------------------------------------------------------------------------------------------ lattice entries
@gpu
@pytest.mark.parametrize("name", ref.PR_ENTRIES)
def test_lattice_entries_bit_equal(name):
    e = ref.pr_entry(name)
    got = api(e["x1"], e["x2"], e["nhood"], e["clamp"], e["batches"])
    ref.accept_pr(e, got)
    if e["clamp"] is None:          # the C entry points on guarded buffers, in the entry's own batches
        b = tuple(min(v, 10000) for v in e["batches"])
        r1, r2 = raw_radii(e["x1"], e["nhood"], b), raw_radii(e["x2"], e["nhood"], b)
        in1, in2 = raw_pr(e["x1"], r1, e["x2"], r2)
        p, r = ref.prec_recall(in1, in2)
        ref.accept_pr(e, dict(radii1=r1, radii2=r2, in1=in1, in2=in2, precision=p, recall=r))


@gpu
def test_chunked_equals_unchunked():
    e = ref.pr_entry("b")
    same_bits(api(e["x1"], e["x2"], e["nhood"], None, (128, 96)), api(e["x1"], e["x2"], e["nhood"]), "lattice b")
    c = float_setup("f64")
    same_bits(api(c["x1"], c["x2"], (3,), None, (128, 96)), c["got"], "float f64")
    same_bits(api(c["x1"], c["x2"], (3,), None, (100, 257)), c["got"], "float f64, odd batches")


_float = {}


def float_setup(name):
    if name not in _float:
        _, N1, N2, D, seed = next(c for c in ref.FLOAT_CASES if c[0] == name)
        c = ref.float_case(N1, N2, D, seed)
        c["got"] = api(c["x1"], c["x2"])
        _float[name] = c
    return _float[name]


@gpu
def test_row_permutation_permutes_the_outputs():
    c = float_setup("f64")
    rng = np.random.default_rng(11)
    p1, p2 = rng.permutation(len(c["x1"])), rng.permutation(len(c["x2"]))
    got = api(c["x1"][p1], c["x2"][p2])
    base = c["got"]
    same_bits(got, dict(radii1=base["radii1"][p1], radii2=base["radii2"][p2], in1=base["in1"][p1], in2=base["in2"][p2],
                        precision=base["precision"], recall=base["recall"]), "permuted")
    e = ref.pr_entry("d")
    got = api(e["x1"][::-1].copy(), e["x2"])
    ref.accept_pr(e, dict(got, radii1=got["radii1"][::-1], in1=got["in1"][::-1]))


@gpu
@pytest.mark.parametrize("name", ["f64", "d"])
def test_padded_rows_give_the_same_bits(name):
    if name == "d":
        e = ref.pr_entry("d")
        x1, x2, base = e["x1"], e["x2"], None
    else:
        c = float_setup(name)
        x1, x2, base = c["x1"], c["x2"], c["got"]
    D = x1.shape[1]
    v1, c1 = dev_rows(x1, D + 12)          # the gaps hold NaN sentinels
    v2, c2 = dev_rows(x2, D + 4)
    got = api(v1, v2)
    c1("padded x1")
    c2("padded x2")
    if base is None:
        ref.accept_pr(e, got)
    else:
        same_bits(got, base, "padded")
    r1 = raw_radii(x1, (3,), ld=D + 12)
    assert np.array_equal(r1.view(np.int32), got["radii1"].view(np.int32))
    in1, in2 = raw_pr(x1, got["radii1"], x2, got["radii2"], ld1=D + 12, ld2=D + 4)
    assert np.array_equal(in1, got["in1"]) and np.array_equal(in2, got["in2"])


# ------------------------------------------------------------------------------------------------ edges, exactly
def ints(n, D, seed, lo=-2, hi=2):
    return np.random.default_rng(seed).integers(lo, hi + 1, (n, D)).astype(np.float32)


# (N1, N2, D, nhood): one past the 128 tile (129), past two tiles (257), past one 32-wide result (33) and one 64-row wave (65);
# D = 4, 20 and 36: under, and one step past, the 32-column k step; four radii with nhood up to 7
EDGES = [(4, 4, 8, (3,)), (129, 257, 36, (3,)), (257, 129, 20, (1, 3, 5, 7)), (33, 65, 4, (2,)), (130, 8, 2048, (7,)), (8, 129, 68, (1, 2, 3, 4))]


@gpu
@pytest.mark.parametrize("N1,N2,D,nhood", EDGES)
def test_edges_against_the_restatement(N1, N2, D, nhood):
    lo, hi = (-1, 1) if D <= 8 else (-2, 2)
    x1, x2 = ints(N1, D, 3 * N1 + D, lo, hi), ints(N2, D, 5 * N2 + D + 1, lo, hi)
    want = ref.evaluate(x1, x2, nhood, np.float32)
    r1, r2 = raw_radii(x1, nhood), raw_radii(x2, nhood)
    assert np.array_equal(r1, want["radii1"]) and np.array_equal(r2, want["radii2"])
    in1, in2 = raw_pr(x1, r1, x2, r2)
    assert np.array_equal(in1, want["in1"]) and np.array_equal(in2, want["in2"])
    same_bits(api(x1, x2, nhood), want, "api")


@gpu
def test_one_row_against_130_and_duplicate_points():
    x1, x2 = ints(1, 36, 1), ints(130, 36, 2)
    r2 = raw_radii(x2, (3,))
    r1 = np.array([[float(np.median(ref.pairwise(x1, x2, np.float32)))]], dtype=np.float32)      # one row has no k-th neighbour: a given radius
    want1, want2 = ref.status(x1, r1, x2, r2, np.float32)
    in1, in2 = raw_pr(x1, r1, x2, r2)
    assert np.array_equal(in1, want1) and np.array_equal(in2, want2) and 0 < in2.sum() < in2.size
    in2b, in1b = raw_pr(x2, r2, x1, r1)                                                          # and as set 2
    w2b, w1b = ref.status(x2, r2, x1, r1, np.float32)
    assert np.array_equal(in2b, w2b) and np.array_equal(in1b, w1b)
    # duplicates: several zero distances -- rows 0..4 equal, so their radii at k <= 4 are 0 and every copy is inside the others' spheres
    d = ints(70, 20, 9)
    d[1:5] = d[0]
    d[40] = d[33]
    want = ref.evaluate(d, d[::-1].copy(), (1, 4, 5), np.float32)
    assert (want["radii1"][:5, :2] == 0).all() and (want["radii1"][:5, 2] > 0).all()
    r = raw_radii(d, (1, 4, 5))
    assert np.array_equal(r, want["radii1"])
    in1, in2 = raw_pr(d, r, d[::-1].copy(), r[::-1].copy())
    assert np.array_equal(in1, want["in1"]) and np.array_equal(in2, want["in2"])


# ------------------------------------------------------------------------------------------------ the product
def raw_gemm(A, B, lda=None, ldb=None, ldc=None):
    a, ca = dev_rows(A, lda)
    b, cb = dev_rows(B, ldb)
    c, cc = guarded((len(A), len(B)), torch.float32, ld=ldc, device=DEV)
    st = L().sfron_gemm_nt_f32(a.data_ptr(), len(A), a.stride(0), b.data_ptr(), len(B), b.stride(0), A.shape[1], c.data_ptr(), c.stride(0), stream())
    assert st == 0, st
    torch.cuda.synchronize()
    for chk in (ca, cb, cc):
        chk("gemm_nt_f32")
    return c.cpu().numpy().copy()


@gpu
@pytest.mark.parametrize("M,N,K", [(5, 1008, 2048), (130, 1008, 2048), (257, 129, 36)])
def test_gemm_nt_integer_operands_are_exact(M, N, K):
    A, B = ints(M, K, M + K), ints(N, K, N + K + 7, -3, 3)           # asymmetric operands: a swapped row / column cannot pass
    want = (A.astype(np.float64) @ B.astype(np.float64).T)
    assert np.abs(want).max() < 2 ** 24
    got = raw_gemm(A, B, lda=K + 4, ldb=K + 8, ldc=N + 3)
    assert np.array_equal(got.astype(np.float64), want)


@gpu
def test_gemm_nt_gaussian_under_bound32():
    rng = np.random.default_rng(21)
    A, B = rng.standard_normal((130, 2048)).astype(np.float32), rng.standard_normal((1008, 2048)).astype(np.float32)
    ref64 = A.astype(np.float64) @ B.astype(np.float64).T
    err, yard = bound32(torch.from_numpy(raw_gemm(A, B)), torch.from_numpy(ref64), torch.from_numpy(A @ B.T), name="gemm_nt_f32", margin=2.0)
    print(f"gemm_nt_f32 130 x 1008 x 2048: max error {err:.3e}, the fp32 CPU product {yard:.3e}")


# ------------------------------------------------------------------------------------------------ float features
@gpu
@pytest.mark.parametrize("name", [c[0] for c in ref.FLOAT_CASES])
def test_float_features(name):
    c = float_setup(name)
    got = c["got"]
    for k in ("radii1", "radii2"):
        err, yard = bound32(torch.from_numpy(got[k]), torch.from_numpy(c["ref64"][k]), torch.from_numpy(c["ref32"][k]), name=f"{name}/{k}")
        print(f"{name}/{k}: max error {err:.3e}, the fp32 restatement {yard:.3e}")
    share = ref.accept_flags(c, got["in1"], got["in2"])
    differ = int((got["in1"] != c["ref64"]["in1"]).sum() + (got["in2"] != c["ref64"]["in2"]).sum())
    print(f"{name}: precision {got['precision'][0]:.4f} (fp64 {c['ref64']['precision'][0]:.4f}), recall {got['recall'][0]:.4f} "
          f"(fp64 {c['ref64']['recall'][0]:.4f}); eps {c['eps']:.3e}; share of flags left out {share:.5f}; flags that differ from fp64: {differ}")


@gpu
@pytest.mark.parametrize("name", [c[0] for c in ref.FLOAT_CASES])
def test_self_distance_is_exactly_zero_on_float_features(name):
    """The norm and the diagonal dot product are summed in the same order, so d(i, i) = (n - 2 n) + n = 0 exactly: with every radius 0,
    x against itself finds each point inside its own sphere (in1 and in2 all set), x against another set finds nothing."""
    c = float_setup(name)
    for x in (c["x1"], c["x2"]):
        assert len(np.unique(x, axis=0)) == len(x)
        zero = np.zeros((len(x), 1), dtype=np.float32)
        in1, in2 = raw_pr(x, zero, x, zero)
        assert in1.all() and in2.all()
    in1, in2 = raw_pr(c["x1"], np.zeros((len(c["x1"]), 1), np.float32), c["x2"], np.zeros((len(c["x2"]), 1), np.float32))
    assert not in1.any() and not in2.any()


# ------------------------------------------------------------------------------------------------ Inception Score
def raw_scores(logits, split, ld=None):
    z, cz = dev_rows(logits, ld)
    N, C = logits.shape
    nbytes = L().sfron_inception_score_workspace(N, C, split)
    ws, cw = guarded(((nbytes + 3) // 4,), torch.float32, device=DEV)
    ns = (N + split - 1) // split
    out, co = guarded((ns * 2,), torch.float32, device=DEV)           # fp64 [ns]
    st = L().sfron_inception_score(z.data_ptr(), N, C, z.stride(0), split, out.data_ptr(), ws.data_ptr(), nbytes, stream())
    assert st == 0, st
    torch.cuda.synchronize()
    for chk in (cz, cw, co):
        chk("inception_score")
    return out.cpu().numpy().view(np.float64).copy(), z.cpu().numpy()


@gpu
@pytest.mark.parametrize("name", ref.IS_ENTRIES)
def test_inception_score_fixture_cases(name):
    from sfron import evaluator
    e = ref.is_entry(name)
    z = (e["acts"] @ e["w"]).astype(np.float32)
    scores, probs = raw_scores(z, e["split_size"], ld=1012)
    assert len(scores) == -(-len(z) // e["split_size"])
    ref.accept_is(e, float(np.mean(scores)), name=name)
    p64 = ref.softmax_rows(z.astype(np.float64))
    bound32(torch.from_numpy(probs), torch.from_numpy(p64), torch.from_numpy(ref.softmax_rows(z)), name=name + "/softmax")
    bound32(torch.from_numpy(scores), torch.from_numpy(ref.split_scores(p64, e["split_size"])),
            torch.from_numpy(ref.split_scores(ref.softmax_rows(z), e["split_size"]).astype(np.float64)), name=name + "/split scores")
    # the head on the device: features x fc.weight through sfron_gemm_nt_f32, then the Python layer
    from sfron import inception
    m = inception.InceptionV3.__new__(inception.InceptionV3)
    m.fc_weight = torch.from_numpy(np.ascontiguousarray(e["w"].T)).to(DEV)
    got = evaluator.compute_inception_score(m, torch.from_numpy(e["acts"]).to(DEV), split_size=e["split_size"])
    ref.accept_is(e, got, name=name + "/device head")
    print(f"{name}: reference {e['ref32']!r}, fp64 {e['ref64']!r}, kernel on CPU logits {float(np.mean(scores))!r}, device head {got!r}")


@gpu
def test_zero_probability_gives_a_finite_score():
    z = np.random.default_rng(5).standard_normal((9, 1008)).astype(np.float32)
    z[3, 17] = -200.0
    z[5, :500] = -150.0
    scores, probs = raw_scores(z, 5000)
    assert probs[3, 17] == 0 and (probs[5, :500] == 0).all()
    assert np.isfinite(scores).all()
    want = ref.split_scores(ref.softmax_rows(z.astype(np.float64)), 5000)            # in fp64 nothing underflows here
    p32 = ref.softmax_rows(z)                                                        # the fp32 formula with the zero terms counted as 0
    with np.errstate(divide="ignore", invalid="ignore"):
        kl = np.where(p32 > 0, p32 * (np.log(p32) - np.log(np.mean(p32, 0, keepdims=True))), np.float32(0))
    yard = np.exp(np.mean(np.sum(kl, 1)))
    bound32(torch.from_numpy(scores), torch.from_numpy(want), torch.tensor([float(yard)], dtype=torch.float64), name="zero probability")


@pytest.fixture(scope="module")
def net(tmp_path_factory):
    from sfron import inception
    root = tmp_path_factory.mktemp("evaluator")
    g = torch.Generator().manual_seed(5)
    real = torch.randint(0, 256, (12, 24, 24, 3), generator=g, dtype=torch.uint8)
    # the sample set: nine of the reference images under a little noise, so that the two manifolds overlap
    fake = (real[:9].float() + torch.randint(-8, 9, (9, 24, 24, 3), generator=g).float()).clamp(0, 255).to(torch.uint8)
    os.makedirs(root / "run" / "ref")
    np.savez(str(root / "run" / "ref" / "images.npz"), arr_0=real.numpy())
    np.savez(str(root / "fake.npz"), arr_0=fake.numpy())
    m = iref.randomize(iref.FIDInceptionV3(), 11, probe=real[:2])
    ckpt = str(root / "inception.pt")
    torch.save(m.state_dict(), ckpt)
    model = inception.InceptionV3(device=DEV).load_state_dict(m.state_dict())
    return root, ckpt, m, model, real, fake


@gpu
def test_inception_score_end_to_end(net):
    from sfron import _lib, evaluator, inception
    root, ckpt, m, model, real, fake = net
    assert model.fc_weight.dtype == torch.float32 and tuple(model.fc_weight.shape) == (1008, 2048)
    assert torch.equal(model.fc_weight.cpu(), m.fc.weight.detach())
    f = model.forward_u8(real, taps=(2048,))[2048]
    got = evaluator.compute_inception_score(model, f, split_size=5)
    w = m.fc.weight.detach().numpy().T
    want64 = ref.inception_score(f.cpu().numpy(), w, 5, np.float64)
    want32 = ref.inception_score(f.cpu().numpy(), w, 5, np.float32)
    biased = ref.inception_score(f.cpu().numpy(), w, 5, np.float64, bias=m.fc.bias.detach().numpy())
    t = lambda v: torch.tensor([v], dtype=torch.float64)
    err, yard = bound32(t(got), t(want64), t(want32), name="IS end to end")
    print(f"IS of 12 images: {got!r}, torch head without bias in fp64 {want64!r} (|diff| {err:.3e}), in fp32 {want32!r} (yardstick {yard:.3e}); "
          f"with fc.bias it would be {biased!r}")
    with pytest.raises(AssertionError):
        bound32(t(biased), t(want64), t(want32))
    sd = {k: v for k, v in m.state_dict().items() if not k.startswith("fc.")}
    headless = inception.InceptionV3(device=DEV).load_state_dict(sd)
    with pytest.raises(_lib.SfronError, match="fc.weight"):
        headless.logits(f)


# ------------------------------------------------------------------------------------------------ refusals
@gpu
def test_refusals_leave_the_outputs_untouched():
    x, _ = dev_rows(ints(40, 16, 1), 20)
    out, co = guarded((40, 4), torch.float32, device=DEV)
    ws, cw = guarded((1 << 16,), torch.float32, device=DEV)
    i1, c1 = guarded((40, 4), torch.uint8, device=DEV)
    i2, c2 = guarded((40, 4), torch.uint8, device=DEV)
    sc, cs = guarded((8,), torch.float32, device=DEV)
    lib, s = L(), stream()
    wsb = 4 << 16

    def radii(X=None, N=40, D=16, ld=20, nh=(3,), n=None, o=None, w=None, wb=wsb):
        arr = (ctypes.c_int * max(len(nh), 1))(*nh)
        return lib.sfron_manifold_radii(x.data_ptr() if X is None else X, N, D, ld, arr, len(nh) if n is None else n, out.data_ptr() if o is None else o,
                                        ws.data_ptr() if w is None else w, wb, s)

    need = lib.sfron_manifold_radii_workspace(40, 0, 0)
    assert radii(wb=need) == 0
    torch.cuda.synchronize()
    out.view(torch.int32).fill_(co.sentinel)
    ws.view(torch.int32).fill_(cw.sentinel)
    bad = [radii(N=3), radii(N=7, nh=(7,)), radii(nh=(0,)), radii(nh=(8,)), radii(nh=(1, 2, 3, 4, 5)), radii(n=0), radii(D=18), radii(D=0), radii(ld=12),
           radii(ld=18), radii(X=x.data_ptr() + 4), radii(w=ws.data_ptr() + 4), radii(wb=need - 1), radii(X=0), radii(o=0), radii(w=0),
           radii(N=1 << 22, D=128, ld=128),                              # 2 GiB of rows
           lib.sfron_manifold_radii(x.data_ptr(), 40, 16, 20, None, 1, out.data_ptr(), ws.data_ptr(), wsb, s)]
    assert bad == [ERR_ARG] * len(bad), bad

    r = out                                                               # radii arguments of the pr call: any device floats

    def pr(X1=None, N1=40, X2=None, N2=40, K1=1, K2=1, D=16, ld1=20, ld2=20, R1=None, R2=None, I1=None, I2=None):
        return lib.sfron_manifold_pr(x.data_ptr() if X1 is None else X1, N1, r.data_ptr() if R1 is None else R1, K1, x.data_ptr() if X2 is None else X2,
                                     N2, r.data_ptr() if R2 is None else R2, K2, D, ld1, ld2, i1.data_ptr() if I1 is None else I1,
                                     i2.data_ptr() if I2 is None else I2, s)

    bad = [pr(N1=0), pr(N2=0), pr(K1=0), pr(K2=5), pr(D=18), pr(ld1=12), pr(ld2=18), pr(X1=x.data_ptr() + 8), pr(X2=x.data_ptr() + 4), pr(X1=0),
           pr(R1=0), pr(R2=r.data_ptr() + 2), pr(I1=0), pr(I2=0), pr(N1=1 << 22, D=128, ld1=128), pr(N2=1 << 22, D=128, ld2=128)]
    assert bad == [ERR_ARG] * len(bad), bad

    def gemm(A=None, M=40, lda=20, B=None, N=40, ldb=20, K=16, C=None, ldc=40):
        return lib.sfron_gemm_nt_f32(x.data_ptr() if A is None else A, M, lda, x.data_ptr() if B is None else B, N, ldb, K, ws.data_ptr() if C is None else C,
                                     ldc, s)

    bad = [gemm(M=0), gemm(N=0), gemm(K=0), gemm(K=18), gemm(lda=12), gemm(ldb=18), gemm(ldc=39), gemm(A=x.data_ptr() + 4), gemm(B=x.data_ptr() + 8),
           gemm(A=0), gemm(B=0), gemm(C=0), gemm(C=ws.data_ptr() + 2), gemm(M=1 << 22, K=128, lda=128), gemm(M=1 << 16, N=1 << 15, ldc=1 << 15)]
    assert bad == [ERR_ARG] * len(bad), bad

    zs, cz = guarded((8, 12), torch.float32, ld=16, device=DEV)
    need = lib.sfron_inception_score_workspace(8, 12, 3)

    def score(Z=None, N=8, C=12, ld=16, split=3, S=None, W=None, wb=wsb):
        return lib.sfron_inception_score(zs.data_ptr() if Z is None else Z, N, C, ld, split, sc.data_ptr() if S is None else S,
                                         ws.data_ptr() if W is None else W, wb, s)

    bad = [score(N=0), score(C=0), score(ld=8), score(split=0), score(Z=0), score(S=0), score(W=0), score(Z=zs.data_ptr() + 4), score(S=sc.data_ptr() + 4),
           score(W=ws.data_ptr() + 8), score(wb=need - 1), score(N=1 << 22, C=128, ld=128)]
    assert bad == [ERR_ARG] * len(bad), bad
    torch.cuda.synchronize()
    for chk, what in ((co, "radii"), (cw, "workspace"), (c1, "in1"), (c2, "in2"), (cs, "scores"), (cz, "logits")):
        untouched(chk, what)

    from sfron import evaluator
    est = evaluator.ManifoldEstimator()
    with pytest.raises(ValueError, match="out of bounds"):
        est.manifold_radii(torch.zeros(3, 16, device=DEV))
    with pytest.raises(ValueError, match="multiple of 4"):
        est.manifold_radii(torch.zeros(30, 18, device=DEV))


# ------------------------------------------------------------------------------------------------ drivers
@gpu
def test_evaluate_npz_equals_the_pieces_and_writes_the_row(net):
    import warnings
    from sfron import evaluator, fid
    root, ckpt, m, model, real, fake = net
    refp, samp, csvp = str(root / "run" / "ref" / "images.npz"), str(root / "fake.npz"), str(root / "out" / "result.csv")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = evaluator.evaluate_npz(refp, samp, model=model, csv_path=csvp)
        fr, fs = fid.InceptionFeatures(model, 2048).add_npz(refp), fid.InceptionFeatures(model, 2048).add_npz(samp)
        want = {"Inception Score": evaluator.compute_inception_score(model, fs.features()),
                "FID": fs.statistics().frechet_distance(fr.statistics())}
        want["Precision"], want["Recall"] = evaluator.compute_prec_recall(fr.features(), fs.features())
    assert list(got) == ["Inception Score", "FID", "Precision", "Recall"] and got == want
    assert all(isinstance(v, float) for v in got.values())
    r = ref.evaluate(fr.features().cpu().numpy(), fs.features().cpu().numpy(), (3,), np.float64)
    print(f"evaluate_npz: {got}; fp64 precision / recall of the same features {r['precision'][0]:.4f} / {r['recall'][0]:.4f}")
    with open(csvp) as f:
        rows = [line.rstrip("\n").split(",") for line in f]
    assert rows[0] == ["", "Inception Score", "FID", "Precision", "Recall"] and len(rows) == 2 and rows[1][0] == "run/ref"
    assert [float(v) for v in rows[1][1:]] == [got[k] for k in rows[0][1:]]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        again = evaluator.evaluate_npz(samp, refp, model=model, csv_path=csvp, name="run/ref")       # the sets swapped: the row is updated in place
    assert again != got
    with open(csvp) as f:
        rows = [line.rstrip("\n").split(",") for line in f]
    assert [r[0] for r in rows] == ["", "run/ref"]
    assert [float(v) for v in rows[1][1:]] == [again[k] for k in rows[0][1:]]
    st = str(root / "stats.npz")
    fr.statistics().save(st)
    with pytest.raises(ValueError, match="mu / sigma"):
        evaluator.evaluate_npz(st, samp, model=model)
    with pytest.raises(ValueError, match="checkpoint"):
        evaluator.evaluate_npz(refp, samp)


def teardown_module(module):
    for name in sorted(RECORD):
        if any(name.startswith(p) for p in ("gemm_nt", "f64", "f2048", "is37", "is1203", "IS end", "zero prob")):
            print(f"  {name}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(RECORD[name].items())))
