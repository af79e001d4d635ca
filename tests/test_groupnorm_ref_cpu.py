"""CPU: the reference of tests/test_gpu_groupnorm.py is independent of the kernels, its bounds are reachable, and its checks can fail.

  * the float64 restatements of tests/groupnorm_ref.py against F.group_norm plus autograd in float64, to 1e-12, for every option (swish, mask,
    accumulate, extra, groups 1 / 3 / 32 / 64, a pixel count that is no power of two), and the order (dx_prev + extra) + gradient in float32;
  * the case table: the restated dispatch rule sends every case to the family and sub-form its row names, also with the padded strides the
    GPU module adds, and k_gn2_stats' LDS request at C = 4096 is exactly 64 KB;
  * the restated rule against the library's own host functions over a grid (they need no GPU);
  * at every case the float32 restatement alone stays at or below 5e-4 mismatches against bf16(ref64), a quarter of bound_bf16's cap, for y
    and for the bf16 form of dx, and passes bound32 with the serial sums;
  * the integer variant: every part_beta is an integer below 2^24, so any float32 summation order gives it exactly;
  * broken references are rejected: one pixel row dropped from part_beta (exact-integer check and bound32) and from dx (bound32), and a y
    with one chunk's rows normalised by another group's statistics (bound_bf16)."""
import pytest
import torch
import torch.nn.functional as F

import groupnorm_ref as G

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
TIGHT = 1e-12
QUARTER_CAP = 5e-4
BY_NAME = {c.name: c for c in G.CASES}


def near(a, b, what):
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert err <= TIGHT * max(1.0, float(b.abs().max())), (what, err)


# ------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("B,HW,C,groups", [(2, 9, 64, 32), (3, 25, 30, 3), (2, 7, 16, 1), (2, 12, 128, 64), (2, 100, 96, 32)])
@pytest.mark.parametrize("swish", [0, 1])
@pytest.mark.parametrize("masked", [0, 1])
def test_restatement_equals_group_norm_autograd(B, HW, C, groups, swish, masked):
    i = G.gn_inputs(G._c(B, HW, C, groups, "cpu"))
    mask, scale = (i["mask"], i["scale"]) if masked else (None, 1.0)
    eps = G.f32(G.EPS)
    x = i["x"].double().requires_grad_(True)
    gm, bt = i["gamma"].double().requires_grad_(True), i["beta"].double().requires_grad_(True)
    z = F.group_norm(x.permute(0, 2, 1), groups, gm, bt, eps=eps).permute(0, 2, 1)
    if swish:
        z = z * torch.sigmoid(z)
    if masked:
        z = z * mask.double() * G.f32(scale)
    z.backward(i["dy"].double())
    y, mean, rstd = G.groupnorm_fwd(i["x"], i["gamma"], i["beta"], groups, G.EPS, swish, mask, scale, F64)
    near(y, z.detach(), "y")
    xg = i["x"].double().view(B, HW, groups, C // groups)
    near(mean, xg.mean((1, 3)), "mean")
    near(rstd, 1.0 / torch.sqrt(xg.permute(0, 2, 1, 3).reshape(B, groups, -1).var(2, unbiased=False) + eps), "rstd")
    r = G.groupnorm_bwd(i["dy"], i["x"], i["gamma"], i["beta"], groups, G.EPS, swish, mask, scale, None, 0, None, F64)
    near(r.dx, x.grad, "dx")
    assert r.pg.shape == r.pb.shape == r.colsum.shape == (B, C)
    near(r.pg.sum(0), gm.grad, "d gamma")
    near(r.pb.sum(0), bt.grad, "d beta")
    near(r.colsum, x.grad.sum(1), "column sums")
    assert torch.equal(r.dx16, x.grad.float().to(BF16))
    for acc, extra in ((1, None), (0, i["extra"]), (1, i["extra"])):
        want = x.grad + (i["dx0"].double() if acc else 0.0) + (extra.double() if extra is not None else 0.0)
        got = G.groupnorm_bwd(i["dy"], i["x"], i["gamma"], i["beta"], groups, G.EPS, swish, mask, scale, i["dx0"], acc, extra, F64)
        near(got.dx, want, f"dx acc={acc}")
        near(got.colsum, want.sum(1), f"column sums acc={acc}")
        near(got.pg, r.pg, "part_gamma does not depend on dx")
    # float32: (dx_prev + extra) + gradient, in that order; the sums over the pixels serial
    r32 = G.groupnorm_bwd(i["dy"], i["x"], i["gamma"], i["beta"], groups, G.EPS, swish, mask, scale, None, 0, None, F32)
    both = G.groupnorm_bwd(i["dy"], i["x"], i["gamma"], i["beta"], groups, G.EPS, swish, mask, scale, i["dx0"], 1, i["extra"], F32)
    assert torch.equal(both.dx, (i["dx0"] + i["extra"]) + r32.dx)
    serial = torch.zeros(B, C)
    for p in range(HW):
        serial = serial + r32.dx[:, p]
    assert torch.equal(r32.colsum, serial)


def test_pixel_sum_float32_is_serial():
    v = torch.tensor([2.0 ** 24, 1.0, 1.0, 1.0, 1.0]).view(1, 5, 1)
    assert float(G.pixel_sum(v, F32)) == 2.0 ** 24                    # every 1 is lost one at a time; a pairwise sum keeps some
    assert float(G.pixel_sum(v.double(), F64)) == 2.0 ** 24 + 4


def test_constant_group_has_zero_variance():
    c = BY_NAME["gn2-3x100x320g32"]
    i = G.gn_inputs(c, "const")
    b, g = i["const"]
    cg = c.C // c.groups
    for dt in (F64, F32):
        y, mean, rstd = G.groupnorm_fwd(i["x"], i["gamma"], i["beta"], c.groups, G.EPS, 1, None, 1.0, dt)
        assert float(mean[b, g]) == 0.75 and abs(float(rstd[b, g]) - 1000.0) <= 1e-4 * 1000.0
        be = i["beta"][g * cg:(g + 1) * cg].to(dt)
        assert torch.equal(y[b, :, g * cg:(g + 1) * cg], (be / (1.0 + torch.exp(-be))).expand(c.HW, cg))


# ------------------------------------------------------------------------------------------------ the dispatch rule
def test_case_table_classes():
    for c in G.CASES:
        assert G.classify(c) == c.cls, (c.name, G.classify(c))
        assert G.classify(c, ldx_more=8, lddx_more=12) == c.cls, (c.name, "with the padded strides of the GPU module")
        assert c.C % c.groups == 0 and c.C // c.groups <= G.TPB
    assert len({c.name for c in G.CASES}) == len(G.CASES)
    for cls in ("gn3.8", "gn3.4", "gn3.2", "gn3.1", "gn3.8w"):
        assert sum(c.cls == cls for c in G.SRC_CASES) == 1
    # the facts the comments of the table state
    assert G.gn3_gpb(64, 1024, 128, 32) == (8, "128K") and 1024 * 32 * 4 == 128 << 10 and G.gn3_gpb(64, 1025, 128, 32) == (4, "128K")
    assert G.gn3_gpb(48, 729, 384, 32) == (8, "512K") and G.gn3_gpb(48, 441, 640, 32) == (8, "512K")
    assert G.gn3_gpb(64, 1024, 320, 32) == (0, None) and G.gn3_gpb(64, 1024, 256, 32) == (4, "128K")
    assert G.gn3_gpb(48, 9, 64, 32)[0] == 8 and G.gn3_gpb(47, 9, 64, 32)[0] == 0
    chunks = {(47, 9): 1, (3, 9): 1, (3, 100): 12, (3, 1000): 32, (3, 72): 9, (2, 25): 3, (3, 25): 3, (24, 529): 22, (48, 729): 11}
    for (B, HW), n in chunks.items():
        assert G.gn_chunks(B, HW) == n, (B, HW, G.gn_chunks(B, HW))
    assert 100 % 12 and 1000 % 32 and 12 % 8 == 4
    assert G.gn2_stats_lds(4096) == 64 << 10 and G.gn2_stats_lds(4) == 64 << 10
    assert G.bwd_cast_ok(2048, 2048, 32) and not G.bwd_cast_ok(4096, 4096, 32)


def test_restated_rule_is_the_library_s():
    import __graft_entry__ as ge
    ge.build()
    from sfron import _lib
    L = _lib.lib()
    for B in (1, 2, 3, 6, 12, 23, 24, 47, 48, 64, 192):
        for HW in (1, 7, 8, 9, 64, 100, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097):
            assert L.sfron_groupnorm_chunks(B, HW) == G.gn_chunks(B, HW), (B, HW)
            for cg in (1, 2, 3, 4, 8, 10, 12, 16, 32, 40, 80, 128):
                for groups in (1, 4, 12, 32, 64):
                    C = cg * groups
                    assert L.sfron_groupnorm_one_launch(B, HW, C, groups) == G.one_launch(B, HW, C, groups), (B, HW, C, groups)
                    assert L.sfron_groupnorm_scratch_bytes(B, HW, C, groups) == G.scratch_bytes(B, HW, C, groups), (B, HW, C, groups)
    for c in G.CASES:
        assert L.sfron_groupnorm_one_launch(c.B, c.HW, c.C, c.groups) == G.one_launch(c.B, c.HW, c.C, c.groups), c.name
        assert L.sfron_groupnorm_chunks(c.B, c.HW) == G.gn_chunks(c.B, c.HW)
        assert L.sfron_groupnorm_scratch_bytes(c.B, c.HW, c.C, c.groups) == G.scratch_bytes(c.B, c.HW, c.C, c.groups)
    for C in (4, 30, 64, 96, 2048, 2052, 4096, 4128, 0):
        for groups in (1, 3, 32, 64, 128, 0):
            for ldx in (C, C + 2, C + 8):
                assert L.sfron_groupnorm_bwd_cast_ok(ldx, C, groups) == G.bwd_cast_ok(ldx, C, groups), (ldx, C, groups)
    assert L.sfron_groupnorm_chunks(0, 9) == 0 and L.sfron_groupnorm_scratch_bytes(0, 9, 64, 32) == 0 == G.scratch_bytes(0, 9, 64, 32)
    assert L.sfron_groupnorm_one_launch(2, 9, 128, 128) == 0 == G.one_launch(2, 9, 128, 128)


# ------------------------------------------------------------------------------------------------ the bounds are reachable
def _share(y32, y64):
    return float((y32.to(BF16) != G.to_bf16(y64)).double().mean())


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c.name)
def test_float32_restatement_meets_a_quarter_of_the_cap(c):
    i = G.gn_inputs(c)
    big = c.B * c.HW * c.C > 4 << 20
    for swish, masked in ((1, 1),) if big else ((0, 0), (0, 1), (1, 0), (1, 1)):
        mask, scale = (i["mask"], i["scale"]) if masked else (None, 1.0)
        y64, m64, r64 = G.groupnorm_fwd(i["x"], i["gamma"], i["beta"], c.groups, G.EPS, swish, mask, scale, F64)
        y32, m32, r32 = G.groupnorm_fwd(i["x"], i["gamma"], i["beta"], c.groups, G.EPS, swish, mask, scale, F32)
        share = _share(y32, y64)
        assert share <= QUARTER_CAP, (c.name, swish, masked, share)
        G.bound_bf16(y32.to(BF16), y64, y32)
        G.stat_close(m32, m64, 1e-6, 1e-6, "mean")
        G.stat_close(r32, r64, 1e-4, 0.0, "rstd")
    if big and c.cls != "gn3.8w" and c.name != "gn2-64x1024x320g32":
        return
    mask, scale = i["mask"], i["scale"]
    w64 = G.groupnorm_bwd(i["dy"], i["x"], i["gamma"], i["beta"], c.groups, G.EPS, 1, mask, scale, i["dx0"], 1, i["extra"], F64)
    w32 = G.groupnorm_bwd(i["dy"], i["x"], i["gamma"], i["beta"], c.groups, G.EPS, 1, mask, scale, i["dx0"], 1, i["extra"], F32)
    share = float((w32.dx16 != w64.dx16).double().mean())
    assert share <= QUARTER_CAP, (c.name, "dx16", share)
    for name in ("dx", "pg", "pb", "colsum"):
        G.bound32(getattr(w32, name), getattr(w64, name), getattr(w32, name))


@pytest.mark.parametrize("c", G.CONST_CASES, ids=lambda c: c.name)
def test_float32_restatement_meets_a_quarter_of_the_cap_constant_group(c):
    i = G.gn_inputs(c, "const")
    for swish, masked in ((0, 0), (0, 1), (1, 0), (1, 1)):
        mask, scale = (i["mask"], i["scale"]) if masked else (None, 1.0)
        y64, m64, r64 = G.groupnorm_fwd(i["x"], i["gamma"], i["beta"], c.groups, G.EPS, swish, mask, scale, F64)
        y32, m32, r32 = G.groupnorm_fwd(i["x"], i["gamma"], i["beta"], c.groups, G.EPS, swish, mask, scale, F32)
        assert _share(y32, y64) <= QUARTER_CAP, (c.name, swish, masked, _share(y32, y64))
        G.bound_bf16(y32.to(BF16), y64, y32)


@pytest.mark.parametrize("name", ["gn3.8-48x9x64g32", "gn3.4-24x529x256g32", "gn2-3x100x320g32", "gn2-3x1000x128g32", "gn1-2x25x96g32-noscratch"])
def test_integer_variant_part_beta_is_exact(name):
    c = BY_NAME[name]
    i = G.gn_inputs(c, "int")
    w64 = G.groupnorm_bwd(i["dy"], i["x"], i["gamma"], i["beta"], c.groups, G.EPS, 0, i["mask"], i["scale"], None, 0, None, F64)
    w32 = G.groupnorm_bwd(i["dy"], i["x"], i["gamma"], i["beta"], c.groups, G.EPS, 0, i["mask"], i["scale"], None, 0, None, F32)
    assert torch.equal(w64.pb, w64.pb.round()) and float(w64.pb.abs().max()) < 2 ** 24 and float(w64.pb.abs().max()) >= 6
    assert float((i["dy"].abs() * i["scale"]).sum(1).max()) < 2 ** 24              # every partial sum of any order, too
    assert torch.equal(w32.pb.double(), w64.pb)


# ------------------------------------------------------------------------------------------------ the checks can fail
def test_broken_references_are_rejected():
    c = BY_NAME["gn2-3x100x320g32"]
    B, HW, C, groups = c.B, c.HW, c.C, c.groups
    cg = C // groups
    # (a) part_beta with one pixel row dropped: the exact-integer comparison, and bound32 on the randn inputs
    i = G.gn_inputs(c, "int")
    w64 = G.groupnorm_bwd(i["dy"], i["x"], i["gamma"], i["beta"], groups, G.EPS, 0, i["mask"], i["scale"], None, 0, None, F64)
    d = torch.where(i["mask"].bool(), i["dy"].double() * 2.0, torch.zeros((), dtype=F64))
    short = w64.pb - d[:, 37]
    assert torch.equal(d.sum(1), w64.pb) and not torch.equal(short.float(), w64.pb.float())
    assert int((short != w64.pb).sum()) > C                           # most channels of every sample notice one row
    i = G.gn_inputs(c)
    args = (i["dy"], i["x"], i["gamma"], i["beta"], groups, G.EPS, 1, i["mask"], i["scale"], None, 0, None)
    w64, w32 = G.groupnorm_bwd(*args, F64), G.groupnorm_bwd(*args, F32)
    G.bound32(w32.pb, w64.pb, w32.pb)
    mean, rstd, xhat = G._stats(i["x"], groups, G.EPS, F32)
    dz = torch.where(i["mask"].bool(), i["dy"] * i["scale"], torch.zeros(())) * G._act_grad(xhat * i["gamma"] + i["beta"])
    with pytest.raises(AssertionError, match="max.got - ref64"):
        G.bound32(w32.pb - dz[:, 37], w64.pb, w32.pb, "pb one row short")
    with pytest.raises(AssertionError, match="max.got - ref64"):
        G.bound32(w32.pg - (dz * xhat)[:, 37], w64.pg, w32.pg, "pg one row short")
    # (b) dx with one pixel row left out of the group sums (k1, k2 formed over HW - 1 rows), and with one row not written
    keep = torch.ones(HW, dtype=torch.bool)
    keep[37] = False
    less = G.groupnorm_bwd(i["dy"] * keep[None, :, None], i["x"], i["gamma"], i["beta"], groups, G.EPS, 1, i["mask"], i["scale"], None, 0, None, F32)
    wrong = less.dx.clone()
    wrong[:, 37] = w32.dx[:, 37]                                      # the row itself as it should be: only the sums miss it
    G.bound32(w32.dx, w64.dx, w32.dx)
    with pytest.raises(AssertionError, match="max.got - ref64"):
        G.bound32(wrong, w64.dx, w32.dx, "dx, sums one row short")
    unwritten = w32.dx.clone()
    unwritten[1, 99] = 0.0
    with pytest.raises(AssertionError, match="max.got - ref64"):
        G.bound32(unwritten, w64.dx, w32.dx, "dx, last row not written")
    # (c) y with the rows of one chunk normalised by the next group's statistics
    y64, m64, r64 = G.groupnorm_fwd(i["x"], i["gamma"], i["beta"], groups, G.EPS, 1, None, 1.0, F64)
    y32, m32, r32 = G.groupnorm_fwd(i["x"], i["gamma"], i["beta"], groups, G.EPS, 1, None, 1.0, F32)
    G.bound_bf16(y32.to(BF16), y64, y32)
    n = G.gn_chunks(B, HW)
    p0, p1 = HW * 5 // n, HW * 6 // n
    ms, rs = torch.roll(m32, 1, 1), torch.roll(r32, 1, 1)
    xh = (i["x"][:, p0:p1] - G._per_channel(ms, cg)) * G._per_channel(rs, cg)
    z = xh * i["gamma"] + i["beta"]
    bad = y32.clone()
    bad[:, p0:p1] = z / (1.0 + torch.exp(-z))
    with pytest.raises(AssertionError, match="elements past"):
        G.bound_bf16(bad.to(BF16), y64, y32, "y, chunk 5 with the neighbouring group's statistics")
    # the statistics tolerances notice a group swap too
    with pytest.raises(AssertionError):
        G.stat_close(ms, m64, 1e-6, 1e-6, "mean")
