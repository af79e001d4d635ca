"""CPU: ADM's centre crop (latents.center_crop_arr: BOX halvings, BICUBIC, crop) as a planned chain of table pairs with the crop folded
back through it (resample.center_crop_plan), the batch layout the device entry point takes (resample.plan_batch) and the host checks of
its wrapper.  Pillow is the yardstick and every comparison is bitwise: the plan is run through ``apply_spec``, the two integer passes
exactly as the kernels are specified."""
import numpy as np
import pytest
from PIL import Image

from test_sd_front_end_cpu import apply_spec, case_image

S = 32
# (H, W) at image_size 32: 0-3 halvings, the exact 2x boundary and one pixel below it, odd sides (a BOX scale slightly above 2), identity
# BICUBIC (s = 1), up-scaling, 8:1 and 16:1 aspect ratios in both orientations
SHAPES = [(64, 64), (63, 64), (64, 63), (65, 97), (127, 200), (128, 128), (129, 131), (255, 300), (256, 257), (257, 513), (300, 90), (90, 300),
          (31, 40), (20, 33), (32, 32), (32, 50), (511, 64), (64, 1030), (200, 67)]


def source(ci):
    H, W = SHAPES[ci]
    return case_image(ci, H, W)


def pillow_crop(a, size=S):
    from sfron import latents
    return np.asarray(latents.center_crop_arr(Image.fromarray(a), size))


def run_plan(a, plan):
    """The stages through apply_spec, each over the window of the previous image that is held (bounds rebased by its origin)."""
    cur = a
    for st in plan.stages:
        assert cur.shape[:2] == (st.in_h, st.in_w)
        bx, by = st.tx.bounds.copy(), st.ty.bounds.copy()
        bx[:, 0] -= st.ox
        by[:, 0] -= st.oy
        cur = apply_spec(cur, st.tx.coeffs, bx, st.ty.coeffs, by)
    return cur


@pytest.mark.parametrize("ci", range(len(SHAPES)))
def test_plan_through_the_spec_equals_center_crop_arr(ci):
    from sfron import resample
    a = source(ci)
    H, W = SHAPES[ci]
    got = run_plan(a, resample.center_crop_plan(W, H, S))
    want = pillow_crop(a)
    assert got.shape == (S, S, 3) and np.array_equal(got, want), int(np.abs(got.astype(int) - want).max())
    if ci % 2 and min(H, W) < 2 * S:
        assert got.min() == 0 and got.max() == 255          # both ends of the clamp (BICUBIC overshoot on saturated bytes)


def test_halvings_and_stage_sizes_worked_values():
    """(w, h) of every stage by the reference text: d // 2 while min >= 64, then round(d * 32 / min)."""
    from sfron import resample
    worked = {(64, 64): [(64, 64), (32, 32), (32, 32)],                         # exactly 2x: one halving, then identity
              (63, 64): [(64, 63), (33, 32)],                                   # one below: none; round(64 * 32 / 63 = 32.51) = 33
              (127, 200): [(200, 127), (100, 63), (51, 32)],                    # round(100 * 32 / 63 = 50.79) = 51
              (129, 131): [(131, 129), (65, 64), (32, 32), (32, 32)],           # 64 >= 64 halves again
              (255, 300): [(300, 255), (150, 127), (75, 63), (38, 32)],         # round(75 * 32 / 63 = 38.10) = 38
              (257, 513): [(513, 257), (256, 128), (128, 64), (64, 32), (64, 32)],
              (20, 33): [(33, 20), (53, 32)],                                   # up-scaling: round(33 * 1.6 = 52.8) = 53
              (32, 50): [(50, 32), (50, 32)],
              (511, 64): [(64, 511), (32, 255), (32, 255)],
              (64, 1030): [(1030, 64), (515, 32), (515, 32)],
              (200, 67): [(67, 200), (33, 100), (32, 97)]}                      # round(100 * 32 / 33 = 96.97) = 97
    for (H, W), sizes in worked.items():
        plan = resample.center_crop_plan(W, H, S)
        assert list(plan.sizes) == sizes, (H, W)
        assert plan.halvings == len(sizes) - 2 and len(plan.stages) == len(sizes) - 1
        assert plan.crop == ((sizes[-1][0] - S) // 2, (sizes[-1][1] - S) // 2)
    assert [resample.center_crop_plan(W, H, S).halvings for H, W in SHAPES] == [1, 0, 0, 1, 1, 2, 2, 2, 3, 3, 1, 1, 0, 0, 0, 0, 1, 1, 1]
    assert resample.center_crop_plan(97, 65, S) is resample.center_crop_plan(97, 65, S)          # cached


@pytest.mark.parametrize("ci", range(len(SHAPES)))
def test_every_stage_forms_exactly_what_the_next_reads(ci):
    from sfron import resample
    H, W = SHAPES[ci]
    plan = resample.center_crop_plan(W, H, S)
    st = plan.stages
    assert (st[0].ox, st[0].oy, st[0].in_w, st[0].in_h) == (0, 0, W, H)
    for s in range(len(st) - 1):
        (x0, x1), (y0, y1) = st[s + 1].tx.rows(), st[s + 1].ty.rows()
        full_w, full_h = plan.sizes[s + 1]
        # the window of stage s is the slice [x0, x1) x [y0, y1) of its full tables, and the next stage knows it as its origin / extents
        want_x, want_y = resample.resample_tables(plan.sizes[s][0], full_w, "box"), resample.resample_tables(plan.sizes[s][1], full_h, "box")
        assert np.array_equal(st[s].tx.bounds, want_x.bounds[x0:x1]) and np.array_equal(st[s].tx.coeffs, want_x.coeffs[x0:x1])
        assert np.array_equal(st[s].ty.bounds, want_y.bounds[y0:y1]) and np.array_equal(st[s].ty.coeffs, want_y.coeffs[y0:y1])
        assert (st[s + 1].ox, st[s + 1].oy, st[s + 1].in_w, st[s + 1].in_h) == (x0, y0, x1 - x0, y1 - y0)
    left, top = plan.crop
    last_w, last_h = plan.sizes[-1]
    want_x = resample.resample_tables(plan.sizes[-2][0], last_w, "bicubic")
    assert st[-1].tx.bounds.shape[0] == st[-1].ty.bounds.shape[0] == S
    assert np.array_equal(st[-1].tx.bounds, want_x.bounds[left:left + S]) and np.array_equal(st[-1].tx.coeffs, want_x.coeffs[left:left + S])


def test_batch_layout_levels_and_launch_count():
    from sfron import _lib, resample
    plans = [resample.center_crop_plan(W, H, S) for H, W in SHAPES]
    for p in plans:
        bp = resample.plan_batch([p.stages])
        assert bp.n_levels == 2 * (1 + p.halvings) and bp.passes.shape == (bp.n_levels, resample.PASS_WORDS)
        assert bp.validate()
    bp = resample.plan_batch([p.stages for p in plans])
    assert bp.n_levels == 8 and bp.validate()                                   # the batch holds three halvings
    assert bp.passes.shape[0] == sum(2 * len(p.stages) for p in plans)
    counts = [sum(1 for p in plans if len(p.stages) > s) for s in range(4)]      # images that have a stage s
    assert np.array_equal(np.diff(bp.level_first), np.repeat(counts, 2))
    assert bp.out_bytes == len(SHAPES) * S * S * 3
    # the last vertical pass of every image, and no other pass, writes out, at the image's slot
    P = bp.passes
    to_out = P[P[:, resample.P_OUT_BUF] == _lib.RESAMPLE_OUT]
    assert sorted(to_out[:, resample.P_OUT_OFF].tolist()) == [i * S * S * 3 for i in range(len(SHAPES))]
    none = [i for i, p in enumerate(plans) if p.halvings == 0]
    assert resample.plan_batch([plans[i].stages for i in none]).n_levels == 2
    # the gather: records, tables and pixels in one buffer, each where the plan says
    host = np.zeros(bp.host_bytes, dtype=np.uint8)
    bp.fill(host, [source(ci) for ci in range(len(SHAPES))])
    assert np.array_equal(host[:P.size * 8].view(np.int64).reshape(P.shape), P)
    assert np.array_equal(host[bp.tables_at:bp.tables_at + bp.tables.size * 4].view(np.int32), bp.tables)
    for ci, off in enumerate(bp.src_off):
        a = source(ci)
        assert np.array_equal(host[bp.pool_at + off:bp.pool_at + off + a.size], a.reshape(-1))


def _broken(bp, **edits):
    """A copy of the plan with fields of one record replaced: edits = {field index: value}, on pass ``at``."""
    import copy
    at = edits.pop("at")
    out = copy.copy(bp)
    out.passes = bp.passes.copy()
    for k, v in edits.items():
        out.passes[at, int(k[1:])] = v
    return out


def test_wrapper_refuses_broken_records_before_the_library(monkeypatch):
    """The checks that need the records' contents sit in the wrapper and answer before the library is reached (no GPU here)."""
    import copy
    from sfron import _lib, resample

    def no_library():
        raise AssertionError("the wrapper reached the library")

    monkeypatch.setattr(_lib, "lib", no_library)
    R = resample
    plans = [R.center_crop_plan(W, H, S) for H, W in ((65, 97), (63, 64), (129, 131))]
    bp = R.plan_batch([p.stages for p in plans])
    assert bp.validate()
    P = bp.passes
    h0 = 0                                                   # a horizontal pass of level 0
    v0 = int(bp.level_first[1])                              # a vertical pass of level 1
    v_last = int(np.flatnonzero(P[:, R.P_OUT_BUF] == _lib.RESAMPLE_OUT)[0])
    f = lambda name: "f%d" % getattr(R, name)
    cases = {
        # (129, 131): 131 -> 65 columns at scale 2.015 reads column 130; (63, 64): the BICUBIC window starts at column 0
        "columns reach past the input": _broken(bp, at=h0 + 2, **{f("P_IN_W"): P[h0 + 2, R.P_IN_W] - 1}),
        "columns start before the origin": _broken(bp, at=h0 + 1, **{f("P_ORG"): 1}),
        "rows reach past the input": _broken(bp, at=v0, **{f("P_IN_H"): P[v0, R.P_IN_H] - 1}),
        "row window past the input": _broken(bp, at=h0, **{f("P_ROW0"): P[h0, R.P_ROW0] + 1}),
        "more taps than ksize": _broken(bp, at=h0, **{f("P_KSIZE"): 1}),
        "input past the pool": _broken(bp, at=h0, **{f("P_IN_OFF"): bp.pool_bytes}),
        "negative input offset": _broken(bp, at=h0, **{f("P_IN_OFF"): -1}),
        "output past the work buffer": _broken(bp, at=h0, **{f("P_OUT_OFF"): bp.work_bytes - 1}),
        "output past out": _broken(bp, at=v_last, **{f("P_OUT_OFF"): bp.out_bytes - S * S * 3 + 1}),
        "coefficients past the blob": _broken(bp, at=h0, **{f("P_K_OFF"): bp.tables.size - 1}),
        "bounds past the blob": _broken(bp, at=v0, **{f("P_B_OFF"): bp.tables.size - 1}),
        "zero outputs": _broken(bp, at=v0, **{f("P_N_OUT"): 0}),
        "a horizontal pass that writes out": _broken(bp, at=h0, **{f("P_OUT_BUF"): _lib.RESAMPLE_OUT}),
        "a vertical pass that reads the pool": _broken(bp, at=v0, **{f("P_IN_BUF"): _lib.RESAMPLE_POOL}),
        "a pass writes what a pass of its level reads": _broken(bp, at=v0, **{f("P_OUT_BUF"): _lib.RESAMPLE_WORK, f("P_OUT_OFF"): P[v0 + 1, R.P_IN_OFF]}),
        "two passes of a level write the same bytes": _broken(bp, at=h0, **{f("P_OUT_OFF"): P[h0 + 1, R.P_OUT_OFF]}),
    }
    # descending row bounds: the vertical tables of one pass reversed in the blob
    rev = copy.copy(bp)
    rev.tables = bp.tables.copy()
    b_off, n = int(P[v0, R.P_B_OFF]), int(P[v0, R.P_N_OUT])
    rev.tables[b_off:b_off + 2 * n] = bp.tables[b_off:b_off + 2 * n].reshape(n, 2)[::-1].reshape(-1)
    cases["descending row bounds"] = rev
    lv = copy.copy(bp)
    lv.level_first = bp.level_first.copy()
    lv.level_first[1] = lv.level_first[2]
    cases["a level list that does not ascend"] = lv
    for name, bad in cases.items():
        assert not bad.validate(), name
        assert R.image_resample_batch_u8(bad, None, None, None, bp.pool_bytes, bp.work_bytes, bp.out_bytes) == _lib.ERR_ARG, name
    for name, sizes in (("pool", (bp.pool_bytes - 1, bp.work_bytes, bp.out_bytes)), ("work", (bp.pool_bytes, bp.work_bytes - 16, bp.out_bytes)),
                        ("out", (bp.pool_bytes, bp.work_bytes, bp.out_bytes - 1))):
        assert not bp.validate(*sizes), name
        assert R.image_resample_batch_u8(bp, None, None, None, *sizes) == _lib.ERR_ARG, name


def test_header_and_bindings_declare_the_batch_entry():
    import os
    import re
    from sfron import _lib, resample
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "sfron.h")).read(), flags=re.S)
    m = re.search(r"\bint sfron_image_resample_batch_u8\((.*?)\)\s*;", hdr, flags=re.S)
    assert m
    params = [p.strip() for p in m.group(1).split(",")]
    res, args = _lib._PROTOS["sfron_image_resample_batch_u8"]
    assert len(params) == len(args) == 15
    for p, a in zip(params, args):
        assert ("*" in p) == (a is _lib._P), p
    body = re.search(r"typedef struct sfron_resample_pass \{(.*?)\} sfron_resample_pass;", hdr, flags=re.S).group(1)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.replace("int64_t", "").split(",")]
    assert names[:13] == ["in_buf", "in_off", "in_w", "in_h", "out_buf", "out_off", "n_out", "org", "row0", "nrows", "k_off", "b_off", "ksize"]
    assert names[13] == "reserved[3]" and resample.PASS_WORDS == 16
    assert [resample.P_IN_BUF, resample.P_ORG, resample.P_KSIZE] == [0, 7, 12]
