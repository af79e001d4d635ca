"""CPU: the fp8 backward of config 5 (include/sfron.h, csrc/fp8.hip) without a GPU -- its entry points are declared and exported, the MX
rule the GPU tests restate agrees with hand-computed cases, and its kernels compile for gfx950 without spills or scratch."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sfron_cast_mx8", "sfron_fp8_transpose_shadow", "sfron_fp8_dgrad", "sfron_dit_fp8_dgrad_workspace_bytes", "sfron_aux_set_fp8_dgrad"]


def mx_ref(x):
    """the rule of include/sfron.h: X = ceil(log2(amax / 448)) per 32-block of a row, clamped to [-127, 127], all-zero -> -127;
    byte = X + 127; code = e4m3fn_RNE(x * 2^-X).  (codes, scale bytes)"""
    M, N = x.shape
    xb = x.float().reshape(M, N // 32, 32)
    amax = xb.abs().amax(dim=2).double()
    X = torch.where(amax > 0, torch.ceil(torch.log2(amax / 448.0)), torch.full_like(amax, -127.0)).clamp(-127, 127)
    q = (xb * torch.pow(2.0, -X).float()[..., None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).reshape(M, N), (X + 127).to(torch.uint8)


def test_new_symbols_declared_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from sfron import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfron.h")).read(), flags=re.S)
    h = _lib.lib()
    for s in NEW:
        assert re.search(rf"\b{s}\s*\(", txt), s
        assert s in _lib.declared_symbols() and hasattr(h, s), s
    assert "sfron_fp8_dgrad_desc" in txt


def test_dgrad_desc_mirror_matches_the_header(tmp_path):
    import ctypes
    from sfron import _lib
    fs = ["A", "a_scales", "B", "M", "w_scale", "epilogue", "c_bf16", "aux", "c_e4m3", "c_scales", "col_partials", "tile_hint"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "sfron.h"\nint main(void) {\nprintf("%zu", sizeof(sfron_fp8_dgrad_desc));\n'
    src += "".join(f'printf(" %zu", offsetof(sfron_fp8_dgrad_desc, {f}));\n' for f in fs) + "return 0; }\n"
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    size, *offs = subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()
    assert ctypes.sizeof(_lib.Fp8DgradDesc) == int(size)
    for f, o in zip(fs, offs):
        assert getattr(_lib.Fp8DgradDesc, f).offset == int(o), f


def test_mx_rule_hand_cases():
    x = torch.zeros(1, 32 * 6)
    x[0, 0] = 448.0           # amax 448 -> X = 0, code 0x7E (448)
    x[0, 32] = 452.0          # X = 1: 226 -> 224 (nearest even) = 0x76
    x[0, 64] = 1.0            # ceil(log2(1 / 448)) = ceil(-8.81) = -8: 256 = 0x78
    x[0, 96 + 5] = -3.0e38    # ceil(log2(3e38 / 448)) = ceil(119.01) = 120: bf16 -2.998e38 * 2^-120 = -226 -> -224 = 0xF6
    x[0, 128] = 1e-39         # a subnormal alone (bf16 11 * 2^-133): X clamps to -127, 11 * 2^-6 = 0.171875 = 0x23
    q, s = mx_ref(x.to(torch.bfloat16))
    assert s.tolist() == [[127, 128, 119, 127 + 120, 0, 0]]
    assert [q[0, j].item() for j in (0, 32, 64, 96 + 5, 128)] == [0x7E, 0x76, 0x78, 0xF6, 0x23]
    assert int(q[0, 1]) == 0 and int(q[0, 191]) == 0
    # nothing saturates: every |code| <= 448 and the largest magnitude of a block lands in (224, 448]
    g = torch.Generator().manual_seed(0)
    y = (torch.randn(64, 1152, generator=g) * torch.exp(torch.randn(64, 1, generator=g) * 4)).to(torch.bfloat16)
    q, s = mx_ref(y)
    v = q.view(torch.float8_e4m3fn).float().abs().reshape(64, 36, 32).amax(dim=2)
    assert (v <= 448).all() and (v > 224 * 0.93).all()


def test_fp8_kernels_compile_without_spills_or_scratch():
    src = os.path.join(ROOT, "unified-unlearning-w-remain-geometry_amd", "csrc", "fp8.hip")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), src, ""], capture_output=True, text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"(.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+spill\s+(\d+)\s+occ\s+(\d+)\s+scratch\s+(\d+)", line)
        if m:
            rows[m.group(1).strip()] = (int(m.group(4)), int(m.group(6)))
    new = [k for k in rows if re.search(r"k_gemm8<[45], [89], 0>", k) or "k_cast_mx8" in k or "k_fp8_transpose_shadow" in k]
    assert len(new) == 5, rows.keys()
    for k in new:
        assert rows[k] == (0, 0), (k, rows[k])
