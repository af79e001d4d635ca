"""CPU: the fp8 weight gradients (include/sfron.h sfron_cast_mx8_t / sfron_fp8_wgrad / sfron_aux_set_fp8_wgrad, csrc/fp8.hip) without a GPU --
the entry points are declared and exported, the ctypes descriptor mirrors the header, the transposed MX rule agrees with hand-computed cases,
and the new kernels compile for gfx950 without spills or scratch."""
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sfron_cast_mx8_t", "sfron_fp8_wgrad_supported", "sfron_fp8_wgrad", "sfron_dit_fp8_wgrad_workspace_bytes", "sfron_aux_set_fp8_wgrad"]


def mx_ref(x):
    """the rule of include/sfron.h per 32-block of a row: X = ceil(log2(amax / 448)) clamped to [-127, 127], all-zero -> -127; byte = X + 127;
    code = e4m3fn_RNE(x * 2^-X).  (codes, scale bytes)"""
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
    assert "sfron_fp8_wgrad_desc" in txt


def test_wgrad_desc_mirror_matches_the_header(tmp_path):
    import ctypes
    from sfron import _lib
    fs = ["A", "a_scales", "B", "b_scales", "N", "K", "M", "c_f32", "ldc", "sumsq_mask", "sumsq_partials"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "sfron.h"\nint main(void) {\nprintf("%zu", sizeof(sfron_fp8_wgrad_desc));\n'
    src += "".join(f'printf(" %zu", offsetof(sfron_fp8_wgrad_desc, {f}));\n' for f in fs) + "return 0; }\n"
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    size, *offs = subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()
    assert ctypes.sizeof(_lib.Fp8WgradDesc) == int(size)
    for f, o in zip(fs, offs):
        assert getattr(_lib.Fp8WgradDesc, f).offset == int(o), f


def test_transposed_mx_rule_hand_cases():
    """mx_ref(x.T): the scale runs along the TOKENS (rows of x) -- one byte per 32 consecutive rows of a column.  This pins the restated
    rule the GPU tests compare the kernels with; it runs no code of the package"""
    x = torch.zeros(64, 3)
    x[0, 0] = 448.0           # column 0, tokens 0..31: X = 0, code 0x7E
    x[40, 0] = 1.0            # column 0, tokens 32..63: X = -8, 1 * 2^8 = 256 = 0x78
    x[5, 1] = 452.0           # column 1: X = 1, 226 -> 224 (nearest even) = 0x76
    x[6, 1] = 1.0             # ... its neighbour in the same 32-token block: 0.5 = 0x30
    x[33, 2] = -3.0e38        # column 2, second block: X = 120, -224 = 0xF6
    q, s = mx_ref(x.to(torch.bfloat16).T.contiguous())
    assert q.shape == (3, 64) and s.shape == (3, 2)
    assert s.tolist() == [[127, 119], [128, 0], [0, 127 + 120]]
    assert [q[0, 0].item(), q[0, 40].item(), q[1, 5].item(), q[1, 6].item(), q[2, 33].item()] == [0x7E, 0x78, 0x76, 0x30, 0xF6]
    # a row-wise cast of x would put tokens 0 and 40 of column 0 under different scales than the transposed one does
    assert int(q[0, 1]) == 0 and int(q[2, 0]) == 0


def test_wgrad_supported_shapes():
    from sfron import _lib
    L = _lib.lib()
    for N, K, M in ((3456, 1152, 8192), (1152, 1152, 8192), (4608, 1152, 8192), (1152, 4608, 8192),
                    (2304, 768, 2048), (768, 768, 2048), (3072, 768, 2048), (768, 3072, 2048)):
        assert L.sfron_fp8_wgrad_supported(N, K, M) == 1, (N, K, M)
    for N, K, M in ((384, 128, 256), (1152, 1152, 8160), (1152, 1152, 96), (0, 192, 128)):
        assert L.sfron_fp8_wgrad_supported(N, K, M) == 0, (N, K, M)


def test_wgrad_kernels_compile_without_spills_or_scratch():
    src = os.path.join(ROOT, "unified-unlearning-w-remain-geometry_amd", "csrc", "fp8.hip")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), src, ""], capture_output=True, text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"(.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+spill\s+(\d+)\s+occ\s+(\d+)\s+scratch\s+(\d+)", line)
        if m:
            rows[m.group(1).strip()] = (int(m.group(4)), int(m.group(6)))
    new = [k for k in rows if "k_wgrad8" in k or "k_mx8_cast_t" in k]
    assert len(new) == 2, rows.keys()
    for k in new:
        assert rows[k] == (0, 0), (k, rows[k])
