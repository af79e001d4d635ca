"""CPU: the C-ABI library loads and exports every symbol include/sfron.h declares (no compute)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from sfron import _lib
    return _lib


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "sfron.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(sfron_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol(built):
    syms = header_symbols()
    assert len(syms) >= 10
    h = built.lib()
    for s in syms:
        assert hasattr(h, s), f"{s} declared in include/sfron.h but not exported by libsfron.so"
    assert sorted(built.declared_symbols()) == syms, "ctypes prototypes and include/sfron.h disagree"
    assert h.sfron_abi_version() == built.ABI_VERSION          # _lib.lib() refuses a library of another version
    assert h.sfron_build_arch() == b"gfx950"


def test_code_object_is_gfx950(built):
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", built.LIB_PATH], capture_output=True, text=True)
    # the fat binary embeds the device code object; its target id must be gfx950
    blob = open(built.LIB_PATH, "rb").read()
    assert b"gfx950" in blob


def test_ops_refuse_cpu_tensors(built):
    import torch
    from sfron import sweep
    with pytest.raises(built.SfronError):
        sweep.mask_from_fisher(torch.zeros(4), torch.zeros(4), 1.0)


def test_descriptor_structs_match_the_header(built):
    """ctypes mirrors of the header's structs: compile a one-line C program against include/sfron.h that prints sizeof and, for EVERY field
    of the mirror, offsetof and the field's size, and compare (a silent mismatch would hand the library garbage descriptors).  The field
    list is the mirror's own _fields_: a Python field the C struct does not have fails to compile."""
    import ctypes
    import tempfile
    mirrors = [("sfron_gemm_desc", built.GemmDesc), ("sfron_fp8_gemm_desc", built.Fp8GemmDesc), ("sfron_fp8_dgrad_desc", built.Fp8DgradDesc),
               ("sfron_fp8_wgrad_desc", built.Fp8WgradDesc), ("sfron_bgemm_desc", built.BGemmDesc), ("sfron_reduce_item", built.ReduceItem),
               ("sfron_wgrad_scatter_item", built.WgradScatterItem), ("sfron_conv_desc", built.ConvDesc), ("sfron_split_src", built.SplitSrc),
               ("sfron_dit_cfg", built.DitCfg), ("sfron_dit_fp8_operands", built.DitFp8Operands), ("sfron_dit_fwd", built.DitFwd),
               ("sfron_dit_bwd", built.DitBwd), ("sfron_wprep_item", built.WprepItem)]
    defined = {c for c in vars(built).values() if isinstance(c, type) and issubclass(c, ctypes.Structure) and c.__module__ == built.__name__}
    assert {c for _, c in mirrors} == defined, "a ctypes.Structure of _lib.py is missing from this table (or the table names a stranger)"
    assert dict(built.DitFp8Operands._fields_)["act_scales"] is ctypes.c_float * 3
    fields = {cname: (cls, [f for f, _ in cls._fields_]) for cname, cls in mirrors}
    lines = []
    for cname, (_, fs) in fields.items():
        lines.append(f'printf("{cname} %zu", sizeof({cname}));')
        for f in fs:
            lines.append(f'printf(" %zu:%zu", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));')
        lines.append('printf("\\n");')
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "sfron.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    assert len(out) == len(mirrors)
    for line in out:
        name, size, *offs = line.split()
        cls, fs = fields[name]
        assert ctypes.sizeof(cls) == int(size), (name, ctypes.sizeof(cls), size)
        assert len(offs) == len(fs)
        for f, o in zip(fs, offs):
            got = (getattr(cls, f).offset, getattr(cls, f).size)
            assert got == tuple(int(v) for v in o.split(":")), (name, f, got, o)


CFG_ENTRY = dict(batch=4, in_channels=4, input_size=16, patch=2, hidden=128, depth=2, heads=2, mlp_hidden=512, num_classes=10, freq_dim=256,
                 out_channels=8)          # the shape of tests/test_gpu_dit_entry.py


def test_dit_pass_argument_checks_come_before_any_gpu_call(built):
    """sfron_dit_forward / sfron_dit_backward refuse a bad descriptor with SFRON_ERR_ARG before their first HIP call: this runs without a GPU,
    with dummy non-NULL addresses that nothing may dereference."""
    import ctypes
    L = built.lib()
    cfg = built.DitCfg(**CFG_ENTRY)
    X = 0x1000                                   # "set" pointer: never dereferenced by a call that is refused

    def fwd(**kw):
        d = built.DitFwd(ctypes.pointer(cfg), X, X, X, X, X, X, None, X)
        for k, v in kw.items():
            setattr(d, k, v)
        return L.sfron_dit_forward(ctypes.byref(d), None)

    def bwd(**kw):
        d = built.DitBwd(ctypes.pointer(cfg), X, X, X, X, X, None, X, **kw)
        return L.sfron_dit_backward(ctypes.byref(d), None)

    assert L.sfron_dit_forward(None, None) == built.ERR_ARG and L.sfron_dit_backward(None, None) == built.ERR_ARG
    assert fwd(cfg=None) == built.ERR_ARG and L.sfron_dit_backward(ctypes.byref(built.DitBwd()), None) == built.ERR_ARG
    assert fwd(params=None) == built.ERR_ARG
    for phase in (5, -1):
        assert fwd(phase=phase) == built.ERR_ARG
    scales = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    f8 = built.DitFp8Operands(X, X, scales, None, None)
    assert fwd(fp8=ctypes.pointer(f8)) == built.ERR_ARG                  # NULL workspace_e4m3
    f8 = built.DitFp8Operands(X, X, (ctypes.c_float * 3)(1.0, 0.0, 1.0), None, X)
    assert fwd(fp8=ctypes.pointer(f8)) == built.ERR_ARG                  # a scale that is not positive
    events = (ctypes.c_void_p * cfg.depth)()
    assert bwd(block_events=events) == built.ERR_ARG                     # block_events without aux
    assert bwd(ada_dmod_out=X) == built.ERR_ARG and bwd(ada_sc_out=X) == built.ERR_ARG
    assert bwd(aux=None, late_bias=X, ada_dmod_out=None, ada_sc_out=X) == built.ERR_ARG
    d = built.DitBwd(ctypes.pointer(cfg), X, X, X, None, X, None, X)       # NULL d_out
    assert L.sfron_dit_backward(ctypes.byref(d), None) == built.ERR_ARG


def test_integration_md_stub_prototypes_match_the_header(built, monkeypatch):
    """INTEGRATION.md section 3's ctypes stub (the text a maintainer of the reference would paste): it must load the library, and every
    prototype it declares must have the header's parameter count with pointers where the header has pointers (the round-4 text had six
    pointers where include/sfron.h has seven: moments landed in each other's slots, status 0).  Executed on the GPU by
    tests/test_gpu_sweep_loss.py::test_integration_md_ctypes_stub_runs_as_written."""
    import ctypes
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("## 3. Raw C ABI from Python"):text.index("## 4. Entry point")]
    blocks = re.findall(r"```python\n(.*?)```", sec, flags=re.S)
    assert len(blocks) == 1
    monkeypatch.chdir(ROOT)
    ns = {}
    exec(compile(blocks[0], "INTEGRATION.md#3", "exec"), ns)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfron.h")).read(), flags=re.S)
    checked = 0
    for name in ("sfron_sumsq_masked", "sfron_clip_coef", "sfron_masked_clip_adam"):
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        fn = getattr(ns["L"], name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), (name, len(fn.argtypes or []), len(params))
        for at, p in zip(fn.argtypes, params):
            is_ptr_c = "*" in p
            is_ptr_py = at is ctypes.c_void_p or isinstance(at, type(ctypes.POINTER(ctypes.c_int)))
            assert is_ptr_c == is_ptr_py, (name, p, at)
            if not is_ptr_c:
                want = {"int64_t": ctypes.c_int64, "double": ctypes.c_double, "float": ctypes.c_float, "int": ctypes.c_int}[p.split()[0]]
                assert at is want, (name, p, at)
        checked += 1
    assert checked == 3 and callable(ns["fused_stage"])
