"""CPU-side checks of the C-ABI boundary: the library builds for gfx950, loads, and exports exactly the
symbols include/hpe.h declares (no compute calls -- there is no GPU in the build container)."""
import os
import re

import pytest

import hpe_amd
from hpe_amd import _lib, build as hbuild, resnet_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return _lib.load()


def _header_functions():
    txt = open(os.path.join(ROOT, "include", "hpe.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(hpe_[a-z0-9_]+)\s*\(", txt)))


def test_header_and_binding_agree(lib):
    hdr = _header_functions()
    assert hdr == _lib.declared_symbols(), (set(hdr) ^ set(_lib.declared_symbols()))
    for name in hdr:
        assert hasattr(lib, name), "library does not export %s" % name


def test_config_struct_matches_header(lib):
    """HpeConfig: the ctypes mirror has the header's fields in the header's order (all 4-byte scalars), and
    hpe_config_init fills the documented defaults with every plan option at -1 (= environment variable, else built-in)."""
    import ctypes as C

    txt = open(os.path.join(ROOT, "include", "hpe.h")).read()
    body = txt[txt.index("typedef struct HpeConfig {"):txt.index("} HpeConfig;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(?:int|float)\s+([a-z_0-9]+)\s*;", body)
    assert fields == [f[0] for f in _lib.HpeConfig._fields_]
    assert C.sizeof(_lib.HpeConfig) == 4 * len(fields)
    assert fields[0] == "struct_size" and tuple(fields[6:]) == _lib.PLAN_OPTIONS
    cfg = _lib.HpeConfig()
    lib.hpe_config_init(C.byref(cfg))
    assert cfg.struct_size == C.sizeof(_lib.HpeConfig)
    assert (cfg.device, cfg.max_batch, cfg.num_stage, cfg.encoder_dtype) == (0, 8, 3, 0) and abs(cfg.bn_eps - 1e-3) < 1e-9
    assert all(getattr(cfg, k) == -1 for k in _lib.PLAN_OPTIONS)


def test_debug_gemm_struct_matches_header(lib):
    """HpeDebugGemm (hpe_debug_gemm_ex): the ctypes mirror has the header's fields in the header's order and types, 22 ints then 8
    pointers with no padding between them; the call checks struct_size before it reads anything else and needs no GPU to refuse."""
    import ctypes as C

    txt = open(os.path.join(ROOT, "include", "hpe.h")).read()
    body = txt[txt.index("typedef struct HpeDebugGemm {") + len("typedef struct HpeDebugGemm {"):txt.index("} HpeDebugGemm;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"\s*(const float\*|float\*|int\*|int)\s+(.+)$", decl.strip(), flags=re.S)
        if m:
            fields += [(n.strip(), m.group(1)) for n in m.group(2).split(",")]
    assert [n for n, _ in fields] == [f[0] for f in _lib.HpeDebugGemm._fields_]
    for (n, ctype), (_, py) in zip(fields, _lib.HpeDebugGemm._fields_):
        assert (py is C.c_int) == (ctype == "int"), n
        assert C.sizeof(py) == (4 if ctype == "int" else 8), n
    n_int = sum(1 for _, t in fields if t == "int")
    assert fields[0][0] == "struct_size" and n_int % 2 == 0 and C.sizeof(_lib.HpeDebugGemm) == 4 * n_int + 8 * (len(fields) - n_int)
    for mode, name in ((_lib.GEMM_DENSE, "DENSE"), (_lib.GEMM_STRIDED, "STRIDED"), (_lib.GEMM_CONV3, "CONV3"), (_lib.GEMM_DUAL, "DUAL")):
        assert re.search(r"#define HPE_GEMM_%s %d\b" % (name, mode), txt)
    assert "hpe_debug_gemm_ex" in _lib.declared_symbols() and hasattr(lib, "hpe_debug_gemm_ex")
    sk = C.c_int(7)
    g = _lib.HpeDebugGemm(struct_size=C.sizeof(_lib.HpeDebugGemm), split_k=C.pointer(sk))
    assert lib.hpe_debug_gemm_ex(None, C.byref(g), None) == 3 and sk.value == 0  # HPE_ERR_STATE: no context; the output is still defined


def test_conv_route_struct_matches_header(lib):
    """HpeConvRoute (hpe_debug_conv_route): the ctypes mirror has the header's fields in the header's order, all 4-byte scalars; the kernel
    and pack numbering of the binding is the header's; the call checks struct_size first and needs neither a context nor a GPU."""
    import ctypes as C

    txt = open(os.path.join(ROOT, "include", "hpe.h")).read()
    body = txt[txt.index("typedef struct HpeConvRoute {") + len("typedef struct HpeConvRoute {"):txt.index("} HpeConvRoute;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"\s*(unsigned|int)\s+(.+)$", decl.strip(), flags=re.S)
        if m:
            fields += [(n.strip(), m.group(1)) for n in m.group(2).split(",")]
    assert [n for n, _ in fields] == [f[0] for f in _lib.HpeConvRoute._fields_]
    assert all((py is C.c_uint) == (t == "unsigned") for (_, t), (_, py) in zip(fields, _lib.HpeConvRoute._fields_))
    assert fields[0][0] == "struct_size" and C.sizeof(_lib.HpeConvRoute) == 4 * len(fields)
    enum = re.findall(r"\bHPE_CONV_K_([A-Z0-9_]+)\b", txt[txt.index("enum {\n    HPE_CONV_K_F32"):txt.index("typedef struct HpeConvRoute")])
    assert tuple(e.lower() for e in enum) == _lib.CONV_KERNELS + ("count",)
    assert "hpe_debug_conv_route" in _lib.declared_symbols() and hasattr(lib, "hpe_debug_conv_route")
    cfg = _lib.HpeConfig()
    lib.hpe_config_init(C.byref(cfg))
    r = _lib.HpeConvRoute()  # struct_size 0
    assert lib.hpe_debug_conv_route(C.byref(cfg), 1, 8, 0, 0, 1, C.byref(r)) == 1 and b"struct_size" in lib.hpe_last_error()
    r = _lib.conv_route(lib, cfg, 0, 8)
    assert _lib.CONV_KERNELS[r.kernel] == "f32" and r.mode == 3 and r.packs == 1 << _lib.ENCODER_PACKINGS.index("stem_w")


def test_create_refuses_foreign_config_struct(lib):
    """hpe_create checks HpeConfig.struct_size before it reads anything else: a zero-initialised struct (hpe_config_init not called: every
    plan option would read 0 = the slowest plan) and a struct of another header revision (shorter: the library would read plan options
    from past its end) are refused with HPE_ERR_INVALID and a message naming both sizes.  Runs without a GPU: the check comes first."""
    import ctypes as C

    h = C.c_void_p()
    zeroed = _lib.HpeConfig()  # ctypes zero-fills
    assert lib.hpe_create(C.byref(zeroed), C.byref(h)) == 1 and not h.value
    assert b"struct_size is 0" in lib.hpe_last_error()

    class OldConfig(C.Structure):  # the round-3 layout: no struct_size, 17 scalars
        _fields_ = [(n, t) for n, t in _lib.HpeConfig._fields_[1:-1]]

    old = OldConfig(device=0, max_batch=8, num_stage=3, bn_eps=1e-3, encoder_dtype=0, n_streams=-1)
    assert lib.hpe_create(C.cast(C.byref(old), C.POINTER(_lib.HpeConfig)), C.byref(h)) == 1 and not h.value
    short = _lib.HpeConfig()
    lib.hpe_config_init(C.byref(short))
    short.struct_size -= 4  # one field fewer: a stub built against the previous header
    assert lib.hpe_create(C.byref(short), C.byref(h)) == 1 and not h.value
    msg = lib.hpe_last_error().decode()
    assert str(C.sizeof(_lib.HpeConfig) - 4) in msg and str(C.sizeof(_lib.HpeConfig)) in msg, msg
    good = _lib.HpeConfig()
    lib.hpe_config_init(C.byref(good))
    rc = lib.hpe_create(C.byref(good), C.byref(h))
    assert rc in (0, 4), rc  # 4 = HPE_ERR_NO_DEVICE in the build container: the struct itself was accepted
    if rc == 0:
        lib.hpe_destroy(h)


def test_layer_table_matches_host_spec(lib):
    import ctypes as C

    geo = (C.c_int * 7)()
    for i, s in enumerate(resnet_spec.CONV_SPECS):
        assert lib.hpe_conv_layer_name(i).decode() == s.name
        assert lib.hpe_bn_layer_name(i).decode() == s.bn_name
        assert lib.hpe_conv_layer_geometry(i, geo) == 0
        assert tuple(geo) == (s.kh, s.kw, s.cin, s.cout, s.stride, s.hin, s.hout)
    assert lib.hpe_conv_layer_name(53) is None


def test_no_cpu_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(hpe_amd.HpeError):
        hpe_amd.HpeEngine()


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "human-pose-estimation_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), f
