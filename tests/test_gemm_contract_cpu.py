"""The host-side contract of the four implicit-GEMM launchers (csrc/gemm_contract.h) through hpe_debug_gemm_check: no GPU, no context,
nothing launched.  Every launch the GPU file makes is accepted; every clause of every kernel, broken once and alone, is refused under the
name tests/gemm_ref.py::contract_violations gives it; the tile table agrees with gemm_ref.TILES in the one place the contract reads it.
hpe_debug_gemm_launch, the launching twin, checks the contract of kernels 1..3 before it looks at its context: with no context at all it
refuses every error case under the clause's name and gets as far as "needs a finalized ctx" on every valid base."""
import ctypes as C

import pytest

import gemm_ref as R
from hpe_amd import _lib, build as hbuild

FIELDS = ("M", "N", "K", "lda", "ldw", "ldy", "ldres", "w_rows", "relu", "Hi", "Wi", "Cin", "Ho", "Wo", "stride", "k1_slabs", "y_slab8")
ADDRESS = dict(x=0x10000, x2=0x20000, wt=0x30000, residual=0x40000, y=0x50000)  # numbers, never dereferenced
OTHERS = ("f32s", "bf16", "bf16_p8")


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return _lib.load()


def check(lib, c, null=(), misaligned=(), kernel="f32"):
    """(return code, clause named in the message or None) of hpe_debug_gemm_check on case c"""
    g = _lib.HpeDebugGemm()
    g.struct_size = C.sizeof(_lib.HpeDebugGemm)
    g.mode, g.tile = c["mode"], c["tile"]
    for k in FIELDS:
        setattr(g, k, c.get(k, 0))
    has = dict(x=True, wt=True, y=True, residual=bool(c.get("use_res")), x2=c["mode"] == R.DUAL)
    for k, a in ADDRESS.items():
        setattr(g, k, a + (4 if k in misaligned else 0) if has[k] and k not in null else None)
    rc = lib.hpe_debug_gemm_check(C.byref(g), R.KERNELS[kernel]["id"], c.get("w_piece", 0))
    if rc == 0:
        return rc, None
    msg = lib.hpe_last_error().decode()
    assert "contract" in msg or "mode" in msg, msg
    return rc, msg.split('clause "')[1].split('"')[0] if 'clause "' in msg else "mode"


def test_every_gpu_case_is_accepted(lib):
    cases = R.all_valid_cases()
    assert len(cases) > 1300
    refused = [(c, name) for c in cases for rc, name in [check(lib, c)] if rc != 0]
    assert not refused, refused[:5]


@pytest.mark.parametrize("kernel", OTHERS)
def test_every_gpu_case_of_the_other_kernels_is_accepted(lib, kernel):
    """every launch of tests/test_gpu_bf16_gemm_edges.py is inside its kernel's contract, for the library and for the restatement"""
    cases = R.all_valid_cases(kernel)
    assert len(cases) >= 175
    refused = [(c, name) for c in cases for rc, name in [check(lib, c, kernel=kernel)] if rc != 0]
    assert not refused, refused[:5]
    assert not [c for c in cases if R.contract_violations(c, kernel=kernel)]
    for c in cases:
        assert c["ldy"] >= c["N"] and (not c["use_res"] or c["ldres"] >= c["N"]), c
        if c["mode"] != R.DENSE:
            assert c["M"] == R.BATCH * c["Ho"] * c["Wo"], c
    if kernel == "bf16":  # three channel slabs per tap: legal here, refused by the 256x256 kernel under its own clause
        c = next(c for c in cases if c["mode"] == R.CONV3 and c["Cin"] == 192)
        assert check(lib, dict(c, tile=7, w_rows=c["N"]), kernel="bf16_p8") == (1, "cin_slabs a power of two")


def launch_without_context(lib, c, null=(), misaligned=(), kernel="f32"):
    """(return code, split_k written, message) of hpe_debug_gemm_launch with a NULL context on case c: fake addresses, nothing can launch"""
    g = _lib.HpeDebugGemm()
    g.struct_size = C.sizeof(_lib.HpeDebugGemm)
    g.mode, g.tile = c["mode"], c["tile"]
    for k in FIELDS:
        setattr(g, k, c.get(k, 0))
    has = dict(x=True, wt=True, y=True, residual=bool(c.get("use_res")), x2=c["mode"] == R.DUAL)
    for k, a in ADDRESS.items():
        setattr(g, k, a + (4 if k in misaligned else 0) if has[k] and k not in null else None)
    g.scale, g.shift = 0x60000, 0x70000
    sk = C.c_int(-1)
    g.split_k = C.pointer(sk)
    rc = lib.hpe_debug_gemm_launch(None, C.byref(g), R.KERNELS[kernel]["id"], c.get("w_piece", 0), None)
    return rc, sk.value, lib.hpe_last_error().decode()


@pytest.mark.parametrize("kernel", OTHERS)
def test_launch_hook_refuses_before_it_needs_a_context(lib, kernel):
    """hpe_debug_gemm_launch on every error case of the kernel, context NULL: HPE_ERR_INVALID, the clause named, split_k = 0.  The valid
    bases pass the contract and stop at the missing context (HPE_ERR_STATE), also with split_k = 0: the order of the checks."""
    k = R.KERNELS[kernel]
    for name, base in R.error_bases(kernel).items():
        if base["mode"] in k["modes"]:
            rc, sk, msg = launch_without_context(lib, base, kernel=kernel)
            assert (rc, sk) == (3, 0) and "finalized" in msg, (name, rc, sk, msg)
    cases = R.error_cases(kernel)
    assert len(cases) > 40
    for i in range(len(cases)):
        c, null, mis = R.error_case(i, kernel)
        want = R.contract_violations(c, null, mis, kernel=kernel)
        rc, sk, msg = launch_without_context(lib, c, null, mis, kernel)
        assert len(want) == 1 and (rc, sk) == (1, 0), (i, cases[i], rc, sk, msg)
        if want[0] == "mode" and c["mode"] == R.STEM:
            assert "mode must be dense" in msg, msg  # the hooks' own guard: the stem is not theirs to launch
        else:
            assert "hpe_debug_gemm_launch" in msg and 'clause "%s"' % want[0] in msg and "nothing was launched" in msg, (i, cases[i], msg)


def test_launch_hook_guards(lib):
    g = _lib.HpeDebugGemm()
    sk = C.c_int(7)
    g.split_k = C.pointer(sk)
    assert lib.hpe_debug_gemm_launch(None, C.byref(g), 2, 0, None) == 1 and b"struct_size" in lib.hpe_last_error() and sk.value == 0
    assert lib.hpe_debug_gemm_launch(None, None, 2, 0, None) == 1
    g.struct_size = C.sizeof(_lib.HpeDebugGemm)
    for kernel in (-1, 4):
        assert lib.hpe_debug_gemm_launch(None, C.byref(g), kernel, 0, None) == 1 and b"kernel" in lib.hpe_last_error()
    sk.value = 7  # kernel 0 is hpe_debug_gemm_ex, which asks for its context first
    assert lib.hpe_debug_gemm_launch(None, C.byref(g), 0, 0, None) == 3 and sk.value == 0
    base = dict(R.error_bases("bf16")["dense"], N=1032, w_rows=1152, ldy=1040, use_res=0)  # scale / shift NULL: the context's, N <= 1024 only
    for k in FIELDS:
        setattr(g, k, base.get(k, 0))
    g.mode, g.tile, g.x, g.wt, g.y = base["mode"], base["tile"], ADDRESS["x"], ADDRESS["wt"], ADDRESS["y"]
    assert lib.hpe_debug_gemm_launch(None, C.byref(g), 2, 0, None) == 1 and b"1024" in lib.hpe_last_error()


def test_fp32_error_cases_name_their_clause(lib):
    for i in range(len(R.ERROR_CASES)):
        c, null, mis = R.error_case(i)
        want = R.contract_violations(c, null, mis)
        assert len(want) == 1 and check(lib, c, null, mis) == (1, want[0]), (i, R.ERROR_CASES[i], want, check(lib, c, null, mis))


@pytest.mark.parametrize("kernel", OTHERS)
def test_other_kernels_clause_by_clause(lib, kernel):
    k = R.KERNELS[kernel]
    for name, base in R.error_bases(kernel).items():
        if base["mode"] in k["modes"]:
            assert R.contract_violations(base, kernel=kernel) == [] and check(lib, base, kernel=kernel) == (0, None), (name, base)
    cases = R.error_cases(kernel)
    seen = set()
    for i in range(len(cases)):
        c, null, mis = R.error_case(i, kernel)
        want = R.contract_violations(c, null, mis, kernel=kernel)
        assert len(want) == 1 and check(lib, c, null, mis, kernel) == (1, want[0]), (i, cases[i], want, check(lib, c, null, mis, kernel))
        seen.add((c["mode"], want[0]))
    # the clauses every launcher has since this contract is one: the divisors of the host and of make_row
    for base, mode in (("strided", R.STRIDED), ("dual", R.DUAL)):
        assert (mode, "Ho, Wo, stride >= 1") in seen and all((base, {f: 0}, (), ()) in cases for f in ("Ho", "Wo", "stride"))
    if R.CONV3 in k["modes"]:
        assert (R.CONV3, "Hi, Wi >= 1") in seen and ("conv3", dict(Hi=0, Ho=0), (), ()) in cases and ("conv3", dict(Wi=0, Wo=0), (), ()) in cases
    else:
        assert ("conv3", {}, (), ()) in cases and (R.CONV3, "mode") in seen  # a mode the kernel lacks
    assert (R.STEM, "mode") in seen  # the stem mode is not the hooks' to ask for


@pytest.mark.parametrize("kernel", sorted(R.KERNELS))
def test_kernel_specific_clauses_stay_kernel_specific(lib, kernel):
    """what breaks a clause that only one launcher has is accepted by the launchers that lack it, by the library and by the restatement:
    three channel slabs per tap (the 256x256 kernel wants a power of two), y_slab8 with N % 8 != 0 (fp32-output kernels only), w_rows
    short of the padded N (the 256x256 kernel clamps instead), ldw below K + 2 * w_piece (f32s only)"""
    k, b = R.KERNELS[kernel], R.error_bases(kernel)
    S = k["slab"]
    probes = [("cin_slabs a power of two", "bf16_p8", dict(b["conv3"], Cin=3 * S, K=27 * S, ldw=27 * S)),
              ("y_slab8 needs N % 8 == 0", ("f32", "f32s"), dict(b["dense"], y_slab8=1, N=60)),
              ("w_rows covers the padded N", ("f32", "f32s", "bf16"), dict(b["dense"], w_rows=b["dense"]["w_rows"] - 4)),
              ("ldw >= K + 2 * w_piece", "f32s", dict(b["dense"], ldw=b["dense"]["K"], w_piece=b["dense"]["K"]))]
    for name, owners, c in probes:
        if c["mode"] not in k["modes"]:
            continue
        want = [name] if kernel in ((owners,) if isinstance(owners, str) else owners) else []
        assert R.contract_violations(c, kernel=kernel) == want, (name, c)
        assert check(lib, c, kernel=kernel) == ((1, name) if want else (0, None)), (name, c)


@pytest.mark.parametrize("kernel", sorted(R.KERNELS))
def test_tile_widths_agree_with_the_python_table(lib, kernel):
    """N = 4: the weights must cover exactly one tile width BN -- accepted at w_rows = BN, refused one tile short and (where the launcher
    has the coverage clause: the 256x256 kernel clamps its weight rows instead, so nothing pins its BN here) four rows short.  Only BN
    is read by the contract; BM and the wave grid of every tile rest on the device-code comparison (the kernel template arguments)."""
    k = R.KERNELS[kernel]
    base = R.error_bases(kernel)["dense"]
    for tile, (BM, BN) in k["tiles"].items():
        c = dict(base, tile=tile, N=4, w_rows=R.pad_to(4, BN))
        assert check(lib, c, kernel=kernel) == (0, None), (tile, c)
        short = "w_rows >= 1" if kernel == "bf16_p8" else "w_rows covers the padded N"
        assert check(lib, dict(c, w_rows=c["w_rows"] - BN), kernel=kernel) == (1, short), tile
        if kernel != "bf16_p8":
            assert check(lib, dict(c, w_rows=BN - 4), kernel=kernel) == (1, short), tile
    assert check(lib, dict(base, tile=max(k["tiles"]) + 1), kernel=kernel) == (1, R.TILE_CLAUSE[kernel])


def test_guards_of_the_hook(lib):
    g = _lib.HpeDebugGemm()
    assert lib.hpe_debug_gemm_check(C.byref(g), 0, 0) == 1 and b"struct_size" in lib.hpe_last_error()
    assert lib.hpe_debug_gemm_check(None, 0, 0) == 1
    g.struct_size = C.sizeof(_lib.HpeDebugGemm)
    assert lib.hpe_debug_gemm_check(C.byref(g), 4, 0) == 1 and b"kernel" in lib.hpe_last_error()
